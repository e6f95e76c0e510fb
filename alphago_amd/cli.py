"""Command-line entry point: ``python -m alphago_amd <command> ...``

Commands
  convert        SGF -> HDF5 training data          (reference game_converter CLI)
  init-model     write a new policy/value model JSON (+ random weights)
  train-sl       supervised policy training          (reference supervised_policy_trainer CLI)
  train-rl       RL policy training by self-play     (reference reinforcement_policy_trainer CLI)
  value-generate self-play positions for the value net
  selfplay-mcts  batched MCTS self-play games (SGF + states / pi / outcomes HDF5)
  selfplay-to-sl MCTS self-play records -> SL training data (most-visited or played move targets;
                 --target dist adds the visit distributions for train-sl --targets pi)
  train-value    value-network regression
  train-pv       dual policy+value net on selfplay-mcts records (pi and outcomes in one step)
  gtp            run a GTP v2 engine on stdin/stdout (reference interface/gtp_wrapper)
  match          play games between two players (policy / mcts / random / external GTP)
  bench          the headline SL throughput benchmark (bench.py)
  serve          HTTP/JSON policy/value/genmove service with dynamic batching

Player specs (gtp/match): ``random``, ``policy:MODEL.json[:greedy|:T]``,
``mcts:POLICY.json[,VALUE.json]:PLAYOUTS`` (a dual ``init-model pv`` file alone is both nets),
``gtp:COMMAND LINE``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import List, Optional


SYMMETRY_CHOICES = ("none", "random", "all")


def default_symmetries() -> str:
    """ALPHAGO_AMD_SYMMETRIES, the default of every --symmetries flag ("none" when unset)."""
    return os.environ.get("ALPHAGO_AMD_SYMMETRIES", "none")


def add_symmetries_arg(p: argparse.ArgumentParser) -> None:
    p.add_argument("--symmetries", choices=SYMMETRY_CHOICES, default=default_symmetries(),
                   help="evaluate every position under one random board symmetry, or average all 8 "
                        "(default: $ALPHAGO_AMD_SYMMETRIES or none)")


def add_score_utility_arg(p: argparse.ArgumentParser) -> None:
    p.add_argument("--score-utility", type=float, default=0.0, metavar="LAMBDA",
                   help="dual nets with the score head: search on (v + LAMBDA * tanh(score / (2 S))) / (1 + LAMBDA) "
                        "instead of the win/loss value v; root values and the resign threshold then speak of this "
                        "utility.  LAMBDA has no tuned value (default 0: the pure value)")


def make_player(spec: str, device=None, symmetries: str = "none", score_utility: float = 0.0):
    from .gtp.client import GTPClientPlayer
    from .models.policy import CNNPolicy, CNNPolicyValue, CNNValue, is_dual_spec
    from .search.arena import RandomPlayer
    from .search.players import GreedyPolicyPlayer, MCTSPlayer, ProbabilisticPolicyPlayer

    if spec == "random":
        return RandomPlayer()
    kind, _, rest = spec.partition(":")
    if kind == "gtp":
        return GTPClientPlayer(rest)
    if kind == "policy":
        path, _, opt = rest.partition(":")
        pol = CNNPolicy.load_model(path, device=device, symmetries=symmetries)
        if opt == "greedy":
            return GreedyPolicyPlayer(pol)
        return ProbabilisticPolicyPlayer(pol, temperature=float(opt) if opt else 1.0)
    if kind == "mcts":
        nets, _, n = rest.rpartition(":")
        if not nets:
            nets, n = n, "1600"
        paths = nets.split(",")
        if is_dual_spec(paths[0]):  # a dual (policy + value) net: the one file is the whole player
            if len(paths) > 1:
                raise ValueError("%s holds a dual policy+value net: no separate value net goes with it" % paths[0])
            pv = CNNPolicyValue.load_model(paths[0], device=device, symmetries=symmetries)
            if score_utility:
                pv.set_score_utility(score_utility)
            return MCTSPlayer(pv, None, n_playout=int(n))
        pol = CNNPolicy.load_model(paths[0], device=device, symmetries=symmetries)
        val = CNNValue.load_model(paths[1], device=device, symmetries=symmetries) if len(paths) > 1 else None
        return MCTSPlayer(pol, val, n_playout=int(n))
    raise ValueError("unknown player spec %r" % spec)


def _init_model(argv):
    from .features import DEFAULT_FEATURES, VALUE_FEATURES
    from .models.policy import CNNPolicy, CNNPolicyValue, CNNValue

    p = argparse.ArgumentParser(prog="alphago_amd init-model")
    p.add_argument("kind", choices=["policy", "value", "pv"],
                   help="pv: the dual policy+value net (one trunk, two heads; 192 filters by default)")
    p.add_argument("json_out")
    p.add_argument("--weights", default=None, help="also write random-init weights (Keras HDF5)")
    p.add_argument("--features", default=None, help="comma-separated feature list")
    p.add_argument("--board", type=int, default=19)
    p.add_argument("--filters", type=int, default=None)
    p.add_argument("--layers", type=int, default=12)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--residual", action="store_true",
                   help="pv only: a residual trunk (stem + two-layer blocks with a skip connection; --layers odd)")
    p.add_argument("--ownership", action="store_true",
                   help="pv only: a third 1x1 head predicting each point's owner at the end of the game "
                        "(trained by train-pv on selfplay-mcts --ownership records)")
    p.add_argument("--gpool", type=int, default=0, metavar="K",
                   help="pv --residual only: a global pooling branch (mean and max over the board -> dense -> "
                        "per-channel bias on the block's skip) in every K-th residual block")
    p.add_argument("--pass-head", action="store_true",
                   help="pv only: a learned pass logit next to the S*S move logits (mean and max of the trunk "
                        "output over the board -> dense), trained by train-pv on the pass column of "
                        "selfplay-mcts records and searched as a child of every node")
    p.add_argument("--score-head", action="store_true",
                   help="pv only: an estimate of the score lead of the player to move (mean and max of the trunk "
                        "output over the board -> dense -> ReLU -> dense), trained by train-pv on selfplay-mcts "
                        "--score records; GTP estimate_score and --score-utility read it")
    p.add_argument("--score-dense", type=int, default=64, metavar="D",
                   help="--score-head: width of the head's hidden layer, a multiple of 8 in 8..512 (default 64)")
    a = p.parse_args(argv)
    if a.score_head and a.kind != "pv":
        p.error("--score-head needs the dual net (init-model pv): the head reads its trunk")
    if a.pass_head and a.kind != "pv":
        p.error("--pass-head needs the dual net (init-model pv): the pass logit joins its policy softmax")
    if a.gpool and not (a.kind == "pv" and a.residual):
        p.error("--gpool needs a residual dual net (init-model pv --residual --gpool K)")
    if a.residual and a.kind != "pv":
        p.error("--residual needs the dual net (init-model pv): a Keras Sequential cannot express a skip connection")
    if a.ownership and a.kind != "pv":
        p.error("--ownership needs the dual net (init-model pv)")
    import torch

    torch.manual_seed(a.seed)
    if a.kind == "policy":
        feats = a.features.split(",") if a.features else DEFAULT_FEATURES
        m = CNNPolicy(feats, board=a.board, filters_per_layer=a.filters or 128, layers=a.layers, device="cpu")
    elif a.kind == "pv":
        feats = a.features.split(",") if a.features else VALUE_FEATURES
        kw = {"residual": 1} if a.residual else {}
        if a.ownership:
            kw["ownership"] = 1
        if a.gpool:
            kw["gpool"] = a.gpool
        if a.pass_head:
            kw["pass_head"] = 1
        if a.score_head:
            kw["score_head"] = 1
            if a.score_dense != 64:
                kw["score_dense"] = a.score_dense
        try:
            m = CNNPolicyValue(feats, board=a.board, filters_per_layer=a.filters or 192, layers=a.layers,
                               device="cpu", **kw)
        except ValueError as e:  # e.g. an even depth for a residual trunk
            p.error(str(e))
    else:
        feats = a.features.split(",") if a.features else VALUE_FEATURES
        m = CNNValue(feats, board=a.board, filters_per_layer=a.filters or 152, layers=a.layers, device="cpu")
    m.save_model(a.json_out, a.weights)
    print(a.json_out)


def gtp_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="alphago_amd gtp")
    p.add_argument("--player", default="random")
    p.add_argument("--size", type=int, default=19)
    add_symmetries_arg(p)
    add_score_utility_arg(p)
    return p


def _gtp(argv):
    a = gtp_parser().parse_args(argv)
    from .gtp.engine import run_gtp

    run_gtp(make_player(a.player, symmetries=a.symmetries, score_utility=a.score_utility), size=a.size)


def match_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="alphago_amd match")
    p.add_argument("player1")
    p.add_argument("player2")
    p.add_argument("--games", type=int, default=10)
    p.add_argument("--size", type=int, default=19)
    p.add_argument("--komi", type=float, default=7.5)
    p.add_argument("--sgf-dir", default=None)
    add_symmetries_arg(p)
    add_score_utility_arg(p)
    return p


def _match(argv):
    a = match_parser().parse_args(argv)
    from .search.arena import play_match

    res = play_match(make_player(a.player1, symmetries=a.symmetries, score_utility=a.score_utility),
                     make_player(a.player2, symmetries=a.symmetries, score_utility=a.score_utility),
                     a.games, a.size, a.komi, sgf_dir=a.sgf_dir)
    print(json.dumps(res))
    return res


from .parallel.launch import ExitCode as _Exit  # noqa: E402  (explicit process exit codes)


def main(argv: Optional[List[str]] = None) -> int:
    """Dispatch a command; returns a process exit code."""
    r = _dispatch(list(sys.argv[1:] if argv is None else argv))
    return int(r) if isinstance(r, _Exit) else 0


def _dispatch(argv: List[str]):
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return _Exit(0)
    cmd, rest = argv[0], argv[1:]
    if cmd == "convert":
        from .data.convert import run_game_converter
        return run_game_converter(rest)
    if cmd == "init-model":
        return _init_model(rest)
    if cmd == "serve":
        from .serve.server import serve_cli
        return _Exit(serve_cli(rest))
    if cmd == "train-sl":
        from .train.sl import run_training
        return run_training(rest)
    if cmd == "train-rl":
        from .train.rl import run
        return run(rest)
    if cmd == "value-generate":
        from .train.value import generate_cli
        return generate_cli(rest)
    if cmd == "selfplay-mcts":
        from .search.selfplay_mcts import selfplay_cli
        return selfplay_cli(rest)
    if cmd == "selfplay-to-sl":
        from .data.selfplay_to_sl import selfplay_to_sl_cli
        return selfplay_to_sl_cli(rest)
    if cmd == "train-value":
        from .train.value import train_cli
        return train_cli(rest)
    if cmd == "train-pv":
        from .train.pv import run_training as run_pv
        return run_pv(rest)
    if cmd == "gtp":
        return _gtp(rest)
    if cmd == "match":
        return _match(rest)
    if cmd == "bench":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, root)
        import bench
        sys.argv = ["bench.py"] + rest
        return _Exit(bench.main() or 0)
    print("unknown command %r\n%s" % (cmd, __doc__))
    return _Exit(2)


if __name__ == "__main__":
    sys.exit(main() or 0)
