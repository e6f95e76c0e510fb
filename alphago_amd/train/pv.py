"""Dual (policy + value) network training on MCTS self-play records.

``python -m alphago_amd train-pv model.json selfplay.h5 out/`` reads ``states``, ``pi`` and
``outcomes`` (and ``moves`` for ``--targets played``) straight from a ``selfplay-mcts`` file -- no
conversion step -- and trains a ``CNNPolicyValue`` model (``init-model pv``) on both targets in one
step: cross-entropy of the policy head against the search's visit distribution (``--targets pi``,
the soft-target head, rows at their full S*S + 1 width) or against the played move
(``--targets played``), plus ``--value-coef`` times the squared error of the value head against the
game outcome for the player to move.  A position whose visit mass is all on the pass has no policy
loss and still trains the value head -- unless the model has the pass head (``init-model pv --pass-head``):
then the policy softmax has S*S + 1 entries, the pass column is a target like any other and a played pass
(move -1) is the one-hot row of the pass.

A model with the ownership head (``init-model pv --ownership``) also reads ``ownership`` and
``ownership_valid`` (``selfplay-mcts --ownership``) and adds ``--ownership-coef`` times the mean squared
error of the ownership head against the final territory map, over the positions of scored games.

A model with the score head (``init-model pv --score-head``) also reads ``score`` and ``score_valid``
(``selfplay-mcts --score``) and adds ``--score-coef`` times the Huber loss (threshold S points) of the head
against the final margin in units of S points, over the positions of scored games.  The score does not move
with the board.

D4 augmentation goes through the input pack's ``sym``: the soft head moves the distribution with the
board, the ownership head moves its target the same way, and the outcome is invariant.  The output
directory holds ``metadata.json`` (per-epoch ``loss``, ``acc``, ``value_loss``, ``value_acc`` and their
``val_`` forms; with the ownership head also ``own_loss`` and ``own_acc``, means over the positions with
a valid ownership row; with the score head also ``score_loss`` and ``score_mae``, the latter in points, means
over the positions with a valid score), ``shuffle.npz`` and ``weights.{epoch:05d}.hdf5`` per epoch, as ``train-sl``
writes them.

Out of scope here: checkpoint / exact resume (``--weights`` restarts from a weights file with a fresh
schedule), the watchdog, streaming datasets (the file is held in host memory) and graph mode.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, Optional

import numpy as np
import torch

from ..io.h5lite import H5File
from ..models.policy import CNNPolicyValue
from ..parallel import dist as agdist
from ..utils.metrics import MetricsLogger
from .engine import make_policy_value_trainer, pass_target_rows
from .sl import MetadataWriter

_KEYS = ("loss", "acc", "value_loss", "value_acc")
_OWN_KEYS = ("own_loss", "own_acc")
_SCORE_KEYS = ("score_loss", "score_mae")


class _PVParser(argparse.ArgumentParser):
    """train-pv's parser: flag combinations that cannot run are parse errors."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if getattr(ns, "fp8_backward", False) and ns.precision != "fp8":
            self.error("--fp8-backward requires --precision fp8")
        return ns, rest


def _parser():
    p = _PVParser(
        prog="alphago_amd train-pv",
        description="Train a dual policy+value network on selfplay-mcts records (states, pi, outcomes).  "
                    "Checkpoint/resume and the watchdog are out of scope: --weights restarts from a weights "
                    "file with a fresh learning-rate schedule.")
    p.add_argument("model", help="dual-net JSON model file (CNNPolicyValue.save_model / init-model pv)")
    p.add_argument("train_data", help="selfplay.h5 written by selfplay-mcts")
    p.add_argument("out_directory")
    p.add_argument("--minibatch", "-B", type=int, default=16)
    p.add_argument("--epochs", "-E", type=int, default=10)
    p.add_argument("--learning-rate", "-r", type=float, default=.03)
    p.add_argument("--decay", "-d", type=float, default=.0001)
    p.add_argument("--value-coef", type=float, default=1.0, help="weight of the value MSE next to the policy CE")
    p.add_argument("--ownership-coef", type=float, default=1.0,
                   help="weight of the ownership MSE (models with the ownership head); 1.0 is a conventional "
                        "starting point, not a tuned value")
    p.add_argument("--score-coef", type=float, default=1.0,
                   help="weight of the score head's Huber loss (models with the score head); 1.0 is a conventional "
                        "starting point, not a tuned value")
    p.add_argument("--targets", default="pi", choices=["pi", "played"],
                   help="pi: the search's visit distribution (soft-target head, default); played: the move played")
    p.add_argument("--no-symmetries", action="store_true", help="disable random D4 augmentation")
    p.add_argument("--train-val-test", nargs=3, type=float, default=[0.93, .05, .02])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp8"],
                   help="HIP backend conv forward precision (fp8: e4m3 block-scaled MFMA forward, bf16 backward "
                        "unless --fp8-backward; a residual trunk needs 192 filters for it)")
    p.add_argument("--fp8-backward", action="store_true",
                   help="with --precision fp8: all-fp8 trunk backward (e5m2 x e4m3 wgrad and dgrad on the 3x3 "
                        "layers above the first; 192-wide trunks)")
    p.add_argument("--metrics", default=None, help="JSONL metrics file (per-epoch records)")
    p.add_argument("--weights", default=None, help="weights file (in out_directory) to start from")
    p.add_argument("--verbose", "-v", default=False, action="store_true")
    return p


def _pad(t: torch.Tensor, B: int, fill) -> torch.Tensor:
    if t.shape[0] == B:
        return t
    return torch.cat([t, torch.full((B - t.shape[0],) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)])


def trainer_kwargs(args, ownership: bool, score: bool = False) -> dict:
    """The keyword arguments make_policy_value_trainer gets for the parsed command line."""
    kw = {"value_coef": args.value_coef}
    if ownership:
        kw["own_coef"] = args.ownership_coef
    if score:
        kw["score_coef"] = args.score_coef
    if args.precision != "bf16":
        kw["precision"] = args.precision
    if args.fp8_backward:
        kw.update(fp8_wgrad=True, fp8_dgrad=True)
    return kw


def run_training(cmd_line_args: Optional[List[str]] = None):
    args = _parser().parse_args(list(sys.argv[1:] if cmd_line_args is None else cmd_line_args))
    env = agdist.init_from_env()
    dev, world, rank = env.device, env.world_size, env.rank
    model = CNNPolicyValue.load_model(args.model, device=dev)
    net = model.model
    if args.weights:
        model.load_weights(os.path.join(args.out_directory, args.weights))
    S = net.board
    with H5File(args.train_data) as f:
        states = np.asarray(f["states"].read())
        pi = np.asarray(f["pi"].read(), dtype=np.float32)
        z = np.asarray(f["outcomes"].read()).astype(np.float32)
        moves = np.asarray(f["moves"].read()).astype(np.int32) if args.targets == "played" else None
        own = own_valid = None
        if getattr(net, "ownership", False):
            if "ownership" not in f or "ownership_valid" not in f:
                raise ValueError("%s has no 'ownership' / 'ownership_valid' datasets, which a model with the "
                                 "ownership head trains on: write the records with selfplay-mcts --ownership"
                                 % args.train_data)
            own = np.asarray(f["ownership"].read()).astype(np.int8)
            own_valid = np.asarray(f["ownership_valid"].read()).astype(np.float32)
        score = score_valid = None
        if getattr(net, "score_head", False):
            if "score" not in f or "score_valid" not in f:
                raise ValueError("%s has no 'score' / 'score_valid' datasets, which a model with the score head "
                                 "trains on: write the records with selfplay-mcts --score" % args.train_data)
            score = np.asarray(f["score"].read()).astype(np.float32)
            score_valid = np.asarray(f["score_valid"].read()).astype(np.float32)
    n_total = states.shape[0]
    if states.shape[1] != model.preprocessor.output_dim or states.shape[2] != S:
        raise ValueError("dataset rows are %s, the model expects (%d, %d, %d)"
                         % (states.shape[1:], model.preprocessor.output_dim, S, S))
    if pi.shape != (n_total, S * S + 1) or z.shape != (n_total,):
        raise ValueError("pi / outcomes do not match states: %s, %s for %d positions" % (pi.shape, z.shape, n_total))
    if own is not None and (own.shape != (n_total, S * S) or own_valid.shape != (n_total,)):
        raise ValueError("ownership / ownership_valid do not match states: %s, %s for %d positions"
                         % (own.shape, own_valid.shape, n_total))
    if score is not None and (score.shape != (n_total,) or score_valid.shape != (n_total,)):
        raise ValueError("score / score_valid do not match states: %s, %s for %d positions"
                         % (score.shape, score_valid.shape, n_total))
    perm = np.random.default_rng(args.seed).permutation(n_total)
    n_train = int(args.train_val_test[0] * n_total)
    n_val = int(args.train_val_test[1] * n_total)
    my_train = perm[:n_train][rank::world]
    my_val = perm[n_train:n_train + n_val][rank::world]
    if len(my_train) == 0:
        raise ValueError("no training positions (%d in the file)" % n_total)
    if env.is_main:
        os.makedirs(args.out_directory, exist_ok=True)
        with open(os.path.join(args.out_directory, "shuffle.npz"), "wb") as f:
            np.save(f, perm)
    agdist.barrier()
    meta = MetadataWriter(os.path.join(args.out_directory, "metadata.json"))
    meta.metadata.update(training_data=args.train_data, model_file=args.model, targets=args.targets,
                         value_coef=args.value_coef)
    if own is not None:
        meta.metadata.update(ownership_coef=args.ownership_coef)
    if score is not None:
        meta.metadata.update(score_coef=args.score_coef)

    B = args.minibatch
    kw = trainer_kwargs(args, own is not None, score is not None)
    trainer = make_policy_value_trainer(net, B, args.learning_rate, args.decay, backend=args.backend, device=dev, **kw)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed * 1000 + rank)
    order_rng = np.random.default_rng(args.seed * 7919 + rank)
    log = MetricsLogger(args.metrics if env.is_main else None)

    def batch(idx):
        """(planes, (policy target, outcomes)) of the rows idx, padded to B with no-loss rows (an
        all-zero distribution / move -1; their outcome 0 is counted out by the caller)."""
        idx = np.sort(idx)
        planes = _pad(torch.from_numpy(states[idx]).to(dev), B, 0)
        zt = _pad(torch.from_numpy(z[idx]).to(dev), B, 0.0)
        if moves is None:
            tgt = _pad(torch.from_numpy(pi[idx]).to(dev), B, 0.0)
        elif getattr(net, "pass_head", False):  # -1 is a played pass here: one-hot rows, padded with no-loss rows
            tgt = _pad(pass_target_rows(torch.from_numpy(moves[idx]).to(dev), S * S), B, 0.0)
        else:
            tgt = _pad(torch.from_numpy(moves[idx]).to(dev), B, -1)
        ownt = None
        if own is not None:  # padding rows are invalid: no ownership term
            ot = _pad(torch.from_numpy(own[idx]).to(dev), B, 0)
            ov = _pad(torch.from_numpy(own_valid[idx]).to(dev), B, 0.0)
            ownt = (ot, ov)
        if score is not None:  # the fourth slot; padding rows are invalid here too
            sct = _pad(torch.from_numpy(score[idx]).to(dev), B, 0.0)
            scv = _pad(torch.from_numpy(score_valid[idx]).to(dev), B, 0.0)
            return planes, (tgt, zt, ownt, (sct, scv))
        if ownt is not None:
            return planes, (tgt, zt, ownt)
        return planes, (tgt, zt)

    steps = max(1, len(my_train) // B)
    for epoch in range(args.epochs):
        t0 = time.perf_counter()
        order = order_rng.permutation(my_train)
        no = 6 if own is not None else 4  # the score head's two sums follow the ownership head's
        nm = no + (2 if score is not None else 0)
        # the metric sums, then the valid ownership rows and the valid score rows
        sums = torch.zeros(nm + 2, device=dev, dtype=torch.float64)
        for s in range(steps):
            idx = order[s * B:(s + 1) * B]
            if len(idx) < B:  # fewer positions than one minibatch: wrap around
                idx = np.resize(order, B)
            planes, tgt = batch(idx)
            sym = None if args.no_symmetries else torch.randint(0, 8, (B,), device=dev, dtype=torch.int32,
                                                                 generator=gen)
            sums[:nm] += torch.stack([m.double() for m in trainer.step(planes, tgt, sym)])
            if own is not None:
                sums[nm] += tgt[2][1].double().sum()
            if score is not None:
                sums[nm + 1] += tgt[3][1].double().sum()
        agdist.all_reduce_sum_(sums)
        seen = steps * B * world
        logs = {k: float(v) / seen for k, v in zip(_KEYS, sums)}
        if own is not None:
            logs.update({k: float(v) / max(1.0, float(sums[nm])) for k, v in zip(_OWN_KEYS, sums[4:6])})
        if score is not None:
            logs.update({k: float(v) / max(1.0, float(sums[nm + 1])) for k, v in zip(_SCORE_KEYS, sums[no:no + 2])})
        if n_val > 0:
            vs = torch.zeros(5, device=dev, dtype=torch.float64)
            vo = torch.zeros(3, device=dev, dtype=torch.float64)
            vsc = torch.zeros(3, device=dev, dtype=torch.float64)
            for i in range(0, len(my_val), B):
                idx = my_val[i:i + B]
                planes, tgt = batch(idx)
                m = torch.stack([x.double() for x in trainer.evaluate(planes, tgt)])
                pad = B - len(idx)  # padding rows: outcome 0 against v, no policy loss
                if pad:
                    pv = trainer.predict(planes)[len(idx):].double()
                    m[2] -= (pv ** 2).sum()
                    m[3] -= (torch.sign(pv) == 0).double().sum()
                vs[:4] += m[:4]
                vs[4] += len(idx)
                if own is not None:
                    vo[:2] += m[4:6]
                    vo[2] += tgt[2][1].double().sum()
                if score is not None:
                    vsc[:2] += m[no:no + 2]
                    vsc[2] += tgt[3][1].double().sum()
            agdist.all_reduce_sum_(vs)
            n = max(1.0, float(vs[4]))
            logs.update({"val_" + k: float(v) / n for k, v in zip(_KEYS, vs[:4])})
            if own is not None:
                agdist.all_reduce_sum_(vo)
                logs.update({"val_" + k: float(v) / max(1.0, float(vo[2])) for k, v in zip(_OWN_KEYS, vo[:2])})
            if score is not None:
                agdist.all_reduce_sum_(vsc)
                logs.update({"val_" + k: float(v) / max(1.0, float(vsc[2])) for k, v in zip(_SCORE_KEYS, vsc[:2])})
        dt = time.perf_counter() - t0
        if env.is_main:
            ep = meta.on_epoch_end(logs)
            model.save_weights(os.path.join(args.out_directory, "weights.%05d.hdf5" % ep))
            log.log(epoch=ep, positions_per_s=seen / dt, **logs)
            if args.verbose:
                print("epoch %d: %s (%.0f pos/s)" % (ep, logs, seen / dt), flush=True)
        agdist.barrier()
    return meta.metadata


if __name__ == "__main__":
    run_training()
