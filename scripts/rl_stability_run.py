"""One measured ``train-rl`` run with the policy diagnostics logged, and a match of its FINAL
(unselected) weights against the SL start (the measurement of profiles/r7/README.md).

The SL net comes from ``scripts/r6/evidence.py sl`` (NETS/sl.{json,hdf5}); the recipe is the README's:
lr 0.01, 512 games per iteration, clip 5, weight decay 1e-4, evaluation every 5 iterations, opponent pool
with a snapshot every 10.  Extra arguments after ``--`` go to train-rl, e.g.
``-- --max-kl 0.01 --entropy-coef 0.01``.

Usage: python scripts/rl_stability_run.py NETS OUT TAG [--iterations N] [--match-games N] [-- train-rl flags]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def wilson(k, n, z=1.96):
    p = k / n
    d = 1 + z * z / n
    c = (p + z * z / (2 * n)) / d
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / d
    return (round(c - h, 4), round(c + h, 4))


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("nets")
    ap.add_argument("out")
    ap.add_argument("tag")
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--match-games", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    from alphago_amd.models.policy import CNNPolicy
    from alphago_amd.search.arena import batched_match
    from alphago_amd.search.selfplay import BatchedSampler
    from alphago_amd.train.rl import run

    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    os.makedirs(a.out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="rl_stability_")
    metrics = os.path.join(a.out, "rl_%s.jsonl" % a.tag)
    if os.path.exists(metrics):
        os.remove(metrics)
    sl_j, sl_w = os.path.join(a.nets, "sl.json"), os.path.join(a.nets, "sl.hdf5")
    t0 = time.perf_counter()
    res = run([sl_w, sl_j, "--model_folder", os.path.join(work, "pool"), "--learning_rate", "0.01", "--save_every", "10",
               "--game_batch_size", str(a.games), "--iterations", str(a.iterations), "--minibatch", "256",
               "--metrics", metrics, "--checkpoint-dir", os.path.join(work, "ck"), "--checkpoint-every",
               str(a.iterations), "--seed", str(a.seed), "--clip-grad-norm", "5", "--weight-decay", "1e-4",
               "--eval-every", "5", "--eval-games", "200", "--log-policy-stats"] + extra)
    secs = time.perf_counter() - t0
    final = res["pool"][-1]  # the last snapshot: iterations is a multiple of save_every
    assert final is not None and final.endswith("weights.%05d.hdf5" % a.iterations), final
    sl = CNNPolicy.load_model(sl_j, device=dev, weights_file=sl_w)
    rl = CNNPolicy.load_model(sl_j, device=dev, weights_file=final)
    m = batched_match(BatchedSampler(rl, 1.0, seed=a.seed * 2 + 1), BatchedSampler(sl, 1.0, seed=a.seed * 2 + 2),
                      a.match_games, seed=a.seed)
    h = res["history"]
    out = {"tag": a.tag, "train_rl_flags": extra, "iterations": a.iterations, "seconds": round(secs, 1),
           "eval_curve": [(r["iteration"] + 1, round(r["eval_win_rate"], 3)) for r in h if "eval_win_rate" in r],
           "best": {k: res["best"][k] for k in ("eval_win_rate", "iteration")},
           "skipped_updates": int(sum(1 for r in h if r.get("skipped"))),
           "final_vs_sl": {"games": a.match_games, "wins": m["player1_wins"], "draws": m["draws"],
                           "win_rate": round(m["player1_win_rate"], 4),
                           "ci95": wilson(m["player1_wins"], a.match_games)}}
    with open(os.path.join(a.out, "summary_%s.json" % a.tag), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
