"""A/B of the dual net's training step with a plain and a residual trunk of the same depth and width.

    python scripts/residual_step_ab.py [--batch 2176] [--layers 13] [--filters 192] [--rounds 4] [--steps 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/residual_step_ab.py --trace

Both nets live in one process and take turns (plain, residual, plain, ...) on the same resident batch, so
the two arms see the same box, clocks and neighbours.  Each window is ``--steps`` full steps
(pack_input, forward, both heads, backward, fused update) between two device events; the result is one
JSON line with every window and the medians.  ``--trace``: a few steps of the residual net only, for a
kernel trace -- its odd layers run the plain epilogues (kernel template mode 0 forward, 3 dgrad) and its
even layers >= 2 the skip-operand ones (mode 4 forward, the dgrad of odd layers mode 7), so one trace holds
both sides of the per-layer comparison."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2176)
    ap.add_argument("--layers", type=int, default=13)
    ap.add_argument("--filters", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = torch.device("cuda:0")
    B, S = a.batch, 19
    g = torch.Generator().manual_seed(0)
    planes = torch.randint(0, 2, (B, 49, S, S), dtype=torch.uint8, generator=g).to(dev)
    moves = torch.randint(0, S * S, (B,), dtype=torch.int32, generator=g).to(dev)
    z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
    arms = {}
    for name, res in (("plain", 0), ("residual", 1)):
        if a.trace and not res:
            continue
        net = he_uniform_(PolicyValueNet(49, S, a.filters, a.layers, residual=res),
                          generator=torch.Generator().manual_seed(1))
        arms[name] = HipPolicyValueTrainer(net, B, lr=0.003, device=dev)

    def window(tr, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            tr.step(planes, (moves, z), sym)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for tr in arms.values():
        window(tr, a.warmup)
    if a.trace:
        window(arms["residual"], 3)
        return
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, tr in arms.items():
            ms[k].append(window(tr, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"batch": B, "layers": a.layers, "filters": a.filters, "steps_per_window": a.steps,
                      "ms_per_step": ms, "median_ms": med,
                      "positions_per_s": {k: B / (v * 1e-3) for k, v in med.items()},
                      "residual_over_plain": med["residual"] / med["plain"]}))


if __name__ == "__main__":
    main()
