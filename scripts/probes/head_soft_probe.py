"""Soft-target policy head (policy_head_train_soft) against the plain training head
(policy_head_train) in one process on the same tensors: 19 x 19, 192 channels, per-board weights and
symmetries.  Same timing as head_reg_probe.py (rounds of 20 back-to-back launches between device
events), the two kernels alternating round by round; best and median of 7 rounds.  B = 2176 is the
SL batch and B = 256 the smallest batch of the 512-thread BoardRows kernel; B = 16 runs the
1024-thread BoardRegs kernel.  Prints one JSON line per row and a markdown table."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from alphago_amd import ops  # noqa: E402

ops.load()
dev = torch.device("cuda")
S, C = 19, 192
ROUNDS, LAUNCHES = 7, 20
rows = []
for B in (2176, 256, 16):
    y = ops.padded_empty(B, S, 1, C, dev)
    y[:, 1:20, 1:20].normal_()
    y.clamp_min_(0)
    w = torch.randn(C, device=dev) * 0.05
    b = torch.zeros(1, device=dev)
    tgt = torch.randint(0, 361, (B,), device=dev, dtype=torch.int32)
    sym = torch.randint(0, 8, (B,), device=dev, dtype=torch.int32)
    wt = torch.randn(B, device=dev)
    dz = torch.zeros_like(y)
    loss = torch.zeros(B, device=dev)
    corr = torch.zeros(B, device=dev)
    dhead = torch.zeros(B, C + 1, device=dev)
    pi = torch.softmax(torch.randn(B, S * S + 1, device=dev), 1).contiguous()  # with the pass column
    fns = {
        "plain": lambda: ops.policy_head_train(y, w, b, tgt, dz, loss, corr, dhead, S, 1.0 / B, weight=wt),
        "soft": lambda: ops.policy_head_train_soft(y, w, b, pi, dz, loss, corr, dhead, S, 1.0 / B, weight=wt,
                                                    sym=sym),
    }
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    for name, t in times.items():
        rows.append((B, name, min(t), statistics.median(t), max(t)))
        print(json.dumps({"B": B, "kernel": name, "us_best": round(min(t), 2), "us_median": round(statistics.median(t), 2),
                          "us_max": round(max(t), 2)}), flush=True)
print("| B | kernel | us best | us median | us max | best vs plain |")
print("|---|---|---|---|---|---|")
plain = {B: best for B, name, best, _, _ in rows if name == "plain"}
for B, name, best, med, worst in rows:
    print("| %d | %s | %.1f | %.1f | %.1f | %.3f |" % (B, name, best, med, worst, best / plain[B]))
