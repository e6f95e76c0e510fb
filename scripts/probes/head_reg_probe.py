"""Policy-head kernel time with the regularised variants on: plain, stats only, stats + entropy
bonus, stats + entropy bonus + KL anchor, at the SL batch (2176) and the RL chunk (256).  Same
timing as head_batch_probe.py (best of 5 rounds of 20 back-to-back launches); prints one JSON line
per configuration and a markdown table."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from alphago_amd import ops  # noqa: E402

ops.load()
dev = torch.device("cuda")
S, C = 19, 192
rows = []
for B in (2176, 256):
    y = ops.padded_empty(B, S, 1, C, dev)
    y[:, 1:20, 1:20].normal_()
    y.clamp_min_(0)
    w = torch.randn(C, device=dev) * 0.05
    b = torch.zeros(1, device=dev)
    tgt = torch.randint(0, 361, (B,), device=dev, dtype=torch.int32)
    wt = torch.randn(B, device=dev)
    dz = torch.zeros_like(y)
    loss = torch.zeros(B, device=dev)
    corr = torch.zeros(B, device=dev)
    dhead = torch.zeros(B, C + 1, device=dev)
    q = torch.softmax(torch.randn(B, S * S, device=dev), 1).contiguous()
    st = torch.zeros(B, 3, device=dev)
    configs = [("plain", {}), ("stats", dict(stats=st)), ("stats + beta", dict(stats=st, ent_coef=0.01)),
               ("stats + beta + kappa", dict(stats=st, ref_probs=q, ent_coef=0.01, kl_coef=0.1))]
    for name, kw in configs:
        fn = lambda: ops.policy_head_train(y, w, b, tgt, dz, loss, corr, dhead, S, 1.0 / B, weight=wt, **kw)  # noqa: E731
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20 * 1e3)
        rows.append((B, name, round(best, 1)))
        print(json.dumps({"B": B, "config": name, "us": round(best, 1), "ns_per_board": round(best * 1e3 / B, 1)}),
              flush=True)
print("| B | configuration | us per launch | vs plain |")
print("|---|---|---|---|")
plain = {B: us for B, name, us in rows if name == "plain"}
for B, name, us in rows:
    print("| %d | %s | %.1f | %+.1f |" % (B, name, us, us - plain[B]))
