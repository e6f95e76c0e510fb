#!/usr/bin/env python
"""Cost of the pass head of the dual net (profiles/pass_head.md).

  python scripts/pass_head_bench.py kernels [--out DIR]   the training head (gpool_fwd + policy_head_soft_pass +
                                                         gpool_bwd_add_masked) against policy_head_soft at B = 2176 and
                                                         256; the inference head (gpool_fwd + policy_value_pass_head)
                                                         against policy_value_head at buckets 1 and 1024
  python scripts/pass_head_bench.py steps   [--out DIR]   trainer step time, 21 x 192 residual net, B = 256 and 2176,
                                                         with and without the head, interleaved round by round

Times come from device events around windows of back-to-back eager launches that end in a synchronise, so a
kernel row includes its launch overhead; the variants of one comparison alternate inside one process; every line
is also written as JSON."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

S, L, F = 19, 21, 192
NP = S * S


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _compare(out, what, size, jobs, n, rounds=5):
    """Warm up every job, then time them round by round, alternating; one record per job."""
    for fn in jobs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in jobs}
    for _ in range(rounds):
        for k, fn in jobs.items():
            us[k].append(_timed(fn, n) * 1e3)
    for k in jobs:
        rec = dict(what=what, size=size, name=k, calls_per_window=n, us_all=[round(v, 2) for v in us[k]],
                   median_us=round(sorted(us[k])[rounds // 2], 2))
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")


def kernels(out):
    from alphago_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(F, generator=g) * 0.05).to(dev)
    b = torch.zeros(1, device=dev)
    pw = (torch.randn(2, F, generator=g) * 0.01).to(dev)
    pb = torch.zeros(1, device=dev)
    for B in (2176, 256, 1024, 1):
        y = ops.padded_empty(B, S, 1, F, dev)
        y[:, 1:S + 1, 1:S + 1] = torch.randn(B, S, S, F, generator=g).clamp_min(0).to(dev).bfloat16()
        P = torch.zeros(B, 2, F, device=dev)
        a = torch.zeros(B, F, dtype=torch.int32, device=dev)
        if B in (2176, 256):  # the training head
            dz = torch.zeros_like(y)
            td = torch.rand(B, NP + 1, generator=g).to(dev)
            loss, corr, dpass = (torch.zeros(B, device=dev) for _ in range(3))
            dhead = torch.zeros(B, F + 1, device=dev)
            dpw = torch.zeros(B, 2 * F + 1, device=dev)

            def soft():
                ops.policy_head_train_soft(y, w, b, td, dz, loss, corr, dhead, S, 1.0 / B)

            def pool():
                ops.gpool_fwd(y, P, a, S)

            def head():
                ops.policy_head_soft_pass(y, w, b, P, pw, pb, td, dz, loss, corr, dhead, dpass, dpw, S, 1.0 / B)

            def back():
                ops.gpool_bwd_add_masked(dpass, pw, a, y, dz, S)

            def all3():
                pool()
                head()
                back()

            _compare(out, "train_head", B, dict(policy_head_soft=soft, gpool_fwd=pool, policy_head_soft_pass=head,
                                                gpool_bwd_add_masked=back, pass_head_total=all3),
                     400 if B == 2176 else 2000)  # windows of 20 ms and more
        if B in (1024, 1):  # the inference head
            probs = torch.zeros(B, NP, device=dev)
            probs1 = torch.zeros(B, NP + 1, device=dev)
            zv = torch.zeros(B, NP, device=dev)
            legal = (torch.rand(B, NP, generator=g) < 0.6).to(torch.uint8).to(dev)

            def pv():
                ops.policy_value_head(y, w, b, w, b, probs, zv, S, legal=legal)

            def pool_i():
                ops.gpool_fwd(y, P, a, S)

            def pvp():
                ops.policy_value_pass_head(y, w, b, w, b, P, pw, pb, probs1, zv, S, legal=legal)

            def both():
                pool_i()
                pvp()

            _compare(out, "infer_head", B, dict(policy_value_head=pv, gpool_fwd=pool_i, policy_value_pass_head=pvp,
                                                pass_head_total=both), 2000)  # windows of 16 ms and more
        del y
        torch.cuda.empty_cache()


def _net(pass_head):
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(0)
    net = he_uniform_(PolicyValueNet(49, S, F, L, residual=1, pass_head=pass_head), generator=g)
    nb = (L - 1) // 2
    with torch.no_grad():  # live block ends, as in tests/test_gpool_engines.py, and a live pass head
        for l in range(2, L, 2):
            net.trunk.weights[l].uniform_(-1, 1, generator=g).mul_((6.0 / (F * 9)) ** 0.5 * nb ** -0.5)
        if pass_head:
            net.pass_w.uniform_(-1, 1, generator=g).mul_((3.0 / (2 * F)) ** 0.5)
    return net


def steps(out):
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = torch.device("cuda:0")
    for B, n in ((256, 40), (2176, 10)):
        g = torch.Generator().manual_seed(B)
        planes = torch.randint(0, 2, (B, 49, S, S), dtype=torch.uint8, generator=g).to(dev)
        pi = torch.rand(B, NP + 1, generator=g) ** 8  # soft targets: the head the pass head replaces is the soft one
        pi = (pi / pi.sum(1, keepdim=True)).to(dev)
        moves = torch.randint(-1, NP, (B,), dtype=torch.int32, generator=g).to(dev)
        z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
        sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
        trs = {k: HipPolicyValueTrainer(_net(k), B, lr=1e-4, device=dev) for k in (0, 1)}
        jobs = {"pass_head=%d soft" % k: (lambda tr=tr: tr.step(planes, (pi, z), sym)) for k, tr in trs.items()}
        # hard moves: the plain head without the pass head, one-hot rows through the new head with it
        jobs.update({"pass_head=%d hard" % k: (lambda tr=tr: tr.step(planes, (moves, z), sym)) for k, tr in trs.items()})
        _compare(out, "step", B, jobs, n)
        del trs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernels", "steps"))
    ap.add_argument("--out", default="bench_out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pass_head_bench.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "pass_head_%s.jsonl" % a.what), "a") as f:
        {"kernels": lambda: kernels(f), "steps": lambda: steps(f)}[a.what]()
