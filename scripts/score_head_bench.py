#!/usr/bin/env python
"""Cost of the score head of the dual net (profiles/score_head.md).

  python scripts/score_head_bench.py kernels [--out DIR]  the training head's launches (gpool_fwd, dense_f32 x 3,
                                                          score_out, gpool_bwd_add_masked_dp, head_grad_sums x 2) at
                                                          B = 2176 and 256; the merged gpool_bwd_add_masked_dp against
                                                          gpool_bwd_add_masked followed by a score-only
                                                          gpool_bwd_add_masked_dp; the inference head (gpool_fwd,
                                                          dense_f32, score_out) at buckets 1 and 1024
  python scripts/score_head_bench.py steps   [--out DIR]  trainer step time, 21 x 192 residual net, B = 256 and 2176:
                                                          without the head, with it, and for a net with the pass head
                                                          too, interleaved round by round

The method is scripts/pass_head_bench.py's: device events around windows of back-to-back eager launches that end in
a synchronise, so a kernel row includes its launch overhead; the variants of one comparison alternate inside one
process; every line is also written as JSON."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

S, L, F, D = 19, 21, 192, 64
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
    w1 = (torch.randn(2 * F, D, generator=g) * 0.05).to(dev)
    b1 = torch.zeros(D, device=dev)
    w2 = (torch.randn(D, generator=g) * 0.1).to(dev)
    b2 = torch.zeros(1, device=dev)
    pw = (torch.randn(2, F, generator=g) * 0.01).to(dev)
    for B in (2176, 256, 1024, 1):
        y = ops.padded_empty(B, S, 1, F, dev)
        y[:, 1:S + 1, 1:S + 1] = torch.randn(B, S, S, F, generator=g).clamp_min(0).to(dev).bfloat16()
        P = torch.zeros(B, 2, F, device=dev)
        a = torch.zeros(B, F, dtype=torch.int32, device=dev)
        up = torch.zeros(B, D, device=dev)
        s = torch.zeros(B, device=dev)

        def pool():
            ops.gpool_fwd(y, P, a, S)

        def fwd_dense():
            ops.dense_f32(P.view(B, -1), w1, up, bias=b1)

        def out_fwd():
            ops.score_out(up, w2, b2, s)

        if B in (2176, 256):  # the training head
            dz = torch.zeros_like(y)
            t = torch.randn(B, generator=g).to(dev)
            valid = torch.ones(B, device=dev)
            loss, ae, dpass = (torch.zeros(B, device=dev) for _ in range(3))
            dpass.normal_()
            du = torch.zeros(B, D, device=dev)
            dout = torch.zeros(B, D + 1, device=dev)
            dw1 = torch.zeros(2 * F, D, device=dev)
            dP = torch.zeros(B, 2, F, device=dev)
            gb1 = torch.zeros(D, device=dev)
            g2 = torch.zeros(D + 1, device=dev)
            sums = torch.zeros(2, device=dev)

            def out_train():
                ops.score_out(up, w2, b2, s, target=t, valid=valid, loss=loss, abserr=ae, du=du, dout=dout,
                              grad_scale=1.0 / B)

            def dw():
                ops.dense_f32(P.view(B, -1), du, dw1, trans_a=True)

            def dp():
                ops.dense_f32(du, w1, dP.view(B, -1), trans_b=True)

            def back():
                ops.gpool_bwd_add_masked_dp(dP, a, y, dz, S)

            def back_merged():
                ops.gpool_bwd_add_masked_dp(dP, a, y, dz, S, dpass=dpass, pass_w=pw)

            def back_pass():
                ops.gpool_bwd_add_masked(dpass, pw, a, y, dz, S)

            def back_split():
                back_pass()
                back()

            def sums2():
                ops.head_grad_sums(du, loss, ae, gb1, sums)
                ops.head_grad_sums(dout, loss, ae, g2, sums)

            def total():
                pool(); fwd_dense(); out_train(); dw(); dp(); back(); sums2()

            def total_shared():  # a net with the pass head: gpool_fwd is the pass head's, the pass rides along
                fwd_dense(); out_train(); dw(); dp(); back_merged(); sums2()

            n = 400 if B == 2176 else 2000
            _compare(out, "train_head", B, dict(gpool_fwd=pool, dense_f32_upre=fwd_dense, score_out=out_train,
                                                dense_f32_dw1=dw, dense_f32_dP=dp, gpool_bwd_add_masked_dp=back,
                                                head_grad_sums_x2=sums2, score_head_total=total,
                                                score_head_total_beside_pass=total_shared), n)
            _compare(out, "merged_vs_split", B, dict(gpool_bwd_add_masked=back_pass, dp_score_only=back,
                                                     dp_merged=back_merged, split_two_launches=back_split), n)
        if B in (1024, 1):  # the inference head

            def total_i():
                pool(); fwd_dense(); out_fwd()

            _compare(out, "infer_head", B, dict(gpool_fwd=pool, dense_f32_upre=fwd_dense, score_out=out_fwd,
                                                score_head_total=total_i), 2000)
        del y
        torch.cuda.empty_cache()


def _net(score_head, pass_head):
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(0)
    net = he_uniform_(PolicyValueNet(49, S, F, L, residual=1, pass_head=pass_head, score_head=score_head),
                      generator=g)
    nb = (L - 1) // 2
    with torch.no_grad():  # live block ends, a live pass head and a live score head
        for l in range(2, L, 2):
            net.trunk.weights[l].uniform_(-1, 1, generator=g).mul_((6.0 / (F * 9)) ** 0.5 * nb ** -0.5)
        if pass_head:
            net.pass_w.uniform_(-1, 1, generator=g).mul_((3.0 / (2 * F)) ** 0.5)
        if score_head:
            net.sc2_w.uniform_(-1, 1, generator=g).mul_((3.0 / D) ** 0.5)
    return net


def steps(out):
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = torch.device("cuda:0")
    for B, n in ((256, 40), (2176, 10)):
        g = torch.Generator().manual_seed(B)
        planes = torch.randint(0, 2, (B, 49, S, S), dtype=torch.uint8, generator=g).to(dev)
        pi = torch.rand(B, NP + 1, generator=g) ** 8
        pi = (pi / pi.sum(1, keepdim=True)).to(dev)
        z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
        sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
        sc = ((torch.randn(B, generator=g) * 12).to(dev), torch.ones(B, device=dev))
        jobs = {}
        trs = []
        for ph in (0, 1):
            for sh in (0, 1):
                tr = HipPolicyValueTrainer(_net(sh, ph), B, lr=1e-4, device=dev)
                trs.append(tr)
                tgt = (pi, z, None, sc) if sh else (pi, z)
                jobs["pass_head=%d score_head=%d" % (ph, sh)] = (lambda tr=tr, tgt=tgt: tr.step(planes, tgt, sym))
        _compare(out, "step", B, jobs, n)
        del trs, jobs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernels", "steps"))
    ap.add_argument("--out", default="bench_out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_head_bench.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "score_head_%s.jsonl" % a.what), "a") as f:
        {"kernels": lambda: kernels(f), "steps": lambda: steps(f)}[a.what]()
