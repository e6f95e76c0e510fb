#!/usr/bin/env python
"""Cost of the global pooling branch (profiles/gpool.md).

  python scripts/gpool_bench.py steps   [--out DIR]   trainer step time, 21 x 192 residual net, B = 256 and 2176,
                                                     gpool off / 3 / 1, the variants interleaved round by round
  python scripts/gpool_bench.py infer   [--out DIR]   engine evaluation time at buckets 1, 16 and 1024, off / 1
  python scripts/gpool_bench.py kernels [--batch B]   the four new launches and a device copy of the same tensor,
                                                     a few times each: run it under rocprofv3 --kernel-trace --stats

Times come from device events around windows that end in a synchronise; every line is also written as JSON."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

S, L, F = 19, 21, 192


def _net(gpool):
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(0)
    net = he_uniform_(PolicyValueNet(49, S, F, L, residual=1, gpool=gpool), generator=g)
    nb = (L - 1) // 2
    with torch.no_grad():  # live block ends and gates, as in tests/test_gpool_engines.py
        for l in range(2, L, 2):
            net.trunk.weights[l].uniform_(-1, 1, generator=g).mul_((6.0 / (F * 9)) ** 0.5 * nb ** -0.5)
        for w in getattr(net.trunk, "gpool_w", ()):
            w.uniform_(-1, 1, generator=g).mul_((3.0 / (2 * F)) ** 0.5 * nb ** -0.5)
    return net


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def steps(out):
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = torch.device("cuda:0")
    for B, n, rounds in ((256, 40, 5), (2176, 10, 5)):
        g = torch.Generator().manual_seed(B)
        planes = torch.randint(0, 2, (B, 49, S, S), dtype=torch.uint8, generator=g).to(dev)
        moves = torch.randint(0, S * S, (B,), dtype=torch.int32, generator=g).to(dev)
        z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
        sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
        trs = {k: HipPolicyValueTrainer(_net(k), B, lr=1e-4, device=dev) for k in (0, 3, 1)}
        for tr in trs.values():  # warm-up: code objects, kernel attributes
            for _ in range(3):
                tr.step(planes, (moves, z), sym)
        torch.cuda.synchronize()
        ms = {k: [] for k in trs}
        for _ in range(rounds):
            for k, tr in trs.items():
                ms[k].append(_timed(lambda: tr.step(planes, (moves, z), sym), n))
        for k in trs:
            rec = dict(what="step", batch=B, gpool=k, branches=len(trs[k].gpool_blocks), steps_per_window=n,
                       ms_per_step=[round(v, 4) for v in ms[k]], median_ms=round(sorted(ms[k])[rounds // 2], 4))
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
        del trs
        torch.cuda.empty_cache()


def infer(out):
    import numpy as np

    from alphago_amd.models.inference import HipPolicyValueInference

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    for bucket, n, rounds in ((1, 200, 5), (16, 200, 5), (1024, 20, 5)):
        x = torch.from_numpy((rng.random((bucket, 49, S, S)) < 0.4).astype(np.uint8)).to(dev)
        engs = {k: HipPolicyValueInference(_net(k).to(dev), dev, buckets=(bucket,)) for k in (0, 1)}
        for e in engs.values():
            for _ in range(3):
                e.evaluate(x)
        torch.cuda.synchronize()
        ms = {k: [] for k in engs}
        for _ in range(rounds):
            for k, e in engs.items():
                ms[k].append(_timed(lambda: e.evaluate(x), n))
        for k in engs:
            rec = dict(what="evaluate", bucket=bucket, gpool=k, calls_per_window=n,
                       ms_per_call=[round(v, 4) for v in ms[k]], median_ms=round(sorted(ms[k])[rounds // 2], 4))
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
        del engs
        torch.cuda.empty_cache()


def kernels(B, out):
    from alphago_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    y = ops.padded_empty(B, S, 1, F, dev)
    y[:, 1:S + 1, 1:S + 1] = torch.randn(B, S, S, F, generator=g).abs().to(dev).bfloat16()
    o = torch.zeros_like(y)
    P = torch.zeros(B, 2, F, device=dev)
    a = torch.zeros(B, F, dtype=torch.int32, device=dev)
    s = torch.zeros(B, F, device=dev)
    w = (torch.randn(2 * F, F, generator=g) * 0.05).to(dev)
    gate = torch.zeros(B, F, device=dev)
    jobs = dict(gpool_fwd_full=lambda: ops.gpool_fwd(y, P, a, S), gpool_fwd_sum=lambda: ops.gpool_fwd(y, s, None, S),
                gpool_bias_add=lambda: ops.gpool_bias_add(y, gate, o, S), gpool_bwd_fill=lambda: ops.gpool_bwd_fill(P, a, o, S),
                gate_dense=lambda: ops.dense_f32(P.view(B, -1), w, gate), device_copy=lambda: o.copy_(y))
    for name, fn in jobs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = sorted(_timed(fn, 20) for _ in range(5))
        rec = dict(what="kernel", name=name, batch=B, tensor_mb=round(y.numel() * 2 / 1e6, 1), us=round(ms[2] * 1e3, 2),
                   us_all=[round(v * 1e3, 2) for v in ms])
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("steps", "infer", "kernels"))
    ap.add_argument("--out", default="bench_out")
    ap.add_argument("--batch", type=int, default=2176)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpool_bench.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "gpool_%s.jsonl" % a.what), "a") as f:
        {"steps": lambda: steps(f), "infer": lambda: infer(f), "kernels": lambda: kernels(a.batch, f)}[a.what]()
