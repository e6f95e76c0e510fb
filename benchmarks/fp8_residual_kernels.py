"""Kernel cost of the fp8 skip operand: each of the four RES kernels of the 192-wide tile against its no-skip
twin on one 192 -> 192 3x3 layer, at the training batch (2176) and the inference batch (1024).

  fwd_both    forward, bf16 + e4m3 outputs, bitmask, amax     (a block end below the top)
  fwd_bf16    forward, bf16 output only                       (the top layer)
  dgrad_both  bitmask dgrad, bf16 + e5m2 outputs              (a block's first layer)
  dgrad_bf16  bitmask dgrad, bf16 output only                 (the dgrad into the stem)

The two arms of a pair alternate inside the process; every figure is the median of ``--repeats`` windows of
``--iters`` launches between device synchronisations, with min and max.  The skip adds one bf16 read of the
output's size; ``skip_bytes`` is that size and ``skip_us_at_layer_bw`` what it costs at the bandwidth the
no-skip launch itself reaches over its own traffic (operand, weights and outputs, each once).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphago_amd import ops  # noqa: E402

S, C, K = 19, 192, 3


def spread(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2)}


def bench(B, iters, repeats, dev):
    g = torch.Generator().manual_seed(B)
    shape = (B, S + 2, S + 2, C)

    def act(dtype):  # zero-bordered random bytes of moderate magnitude
        t = torch.zeros(shape, dtype=torch.float32)
        t[:, 1:-1, 1:-1] = torch.randn(B, S, S, C, generator=g).clamp_min(0)
        return t.to(dtype).view(torch.uint8).to(dev)

    x8, dz8 = act(torch.float8_e4m3fn), act(torch.float8_e5m2)
    w = torch.randn(C, C, K, K, generator=g) * 0.05
    w8, w8t = [torch.zeros(ops.fp8_weight_shape(K, C, C), dtype=torch.uint8, device=dev) for _ in range(2)]
    ops.pack_weights_fp8_multi([w.to(dev), w.to(dev)], [w8, w8t], torch.ones(1, device=dev), [0, 0], [0, 1])
    bias = torch.zeros(C, device=dev)
    sc = torch.tensor([127, 127], dtype=torch.int32, device=dev)
    osc = torch.ones(1, device=dev)
    yb = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
    y8 = torch.zeros(shape, dtype=torch.uint8, device=dev)
    res = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
    res[:, 1:-1, 1:-1] = torch.randn(B, S, S, C, generator=g).to(torch.bfloat16).to(dev)
    mb = torch.zeros(B * (S + 2) ** 2 * ops.mbits_words(C), dtype=torch.int32, device=dev)
    mb_in = torch.randint(-2 ** 31, 2 ** 31 - 1, mb.shape, dtype=torch.int64, generator=g).to(torch.int32).to(dev)
    amax = ops.fp8_amax_buffer(1, dev)[0]

    def fwd(both, r):
        return lambda: ops.conv_fwd_fp8(x8, w8, bias, sc, osc, K, S, 1, 1, y_bf16=yb, y_fp8=y8 if both else None,
                                        amax=amax, mbits=mb if both else None, res=r)

    def dgrad(both, r):
        return lambda: ops.conv_dgrad_fp8_bits(dz8, w8t, mb_in, sc, osc, K, S, y_bf16=yb, y_fp8=y8 if both else None,
                                               amax=None if both else amax, res=r)

    pairs = {"fwd_both": (fwd, True), "fwd_bf16": (fwd, False), "dgrad_both": (dgrad, True),
             "dgrad_bf16": (dgrad, False)}
    px = B * (S + 2) ** 2 * C
    out = {"B": B, "skip_bytes": 2 * px}
    for name, (mk, both) in pairs.items():
        arms = {"plain": mk(both, None), "res": mk(both, res)}
        t = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / iters * 1e6)
        traffic = px + w8.numel() + 2 * px + (px if both else 0)  # operand, weights, bf16 (and byte) outputs
        plain = float(np.median(t["plain"]))
        bw = traffic / (plain * 1e-6)
        out[name] = {"plain_us": spread(t["plain"]), "res_us": spread(t["res"]),
                     "extra_us": round(float(np.median(t["res"])) - plain, 2),
                     "plain_traffic_bytes": traffic, "plain_bw_TBps": round(bw / 1e12, 3),
                     "skip_us_at_layer_bw": round(2 * px / bw * 1e6, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2176,1024")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8_residual_kernels measures on a GPU")
    ops.load()
    dev = torch.device("cuda")
    print(json.dumps({"layer": "192->192 3x3, S=19", "runs": [bench(int(b), a.iters, a.repeats, dev)
                                                              for b in a.batches.split(",")]}))


if __name__ == "__main__":
    main()
