"""fp8 vs bf16 wgrad (+ reduce) of one 3x3 trunk layer, alternating, device-event timed.

    python scripts/probes/wgrad_fp8_bench.py [B [seconds [width [rounds]]]]

width 160: a value-net layer (152 filters padded to 160), default B = 1024; width 192: a policy-net layer.
With the kernel-lab library built and WGRAD_FP8_LAB=1, the rejected 192 tile (one 8-wave 192 x 192
workgroup per CU, lab probe 16) is timed in the same rotation as "fp8-alt"."""
import json
import os
import sys

import torch

from alphago_amd import ops

ops.load()
dev = torch.device("cuda")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
secs = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
Cp = int(sys.argv[3]) if len(sys.argv) > 3 else 160
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 2
if not ops.wgrad_fp8_supported(Cp, Cp, 3):
    sys.exit("width %d: the fp8 wgrad covers 160 and 192" % Cp)
C = 152 if Cp == 160 else Cp
S, K = 19, 3
M = B * S * S
x = ops.padded_empty(B, S, 1, Cp, dev)
x[:, 1:20, 1:20, :C].normal_()
dz = ops.padded_empty(B, S, 1, Cp, dev)
dz[:, 1:20, 1:20, :C].normal_()
x8 = torch.randint(0, 120, x.shape, dtype=torch.uint8, device=dev)
dz8 = torch.randint(0, 120, x.shape, dtype=torch.uint8, device=dev)
x8[:, 0] = 0
dz8[:, 0] = 0
gw = torch.zeros(C, C, 3, 3, device=dev)
gb = torch.zeros(C, device=dev)
xs = torch.tensor([127], dtype=torch.int32, device=dev)
gm = torch.ones(1, device=dev)
ns16 = ops.wgrad_nsplit(M, Cp, Cp, K)
ns8 = ops.wgrad_fp8_nsplit(M, K, width=Cp)
s16 = torch.empty(ns16, 9, Cp, Cp, device=dev)
d16 = torch.zeros(ns16, Cp, device=dev)
s8 = torch.empty(ns8, 9, Cp, Cp, device=dev)
d8 = torch.zeros(ns8, Cp, device=dev)


def bf16():
    ops.conv_wgrad(x, dz, s16, d16, K, S, 1, 1)
    ops.conv_wgrad_reduce(s16, d16, gw, gb, 1.0, 0.0)


def fp8():
    ops.conv_wgrad_fp8(x8, dz8, s8, d8, xs, xs, gm, K, S, 1, 1)
    ops.conv_wgrad_reduce(s8, d8, gw, gb, 1.0, 0.0)


def fp8_alt():
    ops.lab().conv_wgrad_fp8(x8, dz8, s8, d8, xs, xs, gm, K, S, 1, 1, None, 16)
    ops.conv_wgrad_reduce(s8, d8, gw, gb, 1.0, 0.0)


arms = [("bf16", bf16), ("fp8", fp8)]
if Cp == 192 and os.environ.get("WGRAD_FP8_LAB", "0") == "1":
    arms.append(("fp8-alt", fp8_alt))
flops = 2.0 * M * C * C * 9
for rnd in range(rounds):
    for name, fn in arms:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n, ms = 0, 0.0
        while ms < secs * 1e3:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            n += 10
        print(json.dumps({"wgrad": name, "width": Cp, "B": B, "round": rnd, "us": round(ms / n * 1e3, 1),
                          "pflops": round(n * flops / ms / 1e12, 3),
                          "nsplit": ns16 if name == "bf16" else ns8}), flush=True)
