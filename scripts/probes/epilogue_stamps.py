"""Epilogue cycle stamps of the compact-halo 384 tile (tile 388), kernel-lab library.

The lab op's stamp buffer selects conv_fwd_halo384_kernel<.., STAMP>: per wave, s_memtime counts from
the K loop's last barrier to (0) the epilogue operands settled, (1) the last store issued, (2) every
store acknowledged (vmcnt 0), and (3) the wave's whole time.  One 3x3 192 -> 192 layer at B boards,
forward (bias + ReLU + bits) and bitmask dgrad; prints the median and the quartiles over all waves of
the launch, and the per-workgroup maximum (the wave that frees the CU) as a median over workgroups.

Usage: python scripts/probes/epilogue_stamps.py [B] [repeats]
"""
import json
import sys

import torch
from alphago_amd import ops

ops.load()
L = ops.lab()
dev = torch.device("cuda")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 2176
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
S, F = 19, 192
M = B * S * S
torch.manual_seed(0)
x = ops.padded_empty(B, S, 1, F, dev)
x[:, 1:20, 1:20].normal_()
w = torch.randn(F, F, 3, 3, device=dev) * 0.05
wf, wd = ops.packed_weight_like(w, F, F), ops.packed_weight_like(w, F, F, True)
ops.pack_weights([w], [wf], [wd])
bias = torch.randn(F, device=dev) * 0.1
y = ops.padded_empty(B, S, 1, F, dev)
dx = ops.padded_empty(B, S, 1, F, dev)
mb = torch.zeros((B * (S + 2) ** 2 * ops.mbits_words(F),), dtype=torch.int32, device=dev)
ops.conv_fwd(x, wf, bias, y, 3, S, 1, 1, mbits=mb)
nwg = (M + 383) // 384
NAMES = ("settled", "last_store_issued", "stores_acknowledged", "wave_total")


def run(kind):
    st = torch.zeros(nwg * 8 * 4, dtype=torch.int64, device=dev)
    for _ in range(reps):  # the last launch's stamps are read (the earlier ones warm the caches)
        if kind == "fwd":
            L.conv_fwd(x, wf, bias, None, y, 3, S, 1, 1, 0, mb, 388, st)
        else:
            L.conv_fwd(y, wd, None, None, dx, 3, S, 1, 1, ops.MODE_MASKBITS, mb, 388, st)
    torch.cuda.synchronize()
    t = st.view(nwg, 8, 4).double().cpu()
    out = {"kernel": kind + ":388", "B": B, "workgroups": nwg}
    for k, name in enumerate(NAMES):
        v = t[:, :, k].flatten()
        q = torch.quantile(v, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64))
        out[name] = {"q25": q[0].item(), "median": q[1].item(), "q75": q[2].item(),
                     "wg_max_median": t[:, :, k].max(dim=1).values.median().item()}
    out["epilogue_share_of_wave"] = round(out["stores_acknowledged"]["median"] / out["wave_total"]["median"], 4)
    print(json.dumps(out), flush=True)


run("fwd")
run("dgrad")
