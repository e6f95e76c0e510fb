#!/usr/bin/env python
"""One launch of every production conv tile, for a kernel trace.

The conv outputs are bit-identical across tiles by design, so only a trace can tell which kernel a tile
code launched.  This runs, once each at B = 2, S = 19: every production tile code x output width
{64, 128, 160, 192} x mode {bias + ReLU, mask dgrad, none, bitmask dgrad, bias + ReLU + skip, bitmask dgrad +
skip, bitmask dgrad + e5m2 copy} where the combination is legal; split-K; every tile the wgrad launcher
chooses (3x3, 1x1, thin 5x5 and 3x3 layers at 48 and 49 real planes, the small-batch plan); and the
split-free wgrad at ksub 1 / 2 / 4 / 8.  It prints the launch list in order, one line per launch.

    rocprofv3 --kernel-trace -d OUT -- python scripts/probes/tile_sweep.py

Run it on two builds and compare grid, workgroup size, LDS bytes and kernel per launch index
(scripts/isa_compare.py gives the kernels' digests by name).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from alphago_amd import ops  # noqa: E402

B, S = 2, 19
TILES = (36, 37, 64, 128, 256, 384, 385, 386, 387, 388)
BF = torch.bfloat16


def main():
    ops.load(build_if_missing=False)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = 0

    def say(what):
        nonlocal n
        print("%3d %s" % (n, what), flush=True)
        n += 1

    def act(C, P):
        t = torch.zeros(B, S + 2 * P, S + 2 * P, C, dtype=BF)
        t[:, P:P + S, P:P + S, :] = torch.randint(-2, 3, (B, S, S, C), generator=g).to(BF)
        return t.to(dev)

    for cout, cin, K in ((64, 64, 3), (128, 128, 3), (160, 160, 3), (160, 64, 5), (192, 192, 3), (192, 64, 5)):
        P = K // 2
        real = 48 if K == 5 else cin
        w = torch.randint(-2, 3, (cout, real, K, K), generator=g).float().to(dev)
        wf = torch.zeros_like(ops.packed_weight_like(w, cin, cout))
        ops.pack_weights([w], [wf], [torch.zeros_like(ops.packed_weight_like(w, cin, cout, transposed=True))])
        x, bias = act(cin, P), torch.zeros(cout, device=dev)
        y, res, mask = act(cout, 1), act(cout, 1), act(cout, 1)
        mb = torch.zeros(B * (S + 2) ** 2 * ops.mbits_words(cout), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for tile in TILES:
            if cout == 160 and tile == 37:
                continue
            for mode, skip in ((0, False), (1, False), (2, False), (3, False), (0, True), (3, True)):
                say("fwd %dx%d K%d tile %d mode %d%s" % (cout, cin, K, tile, mode, " + skip" if skip else ""))
                ops.conv_fwd(x, wf, bias, y, K, S, P, 1, mode=mode, mask=mask if mode == 1 else None,
                             mbits=mb if mode in (0, 3) else None, tile=tile, res=res if skip else None)
            # the e5m2 copy of the bitmask dgrad: not on the 32-pixel tiles (square layers: the pack serves as the dgrad's)
            if K == 3 and tile >= 64:
                say("dgrad %dx%d tile %d bitmask + e5m2 copy" % (cout, cin, tile))
                y8 = torch.zeros(y.shape, dtype=torch.uint8, device=dev)
                ops.conv_dgrad_bits_bf8(x, wf, y, mb, y8, torch.ones(1, device=dev), K, S,
                                        amax=ops.fp8_amax_buffer(1, dev)[0], tile=tile)
        for mode, skip in ((0, False), (2, False), (3, False), (0, True), (3, True)):
            for ns in (1, 3):
                say("split-K %dx%d K%d mode %d%s nsplit %d" % (cout, cin, K, mode, " + skip" if skip else "", ns))
                ws = torch.zeros(ns * B * S * S * cout, device=dev)
                ops.conv_fwd_splitk(x, wf, bias, y, K, S, P, 1, mode, mb if mode in (0, 3) else None, ws, ns,
                                    res=res if skip else None)
        torch.cuda.synchronize()

    widths = (64, 128, 192)
    layers = [(co, ci, K, 0) for co in widths for ci in widths for K in (3, 1)]
    layers += [(160, 160, 3, 0), (160, 160, 1, 0), (160, 64, 3, 0), (160, 64, 1, 0)]
    layers += [(co, 64, K, cr) for co in (64, 128, 160, 192) for K in (5, 3) for cr in (48, 49)]
    for cout, cin, K, cr in layers:
        P = K // 2
        x, dz = act(cin, P), act(cout, 1)
        for variant in (0, ops.WGRAD_SMALL):
            if variant and (K != 3 or 160 in (cout, cin) or cr):
                continue
            ns = 2
            say("wgrad %dx%d K%d cin_real %d variant %d plan %s" % (cout, cin, K, cr, variant,
                                                                   tuple(ops.wgrad_plan(cout, cin, K, cr, variant))))
            slab = torch.zeros(ns, K * K, cout, cin, device=dev)
            dbs = torch.zeros(ns, cout, device=dev)
            ops.conv_wgrad(x, dz, slab, dbs, K, S, P, 1, cin_real=cr,
                           variant=variant)
        torch.cuda.synchronize()
    for cout, cin, K, cr in ((192, 192, 3, 192), (192, 64, 5, 48), (128, 128, 3, 128), (160, 160, 3, 160)):
        P = K // 2
        x, dz = act(cin, P), act(cout, 1)
        for ksub in (1, 2, 4, 8):
            say("wgrad direct %dx%d K%d cin_real %d ksub %d" % (cout, cin, K, cr, ksub))
            gw, gb = torch.zeros(cout, cr, K, K, device=dev), torch.zeros(cout, device=dev)
            ops.conv_wgrad_direct(x, dz, gw, gb, K, S, P, 1, ksub=ksub)
        torch.cuda.synchronize()
    print("%d launches" % n)


if __name__ == "__main__":
    main()
