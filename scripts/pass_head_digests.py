#!/usr/bin/env python
"""sha256 of every output of the pass-head ops and of the soft head on seeded inputs.

  python scripts/pass_head_digests.py [--tree DIR] [--out FILE]

Two builds that print the same lines compute the same bits: run it on each (one process per build; --tree names
the checkout whose alphago_amd package is loaded, default this one) and compare the outputs.  The cases are
tests/pass_head_refs.PASS_SHAPES with and without sym / weight (policy_head_soft_pass, policy_head_train_soft)
and with and without legal / own (policy_value_pass_head); the last line per inference case says whether a
silent pass (pass_w = 0, pass_b = -1e30) leaves policy_value_own_head's bits in the board columns of probs."""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS_SHAPES = [(192, 192, 7, 19), (160, 152, 7, 19), (192, 192, 257, 19), (8, 8, 3, 9)]  # tests/pass_head_refs.py


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from alphago_amd import ops

    if not torch.cuda.is_available():
        sys.exit("pass_head_digests.py needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def emit(case, outs):
        for k, v in outs.items():
            lines.append("%s %s %s" % (case, k, sha(v)))
            print(lines[-1], flush=True)

    for C, Cr, B, S in PASS_SHAPES:
        SS = S * S
        g = torch.Generator().manual_seed(1000 * C + 10 * B + S)
        y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
        yi = torch.randn(B, S, S, C, generator=g).clamp_min(0)
        yi[..., Cr:] = 0
        y[:, 1:-1, 1:-1] = yi.to(dev)
        w, wv, wo = ((torch.randn(Cr, generator=g) * 0.05).to(dev) for _ in range(3))
        b, bv, bo = (torch.randn(1, generator=g).to(dev) for _ in range(3))
        pw = torch.zeros(2, C)
        pw[:, :Cr] = torch.randn(2, Cr, generator=g) * 0.01
        pw = pw.to(dev)
        pb = torch.tensor([0.75], device=dev)
        P = torch.zeros(B, 2, C, device=dev)
        am = torch.zeros(B, C, dtype=torch.int32, device=dev)
        ops.gpool_fwd(y, P, am, S)
        td = torch.rand(B, SS + 1, generator=g) ** 4
        td[0] = 0  # a board without mass
        td = td.to(dev)
        sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
        wt = (torch.rand(B, generator=g) + 0.5).to(dev)
        lg = (torch.rand(B, SS, generator=g) > 1.0 / 3.0).to(torch.uint8)
        lg[B - 1] = 0
        lg = lg.to(dev)
        shape = "C%d,Cr%d,B%d,S%d" % (C, Cr, B, S)
        for with_sym in (0, 1):
            for weighted in (0, 1):
                kw = dict(sym=sym if with_sym else None, weight=wt if weighted else None)
                tag = "%s sym%d weight%d" % (shape, with_sym, weighted)
                o = dict(dz=torch.zeros_like(y), loss=torch.zeros(B, device=dev), correct=torch.zeros(B, device=dev),
                         dhead=torch.zeros(B, Cr + 1, device=dev), dpass=torch.zeros(B, device=dev),
                         dpw=torch.zeros(B, 2 * Cr + 1, device=dev))
                ops.policy_head_soft_pass(y, w, b, P, pw, pb, td, o["dz"], o["loss"], o["correct"], o["dhead"],
                                          o["dpass"], o["dpw"], S, 1.0 / B, **kw)
                emit("policy_head_soft_pass " + tag, o)
                for T in (SS, SS + 1):
                    s = dict(dz=torch.zeros_like(y), loss=torch.zeros(B, device=dev), correct=torch.zeros(B, device=dev),
                             dhead=torch.zeros(B, Cr + 1, device=dev))
                    ops.policy_head_train_soft(y, w, b, td[:, :T].contiguous(), s["dz"], s["loss"], s["correct"],
                                               s["dhead"], S, 1.0 / B, **kw)
                    emit("policy_head_train_soft T%d %s" % (T, tag), s)
        for legal in (0, 1):
            for own in (0, 1):
                tag = "%s legal%d own%d" % (shape, legal, own)
                lgd = lg if legal else None

                def run(pass_w, pass_b):
                    o = dict(probs=torch.zeros(B, SS + 1, device=dev), zv=torch.zeros(B, SS, device=dev))
                    kw = {}
                    if own:
                        o["own"] = torch.zeros(B, SS, device=dev)
                        kw = dict(wo=wo, bo=bo, own=o["own"])
                    ops.policy_value_pass_head(y, w, b, wv, bv, P, pass_w, pass_b, o["probs"], o["zv"], S, legal=lgd, **kw)
                    return o

                emit("policy_value_pass_head " + tag, run(pw, pb))
                silent = run(torch.zeros_like(pw), torch.tensor([-1e30], device=dev))
                p0, zv0, own0 = (torch.zeros(B, SS, device=dev) for _ in range(3))
                ops.policy_value_own_head(y, w, b, wv, bv, wo, bo, p0, zv0, own0, S, legal=lgd)
                live = lgd.bool().any(1) if legal else torch.ones(B, dtype=torch.bool, device=dev)
                same = torch.equal(silent["probs"][live, :SS].view(torch.int32), p0[live].view(torch.int32))
                lines.append("policy_value_pass_head %s silent_pass_board_columns_equal_own_head %s" % (tag, same))
                print(lines[-1], flush=True)
    torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
