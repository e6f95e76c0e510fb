#!/usr/bin/env python
"""SHA-256 of every output of every 1x1 head op, to compare two builds of the head kernels bit for bit.

Calls each head op at every entry of HEAD_SHAPES (tests/head_refs.py), with and without its optional
inputs (legal, weight, sym, target, ref_probs / stats / coefficients, dz8).  The inputs are drawn on
the CPU from fixed seeds; dz of the accumulating backwards holds prior content.  One line per output
tensor: `<op variant> C=.. C_real=.. B=.. S=.. <output> <sha256>`, and on standard error the number of
lines and the SHA-256 of the whole listing, which is what is worth recording.  Run it on two trees on
one machine and diff the listings:

    python scripts/probes/head_digest.py [--tree DIR] [--out listing.txt]

--tree: import alphago_amd (and its built library) and tests/head_refs.py from DIR instead of the
tree this script is in.  The digests are recorded outputs, not golden values: the device tanhf and
__expf may differ between ROCm releases.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    sys.path.insert(0, tree)

    import torch
    from head_refs import HEAD_SHAPES
    from alphago_amd import ops

    dev = torch.device("cuda")
    out = open(args.out, "w") if args.out else sys.stdout
    lines = []

    def emit(tag, shape, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            h = hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
            lines.append("%-34s C=%d C_real=%d B=%d S=%d %-8s %s" % ((tag,) + shape + (name, h)))
            print(lines[-1], file=out)

    for shape in HEAD_SHAPES:
        C, C_real, B, S = shape
        SS = S * S
        g = torch.Generator().manual_seed(1000003 * C + 10007 * C_real + 101 * B + S)
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        to = lambda t: t.to(dev)  # noqa: E731

        def board(n):
            y = torch.zeros(n, S + 2, S + 2, C, dtype=torch.bfloat16)
            y[:, 1:-1, 1:-1] = rn(n, S, S, C).to(torch.bfloat16)
            return to(y)

        yp = board(B)
        w = [to(rn(C_real) * 0.2) for _ in range(3)]
        bias = [to(rn(1)) for _ in range(3)]
        legal = torch.rand(B, SS, generator=g) < 0.7
        legal[0] = True
        if B > 1:
            legal[1] = False  # an all-illegal board
        legal = to(legal.to(torch.uint8))
        weight = to(rn(B))
        valid = to((torch.rand(B, generator=g) < 0.8).float())
        sym = to(torch.randint(0, 8, (B,), generator=g, dtype=torch.int32))
        target = torch.randint(0, SS, (B,), generator=g, dtype=torch.int32)
        target[0] = -1  # a board without a target
        target = to(target)
        own_target = to(torch.randint(-1, 2, (B, SS), generator=g, dtype=torch.int8))
        ref_probs = to(torch.softmax(rn(B, SS), 1))
        tdist = torch.rand(B, SS + 1, generator=g)
        tdist[0] = 0.0  # no board mass
        tdist = to(tdist)
        g1, g2 = to(rn(B, SS)), to(rn(B, SS))
        dz_prior = to((rn(B, S + 2, S + 2, C) * 0.5).to(torch.bfloat16))
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)  # noqa: E731
        nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731

        # policy_head, inference
        for tag, kw in (("policy_head_probs", {}), ("policy_head_probs legal", dict(legal=legal)),
                        ("policy_head_probs legal T=0.7", dict(legal=legal, temperature=0.7))):
            probs = nan(B, SS)
            ops.policy_head_probs(yp, w[0], bias[0], probs, S, **kw)
            emit(tag, shape, probs=probs)
        probs, stats = nan(B, SS), nan(B, 3)
        ops.policy_head_probs(yp, w[0], bias[0], probs, S, legal=legal, ref_probs=ref_probs, stats=stats)
        emit("policy_head_probs reg", shape, probs=probs, stats=stats)

        # policy_head, training
        for tag, kw in (("policy_head_train", {}), ("policy_head_train weight", dict(weight=weight)),
                        ("policy_head_train bce", dict(bce=True)),
                        ("policy_head_train bce weight", dict(bce=True, weight=weight)),
                        ("policy_head_train probs", dict(probs=nan(B, SS))),
                        ("policy_head_train stats", dict(stats=nan(B, 3))),
                        ("policy_head_train reg", dict(weight=weight, ref_probs=ref_probs, stats=nan(B, 3),
                                                       ent_coef=0.01, kl_coef=0.5, probs=nan(B, SS)))):
            dz, loss, correct, dhead = torch.zeros_like(yp), nan(B), nan(B), nan(B, C_real + 1)
            ops.policy_head_train(yp, w[0], bias[0], target, dz, loss, correct, dhead, S, 0.5, **kw)
            extra = {k: v for k, v in kw.items() if k in ("probs", "stats")}
            emit(tag, shape, dz=dz, loss=loss, correct=correct, dhead=dhead, **extra)

        # policy_head_soft
        for tag, td, kw in (("policy_head_soft", tdist[:, :SS].contiguous(), {}),
                            ("policy_head_soft pass sym", tdist, dict(sym=sym)),
                            ("policy_head_soft sym weight", tdist, dict(sym=sym, weight=weight))):
            dz, loss, correct, dhead = torch.zeros_like(yp), nan(B), nan(B), nan(B, C_real + 1)
            ops.policy_head_train_soft(yp, w[0], bias[0], td, dz, loss, correct, dhead, S, 0.5, **kw)
            emit(tag, shape, dz=dz, loss=loss, correct=correct, dhead=dhead)

        # head_logits / head_backward
        zl = nan(B, SS)
        ops.head_logits(yp, w[1], bias[1], zl, S)
        emit("head_logits", shape, z=zl)
        dz, dhead = torch.zeros_like(yp), nan(B, C_real + 1)
        ops.head_backward(yp, w[1], g1, dz, dhead, S)
        emit("head_backward", shape, dz=dz, dhead=dhead)
        dz, dhead = torch.zeros_like(yp), nan(B, C_real + 1)
        dz8, amax = z(*yp.shape, dtype=torch.uint8), z(64, dtype=torch.int32)
        ops.head_backward(yp, w[1], g1, dz, dhead, S, dz8=dz8, dz8_scale=torch.full((1,), 64.0, device=dev), dz8_amax=amax)
        emit("head_backward dz8", shape, dz8=dz8, amax=amax, dhead=dhead)

        # the accumulating backwards, dz with prior content
        dz, dhead = dz_prior.clone(), nan(B, C_real + 1)
        ops.head_backward_add(yp, w[1], g1, dz, dhead, S)
        emit("head_backward_add", shape, dz=dz, dhead=dhead)
        dz, dh1, dh2 = dz_prior.clone(), nan(B, C_real + 1), nan(B, C_real + 1)
        ops.head_backward_add2(yp, w[1], g1, w[2], g2, dz, dh1, dh2, S)
        emit("head_backward_add2", shape, dz=dz, dhead1=dh1, dhead2=dh2)

        # the dual network's forward heads
        for tag, kw in (("policy_value_head", {}), ("policy_value_head legal", dict(legal=legal))):
            probs, zv = nan(B, SS), nan(B, SS)
            ops.policy_value_head(yp, w[0], bias[0], w[1], bias[1], probs, zv, S, **kw)
            emit(tag, shape, probs=probs, zv=zv)
        for tag, kw in (("policy_value_own_head", {}), ("policy_value_own_head legal", dict(legal=legal))):
            probs, zv, own = nan(B, SS), nan(B, SS), nan(B, SS)
            ops.policy_value_own_head(yp, w[0], bias[0], w[1], bias[1], w[2], bias[2], probs, zv, own, S, **kw)
            emit(tag, shape, probs=probs, zv=zv, own=own)
        zv, own, olog = nan(B, SS), nan(B, SS), nan(B, SS)
        ops.value_own_head(yp, w[1], bias[1], w[2], bias[2], zv, S, own=own, olog=olog)
        emit("value_own_head", shape, zv=zv, own=own, olog=olog)
        for tag, kw in (("value_own_head target", {}),
                        ("value_own_head target sym valid weight", dict(sym=sym, valid=valid, weight=weight))):
            zv, own, oloss, oagree, dlo = nan(B, SS), nan(B, SS), nan(B), nan(B), nan(B, SS)
            ops.value_own_head(yp, w[1], bias[1], w[2], bias[2], zv, S, own=own, target=own_target, oloss=oloss,
                               oagree=oagree, dlo=dlo, grad_scale=0.5, **kw)
            emit(tag, shape, zv=zv, own=own, oloss=oloss, oagree=oagree, dlo=dlo)

        # policy_head_d4: G * Bd boards on the same side of the launch rule as B
        Bd = (B + 7) // 8
        yd = board(8 * Bd)
        symd = to(torch.arange(8, dtype=torch.int32).repeat_interleave(Bd))
        for tag, G, kw in (("policy_head_d4 G=8", 8, {}), ("policy_head_d4 G=8 legal", 8, dict(legal=legal[:Bd].contiguous())),
                           ("policy_head_d4 G=8 legal scratch", 8,
                            dict(legal=legal[:Bd].contiguous(), temperature=0.7, scratch=z(8 * Bd, SS))),
                           ("policy_head_d4 G=1 legal", 1, dict(legal=legal[:Bd].contiguous()))):
            probs = nan(Bd, SS)
            ops.policy_head_probs_d4(yd[:G * Bd], w[0], bias[0], probs, S, symd[:G * Bd].contiguous(), G, **kw)
            emit(tag, shape, probs=probs)
    if args.out:
        out.close()
    print("head_digest: tree %s, %d lines, %d distinct digests, listing sha256 %s" % (
        os.path.basename(tree), len(lines), len({ln.split()[-1] for ln in lines}),
        hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
