"""Float64 reference, written from its formulas, and input builders for the pass head of the dual net
(the PASS variants of head_soft.hip / head_own.hip, gpool_bwd_add_masked): shared by test_pass_head_cpu.py (which
holds the net's torch expression and its autograd to this reference) and test_pass_head_kernels.py (GPU).

Activations, 1x1 head weights and per-board weights are head_refs.head_case's.  With h the (B, S, S, C)
activations (after their ReLU), NP = S * S and inv = float32(1 / NP):

    P[b, 0, c] = (sum_p h[b, p, c]) * inv,  P[b, 1, c] = max_p h[b, p, c],  a[b, c] = lowest pixel attaining it
    z[b] = [h[b] . w + bias (NP entries), P[b].reshape(2 C_real) . pass_w + pass_b]

The target row (NP + 1 entries, the pass last) has its board part moved with the board's symmetry; q = max(t, 0)
with NaN -> 0, m = sum q, has = 0 < m < inf, qh = q / m, L = -sum qh log softmax(z), correct = [first argmax z
== first argmax q], dL/dz = (softmax(z) - qh) * grad_scale * weight.  No autograd here: every gradient is the
closed form.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import head_refs as R
import soft_head_refs as SR

# the soft head's smallest shape of each kind: BoardRegs, padded channels, BoardRows, the smallest
PASS_SHAPES = [(192, 192, 7, 19), (160, 152, 7, 19), (192, 192, 257, 19), (8, 8, 3, 9)]

# the soft head's six row kinds, a pass-majority row and a mixed pass-and-board row
DENSE, VISITS, ZERO, ONE_HOT, NEGATIVE, PASS_ONLY = SR.DENSE, SR.VISITS, SR.ZERO, SR.ONE_HOT, SR.NEGATIVE, SR.PASS_ONLY
PASS_MAJOR, MIXED = 6, 7
KINDS8 = (DENSE, VISITS, ZERO, ONE_HOT, NEGATIVE, PASS_ONLY, PASS_MAJOR, MIXED)
# Fewer than eight boards: board 2 stays the all-zero row (head_case's target-less board).  All eight kinds occur
# together only at B = 257 (the BoardRows shape).  At B = 7 (the BoardRegs and padded-channel shapes) MIXED stands
# in for DENSE: it is a DENSE row with more of its mass on the pass and a higher peak, so those shapes never see a
# row whose pass entry is as small as DENSE's 0.01; NEGATIVE, a DENSE row with five entries negated, has that
# entry.  At B = 3 (the 8-channel shape) only PASS_MAJOR, MIXED and ZERO occur.
KINDS7 = (MIXED, VISITS, ZERO, ONE_HOT, NEGATIVE, PASS_ONLY, PASS_MAJOR)
KINDS3 = (PASS_MAJOR, MIXED, ZERO)

PASS_B_HIGH = 12.0  # lifts the pass logit above every board logit of every case (asserted where it is used)


def inv32(S):
    """float32(1 / (S * S)) as a Python float."""
    return float(np.float32(1.0 / (S * S)))


def kinds_of(B):
    ks = KINDS3 if B == 3 else KINDS7 if B == 7 else None
    return torch.tensor([(ks[b] if ks else KINDS8[b % 8]) for b in range(B)])


@functools.lru_cache(maxsize=None)
def pass_weights(C_real):
    """pass_w (2 C_real,) fp32, small enough that at pass_b = 0 the pass logit stays below the doubled top
    board logit of head_case (checked by argmax_is_decided in the tests)."""
    g = torch.Generator().manual_seed(31 * C_real + 1)
    return (torch.randn(2 * C_real, generator=g) * 0.01).contiguous()


def padded_pass_w(pass_w, C):
    """The zero-padded (2, C) copy the kernels read."""
    cr = pass_w.numel() // 2
    out = torch.zeros(2, C, dtype=pass_w.dtype, device=pass_w.device)
    out[:, :cr] = pass_w.view(2, cr)
    return out


@functools.lru_cache(maxsize=None)
def pass_targets(C, C_real, B, S, with_sym):
    """(tdist (B, NP + 1) fp32 in the original frame, sym (B,) int32 or None, kind (B,)).  Rows are built in
    the frame the head sees and carried back through the D4 table (soft_head_refs.soft_targets' way); the
    pass entry does not move.  Every row with mass has a unique maximum: on odd boards the board maximum
    sits on the 1x1 head's top logit; PASS_ONLY and PASS_MAJOR rows have it on the pass.
      DENSE       softmax of normals, the peak raised by 0.05, 0.01 on the pass
      VISITS      SR.VISIT_COUNTS on ten points and three visits on the pass, over 67
      ZERO        all zero: no loss
      ONE_HOT     1.0 on one board point
      NEGATIVE    a DENSE row with five entries negated (they count as 0)
      PASS_ONLY   1.0 on the pass: a loss now
      PASS_MAJOR  a DENSE board part and 2.0 on the pass (about two thirds of the mass)
      MIXED       a DENSE board part with the peak raised by 0.3 and 0.2 on the pass
    """
    SS = S * S
    c = R.head_case(C, C_real, B, S, "uniform")
    g = torch.Generator().manual_seed(13 * C + 7 * B + S)
    top = R.logits64(c.y, c.w, c.b).argmax(1)
    kind = kinds_of(B)
    qt = torch.zeros(B, SS + 1)
    for b in range(B):
        k = int(kind[b])
        peak = int(top[b]) if b % 2 == 1 else int(torch.randint(0, SS, (1,), generator=g))
        if k in (DENSE, NEGATIVE, PASS_MAJOR, MIXED):
            row = torch.softmax(torch.randn(SS, generator=g), 0)
            row[peak] = row.max() + (0.3 if k == MIXED else 0.05)
            if k == NEGATIVE:
                others = torch.tensor([p for p in torch.randperm(SS, generator=g).tolist() if p != peak][:5])
                row[others] = -row[others] - 0.01
            qt[b, :SS] = row
            qt[b, SS] = {DENSE: 0.01, NEGATIVE: 0.01, PASS_MAJOR: 2.0, MIXED: 0.2}[k]
        elif k == VISITS:
            pts = [peak] + [p for p in torch.randperm(SS, generator=g).tolist() if p != peak][:len(SR.VISIT_COUNTS) - 1]
            n = sum(SR.VISIT_COUNTS) + 3
            qt[b, torch.tensor(pts)] = torch.tensor(SR.VISIT_COUNTS, dtype=torch.float32) / n
            qt[b, SS] = 3.0 / n
        elif k == ONE_HOT:
            qt[b, peak] = 1.0
        elif k == PASS_ONLY:
            qt[b, SS] = 1.0
    sym = SR.cycling_sym(B) if with_sym else None
    tdist = qt.clone()
    if with_sym:  # tdist[b][p] = qt[b][fwd_s(p)]: the kernel's gather brings it back
        tdist[:, :SS] = torch.gather(qt[:, :SS], 1, SR._table(S)[sym.long()])
    return tdist.contiguous(), sym, kind


def transformed_rows(tdist, sym, S):
    """(B, NP + 1) float64 q in the frame of the transformed planes: negatives and NaN as 0, the board part
    scattered to fwd_s(p), the pass entry where it is."""
    SS = S * S
    t = tdist.double()
    q = torch.where(t > 0, t, torch.zeros_like(t))
    if sym is None:
        return q
    fwd = SR._table(S).to(tdist.device)[sym.long()]
    out = q.clone()
    out[:, :SS] = torch.zeros_like(q[:, :SS]).scatter_(1, fwd, q[:, :SS])
    return out


def pool64(y, cr=None):
    """P (B, 2, cr) float64 and a (B, cr) int64 of (B, S, S, C) activations: the mean with the fp32 factor,
    the maximum and the lowest pixel index attaining it."""
    B, S = y.shape[:2]
    cr = y.shape[3] if cr is None else cr
    flat = y[..., :cr].double().reshape(B, S * S, cr)
    a = R.first_argmax(flat.transpose(1, 2).reshape(B * cr, S * S)).view(B, cr)
    return torch.stack([flat.sum(1) * inv32(S), flat.max(1).values], 1), a


def pass_logit_bound(y, pass_w, pass_b):
    """A bound on |fp32 z_pass - exact|: the pooled sums carry at most 362 u each (361 adds and the product with
    inv), the dot product of 2 C terms and the bias (2 C + 2) u of its magnitude; u = 2^-24."""
    B, S = y.shape[:2]
    cr = pass_w.numel() // 2
    P, _ = pool64(y, cr)
    Pabs = torch.stack([y[..., :cr].double().abs().reshape(B, S * S, cr).sum(1) * inv32(S), P[:, 1].abs()], 1)
    w = pass_w.double().view(2, cr).abs()
    mag = (Pabs * w).sum((1, 2)) + abs(float(pass_b))
    return 362 * R.U24 * (Pabs[:, 0] * w[0]).sum(1) + (2 * y.shape[3] + 2) * R.U24 * mag


def pass_head_ref(y, w, b, pass_w, pass_b, tdist, sym, weight, grad_scale):
    """The whole head in float64 from the formulas in the module docstring.  y (B, S, S, C) bf16 interiors, w
    (C_real,), b (1,), pass_w (2 C_real,), pass_b a float, tdist (B, NP + 1).  Returns
      logits (B, NP + 1), q, has, loss (B,), correct (B,), dlogits (B, NP + 1),
      dz (B, S, S, C): the 1x1 head's ReLU'-masked gradient (what the head kernel writes),
      dhead (B, C_real + 1), dpass (B,), dpw (B, 2 C_real + 1) = [dpass * P | dpass],
      dpool (B, S, S, C): the pooling's ReLU'-masked gradient (what gpool_bwd_add_masked adds),
      P (B, 2, C_real), argmax (B, C_real)."""
    B, S, _, C = y.shape
    SS = S * S
    cr = w.numel()
    yd = y.double()
    flat = yd.reshape(B, SS, C)
    P, a = pool64(y, cr)
    pw = pass_w.double().view(2, cr)
    zb = (flat[..., :cr] * w.double()).sum(-1) + b.double()
    zp = (P * pw).sum((1, 2)) + float(pass_b)
    z = torch.cat([zb, zp[:, None]], 1)
    q = transformed_rows(tdist, sym, S)
    m = q.sum(1, keepdim=True)
    has = ((m > 0) & torch.isfinite(m)).squeeze(1)
    qh = torch.where(has[:, None], q / torch.where(has[:, None], m, torch.ones_like(m)), torch.zeros_like(q))
    zmax = z.max(1, keepdim=True).values
    logp = z - zmax - (z - zmax).exp().sum(1, keepdim=True).log()
    loss = -torch.where(qh > 0, qh * logp, torch.zeros_like(logp)).sum(1) * has
    correct = ((R.first_argmax(z) == R.first_argmax(q)) & has).double()
    sc = grad_scale * (weight.double() if weight is not None else torch.ones(B, dtype=torch.float64)) * has
    dl = (logp.exp() - qh) * sc[:, None]
    dl = torch.where(has[:, None], dl, torch.zeros_like(dl))
    relu = (flat > 0).double()
    dz = torch.zeros_like(flat)
    dz[..., :cr] = dl[:, :SS, None] * w.double()
    dz = dz * relu
    dhead = torch.cat([torch.einsum("bp,bpc->bc", dl[:, :SS], flat[..., :cr]), dl[:, :SS].sum(1, keepdim=True)], 1)
    dzp = dl[:, SS]
    dpw = torch.cat([(dzp[:, None, None] * P).reshape(B, 2 * cr), dzp[:, None]], 1)
    dP = dzp[:, None, None] * pw  # (B, 2, cr)
    hit = (torch.arange(SS)[None, :, None] == a[:, None, :]).double()
    dpool = torch.zeros_like(flat)
    dpool[..., :cr] = dP[:, 0][:, None, :] * inv32(S) + hit * dP[:, 1][:, None, :]
    dpool = dpool * relu
    return SimpleNamespace(logits=z, q=q, has=has, loss=loss, correct=correct, dlogits=dl, dz=dz.view(B, S, S, C),
                           dhead=dhead, dpass=dzp, dpw=dpw, dpool=dpool.view(B, S, S, C), P=P, argmax=a)


def pass_probs_ref(y, w, b, pass_w, pass_b, legal):
    """(B, NP + 1) float64 inference probabilities: the softmax over the legal board points (legal (B, NP) uint8
    or None) and the pass, which is always legal."""
    B, S, _, C = y.shape
    cr = w.numel()
    P, _ = pool64(y, cr)
    z = torch.cat([R.logits64(y, w, b), ((P * pass_w.double().view(2, cr)).sum((1, 2)) + float(pass_b))[:, None]], 1)
    if legal is not None:
        ok = torch.cat([legal.bool(), torch.ones(B, 1, dtype=torch.bool)], 1)
        z = z.masked_fill(~ok, -math.inf)
    return torch.softmax(z, 1)
