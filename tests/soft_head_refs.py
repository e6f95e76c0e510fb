"""Float64 oracle and target builder for the soft-target policy head (head_soft.hip): shared by
test_policy_head_soft.py (GPU) and test_soft_targets_cpu.py (CPU checks of the oracle's pieces).

Activations, weights and per-board gradient weights are head_refs.head_case's.  Target rows are built
in the frame the head sees (the transformed frame) and carried back to the original frame through
the D4 table, so the test decides where each row's maximum lands; the oracle goes the other way with
a scatter of its own.
"""
import functools
from types import SimpleNamespace

import torch

import head_refs as R
from alphago_amd.train.engine import symmetry_tables

# the shapes of head_refs.HEAD_SHAPES that reach each launch variant at the smallest size
SOFT_SHAPES = [(192, 192, 7, 19), (160, 152, 7, 19), (192, 192, 257, 19), (256, 256, 257, 19), (64, 64, 257, 9),
               (8, 8, 3, 9)]

# row kinds, board b has kind KINDS[b % 6]; board 2 is the all-zero row (head_case's target-less board)
DENSE, VISITS, ZERO, ONE_HOT, NEGATIVE, PASS_ONLY = range(6)
KINDS = (DENSE, VISITS, ZERO, ONE_HOT, NEGATIVE, PASS_ONLY)
VISIT_COUNTS = (20, 9, 8, 7, 6, 5, 4, 3, 1, 1)  # 64 visits over 10 points, one clear maximum


@functools.lru_cache(maxsize=None)
def _table(S):
    return symmetry_tables(S)


def cycling_sym(B):
    return (torch.arange(B) % 8).to(torch.int32)


@functools.lru_cache(maxsize=None)
def soft_targets(C, C_real, B, S, T, with_sym):
    """(tdist (B, T) fp32 in the original frame, sym (B,) int32 or None, kind (B,)).

    Every row with board mass has a unique maximum by construction (fp32 cannot tie it).  On odd
    boards the maximum sits where the head's argmax is, so that ``correct`` takes both values.
      DENSE      softmax of normals, the peak entry raised by 0.05
      VISITS     VISIT_COUNTS / 64 on ten points (T = S*S + 1: three further visits on the pass, so the
                 board part sums to 64 / 67 and the renormalisation shows)
      ZERO       all zero: no loss
      ONE_HOT    exactly 1.0 on one point
      NEGATIVE   a DENSE row with five entries negated (they count as 0)
      PASS_ONLY  T = S*S + 1: all mass on the pass column (no loss); T = S*S: a DENSE row
    """
    SS = S * S
    assert T in (SS, SS + 1)
    c = R.head_case(C, C_real, B, S, "uniform")
    g = torch.Generator().manual_seed(11 * C + 5 * B + S + T)
    top = R.logits64(c.y, c.w, c.b).argmax(1)
    kind = torch.tensor([KINDS[b % 6] for b in range(B)])
    qt = torch.zeros(B, T)
    for b in range(B):
        k = int(kind[b])
        peak = int(top[b]) if b % 2 == 1 else int(torch.randint(0, SS, (1,), generator=g))
        if k in (DENSE, NEGATIVE) or (k == PASS_ONLY and T == SS):
            row = torch.softmax(torch.randn(SS, generator=g), 0)
            row[peak] = row.max() + 0.05
            if k == NEGATIVE:
                others = torch.tensor([p for p in torch.randperm(SS, generator=g).tolist() if p != peak][:5])
                row[others] = -row[others] - 0.01
            if T == SS + 1:
                qt[b, SS] = 0.125
            qt[b, :SS] = row
        elif k == VISITS:
            pts = [peak] + [p for p in torch.randperm(SS, generator=g).tolist() if p != peak][:len(VISIT_COUNTS) - 1]
            n = sum(VISIT_COUNTS) + (3 if T == SS + 1 else 0)
            qt[b, torch.tensor(pts)] = torch.tensor(VISIT_COUNTS, dtype=torch.float32) / n
            if T == SS + 1:
                qt[b, SS] = 3.0 / n
        elif k == ONE_HOT:
            qt[b, peak] = 1.0
        elif k == PASS_ONLY:
            qt[b, SS] = 1.0
    sym = cycling_sym(B) if with_sym else None
    tdist = qt.clone()
    if with_sym:  # tdist[b][p] = qt[b][fwd_s(p)]: the kernel's gather brings it back
        tdist[:, :SS] = torch.gather(qt[:, :SS], 1, _table(S)[sym.long()])
    return tdist.contiguous(), sym, kind


def transformed(tdist, sym, S):
    """The board part of ``tdist`` in the frame of the transformed planes, float64, negatives as 0:
    the mass of point p goes to fwd_s(p) (the integer-target rule of pack_input)."""
    SS = S * S
    q = tdist[:, :SS].double().clamp_min(0)
    if sym is None:
        return q
    fwd = _table(S).to(tdist.device)[sym.long()]
    return torch.zeros_like(q).scatter_(1, fwd, q)


def soft_policy_ref(y, w, b, tdist, sym, weight, grad_scale):
    """fp64 autograd of the soft-target objective, mirroring head_refs.policy_ref: negatives clamped,
    the pass column dropped, the rest renormalised, CE through log_softmax (no clip), per-board
    weights, boards without mass excluded.  Returns loss (B,), correct (B,), dz (B, S, S, C)
    ReLU'-masked, dhead (B, C_real + 1), the logits and has (B,)."""
    S = y.shape[1]
    cr = w.numel()
    y64 = y.double().requires_grad_(True)
    z = (y64[..., :cr] * w.double()).sum(-1).flatten(1) + b.double()
    z.retain_grad()
    q = transformed(tdist, sym, S)
    m = q.sum(1, keepdim=True)
    has = m.squeeze(1) > 0
    qh = q / torch.where(m > 0, m, torch.ones_like(m))
    wt = (weight.double() if weight is not None else torch.ones_like(z[:, 0])) * has
    per = -(qh * torch.log_softmax(z, 1)).sum(1) * has
    (per * wt).sum().mul(grad_scale).backward()
    dl = z.grad
    yd = y.double()
    dhead = torch.cat([torch.einsum("bp,bpc->bc", dl, yd.flatten(1, 2)[..., :cr]), dl.sum(1, keepdim=True)], 1)
    zd = z.detach()
    correct = ((R.first_argmax(zd) == R.first_argmax(q)) & has).double()
    return SimpleNamespace(loss=per.detach(), correct=correct, dz=y64.grad * (yd > 0), dhead=dhead, logits=zd,
                           has=has, q=q)
