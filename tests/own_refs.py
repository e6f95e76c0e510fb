"""Float64 oracles and input builders for the ownership-head kernels (head_own.hip): shared by
test_own_head_kernels.py (GPU) and test_own_refs.py (CPU checks of the oracles), in the style of
head_refs.py, whose cases (activations, shapes) they extend.

A case adds to ``head_refs.head_case(..., "uniform")``: a value head (wv, bv), an ownership head
(wo, bo), an int8 target in {-1, 0, +1} in the stored frame, a symmetry per board, a validity column
(boards 1 and 4 invalid where they exist) and head_refs' signed per-board weights.
"""
import functools
from types import SimpleNamespace

import torch

import head_refs as R

U24 = R.U24

# Largest |tanhf(x) - tanh(x)| of the device tanhf over the olog values of every case, measured on an
# MI355X against float64 tanh of the kernel's own fp32 logits (7.97e-8, at |x| near 0.65; per case 1.3e-8
# to 7.97e-8), and the allowance the tests use: the measured value times 4.
TANHF_MEASURED = 7.97e-8
TANHF_BOUND = 4 * TANHF_MEASURED


def symmetry_tables(n):
    """(8, n*n) long: fwd[s][p] = index of point p after symmetry s (train/engine.symmetry_tables'
    convention, restated here so that the oracle does not import the code under test)."""
    f = [lambda n, x, y: (x, y), lambda n, x, y: (n - 1 - y, x), lambda n, x, y: (n - 1 - x, n - 1 - y),
         lambda n, x, y: (y, n - 1 - x), lambda n, x, y: (x, n - 1 - y), lambda n, x, y: (n - 1 - x, y),
         lambda n, x, y: (y, x), lambda n, x, y: (n - 1 - y, n - 1 - x)]
    t = torch.empty(8, n * n, dtype=torch.long)
    for s in range(8):
        for x in range(n):
            for y in range(n):
                ox, oy = f[s](n, x, y)
                t[s, x * n + y] = ox * n + oy
    return t


def move_rows(rows, sym, S):
    """(B, S*S) rows moved with their boards: the entry of point p goes to fwd[s][p]
    (apply_symmetry_dist's rule: out = rows.gather(inv), inv[b][i] = the point that lands on i)."""
    inv = torch.argsort(symmetry_tables(S).to(rows.device)[sym.long()], dim=1)
    return torch.gather(rows, 1, inv)


def move_board(y, sym):
    """(B, S, S, C) interior activations moved by the same rule."""
    B, S, _, C = y.shape
    inv = torch.argsort(symmetry_tables(S).to(y.device)[sym.long()], dim=1)
    return torch.gather(y.reshape(B, S * S, C), 1, inv.unsqueeze(2).expand(B, S * S, C)).reshape(B, S, S, C)


@functools.lru_cache(maxsize=None)
def own_case(C, C_real, B, S):
    c = R.head_case(C, C_real, B, S, "uniform")
    g = torch.Generator().manual_seed(11 * C + 13 * B + S + 5)
    SS = S * S
    wv = torch.randn(C_real, generator=g) * 0.05
    bv = torch.randn(1, generator=g)
    wo = torch.randn(C_real, generator=g) * 0.05
    bo = torch.randn(1, generator=g) * 0.5
    target = torch.randint(-1, 2, (B, SS), generator=g).to(torch.int8)
    sym = torch.randint(0, 8, (B,), generator=g, dtype=torch.int32)
    sym[0] = 0
    if B > 2:
        sym[2] = 3  # a rotation that is not its own inverse, always present
    valid = torch.ones(B)
    valid[1] = 0.0
    if B > 4:
        valid[4] = 0.0
    return SimpleNamespace(C=C, C_real=C_real, B=B, S=S, y=c.y, wv=wv, bv=bv, wo=wo, bo=bo, target=target, sym=sym,
                           valid=valid, weight=c.weight)


def own_ref(y, wo, bo, target, sym, valid, weight, grad_scale):
    """float64 ownership forward, loss, agreement and gradient.  ``target`` (B, S*S) in the stored
    frame, moved by ``sym`` (None = identity); ``valid`` / ``weight`` None read as 1."""
    B, S = y.shape[0], y.shape[1]
    SS = S * S
    olog = R.logits64(y, wo, bo)
    own = torch.tanh(olog)
    t = target.double()
    if sym is not None:
        t = move_rows(t, sym, S)
    e = own - t
    loss = (e * e).mean(1)
    agree = ((torch.sign(own) == t) & (t != 0)).double().sum(1)
    k = torch.ones(B, dtype=torch.float64)
    if valid is not None:
        k = k * valid.double()
    if weight is not None:
        k = k * weight.double()
    coef = grad_scale * k * (2.0 / SS)
    dlo = coef.unsqueeze(1) * e * (1 - own * own)
    return SimpleNamespace(olog=olog, own=own, t=t, loss=loss, agree=agree, dlo=dlo, coef=coef)


def own_bound(y, wo, bo):
    """|own - tanh(exact logit)| <= TANHF_BOUND + logits_bound: tanh has slope at most 1."""
    return TANHF_BOUND + R.logits_bound(y, wo, bo)


def dlo_bound(ref, ob):
    """f(own) = (own - t)(1 - own^2) has f' = 1 - 3 own^2 + 2 own t, |f'| <= 4 on |own|, |t| <= 1.  The
    fp32 evaluation adds: own - t (error <= 2 U24), 1 - own^2 (two roundings of values <= 1: 2 U24), their
    product (|q| 2 U24 + |e| 2 U24 + U24 |f| <= 8 U24), three roundings in the coefficient (<= 3 U24 |f| <=
    6 U24) and the last product (<= 2 U24): 16 U24 in units of the coefficient."""
    return ref.coef.abs().unsqueeze(1) * (4 * ob + 16 * U24)


def oloss_bound(ref, ob):
    """(own - t)^2 has slope 2 |own - t| <= 4 in own; the mean of S*S terms adds at most (S*S + 8) U24
    of the (non-negative) sum's mean: per-term square and rounding, the chain, the division."""
    SS = ob.shape[1]
    return (4 * ob + ob * ob).mean(1) + (SS + 8) * U24 * ref.loss


def near_zero_points(ref, ob):
    """Points whose float64 ownership lies within the ``own`` bound of 0: the sign the kernel sees is
    not decided there."""
    return (ref.own.abs() <= ob) & (ref.t != 0)


def backward_add2_ref(y, dz_in, g1, w1, g2, w2):
    """float64 dz = dz_in + g1 x w1 + g2 x w2 where y > 0 (else dz_in) on the interior (B, S, S, C),
    and both [dW | db] blocks (B, C_real + 1)."""
    B, S, _, C = y.shape
    cr = w1.numel()
    w1p = torch.zeros(C, dtype=torch.float64)
    w2p = torch.zeros(C, dtype=torch.float64)
    w1p[:cr] = w1.double()
    w2p[:cr] = w2.double()
    a1 = g1.double().view(B, S, S, 1) * w1p
    a2 = g2.double().view(B, S, S, 1) * w2p
    x = torch.where(y > 0, dz_in.double() + a1 + a2, dz_in.double())
    y2 = y.double().flatten(1, 2)[..., :cr]
    p1 = g1.double().unsqueeze(2) * y2
    p2 = g2.double().unsqueeze(2) * y2
    dh1 = torch.cat([p1.sum(1), g1.double().sum(1, keepdim=True)], 1)
    dh2 = torch.cat([p2.sum(1), g2.double().sum(1, keepdim=True)], 1)
    return SimpleNamespace(x=x, mag=dz_in.double().abs() + a1.abs() + a2.abs(), dh1=dh1, dh2=dh2,
                           p1abs=p1.abs().sum(1), p2abs=p2.abs().sum(1))
