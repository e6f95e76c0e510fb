"""Float64 oracles and input builders for the kernels after the trunk (head.hip, policy_head.h,
sample.hip): shared by test_head_kernels.py (GPU) and test_head_refs.py (CPU checks of the oracles).

Inputs are drawn on the CPU from seeded generators, so the CPU tests see exactly the tensors the
GPU tests hand to the kernels.  Activations are NHWC interiors (B, S, S, C) already rounded to bf16;
``w`` and ``b`` are fp32.  Every reference is plain torch in float64 on the device of its inputs.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

U24 = 2.0 ** -24  # fp32 unit roundoff

# the fused head's clip constants as the kernel holds them (fp32)
EPS_LO = float(np.float32(1e-7))
EPS_HI = float(np.float32(1.0) - np.float32(1e-7))

# (C, C_real, B, S): the smallest shapes that reach each launch variant
#   B < 256: 1024 threads (BoardRegs; head_logits / head_backward <1024>)
#   B >= 256 and S * C / 8 <= 512: 512 threads, row-mapped (BoardRows); head_logits / head_backward <256>
#   B >= 256 and S * C / 8 > 512 (C = 256, S = 19): the 1024-thread kernel again
HEAD_SHAPES = [(192, 192, 7, 19), (160, 152, 7, 19), (192, 192, 257, 19), (160, 152, 257, 19), (256, 256, 257, 19),
               (64, 64, 257, 9), (192, 192, 7, 13), (192, 192, 257, 13), (8, 8, 3, 9)]

SIGNED_WEIGHTS = (1.0, -1.0, 2.0, -0.5, 1.0, 3.0)
CLIP_OFFSETS = (0.0, 8.0, 16.0, 40.0)  # bf16-exact activations of the controlled channel (w = 1)


def pad_nhwc(y):
    """(B, S, S, C) -> zero-bordered (B, S + 2, S + 2, C), same dtype."""
    B, S, _, C = y.shape
    out = torch.zeros(B, S + 2, S + 2, C, dtype=y.dtype, device=y.device)
    out[:, 1:-1, 1:-1] = y
    return out


def border_is_zero(t):
    z = t.clone()
    z[:, 1:-1, 1:-1] = 0
    return not bool(z.float().abs().max() > 0)


@functools.lru_cache(maxsize=None)
def head_case(C, C_real, B, S, regime):
    """Inputs of one head shape.

    regime "uniform": w ~ 0.05 N(0, 1), y = relu(bf16(N(0, 1))): near-uniform softmax.  Boards 0 and 1
    are dead (y = 0, targets 0 and 5), board 2 has no target (-1).

    regime "clip": the same plus channel 0 with w = 1 and activations from CLIP_OFFSETS, so that the
    softmax reaches both clip branches of the head:
      * board 0: one position at 40 (the target), the rest at 0 / 8: p_target > 1 - 1e-7;
      * boards with b % 3 == 1 (board 1 among them): target on a position at offset 0 while ~40 % of
        the board sits at 40: p_target < 1e-7, the positions at 40 are inside the range;
      * every other board: ~40 % of the positions at 40 (inside the range, the target one of them),
        the rest at 0 / 8 / 16 (below 1e-7);
      * board 2 has no target.
    """
    g = torch.Generator().manual_seed(7 * C + 3 * B + S + (1000 if regime == "clip" else 0))
    SS = S * S
    y = torch.randn(B, S, S, C, generator=g).to(torch.bfloat16).clamp_min(0)
    y[..., C_real:] = 0  # the trunk leaves padded channels zero
    w = torch.randn(C_real, generator=g) * 0.05
    b = torch.randn(1, generator=g)
    target = torch.randint(0, SS, (B,), generator=g, dtype=torch.int32)
    if regime == "uniform":
        y[0] = 0
        y[1] = 0
        target[0] = 0
        target[1] = 5
    else:
        assert regime == "clip"
        off = torch.randint(0, 3, (B, SS), generator=g).float() * 8.0
        hot = torch.rand(B, SS, generator=g) < 0.4
        hot[:, 0] = True   # every board has a position at 40 ...
        hot[:, 1] = False  # ... and one at 0
        off[:, 1] = 0.0
        off = torch.where(hot, torch.full_like(off, 40.0), off)
        off[0] = torch.randint(0, 2, (SS,), generator=g).float() * 8.0
        off[0, SS // 2] = 40.0
        for bb in range(B):
            pool = ((off[bb] == 0.0) if bb % 3 == 1 else (off[bb] == 40.0)).nonzero().flatten()
            target[bb] = pool[int(torch.randint(0, len(pool), (1,), generator=g))]
        y[..., 0] = off.view(B, S, S).to(torch.bfloat16)
        w[0] = 1.0
    # The head's top-1 flag is compared exactly, so the leading logit of every board is lifted clear
    # of the runner-up by more than fp32 can move either (argmax_is_decided checks it): its row is
    # doubled (exact in bf16), or in the clip regime its controlled activation goes from 40 to 40.5.
    q = logits64(y, w, b).argmax(1)
    rows = torch.arange(B)
    yq = y.view(B, SS, C)
    if regime == "uniform":
        yq[rows, q] = yq[rows, q] * 2
    else:
        yq[rows, q, 0] = torch.where(yq[rows, q, 0] == 40.0, torch.full_like(yq[rows, q, 0], 40.5), yq[rows, q, 0])
    target[2] = -1
    weight =torch.tensor(SIGNED_WEIGHTS).repeat(B // len(SIGNED_WEIGHTS) + 1)[:B].contiguous()
    return SimpleNamespace(C=C, C_real=C_real, B=B, S=S, y=y, w=w, b=b, target=target, weight=weight)


def logits64(y, w, b):
    """(B, S*S) float64 logits of the 1x1 head conv from the bf16 activations and fp32 w, b."""
    cr = w.numel()
    return (y[..., :cr].double() * w.double()).sum(-1).flatten(1) + b.double()


def logits_bound(y, w, b):
    """|fp32 logit - exact| <= (C + 2) * 2^-24 * (sum_c |y w| + |b|): one rounding per product, at
    most C per summation chain, and the bias add."""
    cr = w.numel()
    mag = (y[..., :cr].double() * w.double()).abs().sum(-1).flatten(1) + b.double().abs()
    return (y.shape[-1] + 2) * U24 * mag


def first_argmax(z):
    """Smallest index among the row maxima (the block argmax's tie rule)."""
    n = z.shape[1]
    idx = torch.arange(n, device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values


def argmax_is_decided(z, bound):
    """True when every row's maximum exceeds every smaller logit by more than twice the fp32 error
    bound of a logit: fp32 cannot reorder them (exact ties stay ties only by construction)."""
    zmax = z.max(1, keepdim=True).values
    below = torch.where(z < zmax, z, torch.full_like(z, -math.inf))
    gap = zmax.squeeze(1) - below.max(1).values
    return bool((gap > 2 * bound.max(1).values).all())


def clip_band_clear(p):
    """No probability within a factor 2 of either clip threshold (the clip is a discontinuity of the
    reference RL loss's gradient, and of the CE loss value at the lower one)."""
    lo = ((p >= 0.5e-7) & (p <= 2e-7)).any()
    hi = ((p >= 1 - 2e-7) & (p <= 1 - 0.5e-7)).any()
    return not bool(lo or hi)


def policy_ref(y, w, b, target, weight, grad_scale, kind):
    """fp64 autograd of the trainers' head objective (TorchPolicyTrainer._loss).

    kind "bce": softmax, clamp(1e-7, 1 - 1e-7) (fp32 constants), mean binary CE over S*S, times
    weight[b], times valid, times grad_scale.  kind "ce": the per-board loss is the clipped CE, the
    gradient that of the unclipped CE times weight[b] * valid * grad_scale.
    Returns loss (B,), correct (B,), dz (B, S, S, C) ReLU'-masked, dhead (B, C_real + 1) per board,
    probs (B, S*S) and the logits."""
    cr = w.numel()
    y64 = y.double().requires_grad_(True)
    w64 = w.double()
    z = (y64[..., :cr] * w64).sum(-1).flatten(1) + b.double()
    z.retain_grad()
    t = target.long()
    valid = t >= 0
    tc = t.clamp_min(0)
    wt = (weight.double() if weight is not None else torch.ones_like(z[:, 0])) * valid
    p = torch.softmax(z, 1)
    if kind == "bce":
        pc = p.clamp(EPS_LO, EPS_HI)
        oh = torch.nn.functional.one_hot(tc, z.shape[1]).double()
        per = -(oh * pc.log() + (1 - oh) * (1 - pc).log()).mean(1) * valid
        obj = (per * wt).sum() * grad_scale
    else:
        lt = torch.log_softmax(z, 1).gather(1, tc.unsqueeze(1)).squeeze(1)
        per = -lt.clamp(math.log(EPS_LO), math.log(EPS_HI)) * valid
        obj = -(lt * wt).sum() * grad_scale
    obj.backward()
    dl = z.grad
    yd = y.double()
    dhead = torch.cat([torch.einsum("bp,bpc->bc", dl, yd.flatten(1, 2)[..., :cr]), dl.sum(1, keepdim=True)], 1)
    zd = z.detach()
    correct = ((first_argmax(zd) == t) & valid).double()
    return SimpleNamespace(loss=per.detach(), correct=correct, dz=y64.grad * (yd > 0), dhead=dhead, probs=p.detach(),
                           logits=zd, dlogits=dl)


# ---------------------------------------------------------------------------- sample_moves
_M64 = (1 << 64) - 1


def mix64(x):
    """One splitmix64 step from state x (sample.hip): add the golden-ratio increment, then the two
    multiply-xorshift rounds."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def u01(seed, b):
    """The sampler's uniform of board b: 24 bits of the hash of (seed, b)."""
    return (mix64((seed * 0x100000001B3 + b) & _M64) >> 40) / 2.0 ** 24


ROW_ONE_HOT, ROW_NO_MOVE, ROW_ALL_ZERO, ROW_LAST_ONLY = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def sample_case(NP, B):
    """(B, NP) fp32 rows: random positive entries, about a third exactly 0, ~1 % negative (the kernel
    clamps them), ~2 % denormal-sized; rows 0-3 are the edge rows above.  Returns (probs, has)."""
    g = torch.Generator().manual_seed(100 + NP)
    p = torch.rand(B, NP, generator=g) + 1e-3
    r = torch.rand(B, NP, generator=g)
    p[r < 1 / 3] = 0.0
    p[(r >= 0.40) & (r < 0.41)] *= -1.0
    p[(r >= 0.50) & (r < 0.52)] = 1e-40
    p[ROW_ONE_HOT] = 0.0
    p[ROW_ONE_HOT, NP // 3] = 1.0
    p[ROW_ALL_ZERO] = 0.0
    p[ROW_LAST_ONLY] = 0.0
    p[ROW_LAST_ONLY, NP - 1] = 0.25
    has = torch.ones(B, dtype=torch.bool)
    has[ROW_NO_MOVE] = False
    return p, has


def sample_cdf(p, beta):
    """float64 weights max(p, 0) ** beta and their running sums."""
    w = p.double().clamp_min(0) ** beta
    w = torch.where(p > 0, w, torch.zeros_like(w))
    return w, w.cumsum(1)


def sample_miss(p, beta, seed, out):
    """Per board: the distance by which the returned entry's interval [cdf[i-1], cdf[i]] misses
    u = u01 * total, relative to total (0 = u inside), and whether the entry has positive weight.
    Boards with total == 0 get miss 0 / positive True; the caller checks them separately."""
    w, cdf = sample_cdf(p, beta)
    B, NP = p.shape
    total = cdf[:, -1]
    u = torch.tensor([u01(seed, b) for b in range(B)], dtype=torch.float64) * total
    i = out.clamp(0, NP - 1).unsqueeze(1)
    hi = cdf.gather(1, i).squeeze(1)
    wi = w.gather(1, i).squeeze(1)
    lo = hi - wi
    miss = torch.maximum(torch.maximum(lo - u, u - hi), torch.zeros_like(u))
    live = total > 0
    miss = torch.where(live, miss / total.clamp_min(1e-300), torch.zeros_like(miss))
    return miss, (wi > 0) | ~live


def sample_exact(p, beta, seed):
    """The float64 inverse-CDF index of every board (-1 where the row has no weight)."""
    w, cdf = sample_cdf(p, beta)
    B = p.shape[0]
    total = cdf[:, -1]
    u = torch.tensor([u01(seed, b) for b in range(B)], dtype=torch.float64) * total
    idx = (cdf <= u.unsqueeze(1)).sum(1).clamp_max(p.shape[1] - 1)
    return torch.where(total > 0, idx, torch.full_like(idx, -1))
