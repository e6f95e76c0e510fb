"""Float64 references of the dual net's score head, written from its formulas (PolicyValueNet's docstring), not from
``score_torch``: shared by test_score_head_cpu.py, test_score_head_kernels.py and test_score_head_engines.py.

With h (B, F, S, S) the trunk output after its ReLU, NP = S * S and inv = float32(1 / NP):

    P[b, 0, c] = (sum_p h[b, c, p]) * inv          P[b, 1, c] = max_p h[b, c, p]   (ties: the lowest p)
    upre[b]    = P[b].reshape(2F) @ sc1_w + sc1_b  u = max(upre, 0)
    s[b]       = u[b] @ sc2_w + sc2_b              score[b] = S * s[b]
    e = s - t,  loss = Huber_delta(e),  g = grad_scale * valid * weight * clamp(e, -delta, delta)
"""
from collections import namedtuple

import torch

U24 = 2.0 ** -24
KINK = 1e-4  # elements this close to a kink of the ReLU or of the Huber loss are not compared


def inv32(S: int) -> float:
    return float(torch.tensor(1.0 / (S * S), dtype=torch.float32))


def first_argmax(z):
    n = z.shape[1]
    idx = torch.arange(n, device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values


def pooled_ref(h):
    """(P (B, 2, F) float64, argmax (B, F)) of h (B, F, S, S)."""
    B, F, S, _ = h.shape
    flat = h.double().reshape(B * F, S * S)
    am = first_argmax(flat)
    mean = flat.sum(1) * inv32(S)
    mx = flat.gather(1, am[:, None])[:, 0]
    return torch.stack([mean.view(B, F), mx.view(B, F)], 1), am.view(B, F)


def score_ref(h, sc1_w, sc1_b, sc2_w, sc2_b):
    """score (B,) in points, float64."""
    P, _ = pooled_ref(h)
    u = (P.reshape(h.shape[0], -1) @ sc1_w.double() + sc1_b.double()).clamp_min(0)
    return ((u @ sc2_w.double().view(-1, 1)).squeeze(1) + sc2_b.double()) * h.shape[2]


def huber(e, delta):
    return torch.where(e.abs() <= delta, 0.5 * e * e, delta * (e.abs() - 0.5 * delta))


OutRef = namedtuple("OutRef", "s e loss abserr g du dout u")


def score_out_ref(upre, w2, b2, t=None, valid=None, weight=None, grad_scale=1.0, delta=1.0):
    """The output layer in float64: every output of ops.score_out."""
    up, w = upre.double(), w2.double().view(-1)
    u = up.clamp_min(0)
    s = u @ w + b2.double().view(-1)[0]
    if t is None:
        return OutRef(s, None, None, None, None, None, None, u)
    e = s - t.double()
    g = grad_scale * e.clamp(-delta, delta)
    if valid is not None:
        g = g * valid.double()
    if weight is not None:
        g = g * weight.double()
    du = torch.where(up > 0, g[:, None] * w[None, :], torch.zeros_like(up))
    dout = torch.cat([g[:, None] * u, g[:, None]], 1)
    return OutRef(s, e, huber(e, delta), e.abs(), g, du, dout, u)


def score_out_bounds(upre, w2, b2, ref, valid=None, weight=None, grad_scale=1.0, delta=1.0):
    """Bounds of the fp32 kernel's error against ``score_out_ref``, from the roundings it makes.

    s: a lane's chain has at most D / 64 <= 8 fused terms, the butterfly 6 adds and the bias 1: fewer than D + 2
    roundings of partial sums bounded by M = sum_j |u w2| + |b2|, so |s - exact| <= (D + 2) 2^-24 M =: sb.
    e = s - t is one more rounding: eb = sb + 2^-24 |e|.  abserr: eb.
    loss: Huber has slope clamp(e), so the error of e moves it by at most (min(|e|, delta) + eb) eb; its own
    evaluation is at most 4 roundings of terms bounded by delta |e| + e^2.
    g: the factor k = grad_scale * valid * weight (two roundings) times clamp(e) (slope <= 1) and one more
    rounding: gb = |k| eb + 3 * 2^-24 |g|.  du = g w2 and dout = g u add one rounding each."""
    D = upre.shape[1]
    M = (ref.u * w2.double().view(-1)).abs().sum(1) + b2.double().abs().view(-1)[0]
    sb = (D + 2) * U24 * M
    if ref.e is None:
        return dict(s=sb)
    eb = sb + U24 * ref.e.abs()
    lb = (ref.e.abs().clamp_max(delta) + eb) * eb + 4 * U24 * (delta * ref.e.abs() + ref.e ** 2)
    k = torch.full_like(ref.e, grad_scale)
    if valid is not None:
        k = k * valid.double()
    if weight is not None:
        k = k * weight.double()
    gb = k.abs() * eb + 3 * U24 * ref.g.abs()
    dub = gb[:, None] * w2.double().view(-1).abs()[None, :] + U24 * ref.du.abs()
    doutb = torch.cat([gb[:, None] * ref.u, gb[:, None]], 1) + U24 * ref.dout.abs()
    return dict(s=sb, e=eb, loss=lb, abserr=eb, g=gb, du=dub, dout=doutb)


def out_case(B, D, seed=0):
    """Seeded inputs of score_out: upre ~ N(0, 1), w2 ~ 0.3 N(0, 1), a target that puts about half the boards past
    the Huber threshold, a validity column with zeros and per-board weights with zeros."""
    g = torch.Generator().manual_seed(1000 * D + B + seed)
    upre = torch.randn(B, D, generator=g)
    w2 = torch.randn(D, generator=g) * 0.3
    b2 = torch.randn(1, generator=g) * 0.1
    t = torch.randn(B, generator=g) * 1.5
    valid = (torch.rand(B, generator=g) > 0.25).float()
    weight = torch.rand(B, generator=g) + 0.5
    if B >= 3:
        valid[1] = 0.0
        weight[2] = 0.0
        valid[0] = weight[0] = 1.0
    return upre, w2, b2, t, valid, weight


BackRef = namedtuple("BackRef", "score loss abserr d_sc1_w d_sc1_b d_sc2_w d_sc2_b dP dh")


def score_backward_ref(h, sc1_w, sc1_b, sc2_w, sc2_b, score_t, valid, weight=None, coef=1.0, delta=1.0, norm=None):
    """The analytic backward of L = coef / norm * sum_b valid_b w_b Huber_delta(s_b - score_t_b / S) in float64:
    the four parameter gradients, dP (B, 2, F) and dh (B, F, S, S), the mean part spread over the board with inv
    and the max part on the argmax pixel alone."""
    B, F, S, _ = h.shape
    norm = B if norm is None else norm
    P, am = pooled_ref(h)
    P2 = P.reshape(B, -1)
    w1, w2 = sc1_w.double(), sc2_w.double().view(-1)
    upre = P2 @ w1 + sc1_b.double()
    o = score_out_ref(upre, w2, sc2_b, score_t.double() / S, valid, weight, coef / norm, delta)
    dP = (o.du @ w1.t()).view(B, 2, F)
    dh = (dP[:, 0] * inv32(S))[:, :, None].expand(B, F, S * S).clone()
    dh.scatter_add_(2, am[:, :, None], dP[:, 1][:, :, None])
    v = valid.double()
    return BackRef(o.s * S, o.loss * v, o.abserr * v * S, P2.t() @ o.du, o.du.sum(0), o.dout[:, :-1].sum(0),
                   o.dout[:, -1].sum(0).view(1), dP, dh.view(B, F, S, S))


def dp_add_expected(dz, y, dp, argmax, S, dpass=None, pass_w=None):
    """ops.gpool_bwd_add_masked_dp's documented order as separately rounded float32 torch operations (the pass
    term's one fused multiply-add through float64), on the tensors' device: padded NHWC dz, y (B, S + 2, S + 2, C), dp (B, 2, C), argmax (B, C) -> the expected dz."""
    B, C, NP = y.shape[0], y.shape[3], S * S
    inv = torch.tensor(inv32(S), device=dz.device)
    q0 = dp[:, 0] * inv
    q01 = q0 + dp[:, 1]
    if dpass is not None:
        r0 = (dpass[:B, None] * pass_w[0][None, :]) * inv
        # the one fused multiply-add of the order: the product of two float32 is exact in float64
        r01 = (dpass[:B, None].double() * pass_w[1][None, :].double() + r0.double()).float()
        q0, q01 = r0 + q0, r01 + q01
    hit = torch.arange(NP, device=dz.device)[None, :, None] == argmax[:, None, :].long()
    add = torch.where(hit, q01[:, None, :], q0[:, None, :].expand(B, NP, C))
    old = dz[:, 1:S + 1, 1:S + 1].reshape(B, NP, C)
    yint = y[:, 1:S + 1, 1:S + 1].reshape(B, NP, C)
    new = torch.where((yint > 0) & (add != 0), (old.float() + add).bfloat16(), old)
    out = dz.clone()
    out[:, 1:S + 1, 1:S + 1] = new.view(B, S, S, C)
    return out
