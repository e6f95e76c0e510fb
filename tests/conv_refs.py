"""Integer-valued operands and fp64 oracles for the convolution kernels (forward, dgrad, wgrad, their
fp8 forms, the split-K finish and the wgrad reduce), and the one Python statement of the ReLU' bitmask
layout.

Every conv kernel multiplies bf16 / fp8 operands exactly and accumulates in fp32.  With small-integer
operands every partial sum is an integer below 2^24, so the result does not depend on tiling, K order,
split count or reduce order and must equal the fp64 reference bit for bit: the GPU tests
(tests/test_conv_exact.py) compare with ``torch.equal`` only.  Everything here runs on the CPU from
seeded generators; tests/test_conv_refs.py proves the value ranges for every committed case.

Layouts: operands and oracles are NHWC over the unpadded board, ``(B, S, S, C_padded)``, the padded
channels zero; ``place`` puts one into a zero- or sentinel-bordered padded buffer.
"""
import functools

import torch
import torch.nn.functional as F

# (S, B, Cin_p, Cout_p, K, Pin): padded channel counts; real counts from ``real_channels``
CASES = [
    (19, 1, 192, 192, 3, 1),   # M = 361, below every large tile: one partial tile
    (19, 3, 192, 192, 3, 1),   # M = 1083: partial last tile at 32, 64, 128, 256 and 384; tiles start mid-row
    (9, 5, 192, 192, 3, 1),    # M = 405: a tile spans five boards
    (13, 3, 128, 128, 3, 1),   # the 128-wide N tile
    (19, 2, 64, 64, 3, 1),     # the 64-wide N tile
    (19, 2, 64, 192, 5, 2),    # first-layer geometry, 48 real planes
    (19, 2, 192, 384, 3, 1),   # blockIdx.y = 1, 16 mask words per pixel
    (13, 3, 128, 192, 3, 2),   # input pad larger than the tap radius
    (19, 2, 160, 160, 3, 1),   # value width (152 real in 160), straddled K-steps
    (19, 2, 64, 160, 5, 2),    # value width, 5x5 first layer (49 real planes)
]
# impulse geometries: a 3x3 and a 5x5 layer (tap placement and the dgrad flip)
IMPULSE_CASES = [(19, 2, 64, 64, 3, 1), (19, 2, 64, 192, 5, 2)]
# dgrad runs the transposed layer (Cout_p channels in, Cin_p out); conv_fwd has no 160 -> 64 shape, so the
# value net's first layer (which needs no dgrad) is not in the list
DGRAD_CASES = [c for c in CASES if not (c[3] == 160 and c[2] != 160)]
# fp8 kernels: the policy and value trunk widths and the value net's first layer
FP8_FWD_CASES = [(19, 3, 192, 192, 3, 1), (19, 2, 160, 160, 3, 1), (19, 2, 64, 160, 5, 2), (9, 5, 192, 192, 3, 1),
                 (9, 5, 160, 160, 3, 1)]
FP8_SQUARE_CASES = [(19, 3, 192, 192, 3, 1), (19, 2, 160, 160, 3, 1), (9, 5, 192, 192, 3, 1), (9, 5, 160, 160, 3, 1)]
ALL_CASES = CASES + [c for c in FP8_FWD_CASES + FP8_SQUARE_CASES if c not in CASES]

MAX_ABS = 256          # |pre-activation| and |dx| bound: integers up to 256 are exact in bf16
MAX_WGRAD = 1 << 24    # every wgrad sum is an exact fp32 integer below this
BF16_SENTINEL = 7.0    # what output buffers hold before a kernel runs (as tests/test_conv_halo384.py)
MBITS_SENTINEL = -1


def case_id(case):
    return "S%d-B%d-%dto%d-K%d-P%d" % tuple(case)


def real_channels(case):
    """(cin_real, cout_real) of a case: 48 real planes of 64 in front of a 5x5 policy layer, 49 in front
    of a 5x5 value layer, 152 real channels in every 160-wide tensor."""
    S, B, Cin, Cout, K, Pin = case
    cout_real = 152 if Cout == 160 else Cout
    if Cin == 64 and K == 5:
        cin_real = 49 if Cout == 160 else 48
    else:
        cin_real = 152 if Cin == 160 else Cin
    return cin_real, cout_real


def n_tile(cout_p):
    """Output-channel tile of the conv kernels (ops.conv_n_tile)."""
    return 160 if cout_p == 160 else 192 if cout_p % 192 == 0 else 128 if cout_p % 128 == 0 else 64


def mbits_words(cout_p):
    return cout_p // n_tile(cout_p) * 8


# ----------------------------------------------------------------------------- draws
def _gen(case, salt):
    S, B, Cin, Cout, K, Pin = case
    return torch.Generator(device="cpu").manual_seed(((S * 131 + B) * 1009 + Cin * 7 + Cout) * 100 + K * 10 + salt)


def _ternary(shape, g):
    return torch.randint(-1, 2, shape, generator=g).double()


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _pad_last(t, C):
    return F.pad(t, (0, C - t.shape[-1]))


def nhwc(t_nchw, C):
    """NCHW -> NHWC with the channels zero-padded to C."""
    return _pad_last(t_nchw.permute(0, 2, 3, 1), C).contiguous()


def place(t_nhwc, P, dtype, fill=0.0):
    """(B, S, S, C) into a padded (B, S + 2P, S + 2P, C) buffer of ``dtype`` whose border holds ``fill``."""
    B, S, _, C = t_nhwc.shape
    out = torch.full((B, S + 2 * P, S + 2 * P, C), fill, dtype=dtype)
    out[:, P:P + S, P:P + S] = t_nhwc.to(dtype)
    return out


def interior(t_padded, P, S):
    return t_padded[:, P:P + S, P:P + S]


def border_mask(B, S, P, C):
    m = torch.ones(B, S + 2 * P, S + 2 * P, C, dtype=torch.bool)
    m[:, P:P + S, P:P + S] = False
    return m


# ----------------------------------------------------------------------------- conditions
def _check_range(name, t, bound=MAX_ABS):
    m = t.abs().max().item()
    assert m <= bound, "%s: max |value| %g exceeds %g" % (name, m, bound)
    assert torch.equal(t, t.round()), "%s: not integer-valued" % name


def _check_share(name, pre):
    share = (pre > 0).double().mean().item()
    assert 0.3 <= share <= 0.7, "%s: positive share %.3f outside [0.3, 0.7]" % (name, share)


# ----------------------------------------------------------------------------- forward / dgrad oracles
def _fwd_from(case, x, w, b, check_share=True):
    S, B, Cin, Cout, K, Pin = case
    pre = F.conv2d(x, w, b, padding=K // 2)
    _check_range("pre-activation " + case_id(case), pre)
    if check_share:
        _check_share("pre-activation " + case_id(case), pre)
    y = pre.clamp_min(0)
    y_bf = y.to(torch.bfloat16)
    assert torch.equal(y_bf.double(), y)  # the bf16 store of the integer is exact
    return {
        "case": case, "x": nhwc(x, Cin), "w": w, "bias": _pad_last(b, Cout).float(),
        "pre": nhwc(pre, Cout), "y": nhwc(y_bf, Cout), "mask": nhwc(y > 0, Cout),
    }


@functools.lru_cache(maxsize=None)
def fwd_case(case):
    """Ternary activations and weights, integer bias in [-8, 8]; pre = conv2d, y = bf16(relu(pre)).
    Returns NHWC tensors padded to the case's channel counts: x (fp64), w (OIHW real, fp64), bias (fp32,
    padded), pre (fp64), y (bf16), mask (bool, y > 0)."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    g = _gen(case, 1)
    x = _ternary((B, ci, S, S), g)
    w = _ternary((co, ci, K, K), g)
    b = _ints((co,), -8, 8, g)
    return _fwd_from(case, x, w, b)


def _dgrad_from(case, dz, w, mask, check_share=True):
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    raw = torch.nn.grad.conv2d_input((B, ci, S, S), w, dz, padding=K // 2)
    _check_range("dx " + case_id(case), raw)
    if check_share:
        share = mask.double().mean().item()
        assert 0.3 <= share <= 0.7
    dx = torch.where(mask, raw, torch.zeros_like(raw))  # +0 where masked, as the kernels store it
    return {
        "case": case, "dz": nhwc(dz, Cout), "w": w, "mask": nhwc(mask, Cin), "dx": nhwc(dx, Cin),
        "raw": nhwc(raw, Cin),
    }


@functools.lru_cache(maxsize=None)
def dgrad_case(case):
    """The layer's dgrad: ternary dz (B, S, S, Cout_p) and weights, a random ReLU' mask over the real
    input channels; dx = conv2d_input(dz, w) * mask, (B, S, S, Cin_p).  The kernel sees the transposed
    layer: Cout_p channels in, Cin_p out."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    g = _gen(case, 2)
    dz = _ternary((B, co, S, S), g)
    w = _ternary((co, ci, K, K), g)
    mask = torch.randint(0, 2, (B, ci, S, S), generator=g).bool()
    return _dgrad_from(case, dz, w, mask)


def mask_activation(mask_nhwc, seed=0):
    """A bf16 activation whose ``> 0`` is ``mask``: positive values of several magnitudes where the mask
    is set, and a mix of negative values, +0.0 and -0.0 where it is not."""
    g = torch.Generator(device="cpu").manual_seed(977 + seed)
    pos = torch.tensor([0.0078125, 0.5, 1.0, 3.0, 200.0])[torch.randint(0, 5, mask_nhwc.shape, generator=g)]
    neg = torch.tensor([-0.0078125, -1.0, -300.0, 0.0, -0.0])[torch.randint(0, 5, mask_nhwc.shape, generator=g)]
    a = torch.where(mask_nhwc, pos, neg).to(torch.bfloat16)
    assert torch.equal(a > 0, mask_nhwc)
    return a


def _impulse_points(S):
    return [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (S // 2, S // 2)]


@functools.lru_cache(maxsize=None)
def impulse_fwd_case(case):
    """Unit impulses at the four corners and the centre of the first and last board, in channels 0 and
    cin_real - 1; w[n, c, kh, kw] = 1 + kh K + kw; zero bias.  Every output is a single weight (or 0):
    a misplaced or mirrored tap changes it."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    x = torch.zeros(B, ci, S, S, dtype=torch.float64)
    for b in (0, B - 1):
        for c in (0, ci - 1):
            for i, j in _impulse_points(S):
                x[b, c, i, j] = 1.0
    w = (1 + torch.arange(K * K, dtype=torch.float64)).view(1, 1, K, K).expand(co, ci, K, K).contiguous()
    return _fwd_from(case, x, w, torch.zeros(co, dtype=torch.float64), check_share=False)


@functools.lru_cache(maxsize=None)
def impulse_dgrad_case(case):
    """The impulses as dz (channels 0 and cout_real - 1) through the same asymmetric weights, all-ones
    mask: dx shows the flipped taps."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    dz = torch.zeros(B, co, S, S, dtype=torch.float64)
    for b in (0, B - 1):
        for n in (0, co - 1):
            for i, j in _impulse_points(S):
                dz[b, n, i, j] = 1.0
    w = (1 + torch.arange(K * K, dtype=torch.float64)).view(1, 1, K, K).expand(co, ci, K, K).contiguous()
    mask = torch.ones(B, ci, S, S, dtype=torch.bool)
    return _dgrad_from(case, dz, w, mask, check_share=False)


# ----------------------------------------------------------------------------- wgrad oracle
@functools.lru_cache(maxsize=None)
def wgrad_case(case):
    """Integer operands in [-4, 4] (exact in bf16, e4m3 and e5m2): x (B, S, S, Cin_p), dz (B, S, S, Cout_p),
    dW = conv2d_weight (cout_real, cin_real, K, K), db = dz.sum over pixels (cout_real)."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    g = _gen(case, 3)
    x = _ints((B, ci, S, S), -4, 4, g)
    dz = _ints((B, co, S, S), -4, 4, g)
    dw = torch.nn.grad.conv2d_weight(x, (co, ci, K, K), dz, padding=K // 2)
    db = dz.sum(dim=(0, 2, 3))
    # every partial sum is bounded by the sum of the products' magnitudes
    bound = float(B * S * S * 16)
    assert bound < MAX_WGRAD
    _check_range("dW " + case_id(case), dw, MAX_WGRAD - 1)
    _check_range("db " + case_id(case), db, MAX_WGRAD - 1)
    return {"case": case, "x": nhwc(x, Cin), "dz": nhwc(dz, Cout), "dw": dw, "db": db}


def wgrad_g0(case, what):
    """An integer-valued starting gradient in [-64, 64] for the scale / beta checks."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = real_channels(case)
    g = _gen(case, 4 if what == "w" else 5)
    return _ints((co, ci, K, K) if what == "w" else (co,), -64, 64, g)


def combine(g0, d, scale, beta):
    """beta * g0 + scale * d in fp64, asserted exact in fp32 (powers of two times integers)."""
    out = beta * g0 + scale * d
    assert torch.equal(out.float().double(), out)
    return out.float()


# ----------------------------------------------------------------------------- ReLU' bitmask layout
def _bit_position(cout_p):
    """(word, bit) of every output channel, from the layout comment at ConvEpilogue (conv_common.h):
    per padded pixel (Cout / BN) * 8 words; a workgroup column ``by`` covers BN channels, its wave half
    ``wn`` BN / 2 of them; lane group q = lane / 16 owns channels nbase + 16 i + r (r < 4) with
    nbase = by BN + wn BN / 2 + 4 q, and channel nbase + 16 i + r is bit 4 i + r of word by 8 + wn 4 + q.
    BN = 192: 24 bits per word; 160: 20; 128: 16; 64: 8."""
    bn = n_tile(cout_p)
    c = torch.arange(cout_p)
    by, cl = c // bn, c % bn
    wn, cw = cl // (bn // 2), cl % (bn // 2)
    i, q, r = cw // 16, (cw % 16) // 4, cw % 4
    return by * 8 + wn * 4 + q, 4 * i + r


def encode_mbits(mask, cout_p):
    """bool (B, S, S, cout_p) -> int32 words (B, S + 2, S + 2, words) over the padded pixel grid (border
    pixels: zero words)."""
    assert mask.dtype == torch.bool and mask.shape[-1] == cout_p
    B, S = mask.shape[0], mask.shape[1]
    word, bit = _bit_position(cout_p)
    words = torch.zeros(B, S, S, mbits_words(cout_p), dtype=torch.int64)
    words.index_add_(3, word, mask.long() << bit)
    out = torch.zeros(B, S + 2, S + 2, mbits_words(cout_p), dtype=torch.int32)
    out[:, 1:S + 1, 1:S + 1] = words.to(torch.int32)  # at most 24 bits per word: no wrap
    return out


def decode_mbits(words, cout_p):
    """int32 words over the padded grid, (B, S + 2, S + 2, words) or flat -> bool (B, S, S, cout_p) of the
    interior pixels; inverse of ``encode_mbits``."""
    assert words.dtype == torch.int32 and words.dim() == 4 and words.shape[-1] == mbits_words(cout_p)
    S = words.shape[1] - 2
    word, bit = (t.to(words.device) for t in _bit_position(cout_p))
    inner = words[:, 1:S + 1, 1:S + 1].long() & 0xFFFFFFFF
    return ((inner[..., word] >> bit) & 1).bool()


def mbits_unused(cout_p):
    """int32 per word slot: the bits no channel owns (a producer leaves them 0)."""
    word, bit = _bit_position(cout_p)
    used = torch.zeros(mbits_words(cout_p), dtype=torch.int64)
    used.index_add_(0, word, torch.ones_like(word) << bit)
    return (~used) & 0xFFFFFFFF


# ----------------------------------------------------------------------------- expected weight packs
def expected_pack(w, cin_p, cout_p):
    """What ops.pack_weights writes for OIHW ``w``: wf (K*K, cout_p, cin_p) with wf[t][n][c] =
    bf16(w[n][c][kh][kw]), t = kh K + kw, and wd (K*K, cin_p, cout_p) with wd[tf][c][n] the same value at
    the flipped tap tf = (K-1-kh) K + (K-1-kw); zeros in every padded row and column."""
    co, ci, K, _ = w.shape
    wf = torch.zeros(K * K, cout_p, cin_p, dtype=torch.bfloat16)
    wd = torch.zeros(K * K, cin_p, cout_p, dtype=torch.bfloat16)
    wb = w.to(torch.bfloat16)
    for kh in range(K):
        for kw in range(K):
            t, tf = kh * K + kw, (K - 1 - kh) * K + (K - 1 - kw)
            wf[t, :co, :ci] = wb[:, :, kh, kw]
            wd[tf, :ci, :co] = wb[:, :, kh, kw].t()
    return wf, wd


def packed(w, cin_p, cout_p, transposed=False):
    """The pack a conv kernel reads, built on the CPU from ``expected_pack`` with the extra all-zero tap
    of ops.packed_weight_like where the reduction width is an odd multiple of 32."""
    wf, wd = expected_pack(w, cin_p, cout_p)
    p = wd if transposed else wf
    red = cout_p if transposed else cin_p
    if red % 64 == 32:
        p = torch.cat([p, torch.zeros_like(p[:1])])
    return p.contiguous()


# ----------------------------------------------------------------------------- naive references
def naive_conv2d(x, w, b, pad):
    """Nested-loop cross-correlation, NCHW fp64: y[b,n,i,j] = bias[n] + sum x[b,c,i+kh-pad,j+kw-pad] w[n,c,kh,kw]."""
    B, C, H, W = x.shape
    N, _, K, K2 = w.shape
    y = torch.zeros(B, N, H, W, dtype=torch.float64)
    for bb in range(B):
        for n in range(N):
            for i in range(H):
                for j in range(W):
                    s = float(b[n]) if b is not None else 0.0
                    for c in range(C):
                        for kh in range(K):
                            for kw in range(K2):
                                ii, jj = i + kh - pad, j + kw - pad
                                if 0 <= ii < H and 0 <= jj < W:
                                    s += float(x[bb, c, ii, jj]) * float(w[n, c, kh, kw])
                    y[bb, n, i, j] = s
    return y


def naive_dgrad(dz, w, pad):
    """dx[b,c,i,j] = sum dz[b,n,i-kh+pad,j-kw+pad] w[n,c,kh,kw]."""
    B, N, H, W = dz.shape
    _, C, K, K2 = w.shape
    dx = torch.zeros(B, C, H, W, dtype=torch.float64)
    for bb in range(B):
        for c in range(C):
            for i in range(H):
                for j in range(W):
                    s = 0.0
                    for n in range(N):
                        for kh in range(K):
                            for kw in range(K2):
                                ii, jj = i - kh + pad, j - kw + pad
                                if 0 <= ii < H and 0 <= jj < W:
                                    s += float(dz[bb, n, ii, jj]) * float(w[n, c, kh, kw])
                    dx[bb, c, i, j] = s
    return dx


def naive_wgrad(x, dz, K, pad):
    """dW[n,c,kh,kw] = sum dz[b,n,i,j] x[b,c,i+kh-pad,j+kw-pad]."""
    B, C, H, W = x.shape
    N = dz.shape[1]
    dw = torch.zeros(N, C, K, K, dtype=torch.float64)
    for n in range(N):
        for c in range(C):
            for kh in range(K):
                for kw in range(K):
                    s = 0.0
                    for bb in range(B):
                        for i in range(H):
                            for j in range(W):
                                ii, jj = i + kh - pad, j + kw - pad
                                if 0 <= ii < H and 0 <= jj < W:
                                    s += float(dz[bb, n, i, j]) * float(x[bb, c, ii, jj])
                    dw[n, c, kh, kw] = s
    return dw


# ----------------------------------------------------------------------------- the comparison
def check_padded(got, want_nhwc, P, sentinel):
    """The comparison the GPU tests make for every padded output: the interior equals the oracle bit for
    bit and all four borders still hold the sentinel.  Returns a list of the failed parts (empty = pass)."""
    B, S = want_nhwc.shape[0], want_nhwc.shape[1]
    bad = []
    if not torch.equal(interior(got, P, S), want_nhwc.to(device=got.device, dtype=got.dtype)):
        bad.append("interior")
    bm = border_mask(B, S, P, got.shape[3]).to(got.device)
    if not (got[bm] == sentinel).all():
        bad.append("border")
    return bad


def check_mbits(words, mask_nhwc, cout_p):
    """The producers' bitmask check: decoded interior bits equal the mask with no exceptions, bits no
    channel owns are 0, border words still hold the sentinel."""
    B, S = mask_nhwc.shape[0], mask_nhwc.shape[1]
    w4 = words.view(B, S + 2, S + 2, mbits_words(cout_p))
    bad = []
    if not torch.equal(decode_mbits(w4, cout_p), mask_nhwc.to(w4.device)):
        bad.append("bits")
    if ((interior(w4, 1, S).long() & mbits_unused(cout_p).to(w4.device)) != 0).any():
        bad.append("unused bits")
    if not (w4[border_mask(B, S, 1, w4.shape[3]).to(w4.device)] == MBITS_SENTINEL).all():
        bad.append("border words")
    return bad
