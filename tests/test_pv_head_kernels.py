"""The dual network's two head kernels (head_pv.hip) against the kernels they are modelled on and
float64 references, over head_refs.HEAD_SHAPES (both launch paths, padded channels, three board
sizes, the 8-channel case).
"""
import pytest
import torch

import head_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


_DEV = {}


def _dev(C, C_real, B, S, dev):
    """One head case on the device (made once, never written): padded activations, interior, policy
    head (the case's w / b), a value head drawn from its own generator, a legal mask with about a
    third of the points masked."""
    key = (C, C_real, B, S)
    if key not in _DEV:
        c = R.head_case(C, C_real, B, S, "uniform")
        g = torch.Generator().manual_seed(31 * C + 5 * B + S)
        wv = torch.randn(C_real, generator=g) * 0.05
        bv = torch.randn(1, generator=g)
        legal = (torch.rand(B, S * S, generator=g) > 1.0 / 3.0).to(torch.uint8)
        legal[:, 0] = 1  # no board without a legal point
        y = c.y.to(dev)
        _DEV[key] = (R.pad_nhwc(y), y, c.w.to(dev), c.b.to(dev), wv.to(dev), bv.to(dev), legal.to(dev))
    return _DEV[key]


def _wide_path(C, B, S):
    """The 1024-thread BoardRegs path of policy_head_go's split."""
    return not (B >= 256 and S * (C // 8) <= 512)


def _bits(t):
    return t.view(torch.int32)


def _run_pv(ops, dev, C, C_real, B, S, legal):
    yp, y, wp, bp, wv, bv, lg = _dev(C, C_real, B, S, dev)
    probs = torch.full((B, S * S), float("nan"), device=dev)
    zv = torch.full((B, S * S), float("nan"), device=dev)
    ops.policy_value_head(yp, wp, bp, wv, bv, probs, zv, S, legal=lg if legal else None)
    torch.cuda.synchronize()
    return probs, zv


# ------------------------------------------------------------------------ 1. probs
@pytest.mark.parametrize("legal", [True, False])
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_pv_head_probs_equal_policy_head(ops, cuda_device, C, C_real, B, S, legal):
    """probs is bit-equal to policy_head_probs on the same (y, wp, bp, legal), with a mask over about
    a third of the points and with none."""
    yp, y, wp, bp, wv, bv, lg = _dev(C, C_real, B, S, cuda_device)
    probs, _ = _run_pv(ops, cuda_device, C, C_real, B, S, legal)
    ref = torch.full_like(probs, float("nan"))
    ops.policy_head_probs(yp, wp, bp, ref, S, legal=lg if legal else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(_bits(probs), _bits(ref))
    if legal:
        assert not bool((probs[lg == 0] != 0).any())


# --------------------------------------------------------------------------- 2. zv
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_pv_head_value_logits(ops, cuda_device, C, C_real, B, S):
    """zv against float64 within head_refs.logits_bound (test_head_logits_vs_fp64's bound); on the
    1024-thread path (BoardRegs::dots = head_dots' order) also bit-equal to head_logits."""
    yp, y, wp, bp, wv, bv, lg = _dev(C, C_real, B, S, cuda_device)
    _, zv = _run_pv(ops, cuda_device, C, C_real, B, S, True)
    err = (zv.double() - R.logits64(y, wv, bv)).abs()
    bound = R.logits_bound(y, wv, bv)
    print("zv max err / bound: %.3g" % (err / bound.clamp_min(1e-300)).max().item())
    assert bool((err <= bound).all())
    if _wide_path(C, B, S):
        z = torch.full_like(zv, float("nan"))
        ops.head_logits(yp, wv, bv, z, S)
        torch.cuda.synchronize()
        assert torch.equal(_bits(zv), _bits(z))


# ------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_pv_head_deterministic_and_overwrites(ops, cuda_device, C, C_real, B, S):
    """Two calls give equal bits; NaN-filled outputs are fully overwritten."""
    p1, z1 = _run_pv(ops, cuda_device, C, C_real, B, S, True)
    p2, z2 = _run_pv(ops, cuda_device, C, C_real, B, S, True)
    assert bool(torch.isfinite(p1).all()) and bool(torch.isfinite(z1).all())
    assert torch.equal(_bits(p1), _bits(p2)) and torch.equal(_bits(z1), _bits(z2))


# ----------------------------------------------------- 4. accumulating backward, exact
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_head_backward_add_exact(ops, cuda_device, C, C_real, B, S):
    """Integer data (dz_in in [-8, 8], dlogits in [-4, 4], w in {+-1, +-2}): every intermediate is an
    integer of magnitude <= 16, exact in fp32 and bf16, so dz is bit-equal to the torch expression.
    The border and the padded channels stay zero; where y <= 0, dz keeps dz_in's bits."""
    dev = cuda_device
    yp, y = _dev(C, C_real, B, S, dev)[:2]
    g = torch.Generator().manual_seed(C + 3 * B + S)
    SS = S * S
    w = (torch.randint(1, 3, (C_real,), generator=g).float() * (torch.randint(0, 2, (C_real,), generator=g) * 2 - 1)).to(dev)
    dl = torch.randint(-4, 5, (B, SS), generator=g).float().to(dev)
    dzi = torch.randint(-8, 9, (B, S, S, C), generator=g).to(torch.bfloat16)
    dzi[..., C_real:] = 0
    dz_in = R.pad_nhwc(dzi.to(dev))
    dz = dz_in.clone()
    dhead = torch.full((B, C_real + 1), float("nan"), device=dev)
    ops.head_backward_add(yp, w, dl, dz, dhead, S)
    torch.cuda.synchronize()
    wp = torch.zeros(C, device=dev)
    wp[:C_real] = w
    inner = dz_in[:, 1:-1, 1:-1]
    ref = torch.where(y > 0, (inner.float() + dl.view(B, S, S, 1) * wp).to(torch.bfloat16), inner)
    out = dz[:, 1:-1, 1:-1]
    assert torch.equal(out.contiguous().view(torch.int16), ref.contiguous().view(torch.int16))
    assert R.border_is_zero(dz)
    assert not bool((dz[..., C_real:] != 0).any())
    keep = y <= 0
    assert torch.equal(out.contiguous().view(torch.int16)[keep], inner.contiguous().view(torch.int16)[keep])
    assert bool(torch.isfinite(dhead).all())


# ---------------------------------------------------- 5. accumulating backward, random
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_head_backward_add_vs_fp64(ops, cuda_device, C, C_real, B, S):
    """Per element |dz - x| <= 2^-8 |x| + 2^-22 (|dz_in| + |dlogits w|), x the float64 value of
    dz_in + dlogits * w.  Derivation: the fp32 result f of the product and the sum takes at most two
    roundings, each at most 2^-24 of a magnitude no larger than |dz_in| + |dlogits w| (a fused
    multiply-add takes one), so |f - x| <= 2^-23 (|dz_in| + |dlogits w|).  The bf16 round-to-nearest
    of f (8 significand bits) is off by at most half an ulp, 2^-8 |f| <= 2^-8 |x| + 2^-31 (...), and
    2^-8 |x| + (2^-23 + 2^-31)(...) is below the stated bound.  Where y <= 0 dz keeps dz_in's bits.
    dhead: test_head_backward_vs_fp64's bounds, (S*S + 2) * 2^-24 * sum_p |dlogits y| per channel and
    the same form for the bias."""
    dev = cuda_device
    yp, y, _, _, wv, _, _ = _dev(C, C_real, B, S, dev)
    g = torch.Generator().manual_seed(2 * C + B + 7 * S)
    SS = S * S
    dl = torch.randn(B, SS, generator=g).to(dev)
    dzi = torch.randn(B, S, S, C, generator=g).to(torch.bfloat16)
    dzi[..., C_real:] = 0
    dz_in = R.pad_nhwc(dzi.to(dev))
    dz = dz_in.clone()
    dhead = torch.full((B, C_real + 1), float("nan"), device=dev)
    ops.head_backward_add(yp, wv, dl, dz, dhead, S)
    torch.cuda.synchronize()
    wp = torch.zeros(C, device=dev, dtype=torch.float64)
    wp[:C_real] = wv.double()
    inner = dz_in[:, 1:-1, 1:-1]
    add = dl.double().view(B, S, S, 1) * wp
    x = inner.double() + add
    out = dz[:, 1:-1, 1:-1]
    live = y > 0
    err = (out.double() - x).abs()
    bound = 2.0 ** -8 * x.abs() + 2.0 ** -22 * (inner.double().abs() + add.abs())
    print("dz max err / bound: %.3g" % (err[live] / bound[live].clamp_min(1e-300)).max().item())
    assert bool((err[live] <= bound[live]).all())
    assert torch.equal(out.contiguous().view(torch.int16)[~live], inner.contiguous().view(torch.int16)[~live])
    assert R.border_is_zero(dz)
    assert not bool((dz[..., C_real:] != 0).any())
    y2 = y.double().flatten(1, 2)[..., :C_real]
    prod = dl.double().unsqueeze(2) * y2
    errw = (dhead[:, :C_real].double() - prod.sum(1)).abs()
    assert bool((errw <= (SS + 2) * R.U24 * prod.abs().sum(1)).all())
    errb = (dhead[:, C_real].double() - dl.double().sum(1)).abs()
    assert bool((errb <= (SS + 2) * R.U24 * dl.double().abs().sum(1)).all())


def test_head_backward_add_refuses_e5m2(ops, cuda_device):
    C, C_real, B, S = 64, 64, 2, 9
    dev = cuda_device
    yp = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="e5m2"):
        ops.head_backward_add(yp, torch.zeros(C_real, device=dev), torch.zeros(B, S * S, device=dev),
                              torch.zeros_like(yp), torch.zeros(B, C_real + 1, device=dev), S,
                              dz8=torch.zeros(yp.shape, dtype=torch.uint8, device=dev))


# ------------------------------------------------------- 6. head_backward keeps its bits
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_head_backward_default_bits(ops, cuda_device, C, C_real, B, S):
    """The overwriting head_backward is untouched by the accumulating op: its dz is still bit-equal to
    test_head_backward_vs_fp64's reference expression, whatever dz held before."""
    dev = cuda_device
    yp, y, w = _dev(C, C_real, B, S, dev)[:3]
    SS = S * S
    dl = torch.randn(B, SS, generator=torch.Generator().manual_seed(C + B + S)).to(dev)
    dz = torch.zeros_like(yp)
    dz[:, 1:-1, 1:-1, :C_real] = 3.0  # overwritten, not added to
    dhead = torch.full((B, C_real + 1), float("nan"), device=dev)
    ops.head_backward(yp, w, dl, dz, dhead, S)
    torch.cuda.synchronize()
    wp = torch.zeros(C, device=dev)
    wp[:C_real] = w
    ref = torch.where(y > 0, (dl.view(B, S, S, 1) * wp).to(torch.bfloat16), torch.zeros_like(y))
    assert torch.equal(dz[:, 1:-1, 1:-1] + 0.0, ref + 0.0)
    assert R.border_is_zero(dz)
