"""The ownership-head kernels (head_own.hip) against float64 references (own_refs.py) and the kernels
they are modelled on, over head_refs.HEAD_SHAPES (both launch paths, padded channels, three board
sizes, the 8-channel case).
"""
import pytest
import torch

import head_refs as R
import own_refs as O

pytestmark = pytest.mark.gpu

GS = 1.0 / 48  # a grad_scale that is no power of two


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


_DEV = {}


def _dev(C, C_real, B, S, dev):
    """One case on the device (made once, never written) and its float64 reference (CPU)."""
    key = (C, C_real, B, S)
    if key not in _DEV:
        c = O.own_case(C, C_real, B, S)
        d = {k: getattr(c, k).to(dev) for k in ("y", "wv", "bv", "wo", "bo", "target", "sym", "valid", "weight")}
        d["yp"] = R.pad_nhwc(d["y"])
        ref = O.own_ref(c.y, c.wo, c.bo, c.target, c.sym, c.valid, c.weight, GS)
        _DEV[key] = (c, d, ref)
    return _DEV[key]


def _wide_path(C, B, S):
    """The 1024-thread BoardRegs path of policy_head_go's split."""
    return not (B >= 256 and S * (C // 8) <= 512)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _run(ops, dev, C, C_real, B, S, target="case", sym="case", valid="case", weight="case", gs=GS):
    c, d, _ = _dev(C, C_real, B, S, dev)
    SS = S * S
    pick = lambda v, name: d[name] if isinstance(v, str) else v
    target, sym, valid, weight = pick(target, "target"), pick(sym, "sym"), pick(valid, "valid"), pick(weight, "weight")
    out = dict(zv=_nan(dev, B, SS), own=_nan(dev, B, SS), olog=_nan(dev, B, SS))
    kw = {}
    if target is not None:
        out.update(oloss=_nan(dev, B), oagree=_nan(dev, B), dlo=_nan(dev, B, SS))
        kw = dict(target=target, sym=sym, valid=valid, weight=weight, oloss=out["oloss"], oagree=out["oagree"],
                  dlo=out["dlo"], grad_scale=gs)
    ops.value_own_head(d["yp"], d["wv"], d["bv"], d["wo"], d["bo"], out["zv"], S, own=out["own"], olog=out["olog"],
                       **kw)
    torch.cuda.synchronize()
    return out


# ----------------------------------------------------------------------- 1. forward logits
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_value_own_head_logits(ops, cuda_device, C, C_real, B, S):
    """zv and olog against float64 within head_refs.logits_bound; on the 1024-thread path (BoardRegs::dots
    = head_dots' order) both are bit-equal to head_logits."""
    c, d, ref = _dev(C, C_real, B, S, cuda_device)
    out = _run(ops, cuda_device, C, C_real, B, S)
    for name, w, b in (("zv", c.wv, c.bv), ("olog", c.wo, c.bo)):
        err = (out[name].double().cpu() - R.logits64(c.y, w, b)).abs()
        bound = R.logits_bound(c.y, w, b)
        print("%s max err / bound: %.3g" % (name, (err / bound.clamp_min(1e-300)).max().item()))
        assert bool((err <= bound).all())
    if _wide_path(C, B, S):
        for name, w, b in (("zv", "wv", "bv"), ("olog", "wo", "bo")):
            z = torch.full_like(out[name], float("nan"))
            ops.head_logits(d["yp"], d[w], d[b], z, S)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out[name]), _bits(z))


# -------------------------------------------------------------------------- 2. tanh output
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_value_own_head_tanh(ops, cuda_device, C, C_real, B, S):
    """own against float64 tanh of the kernel's own olog.  The device tanhf's largest error over the
    olog values of all nine cases was measured on an MI355X at own_refs.TANHF_MEASURED = 7.97e-8 (1.3 ulp
    of a value in [0.5, 1), at |olog| near 0.65); the bound is that times 4, own_refs.TANHF_BOUND =
    3.19e-7."""
    out = _run(ops, cuda_device, C, C_real, B, S)
    err = (out["own"].double() - torch.tanh(out["olog"].double())).abs().max().item()
    print("tanhf max err: %.3g (bound %.3g)" % (err, O.TANHF_BOUND))
    assert err <= O.TANHF_BOUND
    assert bool((out["own"].abs() <= 1).all())


# ------------------------------------------------------------------ 3. gradient and metrics
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_value_own_head_train_vs_fp64(ops, cuda_device, C, C_real, B, S):
    """dlo, oloss and oagree against float64.

    own: |own - tanh(exact logit)| <= TANHF_BOUND + logits_bound =: ob (tanh has slope <= 1).
    dlo = c_b f(own), f = (own - t)(1 - own^2), c_b = grad_scale k_b 2 / SS.  f' = 1 - 3 own^2 + 2 own t has
    magnitude at most 4 on |own|, |t| <= 1, so the error of own moves f by at most 4 ob; the fp32
    evaluation of f and c_b adds at most 16 * 2^-24 (own_refs.dlo_bound counts the roundings):
    |dlo - ref| <= |c_b| (4 ob + 16 * 2^-24).
    oloss: (own - t)^2 has slope <= 4 in own, the mean of S*S terms at most (S*S + 8) * 2^-24 of itself
    (own_refs.oloss_bound).
    oagree: exact, except at points where the float64 |own| is within ob of 0; those are counted and
    must be under 1 % of the case's points (test_own_refs.py checks the reference alone for that), and
    the count of a board may differ from the reference by at most the board's number of such points."""
    c, d, ref = _dev(C, C_real, B, S, cuda_device)
    out = _run(ops, cuda_device, C, C_real, B, S)
    ob = O.own_bound(c.y, c.wo, c.bo)
    err = (out["own"].double().cpu() - ref.own).abs()
    print("own max err / bound: %.3g" % (err / ob).max().item())
    assert bool((err <= ob).all())
    db = O.dlo_bound(ref, ob)
    derr = (out["dlo"].double().cpu() - ref.dlo).abs()
    live = ref.coef != 0
    print("dlo max err / bound: %.3g" % (derr[live] / db[live]).max().item())
    assert bool((derr <= db).all())
    lerr = (out["oloss"].double().cpu() - ref.loss).abs()
    lb = O.oloss_bound(ref, ob)
    print("oloss max err / bound: %.3g" % (lerr / lb).max().item())
    assert bool((lerr <= lb).all())
    near = O.near_zero_points(ref, ob)
    print("undecided points: %d of %d" % (int(near.sum()), near.numel()))
    assert int(near.sum()) < 0.01 * near.numel()
    assert bool(((out["oagree"].double().cpu() - ref.agree).abs() <= near.sum(1)).all())


# ------------------------------------------------------------------- 4. structure, bitwise
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_value_own_head_structure(ops, cuda_device, C, C_real, B, S):
    """valid = 0 or weight = 0 gives dlo rows of exact zeros (loss and agreement are still written);
    doubling weight doubles dlo exactly; a null valid / weight reads as 1; a null target writes own, zv
    and olog only; two calls give equal bits; NaN-filled outputs are fully overwritten."""
    dev = cuda_device
    c, d, ref = _dev(C, C_real, B, S, dev)
    out = _run(ops, dev, C, C_real, B, S)
    for v in out.values():
        assert bool(torch.isfinite(v).all())
    again = _run(ops, dev, C, C_real, B, S)
    for k in out:
        assert torch.equal(_bits(out[k]), _bits(again[k])), k
    dead = (d["valid"] == 0)
    assert int(dead.sum()) >= 1
    assert torch.equal(_bits(out["dlo"][dead]), torch.zeros_like(_bits(out["dlo"][dead])))
    assert bool((out["oloss"][dead] > 0).all())
    w0 = d["weight"].clone()
    w0[0] = 0.0
    z = _run(ops, dev, C, C_real, B, S, weight=w0)
    assert torch.equal(_bits(z["dlo"][0]), torch.zeros_like(_bits(z["dlo"][0])))
    assert torch.equal(_bits(z["dlo"][1:]), _bits(out["dlo"][1:]))
    dbl = _run(ops, dev, C, C_real, B, S, weight=d["weight"] * 2)
    assert torch.equal(_bits(dbl["dlo"]), _bits(out["dlo"] * 2))
    for k in ("oloss", "oagree", "own", "zv", "olog"):
        assert torch.equal(_bits(dbl[k]), _bits(out[k])), k
    ones = _run(ops, dev, C, C_real, B, S, valid=torch.ones_like(d["valid"]), weight=torch.ones_like(d["weight"]))
    null = _run(ops, dev, C, C_real, B, S, valid=None, weight=None)
    assert torch.equal(_bits(ones["dlo"]), _bits(null["dlo"]))
    fwd = _run(ops, dev, C, C_real, B, S, target=None)
    assert set(fwd) == {"zv", "own", "olog"}
    for k in fwd:
        assert torch.equal(_bits(fwd[k]), _bits(out[k])), k


@pytest.mark.parametrize("C,C_real,B,S", [(192, 192, 7, 19), (64, 64, 257, 9), (8, 8, 3, 9), (192, 192, 257, 13)])
@pytest.mark.parametrize("s", range(8))
def test_value_own_head_moves_the_target(ops, cuda_device, C, C_real, B, S, s):
    """(t, sym = s) equals the pre-moved target with sym = 0 (and with a null sym), bit for bit."""
    dev = cuda_device
    c, d, _ = _dev(C, C_real, B, S, dev)
    sym = torch.full((B,), s, dtype=torch.int32, device=dev)
    a = _run(ops, dev, C, C_real, B, S, sym=sym)
    pre = O.move_rows(d["target"], sym, S).contiguous()
    b0 = _run(ops, dev, C, C_real, B, S, target=pre, sym=torch.zeros_like(sym))
    bn = _run(ops, dev, C, C_real, B, S, target=pre, sym=None)
    for k in ("dlo", "oloss", "oagree"):
        assert torch.equal(_bits(a[k]), _bits(b0[k])), k
        assert torch.equal(_bits(a[k]), _bits(bn[k])), k
    if s in (1, 3):  # not an involution: the other direction gives another target
        assert not torch.equal(pre, O.move_rows(d["target"], torch.full_like(sym, 4 - s), S))


# ------------------------------------------------------------------- 5. head_backward_add2
def _add2_inputs(C, C_real, B, S, dev, integer):
    g = torch.Generator().manual_seed(3 * C + B + 11 * S + (1 if integer else 0))
    SS = S * S
    if integer:
        sign = lambda n: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
        w1 = torch.randint(1, 3, (C_real,), generator=g).float() * sign(C_real)
        w2 = torch.randint(1, 3, (C_real,), generator=g).float() * sign(C_real)
        g1 = torch.randint(-2, 3, (B, SS), generator=g).float()
        g2 = torch.randint(-2, 3, (B, SS), generator=g).float()
        dzi = torch.randint(-8, 9, (B, S, S, C), generator=g).to(torch.bfloat16)
    else:
        w1 = torch.randn(C_real, generator=g) * 0.05
        w2 = torch.randn(C_real, generator=g) * 0.05
        g1 = torch.randn(B, SS, generator=g)
        g2 = torch.randn(B, SS, generator=g)
        dzi = torch.randn(B, S, S, C, generator=g).to(torch.bfloat16)
    dzi[..., C_real:] = 0
    return w1, w2, g1, g2, dzi


def _check_untouched(dz, dz_in, y, C_real):
    out, inner = dz[:, 1:-1, 1:-1].contiguous(), dz_in[:, 1:-1, 1:-1].contiguous()
    keep = y <= 0
    assert torch.equal(out.view(torch.int16)[keep], inner.view(torch.int16)[keep])
    assert R.border_is_zero(dz)
    assert not bool((dz[..., C_real:] != 0).any())


@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_head_backward_add2_exact(ops, cuda_device, C, C_real, B, S):
    """Integer data (dz_in in [-8, 8], g1, g2 in [-2, 2], weights in {+-1, +-2}): every intermediate is an
    integer of magnitude <= 16, exact in fp32 and bf16, so dz is bit-equal to the torch expression and to
    two successive head_backward_add calls, whose dhead blocks it also reproduces."""
    dev = cuda_device
    c, d, _ = _dev(C, C_real, B, S, dev)
    w1, w2, g1, g2, dzi = [t.to(dev) for t in _add2_inputs(C, C_real, B, S, dev, True)]
    dz_in = R.pad_nhwc(dzi)
    dz = dz_in.clone()
    dh1, dh2 = _nan(dev, B, C_real + 1), _nan(dev, B, C_real + 1)
    ops.head_backward_add2(d["yp"], w1, g1, w2, g2, dz, dh1, dh2, S)
    torch.cuda.synchronize()
    y = d["y"]
    w1p, w2p = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    w1p[:C_real], w2p[:C_real] = w1, w2
    inner = dz_in[:, 1:-1, 1:-1]
    ref = torch.where(y > 0, (inner.float() + g1.view(B, S, S, 1) * w1p + g2.view(B, S, S, 1) * w2p).to(torch.bfloat16),
                      inner)
    assert torch.equal(dz[:, 1:-1, 1:-1].contiguous().view(torch.int16), ref.contiguous().view(torch.int16))
    two = dz_in.clone()
    e1, e2 = _nan(dev, B, C_real + 1), _nan(dev, B, C_real + 1)
    ops.head_backward_add(d["yp"], w1, g1, two, e1, S)
    ops.head_backward_add(d["yp"], w2, g2, two, e2, S)
    torch.cuda.synchronize()
    assert torch.equal(dz.view(torch.int16), two.view(torch.int16))
    assert torch.equal(_bits(dh1), _bits(e1)) and torch.equal(_bits(dh2), _bits(e2))
    _check_untouched(dz, dz_in, y, C_real)


@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_head_backward_add2_one_head(ops, cuda_device, C, C_real, B, S):
    """g2 = 0, random data: dz and dhead1 are bit-equal to head_backward_add; dhead2 is zero."""
    dev = cuda_device
    c, d, _ = _dev(C, C_real, B, S, dev)
    w1, w2, g1, g2, dzi = [t.to(dev) for t in _add2_inputs(C, C_real, B, S, dev, False)]
    dz_in = R.pad_nhwc(dzi)
    dz, one = dz_in.clone(), dz_in.clone()
    dh1, dh2, e1 = _nan(dev, B, C_real + 1), _nan(dev, B, C_real + 1), _nan(dev, B, C_real + 1)
    ops.head_backward_add2(d["yp"], w1, g1, w2, torch.zeros_like(g2), dz, dh1, dh2, S)
    ops.head_backward_add(d["yp"], w1, g1, one, e1, S)
    torch.cuda.synchronize()
    assert torch.equal(dz.view(torch.int16), one.view(torch.int16))
    assert torch.equal(_bits(dh1), _bits(e1))
    assert not bool((dh2 != 0).any())


@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_head_backward_add2_vs_fp64(ops, cuda_device, C, C_real, B, S):
    """Per element |dz - x| <= 2^-8 |x| + 2^-22 (|dz_in| + |g1 w1| + |g2 w2|), x the float64 value of
    dz_in + g1 w1 + g2 w2.  Derivation: the two fused multiply-adds round once each, by at most 2^-24 of a
    magnitude no larger than M = |dz_in| + |g1 w1| + |g2 w2| (times 1 + 2^-24 for the second), so the fp32
    value f has |f - x| <= 2^-22.9 M; the bf16 round-to-nearest of f is off by at most half an ulp,
    2^-8 |f| <= 2^-8 |x| + 2^-30 M, and the sum is below the stated bound.  Where y <= 0 dz keeps its bits.
    Both dhead blocks: test_head_backward_add_vs_fp64's bounds, (S*S + 2) * 2^-24 * sum_p |g y| per channel
    and the same form for the bias.  Two calls give equal bits."""
    dev = cuda_device
    c, d, _ = _dev(C, C_real, B, S, dev)
    w1, w2, g1, g2, dzi = _add2_inputs(C, C_real, B, S, dev, False)
    dz_in = R.pad_nhwc(dzi.to(dev))
    dz = dz_in.clone()
    dh1, dh2 = _nan(dev, B, C_real + 1), _nan(dev, B, C_real + 1)
    args = [t.to(dev) for t in (w1, g1, w2, g2)]
    ops.head_backward_add2(d["yp"], *args, dz, dh1, dh2, S)
    dzb = dz_in.clone()
    f1, f2 = _nan(dev, B, C_real + 1), _nan(dev, B, C_real + 1)
    ops.head_backward_add2(d["yp"], *args, dzb, f1, f2, S)
    torch.cuda.synchronize()
    assert torch.equal(dz.view(torch.int16), dzb.view(torch.int16))
    assert torch.equal(_bits(dh1), _bits(f1)) and torch.equal(_bits(dh2), _bits(f2))
    ref = O.backward_add2_ref(c.y, dzi, g1, w1, g2, w2)
    out = dz[:, 1:-1, 1:-1].double().cpu()
    live = c.y > 0
    err = (out - ref.x).abs()
    bound = 2.0 ** -8 * ref.x.abs() + 2.0 ** -22 * ref.mag
    print("dz max err / bound: %.3g" % (err[live] / bound[live].clamp_min(1e-300)).max().item())
    assert bool((err[live] <= bound[live]).all())
    _check_untouched(dz, dz_in, d["y"], C_real)
    SS = S * S
    for dh, rh, pabs, g in ((dh1, ref.dh1, ref.p1abs, g1), (dh2, ref.dh2, ref.p2abs, g2)):
        dh = dh.double().cpu()
        assert bool(((dh[:, :C_real] - rh[:, :C_real]).abs() <= (SS + 2) * R.U24 * pabs).all())
        assert bool(((dh[:, C_real] - rh[:, C_real]).abs() <= (SS + 2) * R.U24 * g.double().abs().sum(1)).all())


def test_head_backward_add2_refuses_e5m2(ops, cuda_device):
    C, C_real, B, S = 64, 64, 2, 9
    dev = cuda_device
    yp = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError, match="e5m2"):
        ops.head_backward_add2(yp, z(C_real), z(B, S * S), z(C_real), z(B, S * S), torch.zeros_like(yp),
                               z(B, C_real + 1), z(B, C_real + 1), S,
                               dz8=torch.zeros(yp.shape, dtype=torch.uint8, device=dev))


# --------------------------------------------------------------- 6. policy_value_own_head
@pytest.mark.parametrize("legal", [True, False])
@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_policy_value_own_head(ops, cuda_device, C, C_real, B, S, legal):
    """probs and zv are bit-equal to policy_value_head's, with a legal mask and without; own is bit-equal
    to value_own_head's on the 1024-thread path and within the ``own`` bound of float64 everywhere."""
    dev = cuda_device
    c, d, ref = _dev(C, C_real, B, S, dev)
    hc = R.head_case(C, C_real, B, S, "uniform")
    wp, bp = hc.w.to(dev), hc.b.to(dev)
    g = torch.Generator().manual_seed(17 * C + B + S)
    lg = (torch.rand(B, S * S, generator=g) > 1.0 / 3.0).to(torch.uint8)
    lg[:, 0] = 1
    lg = lg.to(dev) if legal else None
    SS = S * S
    probs, zv, own = _nan(dev, B, SS), _nan(dev, B, SS), _nan(dev, B, SS)
    ops.policy_value_own_head(d["yp"], wp, bp, d["wv"], d["bv"], d["wo"], d["bo"], probs, zv, own, S, legal=lg)
    p0, z0 = _nan(dev, B, SS), _nan(dev, B, SS)
    ops.policy_value_head(d["yp"], wp, bp, d["wv"], d["bv"], p0, z0, S, legal=lg)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p0).all())
    assert torch.equal(_bits(probs), _bits(p0)) and torch.equal(_bits(zv), _bits(z0))
    ob = O.own_bound(c.y, c.wo, c.bo)
    assert bool(((own.double().cpu() - ref.own).abs() <= ob).all())
    if _wide_path(C, B, S):
        assert torch.equal(_bits(own), _bits(_run(ops, dev, C, C_real, B, S, target=None)["own"]))


# ----------------------------------------------------------------------- 7. host checks
def test_own_head_ops_check_their_arguments(ops, cuda_device):
    """A host tensor, a wrong dtype or a wrong shape raises on the host, before any launch."""
    dev = cuda_device
    C, B, S = 64, 2, 9
    SS = S * S
    yp = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
    z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
    w, b = z(C), z(1)
    full = dict(own=z(B, SS), olog=z(B, SS), target=z(B, SS, dtype=torch.int8), oloss=z(B), oagree=z(B), dlo=z(B, SS))
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.value_own_head(yp, w, b, w.cpu(), b, z(B, SS), S)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S, **dict(full, target=full["target"].cpu()))
    with pytest.raises(RuntimeError, match="int8"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S, **dict(full, target=z(B, SS)))
    with pytest.raises(RuntimeError, match="int8"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S, **dict(full, target=z(B, SS + 1, dtype=torch.int8)))
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.value_own_head(yp.float(), w, b, w, b, z(B, SS), S)
    with pytest.raises(RuntimeError, match="zv must be"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS + 1), S)
    with pytest.raises(RuntimeError, match="pad 1"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S + 1)
    with pytest.raises(RuntimeError, match="same"):
        ops.value_own_head(yp, w, b, z(C - 8), b, z(B, SS), S)
    with pytest.raises(RuntimeError, match="needs oloss"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S, target=full["target"])
    with pytest.raises(RuntimeError, match="go with a target"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S, valid=z(B))
    with pytest.raises(RuntimeError, match="sym int32"):
        ops.value_own_head(yp, w, b, w, b, z(B, SS), S, sym=z(B, dtype=torch.int64), **full)
    dzt, dh = torch.zeros_like(yp), z(B, C + 1)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.head_backward_add2(yp, w, z(B, SS).cpu(), w, z(B, SS), dzt, dh, dh.clone(), S)
    with pytest.raises(RuntimeError, match="float32"):
        ops.head_backward_add2(yp, w, z(B, SS).double(), w, z(B, SS), dzt, dh, dh.clone(), S)
    with pytest.raises(RuntimeError, match="head_backward_add2: dz as y"):
        ops.head_backward_add2(yp, w, z(B, SS), w, z(B, SS - 1), dzt, dh, dh.clone(), S)
    with pytest.raises(RuntimeError, match="head_backward_add2: dz as y"):
        ops.head_backward_add2(yp, w, z(B, SS), w, z(B, SS), dzt, dh, z(B, C), S)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.policy_value_own_head(yp, w, b, w, b, w, b, z(B, SS), z(B, SS), z(B, SS).cpu(), S)
    with pytest.raises(RuntimeError, match="must be \\(B, S\\*S\\)"):
        ops.policy_value_own_head(yp, w, b, w, b, w, b, z(B, SS), z(B, SS), z(B, SS + 1), S)
    with pytest.raises(RuntimeError, match="float32"):
        ops.policy_value_own_head(yp, w, b, w, b, w.double(), b, z(B, SS), z(B, SS), z(B, SS), S)
    torch.cuda.synchronize()  # the device is still healthy
