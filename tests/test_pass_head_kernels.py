"""The pass-head kernels (the PASS variants in head_soft.hip / head_own.hip and gpool_bwd_add_masked in gpool.hip)
against the float64 reference of pass_head_refs.py, against the kernels they extend, and exactly on integer data.

policy_head_soft_pass holds the tolerances of tests/test_policy_head_soft.py (loss rtol 1e-3 / atol 1e-4; dz max
error under 1e-2 of the reference max; dhead weight part under 1e-3 of the reference max, per board and summed;
bias part 1e-4; ``correct`` equal; the dz border and the padded channels exactly 0).  The pass_w partial gets the
weight tolerance, dpass and the bias partial the bias tolerance.  ``pooled`` is the output of gpool_fwd on the
same activations, as in the trainer.  Probabilities are held to the family's 1e-5 (test_head_kernels.py, to
which test_pv_head_kernels.py pins policy_value_head bit for bit).
"""
import os
import subprocess
import sys

import pytest
import torch

import head_refs as R
import pass_head_refs as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


_DEV = {}


def _dev(ops, C, C_real, B, S, dev):
    """One head case on the device, made once and written by no test: padded activations, interior, the 1x1
    head, per-board weights, gpool_fwd's pooled rows and argmax, and the pass weights (flat and padded)."""
    key = (C, C_real, B, S)
    if key not in _DEV:
        c = R.head_case(C, C_real, B, S, "uniform")
        y = c.y.to(dev)
        yp = R.pad_nhwc(y)
        P = torch.full((B, 2, C), float("nan"), device=dev)
        a = torch.full((B, C), -7, dtype=torch.int32, device=dev)
        ops.gpool_fwd(yp, P, a, S)
        pw = PR.pass_weights(C_real)
        _DEV[key] = (c, yp, c.w.to(dev), c.b.to(dev), c.weight.to(dev), P, a, pw, PR.padded_pass_w(pw, C).to(dev))
    return _DEV[key]


def _max_err(a, ref):
    return (a.double().cpu() - ref.double().cpu()).abs().max().item()


def _outputs(yp, B, Cr):
    """NaN-filled outputs; the dz border, which no head kernel writes, is zero as in the trainers."""
    dev = yp.device
    nan = float("nan")
    dz = torch.zeros_like(yp)
    dz[:, 1:-1, 1:-1] = nan
    return dict(dz=dz, loss=torch.full((B,), nan, device=dev), correct=torch.full((B,), nan, device=dev),
                dhead=torch.full((B, Cr + 1), nan, device=dev), dpass=torch.full((B,), nan, device=dev),
                dpw=torch.full((B, 2 * Cr + 1), nan, device=dev))


def _run(ops, case, td, S, gs, pass_b, weight=None, sym=None, pass_w=None):
    c, yp, w, b, wt, P, a, pw, pwp = case
    o = _outputs(yp, yp.shape[0], w.numel())
    pb = torch.tensor([pass_b], device=yp.device)
    ops.policy_head_soft_pass(yp, w, b, P, pwp if pass_w is None else pass_w, pb, td, o["dz"], o["loss"], o["correct"],
                              o["dhead"], o["dpass"], o["dpw"], S, gs, weight=weight, sym=sym)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("pass_b", [0.0, PR.PASS_B_HIGH])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("with_sym", [False, True])
@pytest.mark.parametrize("C,C_real,B,S", PR.PASS_SHAPES)
def test_policy_head_soft_pass_vs_fp64(ops, cuda_device, C, C_real, B, S, with_sym, weighted, pass_b):
    case = _dev(ops, C, C_real, B, S, cuda_device)
    c, yp, w, b, wt, P, a, pw, pwp = case
    td, sym, kind = PR.pass_targets(C, C_real, B, S, with_sym)
    gs = 1.0 / B
    o = _run(ops, case, td.to(cuda_device), S, gs, pass_b, weight=wt if weighted else None,
             sym=None if sym is None else sym.to(cuda_device))
    ref = PR.pass_head_ref(c.y, c.w, c.b, pw, pass_b, td, sym, c.weight if weighted else None, gs)
    # the reference's argmax margin first: fp32 cannot reorder the logits, the pass logit included
    bound = torch.cat([R.logits_bound(c.y, c.w, c.b), PR.pass_logit_bound(c.y, pw, pass_b)[:, None]], 1)
    assert R.argmax_is_decided(ref.logits, bound)
    on_pass = R.first_argmax(ref.logits) == S * S
    # the high bias puts every board's argmax on the pass; at 0 only head_case's two dead boards (all board logits
    # equal to the bias) may have it there
    assert bool(on_pass.all()) if pass_b else not bool(on_pass[2:].any())
    qs = ref.q[ref.has].sort(1, descending=True).values
    assert bool((qs[:, 0] - qs[:, 1] > 1e-3).all())
    # test_policy_head_soft.py's comparisons
    Cr = C_real
    for v in o.values():
        assert bool(torch.isfinite(v.float()).all())
    print("loss max err %.3g" % _max_err(o["loss"], ref.loss))
    assert torch.allclose(o["loss"].double().cpu(), ref.loss, rtol=1e-3, atol=1e-4)
    assert torch.equal(o["correct"].double().cpu(), ref.correct)
    dzi = o["dz"][:, 1:-1, 1:-1]
    dzmax = max(ref.dz.abs().max().item(), 1e-6)
    print("dz max err / ref max %.3g" % (_max_err(dzi, ref.dz) / dzmax))
    assert _max_err(dzi, ref.dz) < 1e-2 * dzmax
    assert R.border_is_zero(o["dz"]) and not bool((dzi[..., Cr:] != 0).any())
    for name, got, want, n in (("dhead", o["dhead"], ref.dhead, Cr), ("dpw", o["dpw"], ref.dpw, 2 * Cr)):
        wmax = max(want[:, :n].abs().max().item(), 1e-6)
        print("%s weight part max err / ref max %.3g" % (name, _max_err(got[:, :n], want[:, :n]) / wmax))
        assert _max_err(got[:, :n], want[:, :n]) < 1e-3 * wmax
        smax = max(want[:, :n].sum(0).abs().max().item(), 1e-6)
        assert _max_err(got[:, :n].double().sum(0), want[:, :n].sum(0)) < 1e-3 * smax
        assert _max_err(got[:, n], want[:, n]) < 1e-4
        assert abs(got[:, n].double().sum().item() - want[:, n].sum().item()) < 1e-4
    assert _max_err(o["dpass"], ref.dpass) < 1e-4
    assert torch.equal(o["dpass"], o["dpw"][:, 2 * Cr])
    # boards with no mass: exact zeros out of NaN-filled outputs; a pass-only row is not one of them
    none = ~ref.has
    assert torch.equal(none, kind == PR.ZERO) and bool(none.any())
    for name in ("loss", "correct", "dhead", "dpass", "dpw"):
        assert bool((o[name].cpu()[none] == 0).all()), name
    assert bool((o["dz"].cpu()[none].float() == 0).all())
    live = (kind == PR.PASS_ONLY) | (kind == PR.PASS_MAJOR)
    assert bool((o["loss"].cpu()[live] > 0).all())
    if pass_b:  # the pass is the logit argmax everywhere: correct exactly on the rows whose maximum is the pass
        assert torch.equal(o["correct"].cpu().bool(), live)
    elif B > 3:
        assert 0 < o["correct"].sum().item() < B
    # two runs, the same bits
    o2 = _run(ops, case, td.to(cuda_device), S, gs, pass_b, weight=wt if weighted else None,
              sym=None if sym is None else sym.to(cuda_device))
    for name in o:
        assert torch.equal(o[name].view(torch.int16 if o[name].dtype == torch.bfloat16 else torch.int32),
                           o2[name].view(torch.int16 if o2[name].dtype == torch.bfloat16 else torch.int32)), name


@pytest.mark.parametrize("with_sym", [False, True])
@pytest.mark.parametrize("C,C_real,B,S", PR.PASS_SHAPES)
def test_silent_pass_is_the_soft_head_bit_for_bit(ops, cuda_device, C, C_real, B, S, with_sym):
    """pass_w = 0, pass_b = -1e30 and a zero pass column: every sum gets one more exact zero, so loss, correct,
    dz and dhead carry policy_head_train_soft's bits."""
    import soft_head_refs as SR

    case = _dev(ops, C, C_real, B, S, cuda_device)
    c, yp, w, b, wt, P, a, pw, pwp = case
    td, sym, _ = SR.soft_targets(C, C_real, B, S, S * S + 1, with_sym)
    td = td.to(cuda_device).clone()
    td[:, S * S] = 0.0
    sym = None if sym is None else sym.to(cuda_device)
    gs = 1.0 / B
    o = _run(ops, case, td, S, gs, -1e30, weight=wt, sym=sym, pass_w=torch.zeros_like(pwp))
    s = _outputs(yp, B, C_real)
    ops.policy_head_train_soft(yp, w, b, td, s["dz"], s["loss"], s["correct"], s["dhead"], S, gs, weight=wt, sym=sym)
    torch.cuda.synchronize()
    assert float(o["loss"].sum()) > 0
    for name in ("loss", "correct", "dhead"):
        assert torch.equal(o[name].view(torch.int32), s[name].view(torch.int32)), name
    assert torch.equal(o["dz"].view(torch.int16), s["dz"].view(torch.int16))
    assert not bool(o["dpass"].any()) and not bool(o["dpw"].any())


# ----------------------------------------------------------------------------- gpool_bwd_add_masked
def _padded(B, S, C, device, interior, border=0.0):
    y = torch.full((B, S + 2, S + 2, C), border, dtype=torch.bfloat16, device=device)
    y[:, 1:S + 1, 1:S + 1] = interior.to(device=device, dtype=torch.bfloat16)
    return y


@pytest.mark.parametrize("B,S,C,C_real", [(1, 9, 64, 64), (3, 19, 192, 192), (1, 19, 192, 152), (600, 9, 64, 40)])
def test_gpool_bwd_add_masked_exact_on_integers(ops, cuda_device, B, S, C, C_real):
    """Integer dz in [-8, 8], dpass and pass_w small multiples of powers of two: with inv = float32(1 / S*S) every
    product and sum below is one fp32 rounding that torch reproduces in the same order, and the final sum of a
    small integer and a small addend rounds to bf16 the same way; so the result must EQUAL the torch expression
    of the formula.  B = 1 splits the board over eight workgroups; B = 600 runs one per board."""
    g = torch.Generator().manual_seed(B * 7 + S + C)
    NP = S * S
    yi = torch.randint(-3, 6, (B, S, S, C), generator=g).clamp_min(0).float()   # about a third masked (y == 0)
    yi[..., C_real:] = 0
    yi[0, :, :, 1] = 0.0                                  # an all-zero channel: argmax 0, masked everywhere
    yi[0, 2, 3, 0] = yi[0, 7, 1, 0] = 9.0                 # a planted double maximum: pixel 2 S + 3
    y = _padded(B, S, C, cuda_device, yi)
    dzi = torch.randint(-8, 9, (B, S, S, C), generator=g).float()
    dz = _padded(B, S, C, cuda_device, dzi, border=3.0)
    dz[:, 1:S + 1, 1:S + 1, C_real:] = 5.0                # padded channels: y == 0 there, they must keep their bits
    before = dz.clone()
    P = torch.zeros(B, 2, C, device=cuda_device)
    a = torch.zeros(B, C, dtype=torch.int32, device=cuda_device)
    ops.gpool_fwd(y, P, a, S)
    assert a[0, 0].item() == 2 * S + 3 and a[0, 1].item() == 0
    dpass = (torch.randint(-8, 9, (B,), generator=g).float() / 4).to(cuda_device)
    dpass[0] = 1.5
    pw = torch.zeros(2, C)
    pw[:, :C_real] = torch.randint(-8, 9, (2, C_real), generator=g).float() / 8
    pw = pw.to(cuda_device)
    ops.gpool_bwd_add_masked(dpass, pw, a, y, dz, S)
    torch.cuda.synchronize()
    inv = torch.tensor(PR.inv32(S), device=cuda_device)
    d0 = (dpass[:, None] * pw[0][None, :]) * inv           # (B, C), two roundings
    d1 = dpass[:, None] * pw[1][None, :]
    hit = torch.arange(NP, device=cuda_device)[None, :, None] == a[:, None, :].long()
    add = torch.where(hit, (d0 + d1)[:, None, :], d0[:, None, :].expand(B, NP, C))
    old = before[:, 1:S + 1, 1:S + 1].reshape(B, NP, C)
    yint = y[:, 1:S + 1, 1:S + 1].reshape(B, NP, C)
    want = torch.where(yint > 0, (old.float() + add).bfloat16(), old)
    got = dz[:, 1:S + 1, 1:S + 1].reshape(B, NP, C)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool((got != old)[yint > 0].any())              # something was added
    assert torch.equal(got[yint <= 0].view(torch.int16), old[yint <= 0].view(torch.int16))  # masked pixels keep their bits
    assert torch.equal(got[0, :, 1], old[0, :, 1])         # the all-zero channel, its argmax pixel 0 included
    assert bool((got[..., C_real:] == 5.0).all())          # padded channels
    border = dz.clone()
    border[:, 1:S + 1, 1:S + 1] = 3.0
    assert bool((border == 3.0).all())                     # the border
    assert bool((hit & (yint > 0) & (d1 != 0)[:, None, :]).any())  # the max part reached an unmasked argmax pixel


def test_gpool_bwd_add_masked_against_the_fp64_reference(ops, cuda_device):
    """On head_case activations after policy_head_soft_pass: dz + the pooling's gradient against the reference's
    dz + dpool, within one bf16 rounding of the sum (2^-8 relative) and the head's dz tolerance."""
    C, C_real, B, S = 160, 152, 7, 19
    case = _dev(ops, C, C_real, B, S, cuda_device)
    c, yp, w, b, wt, P, a, pw, pwp = case
    td, sym, _ = PR.pass_targets(C, C_real, B, S, False)
    gs = 1.0 / B
    o = _run(ops, case, td.to(cuda_device), S, gs, 2.0, weight=wt)
    ref = PR.pass_head_ref(c.y, c.w, c.b, pw, 2.0, td, None, c.weight, gs)
    assert torch.equal(a[:, :C_real].cpu().long(), ref.argmax)
    dz = o["dz"].clone()
    ops.gpool_bwd_add_masked(o["dpass"], pwp, a, yp, dz, S)
    torch.cuda.synchronize()
    want = ref.dz + ref.dpool
    assert float(ref.dpool.abs().max()) > 1e-2 * float(ref.dz.abs().max())  # the pooling's part is visible
    err = (dz[:, 1:-1, 1:-1].double().cpu() - want).abs()
    assert float(err.max()) < 1e-2 * float(want.abs().max())
    assert R.border_is_zero(dz) and not bool((dz[:, 1:-1, 1:-1, C_real:] != 0).any())


# ----------------------------------------------------------------------------- policy_value_pass_head
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("legal", [False, True])
@pytest.mark.parametrize("C,C_real,B,S", PR.PASS_SHAPES)
def test_policy_value_pass_head(ops, cuda_device, C, C_real, B, S, legal, own):
    dev = cuda_device
    c, yp, w, b, wt, P, a, pw, pwp = _dev(ops, C, C_real, B, S, dev)
    SS = S * S
    g = torch.Generator().manual_seed(31 * C + 5 * B + S)
    wv, bv = (torch.randn(C_real, generator=g) * 0.05).to(dev), torch.randn(1, generator=g).to(dev)
    wo, bo = (torch.randn(C_real, generator=g) * 0.05).to(dev), torch.randn(1, generator=g).to(dev)
    lg = (torch.rand(B, SS, generator=g) > 1.0 / 3.0).to(torch.uint8)
    lg[B - 1] = 0  # a board with no legal point
    lgd = lg.to(dev) if legal else None
    nan = float("nan")
    probs = torch.full((B, SS + 1), nan, device=dev)
    zv, ownr = torch.full((B, SS), nan, device=dev), torch.full((B, SS), nan, device=dev)
    pb = torch.tensor([0.75], device=dev)
    kw = dict(wo=wo, bo=bo, own=ownr) if own else {}
    ops.policy_value_pass_head(yp, w, b, wv, bv, P, pwp, pb, probs, zv, S, legal=lgd, **kw)
    p0, zv0, own0 = torch.full((B, SS), nan, device=dev), torch.full((B, SS), nan, device=dev), torch.full((B, SS), nan, device=dev)
    ops.policy_value_own_head(yp, w, b, wv, bv, wo, bo, p0, zv0, own0, S, legal=lgd)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(probs).all())
    assert float((probs.double().sum(1) - 1).abs().max()) <= 1e-6
    ref = PR.pass_probs_ref(c.y, c.w, c.b, pw, 0.75, lg if legal else None)
    print("probs max err %.3g, pass entry max err %.3g" % (_max_err(probs, ref), _max_err(probs[:, SS], ref[:, SS])))
    assert _max_err(probs[:, SS], ref[:, SS]) <= 1e-5 and _max_err(probs, ref) <= 1e-5
    assert bool((probs[:, SS] > 0).all())
    if legal:
        assert not bool((probs[:, :SS][lgd == 0] != 0).any())
        assert probs[B - 1, SS].item() == 1.0
    assert torch.equal(zv.view(torch.int32), zv0.view(torch.int32))
    if own:
        assert torch.equal(ownr.view(torch.int32), own0.view(torch.int32))


@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("legal", [False, True])
@pytest.mark.parametrize("C,C_real,B,S", PR.PASS_SHAPES)
def test_silent_pass_probs_are_the_own_head_bit_for_bit(ops, cuda_device, C, C_real, B, S, legal, own):
    """pass_w = 0 and pass_b = -1e30: the pass entry is never the maximum and adds one exact zero to the sum of
    exponentials, so on every board with a legal point the S * S board columns of probs carry
    policy_value_own_head's bits and the pass column is 0.  (A board with no legal point has the pass as its
    only entry: probability 1, where the own head writes zeros.)"""
    dev = cuda_device
    c, yp, w, b, wt, P, a, pw, pwp = _dev(ops, C, C_real, B, S, dev)
    SS = S * S
    g = torch.Generator().manual_seed(31 * C + 5 * B + S)
    wv, bv = (torch.randn(C_real, generator=g) * 0.05).to(dev), torch.randn(1, generator=g).to(dev)
    wo, bo = (torch.randn(C_real, generator=g) * 0.05).to(dev), torch.randn(1, generator=g).to(dev)
    lg = (torch.rand(B, SS, generator=g) > 1.0 / 3.0).to(torch.uint8)
    lg[B - 1] = 0  # a board with no legal point
    lgd = lg.to(dev) if legal else None
    nan = float("nan")
    probs = torch.full((B, SS + 1), nan, device=dev)
    zv, ownr = torch.full((B, SS), nan, device=dev), torch.full((B, SS), nan, device=dev)
    kw = dict(wo=wo, bo=bo, own=ownr) if own else {}
    ops.policy_value_pass_head(yp, w, b, wv, bv, P, torch.zeros_like(pwp), torch.tensor([-1e30], device=dev), probs, zv,
                               S, legal=lgd, **kw)
    p0, zv0, own0 = (torch.full((B, SS), nan, device=dev) for _ in range(3))
    ops.policy_value_own_head(yp, w, b, wv, bv, wo, bo, p0, zv0, own0, S, legal=lgd)
    torch.cuda.synchronize()
    live = lgd.bool().any(1) if legal else torch.ones(B, dtype=torch.bool, device=dev)
    assert int(live.sum()) == (B - 1 if legal else B)
    assert float(p0[live].sum()) > 0
    assert torch.equal(probs[live, :SS].view(torch.int32), p0[live].view(torch.int32))
    assert not bool(probs[live, SS].any())
    if legal:
        assert probs[B - 1, SS].item() == 1.0 and not bool(probs[B - 1, :SS].any())


# ----------------------------------------------------------------------------- host checks, debug library
def test_host_checks(ops, cuda_device):
    C, Cr, B, S = 8, 8, 3, 9
    case = _dev(ops, C, Cr, B, S, cuda_device)
    c, yp, w, b, wt, P, a, pw, pwp = case
    td = torch.full((B, S * S + 1), 1.0, device=cuda_device)
    _run(ops, case, td, S, 1.0 / B, 0.0)  # the well-formed call passes
    pb = torch.zeros(1, device=cuda_device)

    def soft(**kw):
        o = _outputs(yp, B, Cr)
        args = dict(y=yp, w=w, b=b, pooled=P, pass_w=pwp, pass_b=pb, tdist=td, **o)
        args.update(kw)
        ops.policy_head_soft_pass(args["y"], args["w"], args["b"], args["pooled"], args["pass_w"], args["pass_b"],
                                  args["tdist"], args["dz"], args["loss"], args["correct"], args["dhead"], args["dpass"],
                                  args["dpw"], S, 1.0 / B)

    bad = [
        lambda: soft(tdist=td[:, :S * S].contiguous()),   # a narrower row has no pass entry
        lambda: soft(tdist=td.cpu()),
        lambda: soft(tdist=td.double()),
        lambda: soft(pooled=P.cpu()),
        lambda: soft(pooled=P[:, :1].contiguous()),
        lambda: soft(pass_w=pwp.view(-1)),
        lambda: soft(pass_w=pwp.cpu()),
        lambda: soft(pass_b=pb.cpu()),
        lambda: soft(dpass=torch.zeros(B - 1, device=cuda_device)),
        lambda: soft(dpw=torch.zeros(B, 2 * Cr, device=cuda_device)),
        lambda: soft(dpw=torch.zeros(B, 2 * Cr + 1).double().to(cuda_device)),
        lambda: ops.gpool_bwd_add_masked(torch.zeros(B, device=cuda_device), pwp, a, yp, yp.clone().float(), S),
        lambda: ops.gpool_bwd_add_masked(torch.zeros(B - 1, device=cuda_device), pwp, a, yp, yp.clone(), S),
        lambda: ops.gpool_bwd_add_masked(torch.zeros(B), pwp, a, yp, yp.clone(), S),
        lambda: ops.gpool_bwd_add_masked(torch.zeros(B, device=cuda_device), pwp, a.long(), yp, yp.clone(), S),
        lambda: ops.gpool_bwd_add_masked(torch.zeros(B, device=cuda_device), pwp[:1], a, yp, yp.clone(), S),
        lambda: ops.policy_value_pass_head(yp, w, b, w, b, P, pwp, pb, torch.zeros(B, S * S, device=cuda_device),
                                           torch.zeros(B, S * S, device=cuda_device), S),
        lambda: ops.policy_value_pass_head(yp, w, b, w, b, P, pwp, pb, torch.zeros(B, S * S + 1, device=cuda_device),
                                           torch.zeros(B, S * S, device=cuda_device), S, wo=w),
        lambda: ops.policy_value_pass_head(yp, w, b, w, b, P.cpu(), pwp, pb, torch.zeros(B, S * S + 1, device=cuda_device),
                                           torch.zeros(B, S * S, device=cuda_device), S),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail("case %d did not raise" % i)
    torch.cuda.synchronize()


_DEBUG_CHILD = r"""
import torch
from alphago_amd import ops
assert ops.flavor() == "debug"
dev = torch.device("cuda")
B, S, C = 3, 9, 64
g = torch.Generator().manual_seed(1)
y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
y[:, 1:-1, 1:-1] = torch.randn(B, S, S, C, generator=g).clamp_min(0).to(dev)
w = (torch.randn(C, generator=g) * 0.05).to(dev); b = torch.zeros(1, device=dev)
P = torch.zeros(B, 2, C, device=dev); a = torch.zeros(B, C, dtype=torch.int32, device=dev)
ops.gpool_fwd(y, P, a, S)
pw = (torch.randn(2, C, generator=g) * 0.01).to(dev); pb = torch.zeros(1, device=dev)
td = torch.rand(B, S * S + 1, generator=g).to(dev)
dz = torch.zeros_like(y)
loss, corr, dpass = (torch.zeros(B, device=dev) for _ in range(3))
dhead = torch.zeros(B, C + 1, device=dev); dpw = torch.zeros(B, 2 * C + 1, device=dev)
# the bounds-checked kernels run clean on well-formed tensors
ops.policy_head_soft_pass(y, w, b, P, pw, pb, td, dz, loss, corr, dhead, dpass, dpw, S, 1.0 / B)
ops.gpool_bwd_add_masked(dpass, pw, a, y, dz, S)
probs = torch.zeros(B, S * S + 1, device=dev); zv = torch.zeros(B, S * S, device=dev)
ops.policy_value_pass_head(y, w, b, w, b, P, pw, pb, probs, zv, S)
torch.cuda.synchronize()
assert abs(float(probs.sum()) - B) < 1e-4 and float(loss.sum()) > 0
# a short output buffer is refused on the host (the op's always-on extent check), before any launch
try:
    ops.policy_head_soft_pass(y, w, b, P, pw, pb, td, dz, loss, corr, dhead, dpass, dpw[:B - 1], S, 1.0 / B)
except RuntimeError as e:
    assert "dpw must hold (B, 2 C_real + 1)" in str(e), e
    print("DEBUG-OK")
else:
    raise SystemExit("the short buffer was accepted")
"""


def test_debug_library_checks_the_new_accesses(cuda_device):
    """The AGK_DEBUG library runs the three kernels clean with their device-side bounds checks on.  A deliberately
    short output buffer is refused on the host before any launch: by the op's own extent check, which both
    libraries have (the debug library adds no second host check behind it, since it could not be reached)."""
    from alphago_amd import _build

    assert os.path.exists(_build.hip_path("debug")), "debug library not built"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ALPHAGO_AMD_KERNELS="debug", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _DEBUG_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEBUG-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
