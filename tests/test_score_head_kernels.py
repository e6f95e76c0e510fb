"""The score head's kernels: score_out (head_score.hip) against the float64 reference of score_head_refs.py within
bounds counted from its fp32 roundings, and gpool_bwd_add_masked_dp (gpool.hip) bit for bit against the torch
float32 expression of its documented order and against gpool_bwd_add_masked.

Shapes: B = 1 (the map kernel splits a board over eight workgroups; a lone wave in score_out's workgroup), 3 (a
partly filled workgroup), 70 (more than one workgroup, not a multiple of four) and 512 (the first batch at which the
map kernel's split is 1); S = 5 and 19; C = 64, 160 with 152 real channels and 192; D = 8 (fewer elements than
lanes), 64 (one per lane) and 72 (a second, partly filled round)."""
import os
import subprocess
import sys

import pytest
import torch

import score_head_refs as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _nan(*shape, device):
    return torch.full(shape, float("nan"), device=device)


# ----------------------------------------------------------------------------- score_out
OUT_SHAPES = [(1, 8), (3, 64), (70, 72), (512, 64), (70, 8), (3, 72)]


def _run_out(ops, dev, upre, w2, b2, t, valid, weight, gs, delta):
    B, D = upre.shape
    o = dict(s=_nan(B, device=dev), loss=_nan(B, device=dev), abserr=_nan(B, device=dev), du=_nan(B, D, device=dev),
             dout=_nan(B, D + 1, device=dev))
    ops.score_out(upre.to(dev), w2.to(dev), b2.to(dev), o["s"], target=t.to(dev),
                  valid=None if valid is None else valid.to(dev), weight=None if weight is None else weight.to(dev),
                  loss=o["loss"], abserr=o["abserr"], du=o["du"], dout=o["dout"], grad_scale=gs, delta=delta)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("masks", [True, False])
@pytest.mark.parametrize("B,D", OUT_SHAPES)
def test_score_out_vs_fp64(ops, cuda_device, B, D, masks):
    dev = cuda_device
    upre, w2, b2, t, valid, weight = SR.out_case(B, D)
    if not masks:
        valid = weight = None
    gs, delta = 1.0 / B, 1.0
    ref = SR.score_out_ref(upre, w2, b2, t, valid, weight, gs, delta)
    bnd = SR.score_out_bounds(upre, w2, b2, ref, valid, weight, gs, delta)
    # the two kinks, from the reference alone: at most 1 % of the elements, and the bound of e is below the
    # margin, so the kernel takes the reference's branch everywhere else
    near_relu = upre.abs() < SR.KINK
    near_huber = (ref.e.abs() - delta).abs() < SR.KINK
    assert float(near_relu.float().mean()) <= 0.01 and float(near_huber.float().mean()) <= 0.01
    assert float(bnd["e"].max()) < SR.KINK
    if B >= 70:
        assert bool((ref.e.abs() > delta).any()) and bool((ref.e.abs() < delta).any())  # both arms of the loss
    o = _run_out(ops, dev, upre, w2, b2, t, valid, weight, gs, delta)
    for k, v in o.items():
        assert bool(torch.isfinite(v).all()), k

    def check(name, got, want, bound, keep):
        err = (got.double().cpu() - want).abs()
        rel = (err / bound.clamp_min(1e-300))[keep]
        print("%s max err / bound: %.3g" % (name, rel.max().item() if rel.numel() else 0.0))
        assert bool((err <= bound)[keep].all()), name

    board = ~near_huber
    elem = board[:, None] & ~near_relu
    check("s", o["s"], ref.s, bnd["s"], torch.ones(B, dtype=torch.bool))
    check("loss", o["loss"], ref.loss, bnd["loss"], board)
    check("abserr", o["abserr"], ref.abserr, bnd["abserr"], board)
    check("du", o["du"], ref.du, bnd["du"], elem)
    check("dout", o["dout"], ref.dout, bnd["dout"], torch.cat([elem, board[:, None]], 1))
    if masks and B >= 3:  # valid = 0 (board 1) and weight = 0 (board 2): exact zeros
        assert not bool(o["du"][1:3].any()) and not bool(o["dout"][1:3].any())
        assert float(o["loss"][1]) > 0 and float(o["abserr"][2]) > 0  # the metrics do not see the masks
        assert bool(o["du"][0].any())
    # forward mode gives s the same bits and needs no other buffer; two runs are bit-equal
    s2 = _nan(B, device=dev)
    ops.score_out(upre.to(dev), w2.to(dev), b2.to(dev), s2)
    o2 = _run_out(ops, dev, upre, w2, b2, t, valid, weight, gs, delta)
    assert torch.equal(s2.view(torch.int32), o["s"].view(torch.int32))
    for k in o:
        assert torch.equal(o[k].view(torch.int32), o2[k].view(torch.int32)), k


def test_score_out_utility(ops, cuda_device):
    """value <- (value + lam * tanh(s / 2)) / (1 + lam), in [-1, 1]; tanhf and the two divisions within 1e-6."""
    dev = cuda_device
    B, D = 70, 64
    upre, w2, b2, _, _, _ = SR.out_case(B, D, seed=3)
    ref = SR.score_out_ref(upre, w2 * 3, b2)
    v = torch.tanh(torch.randn(B, generator=torch.Generator().manual_seed(1)) * 2)
    v[0], v[1] = 1.0, -1.0
    vd = v.clone().to(dev)
    s = _nan(B, device=dev)
    ops.score_out(upre.to(dev), (w2 * 3).to(dev), b2.to(dev), s, value=vd, utility=0.5)
    torch.cuda.synchronize()
    want = (v.double() + 0.5 * torch.tanh(ref.s / 2)) / 1.5
    assert float((vd.double().cpu() - want).abs().max()) < 1e-6
    assert float(vd.abs().max()) <= 1.0 and float((vd.cpu() - v).abs().max()) > 0.05


# ----------------------------------------------------------------------------- gpool_bwd_add_masked_dp
DP_SHAPES = [(1, 19, 192, 192), (3, 5, 64, 64), (70, 19, 160, 152), (512, 5, 64, 64), (3, 19, 192, 192)]
_DP = {}


def _dp_case(ops, dev, B, S, C, C_real):
    """Random activations (about half masked, an all-zero channel, a planted double maximum), a random dz with a
    marked border and marked padded channels, gpool_fwd's argmax, a random dp, dpass and zero-padded pass_w.  Made
    once and written by no test."""
    key = (B, S, C, C_real)
    if key not in _DP:
        g = torch.Generator().manual_seed(B * 7 + S + C)
        yi = torch.randn(B, S, S, C, generator=g).clamp_min(0)
        yi[..., C_real:] = 0
        yi[0, :, :, 1] = 0.0
        yi[0, 2, 3, 0] = yi[0, 4, 1, 0] = 9.0
        y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
        y[:, 1:S + 1, 1:S + 1] = yi.to(dev).bfloat16()
        dz = torch.full((B, S + 2, S + 2, C), 3.0, dtype=torch.bfloat16, device=dev)
        dz[:, 1:S + 1, 1:S + 1] = (torch.randn(B, S, S, C, generator=g) * 0.1).to(dev).bfloat16()
        dz[:, 1:S + 1, 1:S + 1, C_real:] = 5.0
        P = torch.zeros(B, 2, C, device=dev)
        a = torch.zeros(B, C, dtype=torch.int32, device=dev)
        ops.gpool_fwd(y, P, a, S)
        assert a[0, 0].item() == 2 * S + 3 and a[0, 1].item() == 0
        dp = torch.zeros(B, 2, C)
        dp[:, :, :C_real] = torch.randn(B, 2, C_real, generator=g) * 0.05
        dpass = torch.randn(B, generator=g) * 0.1
        pw = torch.zeros(2, C)
        pw[:, :C_real] = torch.randn(2, C_real, generator=g) * 0.3
        _DP[key] = (y, dz, a, dp.to(dev), dpass.to(dev), pw.to(dev))
    return _DP[key]


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("B,S,C,C_real", DP_SHAPES)
def test_dp_kernel_is_the_documented_order_bit_for_bit(ops, cuda_device, B, S, C, C_real):
    y, dz0, a, dp, dpass, pw = _dp_case(ops, cuda_device, B, S, C, C_real)
    # the score head alone
    dz = dz0.clone()
    ops.gpool_bwd_add_masked_dp(dp, a, y, dz, S)
    torch.cuda.synchronize()
    want = SR.dp_add_expected(dz0, y, dp, a, S)
    assert torch.equal(_bits(dz), _bits(want))
    inner, inner0 = dz[:, 1:S + 1, 1:S + 1], dz0[:, 1:S + 1, 1:S + 1]
    yint = y[:, 1:S + 1, 1:S + 1]
    assert bool((inner != inner0)[yint > 0].any())                               # something was added
    assert torch.equal(_bits(inner[yint <= 0]), _bits(inner0[yint <= 0]))       # masked elements keep their bits
    assert bool((inner[..., C_real:] == 5.0).all())                             # padded channels
    border = dz.clone()
    border[:, 1:S + 1, 1:S + 1] = 3.0
    assert bool((border == 3.0).all())                                          # the border
    assert torch.equal(inner[0, :, :, 1], inner0[0, :, :, 1])                   # the all-zero channel
    # the argmax pixel of the planted double maximum got the max part, its twin did not
    d = inner.float() - inner0.float()
    assert d[0, 2, 3, 0].item() != d[0, 4, 1, 0].item()
    # both heads in one pass
    dzm = dz0.clone()
    ops.gpool_bwd_add_masked_dp(dp, a, y, dzm, S, dpass=dpass, pass_w=pw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dzm), _bits(SR.dp_add_expected(dz0, y, dp, a, S, dpass, pw)))
    assert not torch.equal(_bits(dzm), _bits(dz))
    # dp = 0 with the pass operands: gpool_bwd_add_masked's bits
    dza, dzb = dz0.clone(), dz0.clone()
    ops.gpool_bwd_add_masked_dp(torch.zeros_like(dp), a, y, dza, S, dpass=dpass, pass_w=pw)
    ops.gpool_bwd_add_masked(dpass, pw, a, y, dzb, S)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dza), _bits(dzb)) and not torch.equal(_bits(dza), _bits(dz0))
    # two runs
    dz2 = dz0.clone()
    ops.gpool_bwd_add_masked_dp(dp, a, y, dz2, S, dpass=dpass, pass_w=pw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dz2), _bits(dzm))


def test_a_zero_dp_leaves_dz_alone(ops, cuda_device):
    """The silent head: dp = 0 (either sign) changes no bit, negative zeros in dz included."""
    B, S, C, C_real = 3, 5, 64, 64
    y, dz0, a, dp, dpass, pw = _dp_case(ops, cuda_device, B, S, C, C_real)
    dz0 = dz0.clone()
    dz0[:, 2, 2, :8] = -0.0
    for z in (torch.zeros_like(dp), -torch.zeros_like(dp)):
        dz = dz0.clone()
        ops.gpool_bwd_add_masked_dp(z, a, y, dz, S)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dz), _bits(dz0))


# ----------------------------------------------------------------------------- host checks, debug library
def test_host_checks(ops, cuda_device):
    dev = cuda_device
    B, S, C = 3, 5, 64
    y, dz0, a, dp, dpass, pw = _dp_case(ops, dev, B, S, C, C)
    D = 8
    upre, w2, b2 = torch.zeros(B, D, device=dev), torch.zeros(D, device=dev), torch.zeros(1, device=dev)
    s, t = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    tr = dict(target=t, loss=torch.zeros(B, device=dev), abserr=torch.zeros(B, device=dev),
              du=torch.zeros(B, D, device=dev), dout=torch.zeros(B, D + 1, device=dev))
    ops.score_out(upre, w2, b2, s, **tr)  # the well-formed calls pass
    ops.gpool_bwd_add_masked_dp(dp, a, y, dz0.clone(), S)

    def out(**kw):
        args = dict(tr)
        args.update(kw)
        ops.score_out(args.pop("upre", upre), args.pop("w2", w2), args.pop("b2", b2), args.pop("s", s), **args)

    bad = [
        lambda: out(upre=torch.zeros(B, 12, device=dev), w2=torch.zeros(12, device=dev)),   # D not a multiple of 8
        lambda: out(upre=torch.zeros(B, 520, device=dev), w2=torch.zeros(520, device=dev)),
        lambda: out(upre=upre.cpu()),
        lambda: out(upre=upre.double()),
        lambda: out(w2=torch.zeros(D + 8, device=dev)),
        lambda: out(s=torch.zeros(B - 1, device=dev)),
        lambda: out(target=torch.zeros(B + 1, device=dev)),
        lambda: out(du=torch.zeros(B, D - 1, device=dev)),
        lambda: out(dout=torch.zeros(B, D, device=dev)),
        lambda: out(dout=None),
        lambda: out(valid=torch.zeros(B - 1, device=dev)),
        lambda: out(weight=torch.zeros(B).to(dev).double()),
        lambda: out(delta=0.0),
        lambda: ops.score_out(upre, w2, b2, s, weight=t),                                  # no target
        lambda: ops.score_out(upre, w2, b2, s, value=torch.zeros(B - 1, device=dev), utility=0.5),
        lambda: ops.score_out(upre, w2, b2, s, value=torch.zeros(B, device=dev), utility=-0.5),
        lambda: ops.gpool_bwd_add_masked_dp(dp, a, y, dz0[:B - 1].clone(), S),              # an undersized dz
        lambda: ops.gpool_bwd_add_masked_dp(dp, a, y, dz0.clone().float(), S),
        lambda: ops.gpool_bwd_add_masked_dp(dp[:, :1].contiguous(), a, y, dz0.clone(), S),
        lambda: ops.gpool_bwd_add_masked_dp(dp.cpu(), a, y, dz0.clone(), S),
        lambda: ops.gpool_bwd_add_masked_dp(dp.double(), a, y, dz0.clone(), S),
        lambda: ops.gpool_bwd_add_masked_dp(dp, a.long(), y, dz0.clone(), S),
        lambda: ops.gpool_bwd_add_masked_dp(dp, a[:B - 1], y, dz0.clone(), S),
        lambda: ops.gpool_bwd_add_masked_dp(dp, a, y, dz0.clone(), S, dpass=dpass),         # half of the pass term
        lambda: ops.gpool_bwd_add_masked_dp(dp, a, y, dz0.clone(), S, dpass=dpass[:B - 1], pass_w=pw),
        lambda: ops.gpool_bwd_add_masked_dp(dp, a, y, dz0.clone(), S, dpass=dpass, pass_w=pw[:1]),
        lambda: ops.gpool_bwd_add_masked_dp(dp, a, y, dz0.clone(), S + 1),
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
B, S, C, D = 3, 9, 64, 72
g = torch.Generator().manual_seed(1)
y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
y[:, 1:-1, 1:-1] = torch.randn(B, S, S, C, generator=g).clamp_min(0).to(dev)
P = torch.zeros(B, 2, C, device=dev); a = torch.zeros(B, C, dtype=torch.int32, device=dev)
ops.gpool_fwd(y, P, a, S)
upre = torch.randn(B, D, generator=g).to(dev); w2 = torch.randn(D, generator=g).to(dev); b2 = torch.zeros(1, device=dev)
s, t, loss, ae = (torch.zeros(B, device=dev) for _ in range(4))
du = torch.zeros(B, D, device=dev); dout = torch.zeros(B, D + 1, device=dev)
# the bounds-checked kernels run clean on well-formed tensors
ops.score_out(upre, w2, b2, s, target=t, loss=loss, abserr=ae, du=du, dout=dout, grad_scale=1.0 / B)
dp = (torch.randn(B, 2, C, generator=g) * 0.1).to(dev)
dz = torch.zeros_like(y)
ops.gpool_bwd_add_masked_dp(dp, a, y, dz, S)
ops.gpool_bwd_add_masked_dp(dp, a, y, dz, S, dpass=t, pass_w=torch.zeros(2, C, device=dev))
torch.cuda.synchronize()
assert float(loss.sum()) > 0 and float(dz.float().abs().sum()) > 0
# an undersized dz is refused on the host (the op's always-on extent check), before any launch
try:
    ops.gpool_bwd_add_masked_dp(dp, a, y, dz[:B - 1], S)
except RuntimeError as e:
    assert "dz must have y's shape" in str(e), e
    print("DEBUG-OK")
else:
    raise SystemExit("the short buffer was accepted")
"""


def test_debug_library_checks_the_new_accesses(cuda_device):
    """The AGK_DEBUG library runs both kernels clean with their device-side bounds checks on.  An undersized dz is
    refused on the host before any launch, by the op's own extent check, which both libraries have
    (test_host_checks runs the same call on the production library)."""
    from alphago_amd import _build

    assert os.path.exists(_build.hip_path("debug")), "debug library not built"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ALPHAGO_AMD_KERNELS="debug", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _DEBUG_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEBUG-OK" in r.stdout, r.stdout + r.stderr
