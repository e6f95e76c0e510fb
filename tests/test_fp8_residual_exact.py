"""The skip operand of the fp8 conv kernels (conv_fwd_fp8 / conv_dgrad_fp8_bits ``res=``), bit-exact on
integer data: the operands and oracles of tests/residual_refs.py on the three 192-wide cases, as e4m3 /
e5m2 bytes with both E8M0 exponent pairs of tests/test_conv_exact.py.

The MFMA's block scales multiply the conv sum (and the bias passed in) by m = 2^(ex + ew - 254), a power of
two, and the skip is in real units, so it is passed as res * m (exact in bf16) and every expectation is m
times the oracle's.  The oracles stay where integers are exact in bf16: max |pre + res| <= 256 before the
multiplier (asserted per case; 143 / 147 / 152 for the forward and 123 / 125 / 116 for the dgrad).

Forward:  y = bf16(relu(pre + res)) bitwise, e4m3 bytes == fp8_ref.quantize(y * 2^-4) (ties occur), the
ReLU' bitmask == (y > 0), the 64 amax slots fold to exactly max y, borders untouched.
Bitmask dgrad: dx = (raw + res) under the mask and +0 elsewhere, e5m2 bytes, max |dx|.
The skip buffer's border pixels are NaN (residual_refs.res_buffer): a border read shows in the interior.
Without ``res`` the same launch into the same sentinel buffers gives the no-skip oracle."""
import pytest
import torch

import conv_refs as R
import fp8_ref
import residual_refs as RR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CASES = [c for c in RR.CASES if c[2] == 192 and c[3] == 192]
assert CASES == [(19, 1, 192, 192, 3, 1), (19, 3, 192, 192, 3, 1), (9, 5, 192, 192, 3, 1)]
# E8M0 scale bytes (127 = 2^0): all ones, and activations / gradients 2^2 with weights 2^-1 (product 2)
FP8_EXPONENTS = [(127, 127), (129, 126)]
OUT_SCALE = 2.0 ** -4  # byte outputs of integers / 16: ties to even occur
BYTE_SENTINEL = 0x5A
EXACT_MAX = 256  # integers up to 256 are exact in bf16


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _mult(exps):
    return 2.0 ** (exps[0] - 127 + exps[1] - 127)


def _bytes(t_nhwc, P, dtype, dev):
    """Integer values as e4m3 / e5m2 bytes in a zero-bordered padded buffer (exact: |v| <= 4)."""
    b = R.place(t_nhwc, P, torch.float32).to(dtype)
    assert torch.equal(b.float().double(), R.place(t_nhwc, P, torch.float64))
    return b.view(torch.uint8).to(dev)


def _quant(t64, fmt):
    return torch.from_numpy(fp8_ref.quantize(t64.float().numpy(), fmt))


def _i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def _w8(ops, dev, w, transposed):
    out = torch.zeros(ops.fp8_weight_shape(w.shape[2], 192, 192), dtype=torch.uint8, device=dev)
    ops.pack_weights_fp8_multi([w.float().to(dev)], [out], torch.ones(1, device=dev), [0], [int(transposed)])
    return out


def _amax(slots):
    return slots.view(torch.float32).max().item()


def _skip(res, m, dev):
    """res * m as the kernels read it: bf16, NaN border; exact."""
    buf = RR.res_buffer(res * m)
    assert torch.equal(R.interior(buf, 1, res.shape[1]).double(), res * m)
    return buf.to(dev)


def _sentinels(ops, dev, case):
    S, B, C = case[0], case[1], case[3]
    y = torch.full((B, S + 2, S + 2, C), R.BF16_SENTINEL, dtype=BF, device=dev)
    y8 = torch.full(y.shape, BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    mb = torch.full((B * (S + 2) ** 2 * ops.mbits_words(C),), R.MBITS_SENTINEL, dtype=torch.int32, device=dev)
    return y, y8, mb, ops.fp8_amax_buffer(1, dev)[0]


# ----------------------------------------------------------------------------- forward
def _fwd_run(ops, dev, case, exps, outs, with_res):
    S, B, Cin, Cout, K, Pin = case
    c = RR.fwd_case(case)
    m = _mult(exps)
    assert (c["pre"] + c["res"]).abs().max().item() <= EXACT_MAX
    x8 = _bytes(c["x"], Pin, torch.float8_e4m3fn, dev)
    w8 = _w8(ops, dev, c["w"], False)
    y, y8, mb, amax = _sentinels(ops, dev, case)
    y8 = y8 if outs == "both" else None
    ops.conv_fwd_fp8(x8, w8, (c["bias"] * m).to(dev), _i32(exps, dev), torch.tensor([OUT_SCALE], device=dev), K, S,
                     Pin, 1, y_bf16=y, y_fp8=y8, amax=amax, mbits=mb,
                     **({"res": _skip(c["res"], m, dev)} if with_res else {}))
    torch.cuda.synchronize()
    oracle = c if with_res else R.fwd_case(case)
    want = oracle["y"].double() * m
    assert R.check_padded(y.cpu(), want.to(BF), 1, R.BF16_SENTINEL) == []
    if y8 is not None:
        assert R.check_padded(y8.cpu(), _quant(want * OUT_SCALE, "e4m3"), 1, BYTE_SENTINEL) == []
    assert R.check_mbits(mb.cpu(), oracle["mask"], Cout) == []
    assert torch.equal(oracle["mask"], oracle["y"] > 0)
    assert _amax(amax) == want.max().item()


@pytest.mark.parametrize("outs", ["both", "bf16"])
@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_fp8_forward_res(ops, cuda_device, case, exps, outs):
    """conv_fwd_fp8 with the skip operand: every output follows relu(pre + res)."""
    _fwd_run(ops, cuda_device, case, exps, outs, True)


@pytest.mark.parametrize("outs", ["both", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_fp8_forward_res_is_optional(ops, cuda_device, case, outs):
    """The same launch without ``res`` gives the no-skip oracle."""
    _fwd_run(ops, cuda_device, case, FP8_EXPONENTS[1], outs, False)


# ----------------------------------------------------------------------------- bitmask dgrad
def _dgrad_run(ops, dev, case, exps, outs, with_res):
    S, B, C, _, K, Pin = case
    c = RR.dgrad_case(case)
    m = _mult(exps)
    assert (c["raw"] + c["res"]).abs().max().item() <= EXACT_MAX
    dz8 = _bytes(c["dz"], 1, torch.float8_e5m2, dev)
    w8t = _w8(ops, dev, c["w"], True)
    mbits = R.encode_mbits(c["mask"], C).flatten().to(dev)
    dx, dx8, _, amax = _sentinels(ops, dev, case)
    dx8 = dx8 if outs == "both" else None
    ops.conv_dgrad_fp8_bits(dz8, w8t, mbits, _i32(exps, dev), torch.tensor([OUT_SCALE], device=dev), K, S, y_bf16=dx,
                            y_fp8=dx8, amax=amax, **({"res": _skip(c["res"], m, dev)} if with_res else {}))
    torch.cuda.synchronize()
    want = (c["dx"] if with_res else R.dgrad_case(case)["dx"]) * m
    assert R.check_padded(dx.cpu(), want.to(BF), 1, R.BF16_SENTINEL) == []
    # +0 where the bit is off, the sign bit too (torch.equal takes -0 for +0)
    assert not R.interior(dx.cpu(), 1, S).view(torch.int16)[~c["mask"]].any()
    if dx8 is not None:
        assert R.check_padded(dx8.cpu(), _quant(want * OUT_SCALE, "e5m2"), 1, BYTE_SENTINEL) == []
    assert _amax(amax) == want.abs().max().item()


@pytest.mark.parametrize("outs", ["both", "bf16"])
@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_fp8_dgrad_bits_res(ops, cuda_device, case, exps, outs):
    """conv_dgrad_fp8_bits with the skip gradient: dx = bit ? raw + res : +0."""
    _dgrad_run(ops, cuda_device, case, exps, outs, True)


@pytest.mark.parametrize("outs", ["both", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_fp8_dgrad_bits_res_is_optional(ops, cuda_device, case, outs):
    _dgrad_run(ops, cuda_device, case, FP8_EXPONENTS[1], outs, False)


# ----------------------------------------------------------------------------- refusals (no kernel runs)
def _zero_args(ops, dev, C, S=9, B=1):
    x8 = torch.zeros((B, S + 2, S + 2, C), dtype=torch.uint8, device=dev)
    w8 = torch.zeros(ops.fp8_weight_shape(3, C, C), dtype=torch.uint8, device=dev)
    yb = torch.zeros((B, S + 2, S + 2, C), dtype=BF, device=dev)
    res = torch.zeros_like(yb)
    mb = torch.zeros(B * (S + 2) ** 2 * ops.mbits_words(C), dtype=torch.int32, device=dev)
    return x8, w8, yb, torch.zeros_like(x8), res, mb, _i32((127, 127), dev), torch.ones(1, device=dev)


def _refused(ops, dev, op, C, alias=False, **kw):
    x8, w8, yb, y8, res, mb, sc, osc = _zero_args(ops, dev, C)
    args = dict(y_bf16=yb, y_fp8=y8, res=yb if alias else res)
    args.update(kw)
    with pytest.raises(RuntimeError, match=op):
        if op == "conv_fwd_fp8":
            ops.conv_fwd_fp8(x8, w8, torch.zeros(C, device=dev), sc, osc, 3, 9, 1, 1, **args)
        else:
            ops.conv_dgrad_fp8_bits(x8, w8, mb, sc, osc, 3, 9, **args)


@pytest.mark.parametrize("op", ["conv_fwd_fp8", "conv_dgrad_fp8_bits"])
def test_res_refusals(ops, cuda_device, op):
    dev = cuda_device
    _refused(ops, dev, op, 192, alias=True)               # the skip is the bf16 output
    _refused(ops, dev, op, 192, y_bf16=None)              # no bf16 output: the residual stream is bf16
    _refused(ops, dev, op, 192, res=torch.zeros((1, 11, 11, 192), device=dev))            # fp32
    _refused(ops, dev, op, 192, res=torch.zeros((1, 11, 11, 192), dtype=BF))              # host tensor
    _refused(ops, dev, op, 192, res=torch.zeros((2, 11, 11, 192), dtype=BF, device=dev))  # another shape
    _refused(ops, dev, op, 160)                           # width 160
    if op == "conv_fwd_fp8":
        _refused(ops, dev, op, 128)                       # width 128 (the bitmask dgrad has no such tile at all)


def test_res_refused_as_byte_output_alias(ops, cuda_device):
    """The skip may not be the byte output's memory either (a bf16 view of the same storage)."""
    dev = cuda_device
    x8, w8, yb, _, _, mb, sc, osc = _zero_args(ops, dev, 192)
    store = torch.zeros(yb.numel(), dtype=BF, device=dev)
    res = store.view(yb.shape)
    y8 = store.view(torch.uint8)[:yb.numel()].view(yb.shape)
    with pytest.raises(RuntimeError, match="conv_fwd_fp8"):
        ops.conv_fwd_fp8(x8, w8, torch.zeros(192, device=dev), sc, osc, 3, 9, 1, 1, y_bf16=yb, y_fp8=y8, res=res)
    with pytest.raises(RuntimeError, match="conv_dgrad_fp8_bits"):
        ops.conv_dgrad_fp8_bits(x8, w8, mb, sc, osc, 3, 9, y_bf16=yb, y_fp8=y8, res=res)


def test_dgrad_fp8_bf16_has_no_res(ops, cuda_device):
    """conv_dgrad_fp8_bf16 (the mixed arm's dgrad) takes no skip operand: its schema has none."""
    dev = cuda_device
    x8, w8, yb, _, res, mb, sc, osc = _zero_args(ops, dev, 192)
    with pytest.raises(TypeError):
        ops.conv_dgrad_fp8_bf16(torch.zeros_like(yb), w8, mb, sc, osc, 3, 9, yb, res=res)
