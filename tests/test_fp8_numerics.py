"""The fp8 codecs and delayed-scale kernels, bit for bit, against the software reference of
tests/fp8_ref.py (itself pinned on the CPU by tests/test_fp8_ref.py): saturation, subnormals, ties,
-0, +-Inf, tails and the grid-stride paths of the quantisers; every exponent, guard and untouched
entry of the scale kernels; every byte of the weight packs; saturating conv epilogues.

NaN inputs are out of scope: the kernels' clamp is a med3 / fmin / fmax chain whose NaN result the
source does not define, and no test here feeds a NaN to a quantiser."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import fp8_ref
from test_conv160 import _fwd_fp8_160_case, _fwd_fp8_160_outputs

pytestmark = pytest.mark.gpu

SCALES = [2.0 ** -20, 2.0 ** -8, 1.0, 2.0 ** 7, 2.0 ** 20, 2.0 ** 100, 1.7, 0.3]
QUANTIZERS = {"quantize_fp8": "e4m3", "quantize_fp8_dev": "e4m3", "quantize_bf8": "e5m2"}
DEV_SCALE = ("quantize_fp8_dev", "quantize_bf8")
INF_BITS = 0x7F800000
FLT_MAX = float(np.finfo(np.float32).max)
FLT_TINY = float(np.float32(2.0 ** -149))  # the smallest float32 subnormal


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


# ----------------------------------------------------------------------------------- quantisers
def _all_bf16_bits(keep_inf):
    """Every bf16 bit pattern; NaN patterns (and, keep_inf False, +-Inf) replaced by 0."""
    bits = np.arange(65536, dtype=np.uint16)
    x = fp8_ref.bf16_to_f32(bits)
    bad = np.isnan(x) if keep_inf else ~np.isfinite(x)
    return np.where(bad, 0, bits).astype(np.uint16)


def _small_bf16_bits(n, seed):
    """n fixed pseudo-random bf16 patterns with |x| < 2 (zeros, subnormals and both signs included)."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 65536, size=n).astype(np.uint16) & np.uint16(0xBFFF)).astype(np.uint16)


def _bf16_bits(value):
    b = np.array([value], dtype=np.float32).view(np.uint32) >> 16
    assert fp8_ref.bf16_to_f32(b)[0] == np.float32(value), "not a bf16 value"
    return int(b[0])


def _f32_bits(value):
    return int(np.array([value], dtype=np.float32).view(np.uint32)[0])


def _to_dev(bits, dev):
    return torch.from_numpy(bits.view(np.int16).copy()).to(dev).view(torch.bfloat16)


def _amax_true_bits(bits):
    return _f32_bits(np.abs(fp8_ref.bf16_to_f32(bits)).max())


def _run_quantizer(ops, name, x, scale, amax=None):
    y = torch.full(x.shape, 0x55, dtype=torch.uint8, device=x.device)
    if name == "quantize_fp8":
        ops._ops().quantize_fp8(x, y, float(scale))  # the raw op: any scale, not only 2^e
        return y, None
    if amax is None:
        amax = ops.fp8_amax_buffer(1, x.device)[0]
    getattr(ops, name)(x, y, torch.tensor([scale], dtype=torch.float32, device=x.device), amax)
    return y, amax


def _assert_bytes(y, x, scale, fmt):
    """y == lut[bits of x] through a gather on the device."""
    lut = torch.from_numpy(fp8_ref.bf16_lut(scale, fmt).copy()).to(x.device)
    want = lut[x.view(torch.int16).to(torch.int64) & 0xFFFF]
    torch.cuda.synchronize()
    bad = (want != y).nonzero()
    assert bad.numel() == 0, (int(bad.shape[0]), [(int(i), hex(int(y.flatten()[i])), hex(int(want.flatten()[i])))
                                                 for i in bad.flatten()[:8]])


def _assert_amax(amax, true_bits):
    a = amax.cpu().numpy()
    assert a.min() >= 0  # float bits of non-negative values: int32 order == float order
    assert int(a.max()) == true_bits, (hex(int(a.max())), hex(true_bits))  # so no slot exceeds the true max


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", list(QUANTIZERS))
def test_quantizers_every_bf16_pattern(ops, cuda_device, name, scale):
    """All 65536 bf16 patterns (NaNs replaced by 0, +-Inf kept): every byte, and the amax == +Inf."""
    bits = _all_bf16_bits(keep_inf=True)
    x = _to_dev(bits, cuda_device)
    y, amax = _run_quantizer(ops, name, x, scale)
    _assert_bytes(y, x, scale, QUANTIZERS[name])
    want, _ = fp8_ref.quantize_bf16(bits, scale, QUANTIZERS[name])
    assert np.array_equal(y.cpu().numpy(), want)
    if amax is not None:
        _assert_amax(amax, INF_BITS)


def _absmax(ops, x, scale, amax):
    ops.absmax_bf16(x, amax)
    return None, amax


@pytest.mark.parametrize("name", DEV_SCALE + ("absmax_bf16",))
def test_amax_slots_are_a_running_max(ops, cuda_device, name):
    """Finite input: the slots' max is the largest finite bf16; a slot preloaded with a larger value is
    kept; an all-zero input leaves every slot 0; absmax_bf16 (the y == null path) writes nothing else."""
    run = (lambda x, amax: _absmax(ops, x, 1.0, amax)) if name == "absmax_bf16" else (
        lambda x, amax: _run_quantizer(ops, name, x, 1.0, amax))
    bits = _all_bf16_bits(keep_inf=False)
    x = _to_dev(bits, cuda_device)
    x0 = x.clone()
    buf = torch.zeros(128, dtype=torch.int32, device=cuda_device)
    buf[64:] = 0x12345678
    run(x, buf[:64])
    torch.cuda.synchronize()
    assert _amax_true_bits(bits) == 0x7F7F0000
    _assert_amax(buf[:64], 0x7F7F0000)
    assert (buf[64:] == 0x12345678).all() and torch.equal(x.view(torch.int16), x0.view(torch.int16))
    if name == "absmax_bf16":  # with +-Inf in the input
        amax = ops.fp8_amax_buffer(1, cuda_device)[0]
        ops.absmax_bf16(_to_dev(_all_bf16_bits(keep_inf=True), cuda_device), amax)
        _assert_amax(amax, INF_BITS)
    # running max: 65536 elements are 32 workgroups, slots 0..31
    amax = ops.fp8_amax_buffer(1, cuda_device)[0]
    amax[5] = _f32_bits(FLT_MAX)
    amax[40] = 7
    run(x, amax)
    torch.cuda.synchronize()
    assert int(amax[5]) == _f32_bits(FLT_MAX) and int(amax[40]) == 7
    rest = amax.clone()
    rest[5] = 0
    _assert_amax(rest, 0x7F7F0000)
    # zeros (+0 and -0) leave every slot 0
    z = np.zeros(8 * 300, dtype=np.uint16)
    z[1::2] = 0x8000
    amax = ops.fp8_amax_buffer(1, cuda_device)[0]
    run(_to_dev(z, cuda_device), amax)
    torch.cuda.synchronize()
    assert (amax == 0).all()


# (elements, kernels): a tail group (3 full workgroups + 5 groups of 8), and one tensor just above each
# launch cap -- 1024 workgroups of 256 x 8 elements, 8192 workgroups of 256 x 4 -- whose only large
# value lies in the last group, i.e. in the grid-strided part
TAIL_CASES = [(8 * (256 * 3 + 5), ("quantize_fp8", "quantize_fp8_dev", "quantize_bf8", "absmax_bf16")),
              (8 * (1024 * 256 + 3), ("quantize_fp8_dev", "quantize_bf8", "absmax_bf16")),
              (4 * (8192 * 256) + 8, ("quantize_fp8",))]


@pytest.mark.parametrize("n,names", TAIL_CASES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_quantizers_tail_and_grid_stride(ops, cuda_device, n, names):
    bits = _small_bf16_bits(n, seed=n % 1000)
    bits[n - 3] = _bf16_bits(-1000.0)  # beyond e4m3's range at the scale below; the only |x| >= 2
    x = _to_dev(bits, cuda_device)
    scale = 1.7
    for name in names:
        if name == "absmax_bf16":
            amax = ops.fp8_amax_buffer(1, cuda_device)[0]
            ops.absmax_bf16(x, amax)
        else:
            y, amax = _run_quantizer(ops, name, x, scale)
            _assert_bytes(y, x, scale, QUANTIZERS[name])
            fmt = QUANTIZERS[name]
            assert int(y[n - 3]) == int(fp8_ref.quantize(np.float32(-1000.0) * np.float32(scale), fmt))
        if amax is not None:
            torch.cuda.synchronize()
            _assert_amax(amax, _f32_bits(1000.0))


# --------------------------------------------------------------------------------- scale kernels
BIG = 10 ** 6


def _pow2_distance(fmt_max, m):
    """Relative distance of fmt_max / m from the nearest power of two (exact rational arithmetic)."""
    r = Fraction(fmt_max) / Fraction(m)
    k = fp8_ref.floor_log2_ratio(fmt_max, m)
    return float(min(r / Fraction(2) ** k - 1, 1 - r / Fraction(2) ** (k + 1)))


def _amax_cases(fmt_max):
    """[(amax, is_neighbour)]: 0, fmt_max * 2^-k for k = -20..20, one float32 step either side of three
    of those, the clamps, FLT_MAX, the smallest subnormal, +Inf, and ten values in mid-binade."""
    f32 = np.float32
    cases = [(0.0, False)]
    for k in range(-20, 21):
        m = f32(fmt_max * 2.0 ** -k)
        cases.append((float(m), False))
        if k in (-20, 0, 13):
            cases += [(float(np.nextafter(m, f32(np.inf))), True), (float(np.nextafter(m, f32(0))), True)]
    cases += [(float(f32(v)), False) for v in (1e-30, 1e30, FLT_MAX, FLT_TINY, math.inf)]
    cases += [(float(f32(v)), False) for v in (1.0, 3.7, 0.013, 12345.6, 2.5e-7, 9.1e8, 0.75, 100.0, 6e-4, 3e12)]
    for m, nb in cases:
        if m > 0 and math.isfinite(m):
            d = _pow2_distance(fmt_max, m)
            # the exactness rule: exact points and everything further than 2^-16 from a power of two
            # must be exact; only the one-step neighbours may use the allowance
            assert (0 < d < 2.0 ** -16) if nb else (d == 0 or d > 2.0 ** -16), (m, d)
    assert 10 * sum(nb for _, nb in cases) < len(cases)  # the allowance: under 10 % of all cases
    return cases


def _raw_exponents(m, nb, fmt_max, margin):
    """Unclamped floor(log2(fmt_max / m)) - margin values the kernel may produce: the exact one, and
    for a one-step neighbour also the adjacent one, provided m * 2^(e + margin) <= fmt_max * (1 + 2^-20)
    (the top value then still rounds to the format's maximum)."""
    raw = fp8_ref.scale_exponent(m, fmt_max, margin, -BIG, BIG)
    out = [raw]
    if nb:
        for e in (raw - 1, raw + 1):
            if Fraction(m) * Fraction(2) ** (e + margin) <= Fraction(fmt_max) * (1 + Fraction(1, 2 ** 20)):
                out.append(e)
    return out


def _fill_amax_row(row, m, slot):
    """The value in one slot; smaller values (or 0) in the others."""
    if math.isinf(m):
        small = _f32_bits(FLT_MAX)
    else:
        small = _f32_bits(np.float32(m) * np.float32(0.5)) if m > 0 else 0
    row[:] = 0
    row[1::3] = small
    row[slot] = _f32_bits(m)


def _chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


@pytest.mark.parametrize("max_drop", [0, 1, 3])
@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("L", [13, 64])
def test_fp8_act_scales_exponents_guard_and_untouched_entries(ops, cuda_device, L, margin, max_drop):
    """scales8[l + 1, 0] == 127 - e and osc[l] == 2^e with e = clamp(max(floor(log2(448 / amax)) - margin,
    e_prev - max_drop), -60, 60) -- +Inf selects -60, the smallest multiplier -- while scales8[:, 1],
    scales8[0, 0] and osc[L - 1] stay and every amax slot is cleared."""
    cases = _amax_cases(448.0)
    clamp = lambda e: max(-60, min(60, e))
    slots = (0, 63, 29)
    for ci, chunk in enumerate(_chunks(cases, L - 1)):
        rows = chunk + [(5.0, False)] * (L - len(chunk))  # row L - 1 has no next layer: only cleared
        amax = np.zeros((L, 64), dtype=np.int32)
        s8 = np.zeros((L, 2), dtype=np.int32)
        s8[:, 1] = 200 + np.arange(L)
        s8[0, 0] = 77
        osc = -1.0 - np.arange(L, dtype=np.float32)
        accepted = []
        for l, (m, nb) in enumerate(rows):
            _fill_amax_row(amax[l], m, slots[(l + ci + margin) % 3])
            if l + 1 == L:
                break
            raws = _raw_exponents(m, nb, 448.0, margin)
            base = clamp(raws[0])
            # previous exponent: held back by the guard / exactly at e_prev - max_drop / rising freely
            e_prev = clamp((base + max_drop + 2, base + max_drop, base - 5)[(l + ci) % 3])
            s8[l + 1, 0] = 127 - e_prev
            guard = (lambda e: max(e, e_prev - max_drop)) if max_drop > 0 else (lambda e: e)
            accepted.append([clamp(guard(e)) for e in raws])
        if max_drop > 0 and ci == 0:  # the three guard situations do occur
            exact = [a[0] for a in accepted]
            prev = [127 - int(v) for v in s8[1:, 0]]
            assert any(e == p - max_drop and e > clamp(_raw_exponents(m, False, 448.0, margin)[0])
                       for e, p, (m, _) in zip(exact, prev, rows))
            assert any(e > p for e, p in zip(exact, prev))
        t_amax = torch.from_numpy(amax).to(cuda_device)
        t_s8 = torch.from_numpy(s8).to(cuda_device)
        t_osc = torch.from_numpy(osc).to(cuda_device)
        ops.fp8_act_scales(t_amax, t_s8, t_osc, margin=margin, max_drop=max_drop)
        torch.cuda.synchronize()
        g8, gosc = t_s8.cpu().numpy(), t_osc.cpu().numpy()
        for l, acc in enumerate(accepted):
            e = 127 - int(g8[l + 1, 0])
            assert e in acc, (rows[l], "margin", margin, "max_drop", max_drop, "got", e, "want", acc)
            assert float(gosc[l]) == 2.0 ** e, (rows[l], float(gosc[l]), e)
        assert np.array_equal(g8[:, 1], s8[:, 1]) and g8[0, 0] == 77 and gosc[L - 1] == osc[L - 1]
        assert (t_amax == 0).all()  # every slot of every row, row L - 1 included


@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("L", [13, 64])
def test_fp8_grad_scales_exponents_and_untouched_entries(ops, cuda_device, L, margin):
    """gscales8[l, 0] == 127 - e and gosc[l] == 2^e for every row, e = clamp(floor(log2(57344 / amax))
    - margin, -100, 100), +Inf selecting -100; gscales8[:, 1] stays and the amax is cleared."""
    cases = _amax_cases(57344.0)
    clamp = lambda e: max(-100, min(100, e))
    slots = (0, 63, 29)
    for ci, chunk in enumerate(_chunks(cases, L)):
        rows = chunk + [(5.0, False)] * (L - len(chunk))
        amax = np.zeros((L, 64), dtype=np.int32)
        s8 = np.zeros((L, 2), dtype=np.int32)
        s8[:, 0] = 50 + np.arange(L)
        s8[:, 1] = 200 + np.arange(L)
        osc = -1.0 - np.arange(L, dtype=np.float32)
        for l, (m, nb) in enumerate(rows):
            _fill_amax_row(amax[l], m, slots[(l + ci + margin) % 3])
        t_amax = torch.from_numpy(amax).to(cuda_device)
        t_s8 = torch.from_numpy(s8).to(cuda_device)
        t_osc = torch.from_numpy(osc).to(cuda_device)
        ops.fp8_grad_scales(t_amax, t_s8, t_osc, margin=margin)
        torch.cuda.synchronize()
        g8, gosc = t_s8.cpu().numpy(), t_osc.cpu().numpy()
        for l, (m, nb) in enumerate(rows):
            acc = [clamp(e) for e in _raw_exponents(m, nb, 57344.0, margin)]
            e = 127 - int(g8[l, 0])
            assert e in acc, (m, "margin", margin, "got", e, "want", acc)
            assert float(gosc[l]) == 2.0 ** e, (m, float(gosc[l]), e)
        assert np.array_equal(g8[:, 1], s8[:, 1])
        assert (t_amax == 0).all()


@pytest.mark.parametrize("op", ["fp8_act_scales", "fp8_grad_scales"])
def test_fp8_scale_kernels_reject_more_than_64_layers(ops, cuda_device, op):
    L = 65
    amax = ops.fp8_amax_buffer(L, cuda_device)
    s8 = torch.full((L, 2), 127, dtype=torch.int32, device=cuda_device)
    osc = torch.ones(L, device=cuda_device)
    with pytest.raises(RuntimeError):
        getattr(ops, op)(amax, s8, osc, margin=1)
    torch.cuda.synchronize()
    assert (s8 == 127).all() and (osc == 1).all()


def test_fp8_weight_scales_edges(ops, cuda_device):
    """All-zero layer, 1 / 3 / 4n+1 elements, a negative max in the last tail element, more than one
    round of the vector loop (> 32768 elements), maxima exactly at 448 * 2^-k, and +Inf."""
    rng = np.random.RandomState(5)

    def layer(n, m, at):
        w = (rng.uniform(-0.5, 0.5, size=n) * abs(m)).astype(np.float32) if math.isfinite(m) else \
            rng.uniform(-1, 1, size=n).astype(np.float32)
        w[at] = m
        return w

    layers = [(np.zeros(1000, dtype=np.float32), 0.0), (np.array([-0.0, 0.0, -0.0], dtype=np.float32), 0.0),
              (layer(1, 3.0, 0), 3.0), (layer(3, -0.02, 1), 0.02), (layer(1001, -7.3, 1000), 7.3),
              (layer(40003, 0.11, 33001), 0.11), (layer(40003, -0.11, 40002), 0.11),
              (layer(70000, 5e-5, 69999), 5e-5), (layer(70001, -5e-5, 8), 5e-5),
              (layer(517, math.inf, 300), math.inf), (layer(40003, -math.inf, 40002), math.inf),
              (layer(2, FLT_MAX, 1), FLT_MAX), (layer(5, FLT_TINY, 4), FLT_TINY)]
    for k in (-20, -8, -1, 0, 1, 5, 8, 9, 12, 20):
        m = float(np.float32(448.0 * 2.0 ** -k))
        layers.append((layer(17 + k % 5, m if k % 2 else -m, (k * 7) % 17), m))
    layers = [(w, float(np.float32(m))) for w, m in layers]  # the max as the float32 the kernel reads
    for _, m in layers:
        if 0 < m < math.inf:
            d = _pow2_distance(448.0, m)
            assert d == 0 or d > 2.0 ** -16  # exact points and mid-binade values only: no allowance
    for chunk in _chunks(layers, 24):  # the kernel's layer table holds 24 entries
        ws = [torch.from_numpy(w).to(cuda_device) for w, _ in chunk]
        L = len(ws)
        wscale = torch.full((L,), -1.0, device=cuda_device)
        s8 = torch.full((L, 2), 99, dtype=torch.int32, device=cuda_device)
        ops.fp8_weight_scales(ws, wscale, s8)
        torch.cuda.synchronize()
        for l, (w, m) in enumerate(chunk):
            assert float(np.abs(w).max()) == m
            e = fp8_ref.scale_exponent(m, 448.0, 0, -60, 60)
            assert int(s8[l, 1]) == 127 - e, (l, m, 127 - int(s8[l, 1]), e)
            assert float(wscale[l]) == 2.0 ** e, (l, m, float(wscale[l]), e)
        assert (s8[:, 0] == 99).all()
        for t, (w, _) in zip(ws, chunk):  # inputs untouched
            assert np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32))


# ----------------------------------------------------------------------------------- weight packs
PACK_SCALE = 16.0
# scaled values (the weights are these / 16): exact ties, +-448, beyond the range, subnormals, +-0
PACK_TABLE = np.array([17.0, 19.0, -17.0, 1.0625, 1.1875, -1.1875, 448.0, -448.0, 464.0, -464.0, 480.0, 1000.0,
                       -1e6, 3e38, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 2.0 ** -9, 5 * 2.0 ** -9,
                       7.5 * 2.0 ** -9, 2.0 ** -11, -(2.0 ** -11), 2.0 ** -6, 0.0, -0.0, 0.3, -7.77, 100.1, 432.0,
                       -440.0, 1e-20], dtype=np.float32) / np.float32(PACK_SCALE)


def _pack_reference(w, scale, transposed, shape):
    """The layout comment above pack_weights_fp8_kernel: out[q][n][b], q = tap * CC + chunk, holds
    e4m3(w[n][chunk * cw + b][kh][kw] * scale) -- transposed: of w'[ci][co][kh][kw] =
    w[co][ci][K-1-kh][K-1-kw] -- and 0 for rows >= the real rows, channels >= the real channels and
    the tail chunks q >= K * K * CC."""
    nch, rows_p, cw = shape
    if transposed:
        w = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    rows, chans, K, _ = w.shape
    CC = (chans + cw - 1) // cw
    with np.errstate(over="ignore"):
        q = fp8_ref.quantize(w * np.float32(scale), "e4m3")
    full = np.zeros((K * K, CC * cw, rows_p), dtype=np.uint8)  # [tap][channel][row]
    full[:, :chans, :rows] = q.transpose(2, 3, 1, 0).reshape(K * K, chans, rows)
    out = np.zeros(shape, dtype=np.uint8)
    out[:K * K * CC] = full.reshape(K * K, CC, cw, rows_p).transpose(0, 1, 3, 2).reshape(K * K * CC, rows_p, cw)
    return out


@pytest.mark.parametrize("Cout,Cin,K,cw32", [(152, 49, 5, 1), (152, 49, 5, 0), (152, 152, 3, 1), (152, 152, 3, 0),
                                             (192, 192, 3, 1)])
def test_pack_weights_fp8_every_byte(ops, cuda_device, monkeypatch, Cout, Cin, K, cw32):
    """pack_weights_fp8 with a host and a device scale and pack_weights_fp8_multi, forward and
    transposed: every byte of the buffer, padding included, from a table of edge values."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_CW32", str(cw32))
    n = Cout * Cin * K * K
    w = PACK_TABLE[(np.arange(n) * 7 + 3) % len(PACK_TABLE)].reshape(Cout, Cin, K, K)
    for v in (0x7E, 0xFE, 0x00, 0x80, 0x01, 0x02):  # saturation, both zeros and subnormals do occur
        assert (fp8_ref.quantize(w * np.float32(PACK_SCALE), "e4m3") == v).any()
    wt = torch.from_numpy(w).to(cuda_device)
    cout_p, cin_p = ops.pad_filters(Cout), (ops.pad_filters(Cin) if Cin > 64 else 64)
    shapes = {False: ops.fp8_weight_shape(K, cin_p, cout_p), True: ops.fp8_weight_shape(K, cout_p, cin_p)}
    assert shapes[False][2] == (32 if cw32 and cin_p == 160 else 64)
    assert shapes[True][2] == (32 if cw32 and cout_p == 160 else 64)
    sc = torch.tensor([3.0, PACK_SCALE, 5.0], device=cuda_device)
    new = lambda tr: torch.full(shapes[tr], 0x55, dtype=torch.uint8, device=cuda_device)
    got = {}
    for tr in (False, True):
        host, dev, multi = new(tr), new(tr), new(tr)
        ops._ops().pack_weights_fp8(wt, host, PACK_SCALE, None, tr)
        ops.pack_weights_fp8_into(wt, dev, sc[1:2], transposed=tr)
        got[tr] = (host, dev, multi)
    ops.pack_weights_fp8_multi([wt, wt], [got[False][2], got[True][2]], sc, [1, 1], [0, 1])
    torch.cuda.synchronize()
    for tr in (False, True):
        want = _pack_reference(w, PACK_SCALE, tr, shapes[tr])
        for name, t in zip(("host scale", "device scale", "multi"), got[tr]):
            g = t.cpu().numpy()
            bad = np.argwhere(g != want)
            assert bad.shape[0] == 0, (name, "transposed" if tr else "forward", bad.shape[0],
                                       [(tuple(i), hex(g[tuple(i)]), hex(want[tuple(i)])) for i in bad[:6]])


# ------------------------------------------------------------------------ conv epilogue saturation
def _overflow_scale(ref_abs, limit):
    """A power of two that takes the 90th percentile of |ref| to `limit` or beyond."""
    q = float(torch.quantile(ref_abs.flatten().float(), 0.9))
    assert q > 0
    return 2.0 ** math.ceil(math.log2(limit / q))


def _assert_saturated(y8, ref, scale, fmt, S):
    """y8: (B, S+2, S+2, Cp) bytes; ref: the bf16 copy.  Where |ref * scale| reaches one format step
    past the maximum the byte is the largest finite one (with ref's sign); no NaN / Inf byte anywhere."""
    step_past, top = (480.0, 0x7E) if fmt == "e4m3" else (65536.0, 0x7B)
    mag = y8 & 0x7F
    assert not (mag > top).any()  # e4m3: 0x7f / 0xff; e5m2: 0x7c..0x7f and 0xfc..0xff
    r = ref[:, 1:S + 1, 1:S + 1, :].float() * scale
    over = r.abs() >= step_past
    assert over.float().mean().item() >= 0.01  # not vacuous
    want = torch.full_like(y8[:, 1:S + 1, 1:S + 1, :], top) | ((r < 0).to(torch.uint8) << 7)
    assert torch.equal(y8[:, 1:S + 1, 1:S + 1, :][over], want[over])
    assert (y8[:, 0] == 0).all() and (y8[:, :, 0] == 0).all() and (y8[:, S + 1] == 0).all()  # borders untouched


def _assert_amax_tracks(amax, ref):
    m = ref.float().abs().max().item()
    assert abs(amax.view(torch.float32).max().item() - m) <= 1e-2 * m


@pytest.mark.parametrize("Cp", [160, 192])
def test_conv_fwd_fp8_epilogue_saturates(ops, cuda_device, monkeypatch, Cp):
    """The setup of test_conv_fwd_fp8_160_byte_outputs at B = 1 with an output scale that overflows:
    0x7e, never 0x7f, from the e4m3-only (LDS-staged) and the two-output epilogue alike."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_CW32", "1")
    S = 19
    x8, w8, bp, scales, osc = _fwd_fp8_160_case(ops, cuda_device, 1, Cp=Cp)
    y8, yb, mbits, amax = _fwd_fp8_160_outputs(ops, cuda_device, 1, "both", Cp=Cp)
    ops.conv_fwd_fp8(x8, w8, bp, scales, osc, 3, S, 1, 1, y_bf16=yb, y_fp8=y8, amax=amax, mbits=mbits)
    torch.cuda.synchronize()
    _assert_amax_tracks(amax, yb)
    scale = _overflow_scale(yb[:, 1:S + 1, 1:S + 1, :].abs(), 480.0)
    big = torch.tensor([scale], device=cuda_device)
    for outs in ("fp8", "both"):
        y8s, ybs, mbs, ams = _fwd_fp8_160_outputs(ops, cuda_device, 1, outs, Cp=Cp)
        ops.conv_fwd_fp8(x8, w8, bp, scales, big, 3, S, 1, 1, y_bf16=ybs, y_fp8=y8s, amax=ams, mbits=mbs)
        torch.cuda.synchronize()
        _assert_saturated(y8s, yb, scale, "e4m3", S)
        _assert_amax_tracks(ams, yb)  # independent of the output scale
        assert torch.equal(mbs, mbits) and (ybs is None or torch.equal(ybs, yb))


def _bf(x):
    return x.to(torch.bfloat16).float()


@pytest.mark.parametrize("C,Cp", [(152, 160), (192, 192)])
def test_conv_dgrad_fp8_epilogue_saturates(ops, cuda_device, monkeypatch, C, Cp):
    """The setup of test_conv_dgrad_fp8 at B = 1 with an overflowing e5m2 output scale: 0x7b / 0xfb,
    never an Inf / NaN byte."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_CW32", "1")
    torch.manual_seed(4)
    B, S, K = 1, 19, 3
    dev = cuda_device
    dz = torch.randn(B, C, S, S, device=dev) * 1e-3
    w = torch.randn(C, C, K, K, device=dev) * 0.05
    yprev = _bf(torch.randn(B, C, S, S, device=dev)).clamp_min(0)
    eg = ops.fp8_exponent(float(dz.abs().max()), margin=0) + 7  # e5m2 max 57344 = 448 * 2^7
    dzp = ops.to_padded(dz, 1, Cp)
    dz8 = torch.empty(dzp.shape, dtype=torch.uint8, device=dev)
    ops.quantize_bf8(dzp, dz8, torch.tensor([2.0 ** eg], device=dev), ops.fp8_amax_buffer(1, dev)[0])
    ew = ops.fp8_exponent(float(w.abs().max()), margin=0)
    w8t = torch.zeros(ops.fp8_weight_shape(K, Cp, Cp), dtype=torch.uint8, device=dev)
    ops.pack_weights_fp8_into(w, w8t, torch.tensor([2.0 ** ew], device=dev), transposed=True)
    scales = torch.tensor([127 - eg, 127 - ew], dtype=torch.int32, device=dev)
    mask = ops.to_padded(yprev, 1, Cp)

    def run(osc):
        amax = ops.fp8_amax_buffer(1, dev)[0]
        dx = ops.padded_empty(B, S, 1, Cp, dev)
        dx8 = torch.zeros((B, S + 2, S + 2, Cp), dtype=torch.uint8, device=dev)
        ops.conv_dgrad_fp8(dz8, w8t, mask, scales, torch.tensor([osc], device=dev), K, S, dx, y_fp8=dx8, amax=amax)
        torch.cuda.synchronize()
        return dx, dx8, amax

    dx, _, amax = run(1.0)
    _assert_amax_tracks(amax, dx)
    scale = _overflow_scale(dx[:, 1:S + 1, 1:S + 1, :].abs(), 65536.0)
    dxs, dx8s, amaxs = run(scale)
    assert torch.equal(dxs, dx)
    _assert_saturated(dx8s, dx, scale, "e5m2", S)
    _assert_amax_tracks(amaxs, dx)  # independent of the output scale


@pytest.mark.parametrize("C,Cp", [(152, 160), (192, 192)])
def test_dgrad_bits_bf8_copy_saturates(ops, cuda_device, C, Cp):
    """The setup of test_dgrad_bits_bf8_copy at B = 1 with an overflowing scale of the e5m2 copy."""
    torch.manual_seed(12)
    B, S, K = 1, 19, 3
    dev = cuda_device
    xin = _bf(torch.randn(B, C, S, S, device=dev))
    w0 = _bf(torch.randn(C, C, K, K, device=dev) * 0.05)
    wp0 = ops.packed_weight_like(w0, Cp, Cp)
    ops.pack_weights([w0], [wp0])
    y = ops.padded_empty(B, S, 1, Cp, dev)
    mbits = torch.zeros(B * (S + 2) ** 2 * ops.mbits_words(Cp), dtype=torch.int32, device=dev)
    ops.conv_fwd(ops.to_padded(xin, 1, Cp), wp0, torch.zeros(Cp, device=dev), y, K, S, 1, 1, mbits=mbits)
    w = _bf(torch.randn(C, C, K, K, device=dev) * 0.05)
    wf, wd = ops.packed_weight_like(w, Cp, Cp), ops.packed_weight_like(w, Cp, Cp, transposed=True)
    ops.pack_weights([w], [wf], [wd])
    dz = ops.to_padded(_bf(torch.randn(B, C, S, S, device=dev) * 1e-3), 1, Cp)

    def run(sc):
        dx = ops.padded_empty(B, S, 1, Cp, dev)
        dx8 = torch.zeros(dx.shape, dtype=torch.uint8, device=dev)
        amax = ops.fp8_amax_buffer(1, dev)[0]
        ops.conv_dgrad_bits_bf8(dz, wd, dx, mbits, dx8, torch.tensor([sc], device=dev), K, S, amax=amax)
        torch.cuda.synchronize()
        return dx, dx8, amax

    dx, _, amax = run(2.0 ** 20)
    _assert_amax_tracks(amax, dx)
    scale = _overflow_scale(dx[:, 1:S + 1, 1:S + 1, :].abs(), 65536.0)
    dxs, dx8s, amaxs = run(scale)
    assert torch.equal(dxs, dx)
    _assert_saturated(dx8s, dx, scale, "e5m2", S)
    _assert_amax_tracks(amaxs, dx)  # independent of the scale of the copy
