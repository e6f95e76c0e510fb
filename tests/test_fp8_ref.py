"""The software fp8 reference (tests/fp8_ref.py) against itself and against torch's CPU float8 casts:
it is what tests/test_fp8_numerics.py holds the HIP kernels to, so it is pinned without a GPU."""
import math

import numpy as np
import pytest
import torch

import fp8_ref

SCALES = [2.0 ** -20, 2.0 ** -8, 1.0, 2.0 ** 7, 2.0 ** 20, 2.0 ** 100, 1.7, 0.3]
TORCH_DTYPE = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def test_decode_known_values():
    assert fp8_ref.decode("e4m3", 0x7E) == 448.0 and fp8_ref.decode("e4m3", 0xFE) == -448.0
    assert fp8_ref.decode("e4m3", 0x01) == 2.0 ** -9 and fp8_ref.decode("e4m3", 0x08) == 2.0 ** -6
    assert fp8_ref.decode("e4m3", 0x38) == 1.0 and fp8_ref.decode("e4m3", 0x78) == 256.0
    assert math.isnan(fp8_ref.decode("e4m3", 0x7F)) and math.isnan(fp8_ref.decode("e4m3", 0xFF))
    assert fp8_ref.decode("e5m2", 0x7B) == 57344.0 and fp8_ref.decode("e5m2", 0x01) == 2.0 ** -16
    assert fp8_ref.decode("e5m2", 0x3C) == 1.0 and fp8_ref.decode("e5m2", 0x04) == 2.0 ** -14
    assert fp8_ref.decode("e5m2", 0x7C) == math.inf and fp8_ref.decode("e5m2", 0xFC) == -math.inf
    assert all(math.isnan(fp8_ref.decode("e5m2", b)) for b in (0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF))
    z = fp8_ref.decode("e4m3", 0x80)
    assert z == 0.0 and math.copysign(1.0, z) == -1.0


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_decode_matches_torch_for_every_byte(fmt):
    b = torch.arange(256, dtype=torch.uint8)
    t = b.view(TORCH_DTYPE[fmt]).float().numpy()
    ours = np.array([fp8_ref.decode(fmt, int(x)) for x in b], dtype=np.float32)
    assert np.array_equal(np.isnan(t), np.isnan(ours))
    ok = ~np.isnan(t)
    assert np.array_equal(t[ok].view(np.uint32), ours[ok].view(np.uint32))  # the sign of zero too


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_round_trip_every_finite_byte(fmt):
    top = fp8_ref.FORMATS[fmt][3]
    finite = [b for b in range(256) if (b & 0x7F) <= top]
    assert len(finite) == 2 * (top + 1)
    vals = np.array([fp8_ref.decode(fmt, b) for b in finite], dtype=np.float32)
    assert np.array_equal(fp8_ref.quantize(vals, fmt), np.array(finite, dtype=np.uint8))


def test_quantize_ties_saturation_and_signed_zero():
    q = lambda v, fmt="e4m3": int(fp8_ref.quantize(np.float32(v), fmt))
    assert q(17.0) == q(16.0) and q(19.0) == q(20.0)  # ties between 16, 18, 20 go to the even code
    assert q(2.0 ** -10) == 0x00 and q(3 * 2.0 ** -10) == 0x02 and q(-(2.0 ** -10)) == 0x80
    assert q(464.0) == 0x7E and q(1e9) == 0x7E and q(-1e9) == 0xFE and q(math.inf) == 0x7E
    assert q(-0.0) == 0x80 and q(0.0) == 0x00 and q(-1e-30) == 0x80
    assert q(61440.0, "e5m2") == 0x7B and q(-math.inf, "e5m2") == 0xFB and q(2.0 ** -17, "e5m2") == 0x00
    assert q(3 * 2.0 ** -17, "e5m2") == 0x02 and q(1.125, "e5m2") == 0x3C and q(1.375, "e5m2") == 0x3E
    with pytest.raises(ValueError):
        fp8_ref.quantize(np.float32(math.nan), "e4m3")


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("scale", SCALES)
def test_quantize_bf16_matches_torch_cpu_cast(fmt, scale):
    """All 65536 bf16 patterns (NaNs replaced by 0, +-Inf kept) byte for byte."""
    bits = np.arange(65536, dtype=np.uint16)
    x = fp8_ref.bf16_to_f32(bits)
    bits = np.where(np.isnan(x), 0, bits).astype(np.uint16)
    got, lut = fp8_ref.quantize_bf16(bits, scale, fmt)
    assert lut.shape == (65536,) and np.array_equal(got, lut[bits])
    mx = fp8_ref.FMT_MAX[fmt]
    xt = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).float()
    ref = (xt * torch.tensor(scale, dtype=torch.float32)).clamp(-mx, mx).to(TORCH_DTYPE[fmt]).view(torch.uint8).numpy()
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert ((got & 0x7F) == fp8_ref.FORMATS[fmt][3]).sum() > 1000  # saturation is exercised


@pytest.mark.parametrize("fmt_max,lo,hi", [(448.0, -60, 60), (57344.0, -100, 100)])
def test_scale_exponent_at_and_around_binade_boundaries(fmt_max, lo, hi):
    f32 = np.float32
    for k in range(-40, 41):
        m = f32(fmt_max * 2.0 ** -k)  # fmt_max / m == 2^k exactly
        up, dn = np.nextafter(m, f32(np.inf)), np.nextafter(m, f32(0))
        for margin in (0, 1, 2):
            clamp = lambda e: max(lo, min(hi, e))
            assert fp8_ref.scale_exponent(m, fmt_max, margin, lo, hi) == clamp(k - margin)
            assert fp8_ref.scale_exponent(dn, fmt_max, margin, lo, hi) == clamp(k - margin)
            assert fp8_ref.scale_exponent(up, fmt_max, margin, lo, hi) == clamp(k - 1 - margin)
            e = fp8_ref.scale_exponent(up, fmt_max, margin, -10 ** 6, 10 ** 6)
            assert float(up) * 2.0 ** (e + margin) <= fmt_max < float(up) * 2.0 ** (e + margin + 1)


def test_scale_exponent_special_values():
    assert fp8_ref.scale_exponent(0.0, 448.0, 1, -60, 60) == 0
    assert fp8_ref.scale_exponent(math.inf, 448.0, 1, -60, 60) == -60
    assert fp8_ref.scale_exponent(math.inf, 57344.0, 0, -100, 100) == -100
    assert fp8_ref.scale_exponent(1e30, 448.0, 0, -60, 60) == -60 and fp8_ref.scale_exponent(1e-30, 448.0, 0, -60, 60) == 60
    tiny, big = float(np.float32(2.0 ** -149)), float(np.finfo(np.float32).max)
    assert fp8_ref.scale_exponent(tiny, 448.0, 0, -1000, 1000) == 157  # 448 = 1.75 * 2^8
    assert fp8_ref.scale_exponent(big, 448.0, 0, -1000, 1000) == -120  # 448 / (2 - 2^-23) / 2^127
    assert fp8_ref.scale_exponent(3.0, 448.0, 1, -60, 60) == 6  # 149.3 -> 2^7, one bit of headroom
    with pytest.raises(ValueError):
        fp8_ref.scale_exponent(-1.0, 448.0, 0, -60, 60)
