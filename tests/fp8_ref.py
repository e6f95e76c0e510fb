"""Software reference of the two 8-bit float formats the fp8 kernels write, and of the delayed-scale
exponent rule: plain numpy / Python from the bit layouts, no torch float8 cast inside.

"e4m3" is OCP e4m3fn (bias 7, subnormals at exponent 0, no Inf, 0x7f / 0xff NaN, max 448 = 0x7e);
"e5m2" has bias 15, 0x7c Inf, 0x7d..0x7f NaN, max 57344 = 0x7b.  Every code value and every float32
is dyadic, so the float64 comparisons below are exact.
"""
import math
from fractions import Fraction

import numpy as np

FORMATS = {
    # exponent bits, mantissa bits, bias, largest finite byte
    "e4m3": (4, 3, 7, 0x7E),
    "e5m2": (5, 2, 15, 0x7B),
}
FMT_MAX = {"e4m3": 448.0, "e5m2": 57344.0}
NAN_BYTE = 0x7F  # a NaN pattern in both formats (the lookup tables' entry for NaN inputs)


def decode(fmt, byte):
    """Value of one byte: float, +-inf or nan."""
    ebits, mbits, bias, _ = FORMATS[fmt]
    byte = int(byte) & 0xFF
    sign = -1.0 if byte & 0x80 else 1.0
    e = (byte >> mbits) & ((1 << ebits) - 1)
    m = byte & ((1 << mbits) - 1)
    if fmt == "e4m3":
        if e == 15 and m == 7:
            return math.nan
    elif e == 31:
        return sign * math.inf if m == 0 else math.nan
    if e == 0:
        return sign * math.ldexp(m, 1 - bias - mbits)
    return sign * math.ldexp((1 << mbits) + m, e - bias - mbits)


def finite_codes(fmt):
    """float64 values of the finite non-negative bytes 0 .. max byte (ascending: the byte is the index)."""
    return np.array([decode(fmt, b) for b in range(FORMATS[fmt][3] + 1)], dtype=np.float64)


def quantize(v_f32, fmt):
    """Bytes of float32 values: |v| clamped to the format's maximum, round to nearest with ties to the
    even code, sign bit from signbit(v) (-0 and negatives that round to zero give 0x80).  No NaN."""
    v = np.asarray(v_f32, dtype=np.float32)
    if np.isnan(v).any():
        raise ValueError("quantize: NaN input is not defined")
    codes = finite_codes(fmt)
    a = np.minimum(np.abs(v).astype(np.float64), codes[-1])
    hi = np.searchsorted(codes, a, side="left")  # codes[hi - 1] < a <= codes[hi]
    lo = np.maximum(hi - 1, 0)
    mid = 0.5 * (codes[lo] + codes[hi])  # exact: a few mantissa bits each
    pick_hi = (a > mid) | ((a == mid) & (hi % 2 == 0))
    q = np.where(pick_hi, hi, lo).astype(np.uint8)
    return q | (np.signbit(v).astype(np.uint8) << 7)


def bf16_to_f32(bits_u16):
    return (np.asarray(bits_u16).astype(np.uint32) << 16).view(np.float32)


_LUT = {}


def bf16_lut(scale_f32, fmt):
    """uint8[65536]: the byte of every bf16 bit pattern at this scale (NaN patterns hold NAN_BYTE)."""
    key = (np.float32(scale_f32).tobytes(), fmt)
    if key not in _LUT:
        x = bf16_to_f32(np.arange(65536, dtype=np.uint32))
        nan = np.isnan(x)
        with np.errstate(over="ignore", under="ignore"):
            v = np.where(nan, np.float32(0), x) * np.float32(scale_f32)  # one float32 rounding
        lut = quantize(v, fmt)
        lut[nan] = NAN_BYTE
        lut.setflags(write=False)
        _LUT[key] = lut
    return _LUT[key]


def quantize_bf16(bits_u16, scale_f32, fmt):
    """(bytes, lut): quantize(float32(bf16) * float32(scale)) -- the product rounded once to float32,
    as the kernels compute it -- and the 65536-entry table it was gathered from."""
    lut = bf16_lut(scale_f32, fmt)
    return lut[np.asarray(bits_u16).astype(np.int64) & 0xFFFF], lut


def floor_log2_ratio(fmt_max, m):
    """Exact floor(log2(fmt_max / m)) of two finite positive floats."""
    fa, ea = math.frexp(fmt_max)  # fa, fm in [0.5, 1): the ratio of the two lies in (0.5, 2)
    fm, em = math.frexp(m)
    return ea - em - (0 if Fraction(fa) >= Fraction(fm) else 1)


def scale_exponent(m, fmt_max, margin, lo, hi):
    """clamp(floor(log2(fmt_max / m)) - margin, lo, hi); m == 0 gives 0 (nothing seen: multiplier 1),
    m == +Inf gives lo (the smallest multiplier)."""
    m = float(m)
    if m < 0 or math.isnan(m):
        raise ValueError("scale_exponent: amax must be >= 0")
    if m == 0:
        return 0
    if math.isinf(m):
        return lo
    return max(lo, min(hi, floor_log2_ratio(float(fmt_max), m) - margin))
