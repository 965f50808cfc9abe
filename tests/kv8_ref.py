"""numpy restatement of the fp8 KV-cache row format (include/awq_hip.h, "fp8 KV cache"), for the tests.

A row is the 128 fp16 values of one (sequence, position, KV head).  Its scale is s = 2^k, k the smallest integer with
amax <= 448 * 2^k (amax = max |x| of the row), taken from the exponent and mantissa bits of amax; its codes are OCP e4m3fn
RNE(x * 2^-k), clamped to +-448.  A row of zeros: s = 0, codes 0.  A row holding a NaN or an inf: s = NaN, codes 0.
Value = code * s; fp16 dequantisation saturates to +-65504."""
import numpy as np


def decode_table():
    """the 256 e4m3fn codes as float64 (0x7F / 0xFF: NaN)"""
    c = np.arange(256)
    sign = np.where(c >> 7, -1.0, 1.0)
    e, m = (c >> 3) & 0xF, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return sign * mag


def rne_e4m3(y):
    """y float64 with |y| <= 448 -> e4m3fn code bytes (round to nearest, ties to even)"""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    _, ex = np.frexp(np.where(a > 0, a, 1.0))    # a = f * 2^ex, f in [0.5, 1)
    step = np.where(a < 2.0 ** -6, 2.0 ** -9, 2.0 ** (ex - 1 - 3))
    q = np.round(a / step) * step                # np.round: half to even
    table = decode_table()
    pos = table[:127]                            # non-negative finite codes 0x00 .. 0x7E, increasing
    idx = np.searchsorted(pos, q)
    assert np.all(pos[idx] == q)
    return (idx | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def row_exponent(amax):
    """k of a finite, positive amax (float32 bits: 448 = 1.75 * 2^8)"""
    u = np.asarray(amax, np.float32).view(np.uint32).astype(np.int64)
    return (u >> 23) - 127 - 8 + ((u & 0x7FFFFF) > 0x600000)


def quantize(x):
    """x [..., D] fp16 -> (codes uint8 [..., D], scales float32 [...])"""
    x = np.asarray(x, np.float16).astype(np.float32)
    amax = np.abs(x).max(axis=-1)
    finite = np.isfinite(x).all(axis=-1)
    live = finite & (amax > 0)
    k = np.where(live, row_exponent(np.where(live, amax, 1.0)), 0)
    y = np.where(live[..., None], x.astype(np.float64) * np.exp2(-k.astype(np.float64))[..., None], 0.0)
    codes = rne_e4m3(np.clip(y, -448.0, 448.0))
    scales = np.where(live, np.exp2(k.astype(np.float64)), np.where(finite, 0.0, np.nan)).astype(np.float32)
    return codes, scales


def dequantize(codes, scales):
    """-> float64 values code * s"""
    return decode_table()[np.asarray(codes, np.int64)] * np.asarray(scales, np.float64)[..., None]


def dequantize_fp16(codes, scales):
    v = dequantize(codes, scales)
    v = np.where(np.abs(v) > 65504.0, np.copysign(65504.0, v), v)
    return v.astype(np.float16)


def fake_quant(x):
    """fp16 rows -> the fp16 rows an fp8 cache hands prefill (quantize, then dequantize)"""
    return dequantize_fp16(*quantize(x))
