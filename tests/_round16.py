"""bf16 and fp16 as bits, in integer code (host only, numpy): exact widening to fp32 and the conversion of fp32 to either
format, to nearest even (the contract of the _16 calls) or truncated toward zero (what a test's teeth are measured against).

No conversion flushes a subnormal of either format; fp16 overflows to +-Inf from 65520 on; a NaN becomes a quiet NaN of the
format with the sign kept (compare NaNs with is_nan: payloads are unspecified).  tests/test_spmm16_host.py checks all of it
against torch's CPU conversions."""
import numpy as np

u16, u32, u64, f32 = np.uint16, np.uint32, np.uint64, np.float32
FORMATS = ("bf16", "fp16")


def _bits32(x):
    return np.ascontiguousarray(x, f32).view(u32)


def widen(fmt, h):
    """The fp32 numbers (exactly) of the bits h of format fmt."""
    h = np.ascontiguousarray(h, u16).astype(u32)
    if fmt == "bf16":
        return (h << u32(16)).view(f32)
    assert fmt == "fp16"
    sign, e, m = (h >> u32(15)) << u32(31), (h >> u32(10)) & u32(31), h & u32(1023)
    normal = ((e + u32(112)) << u32(23)) | (m << u32(13))
    special = u32(0x7f800000) | (m << u32(13))                                   # Inf, or a NaN with its payload
    # a subnormal m 2^-24, m < 2^10, with leading bit p: 1.f x 2^(p - 24)
    p = np.zeros_like(m)
    for b in range(1, 10):
        p = np.where(m >> u32(b) != 0, u32(b), p)
    sub = ((p + u32(103)) << u32(23)) | ((m << (u32(23) - p)) & u32(0x7fffff))
    out = np.where(e == 31, special, np.where(e != 0, normal, np.where(m != 0, sub, u32(0))))
    return (sign | out).astype(u32).view(f32)


def convert(fmt, x, nearest=True):
    """The bits of format fmt (uint16) of the fp32 numbers x: to nearest even, or (nearest=False) truncated toward zero."""
    u = _bits32(x)
    a = u & u32(0x7fffffff)
    nan = a > u32(0x7f800000)
    if fmt == "bf16":
        r = (u + u32(0x7fff) + ((u >> u32(16)) & u32(1))) >> u32(16) if nearest else u >> u32(16)
        return np.where(nan, (u >> u32(16)) | u32(0x40), r).astype(u16)
    assert fmt == "fp16"
    sign = (u >> u32(16)) & u32(0x8000)
    # results that are normal in fp16 (|x| >= 2^-14): 13 bits of the fraction go; a carry out of the fraction raises the
    # exponent, and past 65504 (to nearest: from 65520 on) lands on Inf's bits by itself
    b = (a.astype(u64) - u64(112 << 23)) & u64(0xffffffff)
    big = ((b + u64(0xfff) + ((b >> u64(13)) & u64(1))) >> u64(13) if nearest else b >> u64(13)).astype(u32)
    big = np.where(a >= u32(0x7f800000), u32(0x7c00), np.minimum(big, u32(0x7c00) if nearest else u32(0x7bff)))
    # below 2^-14 the result is the integer |x| 2^24 = m 2^(e - 126), m the 24-bit significand
    e = a >> u32(23)
    m = ((a & u32(0x7fffff)) | u32(0x800000)).astype(u64)
    shift = np.minimum(u64(126) - np.minimum(e, u32(112)).astype(u64), u64(40))      # >= 14; from 25 on the result is 0
    q, rem, half = m >> shift, m & ((u64(1) << shift) - u64(1)), u64(1) << (shift - u64(1))
    if nearest:
        q = q + ((rem > half) | ((rem == half) & ((q & u64(1)) == 1))).astype(u64)
    small = np.where(e == 0, u32(0), q.astype(u32))                                   # (an fp32 subnormal is below 2^-126)
    out = np.where(a >= u32(0x38800000), big, small)
    return (sign | np.where(nan, u32(0x7e00), out)).astype(u16)


def is_nan(fmt, h):
    h = np.ascontiguousarray(h, u16)
    if fmt == "bf16":
        return (h & u16(0x7fff)) > u16(0x7f80)
    return (h & u16(0x7fff)) > u16(0x7c00)


def same(fmt, a, b):
    """Bit for bit, a NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, u16), np.ascontiguousarray(b, u16)
    return bool(np.all((a == b) | (is_nan(fmt, a) & is_nan(fmt, b))))
