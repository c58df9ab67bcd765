"""SpMM and SDDMM on 16-bit matrices, without a device (include/spmv_hip.h "SpMM and SDDMM on 16-bit matrices"): the two
symbols are declared, covered by exports.map, exported by the normal and the bounds-checked library and bound with an int
dtype after the handle and void pointers for the dense matrices; a null handle and a bad dtype are refused under the
function's name before anything touches a device; the CsrMatrix methods refuse mixed and foreign dtypes before they reach the
library; the header states the rounding contract; and tests/_round16.py, the integer-code conversions the device tests judge
the kernels by, agrees with torch's CPU conversions on special values and on 10^5 random fp32 bit patterns."""
import ctypes as C
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _round16 as R

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_spmm_16", "spmv_csr_sddmm_16")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_symbols_declared_listed_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    exports_map = (ROOT / "spmv-test_amd" / "csrc" / "exports.map").read_text()
    listed = re.findall(r"[\w*]+(?=;)", exports_map.split("global:")[1].split("local:")[0])
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name in NAMES:
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in listed), f"{name} not covered by exports.map"
        assert name in normal, f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in checked, f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert hasattr(capi.lib(), name)
        fp32 = capi.SIGNATURES[name[:-3]][1]
        args = capi.SIGNATURES[name][1]
        # the handle, then an int dtype, then exactly the arguments of the fp32 call
        assert args[0] == fp32[0] and args[1] is C.c_int and args[2:] == fp32[1:], name
        decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1)
        params = [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
        assert len(params) == len(args) and params[1] == "int dtype" and params[2] == "int k", params
        for p in params:
            if re.search(r"\bd_(X|Y|U)$", p):
                assert p.startswith(("const void *", "void *")), p
            if p.endswith("d_out"):
                assert p == "float *d_out", p


def test_null_handle_and_bad_dtype_are_refused_by_name(pkg):
    """(The handle of the dtype cases is made of zeros and must never be read: the refusal comes before that.)"""
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    fake = (C.c_char * 4096)()
    calls = {
        "spmv_csr_spmm_16": lambda h, dt: lib.spmv_csr_spmm_16(h, dt, 4, p, 4, p, 4, None),
        "spmv_csr_sddmm_16": lambda h, dt: lib.spmv_csr_sddmm_16(h, dt, 4, p, 4, p, 4, p, None),
    }
    for name, call in calls.items():
        assert call(None, capi.ATTN_BF16) == capi.ERR_INVALID
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":") and "null handle" in msg, msg
        for dtype in (capi.ATTN_FP32, 3, -1, 16):
            assert call(C.addressof(fake), dtype) == capi.ERR_INVALID
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and "dtype" in msg, msg


def test_methods_refuse_mixed_and_foreign_dtypes(pkg):
    import torch
    capi = pkg.capi
    m = capi.CsrMatrix.__new__(capi.CsrMatrix)           # (no handle: the checks come first)
    m._h, m._keep, m.rows, m.cols, m.nnz = C.c_void_p(), (), 5, 7, 0
    z = lambda n, w, dt: torch.zeros((n, w), dtype=dt)      # noqa: E731
    bf, hf, f32, f64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
    out = torch.zeros(0)
    for a, b in ((bf, hf), (hf, bf), (bf, f32), (f32, hf), (f64, f64), (f32, f64), (hf, f64)):
        with pytest.raises(ValueError, match="spmm: "):
            m.spmm(z(7, 8, a), z(5, 8, b))
        with pytest.raises(ValueError, match="sddmm: "):
            m.sddmm(z(5, 8, a), z(7, 8, b), out)
    for dt in (bf, hf):
        with pytest.raises(ValueError, match="out must be a contiguous 1-D float32 tensor"):
            m.sddmm(z(5, 8, dt), z(7, 8, dt), out.to(dt))
    with pytest.raises(ValueError, match="spmm: X must be a 2-D float32 tensor"):       # the fp32 message, as before
        m.spmm(z(7, 8, f64), z(5, 8, f32))
    SL = pkg.sparse_layer
    for dt in (bf, hf):
        t = torch.zeros((6, 9), dtype=dt)[:, 1:]                  # rows of 9 elements from an odd one: not 8-byte aligned
        c = SL._operand(t, "X", 6)
        assert c.dtype == dt and c.data_ptr() % 8 == 0 and c.stride(1) == 1 and torch.equal(c, t)
        with pytest.raises(ValueError, match="dY is"):
            SL._operand(torch.zeros((6, 8), dtype=f32), "dY", 6, like=c)
    with pytest.raises(ValueError):
        SL._operand(torch.zeros((6, 8), dtype=f64), "X", 6)
    with pytest.raises(ValueError):
        SL._operand(torch.zeros((6, 65), dtype=bf), "X", 6)
    m._h = C.c_void_p()


def test_header_states_the_rounding_contract():
    flat = re.sub(r"[\s*]+", " ", (ROOT / "include" / "spmv_hip.h").read_text())
    text = flat[flat.index("SpMM and SDDMM on 16-bit matrices"):flat.index("int spmv_csr_spmm_16")]
    assert "widened exactly to fp32 where it enters an fma" in text
    assert "rounded to the dtype once, to nearest even, at its store" in text
    assert "Nothing is accumulated in 16 bits and vals is never rounded" in text
    assert "bit for bit, the round-to-nearest-even conversion to the dtype of what spmv_csr_spmm writes" in text
    assert "Batch invariance carries over" in text and "never written" in text and "never read into a sum" in text
    assert "d_out holds the bits of spmv_csr_sddmm on U and X widened to fp32" in text
    assert "No conversion flushes a subnormal" in text and "NaN of the dtype" in text and "overflows to +-Inf" in text
    assert "counts ELEMENTS" in text and "8-byte aligned" in text and "SPMV_ATTN_FP32 is refused" in text
    assert "SPMV_ERR_NOT_PLANNED" in text and "graph-capturable" in text
    limits = flat[flat.index("Limits of the layouts"):flat.index("int spmv_csr_plan(")]
    assert "spmv_csr_spmm_16, spmv_csr_sddmm_16" in limits


# ---- tests/_round16.py against torch's CPU conversions ------------------------------------------------------------------------
def _torch_dtype(fmt):
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]


def _torch_convert(fmt, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(_torch_dtype(fmt)).view(torch.int16).numpy().view(np.uint16)


def _torch_widen(fmt, h):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(h, np.uint16).view(np.int16)).view(_torch_dtype(fmt))
    return t.to(torch.float32).numpy()


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


SPECIAL = {
    # (fp32 input, the bits it must become)
    "bf16": [(0.0, 0x0000), (-0.0, 0x8000),
             (_f(0x00400000), 0x0040), (_f(0x00010000), 0x0001), (_f(0x00008000), 0x0000), (_f(0x00018000), 0x0002),   # subnormals, two ties
             (_f(0x00008001), 0x0001), (_f(0x00000001), 0x0000),
             (1.0 + 2.0 ** -8, 0x3f80), (1.0 + 2.0 ** -7 + 2.0 ** -8, 0x3f82),                       # ties to an even / from an odd neighbour
             (1.0 + 2.0 ** -8 + 2.0 ** -23, 0x3f81), (_f(0x7f7fffff), 0x7f80), (np.inf, 0x7f80), (-np.inf, 0xff80)],
    "fp16": [(0.0, 0x0000), (-0.0, 0x8000),
             (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000), (1.5 * 2.0 ** -24, 0x0002), (0.75 * 2.0 ** -24, 0x0001),   # subnormals, two ties
             (2.0 ** -25 * (1 + 2.0 ** -23), 0x0001), (1023.5 * 2.0 ** -24, 0x0400), (_f(0x00000001), 0x0000),
             (_f(0x00400000), 0x0000), (-(2.0 ** -24), 0x8001),
             (1.0 + 2.0 ** -11, 0x3c00), (1.0 + 2.0 ** -10 + 2.0 ** -11, 0x3c02), (1.0 + 2.0 ** -11 + 2.0 ** -23, 0x3c01),
             (65504.0, 0x7bff), (65519.996, 0x7bff), (65520.0, 0x7c00), (-65520.0, 0xfc00), (1e30, 0x7c00), (np.inf, 0x7c00)],
}


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_round16_special_values(fmt):
    x = np.array([np.float32(v) for v, _ in SPECIAL[fmt]], np.float32)
    want = np.array([b for _, b in SPECIAL[fmt]], np.uint16)
    got = R.convert(fmt, x)
    assert np.array_equal(got, want), [(float(v), hex(g), hex(w)) for v, g, w in zip(x, got, want) if g != w]
    assert np.array_equal(got, _torch_convert(fmt, x))
    # NaN stays NaN with its sign, quiet or signalling, and nothing else becomes one
    nans = _f([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff])
    h = R.convert(fmt, nans)
    assert R.is_nan(fmt, h).all() and np.array_equal(h >> 15, nans.view(np.uint32) >> 31)
    assert R.is_nan(fmt, _torch_convert(fmt, nans)).all() and not R.is_nan(fmt, got).any()
    assert np.isnan(R.widen(fmt, h)).all()
    # truncation toward zero: never above the magnitude, the neighbour below where the number is not representable
    t = R.convert(fmt, x, nearest=False)
    finite = np.isfinite(x)
    assert np.all(np.abs(R.widen(fmt, t)[finite]) <= np.abs(x[finite]))
    assert np.all(np.abs(R.widen(fmt, t)[finite]) <= np.abs(R.widen(fmt, got)[finite]))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_round16_agrees_with_torch_on_random_bit_patterns(fmt):
    rng = np.random.Generator(np.random.PCG64(1600 + len(fmt)))
    u = rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    # a share of them inside the format's range, where the fractions and the subnormals are: the same sign and fraction bits
    # with the exponent drawn from the format's own
    lo, hi = (0, 255) if fmt == "bf16" else (127 - 26, 127 + 17)
    e = rng.integers(lo, hi, size=u.size // 2, dtype=np.uint64).astype(np.uint32)
    u[: e.size] = (u[: e.size] & np.uint32(0x807fffff)) | (e << np.uint32(23))
    x = u.view(np.float32)
    got, want = R.convert(fmt, x), _torch_convert(fmt, x)
    assert R.same(fmt, got, want), int(np.sum(got != want))
    assert np.array_equal(R.is_nan(fmt, got), np.isnan(x))
    # every bit pattern of the format widens exactly as torch widens it, and comes back as itself
    h = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    w, tw = R.widen(fmt, h), _torch_widen(fmt, h)
    ok = ~R.is_nan(fmt, h)
    assert np.array_equal(w.view(np.uint32)[ok], tw.view(np.uint32)[ok]) and np.isnan(w[~ok]).all() and np.isnan(tw[~ok]).all()
    assert np.array_equal(R.convert(fmt, w)[ok], h[ok]) and np.array_equal(R.convert(fmt, w, nearest=False)[ok], h[ok])
    # truncation is the neighbour toward zero: equal to the nearest conversion or one step below it in magnitude
    t = R.convert(fmt, x, nearest=False)
    fin = np.isfinite(x)
    d = (got[fin] & np.uint16(0x7fff)).astype(np.int32) - (t[fin] & np.uint16(0x7fff)).astype(np.int32)
    assert np.all((d == 0) | (d == 1)) and np.array_equal(got[fin] >> 15, t[fin] >> 15)
    assert np.all(np.abs(R.widen(fmt, t[fin]).astype(np.float64)) <= np.abs(x[fin].astype(np.float64)))
