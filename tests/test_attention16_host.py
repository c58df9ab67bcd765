"""The fused attention calls on 16-bit matrices, without a device (include/spmv_hip.h "Fused attention on 16-bit matrices"):
the three symbols are declared, exported by the normal and the bounds-checked library and bound with the _gqa signature plus
an int dtype after group and void pointers for the matrices; a null handle, a null hs, a bad group and a bad dtype are refused
under the function's name before anything touches a device; the CsrMatrix methods refuse matrices of mixed dtypes by name
before they reach the library; the holder pads to four elements of any dtype; the header states the rounding contract."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GQA = {"spmv_csr_attention_forward_16": "spmv_csr_attention_forward_gqa",
       "spmv_csr_attention_backward_q_16": "spmv_csr_attention_backward_q_gqa",
       "spmv_csr_attention_backward_kv_16": "spmv_csr_attention_backward_kv_gqa"}
NARGS = {"spmv_csr_attention_forward_16": 17, "spmv_csr_attention_backward_q_16": 22, "spmv_csr_attention_backward_kv_16": 22}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_16bit_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name, gqa in GQA.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert name in normal, f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in checked, f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
        args, one = capi.SIGNATURES[name][1], capi.SIGNATURES[gqa][1]
        assert len(args) == NARGS[name]
        # h, hs, group, then an int dtype, then exactly the arguments of the _gqa call after group
        assert args[:3] == one[:3] and args[3] is C.c_int and args[4:] == one[3:]
        decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1)
        params = [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
        assert len(params) == NARGS[name] and params[2] == "int group" and params[3] == "int dtype", params[:4]
        # every matrix is a void pointer, stats and delta stay float
        for p in params:
            if re.search(r"\bd_(Q|K|V|O|dO|dQ|dK|dV)$", p):
                assert p.startswith(("const void *", "void *")), p
            if re.search(r"\bd_(stats|delta)$", p):
                assert p.startswith(("const float *", "float *")), p
    assert re.search(r"enum\s*\{\s*SPMV_ATTN_BF16\s*=\s*1\s*,\s*SPMV_ATTN_FP16\s*=\s*2\s*\}", header)
    assert (capi.ATTN_BF16, capi.ATTN_FP16) == (1, 2)


def test_16bit_calls_refuse_null_pointers_bad_groups_and_bad_dtypes_before_any_device(pkg):
    """(The handle of the later cases is made of zeros and must never be read: every refusal here comes before that.)"""
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    fake = (C.c_char * 4096)()
    calls = {
        "spmv_csr_attention_forward_16": lambda h, s, g, dt: lib.spmv_csr_attention_forward_16(
            h, s, g, dt, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, None),
        "spmv_csr_attention_backward_q_16": lambda h, s, g, dt: lib.spmv_csr_attention_backward_q_16(
            h, s, g, dt, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, 4, p, p, p, 4, None),
        "spmv_csr_attention_backward_kv_16": lambda h, s, g, dt: lib.spmv_csr_attention_backward_kv_16(
            h, s, g, dt, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, p, p, 4, p, 4, None),
    }
    six = capi.AttnHeads(heads=6)
    for name, call in calls.items():
        def refused(h, s, g, dt, word):
            assert call(h, s, g, dt) == capi.ERR_INVALID
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, msg

        refused(None, C.byref(six), 2, capi.ATTN_BF16, "null handle")
        refused(C.addressof(fake), None, 2, capi.ATTN_FP16, "null hs")
        refused(C.addressof(fake), C.byref(six), 0, capi.ATTN_BF16, "group")
        refused(C.addressof(fake), C.byref(six), 4, capi.ATTN_FP16, "group")                    # 6 % 4 != 0
        refused(C.addressof(fake), C.byref(capi.AttnHeads(heads=6, reserved=1)), 2, capi.ATTN_BF16, "reserved")
        for dtype in (0, 3, -1, 16):
            refused(C.addressof(fake), C.byref(six), 2, dtype, "dtype")


def test_methods_refuse_mixed_dtypes_by_name(pkg):
    """The nine methods route matrices that are all bfloat16 or all float16 to the _16 calls; a matrix of another dtype than Q's
    is a ValueError that names it, raised before the library is called (the handle here is never used)."""
    import torch
    capi = pkg.capi
    m = capi.CsrMatrix.__new__(capi.CsrMatrix)           # (no handle: the checks come first)
    m._h, m._keep, m.rows, m.cols, m.nnz = C.c_void_p(), (), 5, 7, 0
    z = lambda n, w, dt: torch.zeros((n, w), dtype=dt)      # noqa: E731
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    stats, delta = torch.zeros((5, 2)), torch.zeros(5)
    with pytest.raises(ValueError, match=r"attention_forward: V is torch\.float16"):
        m.attention_forward(z(5, 8, bf), z(7, 8, bf), z(7, 8, hf), z(5, 8, bf), stats)
    with pytest.raises(ValueError, match=r"attention_forward: O is torch\.float32"):
        m.attention_forward(z(5, 8, hf), z(7, 8, hf), z(7, 8, hf), z(5, 8, f32), stats)
    with pytest.raises(ValueError, match=r"attention_backward_q: dO is torch\.bfloat16"):
        m.attention_backward_q(z(5, 8, hf), z(7, 8, hf), z(7, 8, hf), z(5, 8, hf), z(5, 8, bf), stats, delta, z(5, 8, hf))
    with pytest.raises(ValueError, match=r"attention_backward_kv: dK is torch\.float32"):
        m.attention_backward_kv(z(7, 8, bf), z(5, 8, bf), z(5, 8, bf), z(7, 8, bf), torch.zeros((7, 2)), torch.zeros(7),
                                z(5, 8, f32), z(5, 8, bf))
    # fp32 Q with a 16-bit partner: the existing message, which names the operand
    with pytest.raises(ValueError, match="attention_forward: K must be a 2-D float32 tensor"):
        m.attention_forward(z(5, 8, f32), z(7, 8, bf), z(7, 8, f32), z(5, 8, f32), stats)
    # 16-bit stats are out of scope: stats and delta are float32 in every call
    with pytest.raises(ValueError, match="stats must be a contiguous float32 tensor"):
        m.attention_forward(z(5, 8, bf), z(7, 8, bf), z(7, 8, bf), z(5, 8, bf), stats.to(bf))
    # the 3-D methods alike
    z3 = lambda h, n, w, dt: torch.zeros((h, n, w), dtype=dt)      # noqa: E731
    with pytest.raises(ValueError, match=r"attention_forward_gqa: K is torch\.float32"):
        m.attention_forward_gqa(z3(4, 5, 8, bf), z3(2, 7, 8, f32), z3(2, 7, 8, bf), z3(4, 5, 8, bf), torch.zeros((4, 5, 2)))
    with pytest.raises(ValueError, match=r"attention_forward_heads: O is torch\.bfloat16"):
        m.attention_forward_heads(z3(4, 5, 8, hf), z3(4, 7, 8, hf), z3(4, 7, 8, hf), z3(4, 5, 8, bf), torch.zeros((4, 5, 2)))
    m._h = C.c_void_p()


def test_holder_pads_rows_to_four_elements_of_the_dtype(pkg):
    import torch
    sa = pkg.sparse_attention
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        t = sa._heads_empty(3, 5, 6, "cpu", dt)
        assert t.dtype == dt and t.shape == (3, 5, 6) and t.stride() == (40, 8, 1)
    assert sa._heads_empty(2, 3, 5, "cpu").dtype == torch.float32
    doc = re.sub(r"\s+", " ", sa.FusedSparseAttention.__doc__)
    assert "torch.bfloat16" in doc and "torch.float16" in doc and "stats and delta stay float32" in doc
    with pytest.raises(ValueError, match="float32"):
        sa._operand(torch.zeros((4, 8), dtype=torch.bfloat16), "Q", 4)           # the composed holder stays fp32 only


def test_header_states_the_rounding_contract():
    flat = re.sub(r"[\s*]+", " ", (ROOT / "include" / "spmv_hip.h").read_text())
    text = flat[flat.index("Fused attention on 16-bit matrices"):flat.index("int spmv_csr_attention_forward_16")]
    assert "widened exactly to fp32 where it is used" in text
    assert "rounded to the dtype once, to nearest even, at its store" in text
    assert "Nothing is accumulated in 16 bits" in text
    assert "bit for bit, the round-to-nearest-even conversion to dtype of what the matching _gqa fp32 call writes on the same operands widened to fp32" in text
    assert "stats and delta are that call's bits" in text
    assert "backward_q forms delta from the 16-bit O it is given" in text
    assert "No conversion flushes a subnormal" in text and "NaN of the dtype" in text and "overflows to +-Inf" in text
    assert "counts ELEMENTS" in text and "8-byte aligned" in text and "no multiple of 4 elements" in text
    assert "SPMV_ERR_NOT_PLANNED" in text and "graph-capturable" in text
