"""The fused attention calls that run all heads of one pattern in one launch, without a device (include/spmv_hip.h "Fused
attention, all heads of one pattern in one launch"): the four symbols are declared, exported by the normal and the
bounds-checked library and bound with the right argument counts; spmv_attn_heads_t is 88 bytes on both sides; a null handle
and a null hs are refused under the function's name; CsrMatrix has the four methods; the holder knows heads="loop" and
heads="batched" and nothing else; the header's limits paragraph names the new calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"spmv_csr_attention_plan_heads": 3, "spmv_csr_attention_max_heads": 3, "spmv_csr_attention_forward_heads": 15,
         "spmv_csr_attention_backward_q_heads": 20, "spmv_csr_attention_backward_kv_heads": 20}      # name -> number of arguments
SINGLE = {"spmv_csr_attention_forward_heads": "spmv_csr_attention_forward",
          "spmv_csr_attention_backward_q_heads": "spmv_csr_attention_backward_q",
          "spmv_csr_attention_backward_kv_heads": "spmv_csr_attention_backward_kv"}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_heads_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert name in normal, f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in checked, f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
    for name, single in SINGLE.items():       # hs, then exactly the arguments of the single-head call after h
        args, one = capi.SIGNATURES[name][1], capi.SIGNATURES[single][1]
        assert args[0] is one[0] and args[1] is C.POINTER(capi.AttnHeads) and args[2:] == one[1:]
    for method in ("attention_plan_heads", "attention_max_heads", "attention_forward_heads", "attention_backward_q_heads", "attention_backward_kv_heads"):
        assert callable(getattr(capi.CsrMatrix, method, None)), f"CsrMatrix.{method} missing"


def test_heads_structure_is_88_bytes_on_both_sides(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.AttnHeads) == 88
    assert [n for n, _ in capi.AttnHeads._fields_] == ["heads", "reserved", "q", "k", "v", "o", "d_o", "stats", "delta", "dq", "dk", "dv"]
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    body = re.search(r"typedef struct spmv_attn_heads \{(.*?)\} spmv_attn_heads_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, [n.strip() for n in names.split(",")]) for t, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body)]
    assert fields == [("int32_t", ["heads", "reserved"]), ("int64_t", ["q", "k", "v", "o", "d_o", "stats", "delta", "dq", "dk", "dv"])]


def test_heads_calls_refuse_a_null_handle_and_a_null_hs(pkg):
    """Both refusals come before anything touches a device: a handle that is not null but is never dereferenced before the
    null hs is found would be a bug of its own, so the null-hs case passes a handle made of zeros that is only ever compared
    with NULL."""
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    hs = capi.AttnHeads(heads=1)
    fake = (C.c_char * 4096)()                 # stands for a handle; the null hs must be refused before it is read
    calls = {
        "spmv_csr_attention_forward_heads": lambda h, s: lib.spmv_csr_attention_forward_heads(
            h, s, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, None),
        "spmv_csr_attention_backward_q_heads": lambda h, s: lib.spmv_csr_attention_backward_q_heads(
            h, s, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, 4, p, p, p, 4, None),
        "spmv_csr_attention_backward_kv_heads": lambda h, s: lib.spmv_csr_attention_backward_kv_heads(
            h, s, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, p, p, 4, p, 4, None),
    }
    for name, call in calls.items():
        assert call(None, C.byref(hs)) == capi.ERR_INVALID
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":") and "null handle" in msg, msg
        assert call(C.addressof(fake), None) == capi.ERR_INVALID
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":") and "null hs" in msg, msg
    assert lib.spmv_csr_attention_max_heads(None, 8, 8) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_attention_max_heads:")
    assert lib.spmv_csr_attention_plan_heads(None, 2, None) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_attention_plan_heads:")
    for heads in (0, -1, 65536):
        assert lib.spmv_csr_attention_plan_heads(C.addressof(fake), heads, None) == capi.ERR_INVALID
        assert lib.spmv_last_error().decode().startswith("spmv_csr_attention_plan_heads: heads")


def test_fused_holder_knows_loop_and_batched_only(pkg):
    import inspect
    sa = pkg.sparse_attention
    sig = inspect.signature(sa.FusedSparseAttention.__init__)
    assert sig.parameters["heads"].default == "loop", "the default must stay the loop over the heads"
    with pytest.raises(ValueError, match="heads"):
        sa.FusedSparseAttention(4, 4, None, None, heads="other")       # (refused before the pattern is looked at)


def test_header_limits_paragraph_names_the_heads_calls():
    flat = re.sub(r"\s+", " ", (ROOT / "include" / "spmv_hip.h").read_text())
    limits = flat[flat.index("Limits of the layouts"):flat.index("tests/test_gpu_limits.py")]
    assert "spmv_csr_attention_forward_heads" in limits and "_backward_q_heads" in limits and "_backward_kv_heads" in limits
    assert "heads < 2^32" in limits and "heads <= 65535" in limits
