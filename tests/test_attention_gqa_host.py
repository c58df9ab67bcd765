"""The fused attention calls for grouped-query heads, without a device (include/spmv_hip.h "Fused attention, grouped-query
heads"): the three symbols are declared, exported by the normal and the bounds-checked library and bound with the _heads
signature plus an int group after hs; a null handle, a null hs, a group below 1 and a head count the group does not divide
are refused under the function's name before anything touches a device; spmv_attn_heads_t is still 88 bytes; CsrMatrix has
the three methods and they, like the holder, say what a grouped call is; the header states the order of the sum over the
heads of a group."""
import ctypes as C
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADS = {"spmv_csr_attention_forward_gqa": "spmv_csr_attention_forward_heads",
         "spmv_csr_attention_backward_q_gqa": "spmv_csr_attention_backward_q_heads",
         "spmv_csr_attention_backward_kv_gqa": "spmv_csr_attention_backward_kv_heads"}
NARGS = {"spmv_csr_attention_forward_gqa": 16, "spmv_csr_attention_backward_q_gqa": 21, "spmv_csr_attention_backward_kv_gqa": 21}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_gqa_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name, heads in HEADS.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert name in normal, f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in checked, f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
        args, one = capi.SIGNATURES[name][1], capi.SIGNATURES[heads][1]
        assert len(args) == NARGS[name]
        # h, hs, then an int group, then exactly the arguments of the _heads call after hs
        assert args[:2] == one[:2] and args[2] is C.c_int and args[3:] == one[2:]
        # the declaration in the header: `int group` right after hs
        decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1)
        params = [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
        assert len(params) == NARGS[name] and params[1] == "const spmv_attn_heads_t *hs" and params[2] == "int group", params[:3]
    assert C.sizeof(capi.AttnHeads) == 88, "spmv_attn_heads_t is unchanged"


def test_gqa_calls_refuse_null_pointers_and_bad_groups_before_any_device(pkg):
    """(The handle of the later cases is made of zeros and must never be read: every refusal here comes before that.)"""
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    fake = (C.c_char * 4096)()
    calls = {
        "spmv_csr_attention_forward_gqa": lambda h, s, g: lib.spmv_csr_attention_forward_gqa(
            h, s, g, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, None),
        "spmv_csr_attention_backward_q_gqa": lambda h, s, g: lib.spmv_csr_attention_backward_q_gqa(
            h, s, g, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, 4, p, p, p, 4, None),
        "spmv_csr_attention_backward_kv_gqa": lambda h, s, g: lib.spmv_csr_attention_backward_kv_gqa(
            h, s, g, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, p, p, 4, p, 4, None),
    }
    six = capi.AttnHeads(heads=6)
    for name, call in calls.items():
        def refused(h, s, g, word):
            assert call(h, s, g) == capi.ERR_INVALID
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, msg

        refused(None, C.byref(six), 2, "null handle")
        refused(C.addressof(fake), None, 2, "null hs")
        refused(C.addressof(fake), C.byref(six), 0, "group")
        refused(C.addressof(fake), C.byref(six), -3, "group")
        refused(C.addressof(fake), C.byref(six), 4, "group")                    # 6 % 4 != 0
        refused(C.addressof(fake), C.byref(capi.AttnHeads(heads=6, reserved=1)), 2, "reserved")
        refused(C.addressof(fake), C.byref(capi.AttnHeads(heads=0)), 1, "heads")


def test_gqa_methods_and_holder_say_what_a_grouped_call_is(pkg):
    capi, sa = pkg.capi, pkg.sparse_attention
    for method in ("attention_forward_gqa", "attention_backward_q_gqa", "attention_backward_kv_gqa"):
        f = getattr(capi.CsrMatrix, method, None)
        assert callable(f), f"CsrMatrix.{method} missing"
        doc = re.sub(r"\s+", " ", f.__doc__ or "")
        assert "grouped-query" in doc and "H_kv" in doc, f"CsrMatrix.{method} does not describe the grouped case"
    doc = re.sub(r"\s+", " ", sa.FusedSparseAttention.__doc__)
    assert "Grouped-query heads" in doc and "H % H_kv == 0" in doc and "(H_kv, cols, width)" in doc
    assert "head order" in doc and "ValueError" in doc


def test_header_states_the_head_order_contract():
    flat = re.sub(r"[\s*]+", " ", (ROOT / "include" / "spmv_hip.h").read_text())
    text = flat[flat.index("Fused attention, grouped-query heads"):flat.index("int spmv_csr_attention_forward_gqa")]
    assert "query head y uses K/V head y / g" in text
    assert "dK_c = (..((dK^(0) + dK^(1)) + dK^(2)) .. + dK^(g-1))" in text
    assert "in head order, starting from head 0's value and not from +0" in text
    assert "not a sum over the heads inside a piece" in text
    assert "group = 1 is the _heads call bit for bit" in text and "group = 1 is therefore the _heads call bit for bit" in text
    assert "A key no query lists gets +0" in text
    assert "SPMV_ERR_NOT_PLANNED" in text and "hs->heads % group != 0" in text and "group < 1" in text
    assert "88 bytes" in text
