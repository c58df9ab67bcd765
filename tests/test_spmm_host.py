"""SpMM's C ABI without a device (include/spmv_hip.h "SpMM"): the four entry points are declared, exported by the normal
and the bounds-checked library and bound in capi; with a NULL handle each one refuses (SPMV_ERR_INVALID, a message that
names it) instead of crashing, and spmv_csr_spmm_plan_bytes returns a negative status."""
import ctypes as C
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SPMM = ("spmv_csr_spmm_plan", "spmv_csr_spmm", "spmv_csr_spmm_plan_bytes", "spmv_csr_spmm_describe")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_spmm_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    for name in SPMM:
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert name in _exports(capi.LIB_PATH), f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in _exports(capi.CHECKED_LIB_PATH), f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
    for m in ("spmm_plan", "spmm", "spmm_describe", "spmm_plan_bytes"):
        assert callable(getattr(capi.CsrMatrix, m, None)), f"CsrMatrix.{m} missing"


def test_spmm_entry_points_refuse_a_null_handle(pkg):
    capi = pkg.capi
    lib = capi.lib()

    def last():
        return lib.spmv_last_error().decode()

    assert lib.spmv_csr_spmm_plan(None, None) == capi.ERR_INVALID
    assert "spmv_csr_spmm_plan" in last()
    assert lib.spmv_csr_spmm(None, 4, None, 4, None, 4, None) == capi.ERR_INVALID
    assert "spmv_csr_spmm" in last()
    assert lib.spmv_csr_spmm_plan_bytes(None) < 0
    assert "spmv_csr_spmm_plan_bytes" in last()
    buf = C.create_string_buffer(64)
    assert lib.spmv_csr_spmm_describe(None, buf, 64) == capi.ERR_INVALID
    assert "spmv_csr_spmm_describe" in last()
