"""SpMM and SDDMM at any k, without a device (include/spmv_hip.h "SpMM and SDDMM at any k"): the three symbols are declared,
covered by exports.map, exported by both libraries and bound; a null handle is refused under the function's name; SparseLayer
checks its k_max argument before it touches a device; and every mistake of tests/_cols.py that can change bits does change
bits on the data tests/test_gpu_cols.py runs, so that test tells the documented order from each of them."""
import ctypes as C
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _cols as CO

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_spmm_plan_cols", "spmv_csr_spmm_cols", "spmv_csr_sddmm_cols")


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
        assert name in normal and name in checked, f"{name} not exported"
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name), f"{name} not bound"
    # the run calls take the _16 calls' arguments (an int dtype after the handle, void pointers for the dense matrices)
    for what in ("spmm", "sddmm"):
        assert capi.SIGNATURES[f"spmv_csr_{what}_cols"] == capi.SIGNATURES[f"spmv_csr_{what}_16"]
    assert capi.SIGNATURES["spmv_csr_spmm_plan_cols"][1][1] is C.c_int
    assert re.search(r"#define\s+SPMV_COLS_MAX_K\s+65536\b", header) and capi.COLS_MAX_K == 65536
    for method in ("spmm_plan_cols", "spmm_cols", "sddmm_cols"):
        assert callable(getattr(capi.CsrMatrix, method))


def test_null_handle_and_bad_dtype_are_refused_by_name(pkg):
    """(The handle of the dtype cases is made of zeros and must never be read: the refusal comes before that.)"""
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    fake = (C.c_char * 4096)()
    calls = {
        "spmv_csr_spmm_plan_cols": lambda h, dt: lib.spmv_csr_spmm_plan_cols(h, 128, None),
        "spmv_csr_spmm_cols": lambda h, dt: lib.spmv_csr_spmm_cols(h, dt, 4, p, 4, p, 4, None),
        "spmv_csr_sddmm_cols": lambda h, dt: lib.spmv_csr_sddmm_cols(h, dt, 4, p, 4, p, 4, p, None),
    }
    for name, call in calls.items():
        assert call(None, capi.ATTN_FP32) == capi.ERR_INVALID
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":") and "null handle" in msg, msg
        if name.endswith("plan_cols"):
            continue
        for dtype in (3, -1, 16):
            assert call(C.addressof(fake), dtype) == capi.ERR_INVALID
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and "dtype" in msg, msg
    for k_max in (0, -3, 65537):
        assert lib.spmv_csr_spmm_plan_cols(C.addressof(fake), k_max, None) == capi.ERR_INVALID
        msg = lib.spmv_last_error().decode()
        assert msg.startswith("spmv_csr_spmm_plan_cols:") and "k_max" in msg, msg


def test_sparse_layer_checks_k_max_without_a_device(pkg):
    import inspect
    SL = pkg.sparse_layer
    assert inspect.signature(SL.SparseLayer.__init__).parameters["k_max"].default is None
    for bad in (0, -1, 65537, 64.0, "128", True):
        with pytest.raises(ValueError, match="k_max"):
            SL.SparseLayer(4, 4, None, None, None, k_max=bad)       # (refused before any array is looked at)
    import torch
    assert SL.MAX_K == 64
    wide = torch.zeros((6, 65))
    with pytest.raises(ValueError, match="65 columns"):
        SL._operand(wide, "X", 6)                                   # the default layer's refusal, as before
    assert SL._operand(wide, "X", 6, max_k=192) is wide
    with pytest.raises(ValueError, match="193 columns"):
        SL._operand(torch.zeros((6, 193)), "X", 6, max_k=192)


def test_methods_check_their_tensors_before_the_library(pkg):
    import torch
    capi = pkg.capi
    m = capi.CsrMatrix.__new__(capi.CsrMatrix)           # (no handle: the checks come first)
    m._h, m._keep, m.rows, m.cols, m.nnz = C.c_void_p(), (), 5, 7, 0
    z = lambda n, w, dt: torch.zeros((n, w), dtype=dt)      # noqa: E731
    out = torch.zeros(0)
    for a, b in ((torch.bfloat16, torch.float16), (torch.float32, torch.float16), (torch.float64, torch.float64)):
        with pytest.raises(ValueError, match="spmm_cols: "):
            m.spmm_cols(z(7, 130, a), z(5, 130, b))
        with pytest.raises(ValueError, match="sddmm_cols: "):
            m.sddmm_cols(z(5, 130, a), z(7, 130, b), out)
    with pytest.raises(ValueError, match="do not fit"):
        m.spmm_cols(z(7, 130, torch.float32), z(5, 129, torch.float32))
    with pytest.raises(ValueError, match="do not fit"):
        m.sddmm_cols(z(5, 130, torch.float32), z(7, 129, torch.float32), out)
    with pytest.raises(ValueError, match="out must be"):
        m.sddmm_cols(z(5, 130, torch.float32), z(7, 130, torch.float32), out.to(torch.float64))


# ---- the mistakes of tests/_cols.py change bits on the device tests' data -------------------------------------------------------
def _differ(a, b):
    return int(np.sum(a.view(np.uint32) != b.view(np.uint32)))


@pytest.mark.parametrize("name", ("P1", "P2"))
def test_the_fold_order_shows_from_three_tiles_on(name):
    for k in (65, 130, 192):
        parts = [CO.tile_reference(name, a, b) for a, b in CO.tiles(k)]
        assert len(parts) == (k + 63) // 64
        right, back = CO.fold(parts), CO.fold(parts, "reversed")
        n = _differ(right, back)
        print(f"{name} k={k}: the reversed fold changes {n} of {right.size} results")
        if len(parts) < 3:
            assert n == 0, "two tiles: the same sum in either order"
        else:
            assert n >= 1000, f"{name}, k = {k}: only {n} results tell the fold's order"
        # and a fold from +0 changes nothing on data without a -0 (it is told apart below)
        assert _differ(right, CO.fold(parts, "from_zero")) == 0


@pytest.mark.parametrize("name", ("P1", "P2"))
def test_carried_partials_and_a_wide_butterfly_change_bits(name):
    k = 130
    s, _, U, X = CO.data(name)
    U, X = U[:, :k], X[:, :k]
    right = CO.sddmm_reference(name, k)
    assert np.array_equal(right.view(np.uint32), CO.sddmm(s.rp, s.ci, U, X).view(np.uint32))
    for wrong in ("carried", "butterfly_128"):
        got = CO.sddmm(s.rp, s.ci, U, X, wrong=wrong)
        n = _differ(right, got)
        print(f"{name} k={k}: {wrong} changes {n} of {right.size} results")
        assert n >= 1000, f"{wrong}: only {n} results differ"
        assert np.allclose(got, right, rtol=1e-4, atol=1e-4), "a mistake of the order keeps the values"


def test_a_fold_from_plus_zero_loses_minus_zero():
    k = 128
    s, _, U, X = CO.data("P2")
    U, X = U[:, :k].copy(), X[:, :k].copy()
    where = CO.minus_zero(s, U, X)
    assert where.size >= 6
    parts = CO.tile_results(s.rp, s.ci, U, X)
    right, zero = CO.fold(parts), CO.fold(parts, "from_zero")
    assert (right.view(np.uint32)[where] == 0x80000000).all(), "every tile of these rows gives -0 and so does their fold"
    assert (zero.view(np.uint32)[where] == 0).all()
    assert _differ(right, zero) == where.size
