"""Selection without a device (include/spmv_hip.h "selection"): the seven entry points are declared, exported by the normal
and the bounds-checked library and bound in capi; null handles are refused under each function's name; the numpy statement
of the contract (tests/_select.py) agrees with a naive row-by-row one; the key map is strictly monotone; the two Python
layers refuse bad arguments before any device call."""
import ctypes as C
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _select as S

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_select_topk", "spmv_csr_select_threshold", "spmv_csr_select_values", "spmv_csr_select_gather",
         "spmv_csr_select_scatter", "spmv_csr_select_map_bytes", "spmv_csr_copy_arrays")
METHODS = ("select_topk", "select_threshold", "select_values", "select_gather", "select_scatter", "select_map_bytes", "copy_arrays")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_select_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    globs = re.findall(r"global:\s*([^;]+);", (ROOT / "spmv-test_amd" / "csrc" / "exports.map").read_text())
    patterns = [p for g in globs for p in g.split()]
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name in NAMES:
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), f"{name} not a global of exports.map"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert name in normal, f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in checked, f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
    for m in METHODS:
        assert callable(getattr(capi.CsrMatrix, m, None)), f"CsrMatrix.{m} missing"
    assert re.search(r"enum\s*\{\s*SPMV_SELECT_ABS\s*=\s*1\s*\}", header) and capi.CsrMatrix.SELECT_ABS == 1
    assert header.index("---- the transpose") < header.index("---- selection") < header.index("---- the hot path")


def test_select_entry_points_refuse_null_handles(pkg):
    capi = pkg.capi
    lib = capi.lib()

    def refused(rc, name):
        assert rc == capi.ERR_INVALID, name
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":"), msg

    out = C.c_void_p()
    dummy = C.create_string_buffer(64)
    refused(lib.spmv_csr_select_topk(None, None, 4, 0, 0, None, C.byref(out)), "spmv_csr_select_topk")
    assert out.value is None
    refused(lib.spmv_csr_select_topk(C.addressof(dummy), None, 4, 0, 0, None, None), "spmv_csr_select_topk")
    refused(lib.spmv_csr_select_threshold(None, None, 0.5, 0, 0, None, C.byref(out)), "spmv_csr_select_threshold")
    assert out.value is None
    refused(lib.spmv_csr_select_threshold(C.addressof(dummy), None, 0.5, 0, 0, None, None), "spmv_csr_select_threshold")
    refused(lib.spmv_csr_select_values(None, None, None), "spmv_csr_select_values")
    refused(lib.spmv_csr_select_gather(None, 1, None, 0, None, 0, None), "spmv_csr_select_gather")
    refused(lib.spmv_csr_select_scatter(None, 1, None, 0, None, 0, None), "spmv_csr_select_scatter")
    assert lib.spmv_csr_select_map_bytes(None) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_select_map_bytes:")
    refused(lib.spmv_csr_copy_arrays(None, None, None, None, None), "spmv_csr_copy_arrays")


def test_key_map_is_strictly_monotone():
    sub = S.SUBNORMAL
    floats = np.array([-np.inf, -S.FLT_MAX, -1e30, -2.5, -1.0000001, -1.0, -1e-30, -1.1754944e-38, -4 * sub, -sub,
                       0.0, sub, 4 * sub, 1.1754944e-38, 1e-30, 1.0, 1.0000001, 2.5, 1e30, S.FLT_MAX, np.inf], np.float32)
    assert np.all(np.diff(floats.astype(np.float64)) > 0)
    k = S.keys(floats).astype(np.int64)
    assert np.all(np.diff(k) > 0)
    assert S.keys(np.array([-0.0], np.float32))[0] == S.keys(np.array([0.0], np.float32))[0] == 0x80000000
    nan_keys = S.keys(S.SPECIAL[:4])
    assert np.all(nan_keys == 0) and k.min() > 0            # every number, -Inf included, ranks above every NaN
    # abs: |s| decides, the sign does not
    assert np.array_equal(S.keys(floats, abs_=True), S.keys(np.abs(floats)))
    assert np.array_equal(S.keys(floats), np.array([S._naive_key(x, False) for x in floats], np.uint32))
    assert np.array_equal(S.keys(S.SPECIAL, True), np.array([S._naive_key(x, True) for x in S.SPECIAL], np.uint32))


def test_vectorised_emulation_equals_the_naive_one():
    rng = np.random.default_rng(20240611)
    for case in range(200):
        rows = int(rng.integers(0, 9))
        cols = int(rng.integers(1, 40))
        lengths = rng.integers(0, 24, rows)
        if case % 7 == 0 and rows:
            lengths[rng.integers(0, rows)] = 0
        rp, ci = S.random_csr(rng, rows, cols, lengths, sorted_rows=case % 2 == 0)
        nnz = int(rp[-1])
        vals = S.special_scores(rng, nnz)
        if case % 5 == 0:
            score = np.full(nnz, np.float32(0.75))                   # all ties
        elif case % 5 == 1:
            score = None                                             # the matrix's own values
        else:
            score = S.special_scores(rng, nnz)
        abs_ = bool(case % 3 == 0)
        k = int(rng.choice([1, 2, 3, 5, 8, 23, 24, 2 ** 31 - 1]))
        a = S.host_select_topk(rows, rp, ci, vals, k, score, abs_)
        b = S.naive_select(rows, rp, ci, vals, k=k, score=score, abs_=abs_)
        assert S.same(a, b), f"topk case {case}"
        assert np.array_equal(np.diff(a[0]), np.minimum(np.diff(rp), k))
        for thr in (-np.inf, -0.0, 0.0, 0.25, 2.0, S.FLT_MAX, np.inf, float(S.SUBNORMAL)):
            a = S.host_select_threshold(rows, rp, ci, vals, thr, score, abs_)
            b = S.naive_select(rows, rp, ci, vals, threshold=thr, score=score, abs_=abs_)
            assert S.same(a, b), f"threshold case {case} thr {thr}"
        # the copy case: k >= the longest row
        a = S.host_select_topk(rows, rp, ci, vals, 24, score, abs_)
        assert S.same(a, (rp, ci, vals, np.arange(nnz, dtype=np.uint32)))


def test_threshold_is_a_comparison_of_keys():
    """What the kernels rely on: s >= t  <=>  key(s) >= key(t) for every non-NaN t."""
    rng = np.random.default_rng(5)
    s = np.concatenate([S.SPECIAL, rng.standard_normal(200).astype(np.float32)])
    for t in np.concatenate([S.SPECIAL[4:], s[12:40]]):
        with np.errstate(invalid="ignore"):
            want = s >= t
        assert np.array_equal(S.keys(s) >= S.keys(np.array([t], np.float32))[0], want)
        with np.errstate(invalid="ignore"):
            want = np.abs(s) >= t
        assert np.array_equal(S.keys(s, True) >= S.keys(np.array([t], np.float32))[0], want)


def test_layers_refuse_bad_arguments_before_any_device_call(pkg):
    import torch
    SL, SA, capi = pkg.sparse_layer, pkg.sparse_attention, pkg.capi
    layer = SL.SparseLayer.__new__(SL.SparseLayer)           # no handle: a call that reached the library would fail otherwise
    for bad in (0, -3, 2.5, True, None, "4"):
        with pytest.raises(ValueError, match="SparseLayer.pruned"):
            layer.pruned(bad)
    A = capi.CsrMatrix.__new__(capi.CsrMatrix)
    A._h, A._keep, A.rows, A.cols, A.nnz = C.c_void_p(), (), 4, 6, 5
    Q, K = torch.zeros(4, 8), torch.zeros(6, 8)
    for bad in (0, -1, 1.5, False, None):
        with pytest.raises(ValueError, match="topk_pattern: k"):
            SA.topk_pattern(A, Q, K, bad)
    with pytest.raises(ValueError, match="topk_pattern: A"):
        SA.topk_pattern(object(), Q, K, 2)
    with pytest.raises(ValueError, match="scale"):
        SA.topk_pattern(A, Q, K, 2, scale=float("nan"))
    with pytest.raises(ValueError, match="Q and K"):
        SA.topk_pattern(A, None, K, 2)
    with pytest.raises(ValueError, match="Q has 3 rows"):
        SA.topk_pattern(A, torch.zeros(3, 8), K, 2)
    with pytest.raises(ValueError, match="K has 4 columns"):
        SA.topk_pattern(A, Q, torch.zeros(6, 4), 2)
    with pytest.raises(ValueError, match="columns"):
        SA.topk_pattern(A, torch.zeros(4, 65), torch.zeros(6, 65), 2)
    # the CsrMatrix methods' own checks
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="select_topk: k"):
            A.select_topk(bad)
    with pytest.raises(ValueError, match="NaN"):
        A.select_threshold(float("nan"))
    with pytest.raises(ValueError, match="score must be"):
        A.select_topk(2, score=torch.zeros(5))               # not a device tensor
    with pytest.raises(ValueError, match="not made by select"):
        A.select_gather(torch.zeros(5), torch.zeros(5))
