"""The sparse product without a device (include/spmv_hip.h "the sparse product"): the three entry points are declared,
exported by the normal and the bounds-checked library and bound in capi, with the class boundaries in one constant; null
handles are refused under each function's name; the numpy statement of the contract (tests/_spgemm.py) agrees with a naive
triple loop over dense float64 operands; the order-sensitive inputs of the GPU tests distinguish the contract's order from two
wrong ones; SparseLayer.composed refuses bad arguments before any device call."""
import ctypes as C
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _spgemm as G

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_spgemm", "spmv_csr_spgemm_values", "spmv_csr_spgemm_plan_bytes")
METHODS = ("spgemm", "spgemm_values", "spgemm_plan_bytes")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_spgemm_symbols_declared_exported_and_bound(pkg):
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
    slots = re.search(r"#define\s+SPMV_SPGEMM_CLASS_SLOTS\s+([0-9,\s]+?)\s*(/\*|\n)", header)
    assert slots, "SPMV_SPGEMM_CLASS_SLOTS not defined in include/spmv_hip.h"
    from_header = tuple(int(v) for v in slots.group(1).split(","))
    assert isinstance(capi.SPGEMM_CLASS_SLOTS, tuple) and capi.SPGEMM_CLASS_SLOTS == from_header
    assert len(from_header) >= 2 and all(x < y for x, y in zip(from_header, from_header[1:]))
    assert "SPMV_SPGEMM_CLASS_SLOTS" in (ROOT / "spmv-test_amd" / "csrc" / "kernels_spgemm.hip").read_text()
    assert header.index("---- selection") < header.index("---- the sparse product") < header.index("---- the hot path")


def test_spgemm_entry_points_refuse_null_handles(pkg):
    capi = pkg.capi
    lib = capi.lib()

    def refused(rc, name):
        assert rc == capi.ERR_INVALID, name
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":"), msg

    dummy = C.create_string_buffer(1024)
    for a, b, with_out in ((None, None, True), (C.addressof(dummy), None, True), (None, C.addressof(dummy), True),
                           (C.addressof(dummy), C.addressof(dummy), False)):
        out = C.c_void_p()
        refused(lib.spmv_csr_spgemm(a, b, 0, None, C.byref(out) if with_out else None, None), "spmv_csr_spgemm")
        assert out.value is None
    for c, a, b in ((None, None, None), (C.addressof(dummy), None, None), (C.addressof(dummy), C.addressof(dummy), None),
                    (None, C.addressof(dummy), C.addressof(dummy))):
        refused(lib.spmv_csr_spgemm_values(c, a, b, None), "spmv_csr_spgemm_values")
    assert lib.spmv_csr_spgemm_plan_bytes(None) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_spgemm_plan_bytes:")


def test_contract_agrees_with_a_dense_triple_loop():
    rng = np.random.default_rng(31)
    for case in range(40):
        m, n, p = (int(rng.integers(0, 9)) for _ in range(3))
        (_, _, a), (_, _, b) = G.random_matrix(rng, m, n, 7), G.random_matrix(rng, n, p, 7)
        if case % 4 == 0 and a[2].size:
            a[2][rng.integers(0, a[2].size)] = 0.0                   # a stored zero counts as a nonzero
        rp, ci, va, products = G.spgemm(a, b)
        pat, val, mag = G.naive_dense(m, n, p, a, b)
        assert products == int(sum(b[0][c + 1] - b[0][c] for c in a[1]))
        assert rp.shape == (m + 1,) and rp[0] == 0 and np.array_equal(np.diff(rp), pat.sum(axis=1))
        for i in range(m):
            cols = ci[rp[i]:rp[i + 1]]
            assert np.array_equal(cols, np.flatnonzero(pat[i])), f"case {case} row {i}"       # ascending, once each
            err = np.abs(va[rp[i]:rp[i + 1]].astype(np.float64) - val[i, cols])
            assert np.all(err <= 1e-6 * mag[i, cols]), f"case {case} row {i}: {err.max()}"
        for wrong in G.WRONG:                                        # another order: the same pattern, close values
            w = G.spgemm(a, b, wrong=wrong)
            assert np.array_equal(w[0], rp) and np.array_equal(w[1], ci) and w[3] == products
            dense = val[np.repeat(np.arange(m), np.diff(rp)), ci] if ci.size else np.zeros(0)
            assert np.all(np.abs(w[2].astype(np.float64) - dense) <= 1e-6 * (mag[np.repeat(np.arange(m), np.diff(rp)), ci] if ci.size else 0))


def test_structural_pattern_keeps_cancelled_and_zero_entries():
    a = (np.array([0, 2, 3], np.int32), np.array([0, 0, 1], np.int32), np.array([1.0, -1.0, 0.0], np.float32))
    b = (np.array([0, 1, 2], np.int32), np.array([2, 0], np.int32), np.array([3.0, -0.0], np.float32))
    rp, ci, va, products = G.spgemm(a, b)
    assert rp.tolist() == [0, 1, 2] and ci.tolist() == [2, 0] and products == 3
    assert va.view(np.uint32).tolist() == [0, 0]                     # 3 - 3 = +0; fma(0, -0, +0) = +0


@pytest.mark.parametrize("name", sorted(G.ORDER_CASES))
def test_order_sensitive_inputs_distinguish_the_orders(name):
    (_, _, a), (_, _, b) = G.ORDER_CASES[name]()
    right = G.spgemm(a, b)
    for wrong in G.WRONG:
        other = G.spgemm(a, b, wrong=wrong)
        assert np.array_equal(other[0], right[0]) and np.array_equal(other[1], right[1])
        assert G.differs(right, other) >= 1, f"{name}: the order {wrong} gives the contract's bits"


def test_edge_cases_have_the_rows_they_claim(pkg):
    for T in pkg.capi.SPGEMM_CLASS_SLOTS:
        (_, _, a), (_, _, b), spec = G.edge_case(T)
        rp, _, _, products = G.spgemm(a, b)
        terms = [int(sum(b[0][c + 1] - b[0][c] for c in a[1][a[0][r]:a[0][r + 1]])) for r in range(len(spec))]
        assert terms == [t for t, _ in spec] and np.diff(rp).tolist() == [d for _, d in spec] and products == sum(terms)
        assert (T, T) in spec and (T + 1, T + 1) in spec and (T - 1, T - 1) in spec


def test_composed_refuses_bad_arguments_before_any_device_call(pkg):
    SL = pkg.sparse_layer
    capi = pkg.capi

    def layer(rows, cols):
        l = SL.SparseLayer.__new__(SL.SparseLayer)               # no handle: a call that reached the library would fail otherwise
        l.A = capi.CsrMatrix.__new__(capi.CsrMatrix)
        l.A._h, l.A._keep, l.A.rows, l.A.cols, l.A.nnz = C.c_void_p(), (), rows, cols, 0
        l.k_max, l.vals = None, None
        return l

    second = layer(64, 48)
    for bad in (None, 3, "layer", object()):
        with pytest.raises(ValueError, match="SparseLayer.composed: first must be"):
            second.composed(bad)
    with pytest.raises(ValueError, match="SparseLayer.composed: self is 64 x 48, first is 40 x 48"):
        second.composed(layer(40, 48))
    A = second.A
    with pytest.raises(TypeError, match="spgemm: b must be"):
        A.spgemm(None)
    with pytest.raises(ValueError, match="spgemm: self is 64 x 48"):
        A.spgemm(layer(40, 48).A)
