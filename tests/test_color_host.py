"""The multicolour ordering without a device (include/spmv_hip.h "the multicolour ordering").

  (a) the numpy contract of tests/_color.py yields a proper colouring of at most max degree + 1 colours on every shared pattern,
      with the colours, rounds and class sizes recorded below (recomputed here, never trusted);
  (b) on the permuted matrices each triangle has at most as many levels as there are colours;
  (c) on the generic matrix each wrong variant differs from the contract;
  (d) the permutation contract against a dense permutation, its order inside a row, its inverse and its map;
  (e) the numpy Krylov twins converge on P A P^T with its ILU(0) in at most 2/3 of the plain iterations;
  (f) the six entry points are declared, exported by both libraries and bound, and refuse a null handle.

Recorded for (a), seed 0: (colours, rounds, largest class, smallest class) and levels in natural order
  symmetric_stencil(16)  4096 rows   6, 16, 1319,   2  (classes 1308, 1319, 899, 461, 107, 2)   46 levels
  tridiagonal_case()     3000 rows   3,  6, 1299, 402                                        3000 levels
  generic_case()          257 rows  14, 41,   35,   4                                          27 levels
  stairs_case()           421 rows   5, 14,  173,   5                                           7 levels
  fan_case()             5010 rows   2, 20, 5000,  10                                           2 levels
  arrow_case()            300 rows   2,  3,  299,   1                                           2 levels
Recorded for (c) on generic_case(), rows whose colour differs: A's rows without the transpose 214 (and the colouring is no longer
proper), key = i 228, the stale rounds 125.
Recorded for (e), float32 numpy, b standard normal (seed 2026), tol = 1e-5, iterations plain / natural ILU(0) / multicolour ILU(0):
  symmetric stencil7(16), PCG 45 / 15 / 21; row-scaled stencil7(16), BiCGStab 35 / 10 / 15.
(The counts are printed, not asserted: a float32 dot product may differ by a rounding from one BLAS to the next.)
"""
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _color as K
import _ilu0 as G
import _trsv as T

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_color", "spmv_csr_permute", "spmv_csr_permute_values", "spmv_csr_permute_gather", "spmv_csr_permute_map_bytes",
         "spmv_permute_vector")
METHODS = ("color", "permute", "permute_values", "permute_gather", "permute_map_bytes")
f32, f64 = np.float32, np.float64
# case -> (colours, rounds, largest, smallest), levels of the lower triangle in natural order
RECORDED = {"sym16": ((6, 16, 1319, 2), 46), "tridiagonal": ((3, 6, 1299, 402), 3000), "generic": ((14, 41, 35, 4), 27),
            "stairs": ((5, 14, 173, 5), 7), "fan": ((2, 20, 5000, 10), 2), "arrow": ((2, 3, 299, 1), 2)}


def _cases(pkg):
    return dict(K.color_cases(pkg), sym16=G.symmetric_stencil(pkg)[:3])


@pytest.fixture(scope="module")
def colored(pkg):
    """name -> (n, rp, ci, contract's colouring under seed 0), computed once."""
    return {name: (n, rp, ci, K.color(rp, ci, 0)) for name, (n, rp, ci) in _cases(pkg).items()}


# ---- (a) ------------------------------------------------------------------------------------------------------------------
def test_fmix32_is_the_stated_hash():
    for x in (0, 1, 0x9E3779B9, 0xFFFFFFFF, 4711):
        h = x
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        assert int(K.fmix32([x])[0]) == h
    assert int(K.keys(8, 5)[3]) == int(K.fmix32([3 ^ 5])[0])
    assert np.unique(K.keys(1 << 16, 0x9E3779B9)).size == 1 << 16, "a bijection: keys never tie"


def test_the_contract_colours_properly_within_the_degree_bound(colored):
    for name, (n, rp, ci, (col, perm, cp, info)) in colored.items():
        assert K.is_proper(rp, ci, col), name
        assert info["colors"] <= K.max_degree(rp, ci) + 1, name
        assert np.array_equal(np.sort(perm), np.arange(n)) and cp[0] == 0 and cp[-1] == n, name
        assert np.all(np.diff(col[perm]) >= 0), name
        for c in range(info["colors"]):
            assert np.all(np.diff(perm[cp[c]:cp[c + 1]]) > 0), f"{name}: rows ascend inside colour {c}"
    for seed in K.SEEDS[1:]:
        n, rp, ci = colored["generic"][:3]
        assert K.is_proper(rp, ci, K.color(rp, ci, seed)[0])


def test_the_recorded_counts(colored):
    for name, (want, natural) in RECORDED.items():
        n, rp, ci, (col, perm, cp, info) = colored[name]
        assert (info["colors"], info["rounds"], info["largest"], info["smallest"]) == want, name
        assert K.depth(rp, ci, "lower") == natural, name
    assert np.diff(colored["sym16"][3][2]).tolist() == [1308, 1319, 899, 461, 107, 2]
    info = colored["clique70"][3][3]
    assert (info["colors"], info["rounds"]) == (70, 70)
    assert colored["star5000"][3][3]["colors"] == 2
    for name in ("diagonal", "empty", "rows1"):
        assert (colored[name][3][3]["colors"], colored[name][3][3]["rounds"]) == (1, 1), name
    assert (colored["rows0"][3][3]["colors"], colored["rows0"][3][3]["rounds"]) == (0, 0)


def test_the_shared_cases_have_the_rows_they_claim(colored):
    n, rp, ci = colored["boundary"][:3]
    assert K.neighbour_entries(rp, ci)[:3].tolist() == [K.SERIAL_MAX - 1, K.SERIAL_MAX, K.SERIAL_MAX + 1]
    n, rp, ci = colored["upper"][:3]
    assert np.all(ci > np.repeat(np.arange(n), np.diff(rp)))
    n, rp, ci = colored["generic"][:3]
    ne = K.neighbour_entries(rp, ci)
    assert ne.max() > 64 and np.sum(ne > K.SERIAL_MAX) >= 16 and ne.min() <= K.SERIAL_MAX
    assert K.neighbour_entries(*colored["fan"][1:3]).max() > 2000
    assert K.neighbour_entries(*colored["star5000"][1:3]).max() == 10002
    n, rp, ci = colored["unsorted"][:3]
    assert not G.is_sorted(rp, ci)


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def test_the_permuted_triangles_are_no_deeper_than_the_colours(colored):
    for name, (n, rp, ci, (col, perm, cp, info)) in colored.items():
        if n == 0:
            continue
        brp, bci, _, _ = K.permute(rp, ci, np.zeros(ci.size, f32), perm, perm)
        for uplo in T.UPLOS:
            assert K.depth(brp, bci, uplo) <= info["colors"], f"{name} {uplo}"
    n, rp, ci, (col, perm, cp, info) = colored["sym16"]
    brp, bci, _, _ = K.permute(rp, ci, np.zeros(ci.size, f32), perm, perm)
    assert K.depth(brp, bci, "lower") == K.depth(brp, bci, "upper") == 6


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def test_the_generic_case_distinguishes_the_variants(colored):
    n, rp, ci, (right, _, _, _) = colored["generic"]
    counts = {w: int(np.sum(K.color(rp, ci, 0, wrong=w)[0] != right)) for w in K.WRONG}
    print("rows whose colour differs from the contract:", counts, "of", n)
    assert counts == {"rows_only": 214, "key_i": 228, "stale": 125}
    assert not K.is_proper(rp, ci, K.color(rp, ci, 0, wrong="rows_only")[0]), "without the transpose the colouring is not proper"


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def _dense(rows, cols, rp, ci, va):
    A = np.zeros((rows, cols), f64)
    np.add.at(A, (np.repeat(np.arange(rows), np.diff(rp)), ci), np.asarray(va, f64))
    return A


def test_permute_equals_a_dense_permutation():
    rng = np.random.default_rng(8)
    n, rp, ci, va = G.generic_case()
    rows, cols, rrp, rci, rva = K.rectangular_case()
    for (m, k, p, c, v) in ((n, n, rp, ci, va), (rows, cols, rrp, rci, rva)):
        A = _dense(m, k, p, c, v)
        for rperm, cperm in ((rng.permutation(m), rng.permutation(k)), (rng.permutation(m), None), (None, rng.permutation(k)), (None, None)):
            brp, bci, bva, bmap = K.permute(p, c, v, rperm, cperm, cols=k)
            want = A[np.arange(m) if rperm is None else rperm][:, np.arange(k) if cperm is None else cperm]
            assert np.array_equal(_dense(m, k, brp, bci, bva), want)
            assert T.same(bva, v[bmap]) is None
    perm = K.color(rp, ci, 0)[1]
    brp, bci, bva, _ = K.permute(rp, ci, va, perm, perm)
    assert G.is_sorted(brp, bci) and np.all(T.diagonal(brp, bci)[1] == 1), "P A P^T of a sorted matrix with a diagonal is one: ilu0 accepts it"


def test_permute_orders_a_row_by_new_column_then_position():
    n, rp, ci, va = K.unsorted_case()
    rng = np.random.default_rng(9)
    rperm, cperm = rng.permutation(n), rng.permutation(n)
    brp, bci, bva, bmap = K.permute(rp, ci, va, rperm, cperm)
    row = np.repeat(np.arange(n), np.diff(brp))
    same_row = row[1:] == row[:-1]
    assert np.all(np.diff(bci)[same_row] >= 0)
    tie = same_row & (np.diff(bci) == 0)
    assert tie.any() and np.all(np.diff(bmap.astype(np.int64))[tie] > 0), "repeated columns stay in A's order"
    assert np.array_equal(cperm[bci], ci[bmap])
    # back again: A with stably sorted rows, and the maps compose
    inv_r, inv_c = K.inverse(rperm), K.inverse(cperm)
    crp, cci, cva, cmap = K.permute(brp, bci, bva, inv_r, inv_c)
    srp, sci, sva, smap = K.permute(rp, ci, va)
    assert np.array_equal(crp, srp) and np.array_equal(cci, sci) and T.same(cva, sva) is None
    assert np.array_equal(bmap[cmap], smap)


# ---- (e) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_the_krylov_twins_on_the_multicolour_factor(pkg, oracle, kind):
    (n, rp, ci, va), solver = {"pcg": (G.symmetric_stencil(pkg), G.pcg), "bicgstab": (G.stencil_case(pkg, 16), G.bicgstab)}[kind]
    b = G.krylov_rhs(n)
    tol = 1e-5
    x0, it0, ok0 = solver(lambda v: oracle.spmv(rp, ci, va, v), None, b, np.zeros(n, f32), tol, 500)
    perm = K.color(rp, ci, 0)[1]
    brp, bci, bva, _ = K.permute(rp, ci, va, perm, perm)
    M = G.factor(brp, bci, bva)
    y, it1, ok1 = solver(lambda v: oracle.spmv(brp, bci, bva, v), lambda v: G.apply(brp, bci, M, v), b[perm], np.zeros(n, f32), tol, 500)
    x1 = np.zeros(n, f32)
    x1[perm] = y
    res0, res1 = G.true_residual(rp, ci, va, b, x0), G.true_residual(rp, ci, va, b, x1)
    print(f"{kind}: plain {it0} iterations, true residual {res0:.2e}; with multicolour ILU(0) {it1}, {res1:.2e}")
    assert ok0 and ok1
    assert 3 * it1 <= 2 * it0
    assert res0 <= 2 * tol and res1 <= 2 * tol


# ---- (f) ------------------------------------------------------------------------------------------------------------------
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_color_symbols_declared_exported_and_bound(pkg):
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
    assert callable(capi.permute_vector) and callable(pkg.solvers.multicolor)
    serial = re.search(r"#define\s+SPMV_COLOR_SERIAL_MAX\s+(\d+)", header)
    assert serial and int(serial.group(1)) == capi.SPMV_COLOR_SERIAL_MAX == K.SERIAL_MAX
    for flag, value in (("KEEP_MAP", capi.PERMUTE_KEEP_MAP), ("VIA_TRANSPOSE", capi.PERMUTE_VIA_TRANSPOSE)):
        assert int(re.search(rf"#define\s+SPMV_PERMUTE_{flag}\s+(\d+)", header).group(1)) == value
    assert header.index("---- the incomplete factorisation") < header.index("---- the multicolour ordering") < header.index("---- the hot path")


def test_color_entry_points_refuse_null_handles(pkg):
    import ctypes as C
    capi = pkg.capi
    lib = capi.lib()

    def refused(rc, name):
        assert rc == capi.ERR_INVALID, name
        assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error().decode()

    out = C.c_void_p(77)
    info = (C.c_int64 * 8)(*([5] * 8))
    refused(lib.spmv_csr_color(None, 0, None, None, None, None, 0, info), "spmv_csr_color")
    assert list(info) == [5] * 8
    refused(lib.spmv_csr_permute(None, None, None, 0, None, C.byref(out)), "spmv_csr_permute")
    assert out.value == 77, "*out is untouched"
    refused(lib.spmv_csr_permute_values(None, None, None), "spmv_csr_permute_values")
    refused(lib.spmv_csr_permute_gather(None, 1, None, 0, None, 0, None), "spmv_csr_permute_gather")
    assert lib.spmv_csr_permute_map_bytes(None) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_permute_map_bytes:")
    refused(lib.spmv_permute_vector(None, 4, 0, None, None, None), "spmv_permute_vector")
    refused(lib.spmv_permute_vector(None, -1, 0, None, None, None), "spmv_permute_vector")
    A = capi.CsrMatrix.__new__(capi.CsrMatrix)
    A._h, A._keep, A.rows, A.cols, A.nnz = C.c_void_p(), (), 4, 4, 0
    with pytest.raises(ValueError, match="color: seed ="):
        A.color(seed=-1)
    with pytest.raises(ValueError, match="permute: row_perm must be"):
        A.permute(row_perm=[0, 1, 2, 3])
    with pytest.raises(TypeError, match="permute_values: a must be"):
        A.permute_values(None)
    with pytest.raises(TypeError, match="multicolor: A must be"):
        pkg.solvers.multicolor(None)
