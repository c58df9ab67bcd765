"""The incomplete factorisation without a device (include/spmv_hip.h "the incomplete factorisation").

  (a) on every case and every stored (i, j): |(L U)_ij - a_ij| in float64 <= bound_ij * (|a_ij| + sum_k |l_ik u_kj|);
  (b) on patterns without fill (a tridiagonal matrix, an arrow) `apply` equals a dense float64 solve;
  (c) on the generic matrix each wrong order differs from the contract;
  (d) the five entry points are declared, exported by both libraries and bound;
  (e) the numpy twins of solvers.pcg and solvers.bicgstab converge on the two 4096-row systems of tests/test_gpu_krylov.py.

The bound of (a).  RTOL = 1e-5 is the project's bound relative to the sum of |terms| (tests/_util.py, as tests/test_trsv_host.py
takes it).  Entry (i, j) is the end of a chain of one fma per term and, below the diagonal, one division: t_ij + 1 roundings of
at most 2^-24 each, every one relative to a partial sum that the magnitude bounds (Higham, Accuracy and Stability, theorem 9.3:
|A - L U| <= gamma_n |L| |U|).  So bound_ij = max(RTOL, (t_ij + 2) 2^-24): RTOL up to 165 terms (every generic chain, at most
~120), and 1.8e-5 on the one longer chain there is, the last diagonal of the 300-row arrow with its 299 terms.

Recorded on the generic 257 x 257 matrix (4295 stored entries), entries that differ from the contract: k descending 1244, the
update with the undivided a_ik 1741, the division by a_kk instead of u_kk 1018.

Recorded for (e), float32 numpy, b standard normal (seed 2026), tol = 1e-5:
  system 1 (symmetric stencil7(16) pattern, 6 / -1)   CG 45 iterations, true residual 8.4e-6; PCG with ILU(0) 15, 6.6e-6
  system 2 (the library's row-scaled stencil7(16))    BiCGStab 35 iterations, 5.9e-6; with ILU(0) 10, 4.9e-6
"""
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _ilu0 as G
import _trsv as T

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_ilu0", "spmv_csr_ilu0_values", "spmv_csr_ilu0_solve", "spmv_csr_ilu0_pivot", "spmv_csr_ilu0_plan_bytes")
METHODS = ("ilu0", "ilu0_values", "ilu0_solve", "ilu0_pivot", "ilu0_plan_bytes")
f32, f64 = np.float32, np.float64
U = 2.0 ** -24


def generic_cases():
    """name -> (n, rp, ci, va): every matrix the GPU tests factor with ordinary values, built by dominant_rows."""
    return {"generic": G.generic_case(), "diagonal": G.diagonal_case(), "tridiagonal": G.tridiagonal_case(), "fan": G.fan_case(),
            "stairs": G.stairs_case(), "lengths": G.lengths_case(), "arrow": G.arrow_case()}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_ilu0_symbols_declared_exported_and_bound(pkg):
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
    serial = re.search(r"#define\s+SPMV_ILU0_SERIAL_MAX\s+(\d+)", header)
    assert serial and int(serial.group(1)) == capi.SPMV_ILU0_SERIAL_MAX == G.SERIAL_MAX
    assert header.index("---- the triangular solve") < header.index("---- the incomplete factorisation") < header.index("---- the hot path")
    assert callable(pkg.solvers.pcg) and callable(pkg.solvers.bicgstab)


def test_ilu0_entry_points_refuse_null_handles(pkg):
    import ctypes as C
    capi = pkg.capi
    lib = capi.lib()

    def refused(rc, name):
        assert rc == capi.ERR_INVALID, name
        assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error().decode()

    out, row = C.c_void_p(77), C.c_int64(5)
    refused(lib.spmv_csr_ilu0(None, 0, None, C.byref(out)), "spmv_csr_ilu0")
    assert out.value == 77, "*out is untouched"
    refused(lib.spmv_csr_ilu0_values(None, None, None), "spmv_csr_ilu0_values")
    refused(lib.spmv_csr_ilu0_solve(None, None, None, None), "spmv_csr_ilu0_solve")
    refused(lib.spmv_csr_ilu0_pivot(None, None, C.byref(row)), "spmv_csr_ilu0_pivot")
    assert row.value == 5
    assert lib.spmv_csr_ilu0_plan_bytes(None) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_ilu0_plan_bytes:")
    A = capi.CsrMatrix.__new__(capi.CsrMatrix)
    A._h, A._keep, A.rows, A.cols, A.nnz = C.c_void_p(), (), 4, 4, 0
    with pytest.raises(ValueError, match="ilu0: thin_rows ="):
        A.ilu0(thin_rows=1.5)
    with pytest.raises(TypeError, match="ilu0_values: a must be"):
        A.ilu0_values(None)
    for solver in (pkg.solvers.pcg, pkg.solvers.bicgstab):
        with pytest.raises(TypeError, match="A must be a CsrMatrix"):
            solver(None, None, None)
        with pytest.raises(ValueError, match="tol ="):
            solver(A, None, None, tol=0)


# ---- the cases are what they claim ------------------------------------------------------------------------------------------
def test_every_generic_case_is_row_dominant_and_keeps_its_pivots():
    for name, (n, rp, ci, va) in generic_cases().items():
        assert G.is_sorted(rp, ci), name
        assert G.dominance(rp, ci, va) <= 0.9 * (1 + 1e-6), f"{name}: {G.dominance(rp, ci, va)}"
        M = G.factor(rp, ci, va)
        d = G.diag_positions(rp, ci)
        assert np.all(np.isfinite(M)), name
        assert np.all(np.abs(M[d]) >= 0.1 * np.abs(va[d]) * (1 - 1e-5)), f"{name}: a pivot below 0.1 |a_ii|"


def test_the_shared_cases_have_the_rows_they_claim(pkg):
    n, rp, ci, va = G.lengths_case()
    assert np.diff(rp)[5000:].tolist() == list(G.LENGTHS) and np.all(np.diff(rp)[:5000] == 1)
    n, rp, ci, va = G.generic_case()
    length = np.diff(rp)
    assert length.max() > 64 and np.sum(length > G.SERIAL_MAX) >= 16 and length.min() == 1
    long_rows = np.flatnonzero(length > G.SERIAL_MAX)
    i = long_rows[-1]
    below = ci[rp[i]:rp[i + 1]]
    below = below[below < i]
    assert np.any(length[below] > G.SERIAL_MAX) and np.any(length[below] <= G.SERIAL_MAX), "terms from short and from long rows"
    assert np.array_equal(np.diff(T.order(T.levels(*G.stairs_case()[1:3], "lower"))[0]), (69, 70, 71, 70, 69, 1, 71))
    assert np.array_equal(np.diff(T.order(T.levels(*G.fan_case()[1:3], "lower"))[0]), (10, 5000))
    assert T.levels(*G.tridiagonal_case()[1:3], "lower").max() == 2999
    n, rp, ci, va = G.arrow_case()
    assert np.diff(rp).tolist() == [2] * 299 + [300]
    for m, levels in ((8, 22), (16, 46)):
        n, rp, ci, va = G.stencil_case(pkg, m)
        assert G.is_sorted(rp, ci) and T.levels(rp, ci, "lower").max() + 1 == levels
    n, rp, ci, va = G.symmetric_stencil(pkg)
    A = G.dense(rp, ci, va)
    assert n == 4096 and np.array_equal(A, A.T)


# ---- (a) ------------------------------------------------------------------------------------------------------------------
def test_l_times_u_gives_back_a_on_the_pattern(pkg):
    cases = dict(generic_cases(), stencil=G.stencil_case(pkg))
    for name, (n, rp, ci, va) in cases.items():
        M = G.factor(rp, ci, va)
        prod, mag, terms = G.lu_product(rp, ci, M)
        bound = np.maximum(G.RTOL, (terms + 2) * U)
        err = np.abs(prod - va.astype(f64))
        worst = np.max(err / (bound * (np.abs(va.astype(f64)) + mag)))
        assert worst <= 1.0, f"{name}: {worst} of the bound"
        if name != "arrow":
            assert terms.max() <= 165, name                    # RTOL alone


# ---- (b) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("tridiagonal", "arrow"))
def test_apply_equals_a_dense_solve_where_there_is_no_fill(case):
    """Without fill L U = A up to rounding, so apply() is a backward-stable solve with A: each of its two sweeps and the
    factorisation perturb A componentwise by at most RTOL (the trsv host bound and (a)), and the forward error is at most
    cond(A) times their sum, relative to the largest |x|."""
    n, rp, ci, va = G.tridiagonal_case(400) if case == "tridiagonal" else G.arrow_case()
    r = T.rhs(n, np.random.default_rng(5))
    M = G.factor(rp, ci, va)
    z = G.apply(rp, ci, M, r)
    # each sweep against a dense float64 solve with M's own triangle, within the trsv host bound RTOL * mag
    y = T.solve(rp, ci, M, r, "lower", unit=True)
    for got, rhs, uplo, unit in ((y, r, "lower", True), (z, y, "upper", False)):
        x64, mag = T.dense_solve(rp, ci, M, rhs, uplo, unit)
        assert np.all(np.abs(got.astype(f64) - x64) <= T.RTOL * mag), uplo
    A = G.dense(rp, ci, va)
    x = np.linalg.solve(A, r.astype(f64))
    bound = 3 * G.RTOL * np.linalg.cond(A, np.inf) * np.max(np.abs(x))
    assert np.max(np.abs(z.astype(f64) - x)) <= bound


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def test_the_generic_case_distinguishes_the_orders():
    n, rp, ci, va = G.generic_case()
    right = G.factor(rp, ci, va)
    counts = {w: G.differs(right, G.factor(rp, ci, va, wrong=w)) for w in G.WRONG}
    for w, d in counts.items():
        assert d >= 1, f"the order {w} differs from the contract in {d} of {va.size} entries"
    print("entries that differ from the contract:", counts, "of", va.size)


# ---- (e) ------------------------------------------------------------------------------------------------------------------
def _systems(pkg):
    return {"pcg": (G.symmetric_stencil(pkg), G.pcg), "bicgstab": (G.stencil_case(pkg, 16), G.bicgstab)}


@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_the_numpy_krylov_twins_converge_and_ilu0_helps(pkg, oracle, kind):
    (n, rp, ci, va), solver = _systems(pkg)[kind]
    assert n == 4096
    b = G.krylov_rhs(n)
    M = G.factor(rp, ci, va)
    spmv = lambda v: oracle.spmv(rp, ci, va, v)
    tol = 1e-5
    x0, it0, ok0 = solver(spmv, None, b, np.zeros(n, f32), tol, 500)
    x1, it1, ok1 = solver(spmv, lambda v: G.apply(rp, ci, M, v), b, np.zeros(n, f32), tol, 500)
    res0, res1 = G.true_residual(rp, ci, va, b, x0), G.true_residual(rp, ci, va, b, x1)
    print(f"{kind}: plain {it0} iterations, true residual {res0:.2e}; with ILU(0) {it1}, {res1:.2e}")
    assert ok0 and ok1
    assert res0 <= 2 * tol and res1 <= 2 * tol
    assert (2 * it1 <= it0) if kind == "pcg" else (it1 <= it0)


def test_the_cases_beyond_the_per_launch_caps_have_the_levels_they_claim():
    """tridiagonal_case(4100): 4100 levels of one row in both triangles, more than one launch of the plans' small peel retires
    (4096); stairs_case around the peel's workgroup of 256 rows: lower levels of exactly these sizes.  Both stay dominant."""
    n, rp, ci, va = G.tridiagonal_case(4100)
    assert n == 4100 and np.array_equal(T.levels(rp, ci, "lower"), np.arange(n)) and np.array_equal(T.levels(rp, ci, "upper"), np.arange(n)[::-1])
    sizes = (255, 256, 257, 256, 255, 1, 257)
    m, srp, sci, sva = G.stairs_case(sizes)
    assert m == sum(sizes) and np.array_equal(np.diff(T.order(T.levels(srp, sci, "lower"))[0]), sizes)
    assert T.levels(srp, sci, "upper").max() >= 1
    for name, (k, a, b, c) in (("tridiagonal", (n, rp, ci, va)), ("stairs", (m, srp, sci, sva))):
        assert G.is_sorted(a, b) and G.dominance(a, b, c) <= 0.9 * (1 + 1e-6), name
        M = G.factor(a, b, c)
        assert np.all(np.isfinite(M)) and G.differs(M, c) > k // 2, name


# ---- (f) the iterates of the twins -------------------------------------------------------------------------------------------
def _iterates(pkg, oracle, kind, with_m, wrong=None, dtype=f64):
    system, twin = G.krylov_systems(pkg)[kind]
    return G.twin_iterates(twin, system, G.krylov_rhs(system[0]), with_m, dtype, spmv32=oracle.spmv, wrong=wrong)


@pytest.mark.parametrize("with_m", (False, True))
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_the_float32_twins_stay_close_to_the_float64_twins_and_wrong_ones_do_not(pkg, oracle, kind, with_m):
    """d(k): the float32 twin's deviation from the float64 twin after k = 1, 2, 4 iterations from x = 0 (max norm, relative to
    the float64 x), printed; tests/test_gpu_krylov.py allows the solvers 8 max(d(k), k 2^-23).  Two wrong iterations -- 1 / beta
    for beta, and p updated with the opposite sign -- are the same as the right one at k = 1 (no beta yet) and exceed that bound
    by k = 4, in float64 and in float32 alike: the bound tells them apart."""
    ref = _iterates(pkg, oracle, kind, with_m)
    f32_twin = _iterates(pkg, oracle, kind, with_m, dtype=f32)
    d = {k: G.deviation(f32_twin[k], ref[k]) for k in G.KRYLOV_KS}
    print(f"{kind} {'with' if with_m else 'without'} M: d(k) = " + ", ".join(f"{k}: {d[k]:.2e}" for k in G.KRYLOV_KS))
    for k in G.KRYLOV_KS:
        assert np.all(np.isfinite(ref[k])) and d[k] <= 1e-5, (k, d[k])
    for wrong in G.KRYLOV_WRONG:
        for dtype in (f64, f32):
            bad = _iterates(pkg, oracle, kind, with_m, wrong=wrong, dtype=dtype)
            dev = {k: G.deviation(bad[k], ref[k]) for k in G.KRYLOV_KS}
            print(f"  {wrong} in {dtype.__name__}: " + ", ".join(f"{k}: {dev[k]:.2e}" for k in G.KRYLOV_KS))
            assert dev[1] <= G.krylov_bound(d[1], 1), (wrong, dev)
            assert dev[4] > G.krylov_bound(d[4], 4), f"{wrong}: {dev[4]:.3g} is inside the bound {G.krylov_bound(d[4], 4):.3g}"


def test_the_twins_report_a_breakdown():
    b = np.array([1.0, -2.0, 0.5, 3.0], f32)
    zero = lambda v: np.zeros(4, f32)
    for solver in (G.pcg, G.bicgstab):
        x, it, ok = solver(zero, None, b, np.zeros(4, f32))
        assert not ok and np.all(x == 0)
