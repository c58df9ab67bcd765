"""The triangular solve without a device (include/spmv_hip.h "the triangular solve"): the six entry points are declared,
exported by the normal and the bounds-checked library and bound in capi with the enums and SPMV_TRSV_SERIAL_MAX; null handles
are refused under each function's name; the numpy statement of the contract (tests/_trsv.py) agrees with a dense float64
solve; every generic case is row-dominant, so its reference x is finite and free of zeros; the generic cases tell the
contract's order from three wrong ones; the level sets equal a serial definition; the numpy twin of solvers.gauss_seidel
reduces the residual sweep after sweep."""
import ctypes as C
import fnmatch
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _trsv as G

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_trsv_plan", "spmv_csr_trsv", "spmv_csr_trsv_plan_bytes", "spmv_csr_trsv_plan_info", "spmv_csr_trsv_plan_rows",
         "spmv_csr_trsv_describe")
METHODS = ("trsv_plan", "trsv", "trsv_plan_bytes", "trsv_plan_info", "trsv_plan_rows", "trsv_describe")
f32 = np.float32


def generic_cases(pkg):
    """name -> (n, rp, ci, va, b, uplo): every matrix the GPU tests solve with ordinary values."""
    out = {}
    for u in G.UPLOS:
        out[f"generic-{u}"] = G.generic_case() + (u,)
        out[f"stencil-{u}"] = G.stencil_case(pkg) + (u,)
        out[f"chain-{u}"] = G.chain_case(3000, u) + (u,)
        out[f"stairs-{u}"] = G.stairs_case((69, 70, 71, 70, 69, 1, 71), u) + (u,)
    out["diagonal"] = G.diagonal_case() + ("lower",)
    out["fan"] = G.fan_case() + ("lower",)
    out["lengths"] = G.lengths_case() + ("lower",)
    return out


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_trsv_symbols_declared_exported_and_bound(pkg):
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
    uplo = re.search(r"enum\s*\{\s*SPMV_TRSV_LOWER\s*=\s*(\d+)\s*,\s*SPMV_TRSV_UPPER\s*=\s*(\d+)\s*\}", header)
    diag = re.search(r"enum\s*\{\s*SPMV_TRSV_NON_UNIT\s*=\s*(\d+)\s*,\s*SPMV_TRSV_UNIT\s*=\s*(\d+)\s*\}", header)
    assert uplo and diag, "the SPMV_TRSV_* enums are not in include/spmv_hip.h"
    assert (capi.TRSV_LOWER, capi.TRSV_UPPER) == tuple(int(v) for v in uplo.groups()) == (0, 1)
    assert (capi.TRSV_NON_UNIT, capi.TRSV_UNIT) == tuple(int(v) for v in diag.groups()) == (0, 1)
    serial = re.search(r"#define\s+SPMV_TRSV_SERIAL_MAX\s+(\d+)", header)
    assert serial and int(serial.group(1)) == capi.SPMV_TRSV_SERIAL_MAX == G.SERIAL_MAX
    assert header.index("---- the sparse sum") < header.index("---- the triangular solve") < header.index("---- the hot path")
    assert callable(pkg.solvers.gauss_seidel)


def test_trsv_entry_points_refuse_null_handles_and_bad_enums(pkg):
    capi = pkg.capi
    lib = capi.lib()

    def refused(rc, name):
        assert rc == capi.ERR_INVALID, name
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(name + ":"), msg

    info = (C.c_int64 * 8)()
    buf = C.create_string_buffer(64)
    refused(lib.spmv_csr_trsv_plan(None, 0, 0, None), "spmv_csr_trsv_plan")
    refused(lib.spmv_csr_trsv(None, 0, 0, None, None, None), "spmv_csr_trsv")
    assert lib.spmv_csr_trsv_plan_bytes(None, 0) == capi.ERR_INVALID
    assert lib.spmv_last_error().decode().startswith("spmv_csr_trsv_plan_bytes:")
    refused(lib.spmv_csr_trsv_plan_info(None, 0, info), "spmv_csr_trsv_plan_info")
    refused(lib.spmv_csr_trsv_plan_rows(None, 0, None, None), "spmv_csr_trsv_plan_rows")
    refused(lib.spmv_csr_trsv_describe(None, 0, buf, 64), "spmv_csr_trsv_describe")
    # the wrappers refuse before any call
    A = capi.CsrMatrix.__new__(capi.CsrMatrix)
    A._h, A._keep, A.rows, A.cols, A.nnz = C.c_void_p(), (), 4, 4, 0
    for bad in ("left", 1.5, True, None):
        with pytest.raises(ValueError, match="trsv_plan: uplo ="):
            A.trsv_plan(bad)
    with pytest.raises(ValueError, match="trsv_plan: thin_rows ="):
        A.trsv_plan("lower", thin_rows=1.5)
    with pytest.raises(TypeError, match="gauss_seidel: A must be"):
        pkg.solvers.gauss_seidel(None, None, None)
    A.cols = 5
    with pytest.raises(ValueError, match="gauss_seidel: A is 4 x 5"):
        pkg.solvers.gauss_seidel(A, None, None)


@pytest.mark.parametrize("unit", (False, True))
def test_contract_agrees_with_a_dense_float64_solve(pkg, unit):
    for name, (n, rp, ci, va, b, uplo) in generic_cases(pkg).items():
        if n > 600 and not name.startswith("chain"):
            continue                                           # (a dense 5000 x 5000 walk is minutes; the shapes above cover the sums)
        x = G.solve(rp, ci, va, b, uplo, unit)
        x64, mag = G.dense_solve(rp, ci, va, b, uplo, unit)
        err = np.abs(x.astype(np.float64) - x64)
        assert np.all(err <= G.RTOL * mag), f"{name} unit={unit}: {np.max(err / mag)}"


def test_every_generic_case_is_row_dominant_finite_and_free_of_zeros(pkg):
    for name, (n, rp, ci, va, b, uplo) in generic_cases(pkg).items():
        pos, trow, _, _ = G.terms(rp, ci, uplo)
        dpos, occ = G.diagonal(rp, ci)
        assert np.all(occ == 1), name
        s = np.bincount(trow, weights=np.abs(va[pos].astype(np.float64)), minlength=n)
        d = np.abs(va[dpos].astype(np.float64))
        assert np.all(s <= 0.9 * d * (1 + 1e-6)), f"{name}: row {int(np.argmax(s / d))} has sum |terms| / |d| = {np.max(s / d)}"
        x = G.solve(rp, ci, va, b, uplo)
        assert np.all(np.isfinite(x)) and np.all(x != 0), name
        assert np.max(np.abs(x)) <= 10 * np.max(np.abs(b)) / np.min(d) * (1 + 1e-5), name


def test_the_generic_cases_distinguish_the_orders():
    n, rp, ci, va, b = G.generic_case()
    for uplo in G.UPLOS:
        right = G.solve(rp, ci, va, b, uplo)
        assert G.terms(rp, ci, uplo)[3].max() > G.SERIAL_MAX          # there are long rows
        for wrong in G.WRONG:
            d = G.differs(right, G.solve(rp, ci, va, b, uplo, wrong=wrong))
            assert d >= 1, f"{uplo}: the order {wrong} differs from the contract in {d} of {n} rows"
    n, rp, ci, va, b = G.lengths_case()
    right = G.solve(rp, ci, va, b)
    for wrong in ("desc", "serial_long"):                                 # (nine rows with terms: the orders of the long sums)
        d = G.differs(right, G.solve(rp, ci, va, b, wrong=wrong))
        assert d >= 1, f"lengths:the order {wrong} differs from the contract in {d} of {n} rows"


def test_level_sets_equal_a_serial_definition(pkg):
    for name, (n, rp, ci, va, b, uplo) in generic_cases(pkg).items():
        lev = G.levels(rp, ci, uplo)
        # Kahn's peel, serially: a row joins the level after the one that resolves its last term
        pos, trow, _, count = G.terms(rp, ci, uplo)
        left = count.copy()
        dependents = [[] for _ in range(n)]
        for p, r in zip(ci[pos].tolist(), trow.tolist()):
            dependents[p].append(r)
        front, k, got = [i for i in range(n) if left[i] == 0], 0, np.full(n, -1)
        while front:
            nxt = []
            for c in front:
                got[c] = k
                for i in dependents[c]:
                    left[i] -= 1
                    if left[i] == 0:
                        nxt.append(i)
            front, k = nxt, k + 1
        assert np.array_equal(got, lev), name
        lp, od = G.order(lev)
        assert lp[0] == 0 and lp[-1] == n and np.array_equal(np.sort(od), np.arange(n))
        for j in range(len(lp) - 1):
            rows = od[lp[j]:lp[j + 1]]
            assert np.all(lev[rows] == j) and np.all(np.diff(rows) > 0), name
    n, rp, ci, _, _ = G.stencil_case(pkg)
    r = np.arange(n)
    assert np.array_equal(G.levels(rp, ci, "lower"), r // 64 + (r // 8) % 8 + r % 8)     # i + j + k on the grid


def test_the_shared_cases_have_the_rows_they_claim():
    n, rp, ci, va, b = G.lengths_case()
    count = G.terms(rp, ci, "lower")[3]
    assert sorted(set(count.tolist())) == sorted(G.LENGTHS()) and np.sum(count == 0) == 5000
    n, rp, ci, _, _ = G.generic_case()
    assert any(np.any(np.diff(ci[rp[r]:rp[r + 1]]) < 0) for r in range(n))                # unsorted rows
    assert any(np.unique(ci[rp[r]:rp[r + 1]]).size < rp[r + 1] - rp[r] for r in range(n))  # repeated columns
    for u in G.UPLOS:
        n, rp, ci, _, _ = G.stairs_case((69, 70, 71, 70, 69, 1, 71), u)
        assert np.array_equal(np.diff(G.order(G.levels(rp, ci, u))[0]), (69, 70, 71, 70, 69, 1, 71))
        n, rp, ci, _, _ = G.chain_case(3000, u)
        assert G.levels(rp, ci, u).max() == 2999
    n, rp, ci, _, _ = G.fan_case()
    assert np.array_equal(np.diff(G.order(G.levels(rp, ci, "lower"))[0]), (10, 5000))


def test_the_cases_beyond_the_per_launch_caps_have_the_levels_they_claim():
    """The chains deeper than one launch of the plan's small peel (4096 levels), and level sizes on either side of its
    workgroup of 256 rows: the level counts and sizes by the serial definition, so that a wrong reference cannot hide a wrong
    kernel; every x is finite and the chain's rows depend on their one neighbour."""
    for n, u in ((4097, "lower"), (8193, "upper")):
        m, rp, ci, va, b = G.chain_case(n, u)
        lev = G.levels(rp, ci, u)
        assert m == n and np.array_equal(lev, np.arange(n) if u == "lower" else np.arange(n)[::-1])
        lp, od = G.order(lev)
        assert np.all(np.diff(lp) == 1) and np.array_equal(od, np.arange(n) if u == "lower" else np.arange(n)[::-1])
        count = G.terms(rp, ci, u)[3]
        assert count.sum() == n - 1 and count.max() == 1
        x = G.solve(rp, ci, va, b, u)
        assert np.all(np.isfinite(x)) and np.all(x != 0)
        assert G.differs(x, G.solve(rp, ci, va, b, u, wrong="from_b")) >= 1
    sizes = (255, 256, 257, 256, 255, 1, 257)
    for u in G.UPLOS:
        n, rp, ci, va, b = G.stairs_case(sizes, u)
        assert n == sum(sizes) and np.array_equal(np.diff(G.order(G.levels(rp, ci, u))[0]), sizes)
        assert np.all(np.isfinite(G.solve(rp, ci, va, b, u)))


def test_gauss_seidel_twin_reduces_the_residual(pkg):
    n, rp, ci, va, b = G.stencil_case(pkg)
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(rp)), ci), va.astype(np.float64))
    spmv = lambda x: (A @ x.astype(np.float64)).astype(f32)
    for symmetric in (False, True):
        x = np.zeros(n, f32)
        res = [np.linalg.norm(b - A @ x)]
        for _ in range(4):
            x = G.gauss_seidel(spmv, rp, ci, va, b, x, 1, symmetric)
            res.append(np.linalg.norm(b.astype(np.float64) - A @ x))
        assert all(b_ < 0.9 * a_ for a_, b_ in zip(res, res[1:])), f"symmetric={symmetric}: residuals {res}"
