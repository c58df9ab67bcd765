"""GPU (-m gpu): spmv_csr_trsv_plan / spmv_csr_trsv and their reports (include/spmv_hip.h "the triangular solve").

The expectation is always tests/_trsv.py (numpy), never a kernel of this library, and every x is compared bit for bit (the
uint32 view; a NaN matches any NaN).  That the generic inputs are row-dominant (finite x without zeros) and tell the
contract's order from three wrong ones is proved in tests/test_trsv_host.py.

  1 generic        257 x 257 full, unsorted rows with repeats, the unread triangle NaN; lower / upper, unit / non-unit; the plan
  2 level graphs   a diagonal, a bidiagonal chain across the per-launch cap, a fan after a thin level, sizes around thin_rows, stencil7(8)
  3 row lengths    0, 1, SERIAL_MAX - 1 .. + 1, 63, 64, 65, 129, 5000 terms, in grid launches and in one workgroup's
  4 purity         thin_rows 1 / default / 1 << 30, two streams, owned against borrowed, in place, poisoned x
  5 live values    vals rewritten between solves without a new plan; a captured graph replayed after a rewrite
  6 special values NaN / Inf in b reach exactly their dependents; a zero pivot; -0 and subnormals; unit with a NaN diagonal
  7 refusals       missing / repeated diagonal (unit still solves), shapes, enums, no plan, null arrays; nothing left behind
  8 edges          rows = 0, 1; nnz = 0
  9 downstream     solvers.gauss_seidel against the numpy composition; sparse_sgemv --trsv; a handle made by add(A, I)
"""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import _trsv as G

MIB = 1 << 20
f32 = np.float32
UPLOS = G.UPLOS


def _dev(gpu, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _owned(capi, n, rp, ci, va):
    return capi.CsrMatrix.from_host(n, n, rp, ci, va)


def _borrowed(capi, gpu, n, rp, ci, va):
    t = (_dev(gpu, rp, np.int32), _dev(gpu, ci, np.int32), _dev(gpu, va, np.float32))
    return capi.CsrMatrix.from_device(n, n, *t), t


@functools.lru_cache(maxsize=None)
def _want(key, uplo, unit):
    """The contract's x for a shared case, computed once."""
    n, rp, ci, va, b = _CASES[key]()
    return G.solve(rp, ci, va, b, uplo, unit)


_CASES = {
    "generic": G.generic_case,
    "diagonal": G.diagonal_case,
    "chain-lower": lambda: G.chain_case(3000, "lower"),
    "chain-upper": lambda: G.chain_case(3000, "upper"),
    "fan": G.fan_case,
    "lengths": G.lengths_case,
}


def _solve(gpu, A, b, uplo, unit=False, poison=True):
    import torch
    x = torch.full((A.rows,), float("nan"), device=gpu) if poison else None
    x = A.trsv(_dev(gpu, b, np.float32), x, uplo=uplo, unit=unit)
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _check_plan(A, rp, ci, uplo, thin=None):
    """order / level_ptr equal numpy's, and plan_info is consistent with them."""
    lp, od = G.order(G.levels(rp, ci, uplo))
    got_lp, got_od = A.trsv_plan_rows(uplo)
    assert np.array_equal(got_lp, lp) and np.array_equal(got_od, od), f"{uplo}: the plan's rows"
    info = A.trsv_plan_info(uplo)
    sizes = np.diff(lp)
    count = G.terms(rp, ci, uplo)[3]
    _, occ = G.diagonal(rp, ci)
    bad = np.flatnonzero(occ != 1)
    assert info["levels"] == len(sizes) and info["widest"] == (sizes.max() if sizes.size else 0)
    assert info["long_rows"] == int(np.sum(count > G.SERIAL_MAX))
    assert info["bad_diag_row"] == (int(bad[0]) if bad.size else -1)
    thin_in_force, cap = info["thin_rows"], info["level_cap"]
    assert thin_in_force >= 1 and cap >= 1
    if thin:                                                    # (0: the library's default, whatever it is)
        assert thin_in_force == thin
    launches, k = 0, 0
    while k < len(sizes):                                       # the steps as the header states them
        if sizes[k] > thin_in_force:
            k += 1
        else:
            e = k
            while e < len(sizes) and e - k < cap and sizes[e] <= thin_in_force:
                e += 1
            k = e
        launches += 1
    assert info["launches"] == launches, (info, launches)
    long_terms = int(count[count > G.SERIAL_MAX].sum())
    n = len(rp) - 1
    assert A.trsv_plan_bytes(uplo) == 8 * n + 4 * (len(sizes) + 1) + 4 * (n + 1) + 4 * long_terms
    text = A.trsv_describe(uplo)
    assert text.startswith(f"trsv {uplo} levels={len(sizes)} launches={launches} ")
    return info


# ---- 1. generic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("unit", (False, True))
@pytest.mark.parametrize("uplo", UPLOS)
def test_generic_full_matrix_with_the_other_triangle_nan(pkg, gpu, uplo, unit):
    capi = pkg.capi
    assert capi.SPMV_TRSV_SERIAL_MAX == G.SERIAL_MAX
    n, rp, ci, va, b = G.generic_case()
    A = _owned(capi, n, rp, ci, G.poison_other_triangle(rp, ci, va, uplo))
    assert A.trsv_plan_bytes(uplo) == 0
    A.trsv_plan(uplo)
    _check_plan(A, rp, ci, uplo)
    bad = G.same(_solve(gpu, A, b, uplo, unit), _want("generic", uplo, unit))
    assert bad is None, f"{uplo} unit={unit}: {bad}"
    A.close()


# ---- 2. the shapes of the level graph ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key,uplo", [("diagonal", "lower"), ("diagonal", "upper"), ("chain-lower", "lower"), ("chain-upper", "upper"),
                                      ("fan", "lower")])
def test_level_graph_shapes(pkg, gpu, key, uplo):
    n, rp, ci, va, b = _CASES[key]()
    A = _owned(pkg.capi, n, rp, ci, va)
    A.trsv_plan(uplo)
    info = _check_plan(A, rp, ci, uplo)
    if key.startswith("chain"):
        assert info["levels"] == 3000 and info["level_cap"] < 3000 and info["launches"] == -(-3000 // info["level_cap"])
    if key == "diagonal":
        assert (info["levels"], info["launches"], info["widest"]) == (1, 1, 3000)
    if key == "fan":
        assert (info["levels"], info["launches"], info["widest"]) == (2, 2, 5000) and info["thin_rows"] < 5000
    bad = G.same(_solve(gpu, A, b, uplo), _want(key, uplo, False))
    assert bad is None, f"{key}: {bad}"
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("uplo", UPLOS)
def test_level_sizes_around_an_explicit_thin_threshold(pkg, gpu, uplo):
    thin = 70
    sizes = (thin - 1, thin, thin + 1, thin, thin - 1, 1, thin + 1)
    n, rp, ci, va, b = G.stairs_case(sizes, uplo)
    A = _owned(pkg.capi, n, rp, ci, va)
    A.trsv_plan(uplo, thin_rows=thin)
    info = _check_plan(A, rp, ci, uplo, thin=thin)
    assert info["launches"] == 4                                # [69, 70] [71] [70, 69, 1] [71]
    assert np.array_equal(np.diff(A.trsv_plan_rows(uplo)[0]), sizes)
    bad = G.same(_solve(gpu, A, b, uplo), G.solve(rp, ci, va, b, uplo))
    assert bad is None, bad
    A.close()


DEEP_CHAINS = ((4097, "lower"), (8193, "upper"))           # more levels than one launch of the plan's small peel retires (4096)
EDGE_STAIRS = (255, 256, 257, 256, 255, 1, 257)             # around the peel's workgroup of 256 rows and SPMV_TRSV_THIN_DEFAULT


@pytest.mark.gpu
@pytest.mark.parametrize("n,uplo", DEEP_CHAINS)
def test_chains_deeper_than_one_launch_of_the_small_peel(pkg, gpu, n, uplo):
    """The plan's one-workgroup peel stops after 4096 levels and hands a live frontier back to the host loop, which starts the
    next launch one level further (4097: once, with one row left; 8193: twice).  Levels, order and x against numpy, under the
    three thin thresholds."""
    n, rp, ci, va, b = G.chain_case(n, uplo)
    want = G.solve(rp, ci, va, b, uplo)
    for thin in (1, 0, 1 << 30):
        A = _owned(pkg.capi, n, rp, ci, va)
        A.trsv_plan(uplo, thin_rows=thin)
        info = _check_plan(A, rp, ci, uplo, thin=thin)       # (plan_rows against _trsv.order, launches by the merging rule)
        assert (info["levels"], info["widest"]) == (n, 1)
        assert info["launches"] == -(-n // info["level_cap"]), info
        bad = G.same(_solve(gpu, A, b, uplo), want)
        assert bad is None, f"thin_rows={thin}: {bad}"
        A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("uplo", UPLOS)
def test_level_sizes_around_the_peel_workgroup_and_the_default_thin_threshold(pkg, gpu, uplo):
    """Frontiers of 255, 256, 257, 256, 255, 1, 257 rows: the plan's peel changes between its one-workgroup and its grid kernel
    in both directions at the edge, and the solve crosses the default thin threshold at the same sizes."""
    n, rp, ci, va, b = G.stairs_case(EDGE_STAIRS, uplo)
    A = _owned(pkg.capi, n, rp, ci, va)
    A.trsv_plan(uplo, thin_rows=0)
    info = _check_plan(A, rp, ci, uplo)
    assert info["thin_rows"] == 256 and info["launches"] == 4   # [255, 256] [257] [256, 255, 1] [257]
    assert np.array_equal(np.diff(A.trsv_plan_rows(uplo)[0]), EDGE_STAIRS)
    bad = G.same(_solve(gpu, A, b, uplo), G.solve(rp, ci, va, b, uplo))
    assert bad is None, bad
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("uplo", UPLOS)
def test_stencil7(pkg, gpu, uplo):
    n, rp, ci, va, b = G.stencil_case(pkg)
    A = _owned(pkg.capi, n, rp, ci, va)
    A.trsv_plan(uplo)
    info = _check_plan(A, rp, ci, uplo)
    assert info["levels"] == 22                                 # i + j + k on an 8 x 8 x 8 grid
    for unit in (False, True):
        bad = G.same(_solve(gpu, A, b, uplo, unit), G.solve(rp, ci, va, b, uplo, unit))
        assert bad is None, f"unit={unit}: {bad}"
    A.close()


# ---- 3. row lengths, 4. purity -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thin", (1, 0, 1 << 30))
def test_row_lengths_in_grid_launches_and_in_one_workgroup(pkg, gpu, thin):
    n, rp, ci, va, b = G.lengths_case(pkg.capi.SPMV_TRSV_SERIAL_MAX)
    A = _owned(pkg.capi, n, rp, ci, va)
    A.trsv_plan("lower", thin_rows=thin)
    info = _check_plan(A, rp, ci, "lower", thin=thin)
    assert info["launches"] == (1 if thin == 1 << 30 else 2) and info["long_rows"] == 6
    bad = G.same(_solve(gpu, A, b, "lower"), _want("lengths", "lower", False))
    assert bad is None, f"thin_rows={thin}: {bad}"
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("uplo", UPLOS)
def test_purity_thin_rows_streams_owners_and_in_place(pkg, gpu, uplo):
    import torch
    capi = pkg.capi
    n, rp, ci, va, b = G.generic_case()
    want = _want("generic", uplo, False)
    d_b = _dev(gpu, b)
    for thin in (1, 0, 7, 1 << 30):
        A = _owned(capi, n, rp, ci, va)
        A.trsv_plan(uplo, thin_rows=thin)
        _check_plan(A, rp, ci, uplo, thin=thin)
        x = torch.full((n,), float("nan"), device=gpu)          # poisoned: every row is written
        A.trsv(d_b, x, uplo=uplo)
        torch.cuda.synchronize()
        bad = G.same(x.cpu().numpy(), want)
        assert bad is None, f"thin_rows={thin}: {bad}"
        A.close()
    A, keep = _borrowed(capi, gpu, n, rp, ci, va)
    A.trsv_plan(uplo)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    x1, x2 = torch.full((n,), float("nan"), device=gpu), torch.full((n,), float("nan"), device=gpu)
    torch.cuda.synchronize()
    A.trsv(d_b, x1, uplo=uplo, stream=s1)
    A.trsv(d_b, x2, uplo=uplo, stream=s2)
    torch.cuda.synchronize()
    assert G.same(x1.cpu().numpy(), want) is None and G.same(x2.cpu().numpy(), want) is None
    inplace = d_b.clone()
    assert A.trsv(inplace, inplace, uplo=uplo) is inplace
    torch.cuda.synchronize()
    assert G.same(inplace.cpu().numpy(), want) is None, "in place"
    A.close()


# ---- 5. live values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_values_are_read_live_and_a_solve_replays_in_a_graph(pkg, gpu):
    import torch
    n, rp, ci, va, b = G.generic_case()
    A, (_, _, d_va) = _borrowed(pkg.capi, gpu, n, rp, ci, va)
    A.trsv_plan("lower")
    d_b, x = _dev(gpu, b), torch.full((n,), float("nan"), device=gpu)
    rng = np.random.default_rng(17)

    def rewrite():
        row = np.repeat(np.arange(n), np.diff(rp))
        nv = np.where(ci == row, va * f32(rng.uniform(1.0, 2.0)), va * rng.uniform(0.2, 1.0, va.size).astype(f32)).astype(f32)
        d_va.copy_(_dev(gpu, nv))
        return G.solve(rp, ci, nv, b, "lower")

    A.trsv(d_b, x)
    torch.cuda.synchronize()
    assert G.same(x.cpu().numpy(), _want("generic", "lower", False)) is None
    w1 = rewrite()
    A.trsv(d_b, x)                                              # no new plan
    torch.cuda.synchronize()
    assert G.same(x.cpu().numpy(), w1) is None, "after a rewrite of vals"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.trsv(d_b, x)
    w2 = rewrite()
    x.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert G.same(x.cpu().numpy(), w2) is None, "from a replayed graph"
    assert G.differs(w1, w2) > n // 2
    A.close()


# ---- 6. special values ------------------------------------------------------------------------------------------------------------------
def _reachable(rp, ci, uplo, seeds):
    """The rows whose x depends on b[seeds]: the seeds and everything that has a reached row among its terms."""
    n = len(rp) - 1
    hit = np.zeros(n, bool)
    hit[list(seeds)] = True
    for i in (range(n) if uplo == "lower" else range(n - 1, -1, -1)):
        c = ci[rp[i]:rp[i + 1]]
        c = c[c < i] if uplo == "lower" else c[c > i]
        if c.size and hit[c].any():
            hit[i] = True
    return hit


@pytest.mark.gpu
@pytest.mark.parametrize("uplo", UPLOS)
def test_nan_and_inf_in_b_reach_exactly_their_dependents(pkg, gpu, uplo):
    n, rp, ci, va, b = G.generic_case()
    A = _owned(pkg.capi, n, rp, ci, va)
    A.trsv_plan(uplo)
    clean = _want("generic", uplo, False)
    for value, seeds in ((np.nan, (100,)), (np.inf, (130,)), (-np.inf, (90, 180))):
        bb = b.copy()
        bb[list(seeds)] = value
        hit = _reachable(rp, ci, uplo, seeds)
        assert 0 < hit.sum() < n
        want = G.solve(rp, ci, va, bb, uplo)
        got = _solve(gpu, A, bb, uplo)
        assert G.same(got, want) is None, G.same(got, want)
        assert np.all(np.isfinite(got[~hit])) and G.same(got[~hit], clean[~hit]) is None, "rows that do not depend on the seeds"
        assert not np.isfinite(got[list(seeds)]).any()
    A.close()


@pytest.mark.gpu
def test_zero_pivot_minus_zero_subnormals_and_unit_with_nan_diagonal(pkg, gpu):
    capi = pkg.capi
    tiny = np.float32(1e-41)                                    # subnormal
    # rows: 0: d = 0, b = 1 -> +Inf; 1: d = -0, b = 1 -> -Inf; 2: d = 2, b = -0 -> -0; 3: subnormal / 4 -> subnormal quotient;
    # 4: 1 - (subnormal * x3) / 3; 5: d = 0, b = 0 -> NaN; 6: depends on 2 (-0) and 3
    lists = [[(0, 0.0)], [(1, -0.0)], [(2, 2.0)], [(3, 4.0)], [(3, tiny), (4, 3.0)], [(5, 0.0)], [(6, 1.0), (2, 5.0), (3, 1.0)]]
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    ci = np.array([c for l in lists for c, _ in l], np.int32)
    va = np.array([v for l in lists for _, v in l], f32)
    b = np.array([1.0, 1.0, -0.0, tiny * 3, 1.0, 0.0, 0.0], f32)
    A = _owned(capi, 7, rp, ci, va)
    A.trsv_plan("lower")
    got = _solve(gpu, A, b, "lower")
    want = G.solve(rp, ci, va, b, "lower")
    assert G.same(got, want) is None, G.same(got, want)
    assert got[0] == np.inf and got[1] == -np.inf and np.signbit(got[2]) and got[2] == 0 and np.isnan(got[5])
    assert 0 < got[3] < np.finfo(f32).tiny and got[3] == tiny * 3 / f32(4)
    # unit: a NaN stored on the diagonal changes nothing
    n, rp, ci, va, b = G.generic_case()
    row = np.repeat(np.arange(n), np.diff(rp))
    A2 = _owned(capi, n, rp, ci, np.where(ci == row, f32(np.nan), va))
    for uplo in UPLOS:
        A2.trsv_plan(uplo)
        assert G.same(_solve(gpu, A2, b, uplo, unit=True), _want("generic", uplo, True)) is None
    A.close()
    A2.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_and_repeated_diagonals_are_refused_and_unit_still_solves(pkg, gpu):
    import torch
    capi = pkg.capi
    n, rp, ci, va, b = G.generic_case()
    row = np.repeat(np.arange(n), np.diff(rp))
    d_b, x = _dev(gpu, b), torch.full((n,), 7.0, device=gpu)
    # missing: row 41's diagonal removed; repeated: row 77's stored twice
    keep = ~((ci == row) & (row == 41))
    rp_m = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))]).astype(np.int32)
    at = int(np.flatnonzero((ci == row) & (row == 77))[0])
    ci_r, va_r = np.insert(ci, at, 77), np.insert(va, at, va[at])
    rp_r = rp + (np.arange(n + 1) > 77)
    for (rp_, ci_, va_), bad_row in (((rp_m, ci[keep], va[keep]), 41), ((rp_r.astype(np.int32), ci_r, va_r), 77)):
        A = _owned(capi, n, rp_, ci_, va_)
        for uplo in UPLOS:
            A.trsv_plan(uplo)
            assert A.trsv_plan_info(uplo)["bad_diag_row"] == bad_row
            with pytest.raises(capi.SpmvError, match=f"spmv_csr_trsv: row {bad_row} has no diagonal entry or more than one") as e:
                A.trsv(d_b, x, uplo=uplo)
            assert e.value.status == capi.ERR_INVALID
            torch.cuda.synchronize()
            assert torch.all(x == 7.0), "nothing is launched"
            got = _solve(gpu, A, b, uplo, unit=True)
            assert G.same(got, G.solve(rp_, ci_, va_, b, uplo, unit=True)) is None
        A.close()


@pytest.mark.gpu
def test_refusals_leave_nothing_behind(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    n, rp, ci, va, b = G.generic_case()
    A = _owned(capi, n, rp, ci, va)
    wide = capi.CsrMatrix.from_host(4, 5, np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    d_b, x = _dev(gpu, b), torch.full((n,), 7.0, device=gpu)

    def refused(rc, start):
        assert rc == capi.ERR_INVALID, start
        assert lib.spmv_last_error().decode().startswith(start), lib.spmv_last_error().decode()

    info = (C.c_int64 * 8)()
    free = []
    for _ in range(3):
        refused(lib.spmv_csr_trsv_plan(wide._h, 0, 0, None), "spmv_csr_trsv_plan: the handle is 4 x 5")
        refused(lib.spmv_csr_trsv(wide._h, 0, 0, d_b.data_ptr(), x.data_ptr(), None), "spmv_csr_trsv: the handle is 4 x 5")
        for uplo in (2, -1):
            refused(lib.spmv_csr_trsv_plan(A._h, uplo, 0, None), f"spmv_csr_trsv_plan: uplo = {uplo}")
            refused(lib.spmv_csr_trsv(A._h, uplo, 0, d_b.data_ptr(), x.data_ptr(), None), f"spmv_csr_trsv: uplo = {uplo}")
            assert lib.spmv_csr_trsv_plan_bytes(A._h, uplo) == capi.ERR_INVALID
        refused(lib.spmv_csr_trsv_plan(A._h, 0, -1, None), "spmv_csr_trsv_plan: thin_rows = -1")
        # no plan yet for the upper triangle
        refused(lib.spmv_csr_trsv(A._h, 1, 0, d_b.data_ptr(), x.data_ptr(), None), "spmv_csr_trsv: the handle has no plan for the upper")
        refused(lib.spmv_csr_trsv_plan_info(A._h, 1, info), "spmv_csr_trsv_plan_info: the handle has no plan")
        refused(lib.spmv_csr_trsv_describe(A._h, 1, C.create_string_buffer(8), 8), "spmv_csr_trsv_describe: the handle has no plan")
        capi.check(lib.spmv_csr_trsv_plan(A._h, 0, 0, None))
        for diag in (2, -1):
            refused(lib.spmv_csr_trsv(A._h, 0, diag, d_b.data_ptr(), x.data_ptr(), None), f"spmv_csr_trsv: diag = {diag}")
        refused(lib.spmv_csr_trsv(A._h, 0, 0, None, x.data_ptr(), None), "spmv_csr_trsv: null array")
        refused(lib.spmv_csr_trsv(A._h, 0, 0, d_b.data_ptr(), None, None), "spmv_csr_trsv: null array")
        refused(lib.spmv_csr_trsv_plan_rows(A._h, 0, None, None), "spmv_csr_trsv_plan_rows: null array")
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert torch.all(x == 7.0), "nothing is launched by a refused call"
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    # plans made again and again replace each other; a closed handle takes its plans along
    held = torch.cuda.memory_allocated()
    free = []
    for _ in range(3):
        B = _owned(capi, n, rp, ci, va)
        for uplo in UPLOS:
            B.trsv_plan(uplo)
            B.trsv_plan(uplo, thin_rows=3)
            assert B.trsv_plan_bytes(uplo) > 0
        B.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    assert torch.cuda.memory_allocated() == held
    A.close()
    wide.close()


# ---- 8. edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_rows_one_row_and_no_nonzeros(pkg, gpu):
    import torch
    capi = pkg.capi
    empty = capi.CsrMatrix.from_host(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    for uplo in UPLOS:
        empty.trsv_plan(uplo)
        info = empty.trsv_plan_info(uplo)
        assert (info["levels"], info["launches"], info["widest"], info["bad_diag_row"]) == (0, 0, 0, -1)
        lp, od = empty.trsv_plan_rows(uplo)
        assert lp.tolist() == [0] and od.size == 0
        for unit in (False, True):
            assert empty.trsv(torch.zeros(0, device=gpu), uplo=uplo, unit=unit).numel() == 0
    one = capi.CsrMatrix.from_host(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([3.0], f32))
    hollow = capi.CsrMatrix.from_host(5, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    b5 = np.array([1.5, -2.0, 0.0, np.inf, 1e-40], f32)
    for uplo in UPLOS:
        one.trsv_plan(uplo)
        assert _solve(gpu, one, np.array([1.0], f32), uplo)[0] == f32(1.0) / f32(3.0)
        assert _solve(gpu, one, np.array([1.0], f32), uplo, unit=True)[0] == 1.0
        hollow.trsv_plan(uplo)
        info = hollow.trsv_plan_info(uplo)
        assert (info["levels"], info["launches"], info["widest"], info["bad_diag_row"]) == (1, 1, 5, 0)
        assert G.same(_solve(gpu, hollow, b5, uplo, unit=True), b5) is None      # x = b
        with pytest.raises(capi.SpmvError, match="spmv_csr_trsv: row 0 has no diagonal"):
            hollow.trsv(_dev(gpu, b5), uplo=uplo)
    for h in (empty, one, hollow):
        h.close()


# ---- 9. downstream -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", (False, True))
def test_gauss_seidel_equals_the_numpy_composition(pkg, gpu, oracle, symmetric):
    import torch
    n, rp, ci, va, b = G.stencil_case(pkg)
    A = _owned(pkg.capi, n, rp, ci, va)
    d_b, x = _dev(gpu, b), torch.zeros(n, device=gpu)
    state = pkg.solvers.gauss_seidel(A, d_b, x, sweeps=1, symmetric=symmetric)
    gc.collect()        # (tensors of earlier tests that wait in a reference cycle go now, not during the sweeps below)
    held = torch.cuda.memory_allocated()
    pkg.solvers.gauss_seidel(A, d_b, x, sweeps=2, symmetric=symmetric, state=state)
    assert torch.cuda.memory_allocated() == held, "a sweep after the first allocates nothing"
    torch.cuda.synchronize()
    want = G.gauss_seidel(lambda v: oracle.spmv(rp, ci, va, v), rp, ci, va, b, np.zeros(n, f32), 3, symmetric)
    bad = G.same(x.cpu().numpy(), want)
    assert bad is None, bad
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("uplo,unit", [("lower", False), ("upper", False), ("lower", True)])
def test_tester_executable_solves_a_file(pkg, gpu, tmp_path, uplo, unit):
    import subprocess
    rng = np.random.default_rng(31)
    n = 150                                                     # the reader sorts every row and sums duplicates: sorted, duplicate-free rows
    cols = [rng.choice(n, int(rng.integers(40, 50)) if i % 30 == 7 else int(rng.integers(0, 7)), replace=False) for i in range(n)]
    rp, ci, va = G.from_rows(n, [c[c != i] for i, c in enumerate(cols)], rng)
    row = np.repeat(np.arange(n), np.diff(rp))
    by = np.lexsort((ci, row))
    ci, va = ci[by], va[by]
    lines = [f"{i + 1} {j + 1} {float(v)!r}" for i, j, v in zip(row, ci, va)]
    (tmp_path / "A.mtx").write_text("%%MatrixMarket matrix coordinate real general\n" + f"{n} {n} {len(ci)}\n" + "\n".join(lines) + "\n")
    out = tmp_path / "x.txt"
    cmd = [str(pkg.capi.TESTER_PATH), "--mtx", str(tmp_path / "A.mtx"), "--trsv", uplo, "--out", str(out)] + (["--unit"] if unit else [])
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "========== OK ===========" in run.stdout, run.stdout + run.stderr
    assert f"spmv_csr_trsv: trsv {uplo} levels=" in run.stdout
    got = np.array(out.read_text().split(), dtype=np.float64).astype(f32)                # %.9g round-trips a float
    want = G.solve(rp, ci, va, np.ones(n, f32), uplo, unit)
    assert G.same(got, want) is None, G.same(got, want)


@pytest.mark.gpu
def test_a_sum_handle_gets_its_diagonal_from_add_and_solves(pkg, gpu):
    capi = pkg.capi
    rng = np.random.default_rng(23)
    n = 300
    cols = [rng.choice(n, int(rng.integers(0, 9)), replace=False) for _ in range(n)]
    cols = [c[c != i] for i, c in enumerate(cols)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    va = (rng.uniform(0.05, 1.0, ci.size) * rng.choice([-1.0, 1.0], ci.size)).astype(f32)
    sigma = f32(9.5)                                            # >= 8 terms of at most 1 / 0.9
    A = capi.CsrMatrix.from_host(n, n, rp, ci, va)
    eye = capi.CsrMatrix.from_host(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, f32))
    S = A.add(eye, 1.0, float(sigma), "union")
    s_rp, s_ci, s_va = S.download()
    b = G.rhs(n, rng)
    for uplo in UPLOS:
        S.trsv_plan(uplo)
        assert S.trsv_plan_info(uplo)["bad_diag_row"] == -1
        want = G.solve(s_rp, s_ci, s_va, b, uplo)
        assert np.all(np.isfinite(want)) and np.all(want != 0)
        bad = G.same(_solve(gpu, S, b, uplo), want)
        assert bad is None, bad
    for h in (S, eye, A):
        h.close()
