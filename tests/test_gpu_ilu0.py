"""GPU (-m gpu): spmv_csr_ilu0 / _values / _solve / _pivot (include/spmv_hip.h "the incomplete factorisation").

The expectation is always tests/_ilu0.py (numpy), never a kernel of this library, and M's values are compared bit for bit (the
uint32 view; a NaN matches any NaN).  That the generic inputs are row-dominant (finite factors, pivots of at least 0.1 |a_ii|)
and tell the contract's order from three wrong ones is proved in tests/test_ilu0_host.py.

  1 factorisation  generic 257 x 257, a diagonal, a tridiagonal chain across the per-launch cap, 5000 rows behind 10, level sizes
                   around thin_rows = 70, stencil7(8), stored row lengths 1 .. 129 and 5000, an arrow -- each under thin_rows 1,
                   the default and 1 << 30
  2 purity         two streams, borrowed against owned arrays, M's pattern is A's
  3 the solve      ilu0_solve against _ilu0.apply (through _trsv.solve), in place, a poisoned z
  4 new values     ilu0_values after a rewrite of A's borrowed vals, and in a replayed graph together with ilu0_solve; no allocation
  5 special values a NaN and an Inf in A; a zero pivot and ilu0_pivot; -0 and subnormals
  6 refusals       shapes, order, diagonal, null handles, non-factor handles, m == a, a changed nnz, the other makers' companions
  7 edges          rows = 0 and 1
  8 downstream     add(unsorted, empty).add(I).ilu0(); sparse_sgemv --ilu0
"""
import ctypes as C

import numpy as np
import pytest

import _ilu0 as G
import _trsv as T

MIB = 1 << 20
f32 = np.float32
THINS = (1, 0, 1 << 30)


def _dev(gpu, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _owned(capi, n, rp, ci, va):
    return capi.CsrMatrix.from_host(n, n, rp, ci, va)


def _borrowed(capi, gpu, n, rp, ci, va):
    t = (_dev(gpu, rp, np.int32), _dev(gpu, ci, np.int32), _dev(gpu, va, np.float32))
    return capi.CsrMatrix.from_device(n, n, *t), t


_CASES = {
    "generic": G.generic_case,
    "diagonal": G.diagonal_case,
    "tridiagonal": G.tridiagonal_case,
    "fan": G.fan_case,
    "stairs": G.stairs_case,
    "lengths": G.lengths_case,
    "arrow": G.arrow_case,
}


def _case(pkg, key):
    return G.stencil_case(pkg) if key == "stencil" else _CASES[key]()


_want_cache = {}


def _want(pkg, key):
    """The contract's M for a shared case, computed once."""
    if key not in _want_cache:
        n, rp, ci, va = _case(pkg, key)
        _want_cache[key] = G.factor(rp, ci, va)
    return _want_cache[key]


def _vals(M):
    import torch
    torch.cuda.synchronize()
    return M.download()[2]


# ---- 1. factorisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thin", THINS)
@pytest.mark.parametrize("key", list(_CASES) + ["stencil"])
def test_factor_equals_the_contract_bit_for_bit(pkg, gpu, key, thin):
    capi = pkg.capi
    assert capi.SPMV_ILU0_SERIAL_MAX == G.SERIAL_MAX
    n, rp, ci, va = _case(pkg, key)
    A = _owned(capi, n, rp, ci, va)
    assert A.ilu0_plan_bytes() == 0
    M = A.ilu0(thin_rows=thin)
    m_rp, m_ci, m_va = M.download()
    assert np.array_equal(m_rp, rp) and np.array_equal(m_ci, ci), "M's pattern is A's"
    bad = G.same(m_va, _want(pkg, key))
    assert bad is None, f"{key} thin_rows={thin}: {bad}"
    assert M.ilu0_pivot() == -1
    lo, up = M.trsv_plan_info("lower"), M.trsv_plan_info("upper")
    assert lo["bad_diag_row"] == up["bad_diag_row"] == -1
    assert M.ilu0_plan_bytes() == M.trsv_plan_bytes("lower") + M.trsv_plan_bytes("upper") + 4
    if thin:
        assert lo["thin_rows"] == up["thin_rows"] == thin
    if key == "tridiagonal":
        assert lo["levels"] == 3000 and lo["launches"] == 3                     # three merged launches at the cap
    if key == "fan":
        assert (lo["levels"], lo["widest"]) == (2, 5000)
    if key == "stencil":
        assert lo["levels"] == 22
    M.close()
    A.close()


@pytest.mark.gpu
def test_level_sizes_around_an_explicit_thin_threshold(pkg, gpu):
    n, rp, ci, va = G.stairs_case()
    A = _owned(pkg.capi, n, rp, ci, va)
    M = A.ilu0(thin_rows=70)
    lo = M.trsv_plan_info("lower")
    assert np.array_equal(np.diff(M.trsv_plan_rows("lower")[0]), (69, 70, 71, 70, 69, 1, 71))
    assert lo["thin_rows"] == 70 and lo["launches"] == 4                        # [69, 70] [71] [70, 69, 1] [71]
    bad = G.same(_vals(M), _want(pkg, "stairs"))
    assert bad is None, bad
    M.close()
    A.close()


EDGE_STAIRS = (255, 256, 257, 256, 255, 1, 257)             # around the peel's workgroup of 256 rows and SPMV_TRSV_THIN_DEFAULT


@pytest.mark.gpu
def test_a_chain_deeper_than_one_launch_of_the_small_peel(pkg, gpu):
    """4100 levels of one row: the plans' one-workgroup peel retires 4096 levels a launch and the host loop goes on from the live
    frontier.  The factor, the factor again from new values, and the solve, bit for bit."""
    import torch
    n, rp, ci, va = G.tridiagonal_case(4100)
    A, (_, _, d_va) = _borrowed(pkg.capi, gpu, n, rp, ci, va)
    M = A.ilu0()
    lo, up = M.trsv_plan_info("lower"), M.trsv_plan_info("upper")
    for uplo, info in (("lower", lo), ("upper", up)):
        assert (info["levels"], info["widest"], info["launches"]) == (n, 1, -(-n // info["level_cap"])), info
        lp, od = T.order(T.levels(rp, ci, uplo))
        got_lp, got_od = M.trsv_plan_rows(uplo)
        assert np.array_equal(got_lp, lp) and np.array_equal(got_od, od), f"{uplo}: the plan's rows"
    want = G.factor(rp, ci, va)
    assert G.same(_vals(M), want) is None, G.same(_vals(M), want)
    r = T.rhs(n, np.random.default_rng(5))
    z = M.ilu0_solve(_dev(gpu, r))
    torch.cuda.synchronize()
    assert G.same(z.cpu().numpy(), G.apply(rp, ci, want, r)) is None
    row = np.repeat(np.arange(n), np.diff(rp))
    nv = np.where(ci == row, va * f32(1.5), va * f32(0.75)).astype(f32)          # still dominant
    d_va.copy_(_dev(gpu, nv))
    M.ilu0_values(A)
    want2 = G.factor(rp, ci, nv)
    assert G.differs(want, want2) > n and G.same(_vals(M), want2) is None, "after ilu0_values"
    z = M.ilu0_solve(_dev(gpu, r))
    torch.cuda.synchronize()
    assert G.same(z.cpu().numpy(), G.apply(rp, ci, want2, r)) is None
    assert M.ilu0_pivot() == -1
    M.close()
    A.close()


@pytest.mark.gpu
def test_level_sizes_around_the_peel_workgroup_and_the_default_thin_threshold(pkg, gpu):
    n, rp, ci, va = G.stairs_case(EDGE_STAIRS)
    A = _owned(pkg.capi, n, rp, ci, va)
    M = A.ilu0(thin_rows=0)
    lo = M.trsv_plan_info("lower")
    assert np.array_equal(np.diff(M.trsv_plan_rows("lower")[0]), EDGE_STAIRS)
    assert lo["thin_rows"] == 256 and lo["launches"] == 4                       # [255, 256] [257] [256, 255, 1] [257]
    lp, od = T.order(T.levels(rp, ci, "upper"))
    got_lp, got_od = M.trsv_plan_rows("upper")
    assert np.array_equal(got_lp, lp) and np.array_equal(got_od, od)
    want = G.factor(rp, ci, va)
    bad = G.same(_vals(M), want)
    assert bad is None, bad
    r = T.rhs(n, np.random.default_rng(6))
    z = M.ilu0_solve(_dev(gpu, r))
    assert G.same(z.cpu().numpy(), G.apply(rp, ci, want, r)) is None
    M.close()
    A.close()


# ---- 2. purity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_purity_streams_and_owners(pkg, gpu):
    import torch
    capi = pkg.capi
    n, rp, ci, va = G.generic_case()
    want = _want(pkg, "generic")
    A, keep = _borrowed(capi, gpu, n, rp, ci, va)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    M1, M2 = A.ilu0(stream=s1), A.ilu0(thin_rows=7, stream=s2)
    M1.ilu0_values(A, stream=s1)
    M2.ilu0_values(A, stream=s2)                           # the two handles factor the same arrays at the same time
    torch.cuda.synchronize()
    assert G.same(_vals(M1), want) is None and G.same(_vals(M2), want) is None
    assert M1.ilu0_pivot(stream=s1) == -1 and M2.ilu0_pivot(stream=s2) == -1
    for h in (M1, M2, A):
        h.close()


# ---- 3. the solve ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", ("generic", "arrow"))
def test_solve_equals_apply_in_place_and_over_a_poisoned_z(pkg, gpu, key):
    import torch
    n, rp, ci, va = _case(pkg, key)
    A = _owned(pkg.capi, n, rp, ci, va)
    M = A.ilu0()
    r = T.rhs(n, np.random.default_rng(3))
    want = G.apply(rp, ci, _want(pkg, key), r)
    assert np.all(np.isfinite(want))
    d_r = _dev(gpu, r)
    z = torch.full((n,), float("nan"), device=gpu)
    assert M.ilu0_solve(d_r, z) is z
    fresh = M.ilu0_solve(d_r)
    inplace = d_r.clone()
    assert M.ilu0_solve(inplace, inplace) is inplace
    torch.cuda.synchronize()
    for name, got in (("poisoned z", z), ("a new z", fresh), ("in place", inplace)):
        bad = G.same(got.cpu().numpy(), want)
        assert bad is None, f"{name}: {bad}"
    assert torch.equal(d_r.cpu(), torch.from_numpy(r)), "r is only read"
    M.close()
    A.close()


# ---- 4. new values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_values_after_a_rewrite_in_a_replayed_graph_and_without_allocation(pkg, gpu):
    import torch
    n, rp, ci, va = G.generic_case()
    A, (_, _, d_va) = _borrowed(pkg.capi, gpu, n, rp, ci, va)
    M = A.ilu0()
    r = T.rhs(n, np.random.default_rng(4))
    d_r, z = _dev(gpu, r), torch.full((n,), float("nan"), device=gpu)
    rng = np.random.default_rng(18)
    row = np.repeat(np.arange(n), np.diff(rp))

    def rewrite():                                          # (the diagonal grows, the rest shrinks: still dominant)
        nv = np.where(ci == row, va * f32(rng.uniform(1.0, 2.0)), va * rng.uniform(0.2, 1.0, va.size).astype(f32)).astype(f32)
        d_va.copy_(_dev(gpu, nv))
        m = G.factor(rp, ci, nv)
        return m, G.apply(rp, ci, m, r)

    assert G.same(_vals(M), _want(pkg, "generic")) is None
    m1, z1 = rewrite()
    assert G.same(_vals(M), _want(pkg, "generic")) is None, "M holds its own values"
    M.ilu0_values(A)
    M.ilu0_solve(d_r, z)
    assert G.same(_vals(M), m1) is None, "after a rewrite of A's vals"
    assert G.same(z.cpu().numpy(), z1) is None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        M.ilu0_values(A)
        M.ilu0_solve(d_r, z)
    m2, z2 = rewrite()
    z.fill_(float("nan"))
    g.replay()
    assert G.same(_vals(M), m2) is None, "from a replayed graph"
    assert G.same(z.cpu().numpy(), z2) is None
    assert G.differs(m1, m2) > va.size // 2 and M.ilu0_pivot() == -1
    # a second ilu0_values and a second solve allocate nothing
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info()[0]]
    for _ in range(3):
        M.ilu0_values(A)
        M.ilu0_solve(d_r, z)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    M.close()
    A.close()


# ---- 5. special values --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("value,at_row", [(np.nan, 40), (np.inf, 100), (-np.inf, 8)])
def test_nan_and_inf_in_a_reach_exactly_the_entries_the_contract_says(pkg, gpu, value, at_row):
    n, rp, ci, va = G.generic_case()
    clean = _want(pkg, "generic")
    v = va.copy()
    at = int(rp[at_row]) + (int(rp[at_row + 1]) - int(rp[at_row])) // 2
    v[at] = value
    want = G.factor(rp, ci, v)
    touched = ~np.isfinite(want)
    assert 0 < touched.sum() < va.size
    A = _owned(pkg.capi, n, rp, ci, v)
    M = A.ilu0()
    got = _vals(M)
    assert G.same(got, want) is None, G.same(got, want)
    assert np.array_equal(~np.isfinite(got), touched), "exactly the entries the contract says"
    assert G.same(got[:rp[at_row]], clean[:rp[at_row]]) is None, "the rows before it do not depend on it"
    d = G.diag_positions(rp, ci)
    bad_pivots = np.flatnonzero(~np.isfinite(want[d]) | (want[d] == 0))
    assert M.ilu0_pivot() == (int(bad_pivots[0]) if bad_pivots.size else -1)
    M.close()
    A.close()


@pytest.mark.gpu
def test_zero_pivot_minus_zero_and_subnormals(pkg, gpu):
    capi = pkg.capi
    tiny = np.float32(1e-41)                                    # subnormal
    # a diagonal matrix of 12 rows with the block [[1, 1], [1, 1]] at rows 5, 6: u_66 = 1 - 1 * 1 = 0 exactly.  Row 6 also stores
    # (6, 9); row 9 stores (9, 6): l = 3 / 0 = Inf, u_99 = 1 - Inf * 2 = -Inf.  Row 2: d = -0.  Row 3: subnormal / 4 below row 10.
    lists = [[(i, 2.0 + i)] for i in range(12)]
    lists[5], lists[6], lists[9] = [(5, 1.0), (6, 1.0)], [(5, 1.0), (6, 1.0), (9, 2.0)], [(6, 3.0), (9, 1.0)]
    lists[2] = [(2, -0.0)]
    lists[3] = [(3, 4.0), (10, tiny)]
    lists[10] = [(3, tiny * 3), (10, 1.0)]
    lists[11] = [(2, 1.0), (11, 5.0)]                           # 1 / -0 = -Inf
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    ci = np.array([c for l in lists for c, _ in l], np.int32)
    va = np.array([v for l in lists for _, v in l], f32)
    want = G.factor(rp, ci, va)
    A = _owned(capi, 12, rp, ci, va)
    M = A.ilu0()
    got = _vals(M)
    assert G.same(got, want) is None, G.same(got, want)
    d = G.diag_positions(rp, ci)
    assert got[d[6]] == 0 and got[rp[9]] == np.inf and got[d[9]] == -np.inf
    assert got[d[2]] == 0 and np.signbit(got[d[2]]) and got[rp[11]] == -np.inf
    assert 0 < got[rp[10]] < np.finfo(f32).tiny and got[rp[10]] == tiny * 3 / f32(4)
    assert M.ilu0_pivot() == 2                                  # the smallest of the rows 2, 6, 9
    va2 = va.copy()
    va2[d[2]] = 1.0
    A2 = _owned(capi, 12, rp, ci, va2)
    M.ilu0_values(A2)
    assert M.ilu0_pivot() == 6, "the pivot word is reset by every factorisation"
    va3 = va2.copy()
    va3[d[6]] = 3.0
    A3 = _owned(capi, 12, rp, ci, va3)
    M.ilu0_values(A3)
    assert M.ilu0_pivot() == -1 and G.same(_vals(M), G.factor(rp, ci, va3)) is None
    for h in (M, A, A2, A3):
        h.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_out_untouched(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    n, rp, ci, va = G.generic_case()
    A = _owned(capi, n, rp, ci, va)
    M = A.ilu0()
    before = _vals(M).copy()
    wide = capi.CsrMatrix.from_host(4, 5, np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    row = np.repeat(np.arange(n), np.diff(rp))
    # an unsorted row 8 (its first two columns swapped), a repeated column in row 24, row 41 without its diagonal
    ci_u = ci.copy()
    ci_u[[rp[8], rp[8] + 1]] = ci[[rp[8] + 1, rp[8]]]
    ci_r = ci.copy()
    ci_r[rp[24] + 1] = ci[rp[24]]
    keep = ~((ci == row) & (row == 41))
    rp_m = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))]).astype(np.int32)
    unsorted, repeated = _owned(capi, n, rp, ci_u, va), _owned(capi, n, rp, ci_r, va)
    hollow = _owned(capi, n, rp_m, ci[keep], va[keep])
    shorter = hollow                                        # (also: another nnz than M recorded)
    d_r, z = torch.ones(n, device=gpu), torch.full((n,), 7.0, device=gpu)
    st = torch.cuda.current_stream().cuda_stream

    def refused(rc, start, also=""):
        assert rc == capi.ERR_INVALID, start
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(start) and also in msg, msg

    free = []
    for _ in range(3):
        out = C.c_void_p(77)
        refused(lib.spmv_csr_ilu0(wide._h, 0, st, C.byref(out)), "spmv_csr_ilu0: the handle is 4 x 5")
        refused(lib.spmv_csr_ilu0(unsorted._h, 0, st, C.byref(out)), "spmv_csr_ilu0: row 8 is not strictly ascending", "SPMV_ADD_UNION) sorts a matrix")
        refused(lib.spmv_csr_ilu0(repeated._h, 0, st, C.byref(out)), "spmv_csr_ilu0: row 24 is not strictly ascending", "gives it a diagonal")
        refused(lib.spmv_csr_ilu0(hollow._h, 0, st, C.byref(out)), "spmv_csr_ilu0: row 41 stores no diagonal", "gives it a diagonal")
        refused(lib.spmv_csr_ilu0(None, 0, st, C.byref(out)), "spmv_csr_ilu0: null argument")
        refused(lib.spmv_csr_ilu0(A._h, 0, st, None), "spmv_csr_ilu0: null argument")
        refused(lib.spmv_csr_ilu0(A._h, -1, st, C.byref(out)), "spmv_csr_ilu0: thin_rows = -1")
        assert out.value == 77, "*out is untouched"
        # only a factor handle factors again, solves and reports a pivot
        piv = C.c_int64(5)
        refused(lib.spmv_csr_ilu0_values(A._h, A._h, st), "spmv_csr_ilu0_values: the handle is no factor handle")
        refused(lib.spmv_csr_ilu0_solve(A._h, d_r.data_ptr(), z.data_ptr(), st), "spmv_csr_ilu0_solve: the handle is no factor handle")
        refused(lib.spmv_csr_ilu0_pivot(A._h, st, C.byref(piv)), "spmv_csr_ilu0_pivot: the handle is no factor handle")
        assert piv.value == 5 and A.ilu0_plan_bytes() == 0
        refused(lib.spmv_csr_ilu0_values(M._h, M._h, st), "spmv_csr_ilu0_values: a is m itself")
        refused(lib.spmv_csr_ilu0_values(M._h, None, st), "spmv_csr_ilu0_values: null argument")
        refused(lib.spmv_csr_ilu0_values(M._h, shorter._h, st), f"spmv_csr_ilu0_values: a is {n} x {n} with {va.size - 1} nonzeros")
        refused(lib.spmv_csr_ilu0_values(M._h, wide._h, st), "spmv_csr_ilu0_values: a is 4 x 5")
        refused(lib.spmv_csr_ilu0_solve(M._h, None, z.data_ptr(), st), "spmv_csr_ilu0_solve: null array")
        refused(lib.spmv_csr_ilu0_pivot(M._h, st, None), "spmv_csr_ilu0_pivot: null row")
        # the other makers' companions refuse a factor handle
        refused(lib.spmv_csr_transpose_values(M._h, A._h, st), "spmv_csr_transpose_values: the handle has no map")
        refused(lib.spmv_csr_select_values(M._h, A._h, st), "spmv_csr_select_values: the handle has no map")
        refused(lib.spmv_csr_spgemm_values(M._h, A._h, A._h, st), "spmv_csr_spgemm_values: the handle has no plan")
        refused(lib.spmv_csr_add_values(M._h, A._h, A._h, 1.0, 1.0, st), "spmv_csr_add_values: the handle has no plan")
        if torch.cuda.device_count() > 1:                    # another current device than the handle's
            with torch.cuda.device(1):
                refused(lib.spmv_csr_ilu0(A._h, 0, None, C.byref(out)), "spmv_csr_ilu0")
                refused(lib.spmv_csr_ilu0_values(M._h, A._h, None), "spmv_csr_ilu0_values")
                refused(lib.spmv_csr_ilu0_solve(M._h, d_r.data_ptr(), z.data_ptr(), None), "spmv_csr_ilu0_solve")
                refused(lib.spmv_csr_ilu0_pivot(M._h, None, C.byref(piv)), "spmv_csr_ilu0_pivot")
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert torch.all(z == 7.0), "nothing is launched by a refused call"
    assert G.same(_vals(M), before) is None, "M is untouched by a refused call"
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    # factor handles made again and again take their plans along when they are closed
    held = torch.cuda.memory_allocated()
    free = []
    for _ in range(3):
        B = A.ilu0(thin_rows=3)
        assert B.ilu0_plan_bytes() > 0
        B.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    assert torch.cuda.memory_allocated() == held
    # every spmv_csr_* call accepts a factor handle
    x, y = torch.ones(n, device=gpu), torch.empty(n, device=gpu)
    M.plan(capi.SCALAR)
    M.run(capi.SCALAR, x, y)
    torch.cuda.synchronize()
    want = np.bincount(row, weights=before.astype(np.float64), minlength=n)
    assert np.allclose(y.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    Mt = M.transpose()
    assert Mt.nnz == M.nnz
    for h in (Mt, M, A, wide, unsorted, repeated, hollow):
        h.close()


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_rows_and_one_row(pkg, gpu):
    import torch
    capi = pkg.capi
    empty = capi.CsrMatrix.from_host(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    M0 = empty.ilu0()
    assert (M0.rows, M0.cols, M0.nnz) == (0, 0, 0) and M0.ilu0_pivot() == -1
    M0.ilu0_values(empty)
    assert M0.ilu0_solve(torch.zeros(0, device=gpu)).numel() == 0
    assert M0.trsv_plan_info("lower")["launches"] == 0
    one = capi.CsrMatrix.from_host(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([3.0], f32))
    M1 = one.ilu0()
    assert _vals(M1).tolist() == [3.0] and M1.ilu0_pivot() == -1
    z = M1.ilu0_solve(torch.ones(1, device=gpu))
    torch.cuda.synchronize()
    assert z.cpu().numpy()[0] == f32(1.0) / f32(3.0)
    zero = capi.CsrMatrix.from_host(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([0.0], f32))
    M1.ilu0_values(zero)
    assert M1.ilu0_pivot() == 0
    hollow = capi.CsrMatrix.from_host(5, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    with pytest.raises(capi.SpmvError, match="spmv_csr_ilu0: row 0 stores no diagonal"):
        hollow.ilu0()
    for h in (M0, M1, empty, one, zero, hollow):
        h.close()


# ---- 8. downstream ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_chain_of_sums_sorts_gives_a_diagonal_and_factors(pkg, gpu):
    capi = pkg.capi
    n, rp, ci, va, _ = T.generic_case()                     # unsorted rows with repeated columns
    A = capi.CsrMatrix.from_host(n, n, rp, ci, va)
    with pytest.raises(capi.SpmvError, match="spmv_csr_ilu0: row \\d+ is not strictly ascending"):
        A.ilu0()
    empty = capi.CsrMatrix.from_host(n, n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    eye = capi.CsrMatrix.from_host(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, f32))
    row = np.repeat(np.arange(n), np.diff(rp))
    heaviest = np.bincount(row, weights=np.abs(va.astype(np.float64)), minlength=n).max()
    sigma = float(np.ceil(2 * heaviest / 0.9))              # the sum's diagonal is sigma + a_ii >= sigma - heaviest >= the row's rest / 0.9
    S0 = A.add(empty, 1.0, 0.0, "union")
    S = S0.add(eye, 1.0, sigma, "union")
    s_rp, s_ci, s_va = S.download()
    assert G.is_sorted(s_rp, s_ci) and G.dominance(s_rp, s_ci, s_va) <= 0.9
    M = S.ilu0()
    want = G.factor(s_rp, s_ci, s_va)
    assert np.all(np.isfinite(want))
    bad = G.same(_vals(M), want)
    assert bad is None, bad
    assert M.ilu0_pivot() == -1
    for h in (M, S, S0, eye, empty, A):
        h.close()


@pytest.mark.gpu
def test_tester_executable_factors_a_file(pkg, gpu, tmp_path):
    import subprocess
    rng = np.random.default_rng(32)
    n = 150
    cols = [rng.choice(n, int(rng.integers(40, 50)) if i % 30 == 7 else int(rng.integers(0, 7)), replace=False) for i in range(n)]
    rp, ci, va = G.dominant_rows(n, cols, rng)
    row = np.repeat(np.arange(n), np.diff(rp))
    lines = [f"{i + 1} {j + 1} {float(v)!r}" for i, j, v in zip(row, ci, va)]
    (tmp_path / "A.mtx").write_text("%%MatrixMarket matrix coordinate real general\n" + f"{n} {n} {len(ci)}\n" + "\n".join(lines) + "\n")
    out = tmp_path / "m.txt"
    run = subprocess.run([str(pkg.capi.TESTER_PATH), "--mtx", str(tmp_path / "A.mtx"), "--ilu0", "--out", str(out)], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0 and "========== OK ===========" in run.stdout, run.stdout + run.stderr
    assert f"spmv_csr_ilu0: rows={n} nnz={len(ci)} levels=" in run.stdout and " pivot=-1 " in run.stdout
    got = np.array(out.read_text().split(), dtype=np.float64).astype(f32)                # %.9g round-trips a float
    want = G.factor(rp, ci, va)
    assert G.same(got, want) is None, G.same(got, want)
