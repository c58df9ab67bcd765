"""GPU (-m gpu): spmv_csr_spgemm / spmv_csr_spgemm_values (include/spmv_hip.h "the sparse product").

The expectation is always tests/_spgemm.py (numpy), never a kernel of this library, and every result is compared bit for bit:
row_ptr, col_idx and the uint32 view of vals (a NaN matches any NaN: its sign and payload are the hardware's).  That the
inputs of G.ORDER_CASES tell the contract's order from two wrong ones is proved in tests/test_spgemm_host.py.

  1 generic        257 x 193 times 193 x 300, unsorted rows of 0 .. 40 with repeated columns on both sides, values over 2^20
  2 class edges    terms and distinct columns T - 1, T, T + 1 around every boundary of SPGEMM_CLASS_SLOTS, the full table
  3 one column     p = 1 under a row of 600 entries; B's rows repeating column 0 three times
  4 oversized      44 800 distinct columns in one row; 44 800 terms on 64 columns
  5 type edges     2^31 - 1 columns; m = 0, n = 0, p = 0, nnz = 0 on either side
  6 values         +-Inf, NaN, -0, subnormals, stored zeros, a cancelling pair
  7 purity         two streams, borrowed against owned operands, row blocks, a == b
  8 against SpMM   the chain is spmv_csr_spmm's, gathered at C's pattern
  9 downstream     validate, SPMV_SCALAR / SPMV_AUTO / SPMV_XSKIP on C, the transpose of C
 10 _values        in-place rewrites, a captured graph, the refusals
 11 refusals       shapes, keep_plan, 2^31 result entries (and no memory left behind)
 12 the layer      SparseLayer.composed
 13 the tester     sparse_sgemv --mtx A.mtx --spgemm B.mtx --out C.mtx
"""
import ctypes as C

import numpy as np
import pytest

import _spgemm as G
from _util import RTOL

MIB = 1 << 20


def _dev(gpu, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _owned(capi, mat):
    rows, cols, (rp, ci, va) = mat
    return capi.CsrMatrix.from_host(rows, cols, rp, ci, va)


def _borrowed(capi, gpu, mat):
    rows, cols, (rp, ci, va) = mat
    t = (_dev(gpu, rp, np.int32), _dev(gpu, ci, np.int32), _dev(gpu, va, np.float32))
    return capi.CsrMatrix.from_device(rows, cols, *t), t


def _check(c, want, what, shape=None):
    got = c.download()
    bad = G.same(got, want)
    assert bad is None, f"{what}: {bad}"
    assert c.nnz == len(want[1])
    if shape is not None:
        assert (c.rows, c.cols) == shape, what
    if len(want) > 3:
        assert c.spgemm_products == want[3], f"{what}: products {c.spgemm_products}, expected {want[3]}"
    return got


def _product(capi, a, b, key, what=None):
    """a @ b through owned handles against the contract (computed once per key)."""
    A, B = _owned(capi, a), _owned(capi, b)
    try:
        c = A.spgemm(B)
        try:
            _check(c, G.reference(key, a[2], b[2]), what or str(key), (a[0], b[1]))
            assert c.spgemm_plan_bytes() == 0 and c.transpose_map_bytes() == 0 and c.select_map_bytes() == 0
        finally:
            c.close()
    finally:
        A.close()
        B.close()


# ---- 1 .. 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_generic(pkg, gpu):
    a, b = G.generic_case()
    _product(pkg.capi, a, b, "generic")


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(4))
def test_class_edges(pkg, gpu, which):
    T = pkg.capi.SPGEMM_CLASS_SLOTS[which]
    a, b, spec = G.edge_case(T)
    assert (T, T) in spec                                           # the full table is among the rows
    _product(pkg.capi, a, b, ("edge", T), f"class edge {T}")


def test_there_are_four_classes(pkg):
    assert len(pkg.capi.SPGEMM_CLASS_SLOTS) == 4                    # what test_class_edges is parametrised over


@pytest.mark.gpu
@pytest.mark.parametrize("rep", [1, 3])
def test_one_column(pkg, gpu, rep):
    a, b = G.one_column_case(rep)
    _product(pkg.capi, a, b, ("one_column", rep))


@pytest.mark.gpu
def test_oversized_rows(pkg, gpu):
    a, b = G.oversized_case()
    want = G.reference("oversized", a[2], b[2])
    assert np.diff(want[0]).tolist() == [128, 44800, 0, 64, 64] and max(pkg.capi.SPGEMM_CLASS_SLOTS) < 44800
    _product(pkg.capi, a, b, "oversized")


# ---- 5. the edges of the types ---------------------------------------------------------------------------------------------------
def _csr(rows, cols, lists, vals=None):
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    ci = np.array([c for l in lists for c in l], np.int32)
    va = np.arange(1, ci.size + 1, dtype=np.float32) * np.float32(0.75) if vals is None else np.asarray(vals, np.float32)
    return rows, cols, (rp, ci, va)


@pytest.mark.gpu
def test_columns_up_to_two_to_the_31(pkg, gpu):
    top = 2 ** 31 - 1
    b = _csr(2, top, [[top - 1, 0, top - 1, 5], [top - 2]])
    a = _csr(1, 2, [[1, 0, 0]])
    _product(pkg.capi, a, b, "2^31 - 1 columns")
    assert G.reference("2^31 - 1 columns", a[2], b[2])[1].tolist() == [0, 5, top - 2, top - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["m = 0", "n = 0", "p = 0", "a empty", "b empty", "all zero sizes"])
def test_degenerate_sizes(pkg, gpu, case):
    full_a, full_b = _csr(3, 2, [[1, 0], [], [0]]), _csr(2, 4, [[3, 1], [1]])
    a, b = {"m = 0": (_csr(0, 2, []), full_b),
            "n = 0": (_csr(3, 0, [[], [], []]), _csr(0, 4, [])),
            "p = 0": (full_a, _csr(2, 0, [[], []])),
            "a empty": (_csr(300, 2, [[]] * 300), full_b),
            "b empty": (full_a, _csr(2, 4, [[], []])),
            "all zero sizes": (_csr(0, 0, []), _csr(0, 0, []))}[case]
    want = G.spgemm(a[2], b[2])
    assert len(want[1]) == 0 and want[0].shape == (a[0] + 1,)
    A, B = _owned(pkg.capi, a), _owned(pkg.capi, b)
    for keep in (False, True):
        c = A.spgemm(B, keep_plan=keep)
        _check(c, want, case, (a[0], b[1]))
        pkg.capi.check(pkg.capi.lib().spmv_csr_validate(c._h, 0))
        if keep:
            c.spgemm_values(A, B)
        c.close()
    A.close()
    B.close()


# ---- 6. values ---------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF,
                    0x7F7FFFFF, 0x3F800000, 0xBF800000], np.uint32).view(np.float32)


@pytest.mark.gpu
def test_special_values_and_cancellation(pkg, gpu):
    rng = np.random.default_rng(66)
    (m, n, a), (_, p, b) = G.random_matrix(rng, 70, 40, 20), G.random_matrix(rng, 40, 30, 12)
    for va in (a[2], b[2]):
        hit = rng.random(va.size) < 1 / 3
        va[hit] = rng.choice(SPECIAL, int(hit.sum()))
    # a row whose two terms cancel, a stored zero times a number, -0 times a number
    a_rp = np.concatenate([a[0], [a[0][-1] + 2, a[0][-1] + 4]]).astype(np.int32)
    a = (a_rp, np.concatenate([a[1], [0, 0, 1, 2]]).astype(np.int32), np.concatenate([a[2], [1.0, -1.0, 0.0, -0.0]]).astype(np.float32))
    b[2][b[0][0]:b[0][3]] = np.float32(3.0)
    want = G.spgemm(a, b)
    assert np.isnan(want[2]).any() and np.isinf(want[2]).any() and (want[2] == 0).any()
    A, B = _owned(pkg.capi, (m + 2, n, a)), _owned(pkg.capi, (n, p, b))
    c = A.spgemm(B)
    _check(c, want, "special values", (m + 2, p))
    if b[0][1] > b[0][0]:
        assert c.download()[0][-2] - c.download()[0][-3] > 0        # the cancelled row keeps its entries
    for h in (c, A, B):
        h.close()


# ---- 7. purity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_streams_borrowed_and_owned_give_equal_bytes(pkg, gpu):
    import torch
    a, b = G.generic_case()
    want = G.reference("generic", a[2], b[2])
    Ao, Bo = _owned(pkg.capi, a), _owned(pkg.capi, b)
    (Ab, ta), (Bb, tb) = _borrowed(pkg.capi, gpu, a), _borrowed(pkg.capi, gpu, b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    results = [Ao.spgemm(Bo, stream=s1), Ab.spgemm(Bb, stream=s2), Ao.spgemm(Bb), Ab.spgemm(Bo, keep_plan=True, stream=s1)]
    first = _check(results[0], want, "owned, stream 1")
    for i, c in enumerate(results[1:]):
        got = c.download()
        assert all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(got, first)), i
    assert results[3].spgemm_plan_bytes() == 4 * int(np.count_nonzero(_terms_per_row(a[2], b[2])))
    for h in results + [Ao, Bo, Ab, Bb]:
        h.close()


def _terms_per_row(a, b):
    blen = np.diff(b[0])[a[1]]
    return np.add.reduceat(np.concatenate([blen, [0]]), a[0][:-1]) * (np.diff(a[0]) > 0) if a[1].size else np.zeros(len(a[0]) - 1, int)


@pytest.mark.gpu
@pytest.mark.parametrize("r0,r1", [(0, 64), (64, 257), (37, 101), (100, 101), (5, 5)])
def test_a_row_block_reproduces_its_rows(pkg, gpu, r0, r1):
    (m, n, (rp, ci, va)), b = G.generic_case()
    w_rp, w_ci, w_va, _ = G.reference("generic", (rp, ci, va), b[2])
    lo, hi = int(rp[r0]), int(rp[r1])
    A = pkg.capi.CsrMatrix.from_host(r1 - r0, n, rp[r0:r1 + 1] - lo, ci[lo:hi], va[lo:hi])
    B = _owned(pkg.capi, b)
    c = A.spgemm(B)
    x, y = int(w_rp[r0]), int(w_rp[r1])
    _check(c, (w_rp[r0:r1 + 1] - x, w_ci[x:y], w_va[x:y]), f"rows {r0} .. {r1}")
    for h in (c, A, B):
        h.close()


@pytest.mark.gpu
def test_a_times_itself(pkg, gpu):
    a = G.random_matrix(np.random.default_rng(71), 150, 150, 12)
    A = _owned(pkg.capi, a)
    c = A.spgemm(A, keep_plan=True)
    _check(c, G.spgemm(a[2], a[2]), "a == b", (150, 150))
    c.spgemm_values(A, A)
    _check(c, G.spgemm(a[2], a[2])[:3], "a == b, values again")
    c.close()
    A.close()


# ---- 8. against SpMM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_values_are_the_chain_of_spmm(pkg, gpu):
    import torch
    rng = np.random.default_rng(88)
    n, p = 120, 64
    b_rows = [np.sort(rng.choice(p, int(rng.integers(0, 20)), replace=False)) for _ in range(n)]      # duplicate-free rows
    a_rows = [rng.integers(0, n, int(l)) for l in list(rng.integers(0, 40, 90)) + [512, 300, 0]]
    values = lambda r, k: (np.ldexp(1.0 + r.integers(0, 4096, k) / 4096.0, r.integers(-8, 8, k)) * r.choice([-1.0, 1.0], k)).astype(np.float32)
    a, b = G.from_rows(n, a_rows, rng, values), G.from_rows(p, b_rows, rng, values)
    A, B = _owned(pkg.capi, a), _owned(pkg.capi, b)
    c = A.spgemm(B)
    rp, ci, va = _check(c, G.spgemm(a[2], b[2]), "against SpMM")
    dense = np.zeros((n, p), np.float32)
    dense[np.repeat(np.arange(n), np.diff(b[2][0])), b[2][1]] = b[2][2]
    X, Y = _dev(gpu, dense), torch.full((a[0], p), float("nan"), dtype=torch.float32, device=gpu)
    A.spmm_plan()
    A.spmm(X, Y)
    torch.cuda.synchronize()
    gathered = Y.cpu().numpy()[np.repeat(np.arange(a[0]), np.diff(rp)), ci]
    assert np.array_equal(gathered.view(np.uint32), va.view(np.uint32))
    for h in (c, A, B):
        h.close()


# ---- 9. downstream -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_product_is_an_ordinary_handle(pkg, gpu):
    import torch
    capi = pkg.capi
    a, b = G.generic_case()
    A, B = _owned(capi, a), _owned(capi, b)
    c = A.spgemm(B)
    capi.check(capi.lib().spmv_csr_validate(c._h, 0))
    rp, ci, va = c.download()
    assert all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(c.rows))               # sorted, duplicate-free
    x = np.random.default_rng(91).standard_normal(b[1]).astype(np.float32)

    def dense(mat, absolute=False):
        rows, cols, (mrp, mci, mva) = mat
        D = np.zeros((rows, cols), np.float64)
        np.add.at(D, (np.repeat(np.arange(rows), np.diff(mrp)), mci), np.abs(mva.astype(np.float64)) if absolute else mva.astype(np.float64))
        return D
    y64 = dense(a) @ (dense(b) @ x.astype(np.float64))
    mag = dense(a, True) @ (dense(b, True) @ np.abs(x.astype(np.float64)))
    d_x, d_y = _dev(gpu, x), torch.empty(c.rows, dtype=torch.float32, device=gpu)
    for variant in (capi.SCALAR, capi.AUTO, capi.XSKIP):                # XSKIP: its plan takes sorted, duplicate-free rows
        c.plan(variant)
        d_y.fill_(float("nan"))
        c.run(variant, d_x, d_y)
        torch.cuda.synchronize()
        err = np.abs(d_y.cpu().numpy().astype(np.float64) - y64)
        assert np.all(err <= RTOL * mag + 1e-37), f"variant {variant}: {err.max()}"
    # transpose(C) has the pattern of transpose(B) transpose(A); the values agree within the sums' tolerance
    ct, At, Bt = c.transpose(), A.transpose(), B.transpose()
    d = Bt.spgemm(At)
    (t_rp, t_ci, t_va), (d_rp, d_ci, d_va) = ct.download(), d.download()
    assert np.array_equal(t_rp, d_rp) and np.array_equal(t_ci, d_ci)
    absolute = lambda m: (m[0], m[1], (m[2][0], m[2][1], np.abs(m[2][2])))
    m_va = G.spgemm(absolute(a)[2], absolute(b)[2])[2]
    mag_t = m_va[np.argsort(ci, kind="stable")].astype(np.float64)      # the transpose's storage order
    assert np.all(np.abs(t_va.astype(np.float64) - d_va.astype(np.float64)) <= RTOL * mag_t)
    for h in (d, ct, At, Bt, c, A, B):
        h.close()


# ---- 10. spgemm_values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_values_follow_in_place_rewrites_and_replay_in_a_graph(pkg, gpu):
    import torch
    capi = pkg.capi
    a, b = G.generic_case()
    (A, (_, _, d_a)), (B, (_, _, d_b)) = _borrowed(capi, gpu, a), _borrowed(capi, gpu, b)
    c = A.spgemm(B, keep_plan=True)
    want = G.reference("generic", a[2], b[2])
    _check(c, want, "keep_plan")
    assert c.spgemm_plan_bytes() > 0
    rng = np.random.default_rng(101)

    def rewrite():
        na, nb = G.spread(rng, a[2][2].size), G.spread(rng, b[2][2].size)
        d_a.copy_(_dev(gpu, na))
        d_b.copy_(_dev(gpu, nb))
        return G.spgemm((a[2][0], a[2][1], na), (b[2][0], b[2][1], nb))

    w1 = rewrite()
    c.spgemm_values(A, B)
    torch.cuda.synchronize()
    _check(c, w1[:3], "values after a rewrite")
    fresh = A.spgemm(B)
    _check(fresh, w1, "a fresh product of the rewritten values")
    fresh.close()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.spgemm_values(A, B)
    w2 = rewrite()
    g.replay()
    torch.cuda.synchronize()
    _check(c, w2[:3], "values from a replayed graph")
    # refusals: no plan, another nnz, another shape
    plain = A.spgemm(B)
    with pytest.raises(capi.SpmvError, match="spmv_csr_spgemm_values: the handle has no plan") as e:
        plain.spgemm_values(A, B)
    assert e.value.status == capi.ERR_INVALID
    rp, ci, va = a[2]
    shorter = capi.CsrMatrix.from_host(a[0], a[1], np.minimum(rp, rp[-1] - 1), ci[:-1], va[:-1])
    with pytest.raises(capi.SpmvError, match="spmv_csr_spgemm_values: a is") as e:
        c.spgemm_values(shorter, B)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.SpmvError, match="spmv_csr_spgemm_values: a is"):
        c.spgemm_values(B, A)
    with pytest.raises(capi.SpmvError, match="no map"):
        c.transpose_values(A)
    with pytest.raises(capi.SpmvError, match="no map"):
        c.select_values(A)
    _check(c, w2[:3], "values after the refusals")
    for h in (plain, shorter, c, A, B):
        h.close()


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(pkg, gpu):
    capi = pkg.capi
    lib = capi.lib()
    A, B = _owned(capi, _csr(3, 2, [[1, 0], [], [0]])), _owned(capi, _csr(3, 4, [[3, 1], [1], []]))
    out = C.c_void_p()
    assert lib.spmv_csr_spgemm(A._h, B._h, 0, None, C.byref(out), None) == capi.ERR_INVALID          # 3 x 2 times 3 x 4
    assert lib.spmv_last_error().decode().startswith("spmv_csr_spgemm: a is 3 x 2, b is 3 x 4") and out.value is None
    B2 = _owned(capi, _csr(2, 4, [[3, 1], [1]]))
    for keep in (2, -1):
        assert lib.spmv_csr_spgemm(A._h, B2._h, keep, None, C.byref(out), None) == capi.ERR_INVALID
        assert lib.spmv_last_error().decode().startswith("spmv_csr_spgemm: keep_plan") and out.value is None
    products = C.c_int64(-1)
    capi.check(lib.spmv_csr_spgemm(A._h, B2._h, 0, None, C.byref(out), C.byref(products)))
    assert products.value == 5 and out.value
    capi.check(lib.spmv_csr_destroy(out))
    for h in (A, B, B2):
        h.close()


@pytest.mark.gpu
def test_a_result_of_two_to_the_31_entries_is_refused_and_nothing_leaks(pkg, gpu):
    import torch
    capi = pkg.capi
    m, p = 1 << 16, 1 << 15
    A = capi.CsrMatrix.from_host(m, 1, np.arange(m + 1, dtype=np.int32), np.zeros(m, np.int32), np.ones(m, np.float32))
    B = capi.CsrMatrix.from_host(1, p, np.array([0, p], np.int32), np.arange(p, dtype=np.int32), np.ones(p, np.float32))
    free = []
    for _ in range(3):
        with pytest.raises(capi.SpmvError, match=r"spmv_csr_spgemm: the product has 2147483648 nonzeros") as e:
            A.spgemm(B)
        assert e.value.status == capi.ERR_INVALID
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    # one row fewer fits: 2^31 - 2^15 entries would be 16 GiB of result, so only the count is checked, through products
    out, products = C.c_void_p(), C.c_int64(-1)
    assert capi.lib().spmv_csr_spgemm(A._h, B._h, 0, None, C.byref(out), C.byref(products)) == capi.ERR_INVALID
    assert products.value == 1 << 31 and out.value is None
    A.close()
    B.close()


# ---- 12. the layer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sparse_layer_composed(pkg, gpu):
    import torch
    SL = pkg.sparse_layer
    rng = np.random.default_rng(121)
    second, first = G.random_matrix(rng, 64, 48, 10, repeats=False), G.random_matrix(rng, 48, 40, 10, repeats=False)

    def layer(mat):
        rows, cols, (rp, ci, va) = mat
        vals = _dev(gpu, va / np.float32(64)).requires_grad_(True)
        return SL.SparseLayer(rows, cols, _dev(gpu, rp), _dev(gpu, ci), vals)

    L2, L1 = layer(second), layer(first)
    both = L2.composed(L1)
    assert (both.A.rows, both.A.cols) == (64, 40) and both.vals.is_leaf and both.vals.requires_grad and both.k_max is None
    X = _dev(gpu, rng.standard_normal((40, 8)).astype(np.float32))
    Y = both(X)
    with torch.no_grad():
        Y2 = L2(L1(X))
    torch.cuda.synchronize()

    def dense(mat):
        rows, cols, (rp, ci, va) = mat
        D = np.zeros((rows, cols), np.float64)
        np.add.at(D, (np.repeat(np.arange(rows), np.diff(rp)), ci), va.astype(np.float64) / 64)
        return D
    mag = np.abs(dense(second)) @ (np.abs(dense(first)) @ np.abs(X.cpu().numpy().astype(np.float64)))
    err = np.abs(Y.detach().cpu().numpy().astype(np.float64) - Y2.cpu().numpy().astype(np.float64))
    assert np.all(err <= RTOL * mag + 1e-37), err.max()
    Y.sum().backward()
    torch.cuda.synchronize()
    assert both.vals.grad is not None and both.vals.grad.shape == both.vals.shape and bool(torch.isfinite(both.vals.grad).all())
    assert L1.vals.grad is None and L2.vals.grad is None            # no gradient flows to the parents
    for l in (both, L2, L1):
        l.close()


# ---- 13. the tester executable ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tester_executable_multiplies_two_files(pkg, gpu, tmp_path):
    import subprocess
    rng = np.random.default_rng(131)
    mats = {}
    for name, (rows, cols) in (("A", (40, 30)), ("B", (30, 50))):
        D = np.where(rng.random((rows, cols)) < 0.15, G.spread(rng, rows * cols).reshape(rows, cols), np.float32(0))
        r, c = np.nonzero(D)
        lines = [f"{i + 1} {j + 1} {float(D[i, j])!r}" for i, j in zip(r, c)]
        (tmp_path / f"{name}.mtx").write_text("%%MatrixMarket matrix coordinate real general\n" + f"{rows} {cols} {len(r)}\n" + "\n".join(lines) + "\n")
        mats[name] = (np.concatenate([[0], np.cumsum(np.count_nonzero(D, axis=1))]).astype(np.int32), c.astype(np.int32), D[r, c].astype(np.float32))
    out = tmp_path / "C.mtx"
    run = subprocess.run([str(pkg.capi.TESTER_PATH), "--mtx", str(tmp_path / "A.mtx"), "--spgemm", str(tmp_path / "B.mtx"), "--out", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "========== OK ===========" in run.stdout, run.stdout + run.stderr
    rp, ci, va, products = G.spgemm(mats["A"], mats["B"])
    assert f"nnz {len(ci)} from {products} products" in run.stdout
    body = out.read_text().splitlines()
    assert body[0].startswith("%%MatrixMarket matrix coordinate real general") and body[1].split() == ["40", "50", str(len(ci))]
    got = np.array([l.split() for l in body[2:]], dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(got[:, 0] - 1, np.repeat(np.arange(40), np.diff(rp))) and np.array_equal(got[:, 1] - 1, ci)
    assert np.array_equal(got[:, 2].astype(np.float32).view(np.uint32), va.view(np.uint32))      # %.9g round-trips a float
