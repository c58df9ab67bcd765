"""GPU (-m gpu): spmv_csr_add / _add_values / _add_gather / _add_plan_bytes (include/spmv_hip.h "the sparse sum").

The expectation is always tests/_add.py (numpy), never a kernel of this library, and every result is compared bit for bit:
row_ptr, col_idx and the uint32 view of vals (a NaN matches any NaN: its sign and payload are the hardware's).  That the
generic inputs tell the contract's order from two wrong ones is proved in tests/test_add_host.py.

  1 generic        two 257 x 193 matrices, unsorted rows of 0 .. 40 with repeats (the row-sorted view), three ops, 1/3 and 3
  2 sorted         sorted duplicate-free operands (the operands' own arrays), three ops; sorted with repeated columns
  3 row lengths    0, 1, 2, 63, 64, 65, 129 against 0, 1, 64 and a row of 5000; identical, disjoint, interleaved, below / above
  4 type edges     columns up to 2^31 - 2; m = 0, n = 0, nnz = 0 on either side or both, an empty intersection
  5 values         +-Inf, NaN, -0, subnormals, stored zeros, a cancelling pair; +-0 coefficients against NaNs; copy; A + A
  6 purity         two streams, borrowed against owned operands, row blocks, a == b
  7 downstream     validate, SPMV_SCALAR / SPMV_AUTO on C, the transpose of C
  8 companions     _values after rewrites and from a graph, _gather with strides and poison, refusals, plan bytes
  9 refusals       shapes, op, keep_plan, foreign handles (and no memory left behind)
 10 wrappers       union_pattern / mask_pattern, SparseLayer.grown / summed, sparse_sgemv --add
"""
import ctypes as C

import numpy as np
import pytest

import _add as G
from _util import RTOL

MIB = 1 << 20
f32 = np.float32
THIRD = f32(1) / f32(3)
OPS = G.OPS


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
    bad = G.same(got, want[:3])
    assert bad is None, f"{what}: {bad}"
    assert c.nnz == len(want[1])
    if shape is not None:
        assert (c.rows, c.cols) == shape, what
    return got


def _sum(capi, a, b, alpha, beta, op, key, keep_plan=False):
    """alpha a + beta b through owned handles against the contract (computed once per key)."""
    A, B = _owned(capi, a), _owned(capi, b)
    try:
        c = A.add(B, alpha, beta, op, keep_plan=keep_plan)
        try:
            want = G.reference(key, a[2], b[2], alpha, beta, op, cols=a[1])
            _check(c, want, f"{key} {op}", (a[0], a[1]))
            assert c.transpose_map_bytes() == 0 and c.select_map_bytes() == 0 and c.spgemm_plan_bytes() == 0
            assert c.add_plan_bytes() == (4 * want[3] + 4 * (c.nnz + 1) if keep_plan else 0)
        finally:
            c.close()
    finally:
        A.close()
        B.close()


# ---- 1 .. 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_generic_unsorted_operands(pkg, gpu, op):
    a, b = G.generic_case()
    _sum(pkg.capi, a, b, THIRD, 3.0, op, "generic", keep_plan=(op == "union"))


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("repeats", [False, True])
def test_sorted_operands(pkg, gpu, op, repeats):
    a, b = G.sorted_case(repeats)
    _sum(pkg.capi, a, b, THIRD, 3.0, op, ("sorted", repeats), keep_plan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_one_operand_unsorted(pkg, gpu, op):
    a, b = G.generic_case()[0], G.sorted_matrix(np.random.default_rng(2710), 257, 193, 40)
    _sum(pkg.capi, a, b, THIRD, 3.0, op, "unsorted a, sorted b")
    _sum(pkg.capi, b, a, THIRD, 3.0, op, "sorted a, unsorted b")


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_row_lengths(pkg, gpu, op):
    a, b = G.lengths_case()
    _sum(pkg.capi, a, b, THIRD, 3.0, op, "lengths", keep_plan=True)


# ---- 4. the edges of the types ---------------------------------------------------------------------------------------------------
def _csr(rows, cols, lists, vals=None):
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    ci = np.array([c for l in lists for c in l], np.int32)
    va = np.arange(1, ci.size + 1, dtype=np.float32) * np.float32(0.75) if vals is None else np.asarray(vals, np.float32)
    return rows, cols, (rp, ci, va)


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_columns_up_to_two_to_the_31(pkg, gpu, op):
    top = 2 ** 31 - 1
    a = _csr(2, top, [[top - 1, 0, top - 1, 5], [top - 2]])
    b = _csr(2, top, [[5, top - 1], [top - 1, top - 2, top - 2]])
    _sum(pkg.capi, a, b, THIRD, 3.0, op, "2^31 - 1 columns", keep_plan=True)
    want = G.reference("2^31 - 1 columns", a[2], b[2], THIRD, 3.0, op, cols=top)
    assert want[1].tolist() == {"union": [0, 5, top - 1, top - 2, top - 1], "intersect": [5, top - 1, top - 2], "minus": [0]}[op]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["m = 0", "n = 0", "a empty", "b empty", "both empty", "disjoint"])
def test_degenerate_sizes(pkg, gpu, case):
    full = _csr(3, 4, [[3, 1], [], [0]])
    a, b = {"m = 0": (_csr(0, 4, []), _csr(0, 4, [])),
            "n = 0": (_csr(3, 0, [[], [], []]), _csr(3, 0, [[], [], []])),
            "a empty": (_csr(3, 4, [[], [], []]), full),
            "b empty": (full, _csr(3, 4, [[], [], []])),
            "both empty": (_csr(300, 4, [[]] * 300), _csr(300, 4, [[]] * 300)),
            "disjoint": (full, _csr(3, 4, [[0, 2], [1], [3]]))}[case]
    A, B = _owned(pkg.capi, a), _owned(pkg.capi, b)
    for op in OPS:
        want = G.add(a[2], b[2], THIRD, 3.0, op, cols=a[1])
        if case in ("m = 0", "n = 0", "both empty") or (case, op) in (("a empty", "intersect"), ("a empty", "minus"),
                                                                       ("b empty", "intersect"), ("disjoint", "intersect")):
            assert len(want[1]) == 0
        for keep in (False, True):
            c = A.add(B, THIRD, 3.0, op, keep_plan=keep)
            _check(c, want, f"{case} {op}", (a[0], a[1]))
            pkg.capi.check(pkg.capi.lib().spmv_csr_validate(c._h, 0))
            if keep:
                c.add_values(A, B, 1.0, 1.0)
                assert c.add_plan_bytes() == 4 * want[3] + 4 * (c.nnz + 1)
            c.close()
    A.close()
    B.close()


# ---- 5. values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_special_values_and_cancellation(pkg, gpu, op):
    a, b = G.special_case()
    want = G.reference("special", a[2], b[2], 1.0, 1.0, op, cols=a[1])
    if op == "union":
        assert np.isnan(want[2]).any() and np.isinf(want[2]).any() and (want[2] == 0).any()
        last = slice(want[0][-2], want[0][-1])
        assert want[1][last].tolist() == [5, 7] and want[2][last].view(np.uint32).tolist() == [0, f32(2.0).view(np.uint32)]      # cancelled: stays, +0
    _sum(pkg.capi, a, b, 1.0, 1.0, op, "special")
    _sum(pkg.capi, a, b, THIRD, -3.0, op, "special")


@pytest.mark.gpu
@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_a_zero_coefficient_reads_no_value_of_its_side(pkg, gpu, zero):
    (m, n, a), (_, _, b) = G.order_case()
    nan_b = (b[0], b[1], np.full(b[2].size, np.nan, f32))
    for op, alpha, beta, x, y in (("intersect", 1.0, zero, a, nan_b), ("union", 1.0, zero, a, nan_b), ("union", zero, 3.0, nan_b, a),
                                  ("intersect", zero, zero, nan_b, nan_b)):
        want = G.add(x, y, alpha, beta, op, cols=n)
        assert not np.isnan(want[2]).any()
        X, Y = _owned(pkg.capi, (m, n, x)), _owned(pkg.capi, (m, n, y))
        c = X.add(Y, alpha, beta, op)
        _check(c, want, f"{op} {alpha} {beta}", (m, n))
        for h in (c, X, Y):
            h.close()
    # a NaN or infinite coefficient follows IEEE rules
    for alpha, beta in ((float("nan"), 1.0), (float("inf"), -2.0)):
        A, B = _owned(pkg.capi, (m, n, a)), _owned(pkg.capi, (m, n, b))
        c = A.add(B, alpha, beta)
        _check(c, G.add(a, b, alpha, beta, "union", cols=n), f"coefficients {alpha} {beta}")
        for h in (c, A, B):
            h.close()


@pytest.mark.gpu
def test_the_copy_case_and_a_plus_a(pkg, gpu):
    capi = pkg.capi
    rng = np.random.default_rng(53)
    mat = G.from_rows(50, [rng.choice(50, int(rng.integers(0, 13)), replace=False) for _ in range(60)], rng)      # unsorted, no repeats
    mat[2][2][::5] = G.SPECIAL[np.arange(mat[2][2][::5].size) % G.SPECIAL.size]
    empty = _csr(60, 50, [[]] * 60)
    A, E = _owned(capi, mat), _owned(capi, empty)
    for x in (1.0, 0.0, float("nan")):
        c = A.add(E, 1.0, x)
        got = c.download()
        want = G.sort_rows(mat[2])
        assert G.same(got, want) is None
        keep = ~np.isnan(want[2])
        assert np.array_equal(got[2][keep].view(np.uint32), want[2][keep].view(np.uint32))      # -0, subnormals, Inf: the bits
        c.close()
    srt = G.sorted_case(False)[0]
    S = _owned(capi, srt)
    E2 = _owned(capi, _csr(srt[0], srt[1], [[]] * srt[0]))
    c = S.add(E2)
    assert all(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)) for g, w in zip(c.download(), srt[2]))      # A itself
    c.close()
    c = S.add(S)
    rp, ci, va = c.download()
    assert np.array_equal(rp, srt[2][0]) and np.array_equal(ci, srt[2][1]) and np.array_equal(va, f32(2) * srt[2][2])          # A + A = 2 A
    for h in (c, S, A, E, E2):
        h.close()


# ---- 6. purity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_streams_borrowed_and_owned_give_equal_bytes(pkg, gpu):
    import torch
    a, b = G.generic_case()
    want = G.reference("generic", a[2], b[2], THIRD, 3.0, "union", cols=a[1])
    Ao, Bo = _owned(pkg.capi, a), _owned(pkg.capi, b)
    (Ab, ta), (Bb, tb) = _borrowed(pkg.capi, gpu, a), _borrowed(pkg.capi, gpu, b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    results = [Ao.add(Bo, THIRD, 3.0, stream=s1), Ab.add(Bb, THIRD, 3.0, stream=s2), Ao.add(Bb, THIRD, 3.0),
               Ab.add(Bo, THIRD, 3.0, keep_plan=True, stream=s1)]
    first = _check(results[0], want, "owned, stream 1")
    for i, c in enumerate(results[1:]):
        got = c.download()
        assert all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(got, first)), i
    for h in results + [Ao, Bo, Ab, Bb]:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r0,r1", [(0, 64), (64, 257), (37, 101), (100, 101), (5, 5)])
def test_a_row_block_reproduces_its_rows(pkg, gpu, r0, r1):
    (m, n, a), (_, _, b) = G.generic_case()
    w_rp, w_ci, w_va, _ = G.reference("generic", a, b, THIRD, 3.0, "union", cols=n)

    def block(mat):
        rp, ci, va = mat
        lo, hi = int(rp[r0]), int(rp[r1])
        return pkg.capi.CsrMatrix.from_host(r1 - r0, n, rp[r0:r1 + 1] - lo, ci[lo:hi], va[lo:hi])
    A, B = block(a), block(b)
    c = A.add(B, THIRD, 3.0)
    x, y = int(w_rp[r0]), int(w_rp[r1])
    _check(c, (w_rp[r0:r1 + 1] - x, w_ci[x:y], w_va[x:y]), f"rows {r0} .. {r1}")
    for h in (c, A, B):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_a_with_itself(pkg, gpu, op):
    a, _ = G.generic_case()
    A = _owned(pkg.capi, a)
    c = A.add(A, THIRD, 3.0, op, keep_plan=True)
    want = G.add(a[2], a[2], THIRD, 3.0, op, cols=a[1])
    _check(c, want, f"a == b {op}", (a[0], a[1]))
    c.add_values(A, A, THIRD, 3.0)
    _check(c, want, f"a == b {op}, values again")
    assert (c.nnz == 0) == (op == "minus")
    c.close()
    A.close()


# ---- 7. downstream -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_sum_is_an_ordinary_handle(pkg, gpu):
    import torch
    capi = pkg.capi
    a, b = G.generic_case()
    A, B = _owned(capi, a), _owned(capi, b)
    c = A.add(B, THIRD, 3.0)
    capi.check(capi.lib().spmv_csr_validate(c._h, 0))
    rp, ci, va = c.download()
    assert all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(c.rows))               # sorted, duplicate-free
    x = np.random.default_rng(91).standard_normal(a[1]).astype(np.float32)
    _, val, mag = G.dense_walk(a[0], a[1], a[2], b[2], THIRD, 3.0, "union")
    y64, ymag = val @ x.astype(np.float64), mag @ np.abs(x.astype(np.float64))
    d_x, d_y = _dev(gpu, x), torch.empty(c.rows, dtype=torch.float32, device=gpu)
    for variant in (capi.SCALAR, capi.AUTO):
        c.plan(variant)
        d_y.fill_(float("nan"))
        c.run(variant, d_x, d_y)
        torch.cuda.synchronize()
        err = np.abs(d_y.cpu().numpy().astype(np.float64) - y64)
        assert np.all(err <= 2 * RTOL * ymag + 1e-37), f"variant {variant}: {err.max()}"       # the sum's rounding and the product's
    # transpose(C): the same entries, column-major
    ct = c.transpose()
    t_rp, t_ci, t_va = ct.download()
    order = np.argsort(ci, kind="stable")
    assert np.array_equal(t_ci, np.repeat(np.arange(c.rows), np.diff(rp))[order]) and np.array_equal(t_va.view(np.uint32), va[order].view(np.uint32))
    assert np.array_equal(t_rp, np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=c.cols))]))
    for h in (ct, c, A, B):
        h.close()


# ---- 8. the companions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_values_follow_in_place_rewrites_and_replay_in_a_graph(pkg, gpu):
    import torch
    capi = pkg.capi
    a, b = G.generic_case()
    n = a[1]
    (A, (_, _, d_a)), (B, (_, _, d_b)) = _borrowed(capi, gpu, a), _borrowed(capi, gpu, b)
    c = A.add(B, THIRD, 3.0, keep_plan=True)
    want = G.reference("generic", a[2], b[2], THIRD, 3.0, "union", cols=n)
    _check(c, want, "keep_plan")
    assert c.add_plan_bytes() == 4 * want[3] + 4 * (c.nnz + 1) and want[3] == a[2][1].size + b[2][1].size
    rng = np.random.default_rng(101)

    def rewrite(alpha, beta):
        na, nb = G.spread(rng, a[2][2].size), G.spread(rng, b[2][2].size)
        d_a.copy_(_dev(gpu, na))
        d_b.copy_(_dev(gpu, nb))
        return G.add((a[2][0], a[2][1], na), (b[2][0], b[2][1], nb), alpha, beta, "union", cols=n)

    for alpha, beta in ((f32(-2.5), THIRD), (f32(0.0), f32(7.0)), (THIRD, f32(-0.0))):
        w1 = rewrite(alpha, beta)
        c.add_values(A, B, alpha, beta)
        torch.cuda.synchronize()
        _check(c, w1, f"values after a rewrite, {alpha} {beta}")
    fresh = A.add(B, THIRD, -0.0)
    _check(fresh, w1, "a fresh sum of the rewritten values")
    fresh.close()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.add_values(A, B, 1.5, THIRD)
    w2 = rewrite(1.5, THIRD)
    g.replay()
    torch.cuda.synchronize()
    _check(c, w2, "values from a replayed graph")
    # refusals: no plan, another nnz, another shape, the other companions
    plain = A.add(B)
    with pytest.raises(capi.SpmvError, match="spmv_csr_add_values: the handle has no plan") as e:
        plain.add_values(A, B)
    assert e.value.status == capi.ERR_INVALID
    plain.add_parent_nnz = (A.nnz, B.nnz)
    with pytest.raises(capi.SpmvError, match="spmv_csr_add_gather: the handle has no plan"):
        plain.add_gather(0, torch.zeros(plain.nnz, device=gpu), torch.zeros(A.nnz, device=gpu))
    rp, ci, va = a[2]
    shorter = capi.CsrMatrix.from_host(a[0], a[1], np.minimum(rp, rp[-1] - 1), ci[:-1], va[:-1])
    with pytest.raises(capi.SpmvError, match="spmv_csr_add_values: a is") as e:
        c.add_values(shorter, B)
    assert e.value.status == capi.ERR_INVALID
    wide = _owned(capi, _csr(a[0], a[1] + 1, [[]] * a[0]))
    with pytest.raises(capi.SpmvError, match="spmv_csr_add_values: a is"):
        c.add_values(A, wide)
    for call in (lambda: c.transpose_values(A), lambda: c.select_values(A)):
        with pytest.raises(capi.SpmvError, match="no map"):
            call()
    with pytest.raises(capi.SpmvError, match="spmv_csr_spgemm_values: the handle has no plan"):
        c.spgemm_values(A, B)
    t = A.transpose(keep_map=True)
    with pytest.raises(capi.SpmvError, match="spmv_csr_add_values: the handle has no plan"):
        t.add_values(A, B)
    _check(c, w2, "values after the refusals")
    for h in (t, wide, plain, shorter, c, A, B):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_gather_reaches_the_operands_and_leaves_the_rest(pkg, gpu, op):
    import torch
    capi = pkg.capi
    a, b = G.generic_case()
    A, B = _owned(capi, a), _owned(capi, b)
    c = A.add(B, THIRD, 3.0, op, keep_plan=True)
    rng = np.random.default_rng(111)
    POISON = np.uint32(0xDEADBEEF)
    # the plan in numpy: the entry of every kept term of a side
    n = a[1]
    w_rp, w_ci, _, terms = G.add(a[2], b[2], THIRD, 3.0, op, cols=n)
    key_c = np.repeat(np.arange(a[0], dtype=np.int64), np.diff(w_rp)) * n + w_ci
    seen = 0
    for side, mat in ((0, a[2]), (1, b[2])):
        key = np.repeat(np.arange(a[0], dtype=np.int64), np.diff(mat[0])) * n + mat[1]
        e = np.searchsorted(key_c, key)
        hit = (e < key_c.size) & (key_c[np.minimum(e, max(key_c.size - 1, 0))] == key) if key_c.size else np.zeros(key.size, bool)
        if side == 1 and op == "minus":
            hit[:] = False                                          # under MINUS b has no terms
        seen += int(hit.sum())
        for count, src_stride, dst_stride in ((1, c.nnz, mat[1].size), (3, c.nnz + 5, mat[1].size + 3)):
            src = rng.integers(0, 2 ** 32, (count, src_stride), dtype=np.uint32)
            d_src = _dev(gpu, src.view(np.int32))[:, :c.nnz]
            d_dst = torch.full((count, dst_stride), int(POISON.view(np.int32)), dtype=torch.int32, device=gpu)
            view = d_dst[:, :mat[1].size]
            if count == 1:
                c.add_gather(side, d_src[0], view[0])
            else:
                c.add_gather(side, d_src, view)
            torch.cuda.synchronize()
            want = np.full((count, dst_stride), POISON, np.uint32)
            want[:, np.flatnonzero(hit)] = src[:, e[hit]]
            assert np.array_equal(d_dst.cpu().numpy().view(np.uint32), want), f"side {side} count {count}"
    assert seen == terms and c.add_plan_bytes() == 4 * terms + 4 * (c.nnz + 1)
    # refusals, as spmv_csr_select_scatter's
    lib = capi.lib()
    buf = torch.zeros(4 * (A.nnz + B.nnz + c.nnz) + 8, dtype=torch.int32, device=gpu)
    p = buf.data_ptr()
    for args, msg in (((2, 1, p, 0, p, 0), "side = 2"), ((0, 0, p, 0, p, 0), "count = 0"), ((0, 1, None, 0, p, 0), "null array"),
                      ((0, 1, p + 2, 0, p, 0), "4-byte aligned"), ((0, 1, p, -1, p, 0), "not negative"),
                      ((0, 2, p, c.nnz, p, A.nnz - 1), "dst_stride")):
        if c.nnz == 0 and msg == "null array":
            continue
        assert lib.spmv_csr_add_gather(c._h, *args, None) == capi.ERR_INVALID, msg
        err = lib.spmv_last_error().decode()
        assert err.startswith("spmv_csr_add_gather:") and msg in err, err
    for h in (c, A, B):
        h.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_nothing_behind(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    a, b = G.generic_case()
    A, B = _owned(capi, a), _owned(capi, b)
    W = _owned(capi, _csr(a[0], a[1] + 7, [[]] * a[0]))
    Hh = _owned(capi, _csr(a[0] - 1, a[1], [[]] * (a[0] - 1)))
    out = C.c_void_p()
    free = []
    for _ in range(3):
        assert lib.spmv_csr_add(A._h, W._h, 1.0, 1.0, 0, 0, None, C.byref(out)) == capi.ERR_INVALID
        assert lib.spmv_last_error().decode().startswith("spmv_csr_add: a is 257 x 193, b is 257 x 200") and out.value is None
        assert lib.spmv_csr_add(A._h, Hh._h, 1.0, 1.0, 0, 0, None, C.byref(out)) == capi.ERR_INVALID
        assert lib.spmv_last_error().decode().startswith("spmv_csr_add: a is 257 x 193, b is 256 x 193") and out.value is None
        for op in (3, -1):
            assert lib.spmv_csr_add(A._h, B._h, 1.0, 1.0, op, 0, None, C.byref(out)) == capi.ERR_INVALID
            assert lib.spmv_last_error().decode().startswith(f"spmv_csr_add: op = {op}") and out.value is None
        for keep in (2, -1):
            assert lib.spmv_csr_add(A._h, B._h, 1.0, 1.0, 0, keep, None, C.byref(out)) == capi.ERR_INVALID
            assert lib.spmv_last_error().decode().startswith("spmv_csr_add: keep_plan") and out.value is None
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    # good calls in a row leave nothing behind either (the views, the ranks and the plan are freed)
    free = []
    for _ in range(3):
        capi.check(lib.spmv_csr_add(A._h, B._h, 1.0, 1.0, 0, 0, None, C.byref(out)))
        assert out.value
        capi.check(lib.spmv_csr_destroy(out))
        out = C.c_void_p()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    # foreign handles to the companions
    s = A.select_topk(2, keep_map=True)
    At = A.transpose()
    p = A.spgemm(At, keep_plan=True)
    for h in (s, p, A):
        with pytest.raises(capi.SpmvError, match="spmv_csr_add_values: the handle has no plan"):
            h.add_values(A, B)
        assert h.add_plan_bytes() == 0
    for h in (s, p, At, W, Hh, A, B):
        h.close()


# ---- 10. the wrappers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_union_and_mask_patterns_feed_fused_attention(pkg, gpu):
    import torch
    capi, SA = pkg.capi, pkg.sparse_attention
    rng = np.random.default_rng(121)
    q, k, w = 96, 80, 16
    band = G.from_rows(k, [np.arange(max(0, i * k // q - 3), min(k, i * k // q + 4)) for i in range(q)], rng)
    glob = G.from_rows(k, [rng.permutation(np.array([0, 1, k - 1])) for _ in range(q)], rng)              # unsorted rows
    causal = G.from_rows(k, [np.arange(0, min(k, i * k // q + 1)) for i in range(q)], rng)
    Bh, Gh, Ch = (_owned(capi, m) for m in (band, glob, causal))
    u_rp, u_ci = SA.union_pattern(Bh, Gh)
    U = capi.CsrMatrix.from_device(q, k, u_rp, u_ci, torch.zeros(u_ci.numel(), device=gpu))
    m_rp, m_ci = SA.mask_pattern(U, Ch)
    w_u = G.add(band[2], glob[2], 0.0, 0.0, "union", cols=k)
    w_m = G.add((w_u[0], w_u[1], w_u[2]), causal[2], 0.0, 0.0, "intersect", cols=k)
    assert np.array_equal(u_rp.cpu().numpy(), w_u[0]) and np.array_equal(u_ci.cpu().numpy(), w_u[1])
    assert np.array_equal(m_rp.cpu().numpy(), w_m[0]) and np.array_equal(m_ci.cpu().numpy(), w_m[1])
    assert m_rp.dtype == torch.int32 and m_ci.dtype == torch.int32 and m_ci.numel() < u_ci.numel()
    Q, K, V = (_dev(gpu, rng.standard_normal(s).astype(np.float32)) for s in ((q, w), (k, w), (k, w)))
    outs = []
    for rp, ci in ((m_rp, m_ci), (_dev(gpu, w_m[0]), _dev(gpu, w_m[1]))):                # the device-built and the host-built pattern
        att = SA.FusedSparseAttention(q, k, rp, ci)
        outs.append(att(Q, K, V).detach().cpu().numpy())
        att.close()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    for h in (U, Bh, Gh, Ch):
        h.close()


@pytest.mark.gpu
def test_sparse_layer_grown_and_summed(pkg, gpu):
    import torch
    SL = pkg.sparse_layer
    rng = np.random.default_rng(131)
    old = G.sorted_matrix(rng, 64, 48, 10)
    extra = G.random_matrix(rng, 64, 48, 6)

    def layer(mat):
        rows, cols, (rp, ci, va) = mat
        vals = _dev(gpu, va / np.float32(64)).requires_grad_(True)
        return SL.SparseLayer(rows, cols, _dev(gpu, rp), _dev(gpu, ci), vals)

    L = layer(old)
    grown = L.grown(_dev(gpu, extra[2][0]), _dev(gpu, extra[2][1]))
    want = G.add((old[2][0], old[2][1], old[2][2] / f32(64)), extra[2], 1.0, 0.0, "union", cols=48)
    assert grown.A.nnz == want[1].size > L.A.nnz and grown.vals.is_leaf and grown.vals.requires_grad
    assert G.same(grown.A.download(), want[:3]) is None and grown.growth.add_plan_bytes() == 4 * want[3] + 4 * (grown.A.nnz + 1)
    X = _dev(gpu, rng.standard_normal((48, 8)).astype(np.float32))
    Y = grown(X)
    with torch.no_grad():
        Y0 = L(X)
    torch.cuda.synchronize()
    assert np.array_equal(Y.detach().cpu().numpy().view(np.uint32), Y0.cpu().numpy().view(np.uint32))      # +0 terms change no bit
    Y.sum().backward()
    torch.cuda.synchronize()
    assert grown.vals.grad is not None and grown.vals.grad.shape == (grown.A.nnz,) and L.vals.grad is None
    # optimizer state follows: the gradient on the grown pattern back at the old positions
    back = torch.full((L.A.nnz,), float("nan"), device=gpu)
    grown.growth.add_gather(0, grown.vals.grad, back)
    torch.cuda.synchronize()
    old_pos = np.searchsorted(np.repeat(np.arange(64), np.diff(want[0])) * 48 + want[1], np.repeat(np.arange(64), np.diff(old[2][0])) * 48 + old[2][1])
    assert np.array_equal(back.cpu().numpy(), grown.vals.grad.cpu().numpy()[old_pos])
    # summed: within RTOL of the two parents' outputs added
    other = layer(extra)
    both = L.summed(other, 0.5, -2.0)
    assert both.vals.is_leaf and both.vals.requires_grad and both.k_max is None
    with torch.no_grad():
        Yb, Y1, Y2 = both(X), L(X), other(X)
    torch.cuda.synchronize()

    def dense(mat):
        rows, cols, (rp, ci, va) = mat
        D = np.zeros((rows, cols), np.float64)
        np.add.at(D, (np.repeat(np.arange(rows), np.diff(rp)), ci), va.astype(np.float64) / 64)
        return D
    x64 = np.abs(X.cpu().numpy().astype(np.float64))
    mag = 0.5 * np.abs(dense(old)) @ x64 + 2.0 * (np.abs(dense(extra)) @ x64)
    err = np.abs(Yb.cpu().numpy().astype(np.float64) - (0.5 * Y1.cpu().numpy().astype(np.float64) - 2.0 * Y2.cpu().numpy().astype(np.float64)))
    assert np.all(err <= RTOL * mag + 1e-37), err.max()
    assert L.vals.grad is None and other.vals.grad is None
    for l in (both, other, grown, L):
        l.close()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_tester_executable_adds_two_files(pkg, gpu, tmp_path, op):
    import subprocess
    rng = np.random.default_rng(141)
    mats = {}
    for name in ("A", "B"):
        D = np.where(rng.random((40, 30)) < 0.2, G.spread(rng, 1200).reshape(40, 30), np.float32(0))
        r, c = np.nonzero(D)
        lines = [f"{i + 1} {j + 1} {float(D[i, j])!r}" for i, j in zip(r, c)]
        (tmp_path / f"{name}.mtx").write_text("%%MatrixMarket matrix coordinate real general\n" + f"40 30 {len(r)}\n" + "\n".join(lines) + "\n")
        mats[name] = (np.concatenate([[0], np.cumsum(np.count_nonzero(D, axis=1))]).astype(np.int32), c.astype(np.int32), D[r, c].astype(np.float32))
    out = tmp_path / "C.mtx"
    run = subprocess.run([str(pkg.capi.TESTER_PATH), "--mtx", str(tmp_path / "A.mtx"), "--add", str(tmp_path / "B.mtx"), "--alpha", "0.25",
                          "--beta", "-3", "--op", op, "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "========== OK ===========" in run.stdout, run.stdout + run.stderr
    rp, ci, va, _ = G.add(mats["A"], mats["B"], 0.25, -3.0, op, cols=30)
    assert f"spmv_csr_add: 40 x 30, nnz {len(ci)}" in run.stdout
    body = out.read_text().splitlines()
    assert body[0].startswith("%%MatrixMarket matrix coordinate real general") and body[1].split() == ["40", "30", str(len(ci))]
    got = np.array([l.split() for l in body[2:]], dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(got[:, 0] - 1, np.repeat(np.arange(40), np.diff(rp))) and np.array_equal(got[:, 1] - 1, ci)
    assert np.array_equal(got[:, 2].astype(np.float32).view(np.uint32), va.view(np.uint32))      # %.9g round-trips a float
