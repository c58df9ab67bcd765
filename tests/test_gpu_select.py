"""GPU (-m gpu): spmv_csr_select_topk / spmv_csr_select_threshold and their companions (include/spmv_hip.h "selection").

The expectation is always tests/_select.py (numpy), never a kernel of this library, and every comparison is bit for bit:
row_ptr, col_idx, the uint32 view of vals, and the map (read through select_gather of the positions 0 .. nnz - 1).

  1 row lengths   0 .. 4097 mixed inside wavefronts and sorted by length, k from 1 to 2^31 - 1, plain and shuffled rows
  2 ties          all equal, two values, blocks of 64 and of 65, k at len / 2 and len - 1
  3 keys          lowest mantissa bit, sign, the special set, rows of only NaNs, fewer numbers than k; abs; score = None
  4 threshold     the same matrices, -Inf, -0, +0, a present value, +Inf, FLT_MAX; abs; a result without nonzeros
  5 copy, purity  k >= longest row; two calls and a side stream; row blocks alone; owning and borrowing parents; the result
                  validates and multiplies
  6 companions    select_values, gather / scatter, all in a graph, copy_arrays, every refusal, the two kinds of map
  7 at size       65 536 power-law rows, band and uniform, k = 4, 16
  8 memory        four rounds leave free device memory where it was
  9 the layers    topk_pattern + FusedSparseAttention against dense masked attention; SparseLayer.pruned
 10 checked       one case of 1 and one of 2 through libspmv_hip_checked.so, in a child process
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _select as S
from _util import RTOL, assert_close_to_oracle, synth_problem

ROOT = Path(__file__).resolve().parent.parent
MIB = 1 << 20
EDGE = [0, 1, 2, 63, 64, 65, 127, 128, 511, 512, 513, 1024, 1025, 4097]
KS = [1, 2, 63, 64, 65, 512, 513, 4097, 2 ** 31 - 1]
COLS = 6000


# ---- the matrices (host arrays; built once per process and left unchanged) --------------------------------------------------
_cache = {}


def lengths_matrix(order, form):
    """Rows of the EDGE lengths (twice) among short rows, 300 rows in all: `mixed` so that wavefronts hold unlike rows,
    `sorted` so that they do not.  form: plain (sorted distinct columns) | shuffled (unsorted, ~1/8 duplicate columns)."""
    key = ("lengths", order, form)
    if key not in _cache:
        rng = np.random.default_rng(7)
        lengths = np.concatenate([EDGE, EDGE, rng.integers(0, 48, 300 - 2 * len(EDGE))])
        lengths = np.sort(lengths) if order == "sorted" else rng.permutation(lengths)
        rp, ci = S.random_csr(np.random.default_rng(8), len(lengths), COLS, lengths, sorted_rows=form == "plain")
        va = np.random.default_rng(9).standard_normal(int(rp[-1])).astype(np.float32)
        _cache[key] = (len(lengths), COLS, rp, ci, va)
    return _cache[key]


TIE_ROWS = [64, 65, 512, 513, 4097]


def ties_matrix():
    if "ties" not in _cache:
        rp, ci = S.random_csr(np.random.default_rng(10), len(TIE_ROWS), COLS, TIE_ROWS)
        nnz = int(rp[-1])
        va = np.random.default_rng(11).standard_normal(nnz).astype(np.float32)
        within = np.arange(nnz) - np.repeat(rp[:-1], np.diff(rp))
        rng = np.random.default_rng(12)
        scores = {"all_equal": np.full(nnz, 1.5, np.float32),
                  "two_values": rng.choice(np.array([1.0, -2.0], np.float32), nnz),
                  "blocks_of_64": ((within // 64) % 3).astype(np.float32),
                  "blocks_of_65": ((within // 65) % 3).astype(np.float32)}
        _cache["ties"] = (len(TIE_ROWS), COLS, rp, ci, va, scores)
    return _cache["ties"]


def keys_matrix():
    if "keys" not in _cache:
        lengths = [12, 40, 64, 100, 513, 700, 5, 2000, 0, 3]
        rp, ci = S.random_csr(np.random.default_rng(13), len(lengths), COLS, lengths, sorted_rows=False)
        nnz = int(rp[-1])
        rng = np.random.default_rng(14)
        va = rng.standard_normal(nnz).astype(np.float32)
        nans = np.where(rng.random(nnz) < 0.875, rng.choice(S.SPECIAL[:4], nnz), rng.integers(0, 5, nnz).astype(np.float32))
        nans[rp[3]:rp[4]] = np.resize(S.SPECIAL[:4], 100)                 # a row of only NaNs
        scores = {"lowest_bit": S.f32(0x3F800000 + rng.integers(0, 4, nnz)),
                  "sign": rng.choice(np.array([0.75, -0.75], np.float32), nnz),
                  "special": S.special_scores(rng, nnz, p_special=0.6),
                  "nans": nans.astype(np.float32)}
        _cache["keys"] = (len(lengths), COLS, rp, ci, va, scores)
    return _cache["keys"]


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _dev(gpu, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _read_map(sel, parent_nnz, gpu):
    import torch
    pos = torch.arange(parent_nnz, dtype=torch.int32, device=gpu)
    out = torch.full((sel.nnz,), -1, dtype=torch.int32, device=gpu)
    sel.select_gather(pos, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _got(sel, parent_nnz=None, gpu=None):
    rp, ci, va = sel.download()
    return (rp, ci, va, _read_map(sel, parent_nnz, gpu) if parent_nnz is not None else None)


def _assert_same(got, want, what):
    for name, g, w in zip(("row_ptr", "col_idx", "vals", "map"), got, want):
        if g is None or w is None:
            continue
        g, w = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        assert g.shape == w.shape, f"{what}: {name} has {g.size} entries, expected {w.size}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} places, first {bad[:5].tolist()}: {g[bad[:5]]} != {w[bad[:5]]}"


def _topk(capi, gpu, A, mat, k, score=None, abs_=False, what=""):
    """A.select_topk against the numpy statement, with the map."""
    rows, _, rp, ci, va = mat[:5]
    d_score = None if score is None else _dev(gpu, score, np.float32)
    sel = A.select_topk(k, d_score, abs=abs_, keep_map=True)
    try:
        assert (sel.rows, sel.cols) == (A.rows, A.cols)
        want = S.host_select_topk(rows, rp, ci, va, k, score, abs_)
        _assert_same(_got(sel, A.nnz, gpu), want, f"{what} k={k} abs={abs_}")
        assert sel.select_map_bytes() == 4 * sel.nnz and sel.transpose_map_bytes() == 0
    finally:
        sel.close()


def _threshold(capi, gpu, A, mat, thr, score=None, abs_=False, what=""):
    rows, _, rp, ci, va = mat[:5]
    d_score = None if score is None else _dev(gpu, score, np.float32)
    sel = A.select_threshold(thr, d_score, abs=abs_, keep_map=True)
    try:
        want = S.host_select_threshold(rows, rp, ci, va, thr, score, abs_)
        _assert_same(_got(sel, A.nnz, gpu), want, f"{what} threshold={thr} abs={abs_}")
        return sel.nnz
    finally:
        sel.close()


def _handle(capi, mat):
    rows, cols, rp, ci, va = mat[:5]
    return capi.CsrMatrix.from_host(rows, cols, rp, ci, va)


# ---- 1. row lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "shuffled"])
@pytest.mark.parametrize("order", ["mixed", "sorted"])
def test_row_lengths(pkg, gpu, order, form):
    mat = lengths_matrix(order, form)
    A = _handle(pkg.capi, mat)
    for k in KS:
        _topk(pkg.capi, gpu, A, mat, k, what=f"{order}/{form}")
    A.close()


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_equal", "two_values", "blocks_of_64", "blocks_of_65"])
def test_ties(pkg, gpu, kind):
    mat = ties_matrix()
    A = _handle(pkg.capi, mat)
    for k in sorted({n // 2 for n in TIE_ROWS} | {n - 1 for n in TIE_ROWS}):
        _topk(pkg.capi, gpu, A, mat, k, mat[5][kind], what=kind)
    A.close()


# ---- 3. keys ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("abs_", [False, True])
@pytest.mark.parametrize("kind", ["lowest_bit", "sign", "special", "nans"])
def test_keys(pkg, gpu, kind, abs_):
    mat = keys_matrix()
    A = _handle(pkg.capi, mat)
    for k in (1, 4, 37, 64, 300, 600):
        _topk(pkg.capi, gpu, A, mat, k, mat[5][kind], abs_, what=kind)
    A.close()


@pytest.mark.gpu
def test_null_score_is_the_matrix_own_values(pkg, gpu):
    rows, cols, rp, ci, _, scores = keys_matrix()
    mat = (rows, cols, rp, ci, scores["special"])               # the special set as the matrix's values
    A = _handle(pkg.capi, mat)
    for abs_ in (False, True):
        for k in (2, 70):
            _topk(pkg.capi, gpu, A, mat, k, None, abs_, what="own values")
            explicit = A.select_topk(k, _dev(gpu, mat[4]), abs=abs_)
            implicit = A.select_topk(k, abs=abs_)
            _assert_same(_got(explicit), _got(implicit), "explicit against implicit scores")
            explicit.close()
            implicit.close()
    A.close()


# ---- 4. threshold -------------------------------------------------------------------------------------------------------------
def _thresholds(score, abs_):
    """-Inf, -0, +0, a value present in the scores (in |scores| with abs: the median of what is compared), +Inf, FLT_MAX."""
    finite = score[np.isfinite(score)]
    compared = np.abs(finite) if abs_ else finite
    return [-np.inf, -0.0, 0.0, float(np.sort(compared)[len(compared) // 2]), np.inf, float(S.FLT_MAX)]


@pytest.mark.gpu
@pytest.mark.parametrize("abs_", [False, True])
@pytest.mark.parametrize("which", ["lengths", "ties", "keys"])
def test_threshold(pkg, gpu, which, abs_):
    if which == "lengths":
        mat = lengths_matrix("mixed", "shuffled")
        scores = {"own": None}
    else:
        mat = ties_matrix() if which == "ties" else keys_matrix()
        scores = mat[5]
    A = _handle(pkg.capi, mat)
    kept = []
    for name, score in scores.items():
        for thr in _thresholds(mat[4] if score is None else score, abs_):
            kept.append(_threshold(pkg.capi, gpu, A, mat, thr, score, abs_, what=f"{which}/{name}"))
    assert 0 in kept, "no case kept nothing"
    assert any(0 < n < A.nnz for n in kept)
    A.close()


# ---- 5. copy case and purity --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_copy_case(pkg, gpu):
    capi = pkg.capi
    mat = lengths_matrix("mixed", "shuffled")
    rows, cols, rp, ci, va = mat
    va = va.copy()
    va.view(np.uint32)[:4] = [0x80000000, 0x00000001, 0xFF800000, 0x7F7FFFFF]       # finite oddities and -Inf: no NaN
    A = capi.CsrMatrix.from_host(rows, cols, rp, ci, va)
    ident = np.arange(len(ci), dtype=np.uint32)
    for sel in (A.select_topk(4097, keep_map=True), A.select_topk(2 ** 31 - 1, keep_map=True),
                A.select_threshold(-np.inf, keep_map=True), A.select_threshold(-np.inf, abs=True, keep_map=True)):
        _assert_same(_got(sel, A.nnz, gpu), (rp, ci, va, ident), "the copy case")
        sel.close()
    A.close()


@pytest.mark.gpu
def test_two_calls_a_side_stream_and_both_parents(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    mat = lengths_matrix("mixed", "plain")
    rows, cols, rp, ci, va = mat
    want = S.host_select_topk(rows, rp, ci, va, 16)[:3]
    dev = (_dev(gpu, rp), _dev(gpu, ci), _dev(gpu, va))
    x = np.random.default_rng(3).uniform(-1, 1, cols).astype(np.float32)
    d_x = _dev(gpu, x)
    X = np.random.default_rng(4).uniform(-1, 1, (cols, 5)).astype(np.float32)
    for parent in ("from_host", "from_device"):
        A = capi.CsrMatrix.from_host(rows, cols, rp, ci, va) if parent == "from_host" else capi.CsrMatrix.from_device(rows, cols, *dev)
        A.plan(capi.TILED)
        described = A.plan_describe(capi.TILED)
        first = A.select_topk(16)
        second = A.select_topk(16, keep_map=True)
        y = torch.empty(rows, dtype=torch.float32, device=gpu)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(20):
            A.run(capi.TILED, d_x, y)
        third = A.select_topk(16, stream=side)
        for _ in range(20):
            A.run(capi.TILED, d_x, y)
        torch.cuda.synchronize()
        for sel in (first, second, third):
            _assert_same(_got(sel), want, f"{parent}: a repeated call")
        # the parent: arrays and plans as they were
        _assert_same(A.download(), (rp, ci, va), f"{parent}: the parent changed")
        assert A.plan_describe(capi.TILED) == described
        A.run(capi.TILED, d_x, y)
        torch.cuda.synchronize()
        y64, mag = oracle.spmv_f64(rp, ci, va, x)
        assert_close_to_oracle(y.cpu().numpy(), y64, mag, f"{parent}: the parent's plan after a select")
        # the result is an ordinary handle
        capi.check(capi.lib().spmv_csr_validate(first._h, 0))
        assert (first.rows, first.cols, first.nnz) == (rows, cols, len(want[1]))
        assert first.column_range() == (int(want[1].min()), int(want[1].max()))
        first.plan(capi.AUTO)
        ys = torch.full((rows,), float("nan"), dtype=torch.float32, device=gpu)
        first.run(capi.AUTO, d_x, ys)
        first.spmm_plan()
        Y = torch.full((rows, 5), float("nan"), dtype=torch.float32, device=gpu)
        first.spmm(_dev(gpu, X), Y)
        torch.cuda.synchronize()
        y64, mag = oracle.spmv_f64(*want, x)
        assert_close_to_oracle(ys.cpu().numpy(), y64, mag, f"{parent}: SPMV_AUTO on the selection")
        for c in range(5):
            y64, mag = oracle.spmv_f64(*want, np.ascontiguousarray(X[:, c]))
            assert_close_to_oracle(np.ascontiguousarray(Y.cpu().numpy()[:, c]), y64, mag, f"{parent}: spmm column {c}")
        for h in (first, second, third, A):
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r0,r1", [(0, 64), (64, 192), (128, 300), (1, 65), (37, 101), (63, 64), (250, 300), (5, 5)])
def test_a_row_block_selected_alone_equals_the_rows_of_the_whole(pkg, gpu, r0, r1):
    capi = pkg.capi
    rows, cols, rp, ci, va = lengths_matrix("mixed", "shuffled")
    for k, thr in ((3, 0.25), (70, -0.5)):
        w_rp, w_ci, w_va, _ = S.host_select_topk(rows, rp, ci, va, k)
        t_rp, t_ci, t_va, _ = S.host_select_threshold(rows, rp, ci, va, thr)
        lo, hi = int(rp[r0]), int(rp[r1])
        B = capi.CsrMatrix.from_host(r1 - r0, cols, rp[r0:r1 + 1] - lo, ci[lo:hi], va[lo:hi])
        for sel, (e_rp, e_ci, e_va) in ((B.select_topk(k), (w_rp, w_ci, w_va)), (B.select_threshold(thr), (t_rp, t_ci, t_va))):
            a, b = int(e_rp[r0]), int(e_rp[r1])
            _assert_same(_got(sel), (e_rp[r0:r1 + 1] - a, e_ci[a:b], e_va[a:b]), f"rows {r0}..{r1} k={k}")
            sel.close()
        B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(0, 0), (0, 5), (5, 0), (5, 5), (300, 7)])
def test_without_nonzeros(pkg, gpu, rows, cols):
    capi = pkg.capi
    A = capi.CsrMatrix.from_host(rows, cols, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for sel in (A.select_topk(3, keep_map=True), A.select_threshold(0.0, keep_map=True), A.select_topk(1)):
        assert (sel.rows, sel.cols, sel.nnz) == (rows, cols, 0)
        assert np.array_equal(sel.download()[0], np.zeros(rows + 1, np.int32))
        capi.check(capi.lib().spmv_csr_validate(sel._h, 0))
        sel.close()
    A.close()


# ---- 6. companions ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_select_values_follows_rewritten_values(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    rows, cols, rp, ci, va = lengths_matrix("mixed", "plain")
    d_rp, d_ci, d_va = _dev(gpu, rp), _dev(gpu, ci), _dev(gpu, va)
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    score = np.random.default_rng(21).standard_normal(len(ci)).astype(np.float32)
    sel = A.select_topk(8, _dev(gpu, score), keep_map=True)
    s_rp, s_ci, s_va, s_map = S.host_select_topk(rows, rp, ci, va, 8, score)
    _assert_same(_got(sel, A.nnz, gpu), (s_rp, s_ci, s_va, s_map), "as built")
    x = np.random.default_rng(22).uniform(-1, 1, cols).astype(np.float32)
    d_x = _dev(gpu, x)
    y = torch.empty(rows, dtype=torch.float32, device=gpu)
    sel.plan(capi.TILED)
    sel.plan_set(capi.PANEL, [capi.PANEL, 0, 0, 0, 0, 0, 1, 0])
    new = (va * np.float32(-0.75) + np.float32(0.125)).astype(np.float32)
    d_va.copy_(_dev(gpu, new))                                  # in place: A borrows this tensor
    sel.select_values(A)
    _assert_same(sel.download(), (s_rp, s_ci, new[s_map]), "after select_values")
    y64, mag = oracle.spmv_f64(s_rp, s_ci, new[s_map], x)
    y.fill_(float("nan"))
    sel.run(capi.TILED, d_x, y)
    torch.cuda.synchronize()
    assert_close_to_oracle(y.cpu().numpy(), y64, mag, "a TILED plan made before the refresh")
    with pytest.raises(capi.SpmvError) as e:
        sel.run(capi.PANEL, d_x, y)
    assert e.value.status == capi.ERR_STALE_PLAN
    sel.plan(capi.PANEL)
    y.fill_(float("nan"))
    sel.run(capi.PANEL, d_x, y)
    torch.cuda.synchronize()
    assert_close_to_oracle(y.cpu().numpy(), y64, mag, "a re-planned PANEL")
    sel.close()
    A.close()


@pytest.mark.gpu
def test_gather_then_scatter_is_the_identity_on_the_kept_positions(pkg, gpu):
    import torch
    capi = pkg.capi
    mat = lengths_matrix("mixed", "shuffled")
    rows, _, rp, ci, va = mat
    A = _handle(capi, mat)
    sel = A.select_topk(5, keep_map=True)
    kept = S.host_select_topk(rows, rp, ci, va, 5)[3].astype(np.int64)
    n, m = A.nnz, sel.nnz
    rng = np.random.default_rng(31)
    for count in (1, 3):
        src = rng.integers(1, 2 ** 31 - 1, size=(count, n + 5), dtype=np.int64).astype(np.int32)      # strides beyond the arrays
        d_src = _dev(gpu, src)[:, :n] if count > 1 else _dev(gpu, src)[0, :n]
        mid = torch.full((count, m + 3), -7, dtype=torch.int32, device=gpu)
        d_mid = mid[:, :m] if count > 1 else mid[0, :m]
        back = torch.zeros((count, n + 2), dtype=torch.int32, device=gpu)
        d_back = back[:, :n] if count > 1 else back[0, :n]
        sel.select_gather(d_src, d_mid)
        sel.select_scatter(d_mid, d_back)
        torch.cuda.synchronize()
        assert np.array_equal(mid.cpu().numpy()[:, :m], src[:, :n][:, kept]), f"count={count}: gather"
        assert bool((mid[:, m:] == -7).all()) and bool((back[:, n:] == 0).all()), "words between the arrays were written"
        want = np.zeros((count, n), np.int32)
        want[:, kept] = src[:, :n][:, kept]
        assert np.array_equal(back.cpu().numpy()[:, :n], want), f"count={count}: scatter"
    sel.close()
    A.close()


@pytest.mark.gpu
def test_companions_in_a_graph(pkg, gpu):
    import torch
    capi = pkg.capi
    rows, cols, rp, ci, va = lengths_matrix("sorted", "plain")
    d_va = _dev(gpu, va)
    A = capi.CsrMatrix.from_device(rows, cols, _dev(gpu, rp), _dev(gpu, ci), d_va)
    sel = A.select_topk(6, abs=True, keep_map=True)
    s_rp, s_ci, _, s_map = S.host_select_topk(rows, rp, ci, va, 6, abs_=True)
    n, m = A.nnz, sel.nnz
    src = torch.arange(n, dtype=torch.float32, device=gpu)
    mid = torch.empty(m, dtype=torch.float32, device=gpu)
    back = torch.zeros(n, dtype=torch.float32, device=gpu)
    o_rp = torch.empty(rows + 1, dtype=torch.int32, device=gpu)
    o_ci = torch.empty(m, dtype=torch.int32, device=gpu)
    o_va = torch.empty(m, dtype=torch.float32, device=gpu)

    def enqueue():
        sel.select_values(A)
        sel.select_gather(src, mid)
        sel.select_scatter(mid, back)
        sel.copy_arrays(o_rp, o_ci, o_va)

    enqueue()                                                      # warm (module load) outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    for step in (1, 2):
        new = (va * np.float32(step + 1)).astype(np.float32)
        d_va.copy_(_dev(gpu, new))
        src.mul_(2.0)
        mid.fill_(-1.0)
        back.zero_()
        g.replay()
        torch.cuda.synchronize()
        _assert_same((o_rp.cpu().numpy(), o_ci.cpu().numpy(), o_va.cpu().numpy()), (s_rp, s_ci, new[s_map]), f"replay {step}")
        h_src = src.cpu().numpy()
        assert np.array_equal(mid.cpu().numpy(), h_src[s_map.astype(np.int64)])
        want = np.zeros(n, np.float32)
        want[s_map.astype(np.int64)] = h_src[s_map.astype(np.int64)]
        assert np.array_equal(back.cpu().numpy(), want)
        _assert_same(sel.download(), (s_rp, s_ci, new[s_map]), "copy_arrays against download")
    del g
    sel.close()
    A.close()


@pytest.mark.gpu
def test_refusals(pkg, gpu):
    import ctypes as C
    import torch
    capi = pkg.capi
    lib = capi.lib()
    mat = lengths_matrix("sorted", "plain")
    A = _handle(capi, mat)
    n = A.nnz
    score = torch.zeros(n + 1, dtype=torch.float32, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    out = C.c_void_p()

    def refused(rc, name):
        assert rc == capi.ERR_INVALID, (name, rc)
        assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error().decode()
        assert out.value is None, "*out was written"

    top, thr = "spmv_csr_select_topk", "spmv_csr_select_threshold"
    for k in (0, -1):
        refused(lib.spmv_csr_select_topk(A._h, None, k, 0, 0, st, C.byref(out)), top)
    refused(lib.spmv_csr_select_threshold(A._h, None, float("nan"), 0, 0, st, C.byref(out)), thr)
    for flags in (2, 3, -1):
        refused(lib.spmv_csr_select_topk(A._h, None, 4, flags, 0, st, C.byref(out)), top)
        refused(lib.spmv_csr_select_threshold(A._h, None, 0.5, flags, 0, st, C.byref(out)), thr)
    for keep in (2, -1):
        refused(lib.spmv_csr_select_topk(A._h, None, 4, 0, keep, st, C.byref(out)), top)
        refused(lib.spmv_csr_select_threshold(A._h, None, 0.5, 0, keep, st, C.byref(out)), thr)
    refused(lib.spmv_csr_select_topk(A._h, score.data_ptr() + 2, 4, 0, 0, st, C.byref(out)), top)
    refused(lib.spmv_csr_select_threshold(A._h, score.data_ptr() + 1, 0.5, 0, 0, st, C.byref(out)), thr)
    refused(lib.spmv_csr_select_topk(None, None, 4, 0, 0, st, C.byref(out)), top)
    refused(lib.spmv_csr_select_topk(A._h, None, 4, 0, 0, st, None), top)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            refused(lib.spmv_csr_select_topk(A._h, None, 4, 0, 0, None, C.byref(out)), top)
            refused(lib.spmv_csr_copy_arrays(A._h, None, None, None, None), "spmv_csr_copy_arrays")

    # the companions: which handle carries which map
    sel = A.select_topk(4, keep_map=True)
    bare = A.select_topk(4)
    T = A.transpose(keep_map=True)
    m = sel.nnz
    assert sel.select_map_bytes() == 4 * m and bare.select_map_bytes() == 0 and T.select_map_bytes() == 0 and A.select_map_bytes() == 0
    assert sel.transpose_map_bytes() == 0 and T.transpose_map_bytes() == 4 * n
    src = torch.arange(n, dtype=torch.int32, device=gpu)
    dst = torch.full((3, n + 4), -5, dtype=torch.int32, device=gpu)
    before = dst.clone()
    vals_before = sel.download()[2]

    def companion(rc, name):
        assert rc == capi.ERR_INVALID, (name, rc)
        assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error().decode()

    ga, sc, va_ = "spmv_csr_select_gather", "spmv_csr_select_scatter", "spmv_csr_select_values"
    for h in (bare, T, A):                                           # no select map
        companion(lib.spmv_csr_select_gather(h._h, 1, src.data_ptr(), 0, dst.data_ptr(), 0, st), ga)
        companion(lib.spmv_csr_select_scatter(h._h, 1, src.data_ptr(), 0, dst.data_ptr(), 0, st), sc)
        companion(lib.spmv_csr_select_values(h._h, A._h, st), va_)
    companion(lib.spmv_csr_transpose_gather(sel._h, 1, src.data_ptr(), 0, dst.data_ptr(), 0, st), "spmv_csr_transpose_gather")
    companion(lib.spmv_csr_transpose_values(sel._h, A._h, st), "spmv_csr_transpose_values")
    for fn, name, dst_len in ((lib.spmv_csr_select_gather, ga, m), (lib.spmv_csr_select_scatter, sc, n)):
        companion(fn(sel._h, 0, src.data_ptr(), 0, dst.data_ptr(), 0, st), name)                       # count < 1
        companion(fn(sel._h, 1, None, 0, dst.data_ptr(), 0, st), name)                                 # a null array
        companion(fn(sel._h, 1, src.data_ptr(), 0, None, 0, st), name)
        companion(fn(sel._h, 1, src.data_ptr() + 2, 0, dst.data_ptr(), 0, st), name)                   # alignment
        companion(fn(sel._h, 1, src.data_ptr(), 0, dst.data_ptr() + 1, 0, st), name)
        companion(fn(sel._h, 2, src.data_ptr(), -1, dst.data_ptr(), n + 4, st), name)                  # a negative stride
        companion(fn(sel._h, 2, src.data_ptr(), 0, dst.data_ptr(), -1, st), name)
        companion(fn(sel._h, 2, src.data_ptr(), 0, dst.data_ptr(), dst_len - 1, st), name)             # arrays of dst would overlap
        companion(fn(sel._h, 2, src.data_ptr(), 2 ** 62, dst.data_ptr(), n + 4, st), name)             # byte offsets overflow
    other = capi.CsrMatrix.from_host(3, 3, np.asarray([0, 1, 1, 2], np.int32), np.asarray([0, 2], np.int32), np.ones(2, np.float32))
    companion(lib.spmv_csr_select_values(sel._h, other._h, st), va_)                                    # not the parent's shape
    companion(lib.spmv_csr_select_values(sel._h, bare._h, st), va_)                                     # its shape, not its nnz
    companion(lib.spmv_csr_select_values(sel._h, None, st), va_)
    torch.cuda.synchronize()
    assert torch.equal(dst, before), "a refused call wrote"
    assert np.array_equal(sel.download()[2].view(np.uint32), vals_before.view(np.uint32)), "a refused call changed the values"
    # the Python layer's own checks (dtype, shape, contiguity, device)
    good_dst = torch.empty(m, dtype=torch.int32, device=gpu)
    for bad_src, bad_dst in ((src.double(), good_dst), (src[:-1], good_dst), (src, good_dst.float()), (src.cpu(), good_dst),
                             (torch.zeros(2 * n, dtype=torch.int32, device=gpu)[::2], good_dst), (src, torch.empty((2, m), dtype=torch.int32, device=gpu))):
        with pytest.raises(ValueError, match="select_gather"):
            sel.select_gather(bad_src, bad_dst)
    with pytest.raises(ValueError, match="copy_arrays"):
        sel.copy_arrays(torch.empty(A.rows, dtype=torch.int32, device=gpu), None)
    with pytest.raises(ValueError, match="score must be"):
        A.select_topk(3, score[:n].double())
    for h in (other, T, bare, sel, A):
        h.close()


# ---- 7. at a moderate size ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("band", [8192, 0])
def test_power_law_rows_at_65536(pkg, oracle, gpu, band):
    import torch
    w = pkg.workloads.config("c3", band=band, scale=1 / 64)
    assert w.rows == 65536
    prob = synth_problem(pkg, oracle, gpu, w)
    lengths = np.diff(prob.row_ptr)
    assert lengths.max() > 512 and lengths.min() <= 4, "the law has rows on both sides of every path"
    score = np.random.default_rng(41).standard_normal(len(prob.col_idx)).astype(np.float32)
    d_score = torch.from_numpy(score).to(gpu)
    for k in (4, 16):
        sel = prob.A.select_topk(k, d_score, keep_map=True)
        want = S.host_select_topk(w.rows, prob.row_ptr, prob.col_idx, prob.vals, k, score)
        _assert_same(_got(sel, prob.A.nnz, gpu), want, f"c3/64 band {band} k={k}")
        sel.close()
    prob.A.close()


# ---- 8. memory ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_memory_comes_back(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    w = pkg.workloads.config("c3", band=0, scale=1 / 64)
    rp = pkg.workloads.row_ptr(w)
    ci, va = oracle.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, rp)
    x = torch.ones(w.cols, dtype=torch.float32, device=gpu)
    y = torch.empty(w.rows, dtype=torch.float32, device=gpu)
    free = []
    for _ in range(4):
        A = capi.CsrMatrix.from_host(w.rows, w.cols, rp, ci, va)
        sel = A.select_topk(8, abs=True, keep_map=True)
        thr = A.select_threshold(0.0)
        sel.plan(capi.AUTO)
        sel.run(capi.AUTO, x, y)
        torch.cuda.synchronize()
        for h in (thr, sel, A):
            h.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"


# ---- 9. the layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_topk_pattern_feeds_fused_attention(pkg, gpu):
    import torch
    capi, SA = pkg.capi, pkg.sparse_attention
    rows, cols, kdim, kv, k, scale = 1024, 768, 24, 16, 12, 0.3
    lengths = np.random.default_rng(51).integers(0, 97, rows)
    lengths[:4] = [0, 5, 600, 64]                                   # an empty query, fewer candidates than k, a long row
    rp, ci = S.random_csr(np.random.default_rng(52), rows, cols, lengths)
    d_rp, d_ci = _dev(gpu, rp), _dev(gpu, ci)
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, torch.zeros(len(ci), dtype=torch.float32, device=gpu))
    gen = torch.Generator(device="cpu").manual_seed(53)
    Q, K, V = (torch.randn(s, generator=gen).to(gpu) for s in ((rows, kdim), (cols, kdim), (cols, kv)))
    t_rp, t_ci = SA.topk_pattern(A, Q, K, k, scale=scale)
    # the kept set is the numpy statement's on the scores the device computed
    A.spmm_plan()
    score = torch.empty(A.nnz, dtype=torch.float32, device=gpu)
    A.sddmm(Q, K, score)
    score.mul_(scale)
    torch.cuda.synchronize()
    w_rp, w_ci, _, _ = S.host_select_topk(rows, rp, ci, np.zeros(len(ci), np.float32), k, score.cpu().numpy())
    assert t_rp.dtype == torch.int32 and t_ci.dtype == torch.int32 and t_rp.device == Q.device
    _assert_same((t_rp.cpu().numpy(), t_ci.cpu().numpy()), (w_rp, w_ci), "topk_pattern")
    assert np.array_equal(np.diff(w_rp), np.minimum(lengths, k))
    att = SA.FusedSparseAttention(rows, cols, t_rp, t_ci, scale=scale)
    O = att(Q, K, V)
    torch.cuda.synchronize()
    # dense masked attention on the same kept set: fp64 the reference, torch's fp32 the yardstick (the fused tests' rule)
    mask = torch.zeros((rows, cols), dtype=torch.bool, device=gpu)
    row_of = torch.repeat_interleave(torch.arange(rows, device=gpu), torch.from_numpy(np.diff(w_rp)).to(gpu))
    mask[row_of, t_ci.long()] = True

    def dense(dt):
        s = scale * (Q.to(dt) @ K.to(dt).t())
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=1)
        p = torch.where(mask.any(1, keepdim=True), p, torch.zeros((), dtype=dt, device=gpu))
        return p @ V.to(dt), p

    O64, P = dense(torch.float64)
    O32, _ = dense(torch.float32)
    mag = P @ V.double().abs()
    live = mag > 0
    assert bool((O[~live] == 0).all())
    ours = float(((O.double() - O64).abs()[live] / mag[live]).max())
    yard = float(((O32.double() - O64).abs()[live] / mag[live]).max())
    print(f"topk_pattern + fused attention: normalised error {ours:.3g}, torch fp32 dense {yard:.3g}")
    assert ours <= max(4.0 * yard, RTOL)
    att.close()
    A.close()


@pytest.mark.gpu
def test_sparse_layer_pruned(pkg, oracle, gpu):
    import torch
    capi, SL = pkg.capi, pkg.sparse_layer
    rows, cols, rp, ci, va = lengths_matrix("mixed", "plain")
    k, width = 20, 6
    d_rp, d_ci = _dev(gpu, rp), _dev(gpu, ci)
    vals = _dev(gpu, va).requires_grad_(True)
    layer = SL.SparseLayer(rows, cols, d_rp, d_ci, vals)
    small = layer.pruned(k)
    s_rp, s_ci, s_va, s_map = S.host_select_topk(rows, rp, ci, va, k, abs_=True)
    assert small.vals.is_leaf and small.vals.requires_grad and small.vals.numel() == len(s_ci) and small.vals is not layer.vals
    _assert_same(small.A.download(), (s_rp, s_ci, s_va), "the pruned layer's matrix")
    assert np.array_equal(_read_map(small.selection, layer.A.nnz, gpu), s_map)
    _assert_same(layer.A.download(), (rp, ci, va), "the parent layer")
    X = torch.from_numpy(np.random.default_rng(61).uniform(-1, 1, (cols, width)).astype(np.float32)).to(gpu)
    Yp = small(X)
    Yf = layer(X)
    torch.cuda.synchronize()
    # the parent's forward with the dropped values zeroed: bit for bit where a row lost nothing, the SpMM bound elsewhere
    untouched = np.diff(rp) <= k
    assert untouched.any() and (~untouched).any()
    assert np.array_equal(Yp.detach().cpu().numpy()[untouched].view(np.uint32), Yf.detach().cpu().numpy()[untouched].view(np.uint32))
    zeroed = np.zeros_like(va)
    zeroed[s_map.astype(np.int64)] = va[s_map.astype(np.int64)]
    for c in range(width):
        y64, mag = oracle.spmv_f64(rp, ci, zeroed, np.ascontiguousarray(X.cpu().numpy()[:, c]))
        assert_close_to_oracle(np.ascontiguousarray(Yp.detach().cpu().numpy()[:, c]), y64, mag, f"pruned forward column {c}")
    G = torch.ones_like(Yp)
    Yp.backward(G)
    torch.cuda.synchronize()
    assert small.vals.grad is not None and small.vals.grad.shape == (len(s_ci),) and layer.vals.grad is None
    # dvals[m] = sum_c G[row, c] X[col, c] = the row sum of X at the kept column
    want = X.double().sum(1).cpu().numpy()[s_ci.astype(np.int64)]
    mag = X.double().abs().sum(1).cpu().numpy()[s_ci.astype(np.int64)]
    assert np.all(np.abs(small.vals.grad.cpu().numpy().astype(np.float64) - want) <= RTOL * mag + 1e-37)
    small.close()
    layer.close()


# ---- 10. the checked library --------------------------------------------------------------------------------------------------
CHECKED_CASES = (("lengths", 65), ("ties", 256))


def _checked_case(name):
    if name == "lengths":
        return lengths_matrix("mixed", "shuffled") + (None,)
    mat = ties_matrix()
    return mat[:5] + (mat[5]["blocks_of_65"],)


def child_main(outdir):
    """The child: both cases through libspmv_hip_checked.so; the results and the violation table go to outdir."""
    sys.path.insert(0, os.fspath(ROOT))
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    capi = pkg.capi
    capi.use_library(capi.CHECKED_LIB_PATH)
    gpu = torch.device("cuda:0")
    capi.debug_bounds()
    for name, k in CHECKED_CASES:
        rows, cols, rp, ci, va, score = _checked_case(name)
        A = capi.CsrMatrix.from_host(rows, cols, rp, ci, va)
        sel = A.select_topk(k, None if score is None else _dev(gpu, score), keep_map=True)
        g_rp, g_ci, g_va, g_map = _got(sel, A.nnz, gpu)
        thr = A.select_threshold(0.5, None if score is None else _dev(gpu, score))
        t_rp, t_ci, t_va = thr.download()
        np.savez(Path(outdir) / f"{name}.npz", rp=g_rp, ci=g_ci, va=g_va, map=g_map, t_rp=t_rp, t_ci=t_ci, t_va=t_va,
                 violations=np.asarray(len(capi.debug_bounds())))
        for h in (thr, sel, A):
            h.close()
    print("checked child ok")


@pytest.mark.gpu
def test_checked_library(pkg, gpu, tmp_path):
    assert pkg.capi.CHECKED_LIB_PATH.exists(), f"{pkg.capi.CHECKED_LIB_PATH} missing: build() makes it"
    r = subprocess.run([sys.executable, os.fspath(Path(__file__).resolve()), os.fspath(tmp_path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"the checked child failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    for name, k in CHECKED_CASES:
        rows, _, rp, ci, va, score = _checked_case(name)
        z = np.load(tmp_path / f"{name}.npz")
        assert int(z["violations"]) == 0
        _assert_same((z["rp"], z["ci"], z["va"], z["map"]), S.host_select_topk(rows, rp, ci, va, k, score), f"checked {name}")
        _assert_same((z["t_rp"], z["t_ci"], z["t_va"]), S.host_select_threshold(rows, rp, ci, va, 0.5, score)[:3], f"checked {name} threshold")


if __name__ == "__main__":
    child_main(sys.argv[1])
