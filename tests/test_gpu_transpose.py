"""GPU (-m gpu): spmv_csr_transpose / spmv_csr_transpose_values (include/spmv_hip.h "the transpose").

The expectation is always numpy's (np.argsort(col_idx, kind="stable"), np.bincount: test_transpose_host.host_transpose) or,
at config 4's size, torch's stable sort on the device -- never a kernel of this library.

  structure     T.download() equals the numpy transposition bit for bit (row_ptr, col_idx, the uint32 view of vals with
                NaN payloads, +-Inf, -0.0 and subnormals among them) for every matrix of _exact.MATRICES, plain and
                shuffled (unsorted rows, ~1/8 duplicates), every golden fixture and four stress patterns; owning and
                borrowing parents; spmv_csr_validate, dims, column_range.
  determinism   two transposes, and one made on a side stream while the default stream multiplies: identical bytes.
  involution    transpose(transpose(A)) is A with every row stably sorted by column.
  every path    _exact.Exact data put on T's structure (the row scales belong to T's rows) and carried back to A through
                the inverse permutation: every entry of test_gpu_exact.PATHS on a fresh A.transpose() returns
                Exact.expected() bit for bit (two runs, guard bands, x NaN at A's empty rows; the subnormal copy too).
  SpMM          spmm_plan + spmm on T, k = 1, 4, 17: every column exact.
  values        transpose_values after an in-place rewrite of A's vals; live plans follow, copying plans are stale;
                inside torch.cuda.graph; the refusals.
  at size       configs 2 and 3 (band 8192 and uniform) against the fp64 oracle on the numpy-transposed arrays; config 4
                against torch's stable sort through SPMV_SCALAR products.
  memory        four rounds of create / transpose / plan / run / destroy leave free device memory where it was.
  CLI           sparse_sgemv --transpose.
"""
import subprocess

import numpy as np
import pytest

import _exact as E
from _util import assert_close_to_oracle, synth_problem
from conftest import GOLDEN_NAMES, load_golden
from test_gpu_exact import KNOBS, PATHS, SENTINEL, XS, _Dev, _describe_mismatch, _has_duplicates, _mismatches
from test_transpose_host import host_transpose

pytestmark = pytest.mark.gpu
MIB = 1 << 20
ODD_BITS = (0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff)   # 2 NaNs, +-Inf, -0, subnormals


def _odd_vals(nnz, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    va = rng.standard_normal(nnz).astype(np.float32)
    if nnz:
        pos = rng.choice(nnz, size=min(len(ODD_BITS), nnz), replace=False)
        va.view(np.uint32)[pos] = np.asarray(ODD_BITS[:pos.size], np.uint32)
    return va


def _upload(gpu, rp, ci, va):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(rp, np.int32)).to(gpu), torch.from_numpy(np.ascontiguousarray(ci, np.int32)).to(gpu),
            torch.from_numpy(np.ascontiguousarray(va, np.float32)).to(gpu))


def _same(got, want):
    bad = [n for n, g, w in zip(("row_ptr", "col_idx", "vals"), got, want)
           if not np.array_equal(np.asarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))]
    return "" if not bad else f"{bad} differ"


def _check_structure(capi, gpu, rows, cols, rp, ci, va, what):
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    want = host_transpose(rows, cols, rp, ci, va)[:3]
    lengths = np.diff(rp)
    nonempty = np.flatnonzero(lengths)
    want_range = (int(nonempty[0]), int(nonempty[-1])) if nonempty.size else (rows, -1)
    dev = _upload(gpu, rp, ci, va)
    for parent in ("from_host", "from_device"):
        A = capi.CsrMatrix.from_host(rows, cols, rp, ci, va) if parent == "from_host" else capi.CsrMatrix.from_device(rows, cols, *dev)
        T = A.transpose()
        try:
            assert (T.rows, T.cols, T.nnz) == (cols, rows, len(ci)), f"{what}/{parent}: dims {(T.rows, T.cols, T.nnz)}"
            capi.check(capi.lib().spmv_csr_validate(T._h, 0))
            assert _same(T.download(), want) == "", f"{what}/{parent}: {_same(T.download(), want)}"
            assert T.column_range() == want_range, f"{what}/{parent}: column_range {T.column_range()} != {want_range}"
            assert T.transpose_map_bytes() == 0
            assert _same(A.download(), (rp, ci, va)) == "", f"{what}/{parent}: the parent changed"
        finally:
            T.close()
            A.close()


# ---- 1. structure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "shuffled"])
@pytest.mark.parametrize("name", E.MATRICES)
def test_structure_exact_matrices(pkg, oracle, gpu, name, form):
    s = E.structure(name, pkg, oracle)
    if form == "shuffled":
        s = E.shuffled(s, name)[0]
    _check_structure(pkg.capi, gpu, s.rows, s.cols, s.rp, s.ci, _odd_vals(s.nnz, len(name)), f"{name}/{form}")


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_structure_golden(pkg, gpu, name):
    g = load_golden(name)
    _check_structure(pkg.capi, gpu, g.N, g.M, g.row_ptr, g.col_idx, g.vals, name)


def _stress(which):
    rng = np.random.Generator(np.random.PCG64(77))
    if which == "three_columns":            # 2^20 nonzeros that all lie in 3 columns: long runs of equal keys in every tile
        rows, per = 1 << 17, 8
        rp = np.arange(rows + 1, dtype=np.int64) * per
        return rows, 70_000, rp, rng.choice(np.asarray([5, 40_000, 69_999]), size=rows * per)
    if which == "one_long_row":             # one row of 200 000 nonzeros: every row of T has at most one entry
        return 1, 300_000, np.asarray([0, 200_000]), rng.choice(300_000, size=200_000, replace=False)
    if which == "one_by_one":
        return 1, 1, np.asarray([0, 1]), np.asarray([0])
    raise KeyError(which)


@pytest.mark.parametrize("which", ["three_columns", "one_long_row", "one_by_one"])
def test_structure_stress(pkg, gpu, which):
    rows, cols, rp, ci = _stress(which)
    _check_structure(pkg.capi, gpu, rows, cols, rp, ci, _odd_vals(len(ci), 3), which)


@pytest.mark.parametrize("rows,cols", [(0, 0), (0, 5), (5, 0), (5, 5)])
def test_structure_without_nonzeros(pkg, gpu, rows, cols):
    _check_structure(pkg.capi, gpu, rows, cols, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                     f"empty {rows}x{cols}")


# ---- 2. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_columns", "c2_uniform", "c3_powerlaw"])
def test_two_transposes_and_a_side_stream_give_the_same_bytes(pkg, oracle, gpu, name):
    import torch
    capi = pkg.capi
    if name == "three_columns":
        rows, cols, rp, ci = _stress(name)
    else:
        s = E.shuffled(E.structure(name, pkg, oracle), name)[0]
        rows, cols, rp, ci = s.rows, s.cols, s.rp, s.ci
    va = _odd_vals(len(ci), 9)
    dev = _upload(gpu, rp, ci, va)
    A = capi.CsrMatrix.from_device(rows, cols, *dev)
    first = A.transpose(keep_map=True).download()
    second = A.transpose().download()
    assert _same(second, first) == "", _same(second, first)
    # an unrelated multiply keeps the default stream busy while a side stream transposes
    busy = E.structure("c4_band4096", pkg, oracle)
    B = capi.CsrMatrix.from_device(busy.rows, busy.cols, *_upload(gpu, busy.rp, busy.ci, np.ones(busy.nnz, np.float32)))
    B.plan(capi.TILED)
    bx = torch.ones(busy.cols, dtype=torch.float32, device=gpu)
    by = torch.empty(busy.rows, dtype=torch.float32, device=gpu)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(20):
        B.run(capi.TILED, bx, by)
    third = A.transpose(stream=side)
    for _ in range(20):
        B.run(capi.TILED, bx, by)
    torch.cuda.synchronize()
    assert _same(third.download(), first) == "", _same(third.download(), first)
    assert _same(first, host_transpose(rows, cols, rp, ci, va)[:3]) == ""
    B.close()
    A.close()


# ---- 3. involution ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "shuffled"])
@pytest.mark.parametrize("name", E.MATRICES)
def test_double_transpose_is_the_row_wise_stable_column_sort(pkg, oracle, gpu, name, form):
    capi = pkg.capi
    s = E.structure(name, pkg, oracle)
    if form == "shuffled":
        s = E.shuffled(s, name)[0]
    va = _odd_vals(s.nnz, 11)
    A = capi.CsrMatrix.from_host(s.rows, s.cols, s.rp, s.ci, va)
    T = A.transpose()
    TT = T.transpose()
    order = np.lexsort((np.arange(s.nnz), s.ci, s.row_of))
    if form == "plain":
        assert np.array_equal(order, np.arange(s.nnz)), "a plain matrix has sorted rows"
    assert (TT.rows, TT.cols, TT.nnz) == (s.rows, s.cols, s.nnz)
    assert _same(TT.download(), (s.rp, s.ci[order], va[order])) == "", f"{name}/{form}"
    for h in (TT, T, A):
        h.close()


# ---- 4. every path multiplies by it, exactly ------------------------------------------------------------------------------
def _exact_on_T(s, name):
    """Exact data on the transposed structure, carried back to A's storage order: [(label, A's vals, x, expected)], T's
    structure.  x (one entry per row of A) is NaN at every empty row of A: no nonzero of T refers to it."""
    t_rp, t_ci, _, perm = host_transpose(s.rows, s.cols, s.rp, s.ci, np.zeros(s.nnz, np.float32))
    st = E.Structure(s.cols, s.rows, t_rp, t_ci)
    ex = E.Exact(st, name + "/T")
    empty = np.diff(s.rp) == 0
    out = []
    for label, vt, x, want in (("int", ex.vals(), ex.x(), ex.expected()), ("subnormal", ex.sub_vals(), ex.sub_x(), ex.sub_expected())):
        va = np.empty(s.nnz, np.float32)
        va[perm] = vt
        x = x.copy()
        x[empty] = np.nan
        out.append((label, va, x, want))
    return st, ex, out


def _run_paths_on_T(pkg, monkeypatch, gpu, s, st, problems):
    """Every entry of PATHS on a fresh A.transpose() per path and problem; returns the failures and the labels that ran."""
    capi = pkg.capi

    def make(arrays):
        A = capi.CsrMatrix.from_device(s.rows, s.cols, *arrays)
        T = A.transpose()
        A.close()
        return T

    return _run_paths_on_handle(pkg, monkeypatch, gpu, st, [(label, _upload(gpu, s.rp, s.ci, va), x, want)
                                                            for label, va, x, want in problems], make)


def _run_paths_on_handle(pkg, monkeypatch, gpu, st, problems, make):
    """Every entry of PATHS on a fresh derived handle per path and problem: make(payload) builds it, st is its structure,
    problems = [(label, payload, x, expected y)]; returns the failures and the labels that ran."""
    capi = pkg.capi
    failures, ran = [], set()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    devs = []
    for label, payload, x, want in problems:
        d = _Dev(gpu, st, np.zeros(st.nnz, np.float32))          # (its arrays are not used: y, the guards and the cases are)
        d.add(label, x, want)
        devs.append((d, payload))
    for label, v, env, params, want_desc in PATHS:
        with monkeypatch.context() as mp:
            for k, val in env.items():
                mp.setenv(k, val)
            for d, payload in devs:
                T = make(payload)
                try:
                    try:
                        T.plan(v) if params is None else T.plan_set(v, params)
                    except capi.SpmvError as e:
                        msg = str(e)
                        if v == XS and ("dense-ish" in msg or ("duplicate" in msg and _has_duplicates(st))):
                            continue
                        failures.append(f"{label}: plan refused: {msg}")
                        continue
                    ran.add(label)
                    bad = _describe_mismatch(T.plan_describe(v), want_desc) if st.nnz else ""
                    if bad:
                        failures.append(f"{label}: plan is not the one asked for: {bad}")
                    for case, d_x, exp, _, _ in d.cases:
                        y0, y1 = d.run_twice(capi, T, v, d_x)
                        if not np.array_equal(y0.view(np.uint32), y1.view(np.uint32)):
                            rows = np.flatnonzero(y0.view(np.uint32) != y1.view(np.uint32))
                            failures.append(f"{label}/{case}: {rows.size} rows unwritten, first {rows[:4].tolist()}")
                            continue
                        bad = _mismatches(y0, exp)
                        if bad:
                            failures.append(f"{label}/{case}: {bad}")
                finally:
                    T.close()
    return failures, ran


@pytest.mark.parametrize("form", ["plain", "shuffled"])
@pytest.mark.parametrize("name", E.MATRICES)
def test_every_path_multiplies_by_the_transpose_exactly(pkg, oracle, gpu, monkeypatch, name, form):
    s = E.structure(name, pkg, oracle)
    if form == "shuffled":
        s = E.shuffled(s, name)[0]
    st, _, problems = _exact_on_T(s, f"{name}/{form}")
    failures, ran = _run_paths_on_T(pkg, monkeypatch, gpu, s, st, problems)
    assert not failures, f"{name}/{form}: {len(failures)} failing path(s):\n" + "\n".join(failures)
    assert {p[0] for p in PATHS} - ran <= {"xskip"}, "a path was left out"


def test_xskip_plans_on_the_transpose_of_an_unsorted_matrix(pkg, gpu, monkeypatch):
    """T's rows are always sorted: SPMV_XSKIP refuses an unsorted duplicate-free A and runs its transpose, exactly."""
    capi = pkg.capi
    rng = np.random.Generator(np.random.PCG64(21))
    rows, cols, per = 3000, 2000, 12                                   # 2 output blocks x 3000 inputs: inside the table limit
    rp = np.arange(rows + 1, dtype=np.int32) * per
    ci = np.concatenate([rng.permutation(rng.choice(cols, size=per, replace=False)) for _ in range(rows)]).astype(np.int32)
    s = E.Structure(rows, cols, rp, ci)
    assert not _has_duplicates(s) and np.any(np.diff(ci.reshape(rows, per), axis=1) < 0)
    st, _, problems = _exact_on_T(s, "xskip_unsorted")
    assert not _has_duplicates(st)
    A = capi.CsrMatrix.from_host(rows, cols, rp, ci, problems[0][1])
    with pytest.raises(capi.SpmvError) as e:
        A.plan(capi.XSKIP)
    assert e.value.status == capi.ERR_INVALID and "do not ascend" in str(e.value)
    A.close()
    failures, ran = _run_paths_on_T(pkg, monkeypatch, gpu, s, st, problems)
    assert not failures, "\n".join(failures)
    assert "xskip" in ran


# ---- 5. SpMM on T -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_powerlaw", "wave_pipe_thresholds", "wide_matrix_few_rows"])
def test_spmm_on_the_transpose(pkg, oracle, gpu, name):
    import torch
    capi = pkg.capi
    s = E.shuffled(E.structure(name, pkg, oracle), name)[0]
    st, ex, problems = _exact_on_T(s, name + "/spmm")
    A = capi.CsrMatrix.from_host(s.rows, s.cols, s.rp, s.ci, problems[0][1])
    T = A.transpose()
    T.spmm_plan()
    rng = np.random.Generator(np.random.PCG64(5))
    empty = np.diff(s.rp) == 0
    for k in (1, 4, 17):
        M = rng.integers(-4, 5, size=(st.cols, k)).astype(np.int64)
        X = M.astype(np.float32)
        X[empty] = np.nan
        want = np.stack([ex.expected(ex.int_sums(m=M[:, c])) for c in range(k)], axis=1)
        dX = torch.from_numpy(X).to(gpu)
        dY = torch.full((st.rows, k), float("nan"), dtype=torch.float32, device=gpu)
        T.spmm(dX, dY)
        torch.cuda.synchronize()
        got = dY.cpu().numpy()
        for c in range(k):
            assert _mismatches(got[:, c], want[:, c]) == "", f"{name} k={k} column {c}: {_mismatches(got[:, c], want[:, c])}"
    T.close()
    A.close()


# ---- 6. values refresh ----------------------------------------------------------------------------------------------------
def _refresh_problem(pkg, oracle, gpu, name="c2_uniform"):
    """A borrowing parent with Exact data on T, T with its map, and a function that rewrites A's vals in place with new
    Exact data (another seed) and returns what T's vals and y must then be."""
    import torch
    s = E.shuffled(E.structure(name, pkg, oracle), name)[0]
    t_rp, t_ci, _, perm = host_transpose(s.rows, s.cols, s.rp, s.ci, np.zeros(s.nnz, np.float32))
    st = E.Structure(s.cols, s.rows, t_rp, t_ci)
    d_rp, d_ci, d_va = _upload(gpu, s.rp, s.ci, np.zeros(s.nnz, np.float32))

    def rewrite(seed):
        ex = E.Exact(st, f"{name}/refresh{seed}")
        va = np.empty(s.nnz, np.float32)
        va[perm] = ex.vals()
        d_va.copy_(torch.from_numpy(va).to(gpu))                      # in place: the handle borrows this tensor
        return ex.vals(), torch.from_numpy(ex.x()).to(gpu), ex.expected()

    return s, st, (d_rp, d_ci, d_va), rewrite


def _run(T, v, d_x, rows, gpu):
    import torch
    y = torch.full((rows,), float("nan"), dtype=torch.float32, device=gpu)
    T.run(v, d_x, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_transpose_values_follows_rewritten_values(pkg, oracle, gpu):
    capi = pkg.capi
    s, st, arrays, rewrite = _refresh_problem(pkg, oracle, gpu)
    vt, d_x, want = rewrite(0)
    A = capi.CsrMatrix.from_device(s.rows, s.cols, *arrays)
    T = A.transpose(keep_map=True)
    assert T.transpose_map_bytes() == 4 * s.nnz
    plain = A.transpose()
    assert plain.transpose_map_bytes() == 0
    assert _same(T.download(), (st.rp, st.ci, vt)) == ""
    T.plan(capi.TILED)
    T.plan_set(capi.PANEL, [capi.PANEL, 0, 0, 0, 0, 0, 1, 0])
    for v in (capi.TILED, capi.PANEL):
        assert _mismatches(_run(T, v, d_x, st.rows, gpu), want) == ""
    vt, d_x, want = rewrite(1)
    T.transpose_values(A)
    assert _same(T.download(), (st.rp, st.ci, vt)) == "", "the refreshed values are not numpy's"
    assert _mismatches(_run(T, capi.TILED, d_x, st.rows, gpu), want) == "", "a TILED plan made before the refresh"
    with pytest.raises(capi.SpmvError) as e:
        _run(T, capi.PANEL, d_x, st.rows, gpu)
    assert e.value.status == capi.ERR_STALE_PLAN
    T.plan(capi.PANEL)
    assert _mismatches(_run(T, capi.PANEL, d_x, st.rows, gpu), want) == ""
    # refusals: no map, wrong shape, null
    other = capi.CsrMatrix.from_host(3, 3, np.asarray([0, 1, 1, 2], np.int32), np.asarray([0, 2], np.int32), np.ones(2, np.float32))
    for bad_t, bad_a in ((plain, A), (A, T), (T, other)):
        with pytest.raises(capi.SpmvError) as e:
            bad_t.transpose_values(bad_a)
        assert e.value.status == capi.ERR_INVALID and "spmv_csr_transpose_values" in str(e.value)
    assert capi.lib().spmv_csr_transpose_values(T._h, None, None) == capi.ERR_INVALID
    assert _same(T.download(), (st.rp, st.ci, vt)) == "", "a refused call changed the values"
    for h in (other, plain, T, A):
        h.close()


def test_transpose_values_in_a_graph(pkg, oracle, gpu):
    """transpose_values and a TILED run captured together; replayed after another in-place rewrite: the newest y."""
    import torch
    capi = pkg.capi
    s, st, arrays, rewrite = _refresh_problem(pkg, oracle, gpu, "c4_band4096")
    _, d_x0, want = rewrite(0)
    A = capi.CsrMatrix.from_device(s.rows, s.cols, *arrays)
    T = A.transpose(keep_map=True)
    T.plan(capi.TILED)
    d_x = d_x0.clone()
    y = torch.full((st.rows,), float("nan"), dtype=torch.float32, device=gpu)
    T.transpose_values(A)                                             # warm (module load) outside the capture
    T.run(capi.TILED, d_x, y)
    torch.cuda.synchronize()
    assert _mismatches(y.cpu().numpy(), want) == ""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        T.transpose_values(A)
        T.run(capi.TILED, d_x, y)
    for seed in (1, 2):
        _, d_xn, want = rewrite(seed)
        d_x.copy_(d_xn)
        y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert _mismatches(y.cpu().numpy(), want) == "", f"replay {seed}"
    del g
    T.close()
    A.close()


# ---- 7. real values at size -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,band", [("c2", 8192), ("c2", 0), ("c3", 8192), ("c3", 0)])
def test_real_values_at_full_size(pkg, oracle, gpu, cfg, band):
    import torch
    capi = pkg.capi
    w = pkg.workloads.config(cfg, band=band)
    prob = synth_problem(pkg, oracle, gpu, w)
    t_rp, t_ci, t_va, _ = host_transpose(w.rows, w.cols, prob.row_ptr, prob.col_idx, prob.vals)
    T = prob.A.transpose()
    u = oracle.synth_x(w.seed + 1, 0, w.rows)
    d_u = torch.from_numpy(u).to(gpu)
    y64, mag = oracle.spmv_f64(t_rp, t_ci, t_va, u)
    y_seq = oracle.spmv(t_rp, t_ci, t_va, u)
    for v in (capi.AUTO, capi.SCALAR):
        T.plan(v)
        y = _run(T, v, d_u, T.rows, gpu)
        assert_close_to_oracle(y, y64, mag, f"{cfg} band {band} variant {v} on T")
        if v == capi.SCALAR:
            assert np.array_equal(y.view(np.uint32), y_seq.view(np.uint32)), "SPMV_SCALAR on T is not the sequential sum"
    T.close()
    prob.A.close()


# ---- 8. config 4 at full size, expectation by torch on the device -----------------------------------------------------------
@pytest.mark.parametrize("band", [8192, 0])
def test_config4_against_torch_stable_sort(pkg, gpu, band):
    import torch
    capi, W = pkg.capi, pkg.workloads
    w = W.config("c4", band=band)
    rp = W.row_ptr(w)
    nnz = int(rp[-1])
    d_rp = torch.from_numpy(rp).to(gpu)
    d_ci = torch.empty(nnz, dtype=torch.int32, device=gpu)
    d_va = torch.empty(nnz, dtype=torch.float32, device=gpu)
    capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
    A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
    T = A.transpose(keep_map=True)
    assert T.transpose_map_bytes() == 4 * nnz
    # the expectation: torch's stable sort
    perm = torch.sort(d_ci.long(), stable=True).indices
    row_of = torch.repeat_interleave(torch.arange(w.rows, dtype=torch.int32, device=gpu), torch.from_numpy(np.diff(rp)).to(gpu))
    e_ci = row_of[perm].contiguous()
    del row_of
    e_va = d_va[perm].contiguous()
    e_rp_host = np.concatenate([[0], np.cumsum(torch.bincount(d_ci.long(), minlength=w.cols).cpu().numpy())]).astype(np.int32)
    t_rp_host = np.empty(w.cols + 1, np.int32)
    capi.check(capi.lib().spmv_csr_download(T._h, t_rp_host.ctypes.data, 0, 0))
    assert np.array_equal(t_rp_host, e_rp_host), "t.row_ptr is not cumsum(bincount(col_idx))"
    e_rp = torch.from_numpy(e_rp_host).to(gpu)
    R = capi.CsrMatrix.from_device(w.cols, w.rows, e_rp, e_ci, e_va)
    u = torch.empty(w.rows, dtype=torch.float32, device=gpu)
    capi.synth_x(w.seed, 0, w.rows, u)
    ones = torch.ones(w.rows, dtype=torch.float32, device=gpu)

    def compare(tag):
        for h in (T, R):
            h.plan(capi.SCALAR)
        for what, x in (("synthetic u", u), ("u = 1", ones)):
            yt = torch.full((w.cols,), float("nan"), dtype=torch.float32, device=gpu)
            yr = torch.full((w.cols,), float("nan"), dtype=torch.float32, device=gpu)
            T.run(capi.SCALAR, x, yt)
            R.run(capi.SCALAR, x, yr)
            torch.cuda.synchronize()
            n = int((yt.view(torch.int32) != yr.view(torch.int32)).sum().item())
            assert n == 0, f"band {band}, {tag}, {what}: {n} rows of SPMV_SCALAR on T differ from the torch-built handle's"

    compare("as built")
    T.plan(capi.AUTO)
    R.plan(capi.AUTO)
    assert T.plan_describe(capi.AUTO) == R.plan_describe(capi.AUTO)
    if band:
        assert T.plan_params(capi.AUTO)[0] == capi.TILED, f"a band stays a band: {T.plan_describe(capi.AUTO)}"
    # A's values rewritten in place, then the refresh
    d_va.mul_(-0.75).add_(0.125)
    e_va.copy_(d_va[perm])
    T.transpose_values(A)
    compare("after transpose_values")
    for h in (R, T, A):
        h.close()


# ---- 9. memory ------------------------------------------------------------------------------------------------------------
def test_memory_comes_back(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    s = E.structure("c2_uniform", pkg, oracle)
    va = np.ones(s.nnz, np.float32)
    x = torch.ones(s.rows, dtype=torch.float32, device=gpu)
    y = torch.empty(s.cols, dtype=torch.float32, device=gpu)
    free = []
    for _ in range(4):
        A = capi.CsrMatrix.from_host(s.rows, s.cols, s.rp, s.ci, va)
        T = A.transpose(keep_map=True)
        T.plan(capi.AUTO)
        T.run(capi.AUTO, x, y)
        torch.cuda.synchronize()
        T.close()
        A.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_multiplies_by_the_transpose(pkg, gpu, tmp_path):
    import scipy.io
    import scipy.sparse as sp
    rng = np.random.Generator(np.random.PCG64(6))
    A = (sp.random(5000, 7000, density=0.002, random_state=rng, dtype=np.float64) +
         sp.diags(rng.uniform(-1, 1, 5000), 0, shape=(5000, 7000))).tocsr()
    mtx = tmp_path / "A.mtx"
    scipy.io.mmwrite(str(mtx), A, symmetry="general")
    out = tmp_path / "z.txt"
    r = subprocess.run([str(pkg.capi.TESTER_PATH), "--mtx", str(mtx), "--transpose", "--variant", "tiled", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "========== OK ===========" in r.stdout
    z = np.loadtxt(out, dtype=np.float64)
    At = A.astype(np.float32).astype(np.float64).T
    ref = At @ np.ones(5000)
    mag = abs(At) @ np.ones(5000)
    assert z.shape == (7000,) and np.all(np.abs(z - ref) <= 1e-5 * mag + 1e-30)
