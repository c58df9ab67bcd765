"""spmv_csr_spmm (Y = A X, k right-hand sides, include/spmv_hip.h "SpMM") on the GPU.  What is checked:

  exact          the 21 matrices of tests/_exact.py in five forms (exact, subnormal, dilated with every unreferenced X row
                 NaN / +Inf / -Inf, non-finite, unsorted with duplicates); k in KS with ld = k, k + 3 and k rounded up to
                 4; every column of X its own integer vector, so every column of Y must equal its int64 expectation bit
                 for bit (non-finite form: per row the class of the fp64 oracle, finite rows exact).  Each case runs
                 twice, into Y filled with NaN and with a sentinel: the two agree bit for bit.  Y lies between two bands
                 of 4096 guard floats that every run must leave untouched.
  padding        Y's columns [k, ldy) keep their fill bit for bit; X's columns [k, ldx) hold NaN and change nothing.
  batch          for one plan, column c of a k = 64 run equals the k = 1 run of that column and the k = 13 run with the
                 column at another position, also with every other column NaN / Inf; two handles agree (config 3 with
                 uniform columns at full size: long rows in pieces; and an exact matrix).
  parity         configs 2 and 3 at full size, band 8192 and uniform, k = 8: every column within 1e-5 sum|terms| of the
                 fp64 oracle; config 4 band 8192 and uniform, k = 16, on host-regenerated windows of rows.
  4 GiB          X of 2^24 + 3 rows at k = 64 (4.3 GB, the first and last X rows referenced) and Y of 2^24 + 3 rows at
                 k = 64: exact, data built on the device, only the rows checked copied back.
  live values    borrowed vals rewritten in place: the next run (no re-plan) follows them exactly.
  graph          spmm captured in torch.cuda.graph after spmm_plan, replayed with new X: exact.
  refusals       k = 0 / 65, ldx < k, ldy < k, misaligned X / Y, a run before the plan: the documented status, Y untouched;
                 the capi wrapper's own checks; matrices with rows = 0, cols = 0 (Y all zero) and nnz = 0.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _exact as E
from _util import assert_close_to_oracle

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 13, 16, 31, 32, 33, 64)
KINDS = ("exact", "subnormal", "poison", "nonfinite", "unsorted")
SENTINEL = np.float32(-1.2345e30)
GUARD, GUARD_N = np.float32(3.0e35), 4096


def _lds(k):
    return sorted({k, k + 3, (k + 3) // 4 * 4})


def _bits(t):
    import torch
    return (t + 0.0).view(torch.int32)      # (+0 folds -0: an exact zero sum may carry either sign)


def _int_columns(s, k_int, M):
    """int64 sums per row of k * M[col] for every column of M (cols x n), exact through float64."""
    # (copies: scipy may sum duplicates in place, and the structures are cached)
    A = sp.csr_matrix((k_int.astype(np.float64), s.ci.copy(), s.rp.copy()), shape=(s.rows, s.cols))
    Aabs = sp.csr_matrix((np.abs(k_int).astype(np.float64), s.ci.copy(), s.rp.copy()), shape=(s.rows, s.cols))
    mag = Aabs @ np.abs(M).astype(np.float64)
    assert mag.size == 0 or mag.max() <= E.EXACT_LIMIT
    return np.rint(A @ M.astype(np.float64)).astype(np.int64)


def _columns(s, seed_name, m0):
    """64 integer x vectors in [-4, 4], column 0 = m0."""
    rng = np.random.Generator(np.random.PCG64([sum(map(ord, seed_name)), 64]))
    M = rng.integers(-4, 5, size=(s.cols, 64)).astype(np.int64)
    M[:, 0] = m0
    return M


class _Spmm:
    """One matrix on the device (a borrowing handle, planned) and the checks of one run pair."""

    def __init__(self, capi, gpu, s, vals):
        import torch
        self.gpu, self.s = gpu, s
        self.d_rp = torch.from_numpy(s.rp).to(gpu)
        self.d_ci = torch.from_numpy(s.ci).to(gpu)
        self.d_va = torch.from_numpy(np.ascontiguousarray(vals, np.float32)).to(gpu)
        self.A = capi.CsrMatrix.from_device(s.rows, s.cols, self.d_rp, self.d_ci, self.d_va)
        self.A.spmm_plan()

    def run_pair(self, X64, k, ldx, ldy):
        """X64: (cols, 64) device; runs k columns with these leading dimensions into NaN and sentinel; returns Y[:, :k]."""
        import torch
        s = self.s
        X = torch.full((s.cols, ldx), float("nan"), dtype=torch.float32, device=self.gpu)
        X[:, :k] = X64[:, :k]
        ys = []
        bufs = []
        for fill in (float("nan"), float(SENTINEL)):
            # Y 16-byte aligned (the header asks it) between two bands of GUARD_N guard floats: nothing outside Y is written
            buf = torch.full((2 * GUARD_N + s.rows * ldy,), float(GUARD), dtype=torch.float32, device=self.gpu)
            Y = buf[GUARD_N:GUARD_N + s.rows * ldy].view(s.rows, ldy)
            assert Y.data_ptr() % 16 == 0
            Y.fill_(fill)
            self.A.spmm(X[:, :k], Y[:, :k])
            ys.append(Y)
            bufs.append(buf)
        torch.cuda.synchronize()
        y0, y1 = ys
        bad = []
        for buf in bufs:
            if not (bool((buf[:GUARD_N] == float(GUARD)).all()) and bool((buf[GUARD_N + s.rows * ldy:] == float(GUARD)).all())):
                bad.append("a run wrote outside Y")
        d = (y0[:, :k].view(torch.int32) != y1[:, :k].view(torch.int32)).sum().item()
        if d:
            bad.append(f"{d} entries unwritten")
        if ldy > k:
            nan_bits = torch.tensor([float("nan")], dtype=torch.float32).view(torch.int32).item()
            sent_bits = torch.tensor([float(SENTINEL)], dtype=torch.float32).view(torch.int32).item()
            p0 = (y0[:, k:].view(torch.int32) != nan_bits).sum().item()
            p1 = (y1[:, k:].view(torch.int32) != sent_bits).sum().item()
            if p0 or p1:
                bad.append(f"padding columns written ({p0} + {p1})")
        return y0[:, :k], bad

    def close(self):
        self.A.close()


def _mismatch(y, exp):
    """Entries of y (rows x k, device) that differ from exp (same shape): NaN where exp is NaN, else the same bits."""
    import torch
    ok = torch.where(torch.isnan(exp), torch.isnan(y), _bits(y) == _bits(exp))
    return int((~ok).sum().item())


def _sweep(dev, X64, exp, label):
    """Every k of KS with every ld: the failures."""
    import torch
    failures = []
    d_exp = torch.from_numpy(np.ascontiguousarray(exp, np.float32)).to(dev.gpu)
    for k in KS:
        lds = _lds(k)
        for ldx, ldy in sorted({(ld, ld) for ld in lds} | {(lds[-1], lds[0]), (lds[0], lds[-1])}):
            y, bad = dev.run_pair(X64, k, ldx, ldy)
            n = _mismatch(y, d_exp[:, :k])
            if n:
                bad.append(f"{n} entries differ from the expectation")
            if bad:
                failures.append(f"{label} k={k} ldx={ldx} ldy={ldy}: " + "; ".join(bad))
    return failures


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", E.MATRICES)
def test_spmm_exact_every_column(pkg, oracle, gpu, name, kind):
    import torch
    capi = pkg.capi
    s = E.structure(name, pkg, oracle)
    ex = E.Exact(s, name)
    scale = lambda ints: np.ldexp(ints.astype(np.float64), ex.e[:, None]).astype(np.float32)   # noqa: E731
    failures = []
    if kind in ("exact", "subnormal", "poison"):
        M = _columns(s, name, ex.m)
        ints = _int_columns(s, ex.k, M)
        assert np.array_equal(ints[:, 0], ex.int_sums()) and np.array_equal(ints[:, 63], ex.int_sums(m=M[:, 63]))
        if kind == "subnormal":
            dev = _Spmm(capi, gpu, s, ex.sub_vals())
            X = np.ldexp(M.astype(np.float64), E.SUB_X_EXP).astype(np.float32)
            exp = np.ldexp(ints.astype(np.float64), E.SUB_VAL_EXP + E.SUB_X_EXP).astype(np.float32)
            failures += _sweep(dev, torch.from_numpy(X).to(gpu), exp, "subnormal")
        elif kind == "exact":
            dev = _Spmm(capi, gpu, s, ex.vals())
            failures += _sweep(dev, torch.from_numpy(M.astype(np.float32)).to(gpu), scale(ints), "int")
        else:
            dev = _Spmm(capi, gpu, E.dilate(s), ex.vals())
            for tag, p in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
                Xd = np.full((2 * s.cols + 1, 64), p, np.float32)
                Xd[1::2] = M
                failures += _sweep(dev, torch.from_numpy(Xd).to(gpu), scale(ints), f"poison_{tag}")
    elif kind == "unsorted":
        su, _ = E.shuffled(s, name)
        exu = E.Exact(su, name + "/unsorted")
        M = _columns(su, name + "/unsorted", exu.m)
        ints = _int_columns(su, exu.k, M)
        assert np.array_equal(ints[:, 0], exu.int_sums())
        dev = _Spmm(capi, gpu, su, exu.vals())
        exp = np.ldexp(ints.astype(np.float64), exu.e[:, None]).astype(np.float32)
        failures += _sweep(dev, torch.from_numpy(M.astype(np.float32)).to(gpu), exp, "unsorted_dup")
    else:
        vals, x0, _, _ = E.nonfinite(ex, name)
        special = ~np.isfinite(x0) | (x0 != ex.m)          # what nonfinite() set: kept in every column
        M = _columns(s, name + "/nonfinite", ex.m)
        X = np.where(special[:, None], x0[:, None], M.astype(np.float32)).astype(np.float32)
        M_int = np.where(np.isfinite(X), X, 0).astype(np.int64)
        ints = _int_columns(s, ex.k, M_int)
        exp = scale(ints)
        sd = E.dilate(s)
        Xd = np.full((2 * s.cols + 1, 64), np.nan, np.float32)
        Xd[1::2] = X
        for c in range(64):
            y64, _ = oracle.spmv_f64(sd.rp, sd.ci, vals, Xd[:, c])
            fin = np.isfinite(y64)
            exp[~fin, c] = y64[~fin].astype(np.float32)     # the class of the fp64 oracle
        dev = _Spmm(capi, gpu, sd, vals)
        failures += _sweep(dev, torch.from_numpy(Xd).to(gpu), exp, "nonfinite")
    dev.close()
    assert not failures, f"{name}/{kind}: {len(failures)} failing case(s):\n" + "\n".join(failures[:20])


# ---- batch invariance ------------------------------------------------------------------------------------------------
def _synth_device(pkg, gpu, w):
    import torch
    rp = pkg.workloads.row_ptr(w)
    nnz = int(rp[-1])
    d_rp = torch.from_numpy(rp).to(gpu)
    d_ci = torch.empty(nnz, dtype=torch.int32, device=gpu)
    d_va = torch.empty(nnz, dtype=torch.float32, device=gpu)
    pkg.capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
    torch.cuda.synchronize()
    return rp, d_rp, d_ci, d_va


def _batch_invariance(capi, gpu, rows, cols, d_rp, d_ci, d_va, X64):
    import torch
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    assert A.spmm_plan_bytes() >= 0

    def run(X, ldy=None):
        k = X.shape[1]
        Y = torch.full((rows, ldy or k), float("nan"), dtype=torch.float32, device=gpu)
        A.spmm(X, Y[:, :k])
        torch.cuda.synchronize()
        return Y[:, :k].view(torch.int32)

    Y64 = run(X64)
    assert torch.equal(run(X64), Y64), "two runs differ"
    for c in range(64):
        assert torch.equal(run(X64[:, c:c + 1].contiguous()), Y64[:, c:c + 1]), f"column {c}: k = 1 differs"
    gen = torch.Generator(device=gpu).manual_seed(13)
    for c in (0, 5, 31, 32, 63):
        pos = (c * 7 + 3) % 13
        X13 = torch.randn((cols, 16), generator=gen, device=gpu, dtype=torch.float32)[:, :13]
        X13[:, pos] = X64[:, c]
        assert torch.equal(run(X13, ldy=15)[:, pos], Y64[:, c]), f"column {c} at position {pos} of 13 differs"
        Xp = torch.full((cols, 64), float("nan"), dtype=torch.float32, device=gpu)
        Xp[:, 1::2] = float("inf")
        Xp[:, 2::4] = float("-inf")
        Xp[:, c] = X64[:, c]
        assert torch.equal(run(Xp)[:, c], Y64[:, c]), f"column {c} changes with NaN / Inf beside it"
    B = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    B.spmm_plan()
    assert B.spmm_describe() == A.spmm_describe()
    YB = torch.full((rows, 64), float("nan"), dtype=torch.float32, device=gpu)
    B.spmm(X64, YB)
    torch.cuda.synchronize()
    assert torch.equal(YB.view(torch.int32), Y64), "two handles of one matrix differ"
    d = A.spmm_describe()
    A.close()
    B.close()
    return d


def test_spmm_batch_invariance_c3_uniform_full_size(pkg, gpu):
    import torch
    w = pkg.workloads.config("c3", band=0)
    rp, d_rp, d_ci, d_va = _synth_device(pkg, gpu, w)
    gen = torch.Generator(device=gpu).manual_seed(7)
    X64 = torch.randn((w.cols, 64), generator=gen, device=gpu, dtype=torch.float32)
    d = _batch_invariance(pkg.capi, gpu, w.rows, w.cols, d_rp, d_ci, d_va, X64)
    fields = dict(t.split("=") for t in d.split())
    assert int(fields["long_rows"]) > 0 and int(fields["pieces"]) > int(fields["long_rows"]), d


def test_spmm_batch_invariance_exact_matrix(pkg, oracle, gpu):
    import torch
    s = E.structure("c3_powerlaw", pkg, oracle)
    ex = E.Exact(s, "c3_powerlaw")
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    d_va = torch.from_numpy(ex.vals()).to(gpu)
    gen = torch.Generator(device=gpu).manual_seed(11)
    X64 = torch.randn((s.cols, 64), generator=gen, device=gpu, dtype=torch.float32)
    _batch_invariance(pkg.capi, gpu, s.rows, s.cols, d_rp, d_ci, d_va, X64)


# ---- parity at size ----------------------------------------------------------------------------------------------------
def _x_columns(pkg, gpu, w, k):
    import torch
    X = torch.empty((w.cols, k), dtype=torch.float32, device=gpu)
    col = torch.empty(w.cols, dtype=torch.float32, device=gpu)
    for c in range(k):
        pkg.capi.synth_x(w.seed + 1 + c, 0, w.cols, col)
        X[:, c] = col
    torch.cuda.synchronize()
    return X


@pytest.mark.parametrize("name,band", [("c2", 8192), ("c2", 0), ("c3", 8192), ("c3", 0)])
def test_spmm_parity_c2_c3_full_size(pkg, oracle, gpu, name, band):
    import torch
    from _util import synth_problem
    w = pkg.workloads.config(name, band=band)
    prob = synth_problem(pkg, oracle, gpu, w)
    k = 8
    X = _x_columns(pkg, gpu, w, k)
    prob.A.spmm_plan()
    Y = torch.full((w.rows, k), float("nan"), dtype=torch.float32, device=gpu)
    prob.A.spmm(X, Y)
    torch.cuda.synchronize()
    Yh = Y.cpu().numpy()
    for c in range(k):
        x = oracle.synth_x(w.seed + 1 + c, 0, w.cols)
        y64, mag = oracle.spmv_f64(prob.row_ptr, prob.col_idx, prob.vals, x)
        assert_close_to_oracle(np.ascontiguousarray(Yh[:, c]), y64, mag, f"{w.name} column {c}")


@pytest.mark.parametrize("band", [8192, 0])
def test_spmm_parity_c4_row_windows(pkg, oracle, gpu, band):
    import torch
    w = pkg.workloads.config("c4", band=band)
    rp, d_rp, d_ci, d_va = _synth_device(pkg, gpu, w)
    k = 16
    X = _x_columns(pkg, gpu, w, k)
    A = pkg.capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    Y = torch.full((w.rows, k), float("nan"), dtype=torch.float32, device=gpu)
    A.spmm(X, Y)
    torch.cuda.synchronize()
    assert not torch.isnan(Y).any(), "rows left unwritten"
    xs = [oracle.synth_x(w.seed + 1 + c, 0, w.cols) for c in range(k)]
    n = 1 << 16
    for l0 in (0, 7_654_321, w.rows - n):
        l1 = l0 + n
        rps = (rp[l0:l1 + 1].astype(np.int64) - int(rp[l0])).astype(np.int32)
        ci, va = oracle.synth_fill(w.seed, l0, l1, w.rows, w.cols, w.band, rps)
        Yh = Y[l0:l1].cpu().numpy()
        for c in range(k):
            y64, mag = oracle.spmv_f64(rps, ci, va, xs[c])
            assert_close_to_oracle(np.ascontiguousarray(Yh[:, c]), y64, mag, f"c4 band {band} rows {l0}+ column {c}")
    A.close()


# ---- beyond 4 GiB ------------------------------------------------------------------------------------------------------
def _x_formula(j, c):
    """The integer X[j][c] both sides compute (j int64, c int)."""
    return ((j * 7 + c * 13) % 9) - 4


def test_spmm_x_beyond_4gib(pkg, gpu):
    import torch
    capi = pkg.capi
    cols, k, rows, per = (1 << 24) + 3, 64, 1 << 17, 4
    rng = np.random.Generator(np.random.PCG64(2024))
    ci = rng.integers(0, cols, size=(rows, per)).astype(np.int64)
    ci[0] = (0, cols - 1, cols - 2, 1)
    ci[-1] = (cols - 1, cols - 1, 0, cols - 3)       # a repeated column
    ci[1:1000, 0] = cols - 1 - rng.integers(0, 1 << 16, size=999)
    ci = ci.reshape(-1)
    va = (rng.integers(1, 5, size=ci.size) * rng.choice([-1, 1], size=ci.size)).astype(np.float32)
    rp = (np.arange(rows + 1, dtype=np.int64) * per).astype(np.int32)
    X = torch.empty((cols, k), dtype=torch.float32, device=gpu)             # 4.3 GB, built in slabs on the device
    cc = torch.arange(k, device=gpu, dtype=torch.int64)
    for j0 in range(0, cols, 1 << 20):
        j = torch.arange(j0, min(cols, j0 + (1 << 20)), device=gpu, dtype=torch.int64)[:, None]
        X[j0:j0 + j.shape[0]] = _x_formula(j, cc).to(torch.float32)
    d_rp, d_ci = torch.from_numpy(rp).to(gpu), torch.from_numpy(ci.astype(np.int32)).to(gpu)
    d_va = torch.from_numpy(va).to(gpu)
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    Y = torch.full((rows, k), float("nan"), dtype=torch.float32, device=gpu)
    A.spmm(X, Y)
    torch.cuda.synchronize()
    Xh = _x_formula(ci[:, None], np.arange(k)[None, :]).astype(np.int64)      # X rows of every nonzero
    want = (va.astype(np.int64)[:, None] * Xh).reshape(rows, per, k).sum(axis=1).astype(np.float32)
    assert np.array_equal(Y.cpu().numpy(), want)
    A.close()


def test_spmm_y_beyond_4gib(pkg, gpu):
    import torch
    capi = pkg.capi
    rows, cols, k = (1 << 24) + 3, 4096, 64
    r = torch.arange(rows, device=gpu, dtype=torch.int64)
    lengths = 1 + r % 2
    lengths[(r % 5 == 0) & (r < rows - 65536)] = 0                   # empty rows, but the last 65 536 are not
    rp = torch.zeros(rows + 1, dtype=torch.int64, device=gpu)
    rp[1:] = torch.cumsum(lengths, 0)
    nnz = int(rp[-1].item())
    n = torch.arange(nnz, device=gpu, dtype=torch.int64)
    d_ci = ((n * 2654435761) % cols).to(torch.int32)
    d_va = ((n % 7) - 3).to(torch.float32)
    d_rp = rp.to(torch.int32)
    cc = torch.arange(k, device=gpu, dtype=torch.int64)
    X = _x_formula(torch.arange(cols, device=gpu, dtype=torch.int64)[:, None], cc).to(torch.float32)
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    Y = torch.full((rows, k), float("nan"), dtype=torch.float32, device=gpu)   # 4.3 GB
    A.spmm(X, Y)
    torch.cuda.synchronize()
    rng = np.random.Generator(np.random.PCG64(99))
    sample = np.unique(np.concatenate([np.arange(65536), np.arange(rows - 65536, rows),
                                       rng.integers(0, rows, size=1 << 16)]))
    idx = torch.from_numpy(sample).to(gpu)
    got = Y[idx].cpu().numpy()
    b = rp[idx].cpu().numpy()
    e = rp[idx + 1].cpu().numpy()
    want = np.zeros((sample.size, k), np.int64)
    for t in range(2):                           # at most two nonzeros per row
        has = b + t < e
        nn = (b + t)[has]
        want[has] += ((nn % 7) - 3)[:, None] * _x_formula(((nn * 2654435761) % cols)[:, None], np.arange(k)[None, :])
    assert np.array_equal(got, want.astype(np.float32))
    A.close()


# ---- live values, graph capture -----------------------------------------------------------------------------------------
def _small_exact(pkg, oracle, gpu, name="odd_last_chunk"):
    import torch
    s = E.structure(name, pkg, oracle)
    ex = E.Exact(s, name)
    M = _columns(s, name, ex.m)[:, :24]
    dev = _Spmm(pkg.capi, gpu, s, ex.vals())
    return s, ex, M, dev, torch.from_numpy(M.astype(np.float32)).to(gpu)


def test_spmm_reads_values_live(pkg, oracle, gpu):
    import torch
    s, ex, M, dev, X = _small_exact(pkg, oracle, gpu, "c3_powerlaw")
    Y = torch.empty((s.rows, 24), dtype=torch.float32, device=gpu)
    dev.A.spmm(X, Y)
    torch.cuda.synchronize()
    want = np.ldexp(_int_columns(s, ex.k, M).astype(np.float64), ex.e[:, None]).astype(np.float32)
    assert np.array_equal(Y.cpu().numpy(), want)
    k2 = -ex.k * 2 + np.sign(ex.k)                       # new integers in place, no re-plan
    dev.d_va.copy_(torch.from_numpy(ex.vals(k2)))
    Y.fill_(float("nan"))
    dev.A.spmm(X, Y)
    torch.cuda.synchronize()
    want2 = np.ldexp(_int_columns(s, k2, M).astype(np.float64), ex.e[:, None]).astype(np.float32)
    assert np.array_equal(Y.cpu().numpy(), want2)
    dev.close()


def test_spmm_graph_capture(pkg, oracle, gpu):
    import torch
    s, ex, M, dev, X = _small_exact(pkg, oracle, gpu, "wave_pipe_thresholds")
    Xg = torch.zeros_like(X)
    Y = torch.full((s.rows, 24), float("nan"), dtype=torch.float32, device=gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.A.spmm(Xg, Y)
    Xg.copy_(X)
    g.replay()
    torch.cuda.synchronize()
    want = np.ldexp(_int_columns(s, ex.k, M).astype(np.float64), ex.e[:, None]).astype(np.float32)
    assert np.array_equal(Y.cpu().numpy(), want)
    Xg.copy_(-X)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(Y.cpu().numpy(), -want)
    dev.close()


# ---- refusals and edges ---------------------------------------------------------------------------------------------------
def test_spmm_refusals_leave_y_untouched(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    s = E.structure("many_tiny_rows", pkg, oracle)
    ex = E.Exact(s, "many_tiny_rows")
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    d_va = torch.from_numpy(ex.vals()).to(gpu)
    A = capi.CsrMatrix.from_device(s.rows, s.cols, d_rp, d_ci, d_va)
    X = torch.ones((s.cols, 72), dtype=torch.float32, device=gpu)
    Y = torch.full((s.rows, 72), float(SENTINEL), dtype=torch.float32, device=gpu)
    before = Y.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, yp = X.data_ptr(), Y.data_ptr()
    assert lib.spmv_csr_spmm(A._h, 4, xp, 72, yp, 72, st) == capi.ERR_NOT_PLANNED     # before the plan
    A.spmm_plan()
    A.spmm_plan()                                                                       # idempotent
    assert A.spmm_describe().startswith("row_cap=")
    for k, ldx, ldy, xo, yo in ((0, 72, 72, 0, 0), (65, 72, 72, 0, 0), (8, 7, 72, 0, 0), (8, 72, 7, 0, 0),
                                (8, 72, 72, 4, 0), (8, 72, 72, 0, 8)):
        rc = lib.spmv_csr_spmm(A._h, k, xp + xo, ldx, yp + yo, ldy, st)
        assert rc == capi.ERR_INVALID, (k, ldx, ldy, xo, yo, rc)
    torch.cuda.synchronize()
    assert torch.equal(Y.view(torch.int32), before.view(torch.int32))
    # the wrapper checks before it calls
    with pytest.raises(ValueError):
        A.spmm(X[:, 0], Y)                                   # not 2-D
    with pytest.raises(ValueError):
        A.spmm(X[:, :4].double(), Y)                         # not float32
    with pytest.raises(ValueError):
        A.spmm(torch.ones((4, s.cols), device=gpu).t(), Y)   # column-strided
    with pytest.raises(ValueError):
        A.spmm(X[:-1, :4], Y)                                # X rows != cols
    with pytest.raises(ValueError):
        A.spmm(X[:, :4], Y[:-1])                             # Y rows != rows
    with pytest.raises(ValueError):
        A.spmm(X[:, :8], Y[:, :4])                           # Y narrower than k
    A.close()


@pytest.mark.parametrize("rows,cols,nnz", [(0, 10, 0), (5, 0, 0), (7, 9, 0)])
def test_spmm_empty_shapes(pkg, gpu, rows, cols, nnz):
    import torch
    capi = pkg.capi
    d_rp = torch.zeros(rows + 1, dtype=torch.int32, device=gpu)
    d_ci = torch.zeros(max(nnz, 1), dtype=torch.int32, device=gpu)[:nnz]
    d_va = torch.zeros(max(nnz, 1), dtype=torch.float32, device=gpu)[:nnz]
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    for k in (1, 5, 64):
        X = torch.ones((cols, k), dtype=torch.float32, device=gpu)
        Y = torch.full((rows, k), float("nan"), dtype=torch.float32, device=gpu)
        A.spmm(X, Y)
        torch.cuda.synchronize()
        assert torch.equal(Y, torch.zeros_like(Y))
    A.close()
