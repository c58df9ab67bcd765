"""CPU: the formula matrices of tests/_limits.py and the machinery that computes their expected y.

At scale 1/64 every case fits the host.  Three independent evaluations must agree exactly: torch (on the CPU here, in
slabs small enough that every case crosses many slab boundaries) fills the arrays and computes the expectation, as the
GPU tests do at full size; numpy recomputes the pinned rows from the formulas alone; and the CPU oracle multiplies the
arrays torch filled (oracle.spmv_f64) beside a plain int64 sum of them.  The full-size cases are checked for the sizes
they are built to have, and for what the giant tests can see and smaller ones cannot: the nonzeros a 32-bit c * chunk
would select past 2^29 / 2^30 give a different row sum."""
import numpy as np
import pytest

import _limits as L


def test_full_size_cases_meet_their_conditions():
    L.check_sizes()
    for n in "ABCDEFG":
        c = L.case(n)
        rows = np.asarray([0, 1, c.rows // 2, c.rows - 2, c.rows - 1], np.int64)
        assert np.array_equal(c.start(rows + 1) - c.start(rows), c.length(rows)), n
        assert int(c.start(np.asarray([0], np.int64))[0]) == 0
        for k in (0, min(1 << 29, c.nnz // 2), c.nnz - 1):
            r = c.row_of(k)
            b, e = (int(v) for v in c.start(np.asarray([r, r + 1], np.int64)))
            assert b <= k < e, (n, k, r)
    f = L.case("F")
    assert f.length(np.arange(f.rows - 65536, f.rows, dtype=np.int64)).min() >= 1
    assert f.length(np.arange(0, 64, dtype=np.int64)).min() == 0


@pytest.mark.parametrize("name", "ABCDEFG")
def test_expectation_machinery_at_scale(oracle, name):
    import torch
    c = L.case(name, scaled=True)
    b = L.build(c, torch, torch.device("cpu"), slab=(1 << 20) + 77)
    rp, ci, va, x = b.rp.numpy(), b.ci.numpy(), b.va.numpy(), b.x.numpy()
    exp = b.exp.numpy()
    assert rp[0] == 0 and rp[-1] == c.nnz and np.all(np.diff(rp.astype(np.int64)) >= 0)
    assert 0 <= ci.min() == b.col_min and ci.max() == b.col_max < c.cols
    assert np.abs(va).min() >= 1 and np.abs(va).max() <= 4 and np.array_equal(va, np.rint(va))
    if c.nnz <= 1 << 26:                                                    # the arrays are the formulas', by numpy
        hrp, hci, hva = L.host_arrays(c)
        assert np.array_equal(hrp, rp) and np.array_equal(hci, ci) and np.array_equal(hva, va.astype(np.int64))
    # unreferenced x is NaN, referenced x is the formula
    refd = np.zeros(c.cols, bool)
    refd[ci] = True
    assert np.isnan(x[~refd]).all() and np.array_equal(x[refd], c.x(np.flatnonzero(refd).astype(np.int64)).astype(np.float32))
    # the exact int64 sum on the host and the fp64 oracle of the arrays
    p = va.astype(np.int64) * x[ci].astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(p)])
    want = cs[rp[1:].astype(np.int64)] - cs[rp[:-1].astype(np.int64)]
    mag = np.concatenate([[0], np.cumsum(np.abs(p))])
    assert (mag[rp[1:].astype(np.int64)] - mag[rp[:-1].astype(np.int64)]).max() < L.EXACT_LIMIT
    assert np.array_equal(exp.astype(np.int64), want) and np.array_equal(exp, want.astype(np.float32))
    y64, _ = oracle.spmv_f64(rp, ci, va, x)
    assert np.array_equal(y64, want.astype(np.float64)), "oracle.spmv_f64 differs from the torch expectation"
    # numpy from the formulas alone, on the pinned rows
    rows = L.pinned_rows(c)
    assert np.array_equal(L.host_rows(c, rows), want[rows])
    # the SpMM columns: column 0 is x; every column against numpy on the pinned rows and the oracle on all rows
    expX = L.expected_columns(b, torch, 0, 3, slab=(1 << 19) + 5).numpy()
    assert np.array_equal(expX[:, 0], exp)
    assert np.array_equal(L.host_rows(c, rows[:4096], columns=3), expX[rows[:4096]].astype(np.int64))
    for cc in (1, 2):
        xc = np.zeros(c.cols, np.float32)
        xc[refd] = c.xcol(np.flatnonzero(refd).astype(np.int64), cc)
        y64, _ = oracle.spmv_f64(rp, ci, va, xc)
        assert np.array_equal(y64, expX[:, cc].astype(np.float64))


def _wrapped_sum(c, r, k_true, chunk):
    """The sum of row r if the nonzeros of the chunk that holds k_true were fetched from int32(c * chunk) instead."""
    b, e = (int(v) for v in c.start(np.asarray([r, r + 1], np.int64)))
    k = np.arange(b, e, dtype=np.int64)
    cn = k // chunk
    base32 = (cn * chunk + (1 << 31)) % (1 << 32) - (1 << 31)              # c * chunk in 32-bit arithmetic
    base_bytes = (base32 * 4 + (1 << 31)) % (1 << 32) - (1 << 31)          # ... and as a signed 32-bit BYTE offset
    t = np.arange(e - b, dtype=np.int64)
    col = c.col(np.full(e - b, r, np.int64), t)
    right = int((c.val(k) * c.x(col)).sum())
    out = {}
    for tag, kk in (("index", base32 + k % chunk), ("bytes", base_bytes // 4 + k % chunk)):
        kk = kk % c.nnz                                                    # (inside the array: wrong nonzeros, finite numbers)
        out[tag] = int((c.val(kk) * c.x(col)).sum())
    return right, out


@pytest.mark.parametrize("name", "AB")
def test_a_wrapped_chunk_offset_changes_the_row_sums(name):
    """What the (int64_t) casts of c * chunk in kernels_adaptive.hip and plan_adaptive.hip protect: past 2^29 nonzeros a signed
    32-bit byte offset wraps, past 2^30 an unsigned one does.  The wrapped offset selects other nonzeros of the same valid array,
    whose formula values give another row sum -- wrong, finite, and invisible to every test below 2^29 nonzeros."""
    c = L.case(name)
    for chunk in (4096, 8192, 16384):
        differ = 0
        for k in ((1 << 29) + 5 * chunk, (1 << 30) + 5 * chunk, c.nnz - 1):
            right, wrong = _wrapped_sum(c, c.row_of(k), k, chunk)
            differ += wrong["bytes"] != right
        assert differ >= 2, (name, chunk)
    # below 2^29 nothing wraps: the same evaluation returns the right sum, which is why the scaled cases cannot see it
    s = L.case(name, scaled=True)
    right, wrong = _wrapped_sum(s, s.row_of(s.nnz - 1), s.nnz - 1, 4096)
    assert wrong["index"] == right and wrong["bytes"] == right
