"""tests/_tiled_order.py, the numpy statement of the TILED order of sums, checked on the host: against exact integer sums,
against the fp64 oracle bound, and that the test problems of tests/test_gpu_tiled_rowsums.py hold what they are there for
and tell one order of the additions from another."""
import numpy as np
import pytest

import _tiled_order as TO
from _util import RTOL

BLOCKS = (256, 512, 1024)


def _rowwise(rp, a, dtype):
    out = np.zeros(len(rp) - 1, dtype)
    nz = np.flatnonzero(np.diff(rp) > 0)
    out[nz] = np.add.reduceat(a.astype(dtype), rp[:-1][nz].astype(np.int64))
    return out


@pytest.mark.parametrize("case", TO.CASES)
@pytest.mark.parametrize("block", BLOCKS)
def test_integer_products_sum_exactly(case, block):
    """Small integers: every partial sum is exact in fp32, so any correct order gives the int64 row sums."""
    P = TO.problem(case, block)
    rng = np.random.default_rng(5)
    prod = rng.integers(-64, 65, P.nnz).astype(np.float32)
    y, carry, _ = TO.tiled_spmv(P.rp, prod, 16 * block)
    exact = _rowwise(P.rp, prod, np.int64)
    assert np.array_equal(y.astype(np.int64), exact) and np.all(y == np.round(y))


@pytest.mark.parametrize("case", TO.CASES)
@pytest.mark.parametrize("block", BLOCKS)
def test_general_products_meet_the_oracle_bound(case, block):
    P = TO.problem(case, block)
    y, _, _ = P.want(16 * block)
    fin = np.isfinite(_rowwise(P.rp, P.prod, np.float64))
    y64 = _rowwise(P.rp, np.where(np.isfinite(P.prod), P.prod, 0), np.float64)
    mag = _rowwise(P.rp, np.where(np.isfinite(P.prod), np.abs(P.prod), 0), np.float64)
    err = np.abs(y.astype(np.float64) - y64)
    assert np.all(err[fin] <= RTOL * mag[fin] + 1e-37)
    # the rows that hold an Inf are that Inf, the rows of -0.0 products are +0 (every sum starts from +0)
    for r, kind in P.special.items():
        want = {"negzero": np.float32(0.0), "posinf": np.float32(np.inf), "neginf": np.float32(-np.inf)}[kind]
        assert y[r].view(np.uint32) == want.view(np.uint32), (r, kind, y[r])
        assert np.isfinite(y[r + 1])
    assert not np.isnan(y).any()


@pytest.mark.parametrize("block", BLOCKS)
def test_the_problems_hold_their_cases(block):
    T = 16 * block
    L = TO.problem("lengths", block)
    # every length of the lists at every phase 0..33 of its first word
    lb = TO.chunk_rows(L.rp, (L.nnz + T - 1) // T, T)
    start = L.rp[:-1].astype(np.int64) % T % 32
    for ln in TO.EDGE + TO.BATCH + TO.WIDE:
        rows = np.flatnonzero(np.asarray(L.lengths) == ln)
        assert len(set(start[rows])) == 32, (ln, sorted(set(start[rows])))
    assert all(n > 0 for n in L.want(T)[2])
    C = TO.problem("chunks", block)
    nchunks = (C.nnz + T - 1) // T
    lb = TO.chunk_rows(C.rp, nchunks, T)
    segs = np.diff(lb) + 1                       # segments of a chunk: the head and the rows that begin in it
    # chunks with one, two and three trips of `block` lanes over their segments; block - 1, block, block + 1, 2 block + 3 rows
    for nr in (block - 1, block, block + 1, 2 * block + 3):
        assert nr + 1 in segs, nr
    assert C.nnz % T == 3
    # a row that is a whole chunk; a row with two carried pieces; more 16-lane segments in a chunk than one round of groups
    assert T in C.lengths and np.any(C.rp[:-1][np.asarray(C.lengths) == T] % T == 0)
    reach = (C.rp[1:].astype(np.int64) - 1) // T - C.rp[:-1].astype(np.int64) // T
    assert reach.max() >= 2
    long_per_chunk = np.zeros(nchunks, int)
    for r in np.flatnonzero((np.asarray(C.lengths) > TO.SHORT) & (np.asarray(C.lengths) <= TO.HUGE) & (reach == 0)):
        long_per_chunk[C.rp[r] // T] += 1
    assert long_per_chunk.max() > block // 16 and np.any((long_per_chunk > 0) & (long_per_chunk < block // 16))


def test_the_data_tells_the_orders_apart():
    """A plain left-to-right sum of the 16-lane and wavefront segments, or a tree taken in the other direction, changes bits."""
    P = TO.problem("lengths", 512)
    y, _, _ = P.want(8192)
    seq = np.zeros(P.rows, np.float32)
    for r in range(P.rows):
        acc = np.float32(0)
        for v in P.prod[P.rp[r]:P.rp[r + 1]]:
            acc = np.float32(acc + v)
        seq[r] = acc
    ln = np.asarray(P.lengths)
    whole = (P.rp[:-1] // 8192) == ((P.rp[1:] - 1) // 8192)          # rows inside one chunk
    short = whole & (ln <= TO.SHORT)
    # a short segment is the left-to-right sum (the pad words add +0); most longer ones are not
    assert np.array_equal(y[short].view(np.uint32), (seq[short] + np.float32(0)).view(np.uint32))
    longer = whole & (ln > TO.SHORT)
    assert np.mean(y[longer] != seq[longer]) > 0.5
    old_tree = TO._tree

    def reversed_tree(a, first):
        o = 1
        while o <= first:
            a[:-o:2 * o] = a[:-o:2 * o] + a[o::2 * o]
            o *= 2
        return a[0]
    TO._tree = reversed_tree
    try:
        y2, _, _ = TO.tiled_spmv(P.rp, P.prod, 8192)
    finally:
        TO._tree = old_tree
    assert np.mean(y2[longer] != y[longer]) > 0.3
