"""The contract of spmv_csr_spgemm (include/spmv_hip.h "the sparse product") in numpy, and the matrices its tests share.

C = A B for two CSR matrices.  Row i of C lists, once each and ascending, every column j that occurs in a row b[col] for some
col among row i's entries of A: structural, whatever the values are.  The value of (i, j) is one fma chain from +0 over its
terms -- every pair (s, q) with s a storage position of A's row i, q a storage position of B's row a.col_idx[s] and
b.col_idx[q] == j -- in ascending s and, inside one s, ascending q; the fma is the correctly rounded one of
tests/_attention_order.py.  `products` is the number of terms.

`wrong=` gives the same pattern with the chain in another order: "q_outer" (ascending q, inside one q ascending s) and
"s_desc" (descending s, inside one s ascending q).  A NaN compares as a NaN: its sign and payload are the hardware's.
"""
import functools

import numpy as np

from _attention_order import fma

f32, f64 = np.float32, np.float64
WRONG = ("q_outer", "s_desc")


def terms(a, b):
    """Every term of the product in the contract's order (row, s, q): arrays row, s, q (storage positions in a and in b)."""
    a_rp, a_ci = np.asarray(a[0], np.int64), np.asarray(a[1], np.int64)
    b_rp = np.asarray(b[0], np.int64)
    rows = len(a_rp) - 1
    row_of_s = np.repeat(np.arange(rows, dtype=np.int64), np.diff(a_rp))
    blen = (b_rp[a_ci + 1] - b_rp[a_ci]) if a_ci.size else np.zeros(0, np.int64)
    s = np.repeat(np.arange(a_ci.size, dtype=np.int64), blen)
    first = np.cumsum(blen) - blen                                  # the first term of every s
    q = np.arange(int(blen.sum()), dtype=np.int64) - np.repeat(first, blen) + np.repeat(b_rp[a_ci], blen)
    return row_of_s[s], s, q


def spgemm(a, b, wrong=None):
    """(row_ptr int32, col_idx int32, vals float32, products) of a @ b; a, b = (row_ptr, col_idx, vals)."""
    assert wrong is None or wrong in WRONG
    rows = len(a[0]) - 1
    a_va, b_ci, b_va = np.asarray(a[2], f32), np.asarray(b[1], np.int64), np.asarray(b[2], f32)
    row, s, q = terms(a, b)
    products = int(row.size)
    if products == 0:
        return np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, f32), 0
    col = b_ci[q]
    inner = {None: (q, s), "q_outer": (s, q), "s_desc": (q, -s)}[wrong]          # lexsort: the last key is the primary one
    order = np.lexsort(inner + (col, row))
    row, col, s, q = row[order], col[order], s[order], q[order]
    new = np.concatenate([[True], (row[1:] != row[:-1]) | (col[1:] != col[:-1])])
    start = np.flatnonzero(new)
    entry = np.cumsum(new) - 1                                      # the entry of C a term belongs to
    rank = np.arange(products) - start[entry]                       # its place in the entry's chain
    av, bv = a_va[s], b_va[q]
    acc = np.zeros(start.size, f32)
    for k in range(int(rank.max()) + 1):
        t = np.flatnonzero(rank == k)
        acc[entry[t]] = fma(av[t], bv[t], acc[entry[t]])
    counts = np.bincount(row[start], minlength=rows)
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp, col[start].astype(np.int32), acc, products


def same(got, want):
    """None, or what differs first: row_ptr and col_idx equal, vals equal as uint32 except that a NaN matches any NaN."""
    for name, g, w in zip(("row_ptr", "col_idx"), got[:2], want[:2]):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"{name} has {g.size} entries, expected {w.size}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            return f"{name} differs at {bad.size} places, first {bad[:4].tolist()}: {g[bad[:4]]} != {w[bad[:4]]}"
    g, w = np.ascontiguousarray(got[2], f32), np.ascontiguousarray(want[2], f32)
    if g.shape != w.shape:
        return f"vals has {g.size} entries, expected {w.size}"
    bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w)))
    if bad.size:
        return f"vals differs at {bad.size} places, first {bad[:4].tolist()}: {g[bad[:4]]!r} != {w[bad[:4]]!r}"
    return None


def differs(x, y):
    """How many values of two results with one pattern differ in their bits (NaN against NaN does not count)."""
    g, w = np.asarray(x[2], f32), np.asarray(y[2], f32)
    return int(np.count_nonzero((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))))


def naive_dense(m, n, p, a, b):
    """The triple loop over dense float64 operands: (pattern bool m x p, values float64, sum of |terms| float64).  A stored
    entry counts whatever its value; a repeated column adds."""
    def dense(rows, cols, mat):
        rp, ci, va = mat
        D, A, S = np.zeros((rows, cols), f64), np.zeros((rows, cols), f64), np.zeros((rows, cols), bool)
        for r in range(rows):
            for k in range(int(rp[r]), int(rp[r + 1])):
                D[r, ci[k]] += f64(va[k])
                A[r, ci[k]] += abs(f64(va[k]))
                S[r, ci[k]] = True
        return D, A, S
    Da, Aa, Sa = dense(m, n, a)
    Db, Ab, Sb = dense(n, p, b)
    pat, val, mag = np.zeros((m, p), bool), np.zeros((m, p), f64), np.zeros((m, p), f64)
    for i in range(m):
        for j in range(p):
            for k in range(n):
                if Sa[i, k] and Sb[k, j]:
                    pat[i, j] = True
                    val[i, j] += Da[i, k] * Db[k, j]
                    mag[i, j] += Aa[i, k] * Ab[k, j]
    return pat, val, mag


# ---- the matrices of the tests (host arrays: (rows, cols, (row_ptr, col_idx, vals))) --------------------------------------------
def spread(rng, n):
    """Values whose sums show their order: mantissas in [1, 2), exponents spread over 2^20, both signs."""
    m = 1.0 + rng.integers(0, 4096, n) / 4096.0
    return (np.ldexp(m, rng.integers(-10, 11, n)) * rng.choice([-1.0, 1.0], n)).astype(f32)


def from_rows(cols, rows_of_columns, rng, values=spread):
    lengths = [len(r) for r in rows_of_columns]
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows_of_columns] + [np.zeros(0, np.int64)]).astype(np.int32)
    return len(lengths), cols, (rp, ci, values(rng, int(rp[-1])))


def random_matrix(rng, rows, cols, max_len, repeats=True):
    """Unsorted rows of 0 .. max_len entries; with `repeats` about a sixth of the entries repeat a column of their row."""
    out = []
    for _ in range(rows):
        n = int(rng.integers(0, max_len + 1)) if cols else 0
        c = rng.integers(0, max(cols, 1), n)
        if repeats and n > 1:
            dup = rng.random(n) < 1 / 6
            c = np.where(dup, c[rng.integers(0, n, n)], c)
        out.append(c)
    return from_rows(cols, out, rng)


@functools.lru_cache(maxsize=None)
def generic_case():
    rng = np.random.default_rng(2601)
    return random_matrix(rng, 257, 193, 40), random_matrix(rng, 193, 300, 40)


WIDE, UNIT = 520, 64        # edge_b: rows of 64 distinct columns each (row r: [64 r, 64 r + 64), shuffled), then rows of one column


def edge_b(rng):
    rows = [rng.permutation(np.arange(64 * r, 64 * r + 64)) for r in range(WIDE)] + [[64 * WIDE + u] for u in range(UNIT)]
    return from_rows(64 * WIDE + UNIT, rows, rng)


def edge_row(rng, bound, distinct):
    """A row of A over edge_b with `distinct` result columns (distinct // 64 wide rows, distinct % 64 unit rows) and `bound`
    terms: the others repeat wide row 0, 64 at a time, then unit row 0.  Shuffled."""
    c = list(range(distinct // 64)) + [WIDE + u for u in range(distinct % 64)]
    extra = bound - distinct
    if distinct >= 64:
        c += [0] * (extra // 64)
        extra %= 64
    assert extra == 0 or distinct % 64, (bound, distinct)
    c += [WIDE] * extra
    return rng.permutation(np.asarray(c, np.int64))


@functools.lru_cache(maxsize=None)
def edge_case(T):
    """Around class boundary T: rows with terms = distinct = T - 1, T (the full table), T + 1; terms at the edge with fewer
    distinct columns; distinct columns at the edge with more terms; short and empty rows between them.  Returns a, b and the
    (terms, distinct) of every row."""
    rng = np.random.default_rng(2700 + T)
    b = edge_b(rng)
    spec = [(0, 0), (3, 3)]
    for d in (-1, 0, 1):
        spec += [(T + d, T + d), (0, 0), (T + d, T + d - 64 if T > 64 else T + d - 3), (T + d + 64, T + d), (2, 2)]
    spec.append((0, 0))
    a = from_rows(b[0], [edge_row(rng, bd, ds) for bd, ds in spec], rng)
    return a, b, spec


@functools.lru_cache(maxsize=None)
def one_column_case(rep):
    """p = 1 under a row of A of 600 entries: every term lands on one entry; rep = 3: B's rows hold column 0 three times."""
    rng = np.random.default_rng(2800 + rep)
    b = from_rows(1, [[0] * rep for _ in range(50)], rng)
    a = from_rows(50, [rng.integers(0, 50, n) for n in (2, 600, 0, 65)], rng)
    return a, b


@functools.lru_cache(maxsize=None)
def oversized_case():
    """Between short rows: 700 entries over rows of 64 distinct columns each (44 800 distinct columns, more than any class
    holds), and 700 entries over three further rows of B that each hold the columns 0 .. 63 in an order of their own (44 800
    terms on 64 columns)."""
    rng = np.random.default_rng(2900)
    rows = [rng.permutation(np.arange(64 * r, 64 * r + 64)) for r in range(700)] + [rng.permutation(64) for _ in range(3)]
    b = from_rows(64 * 700 + 5, rows, rng)
    a = from_rows(703, [[3, 1], rng.permutation(700), [], rng.integers(700, 703, 700), [699]], rng)
    return a, b


_references = {}


def reference(key, a, b):
    """spgemm(a, b), computed once per process under `key` and left unchanged."""
    if key not in _references:
        _references[key] = spgemm(a, b)
    return _references[key]


# the inputs on which a wrong order shows in the bits (tests/test_spgemm_host.py proves it, tests/test_gpu_spgemm.py relies on it)
ORDER_CASES = {"generic": generic_case, "one_column": lambda: one_column_case(1), "one_column_repeated": lambda: one_column_case(3),
               "oversized": oversized_case}
