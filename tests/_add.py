"""The contract of spmv_csr_add (include/spmv_hip.h "the sparse sum") in numpy, and the matrices its tests share.

C = alpha A + beta B for two CSR matrices of one shape.  Row i of C lists, once each and ascending, the columns of row i of A
or of B ("union"), of both ("intersect") or of A and not of B ("minus"): structural, whatever the values are.  The terms of
entry (i, j) are the storage positions s of A's row i with column j, ascending, then those of B's row i; a term has its side's
coefficient; the first gives fl(coef * v), every later one fma(coef, v, acc) with the correctly rounded fma of
tests/_attention_order.py.  A side whose coefficient is +0 or -0 has no terms; under "minus" B has none; an entry without
terms is +0.

`wrong=` gives the same pattern with the chain in another order: "b_first" (B's terms before A's) and "desc" (every chain
reversed).  A NaN compares as a NaN: its sign and payload are the hardware's.
"""
import functools

import numpy as np

from _attention_order import fma
from _util import RTOL  # noqa: F401  (the project's bound relative to the sum of |terms|: 1e-5, some 168 roundings of 2^-24)
from _spgemm import differs, from_rows, random_matrix, same, spread  # noqa: F401  (same / differs: re-exported for the tests)

f32, f64 = np.float32, np.float64
OPS = ("union", "intersect", "minus")
WRONG = ("b_first", "desc")


def _keys(mat, cols):
    rp, ci = np.asarray(mat[0], np.int64), np.asarray(mat[1], np.int64)
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    return row * max(cols, 1) + ci if ci.size else np.zeros(0, np.int64)


def add(a, b, alpha, beta, op, wrong=None, cols=None):
    """(row_ptr int32, col_idx int32, vals float32, kept_terms) of alpha a + beta b under op; a, b = (row_ptr, col_idx, vals).
    kept_terms: the terms the plan stores (whatever the coefficients are)."""
    assert op in OPS and (wrong is None or wrong in WRONG)
    rows = len(a[0]) - 1
    assert len(b[0]) - 1 == rows
    if cols is None:
        cols = int(max(np.max(a[1], initial=-1), np.max(b[1], initial=-1))) + 1
    alpha, beta = f32(alpha), f32(beta)
    ka, kb = _keys(a, cols), _keys(b, cols)
    ua, ub = np.unique(ka), np.unique(kb)
    entries = {"union": np.union1d(ua, ub), "intersect": np.intersect1d(ua, ub), "minus": np.setdiff1d(ua, ub)}[op]
    rp = np.concatenate([[0], np.cumsum(np.bincount(entries // max(cols, 1), minlength=rows))]).astype(np.int32)
    ci = (entries % max(cols, 1)).astype(np.int32)
    # the terms: (entry, side, position), the plan's order
    sides = [(0, ka, np.asarray(a[2], f32), alpha)] + ([(1, kb, np.asarray(b[2], f32), beta)] if op != "minus" else [])
    ent, side, pos, coef, val = [], [], [], [], []
    kept_terms = 0
    for sd, k, v, c in sides:
        e = np.searchsorted(entries, k)
        hit = (e < entries.size) & (entries[np.minimum(e, max(entries.size - 1, 0))] == k) if entries.size else np.zeros(k.size, bool)
        p = np.flatnonzero(hit)
        kept_terms += p.size
        if c == 0:                                               # +0 or -0: the pattern, no terms
            continue
        ent.append(e[p]); side.append(np.full(p.size, sd)); pos.append(p); coef.append(np.full(p.size, c, f32)); val.append(v[p])
    acc = np.zeros(entries.size, f32)
    if ent and sum(x.size for x in ent):
        ent, side, pos = np.concatenate(ent), np.concatenate(side), np.concatenate(pos)
        coef, val = np.concatenate(coef), np.concatenate(val)
        inner = {None: (pos, side), "b_first": (pos, -side), "desc": (-pos, -side)}[wrong]     # lexsort: the last key is primary
        order = np.lexsort(inner + (ent,))
        ent, coef, val = ent[order], coef[order], val[order]
        new = np.concatenate([[True], ent[1:] != ent[:-1]])
        start = np.flatnonzero(new)
        rank = np.arange(ent.size) - start[np.cumsum(new) - 1]
        with np.errstate(all="ignore"):
            for k in range(int(rank.max()) + 1):
                t = np.flatnonzero(rank == k)
                acc[ent[t]] = (coef[t] * val[t]).astype(f32) if k == 0 else fma(coef[t], val[t], acc[ent[t]])
    return rp, ci, acc, int(kept_terms)


def dense_walk(rows, cols, a, b, alpha, beta, op):
    """Dense float64: (pattern bool, values float64, sum of |coef v| float64).  A stored entry counts whatever its value."""
    def dense(mat, coef):
        rp, ci, va = mat
        D, A, S = np.zeros((rows, cols), f64), np.zeros((rows, cols), f64), np.zeros((rows, cols), bool)
        for r in range(rows):
            for k in range(int(rp[r]), int(rp[r + 1])):
                S[r, ci[k]] = True
                if coef != 0:
                    D[r, ci[k]] += f64(coef) * f64(va[k])
                    A[r, ci[k]] += abs(f64(coef) * f64(va[k]))
        return D, A, S
    Da, Aa, Sa = dense(a, f32(alpha))
    Db, Ab, Sb = dense(b, f32(beta))
    if op == "union":
        return Sa | Sb, Da + Db, Aa + Ab
    if op == "intersect":
        pat = Sa & Sb
        return pat, np.where(pat, Da + Db, 0.0), np.where(pat, Aa + Ab, 0.0)
    pat = Sa & ~Sb
    return pat, np.where(pat, Da, 0.0), np.where(pat, Aa, 0.0)


def sort_rows(mat):
    """The matrix with every row stably sorted by column."""
    rp, ci, va = (np.asarray(x) for x in mat)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    order = np.lexsort((ci, row))
    return rp, ci[order], va[order]


def sorted_matrix(rng, rows, cols, max_len, repeats=False):
    """Sorted rows of 0 .. max_len entries, duplicate-free unless `repeats`."""
    out = []
    for _ in range(rows):
        n = int(rng.integers(0, max_len + 1)) if cols else 0
        c = np.sort(rng.integers(0, cols, n)) if repeats else np.sort(rng.choice(cols, min(n, cols), replace=False))
        out.append(c)
    return from_rows(cols, out, rng)


# ---- the matrices of the tests (host arrays: (rows, cols, (row_ptr, col_idx, vals))) --------------------------------------------
@functools.lru_cache(maxsize=None)
def generic_case():
    """Two 257 x 193 matrices, unsorted rows of 0 .. 40 entries with repeats on both sides."""
    rng = np.random.default_rng(2701)
    return random_matrix(rng, 257, 193, 40), random_matrix(rng, 257, 193, 40)


@functools.lru_cache(maxsize=None)
def order_case():
    """97 x 61, unsorted rows of 0 .. 24 entries with a sixth repeated: the rows overlap enough for the order to show."""
    rng = np.random.default_rng(2702)
    return random_matrix(rng, 97, 61, 24), random_matrix(rng, 97, 61, 24)


@functools.lru_cache(maxsize=None)
def sorted_case(repeats):
    rng = np.random.default_rng(2703 + int(repeats))
    return sorted_matrix(rng, 300, 211, 30, repeats), sorted_matrix(rng, 300, 211, 30, repeats)


@functools.lru_cache(maxsize=None)
def lengths_case():
    """Row lengths 0, 1, 2, 63, 64, 65, 129 on either side against 0, 1, 64 and one row of 5000 on the other, sorted and
    duplicate-free; then identical rows, disjoint rows, interleaved columns, all of b below and above all of a."""
    rng = np.random.default_rng(2705)
    cols = 20000
    ra, rb = [], []
    pick = lambda n: np.sort(rng.choice(cols, n, replace=False))
    for la in (0, 1, 2, 63, 64, 65, 129):
        for lb in (0, 1, 64):
            ra.append(pick(la)); rb.append(pick(lb))
            ra.append(pick(lb)); rb.append(pick(la))
    for la in (0, 1, 2, 63, 64, 65, 129):
        ra.append(pick(la)); rb.append(pick(5000))
        ra.append(pick(5000)); rb.append(pick(la))
    same_row = pick(70)
    ra.append(same_row); rb.append(same_row)                                  # identical
    ra.append(np.arange(0, 200, 2)); rb.append(np.arange(1, 200, 2))          # disjoint and interleaved
    ra.append(np.arange(0, 300, 3)); rb.append(np.arange(0, 300, 2))          # interleaved with common columns
    ra.append(np.arange(1000, 1100)); rb.append(np.arange(0, 90))             # all of b below all of a
    ra.append(np.arange(0, 90)); rb.append(np.arange(1000, 1100))             # ... above
    return from_rows(cols, ra, rng), from_rows(cols, rb, rng)


SPECIAL = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF,
                    0x7F7FFFFF, 0x3F800000, 0xBF800000], np.uint32).view(f32)


@functools.lru_cache(maxsize=None)
def special_case():
    """Unsorted rows with repeats; a third of the values from SPECIAL on both sides; a last row with a cancelling pair."""
    rng = np.random.default_rng(2706)
    (m, n, a), (_, _, b) = random_matrix(rng, 70, 40, 20), random_matrix(rng, 70, 40, 20)
    def spike(mat):
        rp, ci, va = mat
        va = va.copy()
        hit = rng.random(va.size) < 1 / 3
        va[hit] = SPECIAL[rng.integers(0, SPECIAL.size, int(hit.sum()))]
        rp = np.concatenate([rp, [rp[-1] + 2]]).astype(np.int32)
        return rp, np.concatenate([ci, [5, 7]]).astype(np.int32), va
    a, b = spike(a), spike(b)
    a = (a[0], a[1], np.concatenate([a[2], f32([1.5, 2.0])]))
    b = (b[0], b[1], np.concatenate([b[2], f32([-1.5, 0.0])]))                # 1.5 + -1.5 at column 5: a cancelling pair
    return (m + 1, n, a), (m + 1, n, b)


_references = {}


def reference(key, a, b, alpha, beta, op, cols=None):
    """add(a, b, ...), computed once per process under `key` and left unchanged."""
    key = (key, float(alpha), float(beta), op)
    if key not in _references:
        _references[key] = add(a, b, alpha, beta, op, cols=cols)
    return _references[key]
