"""The contract of spmv_csr_trsv (include/spmv_hip.h "the triangular solve") in numpy, and the matrices its tests share.

x = T^-1 b for the lower ("lower": the entries with col <= row) or the upper triangle of a square CSR matrix; the other
triangle's entries are never read.  The terms of row i are its storage positions s, ascending, with col_idx[s] < i (upper:
> i); a repeated column gives several terms.  For n <= serial_max terms: s = +0, s = fma(v_t, x[c_t], s) in term order (the
correctly rounded fma of tests/_attention_order.py).  For more: 64 chains, chain l over the terms l, l + 64, ... from +0, then
p[l] += p[l + w] for l < w, w = 32, 16, 8, 4, 2, 1, and s = p[0].  Then x_i = fl(fl(b_i - s) / d_i), under unit x_i = fl(b_i - s).

level[i] = 0 for a row without terms, else 1 + max level[c_t]; `order` lists the rows by (level, row) ascending and `level_ptr`
where every level starts.

`wrong=` gives another order of the same sum: "desc" (the terms of a row in descending order), "from_b" (the chain started at
b_i: acc = b_i, acc = fma(-v_t, x[c_t], acc)) and "serial_long" (a row of more than serial_max terms summed as one chain).
A NaN compares as a NaN: its sign and payload are the hardware's.
"""
import functools

import numpy as np

from _attention_order import fma
from _util import RTOL  # noqa: F401  (the project's bound relative to the sum of |terms|: 1e-5)

f32, f64 = np.float32, np.float64
UPLOS = ("lower", "upper")
WRONG = ("desc", "from_b", "serial_long")
SERIAL_MAX = 32          # the header's SPMV_TRSV_SERIAL_MAX (the tests check it against the binding)


def terms(rp, ci, uplo):
    """(pos, row, rank, count): the storage positions of all terms, ascending; each one's row and its number among the row's
    terms; the number of terms of every row."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    pos = np.flatnonzero(ci < row if uplo == "lower" else ci > row)
    trow = row[pos]
    count = np.bincount(trow, minlength=n).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)])
    rank = np.arange(pos.size, dtype=np.int64) - start[trow]
    return pos, trow, rank, count


def diagonal(rp, ci):
    """(position of the first diagonal entry of every row or -1, occurrences)."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    d = np.flatnonzero(ci == row)
    occ = np.bincount(row[d], minlength=n)
    first = np.full(n, -1, np.int64)
    first[row[d][::-1]] = d[::-1]
    return first, occ


def levels(rp, ci, uplo):
    """level[i], by the definition, one row after the other (a term's column is an earlier row of this walk)."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n = len(rp) - 1
    lev = np.zeros(n, np.int64)
    for i in (range(n) if uplo == "lower" else range(n - 1, -1, -1)):
        c = ci[rp[i]:rp[i + 1]]
        c = c[c < i] if uplo == "lower" else c[c > i]
        lev[i] = 1 + lev[c].max() if c.size else 0
    return lev


def order(lev):
    """(level_ptr int32, order int32): the rows by (level, row) ascending."""
    lev = np.asarray(lev, np.int64)
    od = np.lexsort((np.arange(lev.size), lev)).astype(np.int32)
    lp = np.concatenate([[0], np.cumsum(np.bincount(lev, minlength=int(lev.max()) + 1 if lev.size else 0))]).astype(np.int32)
    return lp, od


def solve(rp, ci, va, b, uplo="lower", unit=False, wrong=None, serial_max=SERIAL_MAX, lev=None):
    """x float32 under the contract (or, with wrong=, under another order of the sums)."""
    assert uplo in UPLOS and (wrong is None or wrong in WRONG)
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    va, b = np.asarray(va, f32), np.asarray(b, f32)
    n = len(rp) - 1
    pos, trow, rank, count = terms(rp, ci, uplo)
    if wrong == "desc":
        rank = count[trow] - 1 - rank
    dpos, occ = diagonal(rp, ci)
    if not unit:
        assert np.all(occ == 1), "non-unit: exactly one diagonal entry per row"
    lev = levels(rp, ci, uplo) if lev is None else np.asarray(lev, np.int64)
    lp, od = order(lev)
    is_long = count > serial_max if wrong != "serial_long" else np.zeros(n, bool)
    # the terms level by level, and inside a level by rank
    by = np.lexsort((rank, lev[trow]))
    pos, trow, rank = pos[by], trow[by], rank[by]
    tstart = np.searchsorted(lev[trow], np.arange(len(lp)))
    x = np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for k in range(len(lp) - 1):
            R = od[lp[k]:lp[k + 1]]
            s = b[R].copy() if wrong == "from_b" else np.zeros(R.size, f32)
            t0, t1 = tstart[k], tstart[k + 1]
            if t1 > t0:
                where = np.full(n, -1, np.int64)
                where[R] = np.arange(R.size)
                p_, r_, k_ = pos[t0:t1], trow[t0:t1], rank[t0:t1]
                lg = is_long[r_]
                sign = f32(-1) if wrong == "from_b" else f32(1)
                # short rows: one chain
                ps, rs, ks = p_[~lg], r_[~lg], k_[~lg]
                if ps.size:
                    cut = np.searchsorted(ks, np.arange(int(ks.max()) + 2))
                    for q in range(len(cut) - 1):
                        sel = slice(cut[q], cut[q + 1])
                        at = where[rs[sel]]
                        s[at] = fma(sign * va[ps[sel]], x[ci[ps[sel]]], s[at])
                # long rows: 64 chains and the combine
                pl, rl, kl = p_[lg], r_[lg], k_[lg]
                if pl.size:
                    rows_l = np.unique(rl)
                    slot = np.full(n, -1, np.int64)
                    slot[rows_l] = np.arange(rows_l.size)
                    P = np.zeros((rows_l.size, 64), f32)
                    step = kl // 64
                    cut = np.searchsorted(step, np.arange(int(step.max()) + 2))
                    for q in range(len(cut) - 1):
                        sel = slice(cut[q], cut[q + 1])
                        a_, c_ = slot[rl[sel]], kl[sel] % 64
                        P[a_, c_] = fma(sign * va[pl[sel]], x[ci[pl[sel]]], P[a_, c_])
                    for w in (32, 16, 8, 4, 2, 1):
                        P[:, :w] = P[:, :w] + P[:, w:2 * w]
                    if wrong == "from_b":
                        s[where[rows_l]] = (b[rows_l] + P[:, 0]).astype(f32)
                    else:
                        s[where[rows_l]] = P[:, 0]
            num = s if wrong == "from_b" else (b[R] - s).astype(f32)
            x[R] = num if unit else (num / va[dpos[R]]).astype(f32)
    return x


def dense_solve(rp, ci, va, b, uplo="lower", unit=False):
    """(x float64 of a dense solve with the triangle that is read, mag): mag_i = (|b_i| + sum |v_t x_c|) / |d_i|."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = (ci < row) if uplo == "lower" else (ci > row)
    T = np.zeros((n, n), f64)
    np.add.at(T, (row[keep], ci[keep]), np.asarray(va, f64)[keep])
    d = np.ones(n, f64)
    if not unit:
        dg = ci == row
        d = np.zeros(n, f64)
        np.add.at(d, row[dg], np.asarray(va, f64)[dg])
    x = np.zeros(n, f64)
    mag = np.zeros(n, f64)
    A = np.zeros((n, n), f64)
    np.add.at(A, (row[keep], ci[keep]), np.abs(np.asarray(va, f64)[keep]))
    for i in (range(n) if uplo == "lower" else range(n - 1, -1, -1)):
        x[i] = (float(b[i]) - T[i] @ x) / d[i]
        mag[i] = (abs(float(b[i])) + A[i] @ np.abs(x)) / abs(d[i])
    return x, mag


def same(a, b):
    """None when two float32 arrays are equal bit for bit (a NaN matches any NaN), else a description of the first difference."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return f"{int(bad.sum())} of {a.size} differ, first at {i}: {a[i]!r} ({a.view(np.uint32)[i]:#010x}) and {b[i]!r} ({b.view(np.uint32)[i]:#010x})"


def differs(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


# ---- the cases ----------------------------------------------------------------------------------------------------------
def from_rows(n, cols_of, rng, diag=True):
    """A row-dominant CSR from per-row term columns (in the given order: unsorted, repeats kept): values uniform in [-1, 1)
    without zeros, the diagonal at a random place of the row with |d_i| >= max(sum |lower terms|, sum |upper terms|) / 0.9."""
    rp, ci, va = [0], [], []
    for i in range(n):
        c = np.asarray(cols_of[i], np.int64)
        v = rng.uniform(0.05, 1.0, c.size) * rng.choice([-1.0, 1.0], c.size)
        if diag:
            lo, up = np.abs(v[c < i]).sum(), np.abs(v[c > i]).sum()
            d = max(lo, up, 0.45) / 0.9 * rng.uniform(1.0, 1.5) * rng.choice([-1.0, 1.0])
            at = int(rng.integers(0, c.size + 1))
            c, v = np.insert(c, at, i), np.insert(v, at, d)
        ci.append(c)
        va.append(v)
        rp.append(rp[-1] + c.size)
    return (np.asarray(rp, np.int32), np.concatenate(ci).astype(np.int32) if ci else np.zeros(0, np.int32),
            np.concatenate(va).astype(f32) if va else np.zeros(0, f32))


def rhs(n, rng):
    return (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(f32)


@functools.lru_cache(maxsize=None)
def generic_case():
    """257 x 257, a FULL matrix: unsorted rows with repeated columns, 0 .. 24 entries off the diagonal and every 16th row 70 ..
    120 of them (long rows in both triangles)."""
    rng = np.random.default_rng(4711)
    n = 257
    cols = []
    for i in range(n):
        k = int(rng.integers(70, 121)) if i % 16 == 8 else int(rng.integers(0, 25))
        c = rng.integers(0, n, k)
        cols.append(c[c != i])
    rp, ci, va = from_rows(n, cols, rng)
    return n, rp, ci, va, rhs(n, rng)


def poison_other_triangle(rp, ci, va, uplo):
    """The same matrix with NaN wherever the solve may not read."""
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    out = np.array(va, f32)
    out[(ci > row) if uplo == "lower" else (ci < row)] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def diagonal_case(n=3000):
    rng = np.random.default_rng(1)
    rp, ci, va = from_rows(n, [[] for _ in range(n)], rng)
    return n, rp, ci, va, rhs(n, rng)


@functools.lru_cache(maxsize=None)
def chain_case(n=3000, uplo="lower"):
    """A bidiagonal chain: n levels of one row."""
    rng = np.random.default_rng(2)
    cols = [([i - 1] if i > 0 else []) if uplo == "lower" else ([i + 1] if i < n - 1 else []) for i in range(n)]
    rp, ci, va = from_rows(n, cols, rng)
    return n, rp, ci, va, rhs(n, rng)


@functools.lru_cache(maxsize=None)
def fan_case(heads=10, fans=5000):
    """`fans` rows that depend only on the first `heads` (lower), each on 1 .. heads of them in any order."""
    rng = np.random.default_rng(3)
    n = heads + fans
    cols = [[] for _ in range(heads)] + [rng.integers(0, heads, int(rng.integers(1, heads + 1))) for _ in range(fans)]
    rp, ci, va = from_rows(n, cols, rng)
    return n, rp, ci, va, rhs(n, rng)


@functools.lru_cache(maxsize=None)
def stairs_case(sizes, uplo="lower"):
    """Levels of exactly these sizes: every row of level k > 0 has 1 .. 3 terms in level k - 1 and perhaps one earlier."""
    rng = np.random.default_rng(5)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    n = int(starts[-1])
    cols = []
    for k, m in enumerate(sizes):
        for _ in range(m):
            if k == 0:
                cols.append([])
                continue
            c = list(rng.integers(starts[k - 1], starts[k], int(rng.integers(1, 4))))
            if k > 1 and rng.random() < 0.5:
                c.insert(0, int(rng.integers(0, starts[k - 1])))
            cols.append(c)
    if uplo == "upper":                                      # the mirror image: row i -> n - 1 - i
        cols = [[n - 1 - c for c in cs] for cs in cols[::-1]]
    rp, ci, va = from_rows(n, cols, rng)
    return n, rp, ci, va, rhs(n, rng)


LENGTHS = lambda serial_max=SERIAL_MAX: (0, 1, serial_max - 1, serial_max, serial_max + 1, 63, 64, 65, 129, 5000)


@functools.lru_cache(maxsize=None)
def lengths_case(serial_max=SERIAL_MAX):
    """5000 rows without terms, then one row of each length of LENGTHS above 0 with its terms among them (unsorted; the longer
    rows repeat columns).  Under thin_rows = 1 both levels are grid launches, under 1 << 30 one workgroup walks both."""
    rng = np.random.default_rng(6)
    base = 5000
    cols = [[] for _ in range(base)] + [rng.integers(0, base, m) for m in LENGTHS(serial_max) if m > 0]
    n = len(cols)
    rp, ci, va = from_rows(n, cols, rng)
    return n, rp, ci, va, rhs(n, rng)


def stencil_case(pkg, m=8):
    n, rp, ci, va = pkg.workloads.stencil7(m)
    return n, rp, ci, va, rhs(n, np.random.default_rng(7))


# ---- Gauss-Seidel, the numpy twin of spmv_test_amd.solvers.gauss_seidel ---------------------------------------------------------
def gauss_seidel(spmv, rp, ci, va, b, x, sweeps=1, symmetric=False):
    """x <- x + (D + L)^-1 (b - A x) per sweep (symmetric: then x <- x + (D + U)^-1 (b - A x)); `spmv(x)` gives A x in
    float32 (the oracle's serial sum on the device's side, any float32 product for the host test)."""
    x = np.array(x, f32)
    for _ in range(sweeps):
        for uplo in ("lower", "upper") if symmetric else ("lower",):
            r = (np.asarray(b, f32) - spmv(x)).astype(f32)
            x = (x + solve(rp, ci, va, r, uplo)).astype(f32)
    return x
