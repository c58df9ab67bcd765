"""The contract of spmv_csr_ilu0 (include/spmv_hip.h "the incomplete factorisation") in numpy, the matrices its tests share and
the numpy twins of solvers.pcg and solvers.bicgstab.

M = ILU(0) of a square CSR matrix whose rows are strictly ascending and store their diagonal, on A's pattern; L (unit lower)
and U (upper) in one array.  Rows are taken in ascending i.  w starts as a copy of A's row i.  For each storage position p of
row i with column k < i, ascending: w[p] = fl(w[p] / M[diag_k]) (l = w[p]); then for each position q of row k of M with column
j > k, ascending: if j is stored in row i at position r, w[r] = fma(-l, M[q], w[r]) (the correctly rounded fma of
tests/_attention_order.py).  Row i of M is then w.

`wrong=` gives another factorisation: "desc" (the columns k of a row in descending order), "undivided" (the update applied with
the undivided w[p]) and "a_kk" (the division by A's a_kk instead of u_kk).  apply() is the solve contract of tests/_trsv.py:
lower / unit, then upper / non-unit.

from_rows of _trsv.py dominates each triangle separately; that is not enough here.  dominant_rows() gives |a_ii| >= sum_{j != i}
|a_ij| / 0.9 over the WHOLE row with sorted unique columns.  Strict row dominance survives every elimination step of ILU(0)
(the off-diagonal growth of row i at step k is below the |a_ik| that leaves it), so every pivot is non-zero and |u_ii| >= 0.1
|a_ii|.
"""
import functools

import numpy as np

import _trsv as T
from _attention_order import fma
from _util import RTOL  # noqa: F401  (the project's bound relative to the sum of |terms|: 1e-5)

f32, f64 = np.float32, np.float64
WRONG = ("desc", "undivided", "a_kk")
SERIAL_MAX = 32          # the header's SPMV_ILU0_SERIAL_MAX (the tests check it against the binding)
same, differs = T.same, T.differs


def diag_positions(rp, ci):
    """The storage position of every row's diagonal entry (asserts there is exactly one)."""
    dpos, occ = T.diagonal(rp, ci)
    assert np.all(occ == 1), "every row stores its diagonal once"
    return dpos


def is_sorted(rp, ci):
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return bool(np.all(np.diff(ci)[row[1:] == row[:-1]] > 0))


def factor(rp, ci, va, wrong=None):
    """M's values, float32, under the contract (or, with wrong=, another factorisation)."""
    assert wrong is None or wrong in WRONG
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    va = np.asarray(va, f32)
    n = len(rp) - 1
    assert is_sorted(rp, ci)
    dpos = diag_positions(rp, ci)
    M = va.copy()
    with np.errstate(all="ignore"):
        for i in range(n):
            lo, hi = rp[i], rp[i + 1]
            cols = ci[lo:hi]
            below = np.flatnonzero(cols < i)
            for t in (below[::-1] if wrong == "desc" else below):
                p = lo + t
                k = cols[t]
                pivot = va[dpos[k]] if wrong == "a_kk" else M[dpos[k]]
                used = M[p] if wrong == "undivided" else None
                M[p] = f32(M[p] / pivot)
                l = M[p] if used is None else used
                q = np.arange(dpos[k] + 1, rp[k + 1])
                if q.size == 0:
                    continue
                at = np.searchsorted(cols, ci[q])
                hit = at < cols.size
                hit[hit] = cols[at[hit]] == ci[q][hit]
                r = lo + at[hit]
                M[r] = fma(-l, M[q[hit]], M[r])
    return M


def apply(rp, ci, M, r):
    """z = U^-1 (L^-1 r) through the solve contract of tests/_trsv.py."""
    z = T.solve(rp, ci, M, r, "lower", unit=True)
    return T.solve(rp, ci, M, z, "upper", unit=False)


def lu_product(rp, ci, M):
    """((L U)_ij, mag_ij, terms_ij) in float64 at every stored (i, j): mag is the sum of |l_ik u_kj| over all its terms (the one
    with l_ii = 1 or u_jj included), terms how many there are."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    M = np.asarray(M, f64)
    n = len(rp) - 1
    dpos = diag_positions(rp, ci)
    acc, mag, cnt = np.zeros(M.size, f64), np.zeros(M.size, f64), np.zeros(M.size, np.int64)
    for i in range(n):
        lo, hi = rp[i], rp[i + 1]
        cols = ci[lo:hi]
        for t in np.flatnonzero(cols < i):
            p, k = lo + t, cols[t]
            q = np.arange(dpos[k], rp[k + 1])                 # u_kk and what lies beyond it
            at = np.searchsorted(cols, ci[q])
            hit = at < cols.size
            hit[hit] = cols[at[hit]] == ci[q][hit]
            r = lo + at[hit]
            acc[r] += M[p] * M[q[hit]]
            mag[r] += np.abs(M[p] * M[q[hit]])
            cnt[r] += 1
        up = lo + np.flatnonzero(cols >= i)                   # l_ii = 1
        acc[up] += M[up]
        mag[up] += np.abs(M[up])
        cnt[up] += 1
    return acc, mag, cnt


def dense(rp, ci, va):
    n = len(rp) - 1
    A = np.zeros((n, n), f64)
    A[np.repeat(np.arange(n), np.diff(rp)), ci] = np.asarray(va, f64)
    return A


# ---- the cases ----------------------------------------------------------------------------------------------------------
def dominant_rows(n, cols_of, rng):
    """A CSR with sorted unique columns from per-row off-diagonal columns: values uniform in +-[0.05, 1), the diagonal with
    |d_i| >= sum of the WHOLE row's |off-diagonal| / 0.9."""
    rp, ci, va = [0], [], []
    for i in range(n):
        c = np.unique(np.asarray(cols_of[i], np.int64))
        c = c[c != i]
        v = rng.uniform(0.05, 1.0, c.size) * rng.choice([-1.0, 1.0], c.size)
        d = max(np.abs(v).sum(), 0.45) / 0.9 * rng.uniform(1.0, 1.5) * rng.choice([-1.0, 1.0])
        at = int(np.searchsorted(c, i))
        ci.append(np.insert(c, at, i))
        va.append(np.insert(v, at, d))
        rp.append(rp[-1] + c.size + 1)
    return np.asarray(rp, np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(va).astype(f32)


def dominance(rp, ci, va):
    """max over the rows of sum |off-diagonal| / |diagonal|."""
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    off = np.bincount(row[ci != row], weights=np.abs(np.asarray(va, f64))[ci != row], minlength=n)
    return float(np.max(off / np.abs(np.asarray(va, f64)[diag_positions(rp, ci)]))) if n else 0.0


@functools.lru_cache(maxsize=None)
def generic_case():
    """257 x 257: 0 .. 24 entries off the diagonal and every 16th row 70 .. 120 of them: long rows whose terms come from short
    and from long rows."""
    rng = np.random.default_rng(4712)
    n = 257
    cols = [rng.integers(0, n, int(rng.integers(70, 121)) if i % 16 == 8 else int(rng.integers(0, 25))) for i in range(n)]
    return (n,) + dominant_rows(n, cols, rng)


@functools.lru_cache(maxsize=None)
def diagonal_case(n=3000):
    return (n,) + dominant_rows(n, [[] for _ in range(n)], np.random.default_rng(11))


@functools.lru_cache(maxsize=None)
def tridiagonal_case(n=3000):
    """A chain: n levels of one row (three merged launches at a cap of 1024 levels)."""
    return (n,) + dominant_rows(n, [[c for c in (i - 1, i + 1) if 0 <= c < n] for i in range(n)], np.random.default_rng(12))


@functools.lru_cache(maxsize=None)
def fan_case(heads=10, fans=5000):
    """`fans` rows behind the first `heads`: each stores 1 .. heads of them; the heads store a few of the fans (upper)."""
    rng = np.random.default_rng(13)
    n = heads + fans
    cols = [rng.integers(heads, n, 3) for _ in range(heads)] + [rng.integers(0, heads, int(rng.integers(1, heads + 1))) for _ in range(fans)]
    return (n,) + dominant_rows(n, cols, rng)


@functools.lru_cache(maxsize=None)
def stairs_case(sizes=(69, 70, 71, 70, 69, 1, 71)):
    """Lower levels of exactly these sizes: every row of level k > 0 has 1 .. 3 entries in level k - 1, perhaps one earlier and
    perhaps one in a later row (upper)."""
    rng = np.random.default_rng(15)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    n = int(starts[-1])
    cols = []
    for k, m in enumerate(sizes):
        for _ in range(m):
            c = []
            if k > 0:
                c = list(rng.integers(starts[k - 1], starts[k], int(rng.integers(1, 4))))
                if k > 1 and rng.random() < 0.5:
                    c.append(int(rng.integers(0, starts[k - 1])))
            if k + 1 < len(sizes) and rng.random() < 0.5:
                c.append(int(rng.integers(starts[k + 1], n)))
            cols.append(c)
    return (n,) + dominant_rows(n, cols, rng)


LENGTHS = (1, 31, 32, 33, 63, 64, 65, 129, 5000)


@functools.lru_cache(maxsize=None)
def lengths_case():
    """5000 diagonal rows, then one row of each stored length of LENGTHS (the diagonal counted) with its other entries among them."""
    rng = np.random.default_rng(16)
    base = 5000
    cols = [[] for _ in range(base)] + [rng.choice(base, m - 1, replace=False) for m in LENGTHS]
    n = len(cols)
    return (n,) + dominant_rows(n, cols, rng)


@functools.lru_cache(maxsize=None)
def arrow_case(n=300):
    """The diagonal plus a dense last row and last column: no fill, and every step k updates the last row's diagonal."""
    rng = np.random.default_rng(17)
    return (n,) + dominant_rows(n, [[n - 1] for _ in range(n - 1)] + [list(range(n - 1))], rng)


def stencil_case(pkg, m=8):
    """The library's row-scaled 7-point stencil: weakly dominant in its interior rows (|a_ii| = sum |a_ij|), strictly at the boundary."""
    return pkg.workloads.stencil7(m)


def symmetric_stencil(pkg, m=16):
    """stencil7(m)'s pattern with 6 on the diagonal and -1 off it: symmetric positive definite (the library's own scales its rows)."""
    n, rp, ci, _ = pkg.workloads.stencil7(m)
    row = np.repeat(np.arange(n), np.diff(rp))
    return n, rp, ci, np.where(ci == row, f32(6), f32(-1)).astype(f32)


def krylov_rhs(n, seed=2026):
    return np.random.default_rng(seed).standard_normal(n).astype(f32)


def csr_spmv64(rp, ci, va, x):
    n = len(rp) - 1
    return np.bincount(np.repeat(np.arange(n), np.diff(rp)), weights=np.asarray(va, f64) * np.asarray(x, f64)[ci], minlength=n)


def true_residual(rp, ci, va, b, x):
    """||b - A x|| / ||b|| in float64."""
    return float(np.linalg.norm(np.asarray(b, f64) - csr_spmv64(rp, ci, va, x)) / np.linalg.norm(np.asarray(b, f64)))


# ---- the numpy twins of spmv_test_amd.solvers.pcg / bicgstab ---------------------------------------------------------------
def _bad(v):
    return v == 0 or not np.isfinite(v)


def _dot(a, b):
    return a.dtype.type(np.dot(a, b))


KRYLOV_WRONG = ("beta_inverted", "p_sign")      # other iterations that still converge on the test systems: 1 / beta for beta, p
                                                # updated with the opposite sign of its old direction


def pcg(spmv, prec, b, x, tol=1e-5, maxiter=1000, dtype=f32, wrong=None):
    """(x, iterations, converged): `dtype` throughout; `spmv(v)` gives A v, `prec(r)` M^-1 r (None: r).  The steps of solvers.pcg."""
    assert wrong is None or wrong in KRYLOV_WRONG
    b, x = np.asarray(b, dtype), np.array(x, dtype)
    prec = prec or (lambda v: v.copy())
    r = (b - spmv(x)).astype(dtype)
    z = prec(r)
    p = z.copy()
    q = spmv(p)
    rr, rho, den, bb = _dot(r, r), _dot(r, z), _dot(p, q), _dot(b, b)
    it = 0
    while True:
        if float(rr) <= tol * tol * float(bb):
            return x, it, True
        if it >= maxiter or _bad(rho) or _bad(den) or np.isnan(rr):
            return x, it, False
        alpha = dtype(float(rho) / float(den))
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * q).astype(dtype)
        it += 1
        z = prec(r)
        rr, rho_new = _dot(r, r), _dot(r, z)
        beta = dtype(rho / rho_new) if wrong == "beta_inverted" else dtype(rho_new / rho)
        p = (z - beta * p).astype(dtype) if wrong == "p_sign" else (z + beta * p).astype(dtype)
        q = spmv(p)
        den, rho = _dot(p, q), rho_new


def bicgstab(spmv, prec, b, x, tol=1e-5, maxiter=1000, dtype=f32, wrong=None):
    """(x, iterations, converged): right-preconditioned BiCGStab, `dtype` throughout.  The steps of solvers.bicgstab."""
    assert wrong is None or wrong in KRYLOV_WRONG
    b, x = np.asarray(b, dtype), np.array(x, dtype)
    prec = prec or (lambda v: v.copy())
    n = b.size
    r = (b - spmv(x)).astype(dtype)
    rhat = r.copy()
    p, v = np.zeros(n, dtype), np.zeros(n, dtype)
    rr, bb = _dot(r, r), _dot(b, b)
    rho = alpha = omega = den = tt = dtype(1)
    it = 0

    def guarded(num, d):
        with np.errstate(all="ignore"):
            qv = dtype(num) / dtype(d)
        return qv if np.isfinite(qv) and d != 0 else dtype(0)

    while True:
        if float(rr) <= tol * tol * float(bb):
            return x, it, True
        if it >= maxiter or _bad(rho) or _bad(den) or _bad(tt) or _bad(omega) or np.isnan(rr):
            return x, it, False
        it += 1
        rho_new = _dot(rhat, r)
        beta = guarded(rho * omega, rho_new * alpha) if wrong == "beta_inverted" else guarded(rho_new * alpha, rho * omega)
        p = (r - beta * (p - omega * v)).astype(dtype) if wrong == "p_sign" else (r + beta * (p - omega * v)).astype(dtype)
        y = prec(p)
        v = spmv(y)
        den = _dot(rhat, v)
        alpha = guarded(rho_new, den)
        s = (r - alpha * v).astype(dtype)
        z = prec(s)
        t = spmv(z)
        tt, ts = _dot(t, t), _dot(t, s)
        omega = guarded(ts, tt)
        x = (x + alpha * y + omega * z).astype(dtype)
        r = (s - omega * t).astype(dtype)
        rr, rho = _dot(r, r), rho_new
        if rr == 0:
            tt = omega = dtype(1)


# ---- the iterates of the twins: what tests/test_gpu_krylov.py compares the solvers' x with --------------------------------------
KRYLOV_KS = (1, 2, 4)
NEVER = 1e-20             # a tol no iterate meets: the iteration stops at maxiter


def krylov_systems(pkg):
    """kind -> (the system, the twin): the 512-row versions of the systems of tests/test_gpu_krylov.py."""
    return {"pcg": (symmetric_stencil(pkg, 8), pcg), "bicgstab": (stencil_case(pkg, 8), bicgstab)}


def apply64(rp, ci, M):
    """r -> U^-1 (L^-1 r) in float64 with the float32 factor M widened: dense solves (the systems here have 512 rows)."""
    D = dense(rp, ci, M)
    L, U = np.tril(D, -1) + np.eye(D.shape[0]), np.triu(D)
    return lambda r: np.linalg.solve(U, np.linalg.solve(L, np.asarray(r, f64)))


def twin_iterates(twin, system, b, with_m, dtype, spmv32=None, wrong=None, ks=KRYLOV_KS):
    """{k: x after k iterations from x = 0}: float64 (csr_spmv64, apply64) or float32 (spmv32: a float32 product such as the
    oracle's serial sum; apply()), in both with the factor of factor()."""
    n, rp, ci, va = system
    M = factor(rp, ci, va) if with_m else None
    if dtype is f64:
        spmv = lambda v: csr_spmv64(rp, ci, va, v)
        prec = apply64(rp, ci, M) if with_m else None
    else:
        spmv = lambda v: spmv32(rp, ci, va, v)
        prec = (lambda v: apply(rp, ci, M, v)) if with_m else None
    out = {}
    for k in ks:
        x, it, _ = twin(spmv, prec, np.asarray(b, dtype), np.zeros(n, dtype), NEVER, k, dtype=dtype, wrong=wrong)
        assert it == k, (it, k)
        out[k] = x
    return out


def deviation(x, ref):
    """max |x - ref| / max |ref| in float64."""
    return float(np.max(np.abs(np.asarray(x, f64) - np.asarray(ref, f64))) / np.max(np.abs(np.asarray(ref, f64))))


def krylov_bound(d, k):
    """What a float32 solver may deviate from the float64 twin after k iterations: 8 max(d(k), k 2^-23), d(k) the float32 twin's
    own deviation; the factor 8 is for another order of the dot products and of the rows' sums."""
    return 8 * max(d, k * 2.0 ** -23)
