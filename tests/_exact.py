"""Inputs whose fp32 SpMV is exact in any summation order, and their expected y (host only, numpy + int64).

Values are nonzero integers k in [-4, 4], x entries integers m in [-4, 4] (zero included), and a row may be scaled by
2^e, e in [-40, 40].  While sum |k m| over a row stays within 2^24 units of the row's scale, every partial sum of every
order is an fp32 number, so every kernel and plan must return the one y that int64 arithmetic gives.  The subnormal
copy (k 2^-75, m 2^-74) makes every product a multiple of 2^-149 and most row sums subnormal.

Transforms used by test_gpu_exact.py:
  dilate      column c -> 2c+1 over 2 cols + 1 columns: nothing refers to an even column, so x there can be poisoned
  nonfinite   a few referenced x / vals set to +-Inf and NaN, Inf * 0 included, rows holding +Inf and -Inf
  shuffle     columns shuffled inside each row, about 1/8 of them turned into duplicates of another column of the row
"""
import functools

import numpy as np

EXACT_LIMIT = 1 << 24          # sum |k m| per row, in units of the row's scale
SUB_VAL_EXP, SUB_X_EXP = -75, -74

# the row-length cases of test_gpu_parity.py (copied: a test module is not imported)
EDGE_CASES = {
    "one_row_spanning_30_chunks": ([120_000], 200_000),
    "long_row_between_short_rows": ([3, 0, 5] + [20_000] + [1] * 700 + [9000, 2, 0, 0], 50_000),
    "rows_exactly_chunk_aligned": ([4096, 4096, 2048, 2048, 4096], 10_000),
    "chunk_ends_on_row_boundary_then_empties": ([4096, 0, 0, 0, 17], 5_000),
    "all_rows_empty": ([0] * 1000, 64),
    "trailing_empty_rows": ([5, 7] + [0] * 5000, 100),
    "leading_empty_rows": ([0] * 5000 + [5, 7], 100),
    "single_element": ([1], 1),
    "many_tiny_rows": ([1] * 20_000, 3000),
    "lengths_around_short_threshold": ([31, 32, 33, 34, 63, 64, 65, 127, 128, 129] * 40, 4000),
    "wide_matrix_few_rows": ([7000, 1, 6999], 1_000_000),
    "tall_matrix_one_col": ([1] * 9000, 1),
    "not_multiple_of_anything": ([13] * 777 + [0] + [4099], 5003),
}

SYNTH = {                       # name -> (config, band, scale)
    "c4_band4096": ("c4", 4096, 1 / 64),   # staged windows, 16-bit columns, sorted chunks
    "c3_powerlaw": ("c3", None, 1 / 32),   # rows across chunks: carries, huge segments, wave pieces
    "c2_uniform": ("c2", 0, 1 / 8),        # the panel sweep and the binned layouts
}

SPECIAL = ("wave_pipe_thresholds", "rows_near_64", "stencil7_32", "wide_window", "odd_last_chunk")

MATRICES = sorted(SYNTH) + sorted(EDGE_CASES) + list(SPECIAL)


class Structure:
    """rows, cols, row_ptr (int32), col_idx (int32)."""

    def __init__(self, rows, cols, rp, ci):
        self.rows, self.cols = int(rows), int(cols)
        self.rp = np.ascontiguousarray(rp, np.int32)
        self.ci = np.ascontiguousarray(ci, np.int32)
        self.nnz = int(self.rp[-1])
        assert len(self.ci) == self.nnz and len(self.rp) == self.rows + 1

    @functools.cached_property
    def row_of(self):
        return np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.rp))


def _rng(name, salt=0):
    return np.random.Generator(np.random.PCG64([sum(map(ord, name)) * 7919 + len(name), salt]))


def _sorted_rows(lengths, cols, rng):
    lengths = np.asarray(lengths, np.int64)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    parts = [np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lengths if n]
    ci = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return rp, ci


@functools.lru_cache(maxsize=None)
def structure(name, pkg=None, oracle=None):
    """The column structure of one named matrix (the values come from Exact)."""
    rng = _rng(name)
    if name in SYNTH:
        cfg, band, scale = SYNTH[name]
        w = pkg.workloads.config(cfg, band=band, scale=scale)
        rp = pkg.workloads.row_ptr(w)
        ci, _ = oracle.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, rp)
        return Structure(w.rows, w.cols, rp, ci)
    if name in EDGE_CASES:
        lengths, cols = EDGE_CASES[name]
        rp, ci = _sorted_rows(lengths, cols, rng)
        return Structure(len(lengths), cols, rp, ci)
    if name == "wave_pipe_thresholds":
        # SPMV_WAVE_PIPE: a run is 512 nonzeros, a piece 1024; rows on either side among short rows (mean stays <= 32)
        lengths = rng.integers(0, 12, size=8000)
        for r, n in ((7, 512), (900, 513), (901, 1024), (2500, 1025), (4000, 1028), (7999, 4100)):
            lengths[r] = n
        rp, ci = _sorted_rows(lengths, 9000, rng)
        return Structure(len(lengths), 9000, rp, ci)
    if name == "rows_near_64":
        # SCALAR: mean below 64 keeps k_scalar (thread per row) on rows of 56..68 next to short ones
        lengths = np.where(rng.random(6000) < 0.7, rng.integers(56, 69, size=6000), rng.integers(0, 9, size=6000))
        rp, ci = _sorted_rows(lengths, 5000, rng)
        return Structure(len(lengths), 5000, rp, ci)
    if name == "stencil7_32":
        n, rp, ci, _ = pkg.workloads.stencil7(32)
        return Structure(n, n, rp, ci)
    if name == "wide_window":
        # more than 2^20 columns; each row draws 16 columns within +-60 000 of its diagonal position, so a chunk
        # (256 rows and more) spans well over 2^16 columns; every 64th row draws from all columns
        rows, cols = 8192, (1 << 21) + 5
        lengths = np.full(rows, 16, np.int64)
        rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        centre = (np.arange(rows, dtype=np.int64) * (cols // rows))[:, None]
        ci = np.clip(centre + rng.integers(-60_000, 60_001, size=(rows, 16)), 0, cols - 1)
        ci[::64] = rng.integers(0, cols, size=(rows // 64 + (rows % 64 > 0), 16))
        ci = np.sort(ci, axis=1)          # duplicates possible: allowed outside SPMV_XSKIP, which refuses them
        return Structure(rows, cols, rp, ci.reshape(-1))
    if name == "odd_last_chunk":
        # nnz = 3 (mod 4) and not a multiple of any chunk size: the last chunk ends inside a 16-byte vector
        lengths = rng.integers(0, 40, size=9000)
        lengths[-1] += (3 - int(lengths.sum())) % 4
        rp, ci = _sorted_rows(lengths, 7001, rng)
        assert int(rp[-1]) % 4 == 3
        return Structure(len(lengths), 7001, rp, ci)
    raise KeyError(name)


class Exact:
    """Integer data on a structure: vals = k 2^e[row] (or k 2^-75), x = m (or m 2^-74), and what y must be."""

    def __init__(self, s: Structure, seed_name, scaled=True):
        rng = _rng(seed_name, 1)
        self.s = s
        self.k = (rng.integers(1, 5, size=s.nnz) * rng.choice([-1, 1], size=s.nnz)).astype(np.int64)
        self.m = rng.integers(-4, 5, size=s.cols).astype(np.int64)
        self.e = rng.integers(-40, 41, size=s.rows).astype(np.int64) if scaled else np.zeros(s.rows, np.int64)

    def int_sums(self, k=None, m=None, ci=None, keep=None):
        """int64 sum k m per row (terms where keep is False left out); asserts the exactness condition."""
        k = self.k if k is None else k
        m = self.m if m is None else m
        ci = self.s.ci if ci is None else ci
        p = k * m[ci]
        if keep is not None:
            p = np.where(keep, p, 0)
        cs = np.concatenate([[0], np.cumsum(p)])
        ca = np.concatenate([[0], np.cumsum(np.abs(p))])
        rp = self.s.rp.astype(np.int64)
        mag = ca[rp[1:]] - ca[rp[:-1]]
        assert mag.size == 0 or mag.max() <= EXACT_LIMIT, f"row sum of {mag.max()} units is not exact in fp32"
        return cs[rp[1:]] - cs[rp[:-1]]

    # scaled integers ---------------------------------------------------------------------------------------------
    def vals(self, k=None):
        k = self.k if k is None else k
        return np.ldexp(k.astype(np.float64), self.e[self.s.row_of]).astype(np.float32)

    def x(self, m=None):
        return (self.m if m is None else m).astype(np.float32)

    def expected(self, sums=None):
        sums = self.int_sums() if sums is None else sums
        return np.ldexp(sums.astype(np.float64), self.e).astype(np.float32)

    # the subnormal copy --------------------------------------------------------------------------------------------
    def sub_vals(self):
        return np.ldexp(self.k.astype(np.float64), SUB_VAL_EXP).astype(np.float32)

    def sub_x(self):
        return np.ldexp(self.m.astype(np.float64), SUB_X_EXP).astype(np.float32)

    def sub_expected(self):
        return np.ldexp(self.int_sums().astype(np.float64), SUB_VAL_EXP + SUB_X_EXP).astype(np.float32)


def dilate(s: Structure):
    """Column c -> 2c+1 over 2 cols + 1 columns: x[0], x[cols'-1] and every even entry are never referenced."""
    return Structure(s.rows, 2 * s.cols + 1, s.rp, 2 * s.ci.astype(np.int64) + 1)


def dilated_x(x, poison):
    xd = np.full(2 * len(x) + 1, poison, np.float32)
    xd[1::2] = x
    return xd


def shuffled(s: Structure, seed_name):
    """Columns shuffled inside each row, about 1/8 of them replaced by another column of the same row."""
    rng = _rng(seed_name, 2)
    ci = s.ci.astype(np.int64).copy()
    lengths = np.diff(s.rp).astype(np.int64)
    L = lengths[s.row_of]
    dup = (rng.random(s.nnz) < 0.125) & (L >= 2)
    src = s.rp[:-1].astype(np.int64)[s.row_of] + (rng.random(s.nnz) * L).astype(np.int64)
    ci[dup] = ci[np.minimum(src[dup], s.nnz - 1)]
    order = np.lexsort((rng.random(s.nnz), s.row_of))
    return Structure(s.rows, s.cols, s.rp, ci[order]), order


def chunk_crossing_rows(s: Structure, chunk=4096, limit=4):
    """Rows that hold nonzeros on both sides of a multiple of `chunk` (a chunk boundary of every block size)."""
    if s.nnz <= chunk:
        return np.zeros(0, np.int64)
    cuts = np.arange(chunk, s.nnz, chunk, dtype=np.int64)
    r = np.searchsorted(s.rp.astype(np.int64), cuts, side="right") - 1
    r = r[(s.rp[r] < cuts) & (s.rp[r + 1] > cuts)]
    return np.unique(r)[:limit]


def nonfinite(ex: Exact, seed_name):
    """Non-finite referenced data on ex's structure (column indices of the undilated matrix).  Returns (vals, x, m_int,
    finite_rows): fp32 vals (k 2^e with some entries +-Inf / NaN), fp32 x (m with some entries +-Inf / NaN and some set to
    0 under Inf values), the integer x that the finite rows see, and the mask of rows whose every term stays finite."""
    rng = _rng(seed_name, 3)
    s = ex.s
    vals = ex.vals().astype(np.float32)
    m = ex.m.copy()
    bad_val = np.zeros(s.nnz, bool)
    bad_x = np.zeros(s.cols, bool)
    lengths = np.diff(s.rp)
    if s.nnz:
        # a few values +Inf / -Inf / NaN anywhere
        pos = rng.choice(s.nnz, size=min(9, s.nnz), replace=False)
        vals[pos] = np.resize(np.array([np.inf, -np.inf, np.nan], np.float32), pos.size)
        bad_val[pos] = True
        # Inf values whose x is exactly 0: Inf * 0 = NaN
        pos0 = rng.choice(s.nnz, size=min(4, s.nnz), replace=False)
        pos0 = pos0[~bad_val[pos0]]
        vals[pos0] = np.resize(np.array([np.inf, -np.inf], np.float32), pos0.size)
        bad_val[pos0] = True
        m[s.ci[pos0]] = 0
        # rows holding both +Inf and -Inf (x there nonzero): the two shortest rows of 2+, the longest row, rows across
        # chunk boundaries and a few random ones
        two = np.flatnonzero(lengths >= 2)
        if two.size:
            pm_rows = list(two[np.argsort(lengths[two], kind="stable")[:2]]) + [int(np.argmax(lengths))]
            pm_rows += list(chunk_crossing_rows(s)) + list(rng.choice(two, size=min(3, two.size), replace=False))
            for r in sorted(set(int(r) for r in pm_rows)):
                a, b = int(s.rp[r]), int(s.rp[r + 1]) - 1
                if s.ci[a] == s.ci[b] or bad_val[a] or bad_val[b]:
                    continue
                vals[a], vals[b] = np.inf, -np.inf
                bad_val[a] = bad_val[b] = True
                for c in (s.ci[a], s.ci[b]):
                    if m[c] == 0:
                        m[c] = 3
        # a few referenced x entries +Inf / -Inf / NaN
        ref = np.unique(s.ci)
        cx = rng.choice(ref, size=min(6, ref.size), replace=False)
        bad_x[cx] = True
    x = m.astype(np.float32)
    x[bad_x] = np.resize(np.array([np.inf, -np.inf, np.nan], np.float32), int(bad_x.sum()))
    m_int = np.where(bad_x, 0, m)
    term_bad = bad_val | bad_x[s.ci]
    cb = np.concatenate([[0], np.cumsum(term_bad)])
    finite_rows = (cb[s.rp[1:]] - cb[s.rp[:-1]]) == 0
    return vals, x, m_int, finite_rows
