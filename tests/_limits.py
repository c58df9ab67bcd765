"""Matrices defined by closed integer formulas, at any scale: the inputs of tests/test_gpu_limits.py.

A handle admits rows, cols, nnz < 2^31 (include/spmv_hip.h).  Matrices near those limits cannot be held on the host, and
the device generator spmv_synth_fill is itself code under test there.  So every matrix here is a set of formulas of the
row number r and the nonzero number k:

    length(r)   nonzeros of row r: a table of period P indexed by r % P, a few rows of stated other lengths, and (case F)
                a tail of rows that are never empty
    start(r)    row_ptr[r] in closed form (whole periods + the table's prefix sums + the corrections before r)
    col(r, t)   column of the t-th nonzero of row r
    val(k)      value of nonzero k, one of +-1 .. +-4
    x(j)        x entry j, an integer in [-4, 4] (zeros included)

Each formula uses only + - * // % and comparisons on int64, so the SAME Python source is evaluated by torch on the
device in slabs (build: fills row_ptr, col_idx, vals, and computes the expected y), by numpy on the host for any chosen
rows (host_rows: pins the torch expectation), and at a scaled-down size (Case.scaled).  |val| <= 4, |x| <= 4 and
16 * (longest row) < 2^24: every partial sum of every order, fused or not, is an exactly representable integer, so every
path must return the int64 row sum bit for bit.  No tolerance appears anywhere.

The expected y never comes from a kernel of this library: torch multiplies in int64, takes the prefix sum over slabs of
at most 2^26 nonzeros and differences it at row_ptr (build).

    case  shape                                             what it is for
    A     36 864 x 32 768, rows nearly full, sorted unique   rows of ~32 k nonzeros with k past 2^30: pieces, carries, XSKIP
    B     2^27 rows, lengths 0..64 (mean 8.75), band 8192    bundles, windows, 16-bit columns, sorted chunks past 2^30
    C     like B, columns hashed over 2^24, nnz < 2^30       the binned layouts' streams past the signed byte-offset edge
    D     like C, nnz > 2^30                                 the binned layouts refuse; SPMV_AUTO routes around them
    E     band, nnz = 2^31 - 5                               every int wrap; every panel layout refuses
    F     2^30 + 2^20 + 5 rows of 0 / 1 / 2 nonzeros         y and row_ptr past 4 GiB, grids near 2^31 / 256
    G     3000 x (2^30 + 7), columns at both ends of x       the x descriptor edge on every path
"""
import numpy as np

INT_MAX = (1 << 31) - 1
SLAB = 1 << 26
EXACT_LIMIT = 1 << 24

# lengths 0..64, sum 280 over 32 rows (mean 8.75): a lane per short row, 33 and 64 on either side of the wave's 32
SHORT_TABLE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 0, 64, 33, 31, 32, 1, 0, 0, 2, 3, 1, 0, 3, 4, 1, 0)
assert sum(SHORT_TABLE) == 280 and max(SHORT_TABLE) == 64
A_COLS = 32768
A_GAPS = (0, 3, 1000, 17, 4093, 1, 250, 64)                  # columns a row of case A leaves out
F_TABLE = (0, 1, 2, 1, 0, 1, 2, 0)
G_TABLE = (0, 5, 23, 1, 12, 7, 0, 19, 3, 16, 2, 9, 21, 4, 11, 8)
HASH_A, HASH_B, HASH_P = 2654435761, 805306457, 4294967291


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _table(values, like):
    if _is_torch(like):
        import torch
        return torch.tensor(values, dtype=torch.int64, device=like.device)
    return np.asarray(values, np.int64)


def _prefix(values):
    out = [0]
    for v in values:
        out.append(out[-1] + v)
    return out


class Case:
    """One matrix: sizes, the length table, the rows of other lengths, the column rule."""

    def __init__(self, name, rows, cols, table, columns, specials=(), tail=0, band=0):
        self.name, self.rows, self.cols = name, int(rows), int(cols)
        self.table, self.columns, self.tail, self.band = tuple(table), columns, int(tail), int(band)
        self.P = len(self.table)
        self.pre = _prefix(self.table)
        self.zpre = _prefix([1 if v == 0 else 0 for v in self.table])
        self.specials = tuple(sorted((int(r), int(n)) for r, n in specials))
        assert len({r for r, _ in self.specials}) == len(self.specials)
        assert all(0 <= r < self.rows - self.tail for r, _ in self.specials)
        self.nnz = int(self.start(np.asarray([self.rows], np.int64))[0])
        longest = max([max(self.table) + 1] + [n for _, n in self.specials])
        assert 16 * longest < EXACT_LIMIT and 0 < self.nnz <= INT_MAX and self.rows <= INT_MAX and self.cols <= INT_MAX

    # ---- the formulas (r, t, k, j: int64 arrays of numpy or torch) -----------------------------------------------------
    def _zeros_before(self, r):
        return (r // self.P) * self.zpre[-1] + _table(self.zpre, r)[r % self.P]

    def length(self, r):
        n = _table(self.table, r)[r % self.P]
        if self.tail:
            n = n + (r >= self.rows - self.tail) * (n == 0)
        for row, m in self.specials:
            n = n + (r == row) * (m - self.table[row % self.P])
        return n

    def start(self, r):
        s = (r // self.P) * self.pre[-1] + _table(self.pre, r)[r % self.P]
        if self.tail:
            r0 = self.rows - self.tail
            z0 = (r0 // self.P) * self.zpre[-1] + self.zpre[r0 % self.P]
            s = s + (r > r0) * (self._zeros_before(r) - z0)
        for row, m in self.specials:
            s = s + (r > row) * (m - self.table[row % self.P])
        return s

    def col(self, r, t):
        if self.columns == "full":          # every column but a gap of A_GAPS[r % 8] columns at position s(r): sorted, unique
            gap = _table(A_GAPS, r)[r % len(A_GAPS)]
            s = (r * 7919) % (self.cols - gap + 1)
            return t + gap * (t >= s)
        if self.columns == "band":          # ascending inside [r, r + band): first (31 r) % 1024, step 1 + r % 97 (specials: 1)
            step = 1 + r % 97
            for row, _ in self.specials:
                step = step - (r == row) * (row % 97)
            return r + (r * 31) % 1024 + t * step
        h = ((r * HASH_A + t * HASH_B) % HASH_P)
        if self.columns == "hash":          # anywhere in [0, cols); a row may hold a column twice
            return h % self.cols
        if self.columns == "ends":          # rows below 1024: a window at the far end of x; the others anywhere; both ends referenced
            local = (self.cols - 9000) + (r % 4000) + h % 4000
            c = local * (r < 1024) + (h % self.cols) * (r >= 1024)
            z1, z2 = ((r == 1) * (t == 0)) * 1, ((r == 2) * (t == 0)) * 1      # x[0] and x[cols - 1] are referenced
            return c * (1 - z1 - z2) + (self.cols - 1) * z2
        raise ValueError(self.columns)

    @staticmethod
    def val(k):
        # (reduced by a prime, not a power of two: val(k + 2^30) must not repeat val(k), or a wrapped index would go unseen)
        m = (((k * HASH_A) % HASH_P) // 1024) % 8     # 0..7 -> -4..-1, 1..4
        return m - 4 + (m >= 4)

    @staticmethod
    def x(j):
        return ((j * 7 + j // 13) % 9) - 4

    @staticmethod
    def xcol(j, c):
        """X[j][c] of the SpMM runs; column 0 is x."""
        return ((j * 7 + j // 13 + c * 13 + (j // 5) * (c % 3)) % 9) - 4

    # ---- derived -------------------------------------------------------------------------------------------------------
    def row_of(self, k):
        """The row that holds nonzero k (host, from start() alone)."""
        lo, hi = 0, self.rows                   # start(lo) <= k < start(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if int(self.start(np.asarray([mid], np.int64))[0]) <= k:
                lo = mid
            else:
                hi = mid
        return lo

    def scaled(self, div=64):
        """The same formulas with the rows divided (case G: the columns): nothing reaches 2^29."""
        if self.columns == "ends":
            return Case(self.name + "/64", self.rows, (self.cols - 7) // div + 7, self.table, self.columns, self.specials)
        rows = self.rows // div
        tail = self.tail // div
        sp = {}
        for r, n in self.specials:
            sp[min(r // div, rows - tail - 1)] = n
        cols = self.cols if self.columns in ("full", "hash") else rows + self.band
        return Case(self.name + "/64", rows, cols, self.table, self.columns, tuple(sp.items()), tail, self.band)


def _band_case(name, rows, band=8192, specials=()):
    # the longest band row: 1023 + 64 * 97 columns past r; a special row steps by 1
    assert 1023 + 64 * 97 < band and all(1023 + n < band for _, n in specials)
    return Case(name, rows, rows + band, SHORT_TABLE, "band", specials, band=band)


def _case_e():
    target = (1 << 31) - 5                                   # = 3 (mod 4): the last row ends inside a 16-byte vector
    periods = (target - 700) // 280
    rows = periods * 32 + 20                                  # the last row is position 19 of the table (31), made longer
    base = periods * 280 + sum(SHORT_TABLE[:20])
    last = target - base + SHORT_TABLE[19]
    c = _band_case("E", rows, specials=((rows - 1, last),))
    assert c.nnz == target and c.nnz % 4 == 3 and 512 < last < 2048
    return c


def _case_f():
    rows = (1 << 30) + (1 << 20) + 5
    sp = ((12345, 600), (1 << 29, 5000), ((1 << 30) + 77, 600), (rows - 65536 - 9, 5000))
    return Case("F", rows, 1 << 18, F_TABLE, "hash", sp, tail=65536)


def _case_g():
    sp = ((10, 511), (11, 512), (700, 1025), (1900, 5000), (2999, 700))
    return Case("G", 3000, (1 << 30) + 7, G_TABLE, "ends", sp)


_BUILDERS = {
    "A": lambda: Case("A", 36864, A_COLS, [A_COLS - g for g in A_GAPS], "full"),
    "B": lambda: _band_case("B", 1 << 27),
    "C": lambda: Case("C", (1 << 26) + (1 << 25), 1 << 24, SHORT_TABLE, "hash"),
    "D": lambda: Case("D", 1 << 27, 1 << 24, SHORT_TABLE, "hash"),
    "E": _case_e,
    "F": _case_f,
    "G": _case_g,
}
ORDER = ("G", "C", "F", "A", "B", "D", "E")          # the giant cases, smallest first
_cache = {}


def case(name, scaled=False):
    key = (name, scaled)
    if key not in _cache:
        c = _BUILDERS[name]()
        _cache[key] = c.scaled() if scaled else c
    return _cache[key]


def check_sizes():
    """The conditions the cases are built to meet (the issue's table)."""
    w_lo, w_hi = (1 << 30) + (1 << 26), (1 << 30) + (1 << 28)
    a, b, c, d, e, f, g = (case(n) for n in "ABCDEFG")
    assert w_lo <= a.nnz <= w_hi and (a.rows + 1023) // 1024 * a.cols <= 1 << 27
    assert w_lo <= b.nnz <= w_hi and b.nnz <= 32 * b.rows
    assert (1 << 29) + (1 << 26) <= c.nnz <= (1 << 30) - (1 << 24) and c.cols >= 1 << 22
    assert w_lo <= d.nnz <= w_hi and d.cols == c.cols
    assert (1 << 31) - 1024 <= e.nnz <= (1 << 31) - 2 and e.nnz % 4 == 3 and e.nnz > INT_MAX - 8192
    assert f.rows == (1 << 30) + (1 << 20) + 5 and f.nnz <= 1 << 30
    assert g.cols == (1 << 30) + 7
    for n in "ABCDEFG":
        s = case(n, scaled=True)
        assert s.nnz < 1 << 29 and s.rows < 1 << 29 and s.cols < 1 << 29, n


# ---- torch: the arrays and the expected y, in slabs ----------------------------------------------------------------------
class Built:
    pass


def build(c, torch, device, slab=SLAB):
    """row_ptr, col_idx, vals, x and the expected y (float32, exact) of case c on `device`, by torch alone.  Unreferenced
    x entries are NaN."""
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    b = Built()
    b.case = c
    b.rp = torch.empty(c.rows + 1, dtype=i32, device=device)
    for r0 in range(0, c.rows + 1, slab):
        r = torch.arange(r0, min(c.rows + 1, r0 + slab), dtype=i64, device=device)
        b.rp[r0:r0 + r.numel()] = c.start(r).to(i32)
    b.ci = torch.empty(c.nnz, dtype=i32, device=device)
    b.va = torch.empty(c.nnz, dtype=f32, device=device)
    b.exp = torch.zeros(c.rows, dtype=f32, device=device)
    ref = torch.zeros(c.cols, dtype=torch.bool, device=device)
    b.col_min, b.col_max = c.cols, -1
    for k0, k1, lo, hi, ends in _slabs(b, torch, slab):
        k = torch.arange(k0, k1, dtype=i64, device=device)
        r_first, r_end = lo - 1, _at(b.rp, torch, k1 - 1)     # the rows that hold nonzeros k0 and k1 - 1 (the latter + 1)
        rp_loc = b.rp[r_first:r_end + 1].to(i64)
        r = torch.searchsorted(rp_loc, k, right=True) - 1
        t = k - rp_loc[r]
        r += r_first
        col, val = c.col(r, t), c.val(k)
        b.col_min, b.col_max = min(b.col_min, int(col.min().item())), max(b.col_max, int(col.max().item()))
        b.ci[k0:k1] = col.to(i32)
        b.va[k0:k1] = val.to(f32)
        ref[col] = True
        _difference(torch, b.exp, val * c.x(col), lo, hi, ends, b, "_carry")
    b.x = torch.empty(c.cols, dtype=f32, device=device)
    for j0 in range(0, c.cols, slab):
        j = torch.arange(j0, min(c.cols, j0 + slab), dtype=i64, device=device)
        b.x[j0:j0 + j.numel()] = c.x(j).to(f32)
    b.referenced = ref
    b.x[~ref] = float("nan")
    return b


def _at(rp, torch, v):
    """How many entries of row_ptr are <= v."""
    return int(torch.searchsorted(rp, torch.tensor([v], dtype=torch.int32, device=rp.device), right=True).item())


def _slabs(b, torch, slab):
    """Slabs [k0, k1) of nonzeros with the row boundaries inside: row_ptr[rr] in (k0, k1] for rr in [lo, hi), and their
    positions `ends` (row_ptr[rr] - 1 - k0) in the slab.  Row lo - 1 holds nonzero k0."""
    nnz = b.case.nnz
    for k0 in range(0, nnz, slab):
        k1 = min(nnz, k0 + slab)
        lo, hi = _at(b.rp, torch, k0), _at(b.rp, torch, k1)
        yield k0, k1, lo, hi, b.rp[lo:hi].to(torch.int64) - 1 - k0


def _difference(torch, out, p, lo, hi, ends, b, key):
    """out[rows ending in this slab] = differences of the running int64 prefix sum of p (1-D, or 2-D: a ROW per SpMM
    column, so that the prefix sum runs along contiguous memory) at the row boundaries; the sums at the slab's start and
    at the last boundary seen are carried in b.<key>."""
    zero = torch.zeros(tuple(p.shape[:-1]) + (1,), dtype=torch.int64, device=p.device)
    total, last = getattr(b, key, (zero, zero))
    cs = torch.cumsum(p, -1) + total
    total = cs[..., -1:].clone()
    if hi > lo:
        cb = cs[..., ends]
        d = (cb - torch.cat([last, cb[..., :-1]], -1)).to(out.dtype)
        out[lo - 1:hi - 1] = d if d.dim() == 1 else d.t()
        last = cb[..., -1:].clone()
    setattr(b, key, (total, last))


def expected_columns(b, torch, c0, c1, slab=1 << 24):
    """The expected Y[:, c0:c1] (float32, exact) of an SpMM with X = xcol, from the arrays torch filled: int64 products,
    prefix sums per column over slabs, differences at row_ptr."""
    c = b.case
    out = torch.zeros((c.rows, c1 - c0), dtype=torch.float32, device=b.rp.device)
    cc = torch.arange(c0, c1, dtype=torch.int64, device=b.rp.device)[:, None]
    key = f"_carry_{c0}_{c1}"
    if hasattr(b, key):
        delattr(b, key)
    for k0, k1, lo, hi, ends in _slabs(b, torch, slab):
        p = b.va[k0:k1].to(torch.int64)[None, :] * c.xcol(b.ci[k0:k1].to(torch.int64)[None, :], cc)
        _difference(torch, out, p, lo, hi, ends, b, key)
    delattr(b, key)
    return out


def fill_X(c, torch, device, X, slab=1 << 20):
    """X[j][cc] = xcol(j, cc) for every column of the 2-D float32 tensor X (cols rows), rows no nonzero refers to NaN."""
    cc = torch.arange(X.shape[1], dtype=torch.int64, device=device)[None, :]
    for j0 in range(0, c.cols, slab):
        j = torch.arange(j0, min(c.cols, j0 + slab), dtype=torch.int64, device=device)[:, None]
        X[j0:j0 + j.shape[0]] = c.xcol(j, cc).to(torch.float32)


# ---- numpy: chosen rows from the formulas alone --------------------------------------------------------------------------
def pinned_rows(c, seed=2024):
    """The first and last 65 536 rows, 65 536 seeded random rows and every row that holds nonzero 2^29, 2^30 or nnz - 1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = min(65536, c.rows)
    rows = [np.arange(n), np.arange(c.rows - n, c.rows), rng.integers(0, c.rows, size=n)]
    rows.append(np.asarray([c.row_of(k) for k in (1 << 29, 1 << 30, c.nnz - 1) if k < c.nnz], np.int64))
    return np.unique(np.concatenate(rows).astype(np.int64))


def host_rows(c, rows, columns=0, group=1 << 24):
    """int64 sums of the given rows (and, with columns > 0, of every SpMM column: len(rows) x columns) by numpy."""
    rows = np.asarray(rows, np.int64)
    out = np.zeros((len(rows), max(columns, 1)), np.int64)
    b, n = c.start(rows), c.length(rows)
    assert np.array_equal(c.start(rows + 1), b + n), "start() and length() disagree"
    i0 = 0
    while i0 < len(rows):
        i1 = i0 + max(1, int(np.searchsorted(np.cumsum(n[i0:]), group, side="right")))
        nn = n[i0:i1]
        idx = np.repeat(np.arange(i1 - i0), nn)
        t = np.arange(int(nn.sum()), dtype=np.int64) - np.repeat(np.cumsum(nn) - nn, nn)
        r = rows[i0:i1][idx]
        col, val = c.col(r, t), c.val(b[i0:i1][idx] + t)
        assert col.size == 0 or (col.min() >= 0 and col.max() < c.cols)
        for cc in range(max(columns, 1)):
            p = val * (c.xcol(col, cc) if columns else c.x(col))
            out[i0:i1, cc] = np.rint(np.bincount(idx, weights=p.astype(np.float64), minlength=i1 - i0)).astype(np.int64)
        i0 = i1
    return out if columns else out[:, 0]


def host_arrays(c):
    """The whole matrix on the host (small cases only): row_ptr, col_idx, vals (int64), by numpy."""
    assert c.nnz <= 1 << 26
    r = np.arange(c.rows + 1, dtype=np.int64)
    rp = c.start(r)
    n = np.diff(rp)
    assert np.array_equal(n, c.length(r[:-1]))
    row = np.repeat(r[:-1], n)
    t = np.arange(c.nnz, dtype=np.int64) - rp[row]
    return rp, c.col(row, t), c.val(np.arange(c.nnz, dtype=np.int64))
