"""The contracts of spmv_csr_color and spmv_csr_permute (include/spmv_hip.h "the multicolour ordering") in numpy, and the patterns
their tests share.

Colouring.  The graph is the symmetrised pattern, N(i) = { j != i : (i, j) stored or (j, i) stored }.  key(i) = fmix32(i ^ seed)
compared unsigned; color[i] is the smallest c >= 0 not in { color[j] : j in N(i), key(j) > key(i) }: the sequential greedy
colouring in descending key order.  round(i) = 1 + max(round(j) : j in N(i), key(j) > key(i)), 1 where there is no such j.  perm
lists the rows by (colour, row) ascending, color_ptr where every colour starts in it.  rows = 0: no colour and no round.

`wrong=` gives another colouring: "rows_only" (the neighbours stored in A's rows alone, without the transpose), "key_i" (key(i) = i)
and "stale" (rounds in which EVERY uncoloured row takes the smallest colour unused by all neighbours coloured when the round began,
and of two neighbours that took the same colour the one of the lower key gives it back).

Permutation.  New index r holds old index perm[r].  Row r of B is row row_perm[r] of A, an entry in column j lands in the column c
with col_perm[c] = j, and inside a row the entries ascend by (new column, storage position in A); map[i] is A's storage position of
B's entry i and values are copied as bits.
"""
import functools

import numpy as np

import _ilu0 as G
import _trsv as T

f32 = np.float32
SERIAL_MAX = 32          # the header's SPMV_COLOR_SERIAL_MAX (the tests check it against the binding)
SEEDS = (0, 0x9E3779B9)
WRONG = ("rows_only", "key_i", "stale")


def fmix32(h):
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.uint32)


def keys(n, seed):
    return fmix32(np.arange(n, dtype=np.uint64) ^ np.uint64(seed))


def adjacency(rp, ci, symmetric=True):
    """(ptr, adj): the neighbours of every row, sorted and unique, the row itself left out."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = row != ci
    a, b = row[keep], ci[keep]
    if symmetric:
        a, b = np.concatenate([a, b]), np.concatenate([b, a])
    e = np.unique(a * max(n, 1) + b)
    a, b = e // max(n, 1), e % max(n, 1)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))]).astype(np.int64)
    return ptr, b


def neighbour_entries(rp, ci):
    """The entries of every row's neighbour list as the library counts them: the row of A plus the row of its transpose."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n = len(rp) - 1
    return np.diff(rp) + np.bincount(ci, minlength=n)


def max_degree(rp, ci):
    ptr, _ = adjacency(rp, ci)
    return int(np.diff(ptr).max()) if len(ptr) > 1 else 0


def _mex(used):
    used = np.unique(used)
    gap = np.flatnonzero(used != np.arange(used.size))
    return int(gap[0]) if gap.size else int(used.size)


def _stale(n, ptr, adj, key):
    color = np.full(n, -1, np.int64)
    rounds = 0
    while np.any(color < 0):
        rounds += 1
        old = color.copy()
        todo = np.flatnonzero(old < 0)
        for i in todo:
            nb = adj[ptr[i]:ptr[i + 1]]
            color[i] = _mex(old[nb][old[nb] >= 0])
        for i in todo:
            nb = adj[ptr[i]:ptr[i + 1]]
            clash = nb[(old[nb] < 0) & (color[nb] == color[i]) & (key[nb] > key[i])]
            if clash.size:
                color[i] = -2
        color[color == -2] = -1
    return color, rounds


def color(rp, ci, seed=0, wrong=None):
    """(color int32, perm int32, color_ptr int32, info): info holds colors, rounds, largest and smallest."""
    assert wrong is None or wrong in WRONG
    n = len(rp) - 1
    ptr, adj = adjacency(rp, ci, symmetric=wrong != "rows_only")
    key = np.arange(n, dtype=np.uint32) if wrong == "key_i" else keys(n, seed)
    if wrong == "stale":
        col, rounds = _stale(n, ptr, adj, key)
    else:
        col = np.full(n, -1, np.int64)
        rnd = np.zeros(n, np.int64)
        for i in np.argsort(key)[::-1]:
            nb = adj[ptr[i]:ptr[i + 1]]
            nb = nb[key[nb] > key[i]]
            col[i] = _mex(col[nb])
            rnd[i] = 1 + (rnd[nb].max() if nb.size else 0)
        rounds = int(rnd.max()) if n else 0
    colors = int(col.max()) + 1 if n else 0
    perm = np.lexsort((np.arange(n), col)).astype(np.int32)
    sizes = np.bincount(col, minlength=colors) if n else np.zeros(0, np.int64)
    color_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    info = {"colors": colors, "rounds": rounds, "largest": int(sizes.max()) if n else 0, "smallest": int(sizes.min()) if n else 0}
    return col.astype(np.int32), perm, color_ptr, info


def is_proper(rp, ci, col):
    """No stored off-diagonal entry joins two rows of one colour."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    off = row != ci
    return bool(np.all(np.asarray(col)[row[off]] != np.asarray(col)[ci[off]]))


def inverse(perm):
    inv = np.empty(len(perm), np.int64)
    inv[np.asarray(perm, np.int64)] = np.arange(len(perm))
    return inv


def permute(rp, ci, va, row_perm=None, col_perm=None, cols=None):
    """(row_ptr int32, col_idx int32, vals float32 with A's bits, map uint32) of B = P A Q^T."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    va = np.asarray(va, f32)
    n = len(rp) - 1
    cols = n if cols is None else cols
    row_perm = np.arange(n) if row_perm is None else np.asarray(row_perm, np.int64)
    inv_col = np.arange(cols) if col_perm is None else inverse(col_perm)
    inv_row = inverse(row_perm)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    pos = np.arange(ci.size, dtype=np.int64)
    by = np.lexsort((pos, inv_col[ci], inv_row[row]))
    brp = np.concatenate([[0], np.cumsum(np.diff(rp)[row_perm])]).astype(np.int32)
    return brp, inv_col[ci][by].astype(np.int32), va[by], by.astype(np.uint32)


def depth(rp, ci, uplo):
    """The levels of one triangle's dependency graph (tests/_trsv.py: a serial peel by the definition)."""
    return int(T.levels(rp, ci, uplo).max()) + 1 if len(rp) > 1 else 0


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _csr(rows_of, seed=0):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows_of])]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, np.int32) for r in rows_of] + [np.zeros(0, np.int32)]).astype(np.int32)
    va = (rng.uniform(0.5, 1.5, ci.size) * rng.choice([-1.0, 1.0], ci.size)).astype(f32)
    return len(rows_of), rp, ci, va


@functools.lru_cache(maxsize=None)
def clique_case(n=70):
    """Every row stores every column: n colours in n rounds, and the window of 64 colours slides."""
    return _csr([np.arange(n)] * n, 1)


@functools.lru_cache(maxsize=None)
def star_case(leaves=5000):
    """Row 0 stores every column, every other row its diagonal and column 0: a centre of 2 * leaves + 2 neighbour entries."""
    return _csr([np.arange(leaves + 1)] + [[0, j] for j in range(1, leaves + 1)], 2)


@functools.lru_cache(maxsize=None)
def boundary_case():
    """Rows 0, 1 and 2 hold exactly 31, 32 and 33 neighbour entries (A's and its transpose's counted together): about half stored in
    the row itself, the others in the rows they point to."""
    n = 200
    rows = [[] for _ in range(n)]
    nxt = 3
    for i in range(3):
        want = 31 + i
        for _ in range(want // 2):
            rows[i].append(nxt)
            nxt += 1
        for _ in range(want - want // 2):
            rows[nxt].append(i)
            nxt += 1
    return _csr(rows, 3)


@functools.lru_cache(maxsize=None)
def upper_case(n=300):
    """Strictly upper-triangular: the row of the larger index finds every neighbour through the transpose only."""
    rng = np.random.default_rng(21)
    return _csr([rng.integers(i + 1, n, 4) if i + 1 < n else [] for i in range(n)], 4)


@functools.lru_cache(maxsize=None)
def unsorted_case():
    """tests/_trsv.py's generic matrix: unsorted rows with repeated columns and long rows."""
    return T.generic_case()[:4]


@functools.lru_cache(maxsize=None)
def empty_case(n=300):
    return _csr([[] for _ in range(n)])


@functools.lru_cache(maxsize=None)
def rectangular_case(rows=256, cols=384):
    rng = np.random.default_rng(31)
    n, rp, ci, va = _csr([rng.integers(0, cols, int(rng.integers(0, 12))) for _ in range(rows)], 5)
    return rows, cols, rp, ci, va


LENGTHS = (0, 1, 63, 64, 65, 4095, 4096)


@functools.lru_cache(maxsize=None)
def lengths_case(longest=4096, cols=5000):
    """One row of each length of LENGTHS (and of `longest` when it is none of them), unsorted with repeated columns, then 40 short
    rows; 5000 columns.  Its values hold a NaN with a payload and -0.0."""
    rng = np.random.default_rng(32)
    lens = list(LENGTHS) + ([longest] if longest not in LENGTHS else []) + [int(rng.integers(0, 10)) for _ in range(40)]
    n, rp, ci, va = _csr([rng.integers(0, cols, m) for m in lens], 6)
    va = va.copy()
    va.view(np.uint32)[1] = 0x7FC01234
    va[2] = f32(-0.0)
    return n, cols, rp, ci, va


def color_cases(pkg):
    """name -> (n, rp, ci): every pattern the colouring tests run."""
    cases = {"generic": G.generic_case(), "stairs": G.stairs_case(), "tridiagonal": G.tridiagonal_case(), "fan": G.fan_case(),
             "arrow": G.arrow_case(), "stencil8": G.stencil_case(pkg, 8), "clique70": clique_case(), "star5000": star_case(),
             "boundary": boundary_case(), "upper": upper_case(), "unsorted": unsorted_case(), "diagonal": G.diagonal_case(500),
             "empty": empty_case(), "rows0": _csr([]), "rows1": _csr([[0]])}
    return {k: v[:3] for k, v in cases.items()}
