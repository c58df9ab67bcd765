"""The contract of spmv_csr_select_topk / spmv_csr_select_threshold (include/spmv_hip.h "selection") in numpy: what the GPU
tests compare the library's bytes with.  Everything is exact: integer keys, no sum, no tolerance.

    key(s)     NaN -> 0; else u = bits(s + 0.0f), ~u if its sign bit is set, else u | 0x80000000   (abs: from |s|)
    ranking    inside a row by (key descending, storage position ascending)
    topk       the first min(k, len) of every row's ranking
    threshold  s >= threshold (|s| >= threshold) as an IEEE comparison
    result     the kept positions of a row ascending; col_idx, vals (bits) and map follow the positions
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
SUBNORMAL = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


# two NaN payloads of each sign, +-Inf, +-0, +-smallest subnormal, +-FLT_MAX
SPECIAL_BITS = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                         0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
SPECIAL = f32(SPECIAL_BITS)


def keys(score, abs_=False):
    """The 32-bit key of every score (uint32)."""
    s = np.ascontiguousarray(score, np.float32)
    if abs_:
        s = (s.view(np.uint32) & np.uint32(0x7FFFFFFF)).view(np.float32)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        u = (s + np.float32(0.0)).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = 0
    return k


def _result(rows, rp, ci, vals, keep):
    rp = np.asarray(rp, np.int64)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    pos = np.flatnonzero(keep)          # ascending positions: ascending rows, storage order inside a row
    out_rp = np.concatenate([[0], np.cumsum(np.bincount(row_of[pos], minlength=rows))]).astype(np.int32)
    return out_rp, np.asarray(ci, np.int32)[pos], np.asarray(vals, np.float32)[pos], pos.astype(np.uint32)


def host_select_topk(rows, rp, ci, vals, k, score=None, abs_=False):
    """(row_ptr, col_idx, vals, map) of the per-row top-k, vectorised."""
    rp = np.asarray(rp, np.int64)
    nnz = int(rp[-1])
    key = keys(vals if score is None else score, abs_).astype(np.int64)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    pos = np.arange(nnz, dtype=np.int64)
    order = np.lexsort((pos, -key, row_of))            # by row, then key descending, then position
    rank = np.empty(nnz, np.int64)
    rank[order] = pos - rp[row_of[order]]              # place inside the row's ranking
    return _result(rows, rp, ci, vals, rank < k)


def host_select_threshold(rows, rp, ci, vals, threshold, score=None, abs_=False):
    s = np.ascontiguousarray(vals if score is None else score, np.float32)
    if abs_:
        s = (s.view(np.uint32) & np.uint32(0x7FFFFFFF)).view(np.float32)
    with np.errstate(invalid="ignore"):
        keep = s >= np.float32(threshold)
    return _result(rows, rp, ci, vals, keep)


def _naive_key(x, abs_):
    b = int(np.float32(x).view(np.uint32))
    if abs_:
        b &= 0x7FFFFFFF
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0
    if b == 0x80000000:
        b = 0
    return (~b) & 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000


def naive_select(rows, rp, ci, vals, k=None, threshold=None, score=None, abs_=False):
    """The same, row by row in plain Python (deliberately naive: what the vectorised version is checked against)."""
    s = vals if score is None else score
    out_rp, out_ci, out_va, out_map = [0], [], [], []
    for r in range(rows):
        span = list(range(int(rp[r]), int(rp[r + 1])))
        if k is not None:
            ranking = sorted(span, key=lambda p: (-_naive_key(s[p], abs_), p))
            kept = sorted(ranking[:k])
        else:
            kept = []
            for p in span:
                x = float(np.float32(s[p]))
                if abs_:
                    x = abs(x)
                if x >= float(np.float32(threshold)):       # False for a NaN
                    kept.append(p)
        for p in kept:
            out_ci.append(int(ci[p]))
            out_va.append(vals[p])
            out_map.append(p)
        out_rp.append(len(out_ci))
    return (np.array(out_rp, np.int32), np.array(out_ci, np.int32), np.array(out_va, np.float32), np.array(out_map, np.uint32))


def same(a, b):
    """Bit for bit: row_ptr, col_idx, the uint32 view of vals, and the map where both have one."""
    ok = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) \
        and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))
    if len(a) > 3 and len(b) > 3 and a[3] is not None and b[3] is not None:
        ok = ok and np.array_equal(np.asarray(a[3], np.uint32), np.asarray(b[3], np.uint32))
    return ok


def random_csr(rng, rows, cols, lengths, sorted_rows=True):
    """row_ptr, col_idx of rows with the given lengths: distinct sorted columns, or (sorted_rows = False) shuffled with about
    1/8 of the columns repeated."""
    lengths = np.asarray(lengths, np.int64)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.empty(int(rp[-1]), np.int32)
    for r, n in enumerate(lengths):
        n = int(n)
        if n == 0:
            continue
        if n <= cols:
            c = np.sort(rng.choice(cols, n, replace=False))
        else:
            c = np.sort(rng.integers(0, cols, n))
        if not sorted_rows:
            dup = rng.random(n) < 0.125
            c = np.where(dup, c[rng.integers(0, n, n)], c)
            rng.shuffle(c)
        ci[rp[r]:rp[r + 1]] = c
    return rp, ci


def special_scores(rng, n, p_special=0.3, p_tie=0.3):
    """Scores with many specials and many ties."""
    s = rng.standard_normal(n).astype(np.float32)
    tie = rng.random(n) < p_tie
    s[tie] = rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), int(tie.sum()))
    sp = rng.random(n) < p_special
    s[sp] = rng.choice(SPECIAL, int(sp.sum()))
    return s
