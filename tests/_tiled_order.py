"""The order of the row sums of SPMV_TILED (and SPMV_ADAPTIVE), stated in numpy: what the kernels of
spmv-test_amd/csrc/kernels_adaptive.hip must give bit for bit, written from the description of the order and not from
the device code.

The nonzeros are cut into chunks of T = 16 x workgroup size in storage order.  Chunk c holds the fp32 products
p[k] = vals[k] * x[col_idx[k]] of its nonzeros at the PADDED positions i + (i >> 5) (i: position in the chunk) of a buffer
whose every 33rd word, the pad word, is +0.  Its segments are the head -- the part of a row that began in an earlier chunk,
summed into carry[c] -- and the rows that begin in it (first row: the first r with row_ptr[r] >= c T), each cut at the
chunk's end.  A segment [s, e) is summed over the padded words [pad(s), pad(e)), pad words included:

  e - s <= 32      one lane, left to right from +0;
  33 .. 512        sixteen partials, partial l = +0 + w[pad(s) + l] + w[pad(s) + l + 16] + ..., then the tree
                   a[l] += a[l + 8] (l < 8), a[l] += a[l + 4] (l < 4), += a[l + 2], += a[l + 1]: the result is a[0];
  e - s > 512      sixty-four lanes; lane l walks k = pad(s) + l in steps of 128: a0 += w[k], a1 += w[k + 64] while
                   k + 64 < pad(e), then a0 += w[k] if k < pad(e); a = a0 + a1; the tree over 32, 16, 8, 4, 2, 1.

A row that goes on past its chunk is finished by the fix-up: y[r] = ((y[r] + carry[c + 1]) + carry[c + 2]) + ... over the
chunks the row reaches into.
"""
import numpy as np

f32 = np.float32
SHORT, HUGE, GROUP, WAVE = 32, 512, 16, 64      # kShortSeg, kHugeSeg, the lane group, the wavefront


def pad(i):
    return i + (i >> 5)


def chunk_rows(row_ptr, nchunks, T):
    """lb[c] = first row r with row_ptr[r] >= c T (c < nchunks), lb[nchunks] = rows."""
    rows = len(row_ptr) - 1
    lb = np.searchsorted(np.asarray(row_ptr, np.int64), np.arange(nchunks, dtype=np.int64) * T, side="left")
    return np.append(np.minimum(lb, rows), rows)


def _tree(a, first):
    o = first
    while o >= 1:
        a[:o] = a[:o] + a[o:2 * o]
        o //= 2
    return a[0]


def segment_sum(w, s, e):
    """The sum of products [s, e) of a chunk whose padded words are w."""
    ps, pe = pad(s), pad(e)
    if e - s <= SHORT:
        acc = f32(0.0)
        for k in range(ps, pe):
            acc = f32(acc + w[k])
        return acc
    if e - s <= HUGE:
        a = np.zeros(GROUP, f32)
        for k0 in range(ps, pe, GROUP):
            n = min(GROUP, pe - k0)
            a[:n] = a[:n] + w[k0:k0 + n]
        return _tree(a, GROUP // 2)
    a0, a1 = np.zeros(WAVE, f32), np.zeros(WAVE, f32)
    for l in range(WAVE):
        k = ps + l
        while k + WAVE < pe:
            a0[l] = a0[l] + w[k]
            a1[l] = a1[l] + w[k + WAVE]
            k += 2 * WAVE
        if k < pe:
            a0[l] = a0[l] + w[k]
    return _tree(a0 + a1, WAVE // 2)


def tiled_spmv(row_ptr, prod, T):
    """y of the TILED order for products `prod` (fp32, storage order) and chunks of T nonzeros; also (carry, classes) where
    classes counts the short / long / huge segments summed."""
    row_ptr = np.asarray(row_ptr, np.int64)
    prod = np.ascontiguousarray(prod, f32)
    rows, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    assert prod.shape == (nnz,) and T % 32 == 0
    nchunks = (nnz + T - 1) // T
    y = np.zeros(rows, f32)
    carry = np.zeros(nchunks, f32)
    classes = [0, 0, 0]
    lb = chunk_rows(row_ptr, nchunks, T)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(nchunks):
            base = c * T
            n = min(T, nnz - base)
            lim = base + n
            w = np.zeros(pad(T) + 1, f32)
            idx = np.arange(n)
            w[idx + (idx >> 5)] = prod[base:lim]

            def put(s, e):
                classes[0 if e - s <= SHORT else 1 if e - s <= HUGE else 2] += 1
                return segment_sum(w, s, e)
            carry[c] = put(0, int(min(row_ptr[lb[c]], lim)) - base)
            for r in range(lb[c], lb[c + 1]):
                y[r] = put(int(row_ptr[r]) - base, int(min(row_ptr[r + 1], lim)) - base)
        for c in range(nchunks - 1):
            if lb[c + 1] == lb[c]:
                continue
            r = lb[c + 1] - 1
            endp = int(row_ptr[r + 1])
            if endp <= (c + 1) * T:
                continue
            s = y[r]
            c2 = c + 1
            while c2 * T < endp:
                s = f32(s + carry[c2])
                c2 += 1
            y[r] = s
    return y, carry, classes


# ---- the row-length patterns of tests/test_gpu_tiled_rowsums.py and tests/test_tiled_order_host.py ---------------------
LONG_BATCH = 4      # words a lane of a 16-lane group reads ahead in the 33..512 loop of the shipped kernel

EDGE = [0, 1, 15, 16, 17, 18, 31, 32, 33]
BATCH = [16 * LONG_BATCH - 1, 16 * LONG_BATCH, 16 * LONG_BATCH + 1, 32 * LONG_BATCH - 1, 32 * LONG_BATCH, 32 * LONG_BATCH + 1]
WIDE = [511, 512, 513, 575, 576, 577, 639, 640, 641]


def shifted(lengths, shifts=range(34)):
    """`lengths` once per shift s: a row of s nonzeros in front (none for s = 0) and a row behind that fills up to the next
    multiple of 32, so that the copy for shift s starts s words behind a pad-word boundary of its chunk when the whole list
    starts on one (chunks are multiples of 32)."""
    out = []
    for s in shifts:
        grp = ([s] if s else []) + list(lengths)
        fill = -sum(grp) % 32
        out += grp + [fill + 64]          # 64..95: a long segment of its own
    return out


def small_rows(nrows, total, rng):
    """nrows lengths in 1..8 that sum to total (nrows <= total <= 8 nrows)."""
    assert nrows <= total <= 8 * nrows
    ln = np.ones(nrows, np.int64)
    left = total - nrows
    while left:
        i = rng.integers(0, nrows)
        add = min(left, 8 - ln[i], int(rng.integers(1, 8)))
        ln[i] += add
        left -= add
    return [int(v) for v in ln]


def chunk_patterns(block, rng):
    """Lists of row lengths that are whole numbers of chunks of T = 16 block nonzeros each."""
    T = 16 * block
    pats = {}
    # one row that fills a chunk exactly
    pats["fills_chunk"] = [T] + small_rows(2 * block, T, rng)
    # rows that end in the next chunk with a head of 40 (a 16-lane head, one-term fix-up) and of 9 words (a one-lane head),
    # and one that spans three chunks: 520 words where it begins, a head that fills a chunk (a wavefront head) and a head of
    # 300, a two-term fix-up
    pats["spans_three"] = [T - 5, 5 + 40, T - 40 - 520, 520 + T + 300, T - 300 - 9, 9 + 9, T - 9]
    # a chunk in which block - 1, block, block + 1 and 2 block + 3 rows of lengths 1..8 begin: the second and third trip
    # over the segments of a chunk (segment 0 is the head: block rows are block + 1 segments).  Fewer than 2 block rows of
    # at most 8 cannot fill 16 block words: the row in front reaches in and takes the rest of the chunk as its head.
    for nr in (block - 1, block, block + 1, 2 * block + 3):
        total = T if 8 * nr >= T else 5 * nr
        pats[f"rows_{nr}"] = [T // 2, T // 2 + (T - total)] + small_rows(nr, total, rng)
    # more long segments than one round of block / 16 groups takes, and fewer than one round
    nlong = T // 36
    pats["many_long"] = [36] * nlong + [T - 36 * nlong + T]
    pats["few_long"] = [40, 100, 33] + small_rows(2 * block, T - 173, rng)
    return pats


def row_ptr_of(lengths):
    rp = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(np.asarray(lengths, np.int64), out=rp[1:])
    return rp


def general_values(nnz, rng):
    """fp32 values of mixed exponents and signs: the order of the additions decides the low bits."""
    return (rng.standard_normal(nnz) * np.exp2(rng.integers(-12, 13, nnz))).astype(f32)


CASES = ("lengths", "chunks")
COLS = 4096                     # every chunk's column span fits one LDS window: 16-bit columns unless a knob says otherwise
SPECIAL = (5, 40, 600)          # a short, a long and a wavefront segment


class Problem:
    """One CSR matrix and x of a case at one workgroup size, with what the rows are there for."""

    def __init__(self, case, block):
        rng = np.random.default_rng(1000 * CASES.index(case) + block)
        T = 16 * block
        special = {}
        if case == "lengths":
            # every length on both sides of a class or batch boundary, at every phase of the pad words
            lengths = shifted(EDGE + BATCH + WIDE)
        else:
            lengths = []
            pats = chunk_patterns(block, rng)
            for name, v in pats.items():
                assert sum(v) % T == 0, name
                lengths += v
            for name in (f"rows_{block + 1}", f"rows_{2 * block + 3}"):
                # the same chunks, every row s words later.  (The "lengths" case takes every shift 0..33: a class or batch
                # boundary depends on a segment's phase against the pad words.  Here the rows of 1..8 already begin at every
                # phase inside their chunk, and the shift moves which lane and wave a row falls to and what the head holds:
                # two shifts, or 34 copies of these chunks would be millions of nonzeros.)
                for s in (1, 33):
                    lengths += [s] + pats[name] + [T - s]
            # rows whose products are all -0.0, and rows that hold an Inf, beside finite rows
            for kind in ("negzero", "posinf", "neginf"):
                for ln in SPECIAL:
                    special[len(lengths)] = kind
                    lengths += [ln, 7]
        lengths += [-sum(lengths) % T + 3]        # a ragged last chunk
        self.case, self.block, self.lengths = case, block, lengths
        self.rp = row_ptr_of(lengths)
        self.rows, self.cols, self.nnz = len(lengths), COLS, int(self.rp[-1])
        self.ci = rng.integers(1, COLS, self.nnz).astype(np.int32)
        self.va = general_values(self.nnz, rng)
        self.x = general_values(COLS, rng)
        self.x[0] = 1.0
        for r, kind in special.items():
            k0, k1 = int(self.rp[r]), int(self.rp[r + 1])
            if kind == "negzero":
                self.ci[k0:k1], self.va[k0:k1] = 0, -0.0
            else:
                k = k0 + (k1 - k0) // 2
                self.ci[k], self.va[k] = 0, np.inf if kind == "posinf" else -np.inf
        self.special = special
        self.prod = self.va * self.x[self.ci]     # one fp32 multiplication per nonzero
        self._want = {}

    def want(self, T):
        """(y, carry, classes) of the documented order for chunks of T nonzeros, computed once."""
        if T not in self._want:
            self._want[T] = tiled_spmv(self.rp, self.prod, T)
        return self._want[T]


_problems = {}


def problem(case, block):
    if (case, block) not in _problems:
        _problems[case, block] = Problem(case, block)
    return _problems[case, block]
