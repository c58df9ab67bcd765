"""What a tiled workgroup does before its row sums -- which chunk it takes, when it issues the x window, where a lane's second
segment bounds come from -- must not show in y: every case here is held to the numpy statement of the order
(tests/_tiled_order.py) on raw uint32 views, no tolerance, no row left out, y pre-filled with NaN.

Order.  The mixed launch runs its chunks in one of two orders (SPMV_TILED_ORDER): `lists` -- the 32-bit
chunks first, then the sorted, then the 16-bit ones, each kind through its chunk list -- or `identity` -- workgroup b takes
chunk xcd_chunk(b) whatever its kind, no list read, the ragged last chunk swapped to the front of its XCD's range.  Problems
of 5, 8, 11 and 27 chunks (fewer than the 8 XCDs, exactly 8, remainders 3 and 3 of another quotient) in which all chunks have
16-bit columns but two or three in the middle and the first or the last full one: those span 100 000 columns, so they are
sorted under the default SPMV_SORTED_FROM and take the 32-bit body under SPMV_SORTED_FROM=0.  With and without a ragged last
chunk; no row ends on a chunk boundary, so rows reach into and out of every chunk of another kind.  Each problem runs forced
`identity` and forced `lists`; the plan's report (spmv_csr_plan_chunk_order) must name the forced order.  (Where fewer than
half of the chunks would keep 16-bit columns -- 5 chunks under SPMV_SORTED_FROM=0 -- the plan drops the 16-bit copy, every
chunk takes the 32-bit body in a launch of its own kind and the report says so: 0.)  `auto` must pick identity on a
27-chunk problem in which 3 chunks are of another kind (at most one chunk in eight: the shipped rule, kIdentityShare) and
lists where a quarter of the chunks or more are sorted (3 of 8).

Second trip.  Chunks in which exactly B + 1, B + 2, 2 B and 2 B + 1 segments exist (B the workgroup size; segment 0 is the
head): one lane, two lanes and all lanes take a second trip over the segments, and lane 0 a third.  Each with a head and
without (a row boundary exactly on the chunk boundary), rows of 1..8 nonzeros, one chunk with a 16-lane and a wavefront
segment among the rows of the second trip, the last pattern as the last full chunk; with a ragged chunk behind (the mixed
launch) and without (the lean 16-bit kernel).

Window.  A 16-bit chunk whose window ends at the last column of x, cols not a multiple of 4 (the element-wise copy), and one
whose window is the whole LDS region (wlen == region).

One order problem also runs through spmv_csr_run_vals16 (bf16 values): it shares the bodies.
"""
import re

import numpy as np
import pytest

import _tiled_order as TO

pytestmark = pytest.mark.gpu

KNOBS = ("SPMV_TILED_BLOCK", "SPMV_COL16", "SPMV_SORTED_FROM", "SPMV_PERSIST", "SPMV_MAXPASS", "SPMV_AUTOTUNE", "SPMV_BLOCKS",
         "SPMV_TILED_ORDER")
WIDE = 100_000        # columns a wide chunk spans: above 65 535 (no 16-bit offsets), below 2^18 (what a sorted word holds)
NARROW = 2048         # span of a 16-bit chunk: inside one LDS window at every workgroup size (4832 floats at 256 threads)
ORDER_NONE, ORDER_LISTS, ORDER_IDENTITY = 0, 1, 2     # spmv_csr_plan_chunk_order
REGION = {256: 4832, 512: 9664, 1024: 19328}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_garbage():
    """Later modules compare torch's allocated bytes before and after a call: collect what this module left unreferenced."""
    yield
    import gc
    gc.collect()


def _field(plan, name):
    m = re.search(rf"\b{name}=(\d+)", plan)
    assert m, (name, plan)
    return int(m.group(1))


def _rows_off_the_boundaries(nnz, T, rng, longest=40):
    """row_ptr of rows of 1..longest nonzeros that sum to nnz, none of which ends on a multiple of T inside (0, nnz)."""
    ln = rng.integers(1, longest + 1, nnz // 8 + 2)
    rp = np.concatenate([[0], np.cumsum(ln)])
    rp = rp[rp < nnz]
    rp = rp[(rp % T != 0) | (rp == 0)]
    return np.append(rp, nnz).astype(np.int32)


class OrderProblem:
    def __init__(self, block, nchunks, where, ragged, nmid=None):
        rng = np.random.default_rng(7 * block + 100 * nchunks + (1 if where == "first" else 2) + (10 if ragged else 0))
        T = 16 * block
        nfull = nchunks - (1 if ragged else 0)
        self.nnz = nfull * T + (T // 3 + 5 if ragged else 0)
        m = nfull // 2
        if nmid is None:
            nmid = 2 if nchunks < 11 else 3
        mids = [m - 1, m] if nmid == 2 else [m - 1, m, m + 2]
        self.wide = sorted(set(mids + [0 if where == "first" else nfull - 1]))
        self.nfull, self.nchunks, self.block, self.T = nfull, nchunks, block, T
        self.cols = WIDE + 3
        self.rp = _rows_off_the_boundaries(self.nnz, T, rng)
        self.rows = len(self.rp) - 1
        ci = np.empty(self.nnz, np.int32)
        for c in range(nchunks):
            k0, k1 = c * T, min((c + 1) * T, self.nnz)
            if c in self.wide:
                ci[k0:k1] = rng.integers(0, WIDE, k1 - k0)
                ci[k0 + 5], ci[k0 + 6] = WIDE - 1, 0
            else:
                lo = (c * 3988) % (self.cols - NARROW)
                ci[k0:k1] = rng.integers(lo, lo + NARROW, k1 - k0)
        self.ci = ci
        self.va = TO.general_values(self.nnz, rng)
        self.x = TO.general_values(self.cols, rng)
        self._want = {}

    def want(self, vals=None):
        key = "f32" if vals is None else "16"
        if key not in self._want:
            va = self.va if vals is None else vals
            self._want[key] = TO.tiled_spmv(self.rp, va * self.x[self.ci], self.T)[0]
        return self._want[key]


def _run(capi, gpu, monkeypatch, P, block, env, vals16=None):
    """y of SPMV_TILED at workgroup size `block` under `env`, with the plan line and the order report."""
    import torch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPMV_TILED_BLOCK", str(block))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = [torch.from_numpy(a).to(gpu) for a in (P.rp, P.ci, P.va, P.x)]
    A = capi.CsrMatrix.from_device(P.rows, P.cols, dev[0], dev[1], dev[2])
    try:
        A.plan(capi.TILED)
        plan = A.plan_describe(capi.TILED)
        order = A.plan_chunk_order(capi.TILED)
        y = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
        if vals16 is None:
            A.run(capi.TILED, dev[3], y)
        else:
            A.run_vals16(capi.TILED, vals16, dev[3], y)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
    finally:
        A.close()
    assert _field(plan, "block") == block, plan
    return got, plan, order


def _same_bits(got, want, what):
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} rows differ in a bit; first rows {bad[:6]}: {got[bad[:6]]} against {want[bad[:6]]}"


@pytest.mark.parametrize("shape", [("first", True), ("last", False), ("last", True), ("first", False)], ids=lambda s: f"{s[0]}-{'ragged' if s[1] else 'full'}")
@pytest.mark.parametrize("nchunks", [5, 8, 11, 27])
@pytest.mark.parametrize("block", [256, 512, 1024])
def test_both_chunk_orders_give_the_documented_sums(pkg, gpu, monkeypatch, block, nchunks, shape):
    capi = pkg.capi
    where, ragged = shape
    P = OrderProblem(block, nchunks, where, ragged)
    want = P.want()
    n16 = P.nfull - len(P.wide)
    for kind, env in (("sorted", {}), ("col32", {"SPMV_SORTED_FROM": "0"})):
        for forced, code in (("identity", ORDER_IDENTITY), ("lists", ORDER_LISTS)):
            got, plan, order = _run(capi, gpu, monkeypatch, P, block, dict(env, SPMV_TILED_ORDER=forced))
            print(f"block={block} chunks={nchunks} wide={P.wide} ragged={ragged} {kind} {forced}: order={order}; {plan}")
            assert _field(plan, "chunks") == nchunks, plan
            dropped = kind == "col32" and 2 * n16 < nchunks      # the plan's rule: too few 16-bit chunks to keep the copy
            assert kind == "sorted" or dropped or n16 > 0
            assert _field(plan, "col16_chunks") == (0 if dropped else n16), plan
            assert _field(plan, "sorted_chunks") == (len(P.wide) if kind == "sorted" else 0), plan
            assert order == (ORDER_NONE if dropped else code), (order, plan)
            _same_bits(got, want, f"{kind} {forced}")


@pytest.mark.parametrize("block", [256, 512, 1024])
def test_auto_order_follows_the_share_of_other_chunks(pkg, gpu, monkeypatch, block):
    capi = pkg.capi
    few = OrderProblem(block, 27, "first", False, nmid=2)     # 3 of 27 chunks sorted: 3 x 8 <= 27
    assert len(few.wide) == 3
    got, plan, order = _run(capi, gpu, monkeypatch, few, block, {})
    assert _field(plan, "sorted_chunks") == 3 and order == ORDER_IDENTITY, (order, plan)
    _same_bits(got, few.want(), "auto, few")
    got, plan, order = _run(capi, gpu, monkeypatch, few, block, {"SPMV_TILED_ORDER": "auto"})
    assert order == ORDER_IDENTITY, (order, plan)
    quarter = OrderProblem(block, 8, "first", False)          # 3 of 8 chunks sorted: a quarter and more
    quarter_sorted = len(quarter.wide)
    assert 4 * quarter_sorted >= 8
    got, plan, order = _run(capi, gpu, monkeypatch, quarter, block, {})
    assert _field(plan, "sorted_chunks") == quarter_sorted and order == ORDER_LISTS, (order, plan)
    _same_bits(got, quarter.want(), "auto, a quarter")


def test_16bit_values_share_the_order(pkg, gpu, monkeypatch):
    import torch
    capi = pkg.capi
    block = 512
    P = OrderProblem(block, 11, "last", True)
    v16 = torch.from_numpy(P.va).to(gpu).to(torch.bfloat16)
    want = P.want(v16.to(torch.float32).cpu().numpy())
    for forced, code in (("identity", ORDER_IDENTITY), ("lists", ORDER_LISTS)):
        got, plan, order = _run(capi, gpu, monkeypatch, P, block, {"SPMV_TILED_ORDER": forced}, vals16=v16)
        assert order == code, (order, plan)
        _same_bits(got, want, f"bf16 {forced}")


# ---- the second trip over a chunk's segments ---------------------------------------------------------------------------
def _second_trip_lengths(block, rng):
    """Row lengths, a whole number of chunks: per pattern one filler chunk and one chunk with exactly `segs` segments."""
    T = 16 * block
    out = []

    def chunk(segs, head, special=False):
        m = segs - 1                                   # rows that begin in the chunk
        big = [40, 600] if special else []             # a 16-lane and a wavefront segment, placed in the second trip
        nsmall = m - len(big) - (0 if head else 1)
        if head:
            total = min(T - 7, 5 * nsmall + sum(big))
            small = TO.small_rows(nsmall, total - sum(big), rng)
            rows = small[:block] + big + small[block:]
            assert len(rows) == m and sum(rows) == total
            out.extend([T // 2, T // 2 + (T - total)] + rows)      # the second row is the head: T - total words of it
        else:
            total = min(T - 9, 8 * nsmall + sum(big)) if nsmall * 8 + sum(big) < T else T
            small = TO.small_rows(nsmall, min(total, 8 * nsmall + sum(big)) - sum(big), rng) if total < T else TO.small_rows(nsmall, 8 * nsmall, rng)
            first = T - sum(small) - sum(big)          # a row that begins exactly on the chunk boundary and fills the rest
            rows = ([first] if first > 0 else []) + small[:block] + big + small[block:]
            if first <= 0:                             # 2 B + 1 segments of 8: one more small row instead
                rows = TO.small_rows(m, T, rng)
            assert len(rows) == m and sum(rows) == T, (len(rows), m, sum(rows), T)
            out.extend([T] + rows)

    for segs in (block + 1, block + 2, 2 * block, 2 * block + 1):
        chunk(segs, head=True)
        chunk(segs, head=False)
    chunk(block + 2 + 2, head=True, special=True)
    chunk(2 * block + 1, head=True)                    # ... and once as the last full chunk
    return out


class TripProblem:
    def __init__(self, block, ragged):
        rng = np.random.default_rng(31 * block + (1 if ragged else 0))
        T = 16 * block
        lengths = _second_trip_lengths(block, rng)
        assert sum(lengths) % T == 0
        if ragged:
            lengths = lengths + [3, 8, 1, T // 5]
        self.rp = TO.row_ptr_of(lengths)
        self.rows, self.cols, self.nnz, self.T = len(lengths), TO.COLS, int(self.rp[-1]), T
        self.ci = rng.integers(1, TO.COLS, self.nnz).astype(np.int32)
        self.va = TO.general_values(self.nnz, rng)
        self.x = TO.general_values(TO.COLS, rng)
        lb = TO.chunk_rows(self.rp, -(-self.nnz // T), T)
        self.segments = [int(lb[c + 1] - lb[c]) + 1 for c in range(self.nnz // T)]

    def want(self):
        return TO.tiled_spmv(self.rp, self.va * self.x[self.ci], self.T)[0]


@pytest.mark.parametrize("ragged", [True, False], ids=["mixed", "lean"])
@pytest.mark.parametrize("block", [256, 512, 1024])
def test_second_trip_over_the_segments(pkg, gpu, monkeypatch, block, ragged):
    P = TripProblem(block, ragged)
    for segs in (block + 1, block + 2, 2 * block, 2 * block + 1, block + 4):
        assert segs in P.segments, (segs, P.segments)
    assert P.segments[-1] == 2 * block + 1
    want = P.want()
    for forced in ("identity", "lists"):
        got, plan, order = _run(pkg.capi, gpu, monkeypatch, P, block, {"SPMV_TILED_ORDER": forced, "SPMV_SORTED_FROM": "0"})
        assert _field(plan, "col16_chunks") == P.nnz // P.T, plan
        _same_bits(got, want, f"second trip, {forced}")


# ---- the window ----------------------------------------------------------------------------------------------------------
class WindowProblem:
    def __init__(self, block):
        rng = np.random.default_rng(53 * block)
        T = 16 * block
        region = REGION[block]
        self.cols = 24_003                                  # not a multiple of 4
        nchunks = 4
        self.nnz, self.T = nchunks * T, T
        self.rp = _rows_off_the_boundaries(self.nnz, T, rng, longest=24)
        self.rows = len(self.rp) - 1
        ci = rng.integers(100, 100 + NARROW, self.nnz).astype(np.int32)
        # chunk 1: the window is the whole region: first column a multiple of 4, last column region - 1 behind it
        ci[T:2 * T] = rng.integers(400, 400 + region, T)
        ci[T + 3], ci[T + 4] = 400, 400 + region - 1
        # chunk 2: the window ends at the last column of x
        ci[2 * T:3 * T] = rng.integers(self.cols - 1500, self.cols, T)
        ci[2 * T + 9] = self.cols - 1
        self.ci = ci
        self.va = TO.general_values(self.nnz, rng)
        self.x = TO.general_values(self.cols, rng)

    def want(self):
        return TO.tiled_spmv(self.rp, self.va * self.x[self.ci], self.T)[0]


@pytest.mark.parametrize("block", [256, 512, 1024])
def test_window_at_the_end_of_x_and_as_wide_as_the_region(pkg, gpu, monkeypatch, block):
    P = WindowProblem(block)
    got, plan, _ = _run(pkg.capi, gpu, monkeypatch, P, block, {})
    assert _field(plan, "col16_chunks") == 4 and _field(plan, "staged_single") == 4 and _field(plan, "region") == REGION[block], plan
    _same_bits(got, P.want(), "window")
