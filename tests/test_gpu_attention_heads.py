"""All heads of one pattern in one launch (spmv_csr_attention_forward_heads, _backward_q_heads, _backward_kv_heads and the
holder's heads="batched") on the device.  The claim is bit identity: head y of a _heads call is the single-head call on the
pointers advanced by y strides, so nothing here has a tolerance; every comparison is of raw bits.

One pattern serves most tests: 700 queries x 1200 keys with empty rows, rows of 1 .. 7 entries (inside one step), rows of
9 .. 200 entries, one row of 1100 entries (three pieces) and one key that more than 512 queries list, so that the transpose
has a row in pieces too.  With long rows on A and on T, heads that shared their scratch would not give the single-head bits.

Every operand of a _heads call lives in a buffer of its own between guard bands: outputs start as NaN, the gaps between
rows and between heads hold a guard value that must be intact afterwards, and the gaps of an input hold NaN so that a read
past the width that reached a sum would show.
"""
import ctypes as C

import numpy as np
import pytest

import _exact as E

pytestmark = pytest.mark.gpu

GUARD, GUARD_N = 3.0e35, 1024
SCALE = 2.0 ** -2
ROWS, COLS, HOT = 700, 1200, 7
HEADS = 3
PIECE = 512


def _pattern():
    rng = np.random.Generator(np.random.PCG64(101))
    lengths = np.concatenate([np.zeros(20, np.int64), rng.integers(1, 8, size=520), rng.integers(9, 201, size=159), [1100]])
    lengths = lengths[rng.permutation(len(lengths))]
    assert len(lengths) == ROWS
    rows = []
    for n in lengths:
        c = np.sort(rng.choice(COLS, size=int(n), replace=False))
        if 1 <= n <= 7 and HOT not in c:         # the hot key: in every short row
            c[0] = HOT
            c = np.sort(c)
        rows.append(c)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    s = E.Structure(ROWS, COLS, rp, np.concatenate(rows).astype(np.int32))
    per_key = np.bincount(s.ci, minlength=COLS)
    assert per_key[HOT] > PIECE and (lengths == 0).sum() == 20 and lengths.max() == 1100
    return s, _pieces(lengths), _pieces(per_key)


def _pieces(lengths):
    lengths = np.asarray(lengths, np.int64)
    return int(((lengths[lengths > PIECE] + PIECE - 1) // PIECE).sum())


def _short_pattern():
    rng = np.random.Generator(np.random.PCG64(103))
    lengths = rng.integers(0, 12, size=90)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(70, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    return E.Structure(90, 70, rp, ci)


def _raw(t):
    import torch
    return t.contiguous().view(torch.int32)


class Handles:
    def __init__(self, pkg, s, gpu, heads=None):
        import torch
        self.keep = (torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu),
                     torch.zeros(s.nnz, dtype=torch.float32, device=gpu))
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=False)
        for m in (self.A, self.T):
            if heads is None:
                m.attention_plan()
            else:
                m.attention_plan_heads(heads)

    def close(self):
        self.T.close()
        self.A.close()


class Shared:
    """The pattern, its handles planned for HEADS heads, and the single-head results by (k, kv, seed): computed once."""

    def __init__(self, pkg, gpu):
        self.pkg, self.gpu = pkg, gpu
        self.s, self.pieces_A, self.pieces_T = _pattern()
        self.h = Handles(pkg, self.s, gpu, heads=HEADS)
        self._single = {}

    def data(self, k, kv, seed, heads=HEADS):
        """Per head (Q, K, V, dO), different random numbers in every head."""
        import torch
        gen = torch.Generator(device=self.gpu).manual_seed(seed)
        mk = lambda n, w: torch.randn((heads, n, w), generator=gen, device=self.gpu, dtype=torch.float32)      # noqa: E731
        return dict(Q=mk(ROWS, k), K=mk(COLS, k), V=mk(COLS, kv), dO=mk(ROWS, kv))

    def single(self, k, kv, seed):
        key = (k, kv, seed)
        if key not in self._single:
            d = self.data(k, kv, seed)
            self._single[key] = [single_head(self.h, *(d[n][y] for n in ("Q", "K", "V", "dO"))) for y in range(HEADS)]
        return self._single[key]


@pytest.fixture(scope="module")
def shared(pkg, gpu):
    sh = Shared(pkg, gpu)
    yield sh
    sh.h.close()


def single_head(h, Q, K, V, dO, scale=SCALE):
    """The three single-head calls on contiguous operands into outputs that start as NaN."""
    import torch
    A, T = h.A, h.T
    k, kv = Q.shape[1], V.shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=Q.device)      # noqa: E731
    out = dict(O=nan(A.rows, kv), stats=nan(A.rows, 2), delta=nan(A.rows), dQ=nan(A.rows, k), dK=nan(A.cols, k), dV=nan(A.cols, kv))
    A.attention_forward(Q, K, V, out["O"], out["stats"], scale)
    A.attention_backward_q(Q, K, V, out["O"], dO, out["stats"], out["delta"], out["dQ"], scale)
    T.attention_backward_kv(Q, K, V, dO, out["stats"], out["delta"], out["dK"], out["dV"], scale)
    torch.cuda.synchronize()
    return out


# ---- layouts: (leading dimension of a matrix of w columns, floats from one head to the next) ---------------------------
def _up4(n):
    return (n + 3) // 4 * 4


LAYOUTS = {
    "stacked": lambda heads, rows, w: (_up4(w) + 4, rows * (_up4(w) + 4)),                     # every ld % 4 == 0, stride = rows ld
    "odd_ld": lambda heads, rows, w: (w + 1 + w % 2, _up4(rows * (w + 1 + w % 2))),            # an odd ld: the 4-byte path
    "blocks": lambda heads, rows, w: (heads * _up4(w), _up4(w)),                               # column blocks: stride k, ld heads k
    "padded": lambda heads, rows, w: (_up4(w), rows * _up4(w) + 12),                           # a padded head stride
}


class Guarded:
    """(heads, rows, w) floats at strides (stride, ld, 1) in a flat buffer of its own between guard bands.  Everything that
    is no element holds `gap` (an output: the guard value, which must stay; an input: NaN)."""

    def __init__(self, gpu, heads, rows, w, ld, stride, fill=None):
        import torch
        span = (heads - 1) * stride + (rows - 1) * ld + w
        gap = GUARD if fill is None else float("nan")
        self.buf = torch.full((2 * GUARD_N + span,), gap, dtype=torch.float32, device=gpu)
        self.buf[:GUARD_N] = GUARD
        self.buf[GUARD_N + span:] = GUARD
        self.strides = (stride, ld, 1)
        self.view = torch.as_strided(self.buf, (heads, rows, w), self.strides, GUARD_N)
        self.view.copy_(fill if fill is not None else torch.full((heads, rows, w), float("nan"), device=gpu))
        own = torch.zeros_like(self.buf, dtype=torch.bool)
        torch.as_strided(own, (heads, rows, w), self.strides, GUARD_N).fill_(True)
        self.gaps = ~own
        self.is_output = fill is None

    def intact(self):
        g = self.buf[self.gaps]
        n = GUARD_N
        bands = bool((self.buf[:n] == GUARD).all()) and bool((self.buf[-n:] == GUARD).all())
        return bands and (bool((g == GUARD).all()) if self.is_output else True)


def heads_run(h, d, layout, scale=SCALE, shared_kv=False):
    """The three _heads calls on the operands d (per head, (heads, n, w)) laid out by `layout`; returns the outputs as
    (heads, ...) views and asserts that nothing but the outputs' own elements was written."""
    import torch
    A, T = h.A, h.T
    gpu = d["Q"].device
    heads, k, kv = d["Q"].shape[0], d["Q"].shape[2], d["V"].shape[2]
    lay = LAYOUTS[layout]
    made = []

    def mat(rows, w, fill=None):
        ld, stride = lay(heads, rows, w)
        g = Guarded(gpu, heads, rows, w, ld, stride, fill)
        made.append(g)
        return g.view

    def vec(rows, inner, pad):
        g = Guarded(gpu, heads, rows, inner, inner, rows * inner + pad)
        made.append(g)
        return g.view if inner > 1 else g.view[:, :, 0]

    Q, dO = mat(A.rows, k, d["Q"]), mat(A.rows, kv, d["dO"])
    if shared_kv:       # one K and one V for all heads: stride(0) == 0
        K, V = (mat(A.cols, w, d[n][:1])[0].unsqueeze(0).expand(heads, -1, -1) for n, w in (("K", k), ("V", kv)))
    else:
        K, V = mat(A.cols, k, d["K"]), mat(A.cols, kv, d["V"])
    pad = 0 if layout == "stacked" else 6
    out = dict(O=mat(A.rows, kv), stats=vec(A.rows, 2, pad), delta=vec(A.rows, 1, pad + 1 if pad else 0), dQ=mat(A.rows, k),
               dK=mat(A.cols, k), dV=mat(A.cols, kv))
    A.attention_forward_heads(Q, K, V, out["O"], out["stats"], scale)
    A.attention_backward_q_heads(Q, K, V, out["O"], dO, out["stats"], out["delta"], out["dQ"], scale)
    T.attention_backward_kv_heads(Q, K, V, dO, out["stats"], out["delta"], out["dK"], out["dV"], scale)
    torch.cuda.synchronize()
    assert all(g.intact() for g in made), f"{layout}: a pass wrote outside its outputs' own elements"
    return out


def assert_heads_equal(got, want, tag):
    import torch
    for name in ("O", "stats", "delta", "dQ", "dK", "dV"):
        for y, ref in enumerate(want):
            assert torch.equal(_raw(got[name][y]), _raw(ref[name])), f"{tag}: {name} of head {y} differs from the single-head call"


# ---- bit identity ------------------------------------------------------------------------------------------------------
SHAPES = [(3, 2), (8, 6), (12, 16), (24, 32), (40, 64)]         # V = 1, 2, 4, 8, 16; the widest width ends a slice or not


@pytest.mark.parametrize("layout", ["stacked", "odd_ld"])
@pytest.mark.parametrize("k,kv", SHAPES, ids=[f"k{k}-kv{kv}" for k, kv in SHAPES])
def test_heads_equal_three_single_head_calls_bit_for_bit(shared, k, kv, layout):
    d = shared.data(k, kv, seed=200 + k)
    got = heads_run(shared.h, d, layout)
    assert_heads_equal(got, shared.single(k, kv, seed=200 + k), f"k={k} kv={kv} {layout}")
    # a head is not another head: the data differ per head, so do the results
    assert not bool((got["O"][0] == got["O"][1]).all())


# ---- layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["blocks", "padded"])
@pytest.mark.parametrize("k,kv", [(12, 16), (6, 40)], ids=["k12-kv16", "k6-kv40"])
def test_heads_layouts_column_blocks_and_padded_strides(shared, k, kv, layout):
    """(stacked operands and an odd ld run in the test above, between the same guard bands.)  At k = 12, kv = 16 the column
    blocks are exactly stride = k, ld = heads k; at k = 6 a block is 8 floats wide and its last two columns are guard."""
    d = shared.data(k, kv, seed=300 + k)
    got = heads_run(shared.h, d, layout)
    assert_heads_equal(got, shared.single(k, kv, seed=300 + k), f"k={k} kv={kv} {layout}")
    if layout == "blocks" and k % 4 == 0:
        assert got["dQ"].stride() == (k, HEADS * k, 1) and got["O"].stride() == (kv, HEADS * kv, 1)


# ---- shared inputs -----------------------------------------------------------------------------------------------------
def test_heads_share_one_k_and_v_at_stride_zero(shared):
    k, kv = 12, 16
    d = shared.data(k, kv, seed=401)
    got = heads_run(shared.h, d, "stacked", shared_kv=True)
    want = [single_head(shared.h, d["Q"][y], d["K"][0], d["V"][0], d["dO"][y]) for y in range(HEADS)]
    assert_heads_equal(got, want, "shared K and V")     # (dK and dV per head: the caller sums them)


# ---- a single head -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stacked", "odd_ld"])
def test_one_head_through_the_heads_calls_is_the_plain_call(shared, layout):
    k, kv = 24, 32
    d = {n: t[:1] for n, t in shared.data(k, kv, seed=200 + k).items()}
    got = heads_run(shared.h, d, layout)
    assert_heads_equal(got, shared.single(k, kv, seed=200 + k)[:1], f"heads = 1 {layout}")


# ---- the plan ----------------------------------------------------------------------------------------------------------
def test_heads_plan_grows_and_more_heads_than_planned_are_refused(shared, pkg, gpu):
    import torch
    capi = pkg.capi
    k, kv = 12, 16
    long = Handles(pkg, shared.s, gpu)                      # spmv_csr_attention_plan alone: one head
    short = Handles(pkg, _short_pattern(), gpu)             # no long row on either side
    d2 = {n: t[:2] for n, t in shared.data(k, kv, seed=501).items()}
    for h in (long, short):
        n_q, n_k = h.A.rows, h.A.cols
        gen = torch.Generator(device=gpu).manual_seed(503)
        Q, K, V, dO = (torch.randn((2, n, w), generator=gen, device=gpu) for n, w in ((n_q, k), (n_k, k), (n_k, kv), (n_q, kv)))
        nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)      # noqa: E731
        O, stats, delta, dQ, dK, dV = nan(2, n_q, kv), nan(2, n_q, 2), nan(2, n_q), nan(2, n_q, k), nan(2, n_k, k), nan(2, n_k, kv)
        for call in (lambda: h.A.attention_forward_heads(Q, K, V, O, stats, SCALE),
                     lambda: h.A.attention_backward_q_heads(Q, K, V, O, dO, stats, delta, dQ, SCALE),
                     lambda: h.T.attention_backward_kv_heads(Q, K, V, dO, stats, delta, dK, dV, SCALE)):
            with pytest.raises(capi.SpmvError) as e:
                call()
            assert e.value.status == capi.ERR_NOT_PLANNED and "_heads" in str(e.value)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (O, stats, delta, dQ, dK, dV)), "a refused call wrote to an output"
    d = shared.data(k, kv, seed=501)
    before = single_head(long, *(d[n][0] for n in ("Q", "K", "V", "dO")))
    for m, pieces in ((long.A, shared.pieces_A), (long.T, shared.pieces_T)):
        assert pieces >= 2
        b1 = m.attention_plan_bytes()
        m.attention_plan_heads(3)
        b3 = m.attention_plan_bytes()
        assert b3 - b1 == 2 * pieces * 132 * 4
        m.attention_plan_heads(2)                            # covered already: nothing changes
        assert m.attention_plan_bytes() == b3
    for m in (short.A, short.T):                             # nothing more for a handle without a long row
        b1 = m.attention_plan_bytes()
        m.attention_plan_heads(3)
        assert m.attention_plan_bytes() == b1
    assert shared.pieces_A == 3
    after = single_head(long, *(d[n][0] for n in ("Q", "K", "V", "dO")))
    for name in before:
        assert torch.equal(_raw(before[name]), _raw(after[name])), f"{name} of the single-head call changed when the plan grew"
    got = heads_run(long, d2, "stacked")                     # and two heads now run, on both handles
    want = [single_head(long, *(d[n][y] for n in ("Q", "K", "V", "dO"))) for y in range(2)]
    assert_heads_equal(got, want, "after the plan grew")
    heads_run(short, {n: t for n, t in zip(("Q", "K", "V", "dO"), (Q, K, V, dO))}, "stacked")
    long.close()
    short.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_heads_refusals_launch_nothing(shared, pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h, k, kv, ld = shared.h, 8, 8, 8
    ones = lambda n: torch.ones((2, n, ld), dtype=torch.float32, device=gpu)       # noqa: E731
    Q, K, V, dO, O_in = ones(ROWS), ones(COLS), ones(COLS), ones(ROWS), ones(ROWS)
    stats_in, delta_in = torch.zeros((2, ROWS, 2), device=gpu), torch.zeros((2, ROWS), device=gpu)
    outs = {n: torch.full((2, r, w), float("nan"), dtype=torch.float32, device=gpu) for n, r, w in
            (("O", ROWS, ld), ("dQ", ROWS, ld), ("dK", COLS, ld), ("dV", COLS, ld), ("stats", ROWS, 2), ("delta", ROWS, 1))}
    st = capi._stream_handle()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    good = dict(heads=2, q=ROWS * ld, k=COLS * ld, v=COLS * ld, o=ROWS * ld, d_o=ROWS * ld, stats=2 * ROWS, delta=ROWS,
                dq=ROWS * ld, dk=COLS * ld, dv=COLS * ld)

    def call(which, **change):
        hs = capi.AttnHeads(**dict(good, **change))
        if which == "forward":
            return lib.spmv_csr_attention_forward_heads(h.A._h, C.byref(hs), SCALE, k, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                        p(outs["O"]), ld, p(outs["stats"]), st)
        if which == "backward_q":
            return lib.spmv_csr_attention_backward_q_heads(h.A._h, C.byref(hs), SCALE, k, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                           p(O_in), ld, p(dO), ld, p(stats_in), p(outs["delta"]), p(outs["dQ"]),
                                                           ld, st)
        return lib.spmv_csr_attention_backward_kv_heads(h.T._h, C.byref(hs), SCALE, k, p(Q), ld, p(K), ld, kv, p(V), ld, p(dO),
                                                        ld, p(stats_in), p(delta_in), p(outs["dK"]), ld, p(outs["dV"]), ld, st)

    narrow = {"forward": "o", "backward_q": "dq", "backward_kv": "dv"}      # an output of width 8 at a head stride of 4
    for which in ("forward", "backward_q", "backward_kv"):
        name = f"spmv_csr_attention_{which}_heads"
        cases = [dict(heads=0), dict(reserved=1), dict(q=6), dict(v=ROWS * ld + 6), dict(k=-4), dict(stats=-2),
                 {narrow[which]: 4}, dict(heads=65536), dict(stats=2 * ROWS + 1)]
        if which != "backward_kv":
            cases.append(dict(stats=0) if which == "forward" else dict(delta=0))       # (outputs of width 2 and 1)
        for change in cases:
            assert call(which, **change) == capi.ERR_INVALID, f"{which} {change}"
            assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error()
        assert call(which, heads=HEADS + 1) == capi.ERR_NOT_PLANNED       # (more than the fixture planned)
        assert name in lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs.values()), "a refused call wrote to an output"
    for which in ("forward", "backward_q", "backward_kv"):                 # and the same calls, unchanged, are accepted
        assert call(which) == capi.OK, lib.spmv_last_error()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in outs.values())


# ---- graph capture -----------------------------------------------------------------------------------------------------
def test_heads_calls_are_graph_capturable(shared, gpu):
    import torch
    h, k, kv = shared.h, 12, 16
    data = [shared.data(k, kv, seed=601 + i) for i in range(3)]
    eager = [heads_run(h, d, "stacked") for d in data]                      # (also the warm run of every kernel)
    Q, K, V, dO = (data[0][n].clone() for n in ("Q", "K", "V", "dO"))
    nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)      # noqa: E731
    outs = dict(O=nan(HEADS, ROWS, kv), stats=nan(HEADS, ROWS, 2), delta=nan(HEADS, ROWS), dQ=nan(HEADS, ROWS, k),
                dK=nan(HEADS, COLS, k), dV=nan(HEADS, COLS, kv))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream; the calls take the current stream)
        h.A.attention_forward_heads(Q, K, V, outs["O"], outs["stats"], SCALE)
        h.A.attention_backward_q_heads(Q, K, V, outs["O"], dO, outs["stats"], outs["delta"], outs["dQ"], SCALE)
        h.T.attention_backward_kv_heads(Q, K, V, dO, outs["stats"], outs["delta"], outs["dK"], outs["dV"], SCALE)
    for i in (1, 2):
        for dst, n in ((Q, "Q"), (K, "K"), (V, "V"), (dO, "dO")):
            dst.copy_(data[i][n])
        for o in outs.values():
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for name, t in outs.items():
            assert torch.equal(_raw(t), _raw(eager[i][name])), f"replay {i}: {name} differs from the eager run"


# ---- the holder --------------------------------------------------------------------------------------------------------
def _holders(shared):
    import torch
    s, gpu = shared.s, shared.gpu
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    SA = shared.pkg.sparse_attention
    return (SA.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE, heads="loop"),
            SA.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE, heads="batched"))


def _step(att, Q, K, V, dO):
    import torch
    q, k, v = (t.detach().requires_grad_(True) for t in (Q, K, V))
    O = att(q, k, v)
    O.backward(dO)
    torch.cuda.synchronize()
    return O.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("blocks", [False, True], ids=["stacked", "column-blocks"])
def test_batched_holder_equals_the_loop_through_autograd(shared, monkeypatch, blocks):
    import torch
    loop, batched = _holders(shared)
    k = 8
    gen = torch.Generator(device=shared.gpu).manual_seed(701)
    flat = [torch.randn((n, HEADS * k), generator=gen, device=shared.gpu) for n in (ROWS, COLS, COLS, ROWS)]
    split = lambda t: t.view(t.shape[0], HEADS, k).transpose(0, 1)       # noqa: E731  strides (k, heads k, 1)
    ops = [split(t) if blocks else split(t).contiguous() for t in flat]
    want = _step(loop, *ops)
    capi = shared.pkg.capi
    seen = []
    real = capi.CsrMatrix.attention_forward_heads
    monkeypatch.setattr(capi.CsrMatrix, "attention_forward_heads",
                        lambda self, Q, K, V, *a, **kw: (seen.append((Q.data_ptr(), K.data_ptr(), V.data_ptr(), tuple(Q.stride()))),
                                                         real(self, Q, K, V, *a, **kw))[1])

    def never(*a, **kw):
        raise AssertionError("the batched holder called attention_forward")

    monkeypatch.setattr(capi.CsrMatrix, "attention_forward", never)
    got = _step(batched, *ops)
    for name, g, w in zip(("O", "dQ", "dK", "dV"), got, want):
        assert g.shape == w.shape and torch.equal(_raw(g), _raw(w)), f"{name}: batched differs from the loop"
    base = flat if blocks else ops
    strides = (k, HEADS * k, 1) if blocks else (ROWS * k, k, 1)
    assert seen == [(base[0].data_ptr(), base[1].data_ptr(), base[2].data_ptr(), strides)], "one call, on the caller's memory"
    loop.close()
    batched.close()


def test_batched_holder_copies_what_it_must_and_takes_2d_operands(shared):
    import torch
    loop, batched = _holders(shared)
    gen = torch.Generator(device=shared.gpu).manual_seed(703)
    # heads of 6 columns in column blocks: a head stride of 6 floats is no multiple of 4, so the holder copies once
    k = 6
    flat = [torch.randn((n, HEADS * k), generator=gen, device=shared.gpu) for n in (ROWS, COLS, COLS, ROWS)]
    ops = [t.view(t.shape[0], HEADS, k).transpose(0, 1) for t in flat]
    for name, g, w in zip(("O", "dQ", "dK", "dV"), _step(batched, *ops), _step(loop, *ops)):
        assert torch.equal(_raw(g), _raw(w)), f"{name}: batched differs from the loop (copied operands)"
    # 2-D operands: as before in both modes
    two = [torch.randn((n, 12), generator=gen, device=shared.gpu) for n in (ROWS, COLS, COLS, ROWS)]
    for name, g, w in zip(("O", "dQ", "dK", "dV"), _step(batched, *two), _step(loop, *two)):
        assert g.dim() == 2 and torch.equal(_raw(g), _raw(w)), f"{name}: 2-D operands differ between the modes"
    # a head count beyond what one launch takes is split into the fewest chunks (here the limit is lowered, not the size raised)
    batched.max_heads = 2
    ops = [t.contiguous() for t in ops]
    want = _step(loop, *ops)
    assert batched.head_chunks(HEADS, k, k) == [(0, 2), (2, 3)]
    for name, g, w in zip(("O", "dQ", "dK", "dV"), _step(batched, *ops), want):
        assert torch.equal(_raw(g), _raw(w)), f"{name}: batched in two chunks differs from the loop"
    loop.close()
    batched.close()


def test_batched_holder_takes_one_3d_head_whose_size_is_no_multiple_of_four(pkg, gpu):
    """A contiguous (1, rows, k) tensor has stride(0) = rows k, here 270 and 210: no multiple of 4, and no stride of anything.
    With one head the binding passes stride 0, so the call goes through as it does in the loop."""
    import torch
    s = _short_pattern()
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    SA = pkg.sparse_attention
    loop = SA.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE, heads="loop")
    batched = SA.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE, heads="batched")
    gen = torch.Generator(device=gpu).manual_seed(705)
    k = 3
    assert (s.rows * k) % 4 != 0 and (s.cols * k) % 4 != 0
    ops = [torch.randn((1, n, k), generator=gen, device=gpu) for n in (s.rows, s.cols, s.cols, s.rows)]
    for name, g, w in zip(("O", "dQ", "dK", "dV"), _step(batched, *ops), _step(loop, *ops)):
        assert torch.equal(_raw(g), _raw(w)), f"{name}: one 3-D head differs between the modes"
    loop.close()
    batched.close()


# ---- the launch limits -------------------------------------------------------------------------------------------------
def test_heads_launch_limit_on_either_side(pkg, gpu):
    """rows x lanes per row x heads < 2^32 at k = kv = 64 (16 lanes per row, 16 rows per block of 256): 4096 rows are 256
    blocks, and 256 x 65535 x 256 = 2^32 - 65536 fits; 4097 rows are 257 blocks, which take 65280 heads and no more.  A
    launch at the limit would write 64 GiB of O, so the accepting side is the library's own answer
    (spmv_csr_attention_max_heads, which the holder splits by) and the refusing side is a call that must launch nothing."""
    import torch
    capi = pkg.capi
    lib = capi.lib()
    k = kv = 64
    want = {4096: 65535, 4097: (2 ** 32 - 1) // (257 * 256)}
    assert want[4097] == 65280
    for rows, fit in want.items():
        rp = np.arange(rows + 1, dtype=np.int32)
        h = Handles(pkg, E.Structure(rows, 8, rp, (np.arange(rows) % 8).astype(np.int32)), gpu)
        assert h.A.attention_max_heads(k, kv) == fit
        assert h.A.attention_max_heads(4, 4) == 65535                  # one lane per row: 17 blocks
        h.A.attention_plan_heads(65535)                                # (no long row: nothing is allocated)
        Q, O = torch.ones((rows, k), device=gpu), torch.full((rows, kv), float("nan"), device=gpu)
        K = V = torch.ones((8, k), device=gpu)
        stats = torch.full((rows, 2), float("nan"), device=gpu)
        p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
        for heads in (fit, fit + 1):
            if heads > 65535:
                continue
            hs = capi.AttnHeads(heads=heads, o=rows * kv, stats=2 * rows)      # (inputs shared at stride 0)
            if heads > fit:
                rc = lib.spmv_csr_attention_forward_heads(h.A._h, C.byref(hs), SCALE, k, p(Q), k, p(K), k, kv, p(V), kv, p(O), kv,
                                                          p(stats), capi._stream_handle())
                assert rc == capi.ERR_INVALID
                msg = lib.spmv_last_error().decode()
                assert msg.startswith("spmv_csr_attention_forward_heads:") and "2^32" in msg, msg
        torch.cuda.synchronize()
        assert bool(torch.isnan(O).all()) and bool(torch.isnan(stats).all()), "a refused call wrote to an output"
        h.close()
    # the holder splits by the same answer: 65536 heads would be two launches of 32768 on the small pattern
    s = _short_pattern()
    att = pkg.sparse_attention.FusedSparseAttention(s.rows, s.cols, torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu),
                                                    heads="batched")
    assert att.head_chunks(65536, 8, 8) == [(0, 32768), (32768, 65536)]
    assert att.head_chunks(65535, 8, 8) == [(0, 65535)]
    att.close()
