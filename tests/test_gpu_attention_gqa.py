"""Grouped-query heads on the device (spmv_csr_attention_forward_gqa, _backward_q_gqa, _backward_kv_gqa and the holder's
3-D calls whose K and V carry H_kv heads).  The claim is bit identity with the single-head calls: head y of a _gqa call is
the single-head call on K[y // g], V[y // g], and dK, dV of K/V head c are the single-head results of heads c g .. c g + g - 1
added in fp32 in head order, starting from the first head's value.  So nothing but the holder's accuracy test has a tolerance;
every other comparison is of raw bits.

One pattern serves most tests: 700 queries x 1200 keys with empty rows, rows of 1 .. 7 entries (inside one step), rows of
9 .. 200 entries, one row of 1100 entries (three pieces), one key that more than 512 queries list, so that the transposed
pattern has a row in pieces too (k_attn_add_pieces_gqa: a kernel that summed the heads inside a piece, or in another head
order, would give other bits there), and keys nobody lists.  H = 6 query heads with different data in every head run at
g = 1, 2, 3 and 6 on the first 6 / g heads of K and V.

Every operand of a _gqa call lives in a buffer of its own between guard bands: outputs start as NaN, the gaps between rows
and between heads hold a guard value that must be intact afterwards, and the gaps of an input hold NaN.
"""
import ctypes as C

import numpy as np
import pytest

import _exact as E
from _util import RTOL

pytestmark = pytest.mark.gpu

GUARD, GUARD_N = 3.0e35, 1024
SCALE = 2.0 ** -2
ROWS, COLS, HOT = 700, 1200, 7
H = 6
GROUPS = (1, 2, 3, 6)
PIECE = 512
NAMES = ("O", "stats", "delta", "dQ", "dK", "dV")


def _pattern():
    rng = np.random.Generator(np.random.PCG64(211))
    lengths = np.concatenate([np.zeros(20, np.int64), rng.integers(1, 8, size=520), rng.integers(9, 201, size=159), [1100]])
    lengths = lengths[rng.permutation(len(lengths))]
    assert len(lengths) == ROWS
    rows = []
    for n in lengths:
        c = np.sort(rng.choice(COLS - 20, size=int(n), replace=False))         # the last 20 keys: nobody lists them
        if 1 <= n <= 7 and HOT not in c:           # the hot key: in every short row
            c[0] = HOT
            c = np.sort(c)
        rows.append(c)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    s = E.Structure(ROWS, COLS, rp, np.concatenate(rows).astype(np.int32))
    per_key = np.bincount(s.ci, minlength=COLS)
    assert per_key[HOT] > PIECE and (lengths == 0).sum() == 20 and lengths.max() == 1100 and (per_key == 0).sum() >= 20
    return s


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
    return out


class Shared:
    """The pattern, its handles planned for H heads, and the expectation by (k, kv, seed, g): computed once."""

    def __init__(self, pkg, gpu):
        self.pkg, self.gpu = pkg, gpu
        self.s = _pattern()
        self.h = Handles(pkg, self.s, gpu, heads=H)
        self._single, self._want = {}, {}

    def data(self, k, kv, seed):
        """Q, dO of H heads and K, V of H heads (a run at group g reads the first H / g), different numbers in every head."""
        import torch
        gen = torch.Generator(device=self.gpu).manual_seed(seed)
        mk = lambda n, w: torch.randn((H, n, w), generator=gen, device=self.gpu, dtype=torch.float32)      # noqa: E731
        return dict(Q=mk(ROWS, k), K=mk(COLS, k), V=mk(COLS, kv), dO=mk(ROWS, kv))

    def want(self, k, kv, seed, g):
        """Per query head O, stats, delta, dQ of the single-head call on K[y // g], V[y // g]; per K/V head dK, dV folded in
        torch in head order from the first head's value."""
        import torch
        key = (k, kv, seed, g)
        if key not in self._want:
            d = self.data(k, kv, seed)
            per = []
            for y in range(H):
                c = y // g
                if (k, kv, seed, y, c) not in self._single:
                    self._single[(k, kv, seed, y, c)] = single_head(self.h, d["Q"][y], d["K"][c], d["V"][c], d["dO"][y])
                per.append(self._single[(k, kv, seed, y, c)])
            w = {n: torch.stack([p[n] for p in per]) for n in ("O", "stats", "delta", "dQ")}
            for n in ("dK", "dV"):
                folded = []
                for c in range(H // g):
                    acc = per[c * g][n].clone()
                    for i in range(1, g):
                        acc = acc + per[c * g + i][n]
                    folded.append(acc)
                w[n] = torch.stack(folded)
            torch.cuda.synchronize()
            self._want[key] = w
        return self._want[key]


@pytest.fixture(scope="module")
def shared(pkg, gpu):
    sh = Shared(pkg, gpu)
    yield sh
    sh.h.close()


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
        self.view = torch.as_strided(self.buf, (heads, rows, w), (stride, ld, 1), GUARD_N)
        self.view.copy_(fill if fill is not None else torch.full((heads, rows, w), float("nan"), device=gpu))
        own = torch.zeros_like(self.buf, dtype=torch.bool)
        torch.as_strided(own, (heads, rows, w), (stride, ld, 1), GUARD_N).fill_(True)
        self.gaps = ~own
        self.is_output = fill is None

    def intact(self):
        n = GUARD_N
        bands = bool((self.buf[:n] == GUARD).all()) and bool((self.buf[-n:] == GUARD).all())
        return bands and (bool((self.buf[self.gaps] == GUARD).all()) if self.is_output else True)


def gqa_run(h, d, g, layout, scale=SCALE, heads_call=False):
    """The three _gqa calls at group g on the operands d laid out by `layout` (Q, dO and the query-side outputs with H
    heads, K, V, dK, dV with H / g); returns the outputs and asserts that nothing but their own elements was written.
    heads_call: the _heads calls instead (g = 1 only)."""
    import torch
    A, T = h.A, h.T
    gpu = d["Q"].device
    heads, k, kv = d["Q"].shape[0], d["Q"].shape[2], d["V"].shape[2]
    kvh = heads // g
    lay = LAYOUTS[layout]
    made = []

    def mat(n_heads, rows, w, fill=None):
        ld, stride = lay(n_heads, rows, w)
        made.append(Guarded(gpu, n_heads, rows, w, ld, stride, fill))
        return made[-1].view

    def vec(rows, inner, pad):
        made.append(Guarded(gpu, heads, rows, inner, inner, rows * inner + pad))
        return made[-1].view if inner > 1 else made[-1].view[:, :, 0]

    Q, dO = mat(heads, A.rows, k, d["Q"]), mat(heads, A.rows, kv, d["dO"])
    K, V = mat(kvh, A.cols, k, d["K"][:kvh]), mat(kvh, A.cols, kv, d["V"][:kvh])
    pad = 0 if layout == "stacked" else 6
    out = dict(O=mat(heads, A.rows, kv), stats=vec(A.rows, 2, pad), delta=vec(A.rows, 1, pad + 1 if pad else 0),
               dQ=mat(heads, A.rows, k), dK=mat(kvh, A.cols, k), dV=mat(kvh, A.cols, kv))
    if heads_call:
        assert g == 1
        A.attention_forward_heads(Q, K, V, out["O"], out["stats"], scale)
        A.attention_backward_q_heads(Q, K, V, out["O"], dO, out["stats"], out["delta"], out["dQ"], scale)
        T.attention_backward_kv_heads(Q, K, V, dO, out["stats"], out["delta"], out["dK"], out["dV"], scale)
    else:
        A.attention_forward_gqa(Q, K, V, out["O"], out["stats"], scale)
        A.attention_backward_q_gqa(Q, K, V, out["O"], dO, out["stats"], out["delta"], out["dQ"], scale)
        T.attention_backward_kv_gqa(Q, K, V, dO, out["stats"], out["delta"], out["dK"], out["dV"], scale)
    torch.cuda.synchronize()
    assert all(m.intact() for m in made), f"{layout} g={g}: a pass wrote outside its outputs' own elements"
    return out


def assert_bits(got, want, tag):
    import torch
    for name in NAMES:
        assert got[name].shape == want[name].shape, f"{tag}: {name} is {tuple(got[name].shape)}"
        for y in range(want[name].shape[0]):
            assert torch.equal(_raw(got[name][y]), _raw(want[name][y])), f"{tag}: {name} of head {y} differs in a bit"


# ---- bit identity ------------------------------------------------------------------------------------------------------
SHAPES = [(3, 2), (8, 6), (12, 16), (24, 32), (40, 64)]         # V = 1, 2, 4, 8, 16


@pytest.mark.parametrize("layout", ["stacked", "odd_ld"])
@pytest.mark.parametrize("k,kv", SHAPES, ids=[f"k{k}-kv{kv}" for k, kv in SHAPES])
def test_gqa_equals_the_single_head_calls_folded_in_head_order(shared, k, kv, layout):
    import torch
    seed = 900 + k
    d = shared.data(k, kv, seed)
    for g in GROUPS:
        got = gqa_run(shared.h, d, g, layout)
        assert_bits(got, shared.want(k, kv, seed, g), f"k={k} kv={kv} {layout} g={g}")
    # g = 1 is the _heads call
    one, heads = gqa_run(shared.h, d, 1, layout), gqa_run(shared.h, d, 1, layout, heads_call=True)
    for name in NAMES:
        assert torch.equal(_raw(one[name]), _raw(heads[name])), f"k={k} kv={kv} {layout}: {name} at g = 1 differs from the _heads call"
    # the fold is a sum: dK of a group is no single head's dK, and keys nobody lists get +0
    w2, w1 = shared.want(k, kv, seed, 2), shared.want(k, kv, seed, 1)
    assert not torch.equal(w2["dK"][0], w1["dK"][0])
    per_key = np.bincount(shared.s.ci, minlength=COLS)
    unlisted = torch.from_numpy(per_key == 0).to(shared.gpu)
    got = gqa_run(shared.h, d, 3, layout)
    assert bool((_raw(got["dK"][:, unlisted]) == 0).all()) and bool((_raw(got["dV"][:, unlisted]) == 0).all())


def test_the_expectation_tells_wrong_orders_apart(shared):
    """The pattern and data must make the order visible: folding the heads in reverse order, or summing the heads inside each
    piece of the hot key's row before adding the pieces, gives other bits than the contract somewhere."""
    import torch
    k, kv, seed, g = 12, 16, 912, 3
    d, w = shared.data(k, kv, seed), shared.want(k, kv, seed, g)
    per = [shared._single[(k, kv, seed, y, y // g)]["dK"] for y in range(H)]
    rev = (per[2] + per[1]) + per[0]
    assert not torch.equal(_raw(rev), _raw(w["dK"][0])), "the data do not tell the head order"
    # the hot key's row of T in pieces, per head, by the single-head call on a pattern that is one piece of that row
    s = shared.s
    queries = np.sort(s.row_of[s.ci == HOT])
    assert len(queries) > PIECE
    parts = []
    for lo in range(0, len(queries), PIECE):
        q = queries[lo:lo + PIECE]
        rp = np.zeros(ROWS + 1, np.int32)
        rp[q + 1] = 1
        sub = Handles(shared.pkg, E.Structure(ROWS, COLS, np.cumsum(rp).astype(np.int32), np.full(len(q), HOT, np.int32)), shared.gpu)
        heads = []
        for y in range(g):
            # stats and delta of the whole pattern: the piece's dK, dV are sums over its queries of terms that only need those
            full = shared._single[(k, kv, seed, y, 0)]
            dK, dV = torch.zeros((COLS, k), device=shared.gpu), torch.zeros((COLS, kv), device=shared.gpu)
            sub.T.attention_backward_kv(d["Q"][y], d["K"][0], d["V"][0], d["dO"][y], full["stats"], full["delta"], dK, dV, SCALE)
            heads.append(dK[HOT].clone())
        torch.cuda.synchronize()
        sub.close()
        parts.append(heads)
    # the contract: per head the pieces from +0 in piece order, then the heads in head order
    by_head = []
    for y in range(g):
        acc = torch.zeros(k, device=shared.gpu)
        for p in parts:
            acc = acc + p[y]
        by_head.append(acc)
    contract = (by_head[0] + by_head[1]) + by_head[2]
    assert torch.equal(_raw(contract), _raw(w["dK"][0][HOT])), "the pieces of the hot key do not rebuild the single-head result"
    inside = torch.zeros(k, device=shared.gpu)
    for p in parts:
        inside = inside + ((p[0] + p[1]) + p[2])
    assert not torch.equal(_raw(inside), _raw(contract)), "the data do not tell a sum over the heads inside a piece apart"


# ---- layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["blocks", "padded"])
@pytest.mark.parametrize("k,kv", [(12, 16), (6, 40)], ids=["k12-kv16", "k6-kv40"])
def test_gqa_layouts_column_blocks_and_padded_strides(shared, k, kv, layout):
    """(stacked operands and an odd ld run in the test above, between the same guard bands.)  Column blocks: Q is a block of
    an (n, H k) tensor and K one of an (n, H_kv k) tensor, so the two sides differ in ld as well as in their head count."""
    seed = 950 + k
    d = shared.data(k, kv, seed)
    for g in (2, 3):
        got = gqa_run(shared.h, d, g, layout)
        assert_bits(got, shared.want(k, kv, seed, g), f"k={k} kv={kv} {layout} g={g}")
        if layout == "blocks" and k % 4 == 0:
            assert got["dQ"].stride() == (k, H * k, 1) and got["dK"].stride() == (k, H // g * k, 1)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_gqa_refusals_launch_nothing(shared, pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h, k, kv, ld = shared.h, 8, 8, 8
    ones = lambda heads, n: torch.ones((heads, n, ld), dtype=torch.float32, device=gpu)       # noqa: E731
    Q, K, V, dO, O_in = ones(H, ROWS), ones(H, COLS), ones(H, COLS), ones(H, ROWS), ones(H, ROWS)
    stats_in, delta_in = torch.zeros((H, ROWS, 2), device=gpu), torch.zeros((H, ROWS), device=gpu)
    outs = {n: torch.full((H, r, w), float("nan"), dtype=torch.float32, device=gpu) for n, r, w in
            (("O", ROWS, ld), ("dQ", ROWS, ld), ("dK", COLS, ld), ("dV", COLS, ld), ("stats", ROWS, 2), ("delta", ROWS, 1))}
    st = capi._stream_handle()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    good = dict(heads=4, q=ROWS * ld, k=COLS * ld, v=COLS * ld, o=ROWS * ld, d_o=ROWS * ld, stats=2 * ROWS, delta=ROWS,
                dq=ROWS * ld, dk=COLS * ld, dv=COLS * ld)

    def call(which, group=2, **change):
        hs = capi.AttnHeads(**dict(good, **change))
        if which == "forward":
            return lib.spmv_csr_attention_forward_gqa(h.A._h, C.byref(hs), group, SCALE, k, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                      p(outs["O"]), ld, p(outs["stats"]), st)
        if which == "backward_q":
            return lib.spmv_csr_attention_backward_q_gqa(h.A._h, C.byref(hs), group, SCALE, k, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                         p(O_in), ld, p(dO), ld, p(stats_in), p(outs["delta"]), p(outs["dQ"]),
                                                         ld, st)
        return lib.spmv_csr_attention_backward_kv_gqa(h.T._h, C.byref(hs), group, SCALE, k, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                      p(dO), ld, p(stats_in), p(delta_in), p(outs["dK"]), ld, p(outs["dV"]), ld, st)

    for which in ("forward", "backward_q", "backward_kv"):
        name = f"spmv_csr_attention_{which}_gqa"
        cases = [dict(group=0), dict(group=-1), dict(group=3), dict(reserved=1), dict(heads=0), dict(q=6), dict(k=-4)]
        if which == "backward_kv":
            cases.append(dict(dk=4))                     # a dk stride below k = 8 with two K/V heads
            cases.append(dict(dv=4))
        for change in cases:
            assert call(which, **change) == capi.ERR_INVALID, f"{which} {change}"
            assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error()
        assert call(which, heads=H + 2) == capi.ERR_NOT_PLANNED       # (more than the fixture planned; 8 % 2 == 0)
        assert name in lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs.values()), "a refused call wrote to an output"
    # one K/V head: the dk / dv stride says nothing and may be anything, as an output stride of a one-head _heads call may
    assert call("backward_kv", group=4, dk=0, dv=0) == capi.OK, lib.spmv_last_error()
    for which in ("forward", "backward_q", "backward_kv"):                 # and the same calls, unchanged, are accepted
        assert call(which) == capi.OK, lib.spmv_last_error()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t[:4 if n in ("O", "dQ", "stats", "delta") else 2]).any()) for n, t in outs.items())
    assert all(bool(torch.isnan(t[4 if n in ("O", "dQ", "stats", "delta") else 2:]).all()) for n, t in outs.items())


# ---- graph capture -----------------------------------------------------------------------------------------------------
def test_gqa_calls_are_graph_capturable(shared, gpu):
    import torch
    h, k, kv, g = shared.h, 12, 16, 2
    seeds = (961, 962, 963)
    for seed in seeds:
        shared.want(k, kv, seed, g)                                         # (also the warm run of the single-head kernels)
    gqa_run(h, shared.data(k, kv, seeds[0]), g, "stacked")                  # (and of the _gqa ones)
    d0 = shared.data(k, kv, seeds[0])
    Q, dO = d0["Q"].clone(), d0["dO"].clone()
    K, V = d0["K"][:H // g].clone(), d0["V"][:H // g].clone()
    nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)      # noqa: E731
    outs = dict(O=nan(H, ROWS, kv), stats=nan(H, ROWS, 2), delta=nan(H, ROWS), dQ=nan(H, ROWS, k),
                dK=nan(H // g, COLS, k), dV=nan(H // g, COLS, kv))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream; the calls take the current stream)
        h.A.attention_forward_gqa(Q, K, V, outs["O"], outs["stats"], SCALE)
        h.A.attention_backward_q_gqa(Q, K, V, outs["O"], dO, outs["stats"], outs["delta"], outs["dQ"], SCALE)
        h.T.attention_backward_kv_gqa(Q, K, V, dO, outs["stats"], outs["delta"], outs["dK"], outs["dV"], SCALE)
    for seed in seeds[1:]:
        d = shared.data(k, kv, seed)
        Q.copy_(d["Q"]), dO.copy_(d["dO"]), K.copy_(d["K"][:H // g]), V.copy_(d["V"][:H // g])
        for o in outs.values():
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(outs, shared.want(k, kv, seed, g), f"replay with seed {seed}")


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
    return dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


def _dense_gqa(mask, scale, Q, K, V, dO, dtype, g):
    """(O, dQ, dK, dV, P) of the masked softmax attention with K and V expanded by repeat_interleave, by torch's dense autograd
    in `dtype` (test_gpu_fused_attention's reference with a head dimension); a row without a key gives a zero row of O."""
    import torch
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (Q, K, V))
    ke, ve = k.repeat_interleave(g, dim=0), v.repeat_interleave(g, dim=0)
    full = mask.any(1)
    scores = torch.where(mask, (q @ ke.transpose(1, 2)) * scale, torch.tensor(float("-inf"), dtype=dtype, device=mask.device))
    P = torch.zeros_like(scores)
    P[:, full] = torch.softmax(scores[:, full], dim=2)
    O = P @ ve
    O.backward(dO.to(dtype))
    return dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad), P.detach()


def _magnitudes(mask, scale, Q, K, V, dO, P, g):
    """test_gpu_fused_attention's magnitudes per head; those of dK and dV added over the heads of a group."""
    import torch
    aQ, aK, aV, adO = (x.detach().double().abs() for x in (Q, K.repeat_interleave(g, dim=0), V.repeat_interleave(g, dim=0), dO))
    dP_abs = torch.where(mask, adO @ aV.transpose(1, 2), torch.zeros((), dtype=torch.float64, device=Q.device))
    dS_abs = abs(scale) * P * (dP_abs + (P * dP_abs).sum(2, keepdim=True))
    fold = lambda t: t.view(t.shape[0] // g, g, *t.shape[1:]).sum(1)       # noqa: E731
    return {"O": P @ aV, "dQ": dS_abs @ aK, "dK": fold(dS_abs.transpose(1, 2) @ aQ), "dV": fold(P.transpose(1, 2) @ adO)}


def test_gqa_holder_modes_agree_and_match_dense_autograd(shared):
    """H = 6 on H_kv = 2: "batched" (one _gqa call per pass) and "loop" (per-head calls, dK and dV folded in torch) give the
    same bits through autograd, and both lie within test_gpu_fused_attention's rule of torch's fp64 dense GQA autograd: the
    normalised error is at most max(4 x that of torch's fp32 dense autograd, RTOL)."""
    import torch
    loop, batched = _holders(shared)
    k, kv, hkv = 24, 32, 2
    g = H // hkv
    gen = torch.Generator(device=shared.gpu).manual_seed(971)
    Q, K, V, dO = (torch.randn((n_heads, n, w), generator=gen, device=shared.gpu) for n_heads, n, w in
                   ((H, ROWS, k), (hkv, COLS, k), (hkv, COLS, kv), (H, ROWS, kv)))
    got_l, got_b = _step(loop, Q, K, V, dO), _step(batched, Q, K, V, dO)
    for name in ("O", "dQ", "dK", "dV"):
        assert got_b[name].shape == got_l[name].shape and torch.equal(_raw(got_b[name]), _raw(got_l[name])), f"{name}: batched differs from the loop"
    assert got_b["dK"].shape == (hkv, COLS, k) and got_b["dV"].shape == (hkv, COLS, kv)
    s = shared.s
    mask = torch.zeros((ROWS, COLS), dtype=torch.bool, device=shared.gpu)
    mask[torch.from_numpy(s.row_of).to(shared.gpu), torch.from_numpy(s.ci.astype(np.int64)).to(shared.gpu)] = True
    r64, P = _dense_gqa(mask, SCALE, Q, K, V, dO, torch.float64, g)
    r32, _ = _dense_gqa(mask, SCALE, Q, K, V, dO, torch.float32, g)
    mags = _magnitudes(mask, SCALE, Q, K, V, dO, P, g)
    for what in ("O", "dQ", "dK", "dV"):
        gg, g64, g32, mag = got_b[what], r64[what], r32[what], mags[what]
        live = mag > 0
        assert bool(live.any()) and bool((gg[~live] == 0).all()), f"{what}: a value where nothing contributes"
        ours = float(((gg.double() - g64).abs()[live] / mag[live]).max())
        yard = float(((g32.double() - g64).abs()[live] / mag[live]).max())
        print(f"gqa holder {what}: normalised error fused {ours:.3g}, torch fp32 dense GQA autograd {yard:.3g}")
        assert ours <= max(4.0 * yard, RTOL), f"{what}: {ours:.3g} against {yard:.3g} of torch's fp32 dense autograd"
    loop.close()
    batched.close()


def test_gqa_holder_refuses_other_head_mismatches(shared):
    import torch
    loop, batched = _holders(shared)
    k = 8
    mk = lambda heads, n: torch.randn((heads, n, k), device=shared.gpu)      # noqa: E731
    for att in (loop, batched):
        with pytest.raises(ValueError, match="heads"):
            att(mk(H, ROWS), mk(4, COLS), mk(4, COLS))                      # 6 % 4 != 0
        with pytest.raises(ValueError, match="heads"):
            att(mk(H, ROWS), mk(2, COLS), mk(3, COLS))                      # K and V disagree
        with pytest.raises(ValueError, match="heads"):
            att(mk(2, ROWS), mk(H, COLS), mk(H, COLS))                      # more K/V heads than query heads
    loop.close()
    batched.close()


def test_gqa_holder_chunks_are_whole_groups_and_the_loop_is_the_way_out(shared, monkeypatch):
    import torch
    loop, batched = _holders(shared)
    capi = shared.pkg.capi
    k = kv = 8
    gen = torch.Generator(device=shared.gpu).manual_seed(981)
    calls = []
    real_gqa, real_one = capi.CsrMatrix.attention_backward_kv_gqa, capi.CsrMatrix.attention_backward_kv
    monkeypatch.setattr(capi.CsrMatrix, "attention_backward_kv_gqa",
                        lambda self, Q, *a, **kw: (calls.append(("gqa", Q.shape[0])), real_gqa(self, Q, *a, **kw))[1])
    monkeypatch.setattr(capi.CsrMatrix, "attention_backward_kv",
                        lambda self, Q, *a, **kw: (calls.append(("one", 1)), real_one(self, Q, *a, **kw))[1])
    for hkv, cap, chunks in ((3, 2, [(0, 2), (2, 4), (4, 6)]), (3, 3, [(0, 2), (2, 4), (4, 6)]), (3, 5, [(0, 4), (4, 6)]),
                             (2, 3, [(0, 3), (3, 6)]), (2, 2, None), (3, 1, None)):
        g = H // hkv
        Q, K, V, dO = (torch.randn((n_heads, n, w), generator=gen, device=shared.gpu) for n_heads, n, w in
                       ((H, ROWS, k), (hkv, COLS, k), (hkv, COLS, kv), (H, ROWS, kv)))
        batched.max_heads = None
        want = _step(loop, Q, K, V, dO)
        whole = _step(batched, Q, K, V, dO)
        batched.max_heads = cap
        assert batched.head_chunks(H, k, kv, g) == chunks
        calls.clear()
        got = _step(batched, Q, K, V, dO)
        assert calls == ([("gqa", hi - lo) for lo, hi in chunks] if chunks else [("one", 1)] * H), calls
        for name in ("O", "dQ", "dK", "dV"):
            assert torch.equal(_raw(got[name]), _raw(want[name])), f"H_kv={hkv} cap={cap}: {name} differs from the loop"
            assert torch.equal(_raw(whole[name]), _raw(want[name])), f"H_kv={hkv}: {name} in one launch differs from the loop"
    loop.close()
    batched.close()
