"""Fused attention on 16-bit matrices on the device (spmv_csr_attention_forward_16, _backward_q_16, _backward_kv_16, the nine
CsrMatrix methods on bfloat16 / float16 tensors, and the holder).  The contract has no tolerance: every element of O, dQ, dK
and dV is, bit for bit, torch's round-to-nearest-even conversion of what the fp32 _gqa call writes on the same operands
widened to fp32, and stats and delta are that call's bits; backward_q forms delta from the 16-bit O it is given.  Only the
holder's comparison with torch's dense autograd has a bound.

Patterns P1 and P2 of tests/_order_cases.py: unsorted rows with repeated keys, lengths on both sides of every step and of the
512 boundary, empty rows, every row of P1's transpose in pieces, most of P2's keys listed by nobody.  Every operand of a call
lives in a buffer of its own between guard bands of a recognisable bit pattern: outputs start as NaN, the gaps between rows
and between heads must be intact afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import _order_cases as OC
from _util import RTOL
from test_gpu_attention_gqa import _dense_gqa, _magnitudes, _pattern as gqa_pattern

pytestmark = pytest.mark.gpu

H, HKV = 4, 2
GEOMETRIES = OC.GEOMETRIES + ((8, 8), (24, 32))        # V = 1, 4, 16, 16, 4, 2, 8
SCALES = (0.3, -0.7)
GUARD_BITS, NAN_BITS, GUARD_N = 0x5A5A, 0x7FFF, 1024   # a finite number and a NaN in both dtypes
NAMES = ("O", "stats", "delta", "dQ", "dK", "dV")


def _dtype(name):
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16}[name]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want):
    """Equal bits, or NaN against NaN."""
    import torch
    return bool(((_bits(got) == _bits(want)) | (torch.isnan(got) & torch.isnan(want))).all())


def _truncated_bits(x, dtype):
    """The bits of fp32 x converted to dtype by dropping what does not fit (round toward zero)."""
    import torch
    if dtype == torch.bfloat16:
        return (x.contiguous().view(torch.int32) >> 16).to(torch.int16)
    r = x.to(dtype)
    return torch.where(r.float().abs() > x.abs(), _bits(r) - 1, _bits(r))


class Handles:
    def __init__(self, pkg, s, gpu, heads):
        import torch
        self.s = s
        self.keep = (torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu), torch.zeros(s.nnz, dtype=torch.float32, device=gpu))
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=False)
        self.A.attention_plan_heads(heads)
        self.T.attention_plan_heads(heads)

    def close(self):
        self.T.close()
        self.A.close()


def _up4(n):
    return (n + 3) // 4 * 4


# (leading dimension of a matrix of w columns, elements from one head to the next); every stride is a multiple of 4 elements
LAYOUTS = {
    "ld4": lambda heads, rows, w: (_up4(w) + 4, rows * (_up4(w) + 4) + 8),                 # every ld % 4 == 0: 8-byte accesses
    "odd": lambda heads, rows, w: (w + 1 + w % 2, _up4(rows * (w + 1 + w % 2)) + 4),       # an odd ld: 2-byte accesses
    "blocks": lambda heads, rows, w: (heads * _up4(w), _up4(w)),                           # column blocks of one wide matrix
    "blocks_odd": lambda heads, rows, w: (heads * _up4(w) + 1, _up4(w)),                   # the same on the 2-byte path
}


class Guarded:
    """(heads, rows, w) elements of `dtype` at strides (stride, ld, 1) in a flat buffer of its own between guard bands.
    Everything that is no element holds GUARD_BITS; an output's elements start as NaN."""

    def __init__(self, gpu, dtype, heads, rows, w, ld, stride, fill=None):
        import torch
        span = (heads - 1) * stride + (rows - 1) * ld + w
        self.raw = torch.full((2 * GUARD_N + span,), GUARD_BITS, dtype=torch.int16, device=gpu)
        self.view = torch.as_strided(self.raw.view(dtype), (heads, rows, w), (stride, ld, 1), GUARD_N)
        own = torch.zeros_like(self.raw, dtype=torch.bool)
        torch.as_strided(own, (heads, rows, w), (stride, ld, 1), GUARD_N).fill_(True)
        self.gaps = ~own
        if fill is None:
            torch.as_strided(self.raw, (heads, rows, w), (stride, ld, 1), GUARD_N).fill_(NAN_BITS)
        else:
            self.view.copy_(fill)

    def intact(self):
        return bool((self.raw[self.gaps] == GUARD_BITS).all())


def run16(h, d, layout, scale, one_head=False):
    """The three 16-bit calls on the operands d (Q, dO: H heads; K, V: HKV heads; one_head: head 0 of each through the 2-D
    methods) laid out by `layout`; returns the outputs and asserts that nothing but their own elements was written."""
    import torch
    A, T = h.A, h.T
    gpu, dtype = d["Q"].device, d["Q"].dtype
    heads, kvh = (1, 1) if one_head else (d["Q"].shape[0], d["K"].shape[0])
    k, kv = d["Q"].shape[2], d["V"].shape[2]
    lay = LAYOUTS[layout]
    made = []

    def mat(n_heads, rows, w, fill=None):
        ld, stride = lay(n_heads, rows, w)
        made.append(Guarded(gpu, dtype, n_heads, rows, w, ld, stride, None if fill is None else fill[:n_heads]))
        return made[-1].view

    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)      # noqa: E731
    Q, dO, K, V = mat(heads, A.rows, k, d["Q"]), mat(heads, A.rows, kv, d["dO"]), mat(kvh, A.cols, k, d["K"]), mat(kvh, A.cols, kv, d["V"])
    out = dict(O=mat(heads, A.rows, kv), stats=nan(heads, A.rows, 2), delta=nan(heads, A.rows), dQ=mat(heads, A.rows, k),
               dK=mat(kvh, A.cols, k), dV=mat(kvh, A.cols, kv))
    if one_head:
        o = {n: t[0] for n, t in out.items()}
        A.attention_forward(Q[0], K[0], V[0], o["O"], o["stats"], scale)
        A.attention_backward_q(Q[0], K[0], V[0], o["O"], dO[0], o["stats"], o["delta"], o["dQ"], scale)
        T.attention_backward_kv(Q[0], K[0], V[0], dO[0], o["stats"], o["delta"], o["dK"], o["dV"], scale)
    else:
        A.attention_forward_gqa(Q, K, V, out["O"], out["stats"], scale)
        A.attention_backward_q_gqa(Q, K, V, out["O"], dO, out["stats"], out["delta"], out["dQ"], scale)
        T.attention_backward_kv_gqa(Q, K, V, dO, out["stats"], out["delta"], out["dK"], out["dV"], scale)
    torch.cuda.synchronize()
    assert all(m.intact() for m in made), f"{layout}: a pass wrote outside its outputs' own elements"
    return out


def reference(h, d, scale, one_head=False):
    """What the contract says: the fp32 _gqa calls on the widened operands (backward_q on the widened ROUNDED O), as fp32; the
    caller rounds O, dQ, dK and dV with torch's conversion."""
    import torch
    A, T = h.A, h.T
    nq, nk = (1, 1) if one_head else (d["Q"].shape[0], d["K"].shape[0])
    Q, dO, K, V = d["Q"][:nq].float(), d["dO"][:nq].float(), d["K"][:nk].float(), d["V"][:nk].float()
    k, kv, gpu = Q.shape[2], V.shape[2], Q.device
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)      # noqa: E731
    w = dict(O=nan(nq, A.rows, kv), stats=nan(nq, A.rows, 2), delta=nan(nq, A.rows), dQ=nan(nq, A.rows, k), dK=nan(nk, A.cols, k),
             dV=nan(nk, A.cols, kv))
    A.attention_forward_gqa(Q, K, V, w["O"], w["stats"], scale)
    O16 = w["O"].to(d["Q"].dtype).float()
    A.attention_backward_q_gqa(Q, K, V, O16, dO, w["stats"], w["delta"], w["dQ"], scale)
    T.attention_backward_kv_gqa(Q, K, V, dO, w["stats"], w["delta"], w["dK"], w["dV"], scale)
    torch.cuda.synchronize()
    return w


class Shared:
    def __init__(self, pkg, gpu):
        self.pkg, self.gpu = pkg, gpu
        self.h = {name: Handles(pkg, OC.pattern(name), gpu, H) for name in ("P1", "P2")}
        self._gqa = None

    def gqa(self):
        """test_gpu_attention_gqa's pattern (no repeated keys: torch's dense autograd can state it), planned for H heads."""
        if self._gqa is None:
            self._gqa = Handles(self.pkg, gqa_pattern(), self.gpu, H)
        return self._gqa

    def data(self, h, k, kv, dtype, seed):
        """General random numbers rounded to the dtype, +0 and -0 among them; different in every head."""
        import torch
        gen = torch.Generator(device=self.gpu).manual_seed(seed)
        out = {}
        for name, heads, n, w in (("Q", H, h.A.rows, k), ("K", HKV, h.A.cols, k), ("V", HKV, h.A.cols, kv), ("dO", H, h.A.rows, kv)):
            t = torch.randn((heads, n, w), generator=gen, device=self.gpu, dtype=torch.float32)
            z = torch.rand((heads, n, w), generator=gen, device=self.gpu)
            t = torch.where(z < 0.02, torch.zeros_like(t), t)
            t = torch.where(z > 0.98, -torch.zeros_like(t), t)
            out[name] = t.to(dtype)
        assert bool((_bits(out["Q"]) == 0).any()) and bool((_bits(out["Q"]) == -32768).any()), "+0 and -0 are among the data"
        return out

    def close(self):
        for h in self.h.values():
            h.close()
        if self._gqa is not None:
            self._gqa.close()


@pytest.fixture(scope="module")
def shared(pkg, gpu):
    sh = Shared(pkg, gpu)
    yield sh
    sh.close()


def assert_contract(got, want, dtype, tag, teeth=True):
    import torch
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.shape == w.shape, f"{tag}: {name} is {tuple(g.shape)}"
        if name in ("stats", "delta"):
            assert g.dtype == torch.float32 and _same(g, w), f"{tag}: {name} differs in a bit from the fp32 call's"
            continue
        assert g.dtype == dtype
        rounded = w.to(dtype)
        assert _same(g, rounded), (f"{tag}: {name} differs in a bit from the rounded fp32 result at "
                                   f"{int((_bits(g) != _bits(rounded)).sum())} of {g.numel()} elements")
        if teeth:       # the data tell rounding from truncation on this output
            assert bool((_truncated_bits(w, dtype) != _bits(rounded)).any()), f"{tag}: {name} cannot tell rounding from truncation"


# ---- the contract, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("k,kv", GEOMETRIES, ids=[f"k{k}-kv{kv}" for k, kv in GEOMETRIES])
@pytest.mark.parametrize("pattern", ["P1", "P2"])
def test_16bit_calls_are_the_fp32_calls_rounded_once(shared, pattern, k, kv, dt):
    dtype, h = _dtype(dt), shared.h[pattern]
    for si, scale in enumerate(SCALES):
        d = shared.data(h, k, kv, dtype, 1600 + 10 * k + kv + si)
        for one_head in (False, True):
            want = reference(h, d, scale, one_head)
            for layout in ("ld4", "odd"):
                got = run16(h, d, layout, scale, one_head)
                assert_contract(got, want, dtype, f"{pattern} k={k} kv={kv} {dt} {layout} scale={scale} {'one head' if one_head else 'H=4 on 2'}")


# ---- column blocks and padded rows between guard elements ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("k,kv", [(6, 10), (3, 2), (24, 32), (41, 63)], ids=["k6-kv10", "k3-kv2", "k24-kv32", "k41-kv63"])
def test_16bit_outputs_as_column_blocks_touch_nothing_else(shared, k, kv, dt):
    """(run16 checks the guard elements: nothing at or past a width, between rows or between heads is written.  Padded rows
    on both load paths run in the test above between the same guards.)"""
    dtype, h = _dtype(dt), shared.h["P1"]
    d = shared.data(h, k, kv, dtype, 1700 + k)
    want = reference(h, d, 0.3)
    for layout in ("blocks", "blocks_odd"):
        got = run16(h, d, layout, 0.3)
        assert_contract(got, want, dtype, f"k={k} kv={kv} {dt} {layout}", teeth=False)
        if layout == "blocks":
            assert got["dQ"].stride() == (_up4(k), H * _up4(k), 1) and got["dK"].stride() == (_up4(k), HKV * _up4(k), 1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_16bit_refusals_launch_nothing(shared, pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h = shared.h["P2"]
    rows, cols, k, kv, ld = h.A.rows, h.A.cols, 8, 8, 8
    dtype = torch.bfloat16
    ones = lambda heads, n: torch.ones((heads, n, ld), dtype=dtype, device=gpu)       # noqa: E731
    Q, K, V, dO, O_in = ones(H, rows), ones(H, cols), ones(H, cols), ones(H, rows), ones(H, rows)
    stats_in, delta_in = torch.zeros((H, rows, 2), device=gpu), torch.zeros((H, rows), device=gpu)
    outs = {n: torch.full((H, r, w), float("nan"), dtype=dt, device=gpu) for n, r, w, dt in
            (("O", rows, ld, dtype), ("dQ", rows, ld, dtype), ("dK", cols, ld, dtype), ("dV", cols, ld, dtype),
             ("stats", rows, 2, torch.float32), ("delta", rows, 1, torch.float32))}
    st = capi._stream_handle()
    good = dict(heads=4, q=rows * ld, k=cols * ld, v=cols * ld, o=rows * ld, d_o=rows * ld, stats=2 * rows, delta=rows,
                dq=rows * ld, dk=cols * ld, dv=cols * ld)

    def call(which, group=2, dt=capi.ATTN_BF16, shift=None, **change):
        hs = capi.AttnHeads(**dict(good, **change))
        p = lambda t, name=None: C.c_void_p(t.data_ptr() + (2 if name is not None and name == shift else 0))       # noqa: E731  (2 bytes: one element)
        if which == "forward":
            return lib.spmv_csr_attention_forward_16(h.A._h, C.byref(hs), group, dt, 0.25, k, p(Q, "Q"), ld, p(K, "K"), ld, kv, p(V), ld,
                                                     p(outs["O"], "O"), ld, p(outs["stats"]), st)
        if which == "backward_q":
            return lib.spmv_csr_attention_backward_q_16(h.A._h, C.byref(hs), group, dt, 0.25, k, p(Q, "Q"), ld, p(K, "K"), ld, kv, p(V), ld,
                                                        p(O_in, "O"), ld, p(dO), ld, p(stats_in), p(outs["delta"]), p(outs["dQ"], "dQ"), ld, st)
        return lib.spmv_csr_attention_backward_kv_16(h.T._h, C.byref(hs), group, dt, 0.25, k, p(Q, "Q"), ld, p(K, "K"), ld, kv, p(V), ld,
                                                     p(dO), ld, p(stats_in), p(delta_in), p(outs["dK"], "dK"), ld, p(outs["dV"]), ld, st)

    for which in ("forward", "backward_q", "backward_kv"):
        name = f"spmv_csr_attention_{which}_16"
        out_name = {"forward": "O", "backward_q": "dQ", "backward_kv": "dK"}[which]
        cases = [(dict(dt=0), "dtype"), (dict(dt=3), "dtype"), (dict(shift="Q"), "8-byte aligned"), (dict(shift=out_name), "8-byte aligned"),
                 (dict(q=rows * ld + 2), "no multiple of 4"), (dict(k=cols * ld + 6), "no multiple of 4"),
                 (dict(group=0), "group"), (dict(group=3), "group"), (dict(reserved=1), "reserved"), (dict(heads=0), "heads"), (dict(k=-4), "negative")]
        for change, word in cases:
            assert call(which, **change) == capi.ERR_INVALID, f"{which} {change}"
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, msg
        assert call(which, heads=H + 2) == capi.ERR_NOT_PLANNED       # (more than the fixture planned; 6 % 2 == 0)
        assert name in lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs.values()), "a refused call wrote to an output"
    for which in ("forward", "backward_q", "backward_kv"):                 # and the same calls, unchanged, are accepted
        assert call(which) == capi.OK, lib.spmv_last_error()
        assert call(which, dt=capi.ATTN_FP16) == capi.OK, lib.spmv_last_error()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t[:4 if n in ("O", "dQ", "stats", "delta") else 2]).any()) for n, t in outs.items())


# ---- graph capture --------------------------------------------------------------------------------------------------------------
def test_16bit_calls_are_graph_capturable(shared, gpu):
    import torch
    h, k, kv, scale, dtype = shared.h["P1"], 12, 16, 0.3, torch.bfloat16
    seeds = (1801, 1802, 1803)
    run16(h, shared.data(h, k, kv, dtype, seeds[0]), "ld4", scale)          # (the warm run)
    d0 = shared.data(h, k, kv, dtype, seeds[0])
    Q, dO, K, V = (d0[n].clone() for n in ("Q", "dO", "K", "V"))
    rows, cols = h.A.rows, h.A.cols
    nan = lambda dt, *shape: torch.full(shape, float("nan"), dtype=dt, device=gpu)      # noqa: E731
    outs = dict(O=nan(dtype, H, rows, kv), stats=nan(torch.float32, H, rows, 2), delta=nan(torch.float32, H, rows), dQ=nan(dtype, H, rows, k),
                dK=nan(dtype, HKV, cols, k), dV=nan(dtype, HKV, cols, kv))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream; the calls take the current stream)
        h.A.attention_forward_gqa(Q, K, V, outs["O"], outs["stats"], scale)
        h.A.attention_backward_q_gqa(Q, K, V, outs["O"], dO, outs["stats"], outs["delta"], outs["dQ"], scale)
        h.T.attention_backward_kv_gqa(Q, K, V, dO, outs["stats"], outs["delta"], outs["dK"], outs["dV"], scale)
    for seed in seeds[1:]:
        d = shared.data(h, k, kv, dtype, seed)
        Q.copy_(d["Q"]), dO.copy_(d["dO"]), K.copy_(d["K"]), V.copy_(d["V"])
        for o in outs.values():
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run16(h, d, "ld4", scale)
        for name in NAMES:
            assert _same(outs[name], eager[name]), f"replay with seed {seed}: {name} differs from the eager call"


# ---- the holder -------------------------------------------------------------------------------------------------------------------
def _step(att, Q, K, V, dO):
    import torch
    q, k, v = (t.detach().requires_grad_(True) for t in (Q, K, V))
    O = att(q, k, v)
    O.backward(dO)
    torch.cuda.synchronize()
    return dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_16bit_holder_modes_agree_equal_the_direct_calls_and_match_dense_autograd(shared, dt):
    """H = 4 on 4 and on 2 K/V heads: "batched" and "loop" give the same bits through autograd; O is the direct call's, the
    gradients are the direct calls' on the saved 16-bit O.  Against torch's fp64 dense autograd on the widened inputs, with the
    magnitudes of tests/test_gpu_fused_attention.py: the normalised error is at most max(4 x that of torch's dense autograd run
    in the same 16-bit dtype, RTOL)."""
    import torch
    dtype, h = _dtype(dt), shared.gqa()
    s, gpu = h.s, shared.gpu
    SA = shared.pkg.sparse_attention
    scale, k, kv = 0.25, 24, 32
    loop, batched = (SA.FusedSparseAttention(s.rows, s.cols, h.keep[0], h.keep[1], scale=scale, heads=m) for m in ("loop", "batched"))
    mask = torch.zeros((s.rows, s.cols), dtype=torch.bool, device=gpu)
    mask[torch.from_numpy(s.row_of).to(gpu), torch.from_numpy(s.ci.astype(np.int64)).to(gpu)] = True
    for hkv in (H, HKV):
        g = H // hkv
        gen = torch.Generator(device=gpu).manual_seed(1900 + hkv)
        Q, K, V, dO = (torch.randn((n_heads, n, w), generator=gen, device=gpu).to(dtype) for n_heads, n, w in
                       ((H, s.rows, k), (hkv, s.cols, k), (hkv, s.cols, kv), (H, s.rows, kv)))
        got_l, got_b = _step(loop, Q, K, V, dO), _step(batched, Q, K, V, dO)
        for name in ("O", "dQ", "dK", "dV"):
            assert got_b[name].dtype == dtype and got_b[name].shape == got_l[name].shape
            assert _same(got_b[name], got_l[name]), f"H_kv={hkv} {name}: batched differs from the loop"
        assert got_b["dK"].shape == (hkv, s.cols, k) and got_b["dV"].shape == (hkv, s.cols, kv)
        # the direct calls: forward, then backward on the saved (rounded) O
        nan = lambda dty, *shape: torch.full(shape, float("nan"), dtype=dty, device=gpu)      # noqa: E731
        o = dict(O=nan(dtype, H, s.rows, kv), stats=nan(torch.float32, H, s.rows, 2), delta=nan(torch.float32, H, s.rows),
                 dQ=nan(dtype, H, s.rows, k), dK=nan(dtype, hkv, s.cols, k), dV=nan(dtype, hkv, s.cols, kv))
        h.A.attention_forward_gqa(Q, K, V, o["O"], o["stats"], scale)
        h.A.attention_backward_q_gqa(Q, K, V, got_b["O"], dO, o["stats"], o["delta"], o["dQ"], scale)
        h.T.attention_backward_kv_gqa(Q, K, V, dO, o["stats"], o["delta"], o["dK"], o["dV"], scale)
        torch.cuda.synchronize()
        for name in ("O", "dQ", "dK", "dV"):
            assert _same(got_b[name], o[name]), f"H_kv={hkv} {name}: the holder differs from the direct call"
        r64, P = _dense_gqa(mask, scale, Q, K, V, dO, torch.float64, g)
        r16, _ = _dense_gqa(mask, scale, Q, K, V, dO, dtype, g)
        mags = _magnitudes(mask, scale, Q, K, V, dO, P, g)
        for what in ("O", "dQ", "dK", "dV"):
            gg, g64, g16, mag = got_b[what], r64[what], r16[what], mags[what]
            live = mag > 0
            assert bool(live.any()) and bool((gg[~live] == 0).all()), f"{what}: a value where nothing contributes"
            ours = float(((gg.double() - g64).abs()[live] / mag[live]).max())
            yard = float(((g16.double() - g64).abs()[live] / mag[live]).max())
            print(f"16-bit holder {dt} H_kv={hkv} {what}: normalised error fused {ours:.3g}, torch {dt} dense autograd {yard:.3g}")
            assert ours <= max(4.0 * yard, RTOL), f"{what}: {ours:.3g} against {yard:.3g} of torch's {dt} dense autograd"
    # 2-D operands alike
    got = _step(loop, Q[0], K[0], V[0], dO[0])
    assert got["O"].dtype == dtype and got["dK"].shape == (s.cols, k)
    with pytest.raises(ValueError, match="share one dtype"):
        loop(Q, K.float(), V)
    loop.close()
    batched.close()
