"""The wide fused-attention calls on the device (spmv_csr_attention_*_wide: head widths up to 128 on lane groups of 32 that
walk their rows in steps of T_wide nonzeros; include/spmv_hip.h "Fused attention at head widths up to 128").

Patterns P1 and P2 of tests/_order_cases.py: 40 keys, unsorted rows with repeated keys, row lengths on both sides of every
step and of the 512 boundary, every transposed row of P1 in pieces.  Widths (tests/_attention_wide.WIDTHS): (128, 128), (65, 65)
-- the first past the other calls' limit --, (68, 128), (128, 4) and (4, 100) -- k and kv on different sides of 64 -- and
(97, 66), no multiples of 4.

order       the three passes bit for bit against the numpy statement of the documented order at (V, T) = (32, T_wide): the
            backward passes on general data with caller-made stats and delta, the forward pass on the data whose every expf
            argument is exact (tests/test_attention_wide_host.py asserts the premise); again with a bias and dBias; again with
            four query heads on two K/V heads, one key's gradients -0 in every head.  The host side emulates the rows whose
            lengths _order_cases chose on purpose, not the filler rows.
padding     operands of (64, 20), (8, 40), (16, 12) padded with zeros to (128, 128): the existing _bias and _gqa calls' bits in
            the original columns, +0 in the padded ones.
narrow      at widths up to 64 a _wide call is the existing most general call, bit for bit.
16-bit      bf16 and fp16: every output the fp32 wide call's on the widened operands, rounded once to nearest even.
placement   both load paths, column blocks of one (n, heads * 128) tensor, NaN-filled outputs between guard elements, a row
            block with a rebased row_ptr.
live expf   general scores against the per-nonzero fp64 reference under the rule of tests/test_gpu_attention_multigraph.py.
holder      FusedSparseAttention(wide=True) at width 128 in both heads modes against torch's fp64 dense autograd.
refusals, limits, one graph capture.
"""
import ctypes as C

import numpy as np
import pytest

import _attention_bias as AB
import _attention_order as AO
import _attention_wide as AW
import _order_cases as OC
from _util import RTOL
from test_gpu_attention16 import LAYOUTS, Guarded, _bits as bits16, _dtype, _same, _truncated_bits
from test_gpu_attention_gqa import _magnitudes, _pattern as gqa_pattern
from test_gpu_attention_multigraph import _errors, _references

pytestmark = pytest.mark.gpu

H, HKV, G = 4, 2, 2
f32 = np.float32
NAMES = ("O", "stats", "delta", "dQ", "dBias", "dK", "dV")


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _folded(a):
    return (np.ascontiguousarray(a, f32) + f32(0)).view(np.uint32)


def _same_bits(tag, got, want, fold=True):
    """Every value of `got` (device tensor or numpy) has the bits of `want`; returns how many were compared."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, tag
    g, w = (_folded(got), _folded(want)) if fold else (_bits(got), _bits(want))
    bad = np.flatnonzero((g != w).reshape(-1))
    if bad.size:
        n = int(bad[0])
        raise AssertionError(f"{tag}: {bad.size} of {g.size} values differ in a bit; the first at flat index {n}: "
                             f"{got.reshape(-1)[n]!r} ({g.reshape(-1)[n]:#010x}) against {want.reshape(-1)[n]!r} ({w.reshape(-1)[n]:#010x})")
    return int(g.size)


class Handles:
    """A pattern, its transpose (with the map: the bias of backward_kv) and both plans, narrow and wide, for `heads` heads."""

    def __init__(self, pkg, s, gpu, heads=H, wide=True):
        import torch
        self.s = s
        self.keep = (_dev(gpu, s.rp), _dev(gpu, s.ci), torch.zeros(s.nnz, dtype=torch.float32, device=gpu))
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=True)
        for m in (self.A, self.T):
            m.attention_plan_heads(heads)
            if wide:
                m.attention_plan_wide(heads)
        self.tp, self.ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
        rp_t, ci_t, _ = self.T.download()
        assert np.array_equal(rp_t, self.tp) and np.array_equal(ci_t, self.ti)

    def bias_t(self, bias):
        import torch
        out = torch.empty_like(bias)
        self.T.transpose_gather(bias, out)
        return out

    def close(self):
        self.T.close()
        self.A.close()


@pytest.fixture(scope="module")
def shared(pkg, gpu):
    h = {name: Handles(pkg, OC.pattern(name), gpu) for name in ("P1", "P2")}
    yield h
    for x in h.values():
        x.close()


def _nan(gpu, *shape, dtype=None):
    import torch
    return torch.full(shape, float("nan"), dtype=dtype or torch.float32, device=gpu)


def run(h, Q, K, V, dO, scale, bias=None, stats=None, O=None, delta=None, call="wide", want_dbias=True):
    """The three passes on (heads, n, width) device tensors into NaN-filled outputs.  stats, O, delta: caller-made inputs of
    the backward passes (else the forward pass's and backward_q's).  call: "wide", or the existing most general call ("bias"
    with a bias, else "gqa")."""
    import torch
    A, T = h.A, h.T
    gpu, dt = Q.device, Q.dtype
    nq, nk, k, kv = Q.shape[0], K.shape[0], Q.shape[2], V.shape[2]
    out = dict(O=_nan(gpu, nq, A.rows, kv, dtype=dt), stats=_nan(gpu, nq, A.rows, 2), delta=_nan(gpu, nq, A.rows),
               dQ=_nan(gpu, nq, A.rows, k, dtype=dt), dK=_nan(gpu, nk, A.cols, k, dtype=dt), dV=_nan(gpu, nk, A.cols, kv, dtype=dt))
    if bias is not None and want_dbias:
        out["dBias"] = _nan(gpu, nq, A.nnz)
    bt = h.bias_t(bias) if bias is not None else None
    st = out["stats"] if stats is None else stats
    o_in = out["O"] if O is None else O
    if call == "wide":
        A.attention_forward_wide(Q, K, V, out["O"], out["stats"], bias, scale)
        A.attention_backward_q_wide(Q, K, V, o_in, dO, st, out["delta"], out["dQ"], bias, out.get("dBias"), scale)
        T.attention_backward_kv_wide(Q, K, V, dO, st, out["delta"] if delta is None else delta, out["dK"], out["dV"], bt, scale)
    elif bias is not None:
        A.attention_forward_bias(Q, K, V, bias, out["O"], out["stats"], scale)
        A.attention_backward_q_bias(Q, K, V, bias, o_in, dO, st, out["delta"], out["dQ"], out.get("dBias"), scale)
        T.attention_backward_kv_bias(Q, K, V, bt, dO, st, out["delta"] if delta is None else delta, out["dK"], out["dV"], scale)
    else:
        A.attention_forward_gqa(Q, K, V, out["O"], out["stats"], scale)
        A.attention_backward_q_gqa(Q, K, V, o_in, dO, st, out["delta"], out["dQ"], scale)
        T.attention_backward_kv_gqa(Q, K, V, dO, st, out["delta"] if delta is None else delta, out["dK"], out["dV"], scale)
    torch.cuda.synchronize()
    return out


def chosen_rows(s):
    """The rows whose lengths tests/_order_cases.py chose (every step and piece boundary, one key L times, a low prefix)."""
    chosen = set(OC.LENGTHS) | set(OC.ONE_KEY) | {n for n, _ in OC.LOW_FIRST}
    return [i for i, n in enumerate(np.diff(s.rp).tolist()) if n in chosen]


# ---- 1. the order, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("k,kv", AW.WIDTHS, ids=[f"k{k}-kv{kv}" for k, kv in AW.WIDTHS])
def test_wide_passes_have_the_documented_order(shared, gpu, k, kv, with_bias):
    h = shared["P1"]
    s = h.s
    rows, keys = chosen_rows(s), list(range(0, s.cols, 5))
    nz = np.concatenate([np.arange(s.rp[i], s.rp[i + 1]) for i in rows])
    bias = AB.exact_bias(s, 7 * k + kv) if with_bias else None
    bias_t = AB.transposed_bias(s.ci, bias) if with_bias else None
    d_bias = _dev(gpu, bias)[None] if with_bias else None
    counts = {}
    for case in ("maxima", "stats_q0", "stats_k0"):
        d = OC.attention_data("P1", case, k, kv)
        scale = d["scale"]
        Q, K, V, dO = (_dev(gpu, d[n])[None] for n in ("Q", "K", "V", "dO"))
        made = case.startswith("stats")
        got = run(h, Q, K, V, dO, scale, d_bias, stats=_dev(gpu, d["stats"])[None] if made else None,
                  O=_dev(gpu, d["O"])[None] if made else None, delta=_dev(gpu, d["delta"])[None] if made else None)
        O, stats = AW.attention_forward(s.rp, s.ci, d["Q"], d["K"], d["V"], scale, bias, only=rows)
        want = {"O": O[rows], "stats": stats[rows]}
        if made:
            O, stats = d["O"], d["stats"]
        dQ, delta, dB = AW.attention_backward_q(s.rp, s.ci, d["Q"], d["K"], d["V"], O, d["dO"], stats, scale, bias, only=rows)
        want.update(dQ=dQ[rows], delta=delta[rows])
        if with_bias:
            want["dBias"] = dB[nz]
        if made:            # (maxima: the forward pass and backward_q, as in tests/test_gpu_order.py)
            dK, dV = AW.attention_backward_kv(h.tp, h.ti, d["Q"], d["K"], d["V"], d["dO"], stats, d["delta"], scale, bias_t, only=keys)
            want.update(dK=dK[keys], dV=dV[keys])
        pick = {"O": rows, "stats": rows, "dQ": rows, "delta": rows, "dBias": nz, "dK": keys, "dV": keys}
        for w in want:
            g = got[w][0].cpu().numpy()
            counts[w] = counts.get(w, 0) + _same_bits(f"P1 {case} k={k} kv={kv} bias={with_bias}: {w}", g[pick[w]], want[w])
        assert not np.isnan(got["dQ"].cpu().numpy()).any() and not np.isnan(got["O"].cpu().numpy()).any(), "every row is written"
    print(f"wide k={k} kv={kv} bias={with_bias}: values compared bit for bit with the documented order: "
          + ", ".join(f"{w} {n}" for w, n in counts.items()))


@pytest.mark.parametrize("name,case,minus_zero", [("P2", "stats_k0", True), ("P1", "stats_q0", False)], ids=["P2-minus-zero", "P1-pieces"])
@pytest.mark.parametrize("k,kv", AW.WIDTHS, ids=[f"k{k}-kv{kv}" for k, kv in AW.WIDTHS])
def test_wide_gqa_folds_the_heads_in_the_documented_order(shared, gpu, k, kv, name, case, minus_zero):
    """Four query heads on two K/V heads, caller-made stats and delta: dQ and delta per head, dK_c and dV_c the fold of the two
    single-head emulations from head 0's value.  On P2 one key's gradients are -0 in every head (the zeros are not folded in
    the comparison); on P1 every key's row goes in pieces (the sum over the heads of a group after the sum over the pieces)."""
    import torch
    h = shared[name]
    s = h.s
    per = [OC.attention_data(name, case, k, kv, head=y, minus_zero=minus_zero) for y in range(H)]
    Ks, Vs = [per[c]["K"] for c in range(HKV)], [per[c]["V"] for c in range(HKV)]
    scale = per[0]["scale"]
    lengths = np.diff(h.tp)
    if minus_zero:
        j0 = OC.neg_zero_key()
        keys = sorted({j0} | set(np.argsort(-lengths)[:8].tolist()) | set(np.flatnonzero(lengths == 0)[:2].tolist()))
        rows = AW.one_row_per_length(s.rp)[:12]
    else:
        keys, rows = [0, 21, 39], chosen_rows(s)[::4]
    stack = lambda arrays: _dev(gpu, np.stack(arrays))           # noqa: E731
    Q, dO, O, stats, delta_in = (stack([d[n] for d in per]) for n in ("Q", "dO", "O", "stats", "delta"))
    got = run(h, Q, stack(Ks), stack(Vs), dO, scale, None, stats=stats, O=O, delta=delta_in)
    single = []
    for y, d in enumerate(per):
        K, V = Ks[y // G], Vs[y // G]
        dQ, delta, _ = AW.attention_backward_q(s.rp, s.ci, d["Q"], K, V, d["O"], d["dO"], d["stats"], scale, only=rows)
        dK, dV = AW.attention_backward_kv(h.tp, h.ti, d["Q"], K, V, d["dO"], d["stats"], d["delta"], scale, only=keys)
        single.append(dict(dQ=dQ, delta=delta, dK=dK, dV=dV))
    n = 0
    for y in range(H):
        n += _same_bits(f"head {y}: dQ", got["dQ"][y].cpu().numpy()[rows], single[y]["dQ"][rows])
        n += _same_bits(f"head {y}: delta", got["delta"][y].cpu().numpy()[rows], single[y]["delta"][rows])
    for c in range(HKV):
        for w in ("dK", "dV"):
            fold = AO.gqa_fold([single[c * G + i][w] for i in range(G)])
            n += _same_bits(f"K/V head {c}: {w}", got[w][c].cpu().numpy()[keys], fold[keys], fold=not minus_zero)
    if minus_zero:
        assert np.all(np.signbit(got["dK"][:, j0].cpu().numpy())) and np.all(np.signbit(got["dV"][:, j0].cpu().numpy())), "the -0 key"
        assert not np.any(np.signbit(AO.gqa_fold([single[0]["dV"], single[1]["dV"]], from_zero=True)[j0]))
    assert torch.isfinite(got["dK"]).all() and torch.isfinite(got["dV"]).all()
    print(f"wide gqa {name} {case} k={k} kv={kv}: {n} values compared bit for bit")


# ---- 2. zero padding ---------------------------------------------------------------------------------------------------------------------
def _pad(t, w):
    import torch
    out = torch.zeros(t.shape[:-1] + (w,), dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


@pytest.mark.parametrize("with_bias", [False, True], ids=["gqa", "bias"])
@pytest.mark.parametrize("k,kv", [(64, 20), (8, 40), (16, 12)], ids=["k64-kv20", "k8-kv40", "k16-kv12"])
def test_zero_padded_operands_give_the_narrow_calls_bits(shared, gpu, k, kv, with_bias):
    """General data, four query heads on two K/V heads, caller-made stats (the narrow forward call's) and delta: the wide call
    on the operands padded to (128, 128) against the existing _bias (or _gqa) call on the unpadded ones.  The forward pass is
    compared on the exact-expf data (maxima)."""
    import torch
    h = shared["P1"]
    s = h.s
    Qn, dOn = OC.randn([k, kv, 1], (H, s.rows, k), (H, s.rows, kv))
    Kn, Vn = OC.randn([k, kv, 2], (HKV, s.cols, k), (HKV, s.cols, kv))
    Q, dO, K, V = (_dev(gpu, x) for x in (Qn, dOn, Kn, Vn))
    bias = _dev(gpu, OC.randn([k, kv, 3], (H, s.nnz))[0]) if with_bias else None
    scale = 0.3
    narrow = run(h, Q, K, V, dO, scale, bias, call="existing")
    wide = run(h, _pad(Q, 128), _pad(K, 128), _pad(V, 128), _pad(dO, 128), scale, bias, stats=narrow["stats"], O=_pad(narrow["O"], 128),
               delta=narrow["delta"])
    assert bool(torch.isfinite(narrow["dQ"]).all()) and bool((narrow["dK"] != 0).any())
    width = {"dQ": k, "dK": k, "dV": kv}
    n = 0
    for w in ("delta", "dBias", "dQ", "dK", "dV"):
        if w not in narrow:
            continue
        g = wide[w].cpu().numpy()
        if w in width:
            assert not _bits(g[..., width[w]:]).any(), f"{w}: a padded column is not +0"
            g = g[..., :width[w]]
        n += _same_bits(f"padded ({k}, {kv}) bias={with_bias}: {w}", g, narrow[w].cpu().numpy(), fold=False)
    # the forward pass: data whose every expf argument is exact
    per = [OC.attention_data("P1", "maxima", k, kv, head=y) for y in range(H)]
    Q, dO = (_dev(gpu, np.stack([d[x] for d in per])) for x in ("Q", "dO"))
    K, V = (_dev(gpu, np.stack([per[c][x] for c in range(HKV)])) for x in ("K", "V"))
    eb = _dev(gpu, np.stack([AB.exact_bias(s, 31 * k + y) for y in range(H)])) if with_bias else None
    narrow = run(h, Q, K, V, dO, 0.5, eb, call="existing")
    wide = run(h, _pad(Q, 128), _pad(K, 128), _pad(V, 128), _pad(dO, 128), 0.5, eb)
    g = wide["O"].cpu().numpy()
    assert not _bits(g[..., kv:]).any(), "O: a padded column is not +0"
    n += _same_bits("padded forward: O", g[..., :kv], narrow["O"].cpu().numpy(), fold=False)
    n += _same_bits("padded forward: stats", wide["stats"], narrow["stats"].cpu().numpy(), fold=False)
    print(f"zero padding ({k}, {kv}) -> (128, 128) bias={with_bias}: {n} values bit for bit the narrow call's")


# ---- 3. narrow widths through _wide --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["gqa", "bias"])
@pytest.mark.parametrize("k,kv", OC.GEOMETRIES, ids=[f"k{k}-kv{kv}" for k, kv in OC.GEOMETRIES])
def test_up_to_width_64_a_wide_call_is_the_existing_call(shared, gpu, k, kv, with_bias, dt):
    import torch
    dtype = torch.float32 if dt == "fp32" else torch.bfloat16
    for name in ("P1", "P2"):
        h = shared[name]
        s = h.s
        Qn, dOn = OC.randn([k, kv, 4], (H, s.rows, k), (H, s.rows, kv))
        Kn, Vn = OC.randn([k, kv, 5], (HKV, s.cols, k), (HKV, s.cols, kv))
        Q, dO, K, V = (_dev(gpu, x).to(dtype) for x in (Qn, dOn, Kn, Vn))
        bias = _dev(gpu, OC.randn([k, kv, 6], (H, s.nnz))[0]) if with_bias else None
        a, b = run(h, Q, K, V, dO, 0.3, bias), run(h, Q, K, V, dO, 0.3, bias, call="existing")
        assert set(a) == set(b)
        for w in a:
            assert _same(a[w], b[w]), f"{name} k={k} kv={kv} {dt} bias={with_bias}: {w} differs from the existing call"
        assert not bool(torch.isnan(a["dQ"].float()).any())


# ---- 4. 16-bit ---------------------------------------------------------------------------------------------------------------------------------
def _data16(gpu, h, k, kv, dtype, seed):
    """General numbers of `dtype` with +0 and -0 among them; different in every head."""
    import torch
    gen = torch.Generator(device=gpu).manual_seed(seed)
    out = {}
    for name, heads, n, w in (("Q", H, h.A.rows, k), ("K", HKV, h.A.cols, k), ("V", HKV, h.A.cols, kv), ("dO", H, h.A.rows, kv)):
        t = torch.randn((heads, n, w), generator=gen, device=gpu, dtype=torch.float32)
        z = torch.rand((heads, n, w), generator=gen, device=gpu)
        t = torch.where(z < 0.02, torch.zeros_like(t), t)
        t = torch.where(z > 0.98, -torch.zeros_like(t), t)
        out[name] = t.to(dtype)
    return out


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("k,kv", [(128, 128), (97, 66)], ids=["k128-kv128", "k97-kv66"])
def test_16bit_wide_calls_are_the_fp32_wide_calls_rounded_once(shared, gpu, k, kv, dt):
    """The approach of tests/test_gpu_attention16.py: operands in buffers of their own between guard elements, on the 8-byte and
    the 2-byte load path; the reference is the fp32 wide call on the widened operands (backward_q on the widened rounded O)."""
    import torch
    dtype = _dtype(dt)
    for name in ("P1", "P2"):
        h = shared[name]
        A, T = h.A, h.T
        d = _data16(gpu, h, k, kv, dtype, 2100 + k + kv)
        for with_bias in (False, True):
            bias = _dev(gpu, OC.randn([k, kv, 8], (H, h.s.nnz))[0]) if with_bias else None
            scale = -0.2 if with_bias else 0.15
            want = run(h, d["Q"].float(), d["K"].float(), d["V"].float(), d["dO"].float(), scale, bias)
            O16 = want["O"].to(dtype).float()
            again = run(h, d["Q"].float(), d["K"].float(), d["V"].float(), d["dO"].float(), scale, bias, stats=want["stats"], O=O16)
            want.update({w: again[w] for w in ("delta", "dQ", "dBias", "dK", "dV") if w in again})
            bt = h.bias_t(bias) if with_bias else None
            for layout in ("ld4", "odd"):
                made = []

                def mat(n_heads, rows, w, fill=None):
                    ld, stride = LAYOUTS[layout](n_heads, rows, w)
                    made.append(Guarded(gpu, dtype, n_heads, rows, w, ld, stride, fill))
                    return made[-1].view

                Q, dO, K, V = mat(H, A.rows, k, d["Q"]), mat(H, A.rows, kv, d["dO"]), mat(HKV, A.cols, k, d["K"]), mat(HKV, A.cols, kv, d["V"])
                got = dict(O=mat(H, A.rows, kv), stats=_nan(gpu, H, A.rows, 2), delta=_nan(gpu, H, A.rows), dQ=mat(H, A.rows, k),
                           dK=mat(HKV, A.cols, k), dV=mat(HKV, A.cols, kv))
                if with_bias:
                    got["dBias"] = _nan(gpu, H, A.nnz)
                A.attention_forward_wide(Q, K, V, got["O"], got["stats"], bias, scale)
                A.attention_backward_q_wide(Q, K, V, got["O"], dO, got["stats"], got["delta"], got["dQ"], bias, got.get("dBias"), scale)
                T.attention_backward_kv_wide(Q, K, V, dO, got["stats"], got["delta"], got["dK"], got["dV"], bt, scale)
                torch.cuda.synchronize()
                assert all(m.intact() for m in made), f"{layout}: a pass wrote outside its outputs' own elements"
                tag = f"{name} k={k} kv={kv} {dt} {layout} bias={with_bias}"
                for w in got:
                    if w in ("stats", "delta", "dBias"):
                        assert _same(got[w], want[w]), f"{tag}: {w} differs in a bit from the fp32 wide call's"
                        continue
                    rounded = want[w].to(dtype)
                    assert got[w].dtype == dtype and _same(got[w], rounded), f"{tag}: {w} is not the fp32 wide call's result rounded once"
                    assert bool((_truncated_bits(want[w], dtype) != bits16(rounded)).any()), f"{tag}: {w} cannot tell rounding from truncation"


# ---- 5. placement ------------------------------------------------------------------------------------------------------------------------------
class Guarded32:
    """(heads, rows, w) floats at strides (stride, ld, 1) in a flat buffer of its own; everything that is no element holds a
    guard value, an output's elements start as NaN."""
    GUARD, N = 3.0e35, 1024

    def __init__(self, gpu, heads, rows, w, ld, stride, fill=None):
        import torch
        span = (heads - 1) * stride + (rows - 1) * ld + w
        self.raw = torch.full((2 * self.N + span,), self.GUARD, dtype=torch.float32, device=gpu)
        self.view = torch.as_strided(self.raw, (heads, rows, w), (stride, ld, 1), self.N)
        own = torch.zeros_like(self.raw, dtype=torch.bool)
        torch.as_strided(own, (heads, rows, w), (stride, ld, 1), self.N).fill_(True)
        self.gaps = ~own
        self.view.fill_(float("nan")) if fill is None else self.view.copy_(fill)

    def intact(self):
        return bool((self.raw[self.gaps] == self.GUARD).all())


@pytest.mark.parametrize("k,kv", [(128, 128), (97, 66), (68, 128)], ids=["k128-kv128", "k97-kv66", "k68-kv128"])
def test_wide_outputs_do_not_depend_on_placement(shared, pkg, gpu, k, kv):
    """Stacked heads with every ld a multiple of 4, an odd ld (the 4-byte path), column blocks of one (n, heads * width) matrix
    (no copy) and the same on an odd ld: the same bits as the contiguous run, nothing written but the outputs' own elements.
    Then rows [r0, r1) of P1 as a handle of their own with a rebased row_ptr: the whole matrix's rows."""
    import torch
    h = shared["P1"]
    A, T, s = h.A, h.T, h.s
    Qn, dOn = OC.randn([k, kv, 9], (H, s.rows, k), (H, s.rows, kv))
    Kn, Vn = OC.randn([k, kv, 10], (HKV, s.cols, k), (HKV, s.cols, kv))
    d = {n: _dev(gpu, x) for n, x in (("Q", Qn), ("dO", dOn), ("K", Kn), ("V", Vn))}
    bias = _dev(gpu, OC.randn([k, kv, 11], (H, s.nnz))[0])
    scale = 0.11
    base = run(h, d["Q"], d["K"], d["V"], d["dO"], scale, bias)
    bt = h.bias_t(bias)
    for layout in ("ld4", "odd", "blocks", "blocks_odd"):
        made = []

        def mat(n_heads, rows, w, fill=None):
            ld, stride = LAYOUTS[layout](n_heads, rows, w)
            made.append(Guarded32(gpu, n_heads, rows, w, ld, stride, fill))
            return made[-1].view

        Q, dO, K, V = mat(H, A.rows, k, d["Q"]), mat(H, A.rows, kv, d["dO"]), mat(HKV, A.cols, k, d["K"]), mat(HKV, A.cols, kv, d["V"])
        if layout == "blocks" and k % 4 == 0:
            assert Q.stride() == (k, H * k, 1), "the heads are column blocks of one (rows, heads * k) matrix"
        got = dict(O=mat(H, A.rows, kv), stats=_nan(gpu, H, A.rows, 2), delta=_nan(gpu, H, A.rows), dQ=mat(H, A.rows, k),
                   dK=mat(HKV, A.cols, k), dV=mat(HKV, A.cols, kv), dBias=_nan(gpu, H, A.nnz))
        A.attention_forward_wide(Q, K, V, got["O"], got["stats"], bias, scale)
        A.attention_backward_q_wide(Q, K, V, got["O"], dO, got["stats"], got["delta"], got["dQ"], bias, got["dBias"], scale)
        T.attention_backward_kv_wide(Q, K, V, dO, got["stats"], got["delta"], got["dK"], got["dV"], bt, scale)
        torch.cuda.synchronize()
        assert all(m.intact() for m in made), f"{layout}: a pass wrote outside its outputs' own elements"
        for w in got:
            assert _same(got[w], base[w]), f"k={k} kv={kv} {layout}: {w} depends on the placement"
    # a row block: rows [r0, r1) with row_ptr rebased to 0 and col_idx cut to the block
    r0, r1 = 37, 151
    lo, hi = int(s.rp[r0]), int(s.rp[r1])
    assert (np.diff(s.rp[r0:r1 + 1]) > 512).any(), "the block holds a row in pieces"
    keep = (_dev(gpu, (s.rp[r0:r1 + 1] - lo).astype(np.int32)), _dev(gpu, s.ci[lo:hi].astype(np.int32)),
            torch.zeros(hi - lo, dtype=torch.float32, device=gpu))
    B = pkg.capi.CsrMatrix.from_device(r1 - r0, s.cols, *keep)
    B.attention_plan_wide(H)
    up4 = lambda w: (w + 3) // 4 * 4       # noqa: E731  (rows padded so that every head starts on a 16-byte boundary)
    O, stats = _nan(gpu, H, r1 - r0, up4(kv))[:, :, :kv], _nan(gpu, H, r1 - r0, 2)
    delta, dQ, dB = _nan(gpu, H, r1 - r0), _nan(gpu, H, r1 - r0, up4(k))[:, :, :k], _nan(gpu, H, hi - lo)
    # (the block's rows as heads of their own: 16-byte aligned, a head stride that is a multiple of 4)
    Qb, dOb = (_pad(d[n][:, r0:r1], (w + 3) // 4 * 4)[:, :, :w] for n, w in (("Q", k), ("dO", kv)))
    B.attention_forward_wide(Qb, d["K"], d["V"], O, stats, bias[:, lo:hi], scale)
    B.attention_backward_q_wide(Qb, d["K"], d["V"], O, dOb, stats, delta, dQ, bias[:, lo:hi], dB, scale)
    torch.cuda.synchronize()
    for w, g, b in (("O", O, base["O"][:, r0:r1]), ("stats", stats, base["stats"][:, r0:r1]), ("delta", delta, base["delta"][:, r0:r1]),
                    ("dQ", dQ, base["dQ"][:, r0:r1]), ("dBias", dB, base["dBias"][:, lo:hi])):
        assert _same(g, b), f"k={k} kv={kv}: {w} of the row block differs from the whole matrix's rows"
    B.close()


# ---- 6. the device's own expf ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P1", "P2"])
@pytest.mark.parametrize("k,kv", [(128, 128), (97, 66)], ids=["k128-kv128", "k97-kv66"])
def test_wide_passes_on_general_scores_against_the_per_nonzero_reference(shared, gpu, k, kv, name):
    """The rule and the constants of tests/test_gpu_attention_multigraph.py: the error over the magnitude of the chain is at
    most max(4 x the same reference in fp32, RTOL); D = max t - min t <= 32 is checked on the host."""
    h = shared[name]
    s = h.s
    scale = 0.125
    Qn, dOn = OC.randn([sum(map(ord, name)), k, kv, 1], (s.rows, k), (s.rows, kv))
    Kn, Vn = OC.randn([sum(map(ord, name)), k, kv, 2], (s.cols, k), (s.cols, kv))
    refs = _references(s, Qn, Kn, Vn, dOn, scale)
    got = run(h, *(_dev(gpu, x)[None] for x in (Qn, Kn, Vn, dOn)), scale)
    _errors(f"wide {name} k={k} kv={kv}", {w: got[w][0].cpu().numpy() for w in ("O", "dQ", "dK", "dV")}, *refs)
    lengths = np.diff(s.rp)
    assert not got["O"][0].cpu().numpy()[lengths == 0].any() and not got["dQ"][0].cpu().numpy()[lengths == 0].any()


# ---- 7. the holder ---------------------------------------------------------------------------------------------------------------------------------
def _step(att, Q, K, V, dO, bias=None):
    import torch
    q, k, v = (t.detach().requires_grad_(True) for t in (Q, K, V))
    b = bias.detach().requires_grad_(True) if bias is not None else None
    O = att(q, k, v, b) if bias is not None else att(q, k, v)
    O.backward(dO)
    torch.cuda.synchronize()
    out = dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)
    if bias is not None:
        out["dBias"] = b.grad
    return out


def _dense(mask, scale, Q, K, V, dO, dtype, g, dense_bias=None):
    """test_gpu_attention_gqa._dense_gqa with an optional dense bias (heads, rows, cols): torch's dense autograd in `dtype`."""
    import torch
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (Q, K, V))
    ke, ve = k.repeat_interleave(g, dim=0), v.repeat_interleave(g, dim=0)
    full = mask.any(1)
    scores = (q @ ke.transpose(1, 2)) * scale
    if dense_bias is not None:
        scores = scores + dense_bias.to(dtype)
    scores = torch.where(mask, scores, torch.tensor(float("-inf"), dtype=dtype, device=mask.device))
    P = torch.zeros_like(scores)
    P[:, full] = torch.softmax(scores[:, full], dim=2)
    O = P @ ve
    O.backward(dO.to(dtype))
    return dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad), P.detach()


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_wide_holder_modes_agree_equal_the_direct_calls_and_match_dense_autograd(pkg, gpu, dt, with_bias):
    """FusedSparseAttention(wide=True) at k = kv = 128, H = 4 on 4 and on 2 K/V heads: "batched" and "loop" give the same bits,
    O is the direct _wide call's, and against torch's fp64 dense autograd the normalised error is at most max(4 x torch's dense
    autograd in the same dtype, RTOL) (the rule and the magnitudes of tests/test_gpu_attention16.py)."""
    import torch
    dtype = torch.float32 if dt == "fp32" else torch.bfloat16
    s = gqa_pattern()
    h = Handles(pkg, s, gpu)
    SA = pkg.sparse_attention
    scale, k, kv = 0.125, 128, 128
    loop, batched = (SA.FusedSparseAttention(s.rows, s.cols, h.keep[0], h.keep[1], scale=scale, heads=m, bias=with_bias, wide=True)
                     for m in ("loop", "batched"))
    ri, ci = torch.from_numpy(s.row_of).to(gpu), torch.from_numpy(s.ci.astype(np.int64)).to(gpu)
    mask = torch.zeros((s.rows, s.cols), dtype=torch.bool, device=gpu)
    mask[ri, ci] = True
    for hkv in (H, HKV):
        g = H // hkv
        gen = torch.Generator(device=gpu).manual_seed(2300 + hkv)
        Q, K, V, dO = (torch.randn((n_heads, n, w), generator=gen, device=gpu).to(dtype) for n_heads, n, w in
                       ((H, s.rows, k), (hkv, s.cols, k), (hkv, s.cols, kv), (H, s.rows, kv)))
        bias = torch.randn((H, s.nnz), generator=gen, device=gpu) if with_bias else None
        got_l, got_b = _step(loop, Q, K, V, dO, bias), _step(batched, Q, K, V, dO, bias)
        for name in got_b:
            assert got_b[name].shape == got_l[name].shape and _same(got_b[name], got_l[name]), f"H_kv={hkv} {name}: batched differs from the loop"
        assert got_b["O"].dtype == dtype and got_b["dK"].shape == (hkv, s.cols, k) and got_b["dV"].shape == (hkv, s.cols, kv)
        direct = run(h, Q, K, V, dO, scale, bias)
        assert _same(got_b["O"], direct["O"]), f"H_kv={hkv}: O differs from the direct _wide call's"
        dense_bias = None
        if with_bias:
            dense_bias = torch.zeros((H, s.rows, s.cols), dtype=torch.float64, device=gpu)
            dense_bias[:, ri, ci] = bias.double()
        r64, P = _dense(mask, scale, Q, K, V, dO, torch.float64, g, dense_bias)
        rdt, _ = _dense(mask, scale, Q, K, V, dO, dtype, g, dense_bias)
        mags = _magnitudes(mask, scale, Q, K, V, dO, P, g)
        for what in ("O", "dQ", "dK", "dV"):
            gg, g64, gdt, mag = got_b[what], r64[what], rdt[what], mags[what]
            live = mag > 0
            assert bool(live.any()) and bool((gg[~live] == 0).all()), f"{what}: a value where nothing contributes"
            ours = float(((gg.double() - g64).abs()[live] / mag[live]).max())
            yard = float(((gdt.double() - g64).abs()[live] / mag[live]).max())
            print(f"wide holder {dt} bias={with_bias} H_kv={hkv} {what}: normalised error fused {ours:.3g}, torch {dt} dense autograd {yard:.3g}")
            assert ours <= max(4.0 * yard, RTOL), f"{what}: {ours:.3g} against {yard:.3g} of torch's {dt} dense autograd"
    narrow = SA.FusedSparseAttention(s.rows, s.cols, h.keep[0], h.keep[1], scale=scale)
    with pytest.raises(ValueError, match="65 columns"):
        narrow(torch.zeros((s.rows, 65), device=gpu), torch.zeros((s.cols, 65), device=gpu), torch.zeros((s.cols, 65), device=gpu))
    for att in (loop, batched, narrow):
        att.close()
    h.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_refusals_launch_nothing(shared, pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h = shared["P2"]
    rows, cols, nnz, ld = h.A.rows, h.A.cols, h.A.nnz, 132
    ones = lambda heads, n: torch.ones((heads, n, ld), dtype=torch.float32, device=gpu)       # noqa: E731
    Q, K, V, dO, O_in = ones(H, rows), ones(H, cols), ones(H, cols), ones(H, rows), ones(H, rows)
    stats_in, delta_in = torch.zeros((H, rows, 2), device=gpu), torch.zeros((H, rows), device=gpu)
    bias = torch.zeros((H, nnz), device=gpu)
    outs = {n: torch.full((H, r, w), float("nan"), dtype=torch.float32, device=gpu) for n, r, w in
            (("O", rows, ld), ("dQ", rows, ld), ("dK", cols, ld), ("dV", cols, ld), ("stats", rows, 2), ("delta", rows, 1), ("dBias", nnz, 1))}
    st = capi._stream_handle()
    good = dict(heads=4, q=rows * ld, k=cols * ld, v=cols * ld, o=rows * ld, d_o=rows * ld, stats=2 * rows, delta=rows,
                dq=rows * ld, dk=cols * ld, dv=cols * ld)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731

    def call(which, A=None, T=None, k=128, kv=128, ldq=ld, ldo=ld, b=bias, db=None, heads=4):
        A, T = A or h.A, T or h.T
        hs = capi.AttnHeads(**dict(good, heads=heads))
        if which == "forward":
            return lib.spmv_csr_attention_forward_wide(A._h, C.byref(hs), 2, 0, p(b), nnz, 0.25, k, p(Q), ldq, p(K), ld, kv, p(V), ld,
                                                       p(outs["O"]), ldo, p(outs["stats"]), st)
        if which == "backward_q":
            return lib.spmv_csr_attention_backward_q_wide(A._h, C.byref(hs), 2, 0, p(b), nnz, p(db), nnz, 0.25, k, p(Q), ldq, p(K), ld, kv,
                                                          p(V), ld, p(O_in), ld, p(dO), ld, p(stats_in), p(outs["delta"]), p(outs["dQ"]), ldo, st)
        return lib.spmv_csr_attention_backward_kv_wide(T._h, C.byref(hs), 2, 0, p(b), nnz, 0.25, k, p(Q), ldq, p(K), ld, kv, p(V), ld,
                                                       p(dO), ld, p(stats_in), p(delta_in), p(outs["dK"]), ldo, p(outs["dV"]), ld, st)

    # handles without a wide plan, and with one for fewer heads
    bare = Handles(pkg, h.s, gpu, heads=H, wide=False)
    few = Handles(pkg, h.s, gpu, heads=H, wide=False)
    few.A.attention_plan_wide(2)
    few.T.attention_plan_wide(2)
    for which in ("forward", "backward_q", "backward_kv"):
        name = f"spmv_csr_attention_{which}_wide"
        cases = [(dict(k=0), "need 1 <= k <= 128"), (dict(k=129), "need 1 <= k <= 128"), (dict(kv=0), "1 <= kv <= 128"),
                 (dict(kv=129), "1 <= kv <= 128"), (dict(ldq=127), "below its width"), (dict(ldo=127), "below its width")]
        if which == "backward_q":
            cases.append((dict(b=None, db=outs["dBias"]), "dBias without a bias"))
        for change, word in cases:
            assert call(which, **change) == capi.ERR_INVALID, f"{which} {change}"
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, msg
        for k in (128, 8):          # one rule at every width
            assert call(which, A=bare.A, T=bare.T, k=k, kv=k) == capi.ERR_NOT_PLANNED
            assert name in lib.spmv_last_error().decode() and "plan_wide" in lib.spmv_last_error().decode()
            assert call(which, A=few.A, T=few.T, k=k, kv=k) == capi.ERR_NOT_PLANNED
            assert "the wide plan covers 2" in lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs.values()), "a refused call wrote to an output"
    for which in ("forward", "backward_q", "backward_kv"):                 # and the same calls, unchanged, are accepted
        assert call(which) == capi.OK, lib.spmv_last_error()
        assert call(which, b=None) == capi.OK, lib.spmv_last_error()
        assert call(which, A=few.A, T=few.T, heads=2) == capi.OK, lib.spmv_last_error()
    assert call("backward_q", db=outs["dBias"]) == capi.OK, lib.spmv_last_error()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t[:, :, :128] if n in ("O", "dQ", "dK", "dV") else t).any()) for n, t in outs.items() if n not in ("dK", "dV"))
    assert not bool(torch.isnan(outs["dK"][:2, :, :128]).any()) and bool(torch.isnan(outs["dK"][:, :, 128:]).all())
    # the existing calls keep their limit
    with pytest.raises(capi.SpmvError, match="need 1 <= k <= 64"):
        h.A.attention_forward_gqa(Q[:, :, :65], K[:2, :, :65], V[:2, :, :65], outs["O"][:, :, :65], outs["stats"], 0.25)
    bare.close()
    few.close()


# ---- 9. limits -------------------------------------------------------------------------------------------------------------------------------------
def test_wide_limits_and_plan_bytes(shared, pkg, gpu):
    """max_heads_wide: the launch limit (rows x lanes per row x heads < 2^32 on the row blocks and on the blocks of the pieces,
    heads <= 65535) with 32 lanes per row above width 64: half of max_heads at 64 (16 lanes) up to the cap."""
    import torch

    def limit(m, tp, lanes):
        lengths = np.diff(tp)
        per = 256 // lanes
        pieces = int(np.sum(-(-lengths[lengths > 512] // 512)))
        blocks = max(-(-m.rows // per), -(-pieces // per))
        return min(65535, ((1 << 32) - 1) // (blocks * 256))

    for name in ("P1", "P2"):
        h = shared[name]
        for m, tp in ((h.A, h.s.rp), (h.T, h.tp)):
            narrow, wide = m.attention_max_heads(64, 64), m.attention_max_heads_wide(128, 128)
            assert narrow == limit(m, tp, 16) and wide == limit(m, tp, 32)
            assert m.attention_max_heads_wide(65, 4) == wide and m.attention_max_heads_wide(4, 65) == wide
            for k, kv in OC.GEOMETRIES:
                assert m.attention_max_heads_wide(k, kv) == m.attention_max_heads(k, kv)
    # a handle large enough for the limit to bite: 2^20 rows of one entry
    n = 1 << 20
    rp = torch.arange(n + 1, dtype=torch.int32, device=gpu)
    ci = torch.zeros(n, dtype=torch.int32, device=gpu)
    big = pkg.capi.CsrMatrix.from_device(n, 8, rp, ci, torch.zeros(n, dtype=torch.float32, device=gpu))
    big.attention_plan()
    narrow, wide = big.attention_max_heads(64, 64), big.attention_max_heads_wide(128, 128)
    assert narrow == ((1 << 32) - 1) // (n * 16) == 255 and wide == ((1 << 32) - 1) // (n * 32) == 127 == narrow // 2
    before = big.attention_plan_bytes()
    big.attention_plan_wide(3)
    assert big.attention_plan_bytes() == before, "no long row: the wide plan allocates nothing"
    big.close()
    # plan_bytes: exactly heads x pieces x 260 floats more, once, and only after plan_wide
    s = OC.p1()
    h = Handles(pkg, s, gpu, heads=3, wide=False)
    lengths = np.diff(h.tp)
    pieces = int(np.sum(-(-lengths[lengths > 512] // 512)))
    assert pieces > 0
    before = h.T.attention_plan_bytes()
    h.T.attention_plan_wide(3)
    assert h.T.attention_plan_bytes() - before == 3 * pieces * 260 * 4
    h.T.attention_plan_wide(2)          # (idempotent; it only grows)
    h.T.attention_plan_wide(3)
    assert h.T.attention_plan_bytes() - before == 3 * pieces * 260 * 4
    h.T.attention_plan_wide(5)
    assert h.T.attention_plan_bytes() - before == 5 * pieces * (260 + 132) * 4 - 3 * pieces * 132 * 4
    h.close()


# ---- 10. graph capture ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_calls_are_graph_capturable(shared, gpu):
    import torch
    h, k, kv, scale, dtype = shared["P1"], 128, 128, 0.1, torch.bfloat16
    A, T = h.A, h.T
    d0 = _data16(gpu, h, k, kv, dtype, 2401)
    bias = _dev(gpu, OC.randn([2402], (H, h.s.nnz))[0])
    bt = h.bias_t(bias)
    run(h, d0["Q"], d0["K"], d0["V"], d0["dO"], scale, bias)          # (the warm run)
    Q, dO, K, V = (d0[n].clone() for n in ("Q", "dO", "K", "V"))
    outs = dict(O=_nan(gpu, H, A.rows, kv, dtype=dtype), stats=_nan(gpu, H, A.rows, 2), delta=_nan(gpu, H, A.rows),
                dQ=_nan(gpu, H, A.rows, k, dtype=dtype), dBias=_nan(gpu, H, A.nnz), dK=_nan(gpu, HKV, A.cols, k, dtype=dtype),
                dV=_nan(gpu, HKV, A.cols, kv, dtype=dtype))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream; the calls take the current stream)
        A.attention_forward_wide(Q, K, V, outs["O"], outs["stats"], bias, scale)
        A.attention_backward_q_wide(Q, K, V, outs["O"], dO, outs["stats"], outs["delta"], outs["dQ"], bias, outs["dBias"], scale)
        T.attention_backward_kv_wide(Q, K, V, dO, outs["stats"], outs["delta"], outs["dK"], outs["dV"], bt, scale)
    for seed in (2403, 2404):
        d = _data16(gpu, h, k, kv, dtype, seed)
        Q.copy_(d["Q"]), dO.copy_(d["dO"]), K.copy_(d["K"]), V.copy_(d["V"])
        for o in outs.values():
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(h, d["Q"], d["K"], d["V"], d["dO"], scale, bias)
        for name in outs:
            assert _same(outs[name], eager[name]), f"replay with seed {seed}: {name} differs from the eager call"
