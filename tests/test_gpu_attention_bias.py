"""Fused attention with an additive fp32 bias per nonzero and its gradient, on the device (include/spmv_hip.h "Fused attention
with an additive bias"; spmv_csr_attention_{forward,backward_q,backward_kv}_bias and spmv_csr_transpose_gather).

identity    a bias of -0.0 gives, bit for bit, the _gqa call's (fp32) or the _16 call's O, stats, delta, dQ, dK and dV: P1 and
            P2 of tests/_order_cases.py, all its GEOMETRIES and (8, 8) and (24, 32) (V = 1, 2, 4, 8 and 16), fp32, bf16 and fp16,
            four query heads on two K/V heads.
rounding    on general data stats[:, 0] is, bit for bit, the row maximum of fl(fl(scale * sddmm) + bias).
order       no tolerance: on the data of _attention_bias.ORDER_SETS (every expf argument +-0, <= -128 or -Inf: the host test
            asserts it) with a bias from {-0.0, +0.0, -128, -256, -Inf} that differs per query head, O, stats, dQ, delta,
            dBias, dK and dV equal the emulation of _attention_bias.py on every element; bias_t is made by
            spmv_csr_transpose_gather.  tests/test_attention_bias_host.py shows that each mistake the bias invites changes bits
            of these arrays on these inputs.
live expf   general bias ~ N(0, 1), D = max t - min t <= 32 asserted: the normalised error against the per-nonzero fp64 reference
            with bias is at most max(4 x the fp32 per-nonzero reference's, RTOL), the rule of
            tests/test_gpu_attention_multigraph.py; dBias included; both figures printed.
masks, a null dBias, a shared bias (stride 0), the gather, the refusals, graph capture and the holder: see each test.

Every device array of a direct call -- inputs, outputs, bias, bias_t and dBias -- lies in a buffer of its own between guard
bands; outputs start as NaN.
"""
import ctypes as C

import numpy as np
import pytest

import _attention_bias as AB
import _attention_order as AO
import _order_cases as OC
from _util import RTOL

pytestmark = pytest.mark.gpu

H, G = AB.HEADS, AB.GROUP
HKV = H // G
GUARD_N = 1024
GUARD = {"fp32": 3.0e35, "bf16": 24576.0, "fp16": 24576.0}      # finite and representable in the dtype
NAMES = ("O", "stats", "delta", "dQ", "dK", "dV")
f32, f64 = np.float32, np.float64


def _torch_dtype(dt):
    import torch
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dt]


class Arena:
    """Device arrays between guard bands: put(a) copies a numpy or torch array in, out(shape) makes a NaN-filled output."""

    def __init__(self, gpu):
        self.gpu, self.made = gpu, []

    def _new(self, shape, dt):
        import torch
        n = int(np.prod(shape))
        buf = torch.full((2 * GUARD_N + n,), GUARD[dt], dtype=_torch_dtype(dt), device=self.gpu)
        self.made.append((buf, n, dt))
        return buf[GUARD_N:GUARD_N + n].view(*shape)

    def put(self, a, dt="fp32"):
        import torch
        a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        v = self._new(tuple(a.shape), dt)
        v.copy_(a.to(self.gpu))
        return v

    def out(self, shape, dt="fp32"):
        v = self._new(shape, dt)
        v.fill_(float("nan"))
        return v

    def check(self):
        import torch
        torch.cuda.synchronize()
        for buf, n, dt in self.made:
            assert bool((buf[:GUARD_N] == GUARD[dt]).all()) and bool((buf[GUARD_N + n:] == GUARD[dt]).all()), "a kernel wrote outside an array"


class Handles:
    def __init__(self, pkg, s, gpu, heads=H):
        import torch
        self.s, self.gpu, self.pkg = s, gpu, pkg
        self.keep = (torch.from_numpy(np.ascontiguousarray(s.rp)).to(gpu), torch.from_numpy(np.ascontiguousarray(s.ci)).to(gpu),
                     torch.zeros(s.nnz, dtype=torch.float32, device=gpu))
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=True)
        self.A.attention_plan_heads(heads)
        self.T.attention_plan_heads(heads)
        self.tp, self.ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)

    def close(self):
        self.T.close()
        self.A.close()


@pytest.fixture(scope="module")
def handles(pkg, gpu):
    made = {name: Handles(pkg, OC.pattern(name), gpu) for name in ("P1", "P2")}
    yield made
    for h in made.values():
        h.close()


def _bits(t):
    import torch
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def run(h, d, scale, bias=None, dt="fp32", want_dbias=True, kv_pass=True, made=None):
    """The three passes on d = dict(Q (H, rows, k), K, V (HKV, cols, .), dO and optionally caller-made O, stats, delta), every
    array between guards.  bias None: the unbiased _gqa / _16 calls; else (nnz,) or (H, nnz) numpy or torch, bias_t made by
    transpose_gather.  Returns the outputs (and bias_t); `made`: an Arena to add to."""
    ar = made or Arena(h.gpu)
    s = h.s
    Q, K, V, dO = (ar.put(d[n], dt) for n in ("Q", "K", "V", "dO"))
    k, kv = Q.shape[-1], V.shape[-1]
    got = {}
    if bias is not None:
        b = ar.put(bias)
    if "stats" in d:
        O, stats = ar.put(d["O"], dt), ar.put(d["stats"])
    else:
        O, stats = ar.out((H, s.rows, kv), dt), ar.out((H, s.rows, 2))
        if bias is None:
            h.A.attention_forward_gqa(Q, K, V, O, stats, scale)
        else:
            h.A.attention_forward_bias(Q, K, V, b, O, stats, scale)
        got["O"], got["stats"] = O, stats
    got["delta"], got["dQ"] = ar.out((H, s.rows)), ar.out((H, s.rows, k), dt)
    if bias is None:
        h.A.attention_backward_q_gqa(Q, K, V, O, dO, stats, got["delta"], got["dQ"], scale)
    else:
        if want_dbias:
            got["dBias"] = ar.out((H, s.nnz))
        h.A.attention_backward_q_bias(Q, K, V, b, O, dO, stats, got["delta"], got["dQ"], got.get("dBias"), scale)
    if kv_pass:
        got["dK"], got["dV"] = ar.out((HKV, s.cols, k), dt), ar.out((HKV, s.cols, kv), dt)
        delta_in = ar.put(d["delta"]) if "stats" in d else got["delta"]
        if bias is None:
            h.T.attention_backward_kv_gqa(Q, K, V, dO, stats, delta_in, got["dK"], got["dV"], scale)
        else:
            got["bias_t"] = ar.out(tuple(b.shape))
            h.T.transpose_gather(b, got["bias_t"])
            h.T.attention_backward_kv_bias(Q, K, V, got["bias_t"], dO, stats, delta_in, got["dK"], got["dV"], scale)
    if made is None:
        ar.check()
    return got


def general(h, k, kv, seed, dt="fp32"):
    """Standard normal Q, dO (H heads), K, V (HKV heads) as torch tensors of dtype dt (rounded once from fp32)."""
    import torch
    s = h.s
    Q, dO, K, V = OC.randn(seed, (H, s.rows, k), (H, s.rows, kv), (HKV, s.cols, k), (HKV, s.cols, kv))
    return {n: torch.from_numpy(a).to(_torch_dtype(dt)) for n, a in (("Q", Q), ("dO", dO), ("K", K), ("V", V))}


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("k,kv", AB.GEOMETRIES)
@pytest.mark.parametrize("name", ["P1", "P2"])
def test_a_bias_of_minus_zero_gives_the_unbiased_calls_bits(handles, name, k, kv, dt):
    h = handles[name]
    d = general(h, k, kv, [1, k, kv], dt)
    for scale in (0.3, -0.7):
        want = run(h, d, scale, None, dt)
        got = run(h, d, scale, np.full((H, h.s.nnz), -0.0, f32), dt)
        for w in NAMES:
            assert _same(got[w], want[w]), f"{name} k={k} kv={kv} {dt} scale={scale}: {w} differs from the unbiased call in a bit"
        assert not bool(got["dBias"].isnan().any())


# ---- 2. the rounding of t ------------------------------------------------------------------------------------------------------
def test_the_score_is_the_rounded_product_plus_the_bias(handles, gpu):
    import torch
    s, Q1, K1, b1, scale = AB.general_case()
    h = handles["P2"]
    k = Q1.shape[1]
    d = general(h, k, 8, [2, k])
    d["Q"][:], d["K"][:] = torch.from_numpy(Q1), torch.from_numpy(K1)       # every head the same Q and K; the bias differs per head
    bias = np.stack([np.roll(b1, 17 * y) for y in range(H)])
    got = run(h, d, scale, bias, kv_pass=False)
    ar = Arena(gpu)
    sd = ar.out((s.nnz,))
    h.A.sddmm(ar.put(Q1), ar.put(K1), sd)
    ar.check()
    sd = sd.cpu().numpy()
    lengths = np.diff(s.rp)
    full = np.flatnonzero(lengths > 0)
    assert np.any(lengths == 1), "one-entry rows pin single nonzeros"
    for y in range(H):
        t = ((f32(scale) * sd).astype(f32) + bias[y]).astype(f32)
        want = np.maximum.reduceat(t, s.rp[full].astype(np.int64))
        M = got["stats"][y, :, 0].cpu().numpy()[full]
        assert np.array_equal(M.view(np.uint32), want.view(np.uint32)), f"head {y}: a row maximum is not fl(fl(scale * s) + bias)"
        fused = AO.fma(f32(scale), sd, bias[y])
        assert not np.array_equal(np.maximum.reduceat(fused, s.rp[full].astype(np.int64)).view(np.uint32), want.view(np.uint32))


# ---- 3. the order, no tolerance ------------------------------------------------------------------------------------------------
def _folded(a):
    return (np.ascontiguousarray(a, f32) + f32(0)).view(np.uint32)


def _same_bits(tag, got, want):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, tag
    g, w = _folded(got), _folded(want)
    bad = np.flatnonzero((g != w).reshape(-1))
    if bad.size:
        n = int(bad[0])
        raise AssertionError(f"{tag}: {bad.size} of {g.size} values differ from the documented order in a bit; the first at flat index "
                             f"{n}: {got.reshape(-1)[n]!r} against {want.reshape(-1)[n]!r}")
    return int(g.size)


@pytest.mark.parametrize("name,case,k,kv", AB.ORDER_SETS, ids=[f"{n}-{c}-k{k}-kv{kv}" for n, c, k, kv in AB.ORDER_SETS])
def test_the_biased_passes_have_the_documented_order(handles, name, case, k, kv):
    import torch
    h = handles[name]
    s = h.s
    per, Ks, Vs, bias = AB.order_data(name, case, k, kv)
    kv_pass = case != "maxima"
    stack = lambda arrays: torch.from_numpy(np.stack(arrays))       # noqa: E731
    d = {n: stack([p[n] for p in per]) for n in ("Q", "dO") + (("O", "stats", "delta") if "stats" in per[0] else ())}
    d["K"], d["V"] = stack(Ks), stack(Vs)
    got = run(h, d, per[0]["scale"], bias, kv_pass=kv_pass)
    want = [AB.emulate(s, h.tp, h.ti, per[y], bias[y], kv_pass=kv_pass) for y in range(H)]
    n = 0
    for y in range(H):
        for w in ("O", "stats", "dQ", "delta", "dBias"):
            if w in want[y]:
                n += _same_bits(f"{name} {case} k={k} kv={kv} head {y}: {w}", got[w][y], want[y][w])
    if kv_pass:
        assert np.array_equal(got["bias_t"].cpu().numpy().view(np.uint32),
                              np.stack([AB.transposed_bias(s.ci, bias[y]) for y in range(H)]).view(np.uint32)), "bias_t"
        for c in range(HKV):
            for w in ("dK", "dV"):
                n += _same_bits(f"{name} {case} K/V head {c}: {w}", got[w][c], AO.gqa_fold([want[c * G + i][w] for i in range(G)]))
    print(f"biased passes {name} {case} k={k} kv={kv}: {n} values compared bit for bit")


# ---- 4. live expf ---------------------------------------------------------------------------------------------------------------
def _errors(tag, got, r64, r32, mag):
    for w in ("O", "dQ", "dK", "dV", "dBias"):
        live = mag[w] > 0
        ours = float(np.max(np.abs(got[w].astype(f64) - r64[w])[live] / mag[w][live]))
        yard = float(np.max(np.abs(r32[w].astype(f64) - r64[w])[live] / mag[w][live]))
        print(f"{tag} {w}: normalised error {ours:.3g}, the per-nonzero reference in fp32 {yard:.3g}")
        assert ours <= max(4.0 * yard, RTOL), f"{tag} {w}: {ours:.3g} against {yard:.3g} of the fp32 per-nonzero reference"


def _per_nonzero(s, d, bias, scale, heads=range(H)):
    """Per query head y: (got-shaped fp64 results, fp32 results, magnitudes); dK, dV summed over the heads of a group."""
    out = []
    for y in heads:
        a = [d[n][y if n in ("Q", "dO") else y // G].numpy() for n in ("Q", "K", "V", "dO")]
        r64, mag, t = AB.multiset_attention(s.rp, s.ci, *a, bias[y], scale)
        finite = np.where(np.isfinite(t), t, np.nan)
        spread = [np.nanmax(finite[s.rp[i]:s.rp[i + 1]]) - np.nanmin(finite[s.rp[i]:s.rp[i + 1]]) for i in range(s.rows) if s.rp[i + 1] > s.rp[i]]
        assert max(spread) <= 32.0, "D = max t - min t <= 32"
        r32, _, _ = AB.multiset_attention(s.rp, s.ci, *a, bias[y], scale, dtype=f32)
        out.append((r64, r32, mag))
    return out


def _check_against_per_nonzero(tag, s, got, refs):
    for y, (r64, r32, mag) in enumerate(refs):
        one = {w: got[w][y].cpu().numpy() for w in ("O", "dQ", "dBias")}
        _errors(f"{tag} head {y}", dict(one, dK=r64["dK"].astype(f32), dV=r64["dV"].astype(f32)), r64, r32, mag)
    for c in range(HKV):
        grp = refs[c * G:c * G + G]
        sum_of = lambda i, w: sum(r[i][w] for r in grp)       # noqa: E731
        for w in ("dK", "dV"):
            mag = sum_of(2, w)
            live = mag > 0
            ours = float(np.max(np.abs(got[w][c].cpu().numpy().astype(f64) - sum_of(0, w))[live] / mag[live]))
            yard = float(np.max(np.abs(sum_of(1, w).astype(f64) - sum_of(0, w))[live] / mag[live]))
            print(f"{tag} K/V head {c} {w}: normalised error {ours:.3g}, the per-nonzero reference in fp32 {yard:.3g}")
            assert ours <= max(4.0 * yard, RTOL), f"{tag} {w}: {ours:.3g} against {yard:.3g}"


@pytest.mark.parametrize("name,k,kv,scale", [("P1", 16, 12, 0.3), ("P1", 6, 10, -0.7), ("P2", 8, 40, 0.3), ("P2", 64, 20, 0.25),
                                                 ("P2", 8, 8, 0.3), ("P1", 24, 32, -0.7)])
def test_general_bias_against_the_per_nonzero_reference(handles, name, k, kv, scale):
    h = handles[name]
    s = h.s
    d = general(h, k, kv, [4, k, kv])
    bias = OC.randn([44, k, kv], (H, s.nnz))[0]
    got = run(h, d, scale, bias)
    _check_against_per_nonzero(f"{name} k={k} kv={kv}", s, got, _per_nonzero(s, d, bias, scale))


# ---- 5. masks -------------------------------------------------------------------------------------------------------------------
def test_a_minus_inf_bias_removes_nonzeros_and_a_fully_masked_row_is_nan(pkg, gpu, handles):
    import torch
    import _exact as E
    h = handles["P2"]
    s, k, kv, scale = h.s, 16, 12, 0.3
    d = general(h, k, kv, [5, k, kv])
    rng = np.random.Generator(np.random.PCG64(55))
    gone = rng.random(s.nnz) < 1 / 3
    for i in range(s.rows):                         # never a whole row
        b, e = int(s.rp[i]), int(s.rp[i + 1])
        if e > b and gone[b:e].all():
            gone[b] = False
    bias = np.where(gone, -np.inf, OC.randn(56, (H, s.nnz))[0]).astype(f32)
    got = run(h, d, scale, bias)
    db = got["dBias"].cpu().numpy()
    assert np.all(db[:, gone] == 0), "dBias of a removed nonzero is +-0"
    # the same call on the pattern with those nonzeros removed, each against the per-nonzero reference of the reduced pattern
    keep = ~gone
    rp2 = np.concatenate([[0], np.cumsum(np.add.reduceat(keep, s.rp[:-1][np.diff(s.rp) > 0].astype(np.int64)))])
    lengths2 = np.zeros(s.rows, np.int64)
    lengths2[np.diff(s.rp) > 0] = np.diff(rp2)
    s2 = E.Structure(s.rows, s.cols, np.concatenate([[0], np.cumsum(lengths2)]), s.ci[keep])
    h2 = Handles(pkg, s2, gpu)
    bias2 = np.ascontiguousarray(bias[:, keep])
    got2 = run(h2, d, scale, bias2)
    refs = _per_nonzero(s2, d, bias2, scale)
    _check_against_per_nonzero("reduced pattern", s2, got2, refs)
    _check_against_per_nonzero("masked pattern", s2, dict(got, dBias=got["dBias"][:, torch.from_numpy(keep).to(gpu)]), refs)
    h2.close()
    # a fully masked row gives a NaN row, an empty row zeros
    i_full, i_empty = int(np.flatnonzero(np.diff(s.rp) > 3)[0]), int(np.flatnonzero(np.diff(s.rp) == 0)[0])
    bias3 = bias.copy()
    bias3[:, s.rp[i_full]:s.rp[i_full + 1]] = -np.inf
    got3 = run(h, d, scale, bias3, kv_pass=False)
    assert bool(got3["O"][:, i_full].isnan().all()) and bool((got3["O"][:, i_empty] == 0).all())
    others = [i for i in range(s.rows) if i != i_full]
    assert not bool(got3["O"][:, others].isnan().any())


# ---- 6. d_dbias = NULL, 7. a shared bias ------------------------------------------------------------------------------------------
def test_a_null_dbias_and_a_shared_bias(handles):
    import torch
    h = handles["P1"]
    s, k, kv, scale = h.s, 6, 10, 0.3
    d = general(h, k, kv, [6, k, kv])
    bias = OC.randn(66, (H, s.nnz))[0]
    full = run(h, d, scale, bias)
    none = run(h, d, scale, bias, want_dbias=False)          # (run checks the guard bands)
    assert "dBias" not in none
    for w in NAMES:
        assert _same(full[w], none[w]), f"{w} changes when dBias is not asked for"
    shared = run(h, d, scale, bias[0])                       # (nnz,): stride 0
    repeated = run(h, d, scale, np.repeat(bias[:1], H, axis=0))
    for w in NAMES + ("dBias",):
        assert _same(shared[w], repeated[w]), f"{w}: a shared bias differs from the bias repeated per head"
    assert shared["bias_t"].shape == (s.nnz,) and torch.equal(shared["bias_t"], repeated["bias_t"][0])


# ---- 8. transpose_gather ----------------------------------------------------------------------------------------------------------
def test_transpose_gather_copies_bits_and_refuses_a_handle_without_a_map(pkg, gpu, handles):
    import torch
    capi = pkg.capi
    h = handles["P2"]
    s, count = h.s, 3
    rng = np.random.Generator(np.random.PCG64(8))
    words = rng.integers(0, 2 ** 32, size=(count, s.nnz), dtype=np.uint64).astype(np.uint32)
    words[:, :4] = np.array([0x7FC12345, 0xFFA00001, 0x80000000, 0x7F800001], np.uint32)      # NaN payloads, -0.0, a signalling NaN
    ss, ds = s.nnz + 5, s.nnz + 3                                 # unequal strides, multiples of nothing
    ar = Arena(gpu)
    src = ar.out((count * ss,))
    dst = ar.out((count * ds,))
    src_v = torch.as_strided(src, (count, s.nnz), (ss, 1))
    src_v.copy_(torch.from_numpy(words.view(np.float32)).to(gpu))
    dst_v = torch.as_strided(dst, (count, s.nnz), (ds, 1))
    h.T.transpose_gather(src_v, dst_v)
    ar.check()
    order = np.argsort(s.ci.astype(np.int64), kind="stable")
    assert np.array_equal(dst_v.cpu().numpy().view(np.uint32), words[:, order])
    assert bool(torch.as_strided(dst, (count - 1, ds - s.nnz), (ds, 1), dst.storage_offset() + s.nnz).isnan().all()), "the gaps between the arrays are untouched"
    plain = h.A.transpose(keep_map=False)
    with pytest.raises(capi.SpmvError, match="spmv_csr_transpose_gather: the handle has no map"):
        plain.transpose_gather(src_v[0], dst_v[0])
    lib, st = capi.lib(), capi._stream_handle()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    for args in ((0, p(src), ss, p(dst), ds), (count, None, ss, p(dst), ds), (count, p(src), -1, p(dst), ds),
                 (count, p(src), ss, p(dst), s.nnz - 1), (1, C.c_void_p(src.data_ptr() + 2), 0, p(dst), 0)):
        dst.fill_(float("nan"))
        assert lib.spmv_csr_transpose_gather(h.T._h, *args, st) == capi.ERR_INVALID, args
        assert lib.spmv_last_error().decode().startswith("spmv_csr_transpose_gather:")
        torch.cuda.synchronize()
        assert bool(dst.isnan().all())
    plain.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bias_refusals_launch_nothing(pkg, gpu, handles):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h = handles["P2"]
    rows, cols, nnz, k, kv, ld = h.A.rows, h.A.cols, h.A.nnz, 8, 8, 8
    ones = lambda heads, n: torch.ones((heads, n, ld), device=gpu)       # noqa: E731
    Q, K, V, dO, O_in = ones(H, rows), ones(HKV, cols), ones(HKV, cols), ones(H, rows), ones(H, rows)
    stats_in, delta_in = torch.zeros((H, rows, 2), device=gpu), torch.zeros((H, rows), device=gpu)
    bias = torch.zeros((H, nnz + 1), device=gpu)
    outs = {n: torch.full(shape, float("nan"), device=gpu) for n, shape in
            (("O", (H, rows, ld)), ("dQ", (H, rows, ld)), ("dK", (HKV, cols, ld)), ("dV", (HKV, cols, ld)), ("stats", (H, rows, 2)),
             ("delta", (H, rows)), ("dBias", (H, nnz + 1)))}
    st = capi._stream_handle()
    good = dict(heads=H, q=rows * ld, k=cols * ld, v=cols * ld, o=rows * ld, d_o=rows * ld, stats=2 * rows, delta=rows,
                dq=rows * ld, dk=cols * ld, dv=cols * ld)

    def call(which, group=G, dt=capi.ATTN_FP32, kk=k, b="ok", bs=nnz + 1, db="ok", dbs=nnz + 1, handle=None, **change):
        hs = capi.AttnHeads(**dict(good, **change))
        p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
        bp = {"ok": p(bias), "null": None, "odd": C.c_void_p(bias.data_ptr() + 2)}[b]
        dbp = {"ok": p(outs["dBias"]), "null": None, "odd": C.c_void_p(outs["dBias"].data_ptr() + 2)}[db]
        if which == "forward":
            return lib.spmv_csr_attention_forward_bias(handle or h.A._h, C.byref(hs), group, dt, bp, bs, 0.25, kk, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                       p(outs["O"]), ld, p(outs["stats"]), st)
        if which == "backward_q":
            return lib.spmv_csr_attention_backward_q_bias(handle or h.A._h, C.byref(hs), group, dt, bp, bs, dbp, dbs, 0.25, kk, p(Q), ld, p(K), ld,
                                                          kv, p(V), ld, p(O_in), ld, p(dO), ld, p(stats_in), p(outs["delta"]), p(outs["dQ"]), ld, st)
        return lib.spmv_csr_attention_backward_kv_bias(handle or h.T._h, C.byref(hs), group, dt, bp, bs, 0.25, kk, p(Q), ld, p(K), ld, kv, p(V), ld,
                                                       p(dO), ld, p(stats_in), p(delta_in), p(outs["dK"]), ld, p(outs["dV"]), ld, st)

    unplanned = h.A.transpose(keep_map=False)
    for which in ("forward", "backward_q", "backward_kv"):
        name = f"spmv_csr_attention_{which}_bias"
        cases = [(dict(dt=3), "dtype"), (dict(dt=-1), "dtype"), (dict(b="null"), "null bias"), (dict(b="odd"), "4-byte aligned"),
                 (dict(bs=-1), "negative"),
                 # inherited: k = 65, group = 3, reserved = 1
                 (dict(kk=65), "k = 65"), (dict(group=3), "group"), (dict(reserved=1), "reserved")]
        if which == "backward_q":
            cases += [(dict(db="odd"), "4-byte aligned"), (dict(dbs=-1), "negative"), (dict(dbs=nnz - 1), "below nnz")]
        for change, word in cases:
            assert call(which, **change) == capi.ERR_INVALID, f"{which} {change}"
            msg = lib.spmv_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, msg
        assert call(which, handle=unplanned._h) == capi.ERR_NOT_PLANNED
        assert name in lib.spmv_last_error().decode()
    # the _16 calls go on refusing dtype 0
    hs = capi.AttnHeads(**good)
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    assert lib.spmv_csr_attention_forward_16(h.A._h, C.byref(hs), G, 0, 0.25, k, p(Q), ld, p(K), ld, kv, p(V), ld, p(outs["O"]), ld,
                                             p(outs["stats"]), st) == capi.ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs.values()), "a refused call wrote to an output"
    unplanned.close()
    for which in ("forward", "backward_q", "backward_kv"):                 # and the same calls, unchanged, are accepted
        assert call(which) == capi.OK, lib.spmv_last_error()
    assert call("backward_q", db="null", dbs=0) == capi.OK and call("backward_q", dbs=nnz) == capi.OK
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t[..., :nnz] if n == "dBias" else t).any()) for n, t in outs.items())


# ---- 10. graph capture ----------------------------------------------------------------------------------------------------------------
def test_the_bias_calls_and_the_gather_are_graph_capturable(handles, gpu):
    import torch
    h = handles["P1"]
    s, k, kv, scale = h.s, 12, 16, 0.3
    d = {n: t.to(gpu) for n, t in general(h, k, kv, [10, 0]).items()}
    bias = torch.from_numpy(OC.randn(100, (H, s.nnz))[0]).to(gpu)
    run(h, {n: t.cpu() for n, t in d.items()}, scale, bias.cpu().numpy())          # (the warm run)
    nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)      # noqa: E731
    outs = dict(O=nan(H, s.rows, kv), stats=nan(H, s.rows, 2), delta=nan(H, s.rows), dQ=nan(H, s.rows, k), dBias=nan(H, s.nnz),
                bias_t=nan(H, s.nnz), dK=nan(HKV, s.cols, k), dV=nan(HKV, s.cols, kv))
    Q, K, V, dO = d["Q"], d["K"], d["V"], d["dO"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.A.attention_forward_bias(Q, K, V, bias, outs["O"], outs["stats"], scale)
        h.A.attention_backward_q_bias(Q, K, V, bias, outs["O"], dO, outs["stats"], outs["delta"], outs["dQ"], outs["dBias"], scale)
        h.T.transpose_gather(bias, outs["bias_t"])
        h.T.attention_backward_kv_bias(Q, K, V, outs["bias_t"], dO, outs["stats"], outs["delta"], outs["dK"], outs["dV"], scale)
    for seed in (101, 102):
        new = general(h, k, kv, [10, seed])
        for n, t in d.items():
            t.copy_(new[n])
        bias.copy_(torch.from_numpy(OC.randn(seed, (H, s.nnz))[0]))
        for o in outs.values():
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(h, {n: t.cpu() for n, t in d.items()}, scale, bias.cpu().numpy())
        for name in outs:
            assert _same(outs[name], eager[name]), f"replay with seed {seed}: {name} differs from the eager call"


# ---- 11. the holder -----------------------------------------------------------------------------------------------------------------
def _dense(mask, idx, scale, Q, K, V, dO, bias, dtype, g):
    """torch's dense autograd with an additive bias matrix, in `dtype`: (O, dQ, dK, dV, dBias per nonzero) and P."""
    import torch
    q, k, v, b = (t.detach().to(dtype).requires_grad_(True) for t in (Q, K, V, bias))
    heads = q.shape[0]
    B = torch.zeros((heads,) + tuple(mask.shape), dtype=dtype, device=q.device)
    B[:, idx[0], idx[1]] = b if b.dim() == 2 else b.expand(heads, -1)
    S = scale * q @ k.repeat_interleave(g, 0).transpose(1, 2) + B
    P = torch.softmax(S.masked_fill(~mask, float("-inf")), dim=-1)
    P = torch.where(mask.any(1)[None, :, None], P, torch.zeros_like(P))
    O = P @ v.repeat_interleave(g, 0)
    O.backward(dO.to(dtype))
    return dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad, dBias=b.grad), P.detach()


def _magnitudes(idx, scale, Q, K, V, dO, P, g, shared):
    """The sums of absolute values the errors are divided by (tests/test_gpu_fused_attention.py), in fp64; dBias: p (|dp| + sum p |dp|)"""
    import torch
    q, k, v, do = (t.double().abs() for t in (Q, K.repeat_interleave(g, 0), V.repeat_interleave(g, 0), dO))
    dp = do @ v.transpose(1, 2)
    gm = P * (dp + (P * dp).sum(-1, keepdim=True))
    fold = lambda x: x.view(x.shape[0] // g, g, *x.shape[1:]).sum(1)       # noqa: E731
    db = gm[:, idx[0], idx[1]]
    return dict(O=P @ v, dQ=abs(scale) * gm @ k, dK=fold(abs(scale) * gm.transpose(1, 2) @ q), dV=fold(P.transpose(1, 2) @ do),
                dBias=db.sum(0) if shared else db)


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_the_biased_holder_matches_dense_autograd_with_a_bias_matrix(pkg, gpu, dt):
    """FusedSparseAttention(bias=True) in both heads modes, with a (heads, nnz) and a shared (nnz,) bias, on a duplicate-free
    pattern, against torch's fp64 dense autograd with an additive bias matrix: the normalised error (magnitudes of
    tests/test_gpu_fused_attention.py) of O, dQ, dK, dV and dBias is at most max(4 x that of the same dense autograd run in the
    operands' dtype, RTOL), the holders' rule of tests/test_gpu_attention16.py (and, for fp32, of tests/test_gpu_fused_attention.py).
    "loop" and "batched" give the same bits.  (What a step allocates: the next test.)"""
    import torch
    import _exact as E
    dtype = _torch_dtype(dt)
    rng = np.random.Generator(np.random.PCG64(11))
    rows, cols = 150, 96
    lengths = rng.integers(0, 40, size=rows)
    lengths[:3] = (0, 1, cols)
    rp = np.concatenate([[0], np.cumsum(lengths)])
    ci = np.concatenate([rng.permutation(cols)[:n] for n in lengths])
    s = E.Structure(rows, cols, rp, ci)
    d_rp, d_ci = torch.from_numpy(s.rp.astype(np.int32)).to(gpu), torch.from_numpy(s.ci.astype(np.int32)).to(gpu)
    idx = (torch.from_numpy(s.row_of.astype(np.int64)).to(gpu), torch.from_numpy(s.ci.astype(np.int64)).to(gpu))
    mask = torch.zeros((rows, cols), dtype=torch.bool, device=gpu)
    mask[idx] = True
    scale, k, kv = 0.25, 24, 32
    SA = pkg.sparse_attention
    holders = {m: SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=scale, heads=m, bias=True) for m in ("loop", "batched")}
    with pytest.raises(ValueError):
        holders["loop"](torch.zeros((rows, k), device=gpu), torch.zeros((cols, k), device=gpu), torch.zeros((cols, kv), device=gpu))
    gen = torch.Generator(device=gpu).manual_seed(1100)
    for hkv, shared in ((H, False), (HKV, False), (HKV, True)):
        g = H // hkv
        Q, K, V, dO = (torch.randn((n_heads, n, w), generator=gen, device=gpu).to(dtype) for n_heads, n, w in
                       ((H, rows, k), (hkv, cols, k), (hkv, cols, kv), (H, rows, kv)))
        bias = torch.randn((s.nnz,) if shared else (H, s.nnz), generator=gen, device=gpu)
        got = {}
        for m, att in holders.items():
            q, kk, v, b = (t.detach().requires_grad_(True) for t in (Q, K, V, bias))
            O = att(q, kk, v, b)
            O.backward(dO)
            torch.cuda.synchronize()
            got[m] = dict(O=O.detach(), dQ=q.grad, dK=kk.grad, dV=v.grad, dBias=b.grad)
        for w in ("O", "dQ", "dK", "dV", "dBias"):
            assert got["loop"][w].shape == got["batched"][w].shape and _same(got["loop"][w], got["batched"][w]), f"{w}: loop and batched differ"
        assert got["loop"]["dBias"].shape == bias.shape and got["loop"]["dBias"].dtype == torch.float32
        assert got["loop"]["dK"].shape == K.shape and got["loop"]["O"].dtype == dtype
        r64, P = _dense(mask, idx, scale, Q, K, V, dO, bias, torch.float64, g)
        rdt, _ = _dense(mask, idx, scale, Q, K, V, dO, bias, dtype, g)
        mags = _magnitudes(idx, scale, Q, K, V, dO, P, g, shared)
        for w in ("O", "dQ", "dK", "dV", "dBias"):
            live = mags[w] > 0
            ours = float(((got["loop"][w].double() - r64[w]).abs()[live] / mags[w][live]).max())
            yard = float(((rdt[w].double() - r64[w]).abs()[live] / mags[w][live]).max())
            print(f"holder {dt} H_kv={hkv} shared={shared} {w}: normalised error {ours:.3g}, dense autograd in {dt} {yard:.3g}")
            assert ours <= max(4.0 * yard, RTOL), f"{dt} H_kv={hkv} shared={shared} {w}: {ours:.3g} against {yard:.3g}"
    # 2-D operands are one head
    Q, K, V, dO = (torch.randn((n, w), generator=gen, device=gpu).to(dtype) for n, w in ((rows, k), (cols, k), (cols, kv), (rows, kv)))
    bias = torch.randn((s.nnz,), generator=gen, device=gpu).requires_grad_(True)
    O = holders["loop"](Q, K, V, bias)
    O.backward(dO)
    r64, _ = _dense(mask, idx, scale, Q[None], K[None], V[None], dO[None], bias.detach(), torch.float64, 1)
    assert O.shape == (rows, kv) and bias.grad.shape == (s.nnz,)
    assert float((bias.grad.double() - r64["dBias"]).abs().max()) <= (1e-4 if dt == "fp32" else 0.1)
    for att in holders.values():
        att.close()



def test_a_biased_step_allocates_bias_t_and_dbias_and_nothing_else_of_nnz_size(pkg, gpu, monkeypatch):
    """On the pattern of tests/test_gpu_fused_attention.py's memory test (2000 x 2000, 128 keys per query, k = kv = 8: an array
    of nnz floats, 1 024 000 bytes, dwarfs everything else), two heads in one launch: the peak of one forward-plus-backward
    step of FusedSparseAttention(bias=True) exceeds the measured peak of the unbiased holder on the same operands by bias_t and
    dBias -- (heads, nnz) each, or (nnz,), (heads, nnz) and the (nnz,) sum for a shared bias -- and by less than half an array
    of nnz floats beyond that.  bias_t is made (one transpose_gather) only when dK or dV is asked for and dBias is allocated
    only when the bias requires grad: with neither, the step is the unbiased step's bytes.  A holder made with bias=False keeps
    no map and takes no bias."""
    import torch
    import _exact as E
    rows = cols = 2000
    heads, k = 2, 8
    rng = np.random.Generator(np.random.PCG64(53))
    ci = np.concatenate([np.sort(rng.choice(cols, size=128, replace=False)) for _ in range(rows)])
    s = E.Structure(rows, cols, np.arange(rows + 1) * 128, ci)
    one = 4 * s.nnz
    assert one == 1_024_000
    d_rp, d_ci = torch.from_numpy(s.rp.astype(np.int32)).to(gpu), torch.from_numpy(s.ci.astype(np.int32)).to(gpu)
    gen = torch.Generator(device=gpu).manual_seed(530)
    Q, K, V, dO = (torch.randn((heads, n, k), generator=gen, device=gpu) for n in (rows, cols, cols, rows))
    SA = pkg.sparse_attention
    plain = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25, heads="batched")
    biased = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25, heads="batched", bias=True)
    assert plain.T.transpose_map_bytes() == 0 and biased.T.transpose_map_bytes() == one
    with pytest.raises(ValueError):
        plain(Q, K, V, torch.zeros(s.nnz, device=gpu))
    gathers = []
    real = pkg.capi.CsrMatrix.transpose_gather
    monkeypatch.setattr(pkg.capi.CsrMatrix, "transpose_gather", lambda self, *a, **kw: (gathers.append(1), real(self, *a, **kw))[1])

    def step_bytes(att, bias=None, grads=(True, True, True), bias_grad=True):
        q, kk, v = (t.clone().requires_grad_(g) for t, g in zip((Q, K, V), grads))
        b = () if bias is None else (bias.clone().requires_grad_(bias_grad),)
        att(q, kk, v, *b).backward(dO)                    # warm-up (the plans grow here)
        q.grad = kk.grad = v.grad = None
        for t in b:
            t.grad = None
        del gathers[:]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        att(q, kk, v, *b).backward(dO)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    base = step_bytes(plain)
    base_q = step_bytes(plain, grads=(True, False, False))
    for shared in (False, True):
        bias = torch.randn((s.nnz,) if shared else (heads, s.nnz), generator=gen, device=gpu)
        got = step_bytes(biased, bias)
        assert len(gathers) == 1
        extra = one * ((1 + heads + 1) if shared else 2 * heads)           # bias_t, dBias (heads, nnz) and, shared, its sum
        print(f"one step, shared={shared}: biased {got} bytes, unbiased {base}, bias_t and dBias {extra}, one array of nnz floats {one}")
        assert got - base <= extra + one // 2, f"shared={shared}: {got - base} bytes beyond the unbiased step, bias_t and dBias are {extra}"
        assert got - base >= extra - one // 2, "bias_t and dBias were expected in the step's peak"
        only_q = step_bytes(biased, bias, grads=(True, False, False), bias_grad=False)
        assert not gathers, "bias_t is made only when dK or dV is asked for"
        print(f"one step, only dQ asked for, shared={shared}: biased {only_q} bytes, unbiased {base_q}")
        assert only_q - base_q < one // 2, "without dK, dV and dBias a biased step allocates nothing of nnz size"
        no_dbias = step_bytes(biased, bias, bias_grad=False)
        assert len(gathers) == 1
        assert no_dbias - base <= one * (1 if shared else heads) + one // 2, "dBias is allocated only when the bias requires grad"
    plain.close()
    biased.close()
