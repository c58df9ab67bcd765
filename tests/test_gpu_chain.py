"""GPU (-m gpu): the handles that spmv_csr_select_*, spmv_csr_spgemm and spmv_csr_add build go through every consumer, and the
builders go through each other (tests/_chain.py: the carriers and the programs; tests/test_chain_host.py proves them on the host).

Every expectation is numpy's (_add.add, _spgemm.spgemm, _select.host_select_*, test_transpose_host.host_transpose, _exact.Exact),
never a kernel of this library, and every comparison is bit for bit (+0 / -0 folded where test_gpu_exact.py folds them; a NaN
of a chain matches any NaN) except softmax and attention, which keep the bounds of their own files.

  every path    for each builder (threshold, top-k, product, sum, sum-grown) and structure of _chain.CASES: the carrier's operands
                uploaded, the derived handle built, the operands destroyed, then every entry of test_gpu_exact.PATHS on a fresh
                derived handle (test_gpu_transpose._run_paths_on_handle: two runs, guard bands, misaligned y, plan_describe) with
                the integer and the subnormal problem of Exact; only xskip may be missing, and never for "duplicate" on a
                duplicate-free result
  SpMM          spmm_plan + spmm at k = 1, 4, 17, spmm_plan_cols + spmm_cols at k = 65, 130: every column exact
  SDDMM         sddmm at k = 3, 16, 64 into a separate plain buffer: every nonzero exact
  16-bit        run_vals16 (SPMV_TILED, SPMV_ADAPTIVE; bf16, fp16) with the handle's own integer values narrowed on the host
  softmax       row_softmax, its backward and the fused attention passes on the pattern of program "pattern_algebra": the
                references and bounds of test_gpu_softmax.py and of test_gpu_fused_attention.py's general case, unchanged
  steps         every program: after each step download() is the host composition, validate passes, dims agree, the byte
                queries are 0 for the companions the handle does not carry
  ownership     each program with every handle closed as soon as its last child exists, with all kept open, and on a side
                stream beside a busy default stream: the same bytes
  refresh       K = select_topk(spgemm(add(A, transpose(A)), B), k) with every map and plan kept; the leaves rewritten in place;
                the four _values calls in order; stale SPMV_PANEL plans; SPMV_TILED and spmm follow; the same inside a graph
  memory        four rounds of program "aat_topk" leave free device memory where the first left it
  aliasing      the four _values calls refuse their own target as an operand and leave its values as they were
"""
import types

import numpy as np
import pytest

import _chain as H
import _exact as E
import _round16 as R16
import _select
import _softmax as SM
import _spgemm
import test_gpu_fused_attention as FA
import test_gpu_softmax as SX
from test_gpu_exact import KNOBS, PATHS, _Dev, _describe_mismatch, _has_duplicates, _mismatches  # noqa: F401  (the runner's parts)
from test_gpu_transpose import _run_paths_on_handle

pytestmark = pytest.mark.gpu
MIB = 1 << 20
f32 = np.float32


# ---- the builders on the device ----------------------------------------------------------------------------------------------------
def _tensors(gpu, mat):
    import torch
    rows, cols, (rp, ci, va) = mat
    return rows, cols, tuple(torch.from_numpy(np.ascontiguousarray(a, dt)).to(gpu) for a, dt in ((rp, np.int32), (ci, np.int32), (va, f32)))


def _borrow(capi, t):
    return capi.CsrMatrix.from_device(t[0], t[1], *t[2])


def _device_step(gpu, builder, hs, keep=False, stream=None, **kw):
    import torch
    score = kw.get("score")
    if score is not None:
        score = torch.from_numpy(np.ascontiguousarray(score, f32)).to(gpu)
    if builder == "transpose":
        return hs[0].transpose(keep_map=keep, stream=stream)
    if builder == "select_topk":
        return hs[0].select_topk(kw["k"], score, abs=kw.get("abs", False), keep_map=keep, stream=stream)
    if builder == "select_threshold":
        return hs[0].select_threshold(kw["threshold"], score, abs=kw.get("abs", False), keep_map=keep, stream=stream)
    if builder == "spgemm":
        return hs[0].spgemm(hs[1], keep_plan=keep, stream=stream)
    if builder == "add":
        return hs[0].add(hs[1], kw.get("alpha", 1.0), kw.get("beta", 1.0), kw.get("op", "union"), keep_plan=keep, stream=stream)
    raise KeyError(builder)


def _run_device(capi, gpu, leaves, steps, close_early, stream=None, visit=None):
    """The steps on the device: {name: download()} of every step.  close_early: every handle (leaves too) is destroyed as soon as
    the last step that names it has its result, before that result is downloaded; else all stay open to the end.
    visit(name, builder, handle) sees every result while it is open."""
    last_use = {}
    for i, (_, _, operands, _) in enumerate(steps):
        for o in operands:
            last_use[o] = i
    live = {n: _borrow(capi, _tensors(gpu, m)) for n, m in leaves.items()}
    got = {}
    try:
        for i, (name, builder, operands, kw) in enumerate(steps):
            live[name] = _device_step(gpu, builder, [live[o] for o in operands], stream=stream, **kw)
            if close_early:
                for o in set(operands):
                    if last_use[o] == i:
                        live.pop(o).close()
            got[name] = live[name].download()
            if visit:
                visit(name, builder, live[name])
    finally:
        for h in live.values():
            h.close()
    return got


def _derived(capi, gpu, carrier, tensors):
    """The carrier's builder on borrowed operands, which are destroyed before the child is returned."""
    parents = {n: _borrow(capi, t) for n, t in tensors.items()}
    (_, builder, operands, kw), = carrier.steps
    try:
        return _device_step(gpu, builder, [parents[o] for o in operands], **kw)
    finally:
        for p in parents.values():
            p.close()


def _payload(gpu, carrier, vals):
    return {n: _tensors(gpu, m) for n, m in carrier.leaves(vals).items()}


def _bits_differ(got, want):
    """Strictly bit for bit (no NaN is expected on a carried handle)."""
    return [n for n, g, w in zip(("row_ptr", "col_idx", "vals"), got, want)
            if not np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))]


# ---- 1. every path on a carried handle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", H.CASES)
def test_every_path_multiplies_by_a_derived_handle_exactly(pkg, oracle, gpu, monkeypatch, kind, name):
    """(What these cases found: SPMV_PANEL's sorted blocks refused [product-wide_window] and [sum-wide_window] -- merging the
    repeated columns of wide_window's first and last rows shifts the layout's units of 256 column-sorted nonzeros, and one then
    spans 529 945 columns against the 2^19 a column offset holds.  Such a block is now laid out as all tail)"""
    capi = pkg.capi
    c = H.carrier(kind, name, pkg, oracle)
    _, problems = H.exact_problems(c, f"{name}/{kind}")
    loaded = []
    for label, vals, x, want in problems:
        payload = _payload(gpu, c, vals)
        child = _derived(capi, gpu, c, payload)                  # what every path gets: the target's pattern, these values
        try:
            capi.check(capi.lib().spmv_csr_validate(child._h, 0))
            bad = _bits_differ(child.download(), (c.out.rp, c.out.ci, c.out_vals(vals)))
            assert not bad, f"{kind}/{name}/{label}: {bad} of the derived handle differ from the numpy model"
        finally:
            child.close()
        loaded.append((label, payload, x, want))
    failures, ran = _run_paths_on_handle(pkg, monkeypatch, gpu, c.out, loaded, lambda payload: _derived(capi, gpu, c, payload))
    assert not failures, f"{kind}/{name}: {len(failures)} failing path(s):\n" + "\n".join(failures)
    assert {p[0] for p in PATHS} - ran <= {"xskip"}, "a path was left out"
    if kind not in ("threshold", "topk"):
        assert not _has_duplicates(c.out), "a sum or a product has duplicate-free rows: xskip has no such excuse"


# ---- 2. the other consumers ------------------------------------------------------------------------------------------------------
def _carried(pkg, oracle, gpu, kind, name, tag, scaled=True):
    """(carrier, Exact on its base, the derived handle with the integer values on it; its operands are destroyed)."""
    c = H.carrier(kind, name, pkg, oracle)
    ex = E.Exact(c.base, f"{name}/{kind}/{tag}", scaled=scaled)
    return c, ex, _derived(pkg.capi, gpu, c, _payload(gpu, c, ex.vals()))


@pytest.mark.parametrize("name", H.SPMM_ON)
@pytest.mark.parametrize("kind", H.KINDS)
def test_spmm_on_a_derived_handle(pkg, oracle, gpu, kind, name):
    import torch
    c, ex, h = _carried(pkg, oracle, gpu, kind, name, "spmm")
    try:
        for k in H.SPMM_K + H.SPMM_COLS_K:
            wide = k in H.SPMM_COLS_K
            h.spmm_plan_cols(k) if wide else h.spmm_plan()
            M, want = H.spmm_problem(ex, k, 5)
            dX = torch.from_numpy(M.astype(f32)).to(gpu)
            dY = torch.full((c.out.rows, k), float("nan"), dtype=torch.float32, device=gpu)
            (h.spmm_cols if wide else h.spmm)(dX, dY)
            torch.cuda.synchronize()
            got = dY.cpu().numpy()
            bad = [f"column {col}: {_mismatches(got[:, col], want[:, col])}" for col in range(k) if _mismatches(got[:, col], want[:, col])]
            assert not bad, f"{kind}/{name} k={k}: " + "; ".join(bad[:3])
    finally:
        h.close()


@pytest.mark.parametrize("name", H.SDDMM_ON)
@pytest.mark.parametrize("kind", H.KINDS)
def test_sddmm_on_a_derived_handle(pkg, oracle, gpu, kind, name):
    import torch
    c, _, h = _carried(pkg, oracle, gpu, kind, name, "sddmm")
    try:
        h.spmm_plan()
        before = h.download()[2].copy()
        for k in H.SDDMM_K:
            U, X, want = H.sddmm_problem(c.out, k, 7)
            out = torch.full((c.out.nnz,), float("nan"), dtype=torch.float32, device=gpu)      # a plain buffer of its own
            h.sddmm(torch.from_numpy(U.astype(f32)).to(gpu), torch.from_numpy(X.astype(f32)).to(gpu), out)
            torch.cuda.synchronize()
            assert _mismatches(out.cpu().numpy(), want) == "", f"{kind}/{name} k={k}: {_mismatches(out.cpu().numpy(), want)}"
        assert np.array_equal(h.download()[2].view(np.uint32), before.view(np.uint32)), "sddmm touched the handle's values"
    finally:
        h.close()


@pytest.mark.parametrize("name", H.VALS16_ON)
@pytest.mark.parametrize("kind", H.KINDS)
def test_16bit_values_on_a_derived_handle(pkg, oracle, gpu, kind, name):
    """The handle's own values (integers in [-4, 4], no row scale: fp16 holds them) narrowed on the host; the handle's fp32
    values are then overwritten through nothing: run_vals16 reads the 16-bit array, and the sums are exact."""
    import torch
    capi = pkg.capi
    c, ex, h = _carried(pkg, oracle, gpu, kind, name, "vals16", scaled=False)
    try:
        own = h.download()[2]
        assert np.array_equal(own.view(np.uint32), c.out_vals(ex.vals()).view(np.uint32))
        d_x = torch.from_numpy(ex.x()).to(gpu)
        want = ex.expected()
        for fmt, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            bits = R16.convert(fmt, own)
            assert np.array_equal(R16.widen(fmt, bits).view(np.uint32), own.view(np.uint32)), "the narrowing must be exact"
            v16 = torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(gpu).view(dtype)
            for v, params in ((capi.TILED, None), (capi.ADAPTIVE, [capi.ADAPTIVE, 256, 0, 0, 0, 0, 0, 0])):
                h.plan(v) if params is None else h.plan_set(v, params)
                ys = []
                for fill in (float("nan"), -1.2345e30):
                    d_y = torch.full((c.out.rows,), fill, dtype=torch.float32, device=gpu)
                    h.run_vals16(v, v16, d_x, d_y)
                    torch.cuda.synchronize()
                    ys.append(d_y.cpu().numpy())
                assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32)), f"{kind}/{name} {fmt} variant {v}: rows unwritten"
                assert _mismatches(ys[0], want) == "", f"{kind}/{name} {fmt} variant {v}: {_mismatches(ys[0], want)}"
    finally:
        h.close()


class _SoftmaxOn(SX._Dev):
    """test_gpu_softmax._Dev around a handle that already exists."""

    def __init__(self, gpu, handle):
        self.gpu, self.rows, self.nnz, self.A = gpu, handle.rows, handle.nnz, handle
        handle.spmm_plan()


@pytest.fixture
def algebra_result(pkg, gpu):
    """The last handle of program "pattern_algebra" (topk_pattern -> union -> mask -> difference), its parents destroyed, and
    its structure by the host composition."""
    p = H.programs()["pattern_algebra"]
    live = {n: _borrow(pkg.capi, _tensors(gpu, m)) for n, m in p.leaves.items()}
    for name, builder, operands, kw in p.steps:
        live[name] = _device_step(gpu, builder, [live[o] for o in operands], **kw)
    D = live.pop("D")
    for h in live.values():
        h.close()
    m, n, (rp, ci, va) = p.host["D"]
    assert H.same(D.download(), (rp, ci, va)) is None
    yield D, E.Structure(m, n, rp, ci)
    D.close()


def test_softmax_on_a_derived_pattern(pkg, gpu, algebra_result):
    """test_gpu_softmax.py's parity with the fp64 recipe (forward) and with fp64 (backward), and the exact integer backward."""
    D, s = algebra_result
    dev = _SoftmaxOn(gpu, D)
    L = SX._lengths(s)[s.row_of]
    for i, scale in enumerate(SM.SCALES):
        scores = SM.clipped_scores(np.random.Generator(np.random.PCG64([7, 21 + i])), s.nnz, scale)
        ref, Dm, Lr = SM.recipe(s.rp, scores, scale)
        assert Dm.max() <= 32.0 and ref.min() >= 1e-17
        out, bad = dev.forward(SX._to(gpu, scores), scale)
        assert not bad, (scale, bad)
        ratio = np.abs(out.cpu().numpy().astype(np.float64) - ref) / SM.parity_bound(ref, Dm, Lr)
        print(f"forward scale={scale}: largest error / bound = {ratio.max():.3g}")
        assert ratio.max() <= 1.0, f"scale={scale}: {int((ratio > 1).sum())} entries outside the bound, worst {ratio.max():.3g}"
    P, dP = SX._int_pair("pattern_algebra", s.nnz)
    res = SX._int_backward(s, P, dP)
    for i, scale in enumerate(SX.BWD_SCALES):
        dS, bad = dev.backward(SX._to(gpu, P), SX._to(gpu, dP), scale)
        assert not bad, (scale, bad)
        assert SX._mismatches(dS, SX._to(gpu, scale * res.astype(np.float64)), fold_zeros=True) == 0, f"integer backward, scale={scale}"
        rng = np.random.Generator(np.random.PCG64([7, 41 + i]))
        Pf, dPf = rng.standard_normal(s.nnz).astype(f32), rng.standard_normal(s.nnz).astype(f32)
        ref, mag = SM.backward_recipe(s.rp, Pf, dPf, scale)
        dS, bad = dev.backward(SX._to(gpu, Pf), SX._to(gpu, dPf), scale)
        assert not bad, (scale, bad)
        ratio = np.abs(dS.cpu().numpy().astype(np.float64) - ref) / SM.backward_bound(mag, L)
        print(f"backward scale={scale}: largest error / bound = {ratio.max():.3g}")
        assert ratio.max() <= 1.0, f"backward scale={scale}: worst {ratio.max():.3g}"


@pytest.mark.parametrize("k,kv", [(24, 24), (6, 10)])
def test_fused_attention_on_a_derived_pattern(pkg, gpu, algebra_result, k, kv):
    """The general case of test_gpu_fused_attention.py: forward and both backward passes against the fp64 dense autograd with
    torch's fp32 dense autograd as the yardstick; backward_kv runs on the transpose of the derived handle."""
    import torch
    D, s = algebra_result
    h = types.SimpleNamespace(A=D, T=D.transpose())
    try:
        h.A.attention_plan()
        h.T.attention_plan()
        Q, K, V, dO = FA._randn(gpu, 900 + 64 * k + kv, (s.rows, k), (s.cols, k), (s.cols, kv), (s.rows, kv))
        got = FA._run(h, Q, K, V, dO, FA.SCALE)
        FA._check_general(f"pattern_algebra k={k} kv={kv}", got, FA._mask(s, gpu), float(f32(FA.SCALE)), Q, K, V, dO)
        Lz = torch.from_numpy(np.diff(s.rp)).to(gpu) == 0
        assert bool((got["O"][Lz] == 0).all()) and bool((got["dQ"][Lz] == 0).all())
    finally:
        h.T.close()


# ---- 3. chains -------------------------------------------------------------------------------------------------------------------
def _raw(got):
    return [np.ascontiguousarray(a).view(np.uint32) for a in got]


@pytest.mark.parametrize("name", H.PROGRAMS)
def test_every_step_of_a_program_is_the_host_composition(pkg, gpu, name):
    import torch
    capi = pkg.capi
    p = H.programs()[name]
    host = p.host

    def visit(step, builder, h):
        m, n, (rp, ci, va) = host[step]
        assert (h.rows, h.cols, h.nnz) == (m, n, len(ci)), f"{name}/{step}: dims {(h.rows, h.cols, h.nnz)}"
        capi.check(capi.lib().spmv_csr_validate(h._h, 0))
        assert (h.transpose_map_bytes(), h.select_map_bytes(), h.spgemm_plan_bytes(), h.add_plan_bytes()) == (0, 0, 0, 0), \
            f"{name}/{step}: a companion nobody asked for"

    kept = _run_device(capi, gpu, p.leaves, p.steps, close_early=False, visit=visit)
    for step, _, _, _ in p.steps:
        bad = H.same(kept[step], host[step][2])
        assert bad is None, f"{name}/{step}: {bad}"
    for a, b in p.equal_patterns:
        assert H.same_pattern(kept[a], kept[b]), f"{name}: the patterns of {a} and {b} differ on the device"
    # every handle closed as soon as its last child exists: the same bytes
    early = _run_device(capi, gpu, p.leaves, p.steps, close_early=True)
    # on a side stream, while the default stream multiplies by a leaf
    leaf = next(iter(p.leaves.values()))
    busy = _borrow(capi, _tensors(gpu, leaf))
    bx = torch.ones(max(leaf[1], 1), dtype=torch.float32, device=gpu)
    by = torch.empty(max(leaf[0], 1), dtype=torch.float32, device=gpu)
    busy.plan(capi.SCALAR)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(20):
        busy.run(capi.SCALAR, bx, by)
    with torch.cuda.stream(side):                                   # (the uploads of the leaves go on the side stream too)
        aside = _run_device(capi, gpu, p.leaves, p.steps, close_early=False, stream=side)
    for _ in range(20):
        busy.run(capi.SCALAR, bx, by)
    torch.cuda.synchronize()
    busy.close()
    for step, _, _, _ in p.steps:
        for how, other in (("closed early", early), ("on a side stream", aside)):
            assert all(np.array_equal(g, w) for g, w in zip(_raw(other[step]), _raw(kept[step]))), f"{name}/{step}: other bytes {how}"


def _int_leaf(mat, seed):
    """mat's pattern with integer values in [-4, 4] without 0."""
    rng = np.random.default_rng(seed)
    n = len(mat[2][1])
    return (rng.integers(1, 5, n) * rng.choice([-1, 1], n)).astype(f32)


def _refresh_host(a, b, va, vb, k, first=None):
    """The refresh chain on the host for the leaves' values va, vb: T, S, P, K.  first: (row_ptr, col_idx, map) of the first
    call's selection, which a refresh keeps (None: rank now and return it)."""
    A, B = (a[0], a[1], (a[2][0], a[2][1], va)), (b[0], b[1], (b[2][0], b[2][1], vb))
    env = H.run_host({"A": A, "B": B}, [("T", "transpose", ("A",), {}), ("S", "add", ("A", "T"), dict(alpha=1.0, beta=1.0, op="union")),
                                        ("P", "spgemm", ("S", "B"), {})])
    m, n, (rp, ci, pv) = env["P"]
    if first is None:
        k_rp, k_ci, _, kmap = _select.host_select_topk(m, rp, ci, pv, k, None, True)
        first = (k_rp, k_ci, kmap.astype(np.int64))
    env["K"] = (m, n, (first[0], first[1], pv[first[2]]))
    return env, first


def _int_y(mat, m_int):
    """int64 y = mat m for integer values, with the exactness condition of _exact asserted."""
    rows, cols, (rp, ci, va) = mat
    k = va.astype(np.float64)
    assert np.array_equal(k, np.rint(k)), "the chain's values are integers"
    p = k.astype(np.int64)[:, None] * m_int[ci]
    row = np.repeat(np.arange(rows), np.diff(rp))
    mag = np.zeros((rows, p.shape[1]), np.int64)
    np.add.at(mag, row, np.abs(p))
    assert mag.max(initial=0) <= E.EXACT_LIMIT, "the refresh chain's sums are not exact in fp32"
    y = np.zeros((rows, p.shape[1]), np.int64)
    np.add.at(y, row, p)
    return y.astype(f32)


def test_refresh_chain(pkg, gpu):
    import torch
    capi = pkg.capi
    a, b = H.leaf(3201, 257, 257, 12, special=0.0), H.leaf(3202, 257, 193, 12, special=0.0)
    k, kx = 7, 4
    ta, tb = _tensors(gpu, a), _tensors(gpu, b)
    A, B = _borrow(capi, ta), _borrow(capi, tb)
    T = A.transpose(keep_map=True)
    S = A.add(T, 1.0, 1.0, "union", keep_plan=True)
    P = S.spgemm(B, keep_plan=True)
    K = P.select_topk(k, abs=True, keep_map=True)
    chain = (("T", T), ("S", S), ("P", P), ("K", K))
    try:
        env, kmap = _refresh_host(a, b, a[2][2], b[2][2], k)
        for name, h in chain:
            assert H.same(h.download(), env[name][2]) is None, f"{name} as built: {H.same(h.download(), env[name][2])}"
        companions = lambda h: (h.transpose_map_bytes(), h.add_plan_bytes(), h.spgemm_plan_bytes(), h.select_map_bytes())   # noqa: E731
        for i, (name, h) in enumerate(chain):                       # each carries its own companion and no other
            assert [bool(n) for n in companions(h)] == [j == i for j in range(4)], f"{name}: companions {companions(h)}"
        panel = [capi.PANEL, 0, 0, 0, 0, 0, 1, 0]
        for _, h in chain:
            h.plan_set(capi.PANEL, panel)
            h.plan(capi.TILED)
            h.spmm_plan()
        dY = torch.full((K.rows, kx), float("nan"), dtype=torch.float32, device=gpu)       # the graph's output
        rng = np.random.default_rng(3203)
        m_int = {193: rng.integers(-4, 5, (193, kx)), 257: rng.integers(-4, 5, (257, kx))}
        d_x = {n: torch.from_numpy(m[:, 0].astype(f32)).to(gpu) for n, m in m_int.items()}
        d_X = {n: torch.from_numpy(m.astype(f32)).to(gpu) for n, m in m_int.items()}

        def run(h, v):
            y = torch.full((h.rows,), float("nan"), dtype=torch.float32, device=gpu)
            h.run(v, d_x[h.cols], y)
            torch.cuda.synchronize()
            return y.cpu().numpy()

        def columns_bad(Y, mat):
            got, want = Y.cpu().numpy(), _int_y(mat, m_int[mat[1]])
            return [f"column {c}: {_mismatches(got[:, c], want[:, c])}" for c in range(kx) if _mismatches(got[:, c], want[:, c])]

        def spmm_bad(h, mat):
            Y = torch.full((h.rows, kx), float("nan"), dtype=torch.float32, device=gpu)
            h.spmm(d_X[h.cols], Y)
            torch.cuda.synchronize()
            return columns_bad(Y, mat)

        def rewrite(seed):
            va, vb = _int_leaf(a, seed), _int_leaf(b, seed + 1)
            ta[2][2].copy_(torch.from_numpy(va).to(gpu))                # in place: the handles borrow these tensors
            tb[2][2].copy_(torch.from_numpy(vb).to(gpu))
            return _refresh_host(a, b, va, vb, k, kmap)[0]

        env = rewrite(10)
        refresh = {"T": lambda: T.transpose_values(A), "S": lambda: S.add_values(A, T, 1.0, 1.0),
                   "P": lambda: P.spgemm_values(S, B), "K": lambda: K.select_values(P)}
        for name, h in chain:
            refresh[name]()
            assert H.same(h.download(), env[name][2]) is None, f"{name} refreshed: {H.same(h.download(), env[name][2])}"
            want = _int_y(env[name], m_int[h.cols])[:, 0]
            with pytest.raises(capi.SpmvError) as e:
                run(h, capi.PANEL)
            assert e.value.status == capi.ERR_STALE_PLAN and "values_changed" in str(e.value), f"{name}: {e.value}"
            h.plan(capi.PANEL)
            assert _mismatches(run(h, capi.PANEL), want) == "", f"{name}: SPMV_PANEL after plan"
            assert _mismatches(run(h, capi.TILED), want) == "", f"{name}: the SPMV_TILED plan made before the refresh"
            assert not spmm_bad(h, env[name]), f"{name}: spmm on the plan made before the refresh: {spmm_bad(h, env[name])}"
        # the four refreshes and one spmm in one graph, replayed after two more rewrites
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for name, _ in chain:
                refresh[name]()
            K.spmm(d_X[K.cols], dY)
        for seed in (20, 30):
            env = rewrite(seed)
            dY.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert not columns_bad(dY, env["K"]), f"replay after rewrite {seed}: {columns_bad(dY, env['K'])}"
            for name, h in chain:
                assert H.same(h.download(), env[name][2]) is None, f"{name} after replay {seed}: {H.same(h.download(), env[name][2])}"
        del g
    finally:
        for h in (K, P, S, T, A, B):
            h.close()


def test_memory_comes_back(pkg, gpu):
    import torch
    capi = pkg.capi
    p = H.programs()["aat_topk"]
    free = []
    for _ in range(4):
        _run_device(capi, gpu, p.leaves, p.steps, close_early=False)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"


# ---- 4. a handle as its own operand ---------------------------------------------------------------------------------------------------
def _diag(n, seed):
    rng = np.random.default_rng(seed)
    return n, n, (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), _spgemm.spread(rng, n))


@pytest.mark.parametrize("call", ["transpose_values", "select_values", "add_values", "spgemm_values"])
def test_a_refresh_refuses_its_own_target_as_an_operand(pkg, gpu, call):
    """In each construction the sizes the handle recorded agree with its own, so only the pointer rule can refuse the call: the
    transpose of a square matrix; a selection that dropped nothing; a sum whose b lies inside a; a product with a diagonal a."""
    capi = pkg.capi
    sq = H.leaf(3301, 257, 257, 20)
    if call == "transpose_values":
        parents = [_borrow(capi, _tensors(gpu, sq))]
        t = parents[0].transpose(keep_map=True)
        attempt = lambda: t.transpose_values(t)                        # noqa: E731
    elif call == "select_values":
        parents = [_borrow(capi, _tensors(gpu, sq))]
        t = parents[0].select_topk(10 ** 6, keep_map=True)
        assert t.nnz == parents[0].nnz
        attempt = lambda: t.select_values(t)                           # noqa: E731
    elif call == "add_values":
        m, n, (rp, ci, va) = H.host_step("add", [sq, sq], op="union")            # sorted, duplicate-free: c has a's nnz
        a = (m, n, (rp, ci, va))
        inside = H.host_step("select_topk", [a], k=3)
        parents = [_borrow(capi, _tensors(gpu, a)), _borrow(capi, _tensors(gpu, inside))]
        t = parents[0].add(parents[1], 1.0, 1.0, "union", keep_plan=True)
        assert t.nnz == parents[0].nnz
        attempt = lambda: t.add_values(t, parents[1])                  # noqa: E731
    else:
        parents = [_borrow(capi, _tensors(gpu, _diag(257, 3302))), _borrow(capi, _tensors(gpu, H.host_step("add", [sq, sq], op="union")))]
        t = parents[0].spgemm(parents[1], keep_plan=True)
        assert t.nnz == parents[1].nnz
        attempt = lambda: t.spgemm_values(parents[0], t)               # noqa: E731
    try:
        before = t.download()
        with pytest.raises(capi.SpmvError) as e:
            attempt()
        assert e.value.status == capi.ERR_INVALID and f"spmv_csr_{call}" in str(e.value) and "read while they are written" in str(e.value)
        assert not _bits_differ(t.download(), before), "a refused call changed the target"
    finally:
        t.close()
        for p in parents:
            p.close()


def test_the_same_handle_as_both_operands_stays_allowed(pkg, gpu):
    """a == b in add_values and spgemm_values, where the recorded sizes agree: C = A + A and C = A A refresh as before."""
    capi = pkg.capi
    sq = H.leaf(3303, 257, 257, 20, special=0.0)
    A = _borrow(capi, _tensors(gpu, sq))
    try:
        for build, refresh, step in ((lambda: A.add(A, H.THIRD, 3.0, "union", keep_plan=True), lambda c: c.add_values(A, A, H.THIRD, 3.0),
                                      ("add", dict(alpha=H.THIRD, beta=3.0, op="union"))),
                                     (lambda: A.spgemm(A, keep_plan=True), lambda c: c.spgemm_values(A, A), ("spgemm", {}))):
            c = build()
            try:
                refresh(c)
                want = H.host_step(step[0], [sq, sq], **step[1])
                assert H.same(c.download(), want[2]) is None, f"{step[0]}: {H.same(c.download(), want[2])}"
            finally:
                c.close()
    finally:
        A.close()
