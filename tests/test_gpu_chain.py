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

The handles of spmv_csr_permute (both routes) and spmv_csr_ilu0 go the same ways: as the carrier kinds permuted, permuted-via-
transpose, factor-upper and factor-lower through every path and every other consumer; in the programs "permute_commutes" and
"permuted_product"; every empty handle permuted, and where it is square coloured, planned, solved and refused; and

  scattered     wide_window with its rows and columns relabelled at random by spmv_csr_permute: sorted rows of 16 columns drawn
                from all of 2^21 + 5, no band left, through every path
  colour        colour_of_a_product: color(A A^T + I), the multicolour ordering by permute, ILU(0) in at most `colors` levels and
                its solve, against _color.color, _color.permute, _ilu0.factor and _ilu0.apply, in the three ownership modes
  solved        every square step of "a_plus_at" and "self_operands" and a top-k selection of each: trsv_plan's rows against
                _trsv.levels / _trsv.order, the UNIT solve of both triangles, NON_UNIT on the sum with I
  one map       every _values / _gather / _scatter / _solve / _pivot companion of the six builders refuses every handle another
                builder made, and changes nothing
  refresh 2     M = ilu0(permute(add(A, I), perm, perm)): add_values, permute_values, ilu0_values after a rewrite; stale plans;
                no plan of the solve rebuilt; the same in a graph
"""
import types

import numpy as np
import pytest

import _chain as H
import _color
import _exact as E
import _ilu0
import _round16 as R16
import _select
import _softmax as SM
import _spgemm
import _trsv
import test_gpu_fused_attention as FA
import test_gpu_softmax as SX
from test_gpu_exact import KNOBS, PATHS, _Dev, _describe_mismatch, _has_duplicates, _mismatches  # noqa: F401  (the runner's parts)
from test_gpu_transpose import _run_paths_on_handle
from _util import assert_close_to_oracle

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
    if builder == "permute":
        perm = lambda p: None if p is None else torch.from_numpy(np.ascontiguousarray(p, np.int32)).to(gpu)     # noqa: E731
        return hs[0].permute(perm(kw.get("row_perm")), perm(kw.get("col_perm")), keep_map=keep,
                             via_transpose=kw.get("via_transpose", False), stream=stream)
    if builder == "ilu0":
        return hs[0].ilu0(stream=stream)
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
@pytest.mark.parametrize("kind,name", H.CASES + H.NEW_CASES)
def test_every_path_multiplies_by_a_derived_handle_exactly(pkg, oracle, gpu, monkeypatch, kind, name):
    """(What these cases found: SPMV_PANEL's sorted blocks refused [product-wide_window] and [sum-wide_window] -- merging the
    repeated columns of wide_window's first and last rows shifts the layout's units of 256 column-sorted nonzeros, and one then
    spans 529 945 columns against the 2^19 a column offset holds.  Such a block is now laid out as all tail)

    The permuted kinds put the target on a handle that spmv_csr_permute built (by either route) from a parent whose rows and
    columns are randomly relabelled, the factor kinds on a handle that spmv_csr_ilu0 built from a triangular matrix, whose ILU(0)
    is the matrix itself; the factor kinds have duplicate-free rows, so xskip has no "duplicate" excuse there."""
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
    if kind not in ("threshold", "topk") + H.PERMUTED_KINDS:
        assert not _has_duplicates(c.out), "a sum, a product or a factor has duplicate-free rows: xskip has no such excuse"


# ---- 2. the other consumers ------------------------------------------------------------------------------------------------------
def _carried(pkg, oracle, gpu, kind, name, tag, scaled=True):
    """(carrier, Exact on its base, the derived handle with the integer values on it; its operands are destroyed)."""
    c = H.carrier(kind, name, pkg, oracle)
    ex = H.exact_on(c, f"{name}/{kind}/{tag}", scaled=scaled)
    return c, ex, _derived(pkg.capi, gpu, c, _payload(gpu, c, ex.vals()))


@pytest.mark.parametrize("kind,name", H.consumer_cases(H.SPMM_ON))
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


@pytest.mark.parametrize("kind,name", H.consumer_cases(H.SDDMM_ON))
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


@pytest.mark.parametrize("kind,name", H.consumer_cases(H.VALS16_ON))
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


_FACTOR_OWN = ("ilu0", "trsv lower", "trsv upper")


def _companions(h, own=()):
    """The byte queries that are not 0, those of `own` left out."""
    q = {"transpose": h.transpose_map_bytes(), "select": h.select_map_bytes(), "spgemm": h.spgemm_plan_bytes(), "add": h.add_plan_bytes(),
         "permute": h.permute_map_bytes(), "ilu0": h.ilu0_plan_bytes()}
    if h.rows == h.cols:
        q.update({"trsv " + u: h.trsv_plan_bytes(u) for u in _trsv.UPLOS})
    return {k: v for k, v in q.items() if v and k not in own}


def _check_an_empty_square(capi, gpu, z):
    """An n x n handle without nonzeros: one colour, one level in both triangles, x = b under UNIT, the diagonal refusals."""
    import torch
    n = z.rows
    col, perm, cptr, info = z.color()
    want = _color.color(np.zeros(n + 1, np.int32), np.zeros(0, np.int32))
    assert np.array_equal(col.cpu().numpy(), want[0]) and np.array_equal(perm.cpu().numpy(), want[1]) and np.array_equal(cptr, want[2])
    assert all(info[k] == want[3][k] for k in ("colors", "rounds", "largest", "smallest")), (info, want[3])
    b = _trsv.rhs(n, np.random.default_rng(3150))
    d_b = torch.from_numpy(b).to(gpu)
    for uplo in _trsv.UPLOS:
        z.trsv_plan(uplo)
        lp, od = z.trsv_plan_rows(uplo)
        want_lp, want_od = _trsv.order(np.zeros(n, np.int64))
        assert np.array_equal(lp, want_lp) and np.array_equal(od, want_od), uplo
        x = z.trsv(d_b, torch.full((n,), float("nan"), device=gpu), uplo=uplo, unit=True)
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy().view(np.uint32), b.view(np.uint32)), f"{uplo}: x = b without terms"
        if n:
            with pytest.raises(capi.SpmvError) as e:
                z.trsv(d_b, uplo=uplo)
            assert e.value.status == capi.ERR_INVALID and "row 0 has no diagonal entry" in str(e.value), str(e.value)
    if n:
        with pytest.raises(capi.SpmvError) as e:
            z.ilu0()
        assert e.value.status == capi.ERR_INVALID and "spmv_csr_ilu0: row 0 stores no diagonal entry" in str(e.value), str(e.value)


def test_nothing_by_nothing(pkg, gpu):
    """0 x 0: coloured, planned, solved, permuted by either route, and ilu0 works (no row misses its diagonal)."""
    import torch
    capi = pkg.capi
    Z = _borrow(capi, _tensors(gpu, H._empty(0, 0)))
    try:
        _check_an_empty_square(capi, gpu, Z)
        for via in (False, True):
            P = Z.permute(via_transpose=via, keep_map=True)
            assert (P.rows, P.cols, P.nnz, P.permute_map_bytes()) == (0, 0, 0, 0)
            P.permute_values(Z)
            P.close()
        M = Z.ilu0()
        assert (M.rows, M.cols, M.nnz) == (0, 0, 0) and M.ilu0_pivot() == -1
        M.ilu0_values(Z)
        r = torch.zeros(0, device=gpu)
        assert M.ilu0_solve(r).numel() == 0
        M.close()
    finally:
        Z.close()


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
        assert not _companions(h, own=_FACTOR_OWN if builder == "ilu0" else ()), f"{name}/{step}: {_companions(h)}"
        if step in p.empty and m == n:
            _check_an_empty_square(capi, gpu, h)

    kept = _run_device(capi, gpu, p.leaves, p.steps, close_early=False, visit=visit)
    for step, _, _, _ in p.steps:
        bad = H.same(kept[step], host[step][2])
        assert bad is None, f"{name}/{step}: {bad}"
    for a, b in p.equal_patterns:
        assert H.same_pattern(kept[a], kept[b]), f"{name}: the patterns of {a} and {b} differ on the device"
    for a, b in p.equal_bytes:
        assert all(np.array_equal(g, w) for g, w in zip(_raw(kept[a]), _raw(kept[b]))), f"{name}: {a} and {b} differ on the device"
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


# ---- 3b. permute, colour, ilu0 and trsv as consumers of derived handles ----------------------------------------------------------------
def test_every_path_multiplies_by_a_randomly_relabelled_wide_matrix(pkg, oracle, gpu, monkeypatch):
    """wide_window's rows and columns relabelled at random by spmv_csr_permute: the band is gone, every sorted row of the child
    holds 16 columns drawn from all of 2^21 + 5, and no window of x serves a chunk.  (A block of 4096 such rows spreads its
    65 536 nonzeros evenly, so 256 neighbours in column order span about 2^13 columns, printed below: the 2^19 limit of DESIGN.md
    section 28 is met by a band with outliers, not by a uniform scatter.)  The child must be _color.permute's matrix, and every
    path exact."""
    capi = pkg.capi
    st = E.structure("wide_window", pkg, oracle)
    rng = np.random.default_rng(3160)
    p, q = rng.permutation(st.rows).astype(np.int32), rng.permutation(st.cols).astype(np.int32)
    brp, bci, _, bmap = _color.permute(st.rp, st.ci, np.zeros(st.nnz, f32), p, q, cols=st.cols)
    out = E.Structure(st.rows, st.cols, brp, bci)
    for b0 in range(0, st.rows, 4096):
        by_col = np.sort(bci[brp[b0]:brp[min(b0 + 4096, st.rows)]].astype(np.int64))
        print(f"rows {b0}..: 256 neighbours in column order span at most {int((by_col[255:] - by_col[:-255]).max())} columns")
    assert np.abs(np.diff(bci.astype(np.int64))[out.row_of[1:] == out.row_of[:-1]]).mean() > st.cols // 32, "the rows are not scattered"
    ex = E.Exact(out, "wide_window/relabelled")
    d_rp, d_ci = (torch_from(gpu, a, np.int32) for a in (st.rp, st.ci))
    d_p, d_q = torch_from(gpu, p, np.int32), torch_from(gpu, q, np.int32)

    def parent_vals(vals):
        pv = np.empty(st.nnz, f32)
        pv[bmap.astype(np.int64)] = vals                              # the child's entry i is the parent's entry map[i]
        return torch_from(gpu, pv, f32)

    def make(d_pv):
        parent = capi.CsrMatrix.from_device(st.rows, st.cols, d_rp, d_ci, d_pv)
        try:
            return parent.permute(d_p, d_q)
        finally:
            parent.close()

    loaded = []
    for label, vals, x, want in (("int", ex.vals(), ex.x(), ex.expected()), ("subnormal", ex.sub_vals(), ex.sub_x(), ex.sub_expected())):
        payload = parent_vals(vals)
        child = make(payload)
        try:
            capi.check(capi.lib().spmv_csr_validate(child._h, 0))
            assert not _bits_differ(child.download(), (brp, bci, vals)), f"{label}: the permuted handle differs from the numpy model"
        finally:
            child.close()
        loaded.append((label, payload, x, want))
    failures, ran = _run_paths_on_handle(pkg, monkeypatch, gpu, out, loaded, make)
    assert not failures, f"{len(failures)} failing path(s):\n" + "\n".join(failures)
    assert {p[0] for p in PATHS} - ran <= {"xskip"}, "a path was left out"


def torch_from(gpu, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _colour_of_a_product(capi, gpu, close_early, stream=None):
    """H.colour_of_a_product on the device: every handle's download, the colouring, the levels of M's plans and z."""
    import torch
    c = H.colour_of_a_product()
    live = {n: _borrow(capi, _tensors(gpu, m)) for n, m in c["leaves"].items()}
    got = {}

    def step(name, h, *done):
        live[name] = h
        if close_early:
            for d in done:
                live.pop(d).close()
        got[name] = h.download()

    try:
        step("T", live["A"].transpose(stream=stream))
        step("P", live["A"].spgemm(live["T"], stream=stream), "A", "T")
        step("S", live["P"].add(live["I"], 1.0, 1.0, "union", stream=stream), "P", "I")
        col, perm, cptr, info = live["S"].color(stream=stream)
        got["color"] = (col.cpu().numpy(), perm.cpu().numpy(), cptr, {k: info[k] for k in ("colors", "rounds", "largest", "smallest")})
        step("B", live["S"].permute(perm, perm, stream=stream), "S")
        assert not _companions(live["B"])
        step("M", live["B"].ilu0(stream=stream), "B")
        M = live["M"]
        assert not _companions(M, own=_FACTOR_OWN) and M.ilu0_plan_bytes() > 0 and M.ilu0_pivot(stream=stream) == -1
        capi.check(capi.lib().spmv_csr_validate(M._h, 0))
        got["levels"] = {u: M.trsv_plan_info(u)["levels"] for u in _trsv.UPLOS}
        got["rows"] = {u: M.trsv_plan_rows(u) for u in _trsv.UPLOS}
        z = M.ilu0_solve(torch_from(gpu, c["r"], f32), torch.full((M.rows,), float("nan"), device=gpu), stream=stream)
        torch.cuda.synchronize()
        got["z"] = z.cpu().numpy()
    finally:
        for h in live.values():
            h.close()
    return got


def test_colour_of_a_product(pkg, gpu):
    """color, permute, ilu0 and ilu0_solve on a sum of a product and I, none of whose operands a caller made."""
    import torch
    capi = pkg.capi
    c = H.colour_of_a_product()
    env, (col, perm, cptr, info) = c["env"], c["color"]
    kept = _colour_of_a_product(capi, gpu, close_early=False)
    for name in ("T", "P", "S", "B", "M"):
        assert H.same(kept[name], env[name][2]) is None, f"{name}: {H.same(kept[name], env[name][2])}"
    g_col, g_perm, g_cptr, g_info = kept["color"]
    assert np.array_equal(g_col, col) and np.array_equal(g_perm, perm) and np.array_equal(g_cptr, cptr)
    assert g_info == {k: info[k] for k in g_info}, (g_info, info)
    _, _, (brp, bci, _) = env["B"]
    for uplo in _trsv.UPLOS:
        assert kept["levels"][uplo] <= info["colors"], (uplo, kept["levels"], info)
        lp, od = _trsv.order(_trsv.levels(brp, bci, uplo))
        assert np.array_equal(kept["rows"][uplo][0], lp) and np.array_equal(kept["rows"][uplo][1], od), uplo
    assert _ilu0.same(kept["z"], c["z"]) is None, _ilu0.same(kept["z"], c["z"])
    early = _colour_of_a_product(capi, gpu, close_early=True)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        aside = _colour_of_a_product(capi, gpu, close_early=False, stream=side)
    torch.cuda.synchronize()
    for how, other in (("closed early", early), ("on a side stream", aside)):
        for name in ("T", "P", "S", "B", "M"):
            assert all(np.array_equal(g, w) for g, w in zip(_raw(other[name]), _raw(kept[name]))), f"{name}: other bytes {how}"
        assert np.array_equal(other["z"].view(np.uint32), kept["z"].view(np.uint32)) and other["levels"] == kept["levels"], how
        assert all(np.array_equal(a, b) for a, b in zip(other["color"][:3], kept["color"][:3])), how


@pytest.mark.parametrize("name", H.SOLVED)
def test_selected_then_solved(pkg, gpu, name):
    """trsv as a consumer of transposes, sums, products and selections (rows unsorted, repeated columns, a 5000-entry row):
    trsv_plan's rows are _trsv.levels / _trsv.order, the UNIT solve of both triangles is _trsv.solve; NON_UNIT on the sum
    with I, which has exactly one diagonal entry per row.  With all handles kept open, with every handle closed as soon as its
    last child exists (the selection and the sum of a step are then solved after the step's operands are gone), and on a side
    stream.  (The programs' values are not dominant and 2 % of them are NaN or Inf: of a solve's 257 entries 8 .. 231 are
    finite, the others must be the contract's Inf or a NaN.  6 .. 211 levels.)"""
    import torch
    capi = pkg.capi
    p = H.programs()[name]
    ident = H.identity(257)
    I = _borrow(capi, _tensors(gpu, ident))
    wants = {}

    def want(what, mat, unit):
        """{uplo: (level_ptr, order, x)} and b, computed once."""
        if what not in wants:
            if unit:
                wants[what] = H.triangles(mat)
            else:
                rp, ci, va = mat[2]
                b = _trsv.rhs(mat[0], np.random.default_rng(3143))
                tri = {}
                for uplo in _trsv.UPLOS:
                    lev = _trsv.levels(rp, ci, uplo)
                    tri[uplo] = _trsv.order(lev) + (_trsv.solve(rp, ci, va, b, uplo, unit=False, lev=lev),)
                wants[what] = (tri, b)
        return wants[what]

    def solved(how, what, h, mat, unit):
        tri, b = want(what, mat, unit)
        d_b = torch_from(gpu, b, f32)
        for uplo in _trsv.UPLOS:
            h.trsv_plan(uplo)
            lp, od = h.trsv_plan_rows(uplo)
            want_lp, want_od, want_x = tri[uplo]
            assert np.array_equal(lp, want_lp) and np.array_equal(od, want_od), f"{name}/{what}/{uplo} ({how}): the plan's rows"
            x = h.trsv(d_b, torch.full((h.rows,), float("nan"), device=gpu), uplo=uplo, unit=unit)
            torch.cuda.synchronize()
            bad = _trsv.same(x.cpu().numpy(), want_x)
            assert bad is None, f"{name}/{what}/{uplo} unit={unit} ({how}): {bad}"

    def visitor(how):
        def visit(step, builder, h):
            mat = p.host[step]
            assert h.rows == h.cols == 257
            solved(how, step, h, mat, True)
            K = h.select_topk(H.SOLVED_K)
            S = h.add(I, 1.0, 1.0, "union")
            try:
                solved(how, step + " top-k", K, H.host_step("select_topk", [mat], k=H.SOLVED_K), True)
                solved(how, step + " + I", S, H.host_step("add", [mat, ident], op="union"), False)
            finally:
                K.close()
                S.close()
        return visit

    try:
        _run_device(capi, gpu, p.leaves, p.steps, close_early=False, visit=visitor("kept open"))
        _run_device(capi, gpu, p.leaves, p.steps, close_early=True, visit=visitor("closed early"))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            _run_device(capi, gpu, p.leaves, p.steps, close_early=False, stream=side, visit=visitor("on a side stream"))
        torch.cuda.synchronize()
    finally:
        I.close()


def test_one_map_per_handle(pkg, gpu):
    """Six handles of one shape and one nnz, one from each builder with its companion kept: every _values / _gather / _scatter
    call of another builder, and ilu0_solve and ilu0_pivot, refuse them by what made them; no value and no destination changes."""
    import ctypes as C
    import torch
    capi = pkg.capi
    L = capi.lib()
    sq = H.leaf(3301, 257, 257, 20, special=0.0)
    s_mat = H.host_step("add", [sq, H.identity(257)], alpha=1.0, beta=64.0, op="union")     # sorted, duplicate-free, a diagonal
    inside = H.host_step("select_topk", [s_mat], k=3)
    S, D, IN = (_borrow(capi, _tensors(gpu, m)) for m in (s_mat, _diag(257, 3302), inside))
    perm = torch_from(gpu, np.random.default_rng(3303).permutation(257), np.int32)
    made = {"transpose": S.transpose(keep_map=True), "select": S.select_topk(10 ** 6, keep_map=True), "spgemm": D.spgemm(S, keep_plan=True),
            "add": S.add(IN, 1.0, 1.0, "union", keep_plan=True), "permute": S.permute(perm, perm, keep_map=True), "ilu0": S.ilu0()}
    nnz = S.nnz
    src = torch.arange(nnz, dtype=torch.float32, device=gpu)
    dst = torch.full((nnz,), -7.0, device=gpu)
    row = C.c_int64(-2)
    sp, dp = src.data_ptr(), dst.data_ptr()
    calls = {
        "transpose": [("transpose_values", lambda h: L.spmv_csr_transpose_values(h, S._h, None)),
                      ("transpose_gather", lambda h: L.spmv_csr_transpose_gather(h, 1, sp, 0, dp, 0, None))],
        "select": [("select_values", lambda h: L.spmv_csr_select_values(h, S._h, None)),
                   ("select_gather", lambda h: L.spmv_csr_select_gather(h, 1, sp, 0, dp, 0, None)),
                   ("select_scatter", lambda h: L.spmv_csr_select_scatter(h, 1, sp, 0, dp, 0, None))],
        "spgemm": [("spgemm_values", lambda h: L.spmv_csr_spgemm_values(h, D._h, S._h, None))],
        "add": [("add_values", lambda h: L.spmv_csr_add_values(h, S._h, IN._h, 1.0, 1.0, None)),
                ("add_gather", lambda h: L.spmv_csr_add_gather(h, 0, 1, sp, 0, dp, 0, None))],
        "permute": [("permute_values", lambda h: L.spmv_csr_permute_values(h, S._h, None)),
                    ("permute_gather", lambda h: L.spmv_csr_permute_gather(h, 1, sp, 0, dp, 0, None))],
        "ilu0": [("ilu0_values", lambda h: L.spmv_csr_ilu0_values(h, S._h, None)),
                 ("ilu0_solve", lambda h: L.spmv_csr_ilu0_solve(h, sp, dp, None)),
                 ("ilu0_pivot", lambda h: L.spmv_csr_ilu0_pivot(h, None, C.byref(row)))],
    }
    try:
        for maker, h in made.items():
            assert (h.rows, h.cols, h.nnz) == (257, 257, nnz), maker
            own = _FACTOR_OWN if maker == "ilu0" else (maker,)
            assert not _companions(h, own=own) and all(k in _companions(h) for k in own), f"{maker}: {_companions(h)}"
            before = h.download()
            for family, fns in calls.items():
                if family == maker:
                    continue
                for call, fn in fns:
                    rc = fn(h._h)
                    msg = L.spmv_last_error().decode(errors="replace")
                    assert rc == capi.ERR_INVALID, f"{call} on a handle made by {maker}: status {rc}"
                    assert f"spmv_csr_{call}:" in msg and ("was not made by" in msg), f"{call} on a handle made by {maker}: {msg}"
            torch.cuda.synchronize()
            assert not _bits_differ(h.download(), before), f"a refused call changed the handle made by {maker}"
        assert bool((dst == -7.0).all()) and row.value == -2, "a refused call wrote its destination"
    finally:
        for h in list(made.values()) + [S, D, IN]:
            h.close()


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


REFRESH2_BETA = 64.0       # S = A + 64 I: integer values, and every row dominant (at most 12 entries of magnitude 4 beside 64)


def _refresh2_host(a, va, perm):
    """S = A + 64 I, B = permute(S, perm, perm), M = ILU(0) of B on the host for A's values va."""
    A = (a[0], a[1], (a[2][0], a[2][1], va))
    return H.run_host({"A": A, "I": H.identity(a[0])},
                      [("S", "add", ("A", "I"), dict(alpha=1.0, beta=REFRESH2_BETA, op="union")),
                       ("B", "permute", ("S",), dict(row_perm=perm, col_perm=perm)), ("M", "ilu0", ("B",), {})])


def test_refresh_through_permute_and_ilu0(pkg, gpu):
    """M = ilu0(B), B = permute(S, perm, perm) with its map, S = add(A, I) with its plan, perm from color(S).  A's values are
    rewritten in place and add_values, permute_values and ilu0_values called in order: B and M hold the host composition of the
    new values; the SPMV_PANEL plans made before answer SPMV_ERR_STALE_PLAN, SPMV_TILED and spmm follow (B exactly, on
    integers; M within 1e-5 of the sum of |terms| against float64 on the model's factor); ilu0_solve uses the new factor; no
    plan of the solve was rebuilt and nothing was allocated.  Then the three calls and a solve replay from a graph.  (run_vals16
    takes its 16-bit values with every call and keeps no plan of its own: it runs once on SPMV_TILED's, made before the refresh.)"""
    import torch
    capi = pkg.capi
    a = H.leaf(3211, 257, 257, 12, special=0.0)
    kx = 4
    ta, ti = _tensors(gpu, (a[0], a[1], (a[2][0], a[2][1], _int_leaf(a, 5)))), _tensors(gpu, H.identity(257))
    A, I = _borrow(capi, ta), _borrow(capi, ti)
    S = A.add(I, 1.0, REFRESH2_BETA, "union", keep_plan=True)
    _, d_perm, _, _ = S.color()
    perm = d_perm.cpu().numpy()
    B = S.permute(d_perm, d_perm, keep_map=True)
    M = B.ilu0()
    chain = (("S", S), ("B", B), ("M", M))
    rng = np.random.default_rng(3212)
    m_int = rng.integers(-4, 5, (257, kx))
    d_x, d_X = torch_from(gpu, m_int[:, 0], f32), torch_from(gpu, m_int, f32)
    r = _trsv.rhs(257, rng)
    d_r, d_z = torch_from(gpu, r, f32), torch.full((257,), float("nan"), device=gpu)

    def rewrite(seed):
        va = _int_leaf(a, seed)
        ta[2][2].copy_(torch.from_numpy(va).to(gpu))                    # in place: A borrows this tensor
        return _refresh2_host(a, va, perm)

    def products(mat):
        """(float64 mat m_int, the sum of |terms|) per row and column."""
        rows, _, (rp, ci, va) = mat
        row = np.repeat(np.arange(rows), np.diff(rp))
        t = va.astype(np.float64)[:, None] * m_int[ci]
        y, mag = np.zeros((rows, kx)), np.zeros((rows, kx))
        np.add.at(y, row, t)
        np.add.at(mag, row, np.abs(t))
        return y, mag

    def check_y(what, got, mat, exact):
        if exact:
            want = _int_y(mat, m_int)
            bad = [f"column {c}: {_mismatches(got[:, c], want[:, c])}" for c in range(got.shape[1]) if _mismatches(got[:, c], want[:, c])]
            assert not bad, f"{what}: {bad[:3]}"
        else:
            y, mag = products(mat)
            for c in range(got.shape[1]):
                assert_close_to_oracle(got[:, c], y[:, c], mag[:, c], f"{what}, column {c}")

    def run(h, v):
        y = torch.full((h.rows,), float("nan"), dtype=torch.float32, device=gpu)
        h.run(v, d_x, y)
        torch.cuda.synchronize()
        return y.cpu().numpy()[:, None]

    def spmm(h):
        Y = torch.full((h.rows, kx), float("nan"), dtype=torch.float32, device=gpu)
        h.spmm(d_X, Y)
        torch.cuda.synchronize()
        return Y.cpu().numpy()

    try:
        env = _refresh2_host(a, _int_leaf(a, 5), perm)
        assert np.array_equal(perm, _color.color(env["S"][2][0], env["S"][2][1])[1]), "the device's colouring"
        for name, h in chain:
            assert H.same(h.download(), env[name][2]) is None, f"{name} as built: {H.same(h.download(), env[name][2])}"
        assert _companions(S) == {"add": S.add_plan_bytes()} and _companions(B) == {"permute": 4 * B.nnz}
        assert not _companions(M, own=_FACTOR_OWN)
        for h in (B, M):
            h.plan_set(capi.PANEL, [capi.PANEL, 0, 0, 0, 0, 0, 1, 0])
            h.plan(capi.TILED)
            h.spmm_plan()
            check_y("as built", run(h, capi.TILED), env["B" if h is B else "M"], h is B)
        plan_bytes = {u: M.trsv_plan_bytes(u) for u in _trsv.UPLOS}
        plan_rows = {u: M.trsv_plan_rows(u) for u in _trsv.UPLOS}
        env = rewrite(10)
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        S.add_values(A, I, 1.0, REFRESH2_BETA)
        B.permute_values(S)
        M.ilu0_values(B)
        M.ilu0_solve(d_r, d_z)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free, "a refresh or the solve allocated device memory"
        assert {u: M.trsv_plan_bytes(u) for u in _trsv.UPLOS} == plan_bytes, "a plan of the solve was rebuilt"
        for u in _trsv.UPLOS:
            assert all(np.array_equal(g, w) for g, w in zip(M.trsv_plan_rows(u), plan_rows[u])), u
        for name, h in chain:
            assert H.same(h.download(), env[name][2]) is None, f"{name} refreshed: {H.same(h.download(), env[name][2])}"
        assert M.ilu0_pivot() == -1 and np.all(np.isfinite(env["M"][2][2]))
        want_z = _ilu0.apply(*env["M"][2], r)
        assert _ilu0.same(d_z.cpu().numpy(), want_z) is None, f"ilu0_solve after ilu0_values: {_ilu0.same(d_z.cpu().numpy(), want_z)}"
        for name, h in chain[1:]:
            with pytest.raises(capi.SpmvError) as e:
                run(h, capi.PANEL)
            assert e.value.status == capi.ERR_STALE_PLAN and "values_changed" in str(e.value), f"{name}: {e.value}"
            h.plan(capi.PANEL)
            check_y(f"{name}: SPMV_PANEL after plan", run(h, capi.PANEL), env[name], h is B)
            check_y(f"{name}: the SPMV_TILED plan made before the refresh", run(h, capi.TILED), env[name], h is B)
            check_y(f"{name}: spmm on the plan made before the refresh", spmm(h), env[name], h is B)
        # run_vals16 keeps no plan of its own: it reads SPMV_TILED's, made before the refresh, and the 16-bit values of the call
        own = env["B"][2][2]
        bits = R16.convert("bf16", own)
        assert np.array_equal(R16.widen("bf16", bits).view(np.uint32), own.view(np.uint32)), "the narrowing must be exact"
        v16 = torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(gpu).view(torch.bfloat16)
        y16 = torch.full((B.rows,), float("nan"), dtype=torch.float32, device=gpu)
        B.run_vals16(capi.TILED, v16, d_x, y16)
        torch.cuda.synchronize()
        check_y("B: run_vals16 on the SPMV_TILED plan made before the refresh", y16.cpu().numpy()[:, None], env["B"], True)
        # the three refreshes and one solve in one graph, replayed after two more rewrites
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            S.add_values(A, I, 1.0, REFRESH2_BETA)
            B.permute_values(S)
            M.ilu0_values(B)
            M.ilu0_solve(d_r, d_z)
        for seed in (20, 30):
            env = rewrite(seed)
            d_z.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            for name, h in chain:
                assert H.same(h.download(), env[name][2]) is None, f"{name} after replay {seed}: {H.same(h.download(), env[name][2])}"
            want_z = _ilu0.apply(*env["M"][2], r)
            assert _ilu0.same(d_z.cpu().numpy(), want_z) is None, f"the solve after replay {seed}"
        del g
    finally:
        for h in (M, B, S, A, I):
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
    free = []
    for _ in range(4):
        _colour_of_a_product(capi, gpu, close_early=False)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"colour_of_a_product: free device memory per round: {free}"


# ---- 4. a handle as its own operand ---------------------------------------------------------------------------------------------------
def _diag(n, seed):
    rng = np.random.default_rng(seed)
    return n, n, (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), _spgemm.spread(rng, n))


@pytest.mark.parametrize("call", ["transpose_values", "select_values", "add_values", "spgemm_values", "permute_values", "ilu0_values"])
def test_a_refresh_refuses_its_own_target_as_an_operand(pkg, gpu, call):
    """In each construction the sizes the handle recorded agree with its own, so only the pointer rule can refuse the call: the
    transpose of a square matrix; a selection that dropped nothing; a sum whose b lies inside a; a product with a diagonal a; any
    permuted handle; any factor handle."""
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
    elif call == "permute_values":
        parents = [_borrow(capi, _tensors(gpu, sq))]
        t = parents[0].permute(keep_map=True)
        attempt = lambda: t.permute_values(t)                          # noqa: E731
    elif call == "ilu0_values":
        parents = [_borrow(capi, _tensors(gpu, H.host_step("add", [sq, H.identity(257)], alpha=1.0, beta=64.0, op="union")))]
        t = parents[0].ilu0()
        attempt = lambda: t.ilu0_values(t)                             # noqa: E731
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
