"""spmv_csr_spmm_cols and spmv_csr_sddmm_cols on the GPU (include/spmv_hip.h "SpMM and SDDMM at any k"), with no tolerance
anywhere but in the one fp64 check of the larger structure.

Patterns and data are tests/_cols.py's (P1, P2, and P1's transpose, where every row goes in pieces), widths 65 .. 257, the
dtypes fp32, bf16 and fp16.  A 16-bit case runs on the data rounded to the format; its reference is the fp32 reference of the
widened data, for SpMM rounded once by tests/_round16.py.
  order        both calls are tests/_cols.py bit for bit (fp32), at an ld on the vector path and one on the element path, on
               column-block views of wider tensors whose other columns, like every row no nonzero refers to, hold NaN; Y and out
               start as NaN and Y's columns >= k keep it.
  narrow       tile t of spmm_cols is the narrow call on that column block, sddmm_cols the fp32 fold of the narrow calls'
               results, in all three dtypes; at k = 1, 13 and 64 both are the narrow calls' bits; a column of a k = 130 call has
               the bits of a k = 64 narrow call on columns [40, 104).
  minus zero   a result whose every tile is -0 stays -0 (a fold started from +0 would lose it).
  blocks       a structure of 8000 rows with long rows, against the narrow calls and fp64.
  plan         NOT_PLANNED before and beyond the plan, growth keeps results, plan_bytes, the narrow calls' bits unchanged.
  refusals, empty shapes, graph capture."""
import numpy as np
import pytest

import _cols as CO
import _exact as E
import _round16 as R
from _util import RTOL

pytestmark = pytest.mark.gpu

FORMATS = ("fp32",) + R.FORMATS
NAN32 = np.float32(np.nan)


def lds(k):
    """(vector path, element path): k + 4 rounded up to a multiple of 4; and k itself where that is no multiple of 4 (else k + 1)."""
    return (k + 4 + 3) // 4 * 4, (k if k % 4 else k + 1)


def _torch_dtype(fmt):
    import torch
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[fmt]


def in_format(fmt, x):
    """x (fp32) rounded to the format, as fp32 numbers."""
    x = np.ascontiguousarray(x, np.float32)
    return x if fmt == "fp32" else R.widen(fmt, R.convert(fmt, x))


def rounded(fmt, y):
    """What a store of the fp32 numbers y leaves in a matrix of the format, as fp32 numbers."""
    return in_format(fmt, y)


def operand(gpu, fmt, data, ld, nan_rows=None, first=0):
    """A (n, k) view with stride ld at column `first` of a wider device tensor; every other column and all of nan_rows are NaN.
    (data holds numbers of the format, so the conversion is exact.)"""
    import torch
    n, k = data.shape
    full = np.full((n, first + ld), NAN32, np.float32)
    full[:, first:first + k] = data
    if nan_rows is not None:
        full[nan_rows] = NAN32
    t = torch.from_numpy(full).to(gpu).to(_torch_dtype(fmt))
    if first:                                     # (a view that starts inside the rows: the base moves, the stride stays)
        assert (first * t.element_size()) % 16 == 0
    return t[:, first:first + k]


def host(t):
    import torch
    return t.to(torch.float32).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(bits(a), bits(b))


class Handle:
    def __init__(self, pkg, gpu, s, vals, k_max=CO.K_MAX):
        import torch
        self.s, self.vals, self.gpu = s, vals, gpu
        self.keep = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (s.rp, s.ci, vals)]
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        if k_max:
            self.A.spmm_plan_cols(k_max)
        self.unref_cols = np.setdiff1d(np.arange(s.cols), s.ci)
        self.empty_rows = np.flatnonzero(np.diff(s.rp) == 0)

    def spmm(self, fmt, X, ldx, ldy, cols=True, nan_rows=None, first=0):
        """(Y[:, :k], Y[:, k:]) as fp32 of one call on X (cols, k), Y pre-filled with NaN."""
        import torch
        k = X.shape[1]
        Xd = operand(self.gpu, fmt, X, ldx, nan_rows, first)
        Y = torch.full((self.s.rows, ldy), float("nan"), dtype=_torch_dtype(fmt), device=self.gpu)
        (self.A.spmm_cols if cols else self.A.spmm)(Xd, Y[:, :k])
        torch.cuda.synchronize()
        y = host(Y)
        return y[:, :k], y[:, k:]

    def sddmm(self, fmt, U, X, ldu, ldx, cols=True, u_nan=None, x_nan=None, first=0):
        import torch
        Ud, Xd = operand(self.gpu, fmt, U, ldu, u_nan, first), operand(self.gpu, fmt, X, ldx, x_nan, first)
        out = torch.full((self.s.nnz,), float("nan"), dtype=torch.float32, device=self.gpu)
        (self.A.sddmm_cols if cols else self.A.sddmm)(Ud, Xd, out)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def narrow_spmm(self, fmt, X):
        """The narrow calls on the column blocks of X, side by side."""
        return np.concatenate([self.spmm(fmt, X[:, a:b], *lds(b - a)[:1] * 2, cols=False)[0] for a, b in CO.tiles(X.shape[1])], axis=1)

    def narrow_sddmm(self, fmt, U, X):
        """The fp32 fold of the narrow calls' results over the column blocks."""
        return CO.fold([self.sddmm(fmt, U[:, a:b], X[:, a:b], *lds(b - a)[:1] * 2, cols=False) for a, b in CO.tiles(U.shape[1])])


@pytest.fixture(scope="module")
def handles(pkg, gpu):
    out = {}
    for name in CO.PATTERNS:
        s, vals, _, _ = CO.data(name)
        out[name] = Handle(pkg, gpu, s, vals)
    assert (np.diff(out["P1T"].s.rp) > 512).all() and np.diff(out["P1"].s.rp).max() > 1536
    assert out["P2"].unref_cols.size and out["P2"].empty_rows.size and out["P1T"].unref_cols.size
    yield out
    for h in out.values():
        h.A.close()


# ---- the documented order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CO.WIDTHS)
@pytest.mark.parametrize("name", CO.PATTERNS)
def test_spmm_cols_is_the_documented_order(handles, name, k):
    h = handles[name]
    _, _, _, X = CO.data(name)
    want = CO.spmm_reference(name)[:, :k]
    for i, ld in enumerate(lds(k)):
        first = 64 * i                                      # the second case is a column block inside wider rows
        y, pad = h.spmm("fp32", X[:, :k], ld, ld, nan_rows=h.unref_cols, first=first)
        assert not np.isnan(y).any(), f"k = {k}, ld = {ld}: a NaN of the padding or of an unreferenced row was read, or Y not written"
        bad = np.argwhere(bits(y) != bits(want))
        assert bad.size == 0, f"k = {k}, ld = {ld}: {len(bad)} elements differ from the documented order, first {bad[0]}"
        assert np.isnan(pad).all(), f"k = {k}, ld = {ld}: Y was written at columns >= k"


@pytest.mark.parametrize("k", CO.WIDTHS)
@pytest.mark.parametrize("name", CO.PATTERNS)
def test_sddmm_cols_is_the_documented_order(handles, name, k):
    h = handles[name]
    _, _, U, X = CO.data(name)
    want = CO.sddmm_reference(name, k)
    fast, slow = lds(k)
    for ldu, ldx, first in ((fast, fast, 0), (slow, slow, 0), (fast, slow, 64)):
        out = h.sddmm("fp32", U[:, :k], X[:, :k], ldu, ldx, u_nan=h.empty_rows, x_nan=h.unref_cols, first=first)
        assert not np.isnan(out).any(), f"k = {k}, ld = {ldu}, {ldx}: a NaN of the padding or of an unused row was read"
        bad = np.flatnonzero(bits(out) != bits(want))
        assert bad.size == 0, f"k = {k}, ld = {ldu}, {ldx}: {bad.size} nonzeros differ from the documented order, first {bad[0]}"
    if len(CO.tiles(k)) >= 3:                                # (the reference has teeth here: tests/test_cols_host.py)
        assert (bits(want) != bits(CO.sddmm_reference(name, k, "reversed"))).sum() >= 1000


# ---- agreement with the narrow calls, all three dtypes --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", CO.PATTERNS)
def test_cols_calls_agree_with_the_narrow_calls(handles, name, fmt):
    h = handles[name]
    _, _, U, X = CO.data(name)
    U, X = in_format(fmt, U), in_format(fmt, X)
    for k in CO.WIDTHS + (1, 13, 64):
        for ld in lds(k):
            y, pad = h.spmm(fmt, X[:, :k], ld, ld, nan_rows=h.unref_cols)
            assert same_bits(y, h.narrow_spmm(fmt, X[:, :k])), f"{fmt} k = {k}, ld = {ld}: spmm_cols differs from the narrow calls"
            assert np.isnan(pad).all(), f"{fmt} k = {k}, ld = {ld}: Y was written at columns >= k"
            out = h.sddmm(fmt, U[:, :k], X[:, :k], ld, ld, u_nan=h.empty_rows, x_nan=h.unref_cols)
            assert same_bits(out, h.narrow_sddmm(fmt, U[:, :k], X[:, :k])), f"{fmt} k = {k}, ld = {ld}: sddmm_cols differs from the fold"
    if fmt != "fp32":
        # the 16-bit calls against the fp32 references of the widened data: Y rounded once, out the fp32 call's bits
        k = 130
        y32, _ = h.spmm("fp32", X[:, :k], 136, 136)
        y, _ = h.spmm(fmt, X[:, :k], 136, 136)
        assert same_bits(y, rounded(fmt, y32)), f"{fmt}: Y is not the fp32 call's Y rounded once"
        assert np.mean(bits(rounded(fmt, y32)) != bits(y32)) > 0.9
        assert same_bits(h.sddmm(fmt, U[:, :k], X[:, :k], 136, 136), h.sddmm("fp32", U[:, :k], X[:, :k], 130, 130))


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_columns_bits_do_not_depend_on_the_batch(handles, fmt):
    h = handles["P1"]
    X = in_format(fmt, CO.data("P1")[3])
    wide, _ = h.spmm(fmt, X[:, :130], 136, 136)
    narrow, _ = h.spmm(fmt, X[:, 40:104], 64, 68, cols=False)
    assert same_bits(wide[:, 40:104], narrow), "a column of a k = 130 call differs from the k = 64 narrow call on columns [40, 104)"
    again, _ = h.spmm(fmt, X[:, 3:], 254, 256)              # the same columns, three places further left, at k = 254
    assert same_bits(again[:, 37:101], narrow), "a column's bits change with its position in the batch"


def test_a_result_of_minus_zero_in_every_tile_stays_minus_zero(handles):
    h = handles["P2"]
    for k in (128, 192):
        s, _, U, X = CO.data("P2")
        U, X = U[:, :k].copy(), X[:, :k].copy()
        where = CO.minus_zero(s, U, X)
        out = h.sddmm("fp32", U, X, k, k)
        assert (bits(out)[where] == 0x80000000).all(), f"k = {k}: a -0 of every tile came out as {bits(out)[where][:4]}"
        assert same_bits(out, h.narrow_sddmm("fp32", U, X))


# ---- more than one block ---------------------------------------------------------------------------------------------------------
def test_more_than_one_block_against_the_narrow_calls_and_fp64(pkg, gpu):
    s = E.structure("wave_pipe_thresholds")                  # 8000 rows: two sort blocks of the plan, 500 workgroups, 5 long rows
    assert s.rows > 4096 and (np.diff(s.rp) > 512).sum() >= 3
    k = 130
    from _order_cases import randn
    vals, U, X = randn([2300], (s.nnz,), (s.rows, k), (s.cols, k))
    h = Handle(pkg, gpu, s, vals, k_max=k)
    try:
        assert "long_rows=5 " in h.A.spmm_describe()
        y, _ = h.spmm("fp32", X, 136, 136)
        assert same_bits(y, h.narrow_spmm("fp32", X)), "spmm_cols differs from the narrow calls"
        out = h.sddmm("fp32", U, X, 130, 136)
        assert same_bits(out, h.narrow_sddmm("fp32", U, X)), "sddmm_cols differs from the fold of the narrow calls"
        # fp64, within the project's bound relative to the magnitude sum |u_c x_c|
        Ui, Xj = U[s.row_of].astype(np.float64), X[s.ci].astype(np.float64)
        ref, mag = np.einsum("nc,nc->n", Ui, Xj), np.einsum("nc,nc->n", np.abs(Ui), np.abs(Xj))
        err = np.abs(out.astype(np.float64) - ref)
        print(f"sddmm_cols k={k}: max err / magnitude = {np.max(err / mag):.3g} (bound {RTOL:g})")
        assert (err <= RTOL * mag + 1e-37).all()
    finally:
        h.A.close()


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def test_plan_rules(pkg, handles, gpu):
    import torch
    capi = pkg.capi
    s, vals, U, X = CO.data("P1")
    h = Handle(pkg, gpu, s, vals, k_max=0)
    try:
        Xd, Ud = operand(gpu, "fp32", X[:, :132], 136), operand(gpu, "fp32", U[:, :132], 136)
        Y = torch.full((s.rows, 136), float("nan"), device=gpu)
        out = torch.full((s.nnz,), float("nan"), device=gpu)

        def refused(k):
            for call in (lambda: h.A.spmm_cols(Xd[:, :k], Y[:, :k]), lambda: h.A.sddmm_cols(Ud[:, :k], Xd[:, :k], out)):
                with pytest.raises(capi.SpmvError) as e:
                    call()
                assert e.value.status == capi.ERR_NOT_PLANNED and "spmv_csr_spmm_plan_cols" in str(e.value)
            torch.cuda.synchronize()
            assert bool(torch.isnan(Y).all()) and bool(torch.isnan(out).all())

        refused(8)                                           # not planned at all
        h.A.spmm_plan()
        refused(8)                                           # the narrow plan alone does not serve, at any width
        narrow_bytes, line = h.A.spmm_plan_bytes(), h.A.spmm_describe()
        pieces = int(line.split("pieces=")[1])
        assert pieces > 0
        y_narrow = h.spmm("fp32", X[:, :64], 64, 64, cols=False)[0]
        h.A.spmm_plan_cols(64)
        assert h.A.spmm_plan_bytes() == narrow_bytes + pieces * 64 * 4 and h.A.spmm_describe() == line
        refused(65)                                          # beyond the plan
        y64 = h.spmm("fp32", X[:, :64], 64, 64)[0]
        assert same_bits(y64, y_narrow)
        h.A.spmm_plan_cols(130)                              # growing keeps results
        assert h.A.spmm_plan_bytes() == narrow_bytes + pieces * 3 * 64 * 4
        h.A.spmm_plan_cols(70), h.A.spmm_plan_cols(130)      # repeated and smaller: nothing changes
        assert h.A.spmm_plan_bytes() == narrow_bytes + pieces * 3 * 64 * 4 and h.A.spmm_describe() == line
        refused(131)
        assert same_bits(h.spmm("fp32", X[:, :64], 64, 64)[0], y_narrow)
        assert same_bits(h.spmm("fp32", X[:, :130], 132, 132)[0], CO.spmm_reference("P1")[:, :130])
        assert same_bits(h.spmm("fp32", X[:, :64], 64, 64, cols=False)[0], y_narrow), "the narrow call after _plan_cols"
        h.A.spmm_plan_cols(192)                              # within three tiles: covered without a new allocation
        assert h.A.spmm_plan_bytes() == narrow_bytes + pieces * 3 * 64 * 4
    finally:
        h.A.close()
    # one rule on a handle without a long row
    s2 = CO.pattern("P2")
    short = E.Structure(3, s2.cols, np.array([0, 2, 2, 5]), np.arange(5))
    g = Handle(pkg, gpu, short, np.ones(5, np.float32), k_max=0)
    try:
        g.A.spmm_plan()
        x = torch.ones((short.cols, 8), device=gpu)
        y = torch.full((3, 8), float("nan"), device=gpu)
        with pytest.raises(capi.SpmvError) as e:
            g.A.spmm_cols(x, y)
        assert e.value.status == capi.ERR_NOT_PLANNED
        before = g.A.spmm_plan_bytes()
        g.A.spmm_plan_cols(8)
        assert g.A.spmm_plan_bytes() == before               # no pieces: no scratch
        g.A.spmm_cols(x, y)
        torch.cuda.synchronize()
        assert y.cpu().numpy()[:, 0].tolist() == [2.0, 0.0, 3.0]
    finally:
        g.A.close()


# ---- refusals launch nothing -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(pkg, handles, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h = handles["P2"].A
    k, ld = 130, 136
    X = torch.ones((h.cols + 1, ld), device=gpu)
    U = torch.ones((h.rows + 1, ld), device=gpu)
    Y = torch.full((h.rows + 1, ld), float("nan"), device=gpu)
    out = torch.full((h.nnz,), float("nan"), device=gpu)
    stream = capi._stream_handle()

    def spmm(dt=capi.ATTN_FP32, kk=k, x=X.data_ptr(), ldx=ld, y=Y.data_ptr(), ldy=ld):
        return "spmv_csr_spmm_cols", lib.spmv_csr_spmm_cols(h._h, dt, kk, x, ldx, y, ldy, stream)

    def sddmm(dt=capi.ATTN_FP32, kk=k, u=U.data_ptr(), ldu=ld, x=X.data_ptr(), ldx=ld, o=out.data_ptr()):
        return "spmv_csr_sddmm_cols", lib.spmv_csr_sddmm_cols(h._h, dt, kk, u, ldu, x, ldx, o, stream)

    INV = capi.ERR_INVALID
    big = 65537
    refused = [
        (spmm, dict(kk=0)), (sddmm, dict(kk=0)), (spmm, dict(kk=big, ldx=big, ldy=big)), (sddmm, dict(kk=big, ldu=big, ldx=big)),
        (spmm, dict(ldx=k - 1)), (spmm, dict(ldy=k - 1)), (sddmm, dict(ldu=k - 1)), (sddmm, dict(ldx=k - 1)),
        (spmm, dict(x=X.data_ptr() + 4)), (spmm, dict(y=Y.data_ptr() + 8)), (sddmm, dict(u=U.data_ptr() + 4)), (sddmm, dict(x=X.data_ptr() + 8)),
        (spmm, dict(dt=capi.ATTN_BF16, x=X.data_ptr() + 4)), (sddmm, dict(dt=capi.ATTN_FP16, u=U.data_ptr() + 2)),
        (sddmm, dict(o=out.data_ptr() + 2)), (sddmm, dict(o=None)), (spmm, dict(x=None)), (spmm, dict(y=None)),
        (spmm, dict(dt=3)), (spmm, dict(dt=-1)), (sddmm, dict(dt=3)), (sddmm, dict(dt=7)),
    ]
    for call, kw in refused:
        name, rc = call(**kw)
        msg = lib.spmv_last_error().decode()
        assert rc == INV, f"{name}({kw}) returned {rc}: {msg}"
        assert msg.startswith(name), f"{name}({kw}): {msg}"
    assert lib.spmv_csr_spmm_plan_cols(h._h, 0, stream) == INV and lib.spmv_csr_spmm_plan_cols(h._h, big, stream) == INV
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all()) and bool(torch.isnan(out).all()), "a refused call wrote to its output"
    assert spmm()[1] == capi.OK and sddmm()[1] == capi.OK, lib.spmv_last_error()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Y[: h.rows, :k]).any()) and not bool(torch.isnan(out).any())
    assert bool(torch.isnan(Y[:, k:]).all()) and bool(torch.isnan(Y[h.rows:]).all())


# ---- empty shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,nnz", [(0, 10, 0), (5, 0, 0), (7, 9, 0)])
def test_cols_empty_shapes(pkg, gpu, rows, cols, nnz):
    import torch
    d_rp = torch.zeros(rows + 1, dtype=torch.int32, device=gpu)
    d_ci = torch.zeros(max(nnz, 1), dtype=torch.int32, device=gpu)[:nnz]
    d_va = torch.zeros(max(nnz, 1), dtype=torch.float32, device=gpu)[:nnz]
    A = pkg.capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan_cols(130)
    for k in (1, 64, 65, 130):
        for dt in (torch.float32, torch.bfloat16):
            X = torch.ones((cols, k), dtype=dt, device=gpu)
            U = torch.ones((rows, k), dtype=dt, device=gpu)
            Y = torch.full((rows, k), float("nan"), dtype=dt, device=gpu)
            out = torch.zeros(0, dtype=torch.float32, device=gpu)
            A.spmm_cols(X, Y)
            A.sddmm_cols(U, X, out)
            torch.cuda.synchronize()
            assert torch.equal(Y, torch.zeros_like(Y))
    A.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
def test_both_calls_are_graph_capturable(handles, gpu):
    import torch
    h = handles["P1"]
    _, _, U0, X0 = CO.data("P1")
    k, ld = 130, 136
    h.spmm("fp32", X0[:, :k], ld, ld), h.sddmm("fp32", U0[:, :k], X0[:, :k], ld, ld)        # (the warm runs)
    X, U = operand(gpu, "fp32", X0[:, :k], ld), operand(gpu, "fp32", U0[:, :k], ld)
    Y = torch.full((h.s.rows, ld), float("nan"), device=gpu)
    out = torch.full((h.s.nnz,), float("nan"), device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream: the graph is a chain, no parallel branches)
        h.A.spmm_cols(X, Y[:, :k])
        h.A.sddmm_cols(U, X, out)
    for shift in (7, 100):                                   # fresh operands: other columns of the data
        x, u = X0[:, shift:shift + k], U0[:, shift:shift + k]
        X.copy_(torch.from_numpy(np.ascontiguousarray(x)).to(gpu)), U.copy_(torch.from_numpy(np.ascontiguousarray(u)).to(gpu))
        Y.fill_(float("nan")), out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        y = Y.cpu().numpy()
        assert same_bits(y[:, :k], h.spmm("fp32", x, ld, ld)[0]) and np.isnan(y[:, k:]).all(), f"replay {shift}: Y differs from the direct call"
        assert same_bits(out.cpu().numpy(), h.sddmm("fp32", u, x, ld, ld)), f"replay {shift}: out differs from the direct call"
