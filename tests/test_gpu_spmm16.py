"""spmv_csr_spmm_16 and spmv_csr_sddmm_16 on the GPU (include/spmv_hip.h "SpMM and SDDMM on 16-bit matrices"), judged by the
fp32 calls and tests/_round16.py's integer-code conversions, with no tolerance anywhere.

Patterns P1 and P2 of tests/_order_cases.py and P1's transpose ("P1T": every row in pieces), random normal fp32 values, both
dtypes:
  contract       Y16 == round_to_nearest_even(spmm_fp32(widen(X16))) and out == sddmm_fp32(widen(U16), widen(X16)), bit for
                 bit, for k in KS at a fast ld (a multiple of 4: 8-byte slices) and a slow one (2-byte accesses).  Before the
                 comparison the reference itself is checked for teeth: at least a quarter of the compared Y elements differ
                 from the fp32 reference truncated toward zero, so a kernel that truncates fails.  In the same calls Y's
                 columns >= k keep their poison, and NaN in every column >= k of the operands and in every operand row that no
                 nonzero refers to reaches no result.
  invariance     a column's bits are the same at k = 5 and at k = 64, and at another position in the batch.
  construction   hand-made rows, short and longer than 512 (the store of k_spmm_combine): ties to even, fp16 overflow and
                 underflow, subnormals kept, NaN confined to its row, +0 for an empty row.
  symmetry       T.sddmm(X16, U16)[i] == A.sddmm(U16, X16)[perm[i]].
  refusals       launch nothing: the outputs keep their poison and the message names the function.
  graph          both calls captured and replayed on fresh operands give the direct call's bits."""
import ctypes as C

import numpy as np
import pytest

import _exact as E
import _order_cases as OC
import _round16 as R

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 8, 12, 17, 33, 64)
PATTERNS = ("P1", "P2", "P1T")
POISON = {"bf16": 0x7fc1, "fp16": 0x7e01}        # a NaN of the format: the padding of every operand, the fill of every output


def lds(k):
    """(fast, slow): a multiple of 4 elements (one 8-byte access per slice), and one that is not (2-byte accesses)."""
    w = 4 * ((k + 3) // 4)
    return w + 4, w + 1


def _dtype(fmt):
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]


def dev16(gpu, fmt, bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(gpu).view(_dtype(fmt))


def bits16(t):
    import torch
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def bits32(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def padded(fmt, data, ld, nan_rows=None):
    """(n, ld) bits: `data` (n, k) in the leading columns, the format's NaN in every other column and in all of nan_rows."""
    full = np.full((data.shape[0], ld), POISON[fmt], np.uint16)
    full[:, : data.shape[1]] = data
    if nan_rows is not None:
        full[nan_rows] = POISON[fmt]
    return full


def normal16(fmt, seed, shape):
    """Random normal numbers of the format, as bits."""
    return R.convert(fmt, OC.randn(seed, shape)[0])


class Handle:
    """One pattern on the device with its SpMM plan, and what the host needs to know of it."""

    def __init__(self, pkg, gpu, A, keep=()):
        self.A, self.keep = A, keep
        rp, ci, va = A.download()
        self.s = E.Structure(A.rows, A.cols, rp, ci)
        self.vals = va
        self.unref_cols = np.setdiff1d(np.arange(A.cols), ci)                       # X rows that no nonzero refers to
        self.empty_rows = np.flatnonzero(np.diff(rp) == 0)
        A.spmm_plan()


@pytest.fixture(scope="module")
def handles(pkg, gpu):
    import torch
    out = {}
    for i, name in enumerate(("P1", "P2")):
        s = OC.pattern(name)
        vals = OC.randn(1700 + i, (s.nnz,))[0]                                      # fp32, full mantissa
        d = [torch.from_numpy(a).to(gpu) for a in (s.rp, s.ci, vals)]
        out[name] = Handle(pkg, gpu, pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *d), keep=d)
    out["P1T"] = Handle(pkg, gpu, out["P1"].A.transpose())
    assert out["P1"].s.nnz == out["P1T"].s.nnz and (np.diff(out["P1T"].s.rp) > 512).all()
    assert np.diff(out["P1"].s.rp).max() > 1025 and np.diff(out["P2"].s.rp).max() > 512
    assert out["P1T"].unref_cols.size and out["P2"].unref_cols.size and out["P2"].empty_rows.size
    yield out
    for h in reversed(list(out.values())):
        h.A.close()


def spmm16(h, gpu, fmt, X, k, ld_x, ld_y, nan_rows=None):
    """Y's bits (rows, ld_y), poison included, of one call on the bits X (cols, k) laid out at ld_x."""
    import torch
    Xd = dev16(gpu, fmt, padded(fmt, X, ld_x, nan_rows))
    Yd = dev16(gpu, fmt, np.full((h.A.rows, ld_y), POISON[fmt], np.uint16))
    h.A.spmm(Xd[:, :k], Yd[:, :k])
    torch.cuda.synchronize()
    return bits16(Yd)


def spmm32(h, gpu, Xw):
    import torch
    Xd = torch.from_numpy(np.ascontiguousarray(Xw, np.float32)).to(gpu)
    Yd = torch.full((h.A.rows, Xw.shape[1]), float("nan"), dtype=torch.float32, device=gpu)
    h.A.spmm(Xd, Yd)
    torch.cuda.synchronize()
    return Yd.cpu().numpy()


def sddmm16(h, gpu, fmt, U, X, k, ld_u, ld_x, u_nan=None, x_nan=None):
    import torch
    Ud, Xd = dev16(gpu, fmt, padded(fmt, U, ld_u, u_nan)), dev16(gpu, fmt, padded(fmt, X, ld_x, x_nan))
    out = torch.full((h.A.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    h.A.sddmm(Ud[:, :k], Xd[:, :k], out)
    torch.cuda.synchronize()
    return bits32(out)


def sddmm32(h, gpu, Uw, Xw):
    import torch
    Ud, Xd = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu) for a in (Uw, Xw))
    out = torch.full((h.A.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    h.A.sddmm(Ud, Xd, out)
    torch.cuda.synchronize()
    return bits32(out)


# ---- the contract, with the untouched and the unread ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("name", PATTERNS)
def test_spmm16_is_the_fp32_call_rounded_once(handles, gpu, name, fmt):
    h = handles[name]
    for k in KS:
        X = normal16(fmt, [1710, PATTERNS.index(name), k], (h.A.cols, k))
        Xw = R.widen(fmt, X)
        Xw[h.unref_cols] = 0.0
        Y32 = spmm32(h, gpu, Xw)
        assert not np.isnan(Y32).any()
        want = R.convert(fmt, Y32)
        differ = float(np.mean(want != R.convert(fmt, Y32, nearest=False)))
        print(f"{name} {fmt} k={k}: {differ:.3f} of {want.size} elements differ from the truncated reference")
        assert differ >= 0.25, f"k = {k}: the reference has no teeth against truncation ({differ:.3f})"
        for ld in lds(k):
            Y = spmm16(h, gpu, fmt, X, k, ld, ld, nan_rows=h.unref_cols)
            assert not R.is_nan(fmt, Y[:, :k]).any(), f"k = {k}, ld = {ld}: a NaN of the padding or of an unreferenced row was read"
            bad = np.argwhere(Y[:, :k] != want)
            assert bad.size == 0, f"k = {k}, ld = {ld}: {len(bad)} elements differ, first {bad[0]}: " \
                                  f"{Y[tuple(bad[0])]:#06x} != {want[tuple(bad[0])]:#06x} (fp32 {Y32[tuple(bad[0])]!r})"
            assert (Y[:, k:] == POISON[fmt]).all(), f"k = {k}, ld = {ld}: Y was written at columns >= k"


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm16_is_the_fp32_call_on_the_widened_operands(handles, gpu, name, fmt):
    h = handles[name]
    for k in KS:
        U = normal16(fmt, [1720, PATTERNS.index(name), k], (h.A.rows, k))
        X = normal16(fmt, [1721, PATTERNS.index(name), k], (h.A.cols, k))
        Uw, Xw = R.widen(fmt, U), R.widen(fmt, X)
        Uw[h.empty_rows], Xw[h.unref_cols] = 0.0, 0.0
        want = sddmm32(h, gpu, Uw, Xw)
        assert not np.isnan(want.view(np.float32)).any()
        for ld in lds(k):
            out = sddmm16(h, gpu, fmt, U, X, k, ld, ld, u_nan=h.empty_rows, x_nan=h.unref_cols)
            assert not np.isnan(out.view(np.float32)).any(), f"k = {k}, ld = {ld}: a NaN of the padding or of an unused row was read"
            bad = np.flatnonzero(out != want)
            assert bad.size == 0, f"k = {k}, ld = {ld}: {bad.size} nonzeros differ, first {bad[0]}"
        # the two leading dimensions need not agree
        fast, slow = lds(k)
        assert np.array_equal(sddmm16(h, gpu, fmt, U, X, k, fast, slow), want), f"k = {k}: ldu = {fast}, ldx = {slow}"


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("name", ("P1", "P2"))
def test_a_columns_bits_do_not_depend_on_k_or_its_position(handles, gpu, name, fmt):
    h = handles[name]
    X = normal16(fmt, [1730, PATTERNS.index(name)], (h.A.cols, 64))
    Y64 = spmm16(h, gpu, fmt, X, 64, 68, 68)[:, :64]
    for ld_x, ld_y in (lds(5), lds(5)[::-1], (8, 8)):
        Y5 = spmm16(h, gpu, fmt, X[:, :5], 5, ld_x, ld_y)
        assert np.array_equal(Y5[:, :5], Y64[:, :5]), f"k = 5 at ld {ld_x}, {ld_y} differs from the same columns at k = 64"
        assert (Y5[:, 5:] == POISON[fmt]).all()
    shift = (np.arange(64) + 7) % 64                       # column j of the second batch is column j + 7 of the first
    Ys = spmm16(h, gpu, fmt, X[:, shift], 64, 65, 68)[:, :64]
    assert np.array_equal(Ys, Y64[:, shift]), "a column's bits change with its position in the batch"
    sub = np.array([63, 2, 40, 17, 5, 5, 31])              # seven of them, one twice, in a batch of k = 7
    Y7 = spmm16(h, gpu, fmt, X[:, sub], 7, 12, 9)[:, :7]
    assert np.array_equal(Y7, Y64[:, sub]), "a column's bits change with the other columns of the batch"


# ---- rounding at the store, by construction ------------------------------------------------------------------------------------
def _construction(fmt):
    """(cases, table): a case is (vals value, X values of the row's nonzeros, the fp32 number Y must hold, or 'nan'); the
    table lists the distinct X values (X row i holds table[i] in every column; row 0 is the zero the long rows are filled with)."""
    if fmt == "bf16":
        sub = 2.0 ** -130                                   # a bf16 subnormal (the least is 2^-133)
        cases = [(1.0, [1.0, 2.0 ** -8], 1.0),                                  # a tie, to the even neighbour below
                 (1.0, [1.0, 2.0 ** -7, 2.0 ** -8], 1.0 + 2.0 ** -6),           # a tie, to the even neighbour above
                 (1.0, [sub], sub), (0.5, [2.0 ** -132], 2.0 ** -133),          # subnormals are kept
                 (0.5, [2.0 ** -133], 0.0),                                     # 2^-134: a tie between 0 and the least subnormal
                 (1.0, [1.0, 2.0 ** -8, 2.0 ** -20], 1.0 + 2.0 ** -7)]          # above the tie: up
    else:
        cases = [(1.0, [1.0, 2.0 ** -11], 1.0),
                 (1.0, [65504.0, 16.0], np.inf), (1.0, [65504.0, 8.0], 65504.0),
                 (0.5, [2.0 ** -24], 0.0), (0.75, [2.0 ** -24], 2.0 ** -24),
                 (1.0, [2.0 ** -15, 2.0 ** -24], 2.0 ** -15 + 2.0 ** -24),      # an fp16 subnormal is kept
                 (-1.0, [65504.0, 16.0], -np.inf)]
    cases += [(1.0, [1.0, "nan"], "nan"), (1.0, [3.0], 3.0)]
    table = [0.0]
    for _, xs, _ in cases:
        table += [x for x in xs if x not in table]
    return cases, table


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_rounding_happens_once_at_the_store(pkg, gpu, fmt):
    import torch
    cases, table = _construction(fmt)
    FILL = 600                                              # references to the zero row that make a row longer than 512
    cols, vals, want = [], [], []
    for long in (False, True):
        for v, xs, y in cases:
            ids = [table.index(x) for x in xs]
            if long:                                        # the first element in the first piece, the others in the last
                ids = ids[:1] + [0] * FILL + ids[1:] if len(ids) > 1 else [0] * FILL + ids
            cols.append(np.array(ids, np.int64))
            vals.append(np.full(len(ids), v, np.float32))
            want.append(y)
        if not long:
            cols.append(np.zeros(0, np.int64)), vals.append(np.zeros(0, np.float32)), want.append(0.0)      # an empty row: +0
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    assert (np.diff(rp) > 512).sum() == len(cases)
    d = [torch.from_numpy(a).to(gpu) for a in (rp, np.concatenate(cols).astype(np.int32), np.concatenate(vals))]
    A = pkg.capi.CsrMatrix.from_device(len(cols), len(table), *d)
    h = Handle(pkg, gpu, A, keep=d)
    assert f"long_rows={len(cases)}" in A.spmm_describe()
    column = np.array([np.nan if x == "nan" else x for x in table], np.float32)
    xbits = R.convert(fmt, column)
    assert np.array_equal(R.widen(fmt, xbits).view(np.uint32)[column == column], column.view(np.uint32)[column == column]), "exact in the format"
    wbits = R.convert(fmt, np.array([np.nan if y == "nan" else y for y in want], np.float32))
    try:
        for k in (4, 5):
            X = np.repeat(xbits[:, None], k, axis=1)
            Y32 = spmm32(h, gpu, R.widen(fmt, X))
            for ld in lds(k):
                Y = spmm16(h, gpu, fmt, X, k, ld, ld)
                for r, (w, y) in enumerate(zip(wbits, want)):
                    what = f"k = {k}, ld = {ld}, row {r} ({'long' if rp[r + 1] - rp[r] > 512 else 'short'}, wants {y})"
                    if y == "nan":
                        assert R.is_nan(fmt, Y[r, :k]).all(), what
                    else:
                        assert (Y[r, :k] == w).all(), f"{what}: {Y[r, 0]:#06x} != {w:#06x}"
                assert R.same(fmt, Y[:, :k], R.convert(fmt, Y32)) and (Y[:, k:] == POISON[fmt]).all()
    finally:
        A.close()


# ---- SDDMM: the operands trade places on the transposed pattern ----------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_sddmm16_symmetry_with_the_transposed_handle(handles, gpu, fmt):
    a, t = handles["P1"], handles["P1T"]
    perm = np.argsort(a.s.ci, kind="stable")
    for k in (5, 17, 64):
        U = normal16(fmt, [1740, k], (a.A.rows, k))
        X = normal16(fmt, [1741, k], (a.A.cols, k))
        fast, slow = lds(k)
        base = sddmm16(a, gpu, fmt, U, X, k, fast, fast)
        assert np.array_equal(sddmm16(t, gpu, fmt, X, U, k, slow, fast), base[perm]), f"k = {k}: T.sddmm(X, U) != A.sddmm(U, X)[perm]"


# ---- refusals launch nothing ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_name_the_function(pkg, handles, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    h = handles["P2"].A
    k, ld, fmt = 8, 12, "bf16"
    poison = POISON[fmt]
    X = dev16(gpu, fmt, np.full((h.cols + 1, ld), 0x3f80, np.uint16))
    U = dev16(gpu, fmt, np.full((h.rows + 1, ld), 0x3f80, np.uint16))
    Y = dev16(gpu, fmt, np.full((h.rows + 1, ld), poison, np.uint16))
    out = torch.full((h.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    stream = capi._stream_handle()
    s = handles["P2"].s
    d = [torch.from_numpy(a).to(gpu) for a in (s.rp, s.ci, handles["P2"].vals)]
    unplanned = capi.CsrMatrix.from_device(s.rows, s.cols, *d)

    def spmm(hh=h, dt=capi.ATTN_BF16, kk=k, x=X.data_ptr(), ldx=ld, y=Y.data_ptr(), ldy=ld):
        return "spmv_csr_spmm_16", lib.spmv_csr_spmm_16(hh._h, dt, kk, x, ldx, y, ldy, stream)

    def sddmm(hh=h, dt=capi.ATTN_BF16, kk=k, u=U.data_ptr(), ldu=ld, x=X.data_ptr(), ldx=ld, o=out.data_ptr()):
        return "spmv_csr_sddmm_16", lib.spmv_csr_sddmm_16(hh._h, dt, kk, u, ldu, x, ldx, o, stream)

    INV, NOPLAN = capi.ERR_INVALID, capi.ERR_NOT_PLANNED
    refused = [
        (spmm, dict(dt=0), INV), (spmm, dict(dt=3), INV), (sddmm, dict(dt=0), INV), (sddmm, dict(dt=3), INV),
        (spmm, dict(x=X.data_ptr() + 2), INV), (spmm, dict(y=Y.data_ptr() + 2), INV),                      # a base off by 2 bytes
        (sddmm, dict(u=U.data_ptr() + 2), INV), (sddmm, dict(x=X.data_ptr() + 2), INV),
        (spmm, dict(ldx=k - 1), INV), (spmm, dict(ldy=k - 1), INV), (sddmm, dict(ldu=k - 1), INV), (sddmm, dict(ldx=k - 1), INV),
        (spmm, dict(kk=0), INV), (spmm, dict(kk=65, ldx=68, ldy=68), INV), (sddmm, dict(kk=0), INV), (sddmm, dict(kk=65, ldu=68, ldx=68), INV),
        (spmm, dict(hh=unplanned), NOPLAN), (sddmm, dict(hh=unplanned), NOPLAN),
        (sddmm, dict(o=None), INV), (sddmm, dict(o=out.data_ptr() + 2), INV), (spmm, dict(x=None), INV), (spmm, dict(y=None), INV),
    ]
    try:
        for call, kw, status in refused:
            name, rc = call(**kw)
            msg = lib.spmv_last_error().decode()
            assert rc == status, f"{name}({kw}) returned {rc}: {msg}"
            assert msg.startswith(name), f"{name}({kw}): {msg}"
        torch.cuda.synchronize()
        assert (bits16(Y) == poison).all() and bool(torch.isnan(out).all()), "a refused call wrote to its output"
        # and the calls go through as they stand
        assert spmm()[1] == capi.OK and sddmm()[1] == capi.OK, lib.spmv_last_error()
        torch.cuda.synchronize()
        assert not R.is_nan(fmt, bits16(Y)[: h.rows, :k]).any() and not bool(torch.isnan(out).any())
    finally:
        unplanned.close()


# ---- graph capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_both_calls_are_graph_capturable(handles, gpu, fmt):
    import torch
    h = handles["P1"]
    k, ld = 12, 16
    first = [normal16(fmt, [1750, i], (n, k)) for i, n in enumerate((h.A.cols, h.A.rows))]
    spmm16(h, gpu, fmt, first[0], k, ld, ld), sddmm16(h, gpu, fmt, first[1], first[0], k, ld, ld)       # (the warm runs)
    X, U = dev16(gpu, fmt, padded(fmt, first[0], ld)), dev16(gpu, fmt, padded(fmt, first[1], ld))
    Y = dev16(gpu, fmt, np.full((h.A.rows, ld), POISON[fmt], np.uint16))
    out = torch.full((h.A.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream; the calls take the current stream)
        h.A.spmm(X[:, :k], Y[:, :k])
        h.A.sddmm(U[:, :k], X[:, :k], out)
    for seed in (1751, 1752):
        x, u = normal16(fmt, [seed, 0], (h.A.cols, k)), normal16(fmt, [seed, 1], (h.A.rows, k))
        X.copy_(dev16(gpu, fmt, padded(fmt, x, ld))), U.copy_(dev16(gpu, fmt, padded(fmt, u, ld)))
        Y.copy_(dev16(gpu, fmt, np.full((h.A.rows, ld), POISON[fmt], np.uint16))), out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits16(Y), spmm16(h, gpu, fmt, x, k, ld, ld)), f"replay with seed {seed}: Y differs from the direct call"
        assert np.array_equal(bits32(out), sddmm16(h, gpu, fmt, u, x, k, ld, ld)), f"replay with seed {seed}: out differs from the direct call"
