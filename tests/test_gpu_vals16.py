"""spmv_csr_run_vals16 on the device: y = A x with the values of A read from a bf16 or fp16 array, fp32 x, y and sums
(include/spmv_hip.h, "SpMV on 16-bit values").

The contract is bit for bit: y is what spmv_csr_run writes on a handle with the same pattern and plan and vals = the 16-bit
values widened exactly, so the order of every sum is the one tests/_tiled_order.py states.  The conversions are the integer
code of tests/_round16.py.  Every handle here is created with vals all NaN unless a test says otherwise: a result without a
NaN of its own shows the handle's values are never read.

  documented order   both formats x the two problems of tests/_tiled_order.py x 256, 512, 1024 threads x the six modes of
                     tests/test_gpu_tiled_rowsums.py (same knobs, same plan_describe assertions), every row compared as uint32,
                     a NaN equal to any NaN (an fp16 overflow to Inf can meet an Inf of the other sign in a row)
  the fp32 call      at 512 threads the bits of spmv_csr_run on the widened values and the same plan, in every mode (persist:
                     the persistent fp32 kernel against the one-shot 16-bit one); the unrounded values differ in some row
  live values        the array overwritten in place between two runs of one plan
  row block          y inside a larger array at 4-byte alignment with guard words, nnz == 0, rows == 0
  SPMV_AUTO          resolved to tiled: the bits of the SPMV_TILED call; resolved to panel: SPMV_ERR_VARIANT, y untouched
  refusals           every status of the header's list with its message prefix and y untouched
  graph capture      one captured run_vals16 replayed twice
"""
import numpy as np
import pytest

import _round16 as R
import _tiled_order as TO
from test_gpu_tiled_rowsums import MODES, _field

pytestmark = pytest.mark.gpu

KNOBS = ("SPMV_TILED_BLOCK", "SPMV_COL16", "SPMV_SORTED_FROM", "SPMV_PERSIST", "SPMV_MAXPASS", "SPMV_AUTOTUNE", "SPMV_BLOCKS")
NAME = "spmv_csr_run_vals16"


def _torch_dtype(fmt):
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]


def _to_device(fmt, bits, dev):
    """The uint16 bits of format fmt as a device tensor of that dtype."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(dev).view(_torch_dtype(fmt))


def _same(got, want):
    """Row for row as uint32, a NaN equal to any NaN: the rows that differ."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    return np.flatnonzero((g != w) & ~(np.isnan(got) & np.isnan(want)))


_va16, _want = {}, {}


def va16_of(fmt, case, block):
    if (fmt, case, block) not in _va16:
        _va16[fmt, case, block] = R.convert(fmt, TO.problem(case, block).va)
    return _va16[fmt, case, block]


def want_of(fmt, case, block, T):
    """y of the documented order on the widened values for chunks of T nonzeros, computed once."""
    if (fmt, case, block, T) not in _want:
        P = TO.problem(case, block)
        _want[fmt, case, block, T] = TO.tiled_spmv(P.rp, R.widen(fmt, va16_of(fmt, case, block)) * P.x[P.ci], T)[0]
    return _want[fmt, case, block, T]


@pytest.fixture(scope="module")
def device_problem(pkg, gpu):
    """The device copy of a problem, made once per (case, block): pattern, x, and vals all NaN."""
    import torch
    made = {}

    def get(case, block):
        if (case, block) not in made:
            P = TO.problem(case, block)
            d = [torch.from_numpy(a).to(gpu) for a in (P.rp, P.ci, P.x)]
            made[case, block] = (P, d + [torch.full((P.nnz,), float("nan"), dtype=torch.float32, device=gpu)])
        return made[case, block]
    return get


def _set_mode(monkeypatch, block, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPMV_TILED_BLOCK", str(block))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _planned(capi, P, d_rp, d_ci, d_va, vname, block, mode, says):
    """A handle planned in `mode`, with the plan_describe assertions of tests/test_gpu_tiled_rowsums.py: (A, plan, run_block)."""
    v = capi.VARIANTS[vname]
    A = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_va)
    try:
        A.plan(v)
        plan = A.plan_describe(v)
        run_block = _field(plan, "block")
        if vname == "tiled":
            assert run_block == block, plan
        chunks = _field(plan, "chunks")
        assert chunks == -(-P.nnz // (16 * run_block)), plan
        for name, how in says.items():
            n = _field(plan, name)
            assert (n == 0) if how == "none" else (n >= chunks - 1), (name, how, plan)
        if mode == "persist":
            assert _field(plan, "persist") == 1, plan
    except BaseException:
        A.close()
        raise
    return A, plan, run_block


# ---- 1. the documented order, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("case", TO.CASES)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_row_sums_on_16bit_values_have_the_documented_order(pkg, gpu, device_problem, monkeypatch, fmt, case, block, mode):
    import torch
    capi = pkg.capi
    vname, env, says = MODES[mode]
    _set_mode(monkeypatch, block, env)
    P, (d_rp, d_ci, d_x, d_nan) = device_problem(case, block)
    d_v16 = _to_device(fmt, va16_of(fmt, case, block), gpu)
    A, plan, run_block = _planned(capi, P, d_rp, d_ci, d_nan, vname, block, mode, says)
    try:
        y = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
        A.run_vals16(capi.VARIANTS[vname], d_v16, d_x, y)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
    finally:
        A.close()
    want = want_of(fmt, case, block, 16 * run_block)
    print(f"{fmt} {case} block={run_block} {mode}: {P.rows} rows, {P.nnz} nonzeros; {plan}")
    assert np.isnan(want).sum() < P.rows // 8, "the reference itself is mostly NaN: the problem checks nothing"
    bad = _same(got, want)
    assert bad.size == 0, (f"{bad.size} of {P.rows} rows differ from the documented order on the widened values; first rows {bad[:6]} "
                           f"of lengths {[P.lengths[b] for b in bad[:6]]}: {got[bad[:6]]} against {want[bad[:6]]}")


# ---- 2. equality with the fp32 call on the widened values ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", TO.CASES)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_bits_of_the_fp32_call_on_the_widened_values(pkg, gpu, device_problem, monkeypatch, fmt, case, mode):
    import torch
    capi = pkg.capi
    block = 512
    vname, env, says = MODES[mode]
    v = capi.VARIANTS[vname]
    _set_mode(monkeypatch, block, env)
    P, (d_rp, d_ci, d_x, d_nan) = device_problem(case, block)
    bits = va16_of(fmt, case, block)
    d_v16 = _to_device(fmt, bits, gpu)
    d_wide = torch.from_numpy(R.widen(fmt, bits)).to(gpu)
    d_va = torch.from_numpy(P.va).to(gpu)
    A, plan, _ = _planned(capi, P, d_rp, d_ci, d_nan, vname, block, mode, says)
    B, plan_b, _ = _planned(capi, P, d_rp, d_ci, d_wide, vname, block, mode, says)
    Cm, _, _ = _planned(capi, P, d_rp, d_ci, d_va, vname, block, mode, says)
    try:
        assert plan_b == plan
        ys = [torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu) for _ in range(3)]
        A.run_vals16(v, d_v16, d_x, ys[0])
        B.run(v, d_x, ys[1])
        Cm.run(v, d_x, ys[2])
        torch.cuda.synchronize()
        y16, y32, yraw = (y.cpu().numpy() for y in ys)
    finally:
        A.close(), B.close(), Cm.close()
    bad = _same(y16, y32)
    assert bad.size == 0, f"{bad.size} rows differ from spmv_csr_run on the widened values; first {bad[:6]}: {y16[bad[:6]]} against {y32[bad[:6]]}"
    assert _same(y16, yraw).size > 0, "the unrounded values give the same bits: the problem cannot tell the values apart"


# ---- 3. live values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_values_are_read_live(pkg, gpu, device_problem, monkeypatch, fmt):
    import torch
    capi = pkg.capi
    _set_mode(monkeypatch, 256, {})
    P, (d_rp, d_ci, d_x, d_nan) = device_problem("lengths", 256)
    d_v16 = _to_device(fmt, va16_of(fmt, "lengths", 256), gpu)
    second = R.convert(fmt, (P.va * np.float32(0.75) + np.float32(0.001)).astype(np.float32))
    A = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_nan)
    try:
        A.plan(capi.TILED)
        y = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
        A.run_vals16(capi.TILED, d_v16, d_x, y)
        torch.cuda.synchronize()
        first = y.cpu().numpy()
        d_v16.copy_(_to_device(fmt, second, gpu))           # in place: the same address, no new plan
        y.fill_(float("nan"))
        A.run_vals16(capi.TILED, d_v16, d_x, y)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
    finally:
        A.close()
    assert _same(first, want_of(fmt, "lengths", 256, 4096)).size == 0
    want = TO.tiled_spmv(P.rp, R.widen(fmt, second) * P.x[P.ci], 4096)[0]
    assert _same(got, want).size == 0 and _same(got, first).size > 0


# ---- 4. row block, no nonzeros, no rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", ["tiled", "adaptive"])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_y_inside_a_larger_array_with_guards(pkg, gpu, device_problem, monkeypatch, fmt, vname):
    import torch
    capi = pkg.capi
    _set_mode(monkeypatch, 256, {})
    P, (d_rp, d_ci, d_x, d_nan) = device_problem("lengths", 256)
    d_v16 = _to_device(fmt, va16_of(fmt, "lengths", 256), gpu)
    v = capi.VARIANTS[vname]
    guard = np.float32(-12345.5)
    big = torch.full((P.rows + 8,), float(guard), dtype=torch.float32, device=gpu)
    y = big[3:3 + P.rows]
    assert y.data_ptr() % 16 == 12                          # 4-byte alignment only
    A = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_nan)
    try:
        A.plan(v)
        A.run_vals16(v, d_v16, d_x, y)
        torch.cuda.synchronize()
        out = big.cpu().numpy()
    finally:
        A.close()
    assert np.all(out[:3] == guard) and np.all(out[3 + P.rows:] == guard), "a guard word beside y was written"
    assert _same(out[3:3 + P.rows], want_of(fmt, "lengths", 256, 4096)).size == 0


@pytest.mark.parametrize("rows,cols", [(7, 9), (0, 10)])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_no_nonzeros_and_no_rows(pkg, gpu, fmt, rows, cols):
    import torch
    capi = pkg.capi
    d_rp = torch.zeros(rows + 1, dtype=torch.int32, device=gpu)
    d_ci = torch.zeros(1, dtype=torch.int32, device=gpu)[:0]
    d_va = torch.zeros(1, dtype=torch.float32, device=gpu)[:0]
    d_v16 = torch.zeros(8, dtype=_torch_dtype(fmt), device=gpu)[:0]
    x = torch.ones(max(cols, 4), dtype=torch.float32, device=gpu)
    y = torch.full((max(rows, 1),), float("nan"), dtype=torch.float32, device=gpu)
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    try:
        for v in (capi.TILED, capi.ADAPTIVE):
            A.plan(v)
            y.fill_(float("nan"))
            A.run_vals16(v, d_v16, x, y)
            # nnz == 0: a null array is no refusal either
            assert capi.lib().spmv_csr_run_vals16(A._h, v, capi.ATTN_BF16, None, x.data_ptr(), y.data_ptr(), None) == capi.OK
            torch.cuda.synchronize()
            if rows:
                assert torch.equal(y[:rows].view(torch.int32), torch.zeros(rows, dtype=torch.int32, device=gpu))
            else:
                assert bool(torch.isnan(y).all())
    finally:
        A.close()


# ---- 5. SPMV_AUTO -------------------------------------------------------------------------------------------------------------------
def _random_csr(rows, cols, per_row, band, seed):
    rng = np.random.default_rng(seed)
    rp = (np.arange(rows + 1, dtype=np.int64) * per_row).astype(np.int32)
    if band:
        lo = np.minimum(np.maximum(np.arange(rows, dtype=np.int64) * cols // rows - band // 2, 0), cols - band)
        ci = lo[:, None] + rng.integers(0, band, (rows, per_row))
    else:
        ci = rng.integers(0, cols, (rows, per_row))
    ci = np.sort(ci, axis=1).astype(np.int32).reshape(-1)
    return rp, ci, TO.general_values(rows * per_row, rng), TO.general_values(cols, rng)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_auto_resolved_to_tiled_runs_with_the_bits_of_tiled(pkg, gpu, monkeypatch, fmt):
    import torch
    capi = pkg.capi
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rows, cols = 16384, 65536
    rp, ci, va, x = _random_csr(rows, cols, 16, 8192, 5)
    d_rp, d_ci, d_x = (torch.from_numpy(a).to(gpu) for a in (rp, ci, x))
    d_nan = torch.full((len(ci),), float("nan"), dtype=torch.float32, device=gpu)
    bits = R.convert(fmt, va)
    d_v16 = _to_device(fmt, bits, gpu)
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_nan)
    try:
        A.plan(capi.AUTO)
        assert A.plan_params(capi.AUTO)[0] == capi.TILED, A.plan_describe(capi.AUTO)
        A.plan(capi.TILED)
        ya, yt = (torch.full((rows,), float("nan"), dtype=torch.float32, device=gpu) for _ in range(2))
        A.run_vals16(capi.AUTO, d_v16, d_x, ya)
        A.run_vals16(capi.TILED, d_v16, d_x, yt)
        torch.cuda.synchronize()
        got_a, got_t = ya.cpu().numpy(), yt.cpu().numpy()
    finally:
        A.close()
    assert not np.isnan(got_t).any() and np.array_equal(got_a.view(np.uint32), got_t.view(np.uint32))
    # and they are the product: each row against the fp64 sum of the widened values' products, relative to the row's magnitude
    prod = R.widen(fmt, bits).astype(np.float64) * x[ci].astype(np.float64)
    row_of = np.repeat(np.arange(rows), 16)
    y64, mag = np.bincount(row_of, weights=prod, minlength=rows), np.bincount(row_of, weights=np.abs(prod), minlength=rows)
    assert np.all(np.abs(got_t - y64) <= 1e-5 * mag)


# The smallest matrix of uniform columns that SPMV_AUTO's rule hands to the panel family: x of 4 MiB (2^20 columns: "x fills one
# XCD's L2"), nothing staged or sorted by TILED (a chunk's columns span all of x), too few rows for the sorted blocks and an x
# below the binned layouts' 8 MiB: the panel sweep.  tests/test_gpu_plans.py shows the rule at 2Mi x 2Mi.
PANEL_ROWS, PANEL_COLS = 8192, 1 << 20


def test_auto_resolved_to_panel_is_refused(pkg, gpu, monkeypatch):
    import torch
    capi = pkg.capi
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rp, ci, va, x = _random_csr(PANEL_ROWS, PANEL_COLS, 16, 0, 6)
    d_rp, d_ci, d_va, d_x = (torch.from_numpy(a).to(gpu) for a in (rp, ci, va, x))
    d_v16 = _to_device("bf16", R.convert("bf16", va), gpu)
    A = capi.CsrMatrix.from_device(PANEL_ROWS, PANEL_COLS, d_rp, d_ci, d_va)
    try:
        A.plan(capi.AUTO)
        assert A.plan_params(capi.AUTO)[0] == capi.PANEL, A.plan_describe(capi.AUTO)
        y = torch.full((PANEL_ROWS,), float("nan"), dtype=torch.float32, device=gpu)
        with pytest.raises(capi.SpmvError) as e:
            A.run_vals16(capi.AUTO, d_v16, d_x, y)
        torch.cuda.synchronize()
        assert e.value.status == capi.ERR_VARIANT
        msg = str(e.value)
        assert NAME + ":" in msg and "SPMV_AUTO resolved to panel" in msg, msg
        assert bool(torch.isnan(y).all()), "a refused call wrote y"
    finally:
        A.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, gpu, device_problem, monkeypatch):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    _set_mode(monkeypatch, 256, {})
    P, (d_rp, d_ci, d_x, d_nan) = device_problem("lengths", 256)
    d_v16 = _to_device("bf16", va16_of("bf16", "lengths", 256), gpu)
    pad = torch.zeros(P.nnz + 8, dtype=torch.bfloat16, device=gpu)
    xpad = torch.zeros(P.cols + 8, dtype=torch.float32, device=gpu)
    y = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
    A = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_nan)
    U = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_nan)         # never planned
    BF = capi.ATTN_BF16
    v16, px, py = d_v16.data_ptr(), d_x.data_ptr(), y.data_ptr()
    assert v16 % 16 == 0 and px % 16 == 0

    def refused(status, fragment, h, variant, dtype, a, b, c):
        assert lib.spmv_csr_run_vals16(h, variant, dtype, a, b, c, None) == status, fragment
        msg = lib.spmv_last_error().decode()
        assert fragment in msg, msg
        if status == capi.ERR_INVALID:
            assert msg.startswith(NAME + ":"), msg
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()), f"{fragment}: a refused call wrote y"

    try:
        A.plan(capi.TILED)
        A.plan(capi.ADAPTIVE)
        T, INV = capi.TILED, capi.ERR_INVALID
        refused(INV, "null handle", None, T, BF, v16, px, py)
        for dtype in (capi.ATTN_FP32, 3, -1, 16):
            refused(INV, "dtype", A._h, T, dtype, v16, px, py)
        refused(INV, "null", A._h, T, BF, None, px, py)
        refused(INV, "null", A._h, T, BF, v16, None, py)
        refused(INV, "null", A._h, T, BF, v16, px, None)
        for off in (2, 4, 8):                                   # bytes: vals16 is read with 8-byte loads from 16-byte aligned chunks
            refused(INV, "16-byte aligned", A._h, T, BF, pad.data_ptr() + off, px, py)
        for off in (4, 8):
            refused(INV, "16-byte aligned", A._h, T, BF, v16, xpad.data_ptr() + off, py)
        if torch.cuda.device_count() >= 2:                      # another current device than the handle's
            with torch.cuda.device(1):
                refused(INV, "device", A._h, T, BF, v16, px, py)
        for name in ("scalar", "wave_pipe", "panel", "wave", "vector", "xskip"):
            refused(capi.ERR_VARIANT, NAME + ":", A._h, capi.ALL_VARIANTS[name], BF, v16, px, py)
            assert name in lib.spmv_last_error().decode()
        refused(capi.ERR_VARIANT, NAME + ":", A._h, 77, BF, v16, px, py)
        for v in (capi.TILED, capi.ADAPTIVE, capi.AUTO):
            refused(capi.ERR_NOT_PLANNED, "before spmv_csr_plan", U._h, v, BF, v16, px, py)
        # the method's own checks come before the library
        with pytest.raises(ValueError, match="run_vals16"):
            A.run_vals16(T, d_v16[:-1], d_x, y)
        with pytest.raises(ValueError, match="run_vals16"):
            A.run_vals16(T, d_v16.to(torch.float32), d_x, y)
        with pytest.raises(ValueError, match="run_vals16"):
            A.run_vals16(T, torch.zeros(2 * P.nnz, dtype=torch.bfloat16, device=gpu)[::2], d_x, y)     # not contiguous
        # and after all of them the handle still runs
        A.run_vals16(T, d_v16, d_x, y)
        torch.cuda.synchronize()
        assert _same(y.cpu().numpy(), want_of("bf16", "lengths", 256, 4096)).size == 0
    finally:
        A.close(), U.close()


# ---- 7. graph capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_one_captured_run_replays_with_the_eager_bits(pkg, gpu, device_problem, monkeypatch, fmt):
    import torch
    capi = pkg.capi
    _set_mode(monkeypatch, 256, {})
    P, (d_rp, d_ci, d_x, d_nan) = device_problem("lengths", 256)
    d_v16 = _to_device(fmt, va16_of(fmt, "lengths", 256), gpu)
    A = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_nan)
    try:
        A.plan(capi.TILED)
        eager = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
        A.run_vals16(capi.TILED, d_v16, d_x, eager)
        torch.cuda.synchronize()
        y = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                               # one branch: a single call on the capture stream
            A.run_vals16(capi.TILED, d_v16, d_x, y)
        for _ in range(2):
            y.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y.view(torch.int32), eager.view(torch.int32))
        del g
    finally:
        A.close()
    assert _same(eager.cpu().numpy(), want_of(fmt, "lengths", 256, 4096)).size == 0
