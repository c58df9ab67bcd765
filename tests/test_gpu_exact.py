"""Every SpMV path against an answer that needs no tolerance (inputs and expectations: tests/_exact.py).

Integer values and x (rows scaled by 2^e, e in [-40, 40]) make every fp32 sum exact in any order, so each variant and
plan path must return the int64 expectation bit for bit: a dropped, doubled or misplaced product, a carry added to the
wrong row or a flushed subnormal cannot hide under the 1e-5 * sum|terms| bound of _util.assert_close_to_oracle.  The
other properties give per-row answers that do not depend on the order either:

  exact      integer data, rows scaled by 2^e                     y bit-identical to the int64 expectation
  subnormal  vals k 2^-75, x m 2^-74 (products multiples of 2^-149) y bit-identical (no path may flush subnormals)
  poison     columns dilated c -> 2c+1; every x entry no nonzero refers to (x[0], x[cols-1], every even one) NaN,
             then +Inf, then -Inf                                  y bit-identical to the undilated expectation
  nonfinite  dilated, NaN poison, and a few referenced x and vals +-Inf / NaN, Inf values under x = 0 (Inf * 0), rows
             holding +Inf and -Inf (short, longest, across chunk boundaries)
                                                                   per row the class (NaN, +Inf, -Inf, finite) of
                                                                   the fp64 oracle; finite rows exact.  SPMV_XSKIP
                                                                   leaves out the terms whose x is +-0.
  unsorted   columns shuffled inside rows, ~1/8 duplicates          y bit-identical (every path but SPMV_XSKIP)

Signed zeros compare equal (an exact zero sum is +0 or -0 depending on whether a kernel seeds its accumulator with +0).
Every run is made twice, into y filled with NaN and into y filled with a finite sentinel; the two must agree bit for
bit, so a row a kernel leaves unwritten fails even where the expected value is NaN.  y is a view one float past a 16-byte
boundary inside a buffer with 4096 guard floats on either side, which every run must leave untouched.

Paths (PATHS below; a fresh handle per path, the knobs set in the environment for its plan and its runs; each path also
checks that spmv_csr_plan_describe reports the plan it asked for):
  scalar                        SPMV_SCALAR: k_scalar (mean row <= 64), k_scalar_long (mean > 64: the long-row matrices)
  wave                          SPMV_WAVE: the bundles (mean <= 32) or a wavefront per row
  wave/per_row                  SPMV_WAVE_PER_ROW=1: a wavefront per row on every matrix
  wave_pipe/block512, /block1024  SPMV_WAVE_BLOCK: rows per window block of SPMV_WAVE_PIPE
  wave_pipe/col16_off           SPMV_WAVE_COL16=0: 32-bit columns in the windows and the pieces
  vector/w2 .. /w32             spmv_csr_plan_set(SPMV_VECTOR, lanes per row 2, 4, 8, 16, 32)
  adaptive/b256                 spmv_csr_plan_set(SPMV_ADAPTIVE, 256 threads): the only size its kernel is built for;
                                512 and 1024 are refused (test_knobs_reach_their_kernels)
  tiled/b256|b512|b1024_c16|_c32  spmv_csr_plan_set(SPMV_TILED, block, 8 passes, 16-bit columns on | off)
  tiled/sorted_from1            SPMV_SORTED_FROM=1 (and SPMV_BLOCKS=0, which would take most chunks of a narrow band
                                first): every windowed chunk gathers in column order (k_sorted)
  tiled/blocks0, tiled/blocks1  SPMV_BLOCKS=0 | 1: the block lists of 256-column blocks off | on
  tiled/persist                 SPMV_PERSIST=1: resident workgroups walk the chunks
  tiled/maxpass1                spmv_csr_plan_set(SPMV_TILED, 512, 1 pass): chunks with wider spans are not staged
  panel/m1_step4, m1_step8      params[6] = 1 (panel sweep, x through L2), SPMV_PANEL_STEP=4 | 8
  panel/m2                      params[6] = 2 (the sweep with x panels staged in LDS)
  panel/m3_r4096_w4|_w8, _r8192_w4  params[6] = 3 (sorted blocks), rows per block x waves per workgroup; 8192 x 8 does
                                not fit LDS and is refused (test_knobs_reach_their_kernels)
  panel/m4_wide0, m4_wide1      params[6] = 4 (binned), SPMV_BINNED_WIDE=0 | 1
  panel/m5_r4096|8192|16384     params[6] = 5 (binned, products stored in bin order), rows per bin
  panel/m5_fill1                params[6] = 5, SPMV_BS_FILL=1 (the one-pass fill)
  xskip                         SPMV_XSKIP: its "dense-ish" refusal (and "duplicate" on rows with duplicates) accepted
  auto                          SPMV_AUTO

The dense side (spmv_dense_gemv modes 0-3, spmv_asp_retile + spmv_asp_gemv_ws, tcsr and the WSP / AWSP / AWSP_REF
bitmaps) gets integer A and x (finite values only) at shapes that are not multiples of the tiles and slabs.
"""
import numpy as np
import pytest

import _exact as E
from _util import assert_close_to_oracle

SENTINEL = np.float32(-1.2345e30)
GUARD, GUARD_N = np.float32(3.0e35), 4096
KNOBS = ("SPMV_AUTOTUNE", "SPMV_TILED_BLOCK", "SPMV_MAXPASS", "SPMV_COL16", "SPMV_SORTED_FROM", "SPMV_BLOCKS",
         "SPMV_PERSIST", "SPMV_WAVE_BLOCK", "SPMV_WAVE_COL16", "SPMV_WAVE_PER_ROW", "SPMV_PANEL_STEP",
         "SPMV_BINNED_WIDE", "SPMV_BS_FILL", "SPMV_AUTO_SORTED_BLOCKS", "SPMV_AUTO_BINNED", "SPMV_PANEL_SORTED",
         "SPMV_PANEL_LDS", "SPMV_PANEL_BITS", "SPMV_PANEL_WAVES", "SPMV_BINNED_SPLITS", "SPMV_BS_BINS",
         "SPMV_CHECK_VALUES", "SPMV_PLAN_COST")

# (label, variant, environment, spmv_csr_plan_set params or None for spmv_csr_plan, what spmv_csr_plan_describe must say)
S, WV, WP, VE, AD, TI, PA, AU, XS = range(9)
PATHS = (
    [("scalar", S, {}, None, {}),
     ("wave", WV, {}, None, {}),
     ("wave/per_row", WV, {"SPMV_WAVE_PER_ROW": "1"}, None, {}),
     ("wave_pipe/block512", WP, {"SPMV_WAVE_BLOCK": "512"}, None, {"block_rows": "512"}),
     ("wave_pipe/block1024", WP, {"SPMV_WAVE_BLOCK": "1024"}, None, {"block_rows": "1024"}),
     ("wave_pipe/col16_off", WP, {"SPMV_WAVE_COL16": "0"}, None, {"col16": "0"})]
    + [(f"vector/w{w}", VE, {}, [VE, w, 0, 0, 0, 0, 0, 0], {"lanes_per_row": str(w)}) for w in (2, 4, 8, 16, 32)]
    + [("adaptive/b256", AD, {}, [AD, 256, 0, 0, 0, 0, 0, 0], {"block": "256"})]
    + [(f"tiled/b{b}_c{16 if c else 32}", TI, {}, [TI, b, 8, c, 0, 0, 0, 0], {"block": str(b), "maxpass": "8"} if c else
        {"block": str(b), "maxpass": "8", "col16_chunks": "0"}) for b in (256, 512, 1024) for c in (1, 0)]
    + [("tiled/sorted_from1", TI, {"SPMV_SORTED_FROM": "1", "SPMV_BLOCKS": "0"}, None, {}),
       ("tiled/blocks0", TI, {"SPMV_BLOCKS": "0"}, None, {"block_list_chunks": "0"}),
       ("tiled/blocks1", TI, {"SPMV_BLOCKS": "1"}, None, {}),
       ("tiled/persist", TI, {"SPMV_PERSIST": "1"}, None, {"persist": "1"}),
       ("tiled/maxpass1", TI, {}, [TI, 512, 1, 1, 0, 0, 0, 0], {"block": "512", "maxpass": "1"})]
    + [(f"panel/m1_step{st}", PA, {"SPMV_PANEL_STEP": str(st)}, [PA, 0, 0, 0, 0, 0, 1, 0],
        {"x_panels_in": "L2", "nonzeros_per_step": str(256 * st)}) for st in (4, 8)]
    + [("panel/m2", PA, {}, [PA, 0, 0, 0, 0, 0, 2, 0], {"x_panels_in": "LDS"})]
    + [(f"panel/m3_r{r}_w{w}", PA, {}, [PA, 0, 0, 0, r, w, 3, 0], {"rows_per_block": str(r), "wavefronts": str(w)})
       for r, w in ((4096, 4), (4096, 8), (8192, 4))]
    + [(f"panel/m4_wide{wd}", PA, {"SPMV_BINNED_WIDE": str(wd)}, [PA, 0, 0, 0, 0, 0, 4, 0],
        {"binned": None, "products_per_lane": "4" if wd else "2"}) for wd in (0, 1)]
    + [(f"panel/m5_r{r}", PA, {}, [PA, 0, 0, 0, r, 0, 5, 0], {"scattered_products": None, "rows_per_bin": str(r)})
       for r in (4096, 8192, 16384)]
    + [("panel/m5_fill1", PA, {"SPMV_BS_FILL": "1"}, [PA, 0, 0, 0, 0, 0, 5, 0], {"scattered_products": None}),
       ("xskip", XS, {}, None, {"output_blocks": None}),
       ("auto", AU, {}, None, {})]
)
KINDS = ("exact", "subnormal", "poison", "nonfinite", "unsorted")


def _struct(name, pkg, oracle):
    return E.structure(name, pkg, oracle)


def _has_duplicates(s):
    same = s.ci[1:] == s.ci[:-1]
    return bool(np.any(same & (s.row_of[1:] == s.row_of[:-1]))) if s.nnz > 1 else False


def _mismatches(y, exp, y64=None, limit=4):
    """Rows where y differs from the expectation: bits of the finite rows (+-0 folded), class of the others."""
    fin = np.ones(len(y), bool) if y64 is None else np.isfinite(y64)
    a, b = (y[fin] + np.float32(0)).view(np.uint32), (exp[fin] + np.float32(0)).view(np.uint32)
    bad = np.flatnonzero(fin)[np.flatnonzero(a != b)]
    out = []
    if bad.size:
        out.append(f"{bad.size} finite rows differ, first {bad[:limit].tolist()}: got {y[bad[:limit]].tolist()}, "
                   f"want {exp[bad[:limit]].tolist()}")
    if y64 is not None:
        for what, f in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
            c = np.flatnonzero(f(y) != f(y64))
            if c.size:
                out.append(f"{c.size} rows disagree on {what}, first {c[:limit].tolist()}: got {y[c[:limit]].tolist()}, "
                           f"oracle {y64[c[:limit]].tolist()}")
    return "; ".join(out)


class _Dev:
    """One matrix on the device (borrowed by a fresh handle per path) and the x vectors to run it with."""

    def __init__(self, gpu, s, vals):
        import torch
        self.s = s
        self.d_rp = torch.from_numpy(s.rp).to(gpu)
        self.d_ci = torch.from_numpy(s.ci).to(gpu)
        self.d_va = torch.from_numpy(np.ascontiguousarray(vals, np.float32)).to(gpu)
        # y: a view one float past a 16-byte boundary (spmv_csr_run asks 4-byte alignment of y only), GUARD_N guard floats
        # on either side: a store outside y[0, rows), or a vector store that assumes alignment, shows in the guards
        n = max(s.rows, 1)
        self.buf = torch.full((GUARD_N + 1 + n + GUARD_N,), float(GUARD), dtype=torch.float32, device=gpu)
        self.d_y = self.buf[GUARD_N + 1:GUARD_N + 1 + n]
        assert self.d_y.data_ptr() % 16 == 4
        self.gpu = gpu
        self.cases = []          # (label, d_x, expected, oracle y64 or None, XSKIP's (expected, y64) or None)

    def add(self, label, x, expected, y64=None, xskip=None):
        import torch
        d_x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.gpu)
        if d_x.numel() == 0:
            d_x = torch.zeros(4, dtype=torch.float32, device=self.gpu)
        self.cases.append((label, d_x, expected, y64, xskip))

    def run_twice(self, capi, A, v, d_x):
        import torch
        ys = []
        for fill in (float("nan"), float(SENTINEL)):
            self.d_y.fill_(fill)
            A.run(v, d_x, self.d_y)
            torch.cuda.synchronize()
            ys.append(self.d_y[:self.s.rows].cpu().numpy())
            lo, hi = self.buf[:GUARD_N + 1], self.buf[GUARD_N + 1 + self.d_y.numel():]
            assert bool((lo == float(GUARD)).all()) and bool((hi == float(GUARD)).all()), \
                f"{capi.lib().spmv_variant_name(v).decode()}: a run wrote outside y[0, rows)"
        return ys


def _run_paths(pkg, monkeypatch, devs, skip_xskip=False):
    """Every path of PATHS on every device matrix in devs; returns the list of failures (all paths run first)."""
    capi = pkg.capi
    failures = []
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for label, v, env, params, want in PATHS:
        if v == XS and skip_xskip:
            continue
        with monkeypatch.context() as mp:
            for k, val in env.items():
                mp.setenv(k, val)
            for dev in devs:
                A = capi.CsrMatrix.from_device(dev.s.rows, dev.s.cols, dev.d_rp, dev.d_ci, dev.d_va)
                try:
                    try:
                        if params is None:
                            A.plan(v)
                        else:
                            A.plan_set(v, params)
                    except capi.SpmvError as e:
                        msg = str(e)
                        if v == XS and ("dense-ish" in msg or ("duplicate" in msg and _has_duplicates(dev.s))):
                            continue
                        failures.append(f"{label}: plan refused: {msg}")
                        continue
                    bad = _describe_mismatch(A.plan_describe(v), want) if dev.s.nnz else ""
                    if bad:
                        failures.append(f"{label}: plan is not the one asked for: {bad}")
                    for case, d_x, exp, y64, xs in dev.cases:
                        if v == XS and xs is not None:
                            exp, y64 = xs
                        y0, y1 = dev.run_twice(capi, A, v, d_x)
                        if not np.array_equal(y0.view(np.uint32), y1.view(np.uint32)):
                            rows = np.flatnonzero(y0.view(np.uint32) != y1.view(np.uint32))
                            failures.append(f"{label}/{case}: {rows.size} rows unwritten, first {rows[:4].tolist()}")
                            continue
                        bad = _mismatches(y0, exp, y64)
                        if bad:
                            failures.append(f"{label}/{case}: {bad}")
                finally:
                    A.close()
    return failures


def _describe_fields(desc):
    """spmv_csr_plan_describe as {key: value}; bare words ("binned", "scattered_products") map to None, and so does a
    wanted key whose value does not matter."""
    return {tok.split("=", 1)[0]: (tok.split("=", 1)[1] if "=" in tok else None) for tok in desc.split()}


def _describe_mismatch(desc, want):
    got = _describe_fields(desc)
    if got.get("blocks") == "0":          # the wave plan of a matrix of mean row > 32: a wavefront per row, no row blocks
        return ""
    bad = [f"{k}={v}" for k, v in want.items() if k not in got or (v is not None and got[k] != v)]
    return f"{bad} not in '{desc}'" if bad else ""


def _filtered_csr(s, keep):
    """The CSR of s without the terms where keep is False (for the SPMV_XSKIP expectation)."""
    cnt = np.concatenate([[0], np.cumsum(keep)])
    rp = cnt[s.rp.astype(np.int64)].astype(np.int32)
    return rp, s.ci[keep]


# ---- the GPU runs ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", E.MATRICES)
def test_every_path_exact(pkg, oracle, gpu, monkeypatch, name, kind):
    s = _struct(name, pkg, oracle)
    ex = E.Exact(s, name)
    if kind == "exact":
        dev = _Dev(gpu, s, ex.vals())
        dev.add("int", ex.x(), ex.expected())
    elif kind == "subnormal":
        dev = _Dev(gpu, s, ex.sub_vals())
        dev.add("subnormal", ex.sub_x(), ex.sub_expected())
    elif kind == "poison":
        dev = _Dev(gpu, E.dilate(s), ex.vals())
        want = ex.expected()
        for tag, p in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            dev.add(f"poison_{tag}", E.dilated_x(ex.x(), p), want)
    elif kind == "nonfinite":
        vals, x, m_int, finite_rows = E.nonfinite(ex, name)
        sd = E.dilate(s)
        xd = E.dilated_x(x, np.nan)
        y64, _ = oracle.spmv_f64(sd.rp, sd.ci, vals, xd)
        assert np.array_equal(np.isfinite(y64), finite_rows), "the builder's finite rows disagree with the oracle"
        want = ex.expected(ex.int_sums(m=m_int))
        keep = x[s.ci] != 0
        rp_k, ci_k = _filtered_csr(sd, keep)
        y64_k, _ = oracle.spmv_f64(rp_k, ci_k, vals[keep], xd)
        want_k = ex.expected(ex.int_sums(m=m_int, keep=keep))
        dev = _Dev(gpu, sd, vals)
        dev.add("nonfinite", xd, want, y64, xskip=(want_k, y64_k))
    else:
        su, _ = E.shuffled(s, name)
        exu = E.Exact(su, name + "/unsorted")
        dev = _Dev(gpu, su, exu.vals())
        dev.add("unsorted_dup", exu.x(), exu.expected())
    failures = _run_paths(pkg, monkeypatch, [dev], skip_xskip=(kind == "unsorted"))
    assert not failures, f"{name}/{kind}: {len(failures)} failing path(s):\n" + "\n".join(failures)


@pytest.mark.gpu
def test_knobs_reach_their_kernels(pkg, oracle, gpu, monkeypatch):
    """The knobs above change the plan where they can: on the headline matrix sorted chunks, 16-bit columns and staged
    windows appear, SPMV_SORTED_FROM=1 sorts, a one-pass budget leaves chunks unstaged; power-law rows span chunks and
    leave SPMV_WAVE_PIPE long rows in pieces; SPMV_BLOCKS turns the block lists on and off.  The sizes the kernels are
    not built for are refused, not run."""
    import torch
    capi = pkg.capi
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def describe(name, v, params=None, **env):
        s = _struct(name, pkg, oracle)
        d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
        d_va = torch.ones(max(s.nnz, 1), dtype=torch.float32, device=gpu)
        A = capi.CsrMatrix.from_device(s.rows, s.cols, d_rp, d_ci, d_va)
        with monkeypatch.context() as mp:
            for k, val in env.items():
                mp.setenv(k, val)
            if params is None:
                A.plan(v)
            else:
                A.plan_set(v, params)
        got = {k: (int(x) if x is not None and x.lstrip("-").isdigit() else x)
               for k, x in _describe_fields(A.plan_describe(v)).items()}
        A.close()
        return got

    for b in (256, 512, 1024):
        d = describe("c4_band4096", TI, [TI, b, 8, 1, 0, 0, 0, 0])
        assert d["col16_chunks"] > 0 and d["staged_single"] + d["staged_full"] > 0, d
        assert describe("c4_band4096", TI, [TI, b, 8, 0, 0, 0, 0, 0])["col16_chunks"] == 0
    d = describe("c4_band4096", TI, SPMV_SORTED_FROM="1", SPMV_BLOCKS="0")
    assert d["sorted_chunks"] > 0.9 * d["chunks"], d
    assert describe("c4_band4096", TI, SPMV_SORTED_FROM="0")["sorted_chunks"] == 0
    d = describe("wide_window", TI, [TI, 512, 1, 1, 0, 0, 0, 0])
    assert d["staged_single"] + d["staged_full"] < d["chunks"], d
    assert describe("c3_powerlaw", AD, [AD, 256, 0, 0, 0, 0, 0, 0])["spanning_rows"] > 0
    d = describe("wave_pipe_thresholds", WP, SPMV_WAVE_BLOCK="512")
    assert d["long_rows"] == 5 and d["pieces"] == 1 + 1 + 2 + 2 + 5, d
    # chunks of the headline band that would gather in column order take a block list first, unless SPMV_BLOCKS=0
    assert describe("c4_band4096", TI, SPMV_SORTED_FROM="1", SPMV_BLOCKS="1")["block_list_chunks"] > 0
    assert describe("c4_band4096", TI, SPMV_PERSIST="1")["persist"] == 1
    for params in ([AD, 512, 0, 0, 0, 0, 0, 0], [AD, 1024, 0, 0, 0, 0, 0, 0], [PA, 0, 0, 0, 8192, 8, 3, 0]):
        with pytest.raises(capi.SpmvError) as e:
            describe("c2_uniform", params[0], params)
        assert e.value.status == capi.ERR_INVALID, params


# ---- the CPU side: the oracle reproduces the expectation; the tolerance misses what these tests catch ----------------
@pytest.mark.parametrize("name", E.MATRICES)
def test_oracle_reproduces_the_exact_expectation(pkg, oracle, name):
    s = _struct(name, pkg, oracle)
    ex = E.Exact(s, name)
    for what, vals, x, want in (("int", ex.vals(), ex.x(), ex.expected()),
                                ("subnormal", ex.sub_vals(), ex.sub_x(), ex.sub_expected())):
        y = oracle.spmv(s.rp, s.ci, vals, x)
        y64, _ = oracle.spmv_f64(s.rp, s.ci, vals, x)
        assert _mismatches(y, want) == "", f"{name}/{what} oracle.spmv: {_mismatches(y, want)}"
        assert _mismatches(y64.astype(np.float32), want) == "", f"{name}/{what} oracle.spmv_f64"
        assert np.array_equal(y64.astype(np.float32).astype(np.float64), y64), f"{name}/{what}: fp64 sum not exact"
    if what == "subnormal" and s.nnz:
        nz = want[want != 0]
        assert nz.size == 0 or np.mean(np.abs(nz) < np.finfo(np.float32).tiny) > 0.5, "most sums should be subnormal"
    # dilated with poison: the oracle reads only the referenced entries
    sd = E.dilate(s)
    y = oracle.spmv(sd.rp, sd.ci, ex.vals(), E.dilated_x(ex.x(), np.nan))
    assert _mismatches(y, ex.expected()) == ""
    # non-finite data: the builder's finite rows are the oracle's, and exact there
    vals, x, m_int, finite_rows = E.nonfinite(ex, name)
    y = oracle.spmv(s.rp, s.ci, vals, x)
    y64, _ = oracle.spmv_f64(s.rp, s.ci, vals, x)
    assert np.array_equal(np.isfinite(y64), finite_rows)
    assert _mismatches(y, ex.expected(ex.int_sums(m=m_int)), y64) == ""
    # shuffled with duplicates
    su, _ = E.shuffled(s, name)
    exu = E.Exact(su, name + "/unsorted")
    assert _mismatches(oracle.spmv(su.rp, su.ci, exu.vals(), exu.x()), exu.expected()) == ""


def test_nonfinite_builder_covers_every_class(pkg, oracle):
    """The non-finite transform yields NaN (from NaN data, Inf - Inf and Inf * 0), +Inf and -Inf rows next to finite ones."""
    s = _struct("c3_powerlaw", pkg, oracle)
    ex = E.Exact(s, "c3_powerlaw")
    vals, x, _, finite_rows = E.nonfinite(ex, "c3_powerlaw")
    y64, _ = oracle.spmv_f64(s.rp, s.ci, vals, x)
    assert np.isnan(y64).any() and np.isposinf(y64).any() and np.isneginf(y64).any() and finite_rows.mean() > 0.99
    inf0 = np.isinf(vals) & (x[s.ci] == 0)
    assert inf0.any(), "no Inf * 0 term"
    assert len(E.chunk_crossing_rows(s)) > 0


def test_shuffle_makes_unsorted_rows_with_duplicates(pkg, oracle):
    s = _struct("c4_band4096", pkg, oracle)
    su, _ = E.shuffled(s, "c4_band4096")
    d = np.diff(su.ci.astype(np.int64))
    same_row = su.row_of[1:] == su.row_of[:-1]
    assert (d[same_row] < 0).mean() > 0.3
    assert _has_duplicates(su)
    assert np.array_equal(np.diff(su.rp), np.diff(s.rp))


def test_tolerance_misses_a_dropped_product_the_exact_check_does_not(pkg, oracle):
    """Why the tests above exist: on the 120 000-term row a kernel that drops one small product still passes the
    1e-5 * sum|terms| bound every parity test uses, and fails the exact comparison."""
    s = _struct("one_row_spanning_30_chunks", pkg, oracle)
    ex = E.Exact(s, "drop", scaled=False)
    vals, x = ex.vals(), ex.x()
    want = ex.expected()
    y64, mag = oracle.spmv_f64(s.rp, s.ci, vals, x)
    p = ex.k * ex.m[s.ci]
    drop = int(np.flatnonzero(np.abs(p) == 1)[0])          # one product of magnitude 1 among 120 000
    y_wrong = (want.astype(np.float64) - p[drop]).astype(np.float32)
    assert_close_to_oracle(y_wrong, y64, mag, "a dropped product")         # the bound lets it through ...
    assert _mismatches(y_wrong, want) != ""                                # ... the exact comparison does not
    twice = (want.astype(np.float64) + p[drop]).astype(np.float32)         # nor a doubled one
    assert_close_to_oracle(twice, y64, mag, "a doubled product")
    assert _mismatches(twice, want) != ""
    # and a flushed subnormal sum passes the bound's 1e-37 floor
    sub = ex.sub_expected()
    assert sub[0] != 0 and abs(sub[0]) < np.finfo(np.float32).tiny
    ys64, smag = oracle.spmv_f64(s.rp, s.ci, ex.sub_vals(), ex.sub_x())
    assert_close_to_oracle(np.zeros(1, np.float32), ys64, smag, "a flushed subnormal")
    assert _mismatches(np.zeros(1, np.float32), sub) != ""


# ---- the dense slots -------------------------------------------------------------------------------------------------
DENSE_SHAPES = [(1, 1), (1, 1000), (1000, 1), (33, 65), (63, 257), (257, 255), (4097, 300), (300, 4097), (129, 70)]


def _dense_ints(M, N, seed, zero=0.3):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.integers(-4, 5, size=(M, N)).astype(np.int64)
    A[rng.random((M, N)) < zero] = 0
    x = rng.integers(-4, 5, size=M).astype(np.int64)
    return A, x


def _dense_expected(A, x, exp=0):
    return np.ldexp((x @ A).astype(np.float64), exp).astype(np.float32)


def _dense_run_twice(fn, N, gpu):
    import torch
    dy = torch.empty(max(N, 1), dtype=torch.float32, device=gpu)
    ys = []
    for fill in (float("nan"), float(SENTINEL)):
        dy.fill_(fill)
        fn(dy)
        torch.cuda.synchronize()
        ys.append(dy[:N].cpu().numpy())
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32)), "outputs left unwritten"
    return ys[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N", DENSE_SHAPES)
def test_dense_gemv_exact(pkg, gpu, mode, M, N):
    """spmv_dense_gemv y = A^T x: integers (and the subnormal copy: A k 2^-75, x m 2^-74) bit-identical to int64, with
    and without a caller's workspace; M = 129 and 1000 leave the last of the 64 slabs of modes 2 / 3 ragged."""
    import torch
    capi = pkg.capi
    A, x = _dense_ints(M, N, seed=M * 7 + N + mode)
    assert np.abs(A).sum(axis=0).max() * 4 <= E.EXACT_LIMIT
    for tag, Af, xf, want in (("int", A.astype(np.float32), x.astype(np.float32), _dense_expected(A, x)),
                              ("subnormal", np.ldexp(A, E.SUB_VAL_EXP).astype(np.float32),
                               np.ldexp(x, E.SUB_X_EXP).astype(np.float32), _dense_expected(A, x, E.SUB_VAL_EXP + E.SUB_X_EXP))):
        dA, dx = torch.from_numpy(Af).to(gpu), torch.from_numpy(xf).to(gpu)
        y = _dense_run_twice(lambda dy: capi.dense_gemv(dA, dx, dy, mode), N, gpu)
        assert _mismatches(y, want) == "", f"mode {mode} {M}x{N} {tag}: {_mismatches(y, want)}"
        nb = capi.dense_gemv_workspace_bytes(N, mode)
        if nb:
            ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=gpu)
            y = _dense_run_twice(lambda dy: capi.dense_gemv(dA, dx, dy, mode, workspace=ws), N, gpu)
            assert _mismatches(y, want) == "", f"mode {mode} {M}x{N} {tag} (workspace): {_mismatches(y, want)}"


def _blocky_ints(M, N, seed):
    """Integer A whose 32 x 32 blocks are all-zero, fully dense or about half full, in turn."""
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.integers(1, 5, size=(M, N)) * rng.choice([-1, 1], size=(M, N))
    kind = rng.integers(0, 3, size=(M // 32, N // 32))
    kind.flat[0] = 0
    kind.flat[-1] = 1
    mask = np.repeat(np.repeat(kind, 32, axis=0), 32, axis=1)
    A[(mask == 0) | ((mask == 2) & (rng.random((M, N)) < 0.5))] = 0
    x = rng.integers(-4, 5, size=M)
    return A.astype(np.int64), x.astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", [(32, 32), (64, 96), (96, 64), (256, 384), (1024, 64), (64, 1024), (2048, 160)])
def test_bitmap_formats_and_asp_exact(pkg, gpu, M, N):
    """spmv_asp_retile + spmv_asp_gemv_ws, the tiled bitmap-CSR and the WSP / AWSP / AWSP_REF bitmaps on integer A with
    all-zero, full and half-full 32 x 32 blocks: bit-identical to the int64 A^T x."""
    import torch
    capi = pkg.capi
    A, x = _blocky_ints(M, N, seed=M + 3 * N)
    want = _dense_expected(A, x)
    Af, xf = A.astype(np.float32), x.astype(np.float32)
    dA, dx = torch.from_numpy(Af).to(gpu), torch.from_numpy(xf).to(gpu)
    fails = []
    asp = torch.empty(M * N, dtype=torch.float32, device=gpu)
    capi.asp_retile(dA, asp)
    ws = torch.empty((capi.dense_gemv_workspace_bytes(N, 3) + 3) // 4, dtype=torch.float32, device=gpu)
    y = _dense_run_twice(lambda dy: capi.asp_gemv(M, N, asp, dx, dy, ws), N, gpu)
    if _mismatches(y, want):
        fails.append(f"asp: {_mismatches(y, want)}")
    t = capi.TcsrMatrix.from_dense_device(dA)
    y = _dense_run_twice(lambda dy: t.run(dx, dy), N, gpu)
    if _mismatches(y, want):
        fails.append(f"tcsr: {_mismatches(y, want)}")
    t.close()
    for fmt in ("wsp", "awsp", "awsp_ref"):
        B = capi.BitmapMatrix.from_dense_device(fmt, dA)
        y = _dense_run_twice(lambda dy: B.run(dx, dy), N, gpu)
        if _mismatches(y, want):
            fails.append(f"{fmt}: {_mismatches(y, want)}")
        B.close()
    assert not fails, f"{M}x{N}: " + "; ".join(fails)
