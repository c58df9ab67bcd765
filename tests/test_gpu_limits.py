"""GPU (-m gpu): every SpMV path and SpMM at the 32-bit edges one handle admits (rows, cols, nnz < 2^31).

The matrices are the formula cases of tests/_limits.py.  Past 2^29 nonzeros a signed 32-bit byte offset into vals /
col_idx overflows, past 2^30 an unsigned one wraps and one buffer descriptor no longer covers the array, near INT_MAX
k += 64 and nnz + slack wrap in int; rows >= 2^30 take y and row_ptr past 4 GiB and cols >= 2^30 does the same to x.  A
wrapped index reads the wrong nonzeros of a valid array and returns finite numbers, so every check here is exact: integer
data, the expectation computed by torch in int64 (never by a kernel of this library) and pinned by numpy on chosen rows.

Per case (a child process of its own for the giant ones; the parent asserts on the child's JSON report):
  * spmv_csr_create_device, spmv_csr_validate, spmv_csr_dims, spmv_csr_column_range, spmv_csr_download (bits, by slabs);
  * every entry of test_gpu_exact.PATHS either plans (spmv_csr_plan_describe names the plan asked for; two runs, into NaN
    and into a sentinel, equal the expectation bit for bit on ALL rows) or is refused with SPMV_ERR_INVALID and a message
    that names the limit (nothing launched; the same handle then plans and runs SPMV_TILED exactly).  Which of the two is
    known in advance: refusal() below, from the limits the plans enforce;
  * SPMV_AUTO resolves as AUTO_WANT says;
  * (the *_checked cases) the panel-family paths through lib/libspmv_hip_checked.so: no violation, y bit-identical;
  * (the spmm cases) k = 64, 17, 4, 1 columns of integer X: every column exact, column c the same bits whatever k is;
  * free device memory at the end is back within 2 MiB of the start.
y is always a view one float past a 16-byte boundary inside a buffer with 4096 guard floats on either side (Y of SpMM:
16-byte aligned, as the header requires, guard bands alike); the guards must be untouched after every run.

The giant cases run smallest first (G, C, F, A, B, D, E, then the checked and SpMM runs).  When a child ends by a signal,
an abort or its time limit, that case fails and every later giant case fails with "not run" without touching the GPU.
Run this module as a step of its own, with -x.  Time limits: five times the measured wall time of the child (DESIGN.md,
"The 32-bit edges"), at least 120 s."""
import gc
import json
import os
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np
import pytest

import _limits as L
from test_gpu_exact import KNOBS, PATHS, _describe_fields, _describe_mismatch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
S, WV, WP, VE, AD, TI, PA, AU, XS = range(9)
SENTINEL = -1.2345e30
GUARD, GUARD_N = 3.0e35, 4096
MIB, GIB = 1 << 20, 1 << 30
ERR_INVALID = -2

# the giant runs in order: (id, case, kind); kind "spmv" = every path, "checked" = the bounds-checked build, "spmm"
GIANT = ([(n, n, "spmv") for n in L.ORDER] + [("C_checked", "C", "checked"), ("A_checked", "A", "checked")]
         + [(f"{n}_spmm", n, "spmm") for n in ("A", "B", "E")])
# seconds a child may take: max(120, 5 x measured).  Measured (child wall time, warm-up included): G 4, C 10, F 13, A 44
# (38 of them numpy pinning all 36 864 rows), B 7, D 8, E 7, C_checked 13, A_checked 57, A_spmm 39, B_spmm 22, E_spmm 40
LIMIT = {"G": 120, "C": 120, "F": 120, "A": 220, "B": 120, "D": 120, "E": 120, "C_checked": 120, "A_checked": 290,
         "A_spmm": 200, "B_spmm": 120, "E_spmm": 200}
# what SPMV_AUTO must resolve to: (variant, the panel layouts params[6] allowed)
AUTO_WANT = {"C": (PA, (4, 5)), "D": (PA, (1, 3)), "E": (TI, ())}
SPMM_KS = (64, 17, 4, 1)


def refusal(c, label):
    """None where the path must plan and run case c, else a piece of the message its refusal must carry.
    The limits (include/spmv_hip.h "Limits of the layouts"; csrc line of each check):
      panel sweep, m1 / m2   nnz <= INT_MAX - 4 * kStepMax (= 8192)            kernels_panel.hip build_panel
                             cols <= 4096 panels of 2^17 (m2: 2^14) columns    kernels_panel.hip build_panel
      sorted blocks, m3      nnz <= INT_MAX / 17 * 16 - 4096                   kernels_panel.hip build_panel
      binned, m4 / m5        cols <= 4096 panels of 2^15 columns               kernels_binned.hip plan_binned
                             nnz <= 2^30 - 8 * panels - 512                    kernels_binned.hip plan_binned
      xskip                  ceil(rows / 1024) * cols <= 2^27                  kernels_xskip.hip plan_xskip"""
    if label.startswith("panel/m1") or label == "panel/m2":
        if c.nnz > L.INT_MAX - 8192:
            return "too close to 2^31"
        bits = 14 if label == "panel/m2" else 17
        return "panels" if (c.cols + (1 << bits) - 1) >> bits > 4096 else None
    if label.startswith("panel/m3"):
        if c.nnz > L.INT_MAX // 17 * 16 - 4096:
            return "too close to 2^31"
        return None       # (columns spread too far for a block to share lines of x go to the layout's tail: no refusal)
    if label.startswith("panel/m4") or label.startswith("panel/m5"):
        panels = (c.cols + 32767) >> 15
        if panels > 4096:
            return "panels"
        return "2^30" if c.nnz > (1 << 30) - 8 * panels - 512 else None
    if label == "xskip":
        if (c.rows + 1023) // 1024 * c.cols > 1 << 27:
            return "2^27"
        return "sorted, duplicate-free" if c.columns in ("hash", "ends") else None      # (kernels_xskip.hip plan_xskip)
    return None


def bytes_needed(c, kind):
    """Device bytes a run of case c needs, from its sizes: CSR, x, y and the expectation with their comparison's
    temporaries, the largest plan (the scattered layout's copies and fill temporaries: 24 bytes per nonzero; XSKIP and the
    sweep less), the slab temporaries of the expectation (16 int64 arrays of 2^26), and for SpMM X, Y and 16 columns of
    expectation (with the comparison's copy of both)."""
    n = 8 * c.nnz + 4 * (c.rows + 1) + 5 * c.cols + 4 * 4 * c.rows + 16 * 8 * min(c.nnz, L.SLAB)
    if kind == "spmm":
        return n + 4 * 64 * c.cols + (64 + 17 + 17 + 3 * 8) * 4 * c.rows + 12 * 8 * 8 * min(c.nnz, 1 << 24)
    return n + 24 * c.nnz


# ---- the child -------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats (as rows x ld) inside a buffer with GUARD_N guard floats on either side; offset = 1: the view starts one
    float past a 16-byte boundary."""

    def __init__(self, torch, dev, n, offset):
        self.torch = torch
        self.lo = GUARD_N + offset
        self.buf = torch.full((self.lo + n + GUARD_N,), GUARD, dtype=torch.float32, device=dev)
        self.y = self.buf[self.lo:self.lo + n]
        assert self.y.data_ptr() % 16 == 4 * offset
        self.n = n

    def guards_intact(self):
        return bool((self.buf[:self.lo] == GUARD).all().item()) and bool((self.buf[self.lo + self.n:] == GUARD).all().item())

    def untouched(self, fill):
        return self.guards_intact() and bool((self.y == fill).all().item())


def _diff(torch, y, exp, limit=4, raw=False):
    """'' when y equals exp bit for bit on every row (an exact zero sum may be -0; raw: not even that), else what differs
    (only those entries are downloaded)."""
    bad = (y.view(torch.int32) != exp.view(torch.int32)) if raw else ((y + 0.0).view(torch.int32) != exp.view(torch.int32))
    n = int(bad.sum().item())
    if not n:
        return ""
    idx = bad.view(-1).nonzero()[:limit, 0]
    return (f"{n} entries differ, first {idx.tolist()}: got {y.reshape(-1)[idx].tolist()}, "
            f"want {exp.reshape(-1)[idx].tolist()}")


class Report:
    def __init__(self, path):
        self.path, self.d = path, {"failures": [], "paths": {}, "notes": {}, "done": False}
        self.t0 = time.time()

    def fail(self, msg):
        self.d["failures"].append(msg)
        print("FAIL", msg, flush=True)

    def note(self, key, value):
        self.d["notes"][key] = value
        print(f"  {key}: {value}", flush=True)

    def save(self):
        self.d["wall_s"] = round(time.time() - self.t0, 1)
        if self.path:
            Path(self.path).write_text(json.dumps(self.d, indent=1))


def _set_env(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in env.items():
        os.environ[k] = v


def _free(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def run_case(c, kind, rep, torch, dev, capi, pin=True, paths=None):
    """Everything the module's docstring lists for one case; failures and notes go to rep."""
    t_start = time.time()
    low = [_free(torch)]

    def sample():
        low[0] = min(low[0], torch.cuda.mem_get_info()[0])

    need = bytes_needed(c, kind)
    rep.note("sizes", f"rows={c.rows} cols={c.cols} nnz={c.nnz} needs={need / GIB:.1f} GiB free={low[0] / GIB:.1f} GiB")
    if low[0] < need:
        rep.fail(f"{c.name}: {low[0] / GIB:.1f} GiB of device memory free, the case needs {need / GIB:.1f} GiB")
        return
    b = L.build(c, torch, dev)
    torch.cuda.synchronize()
    sample()
    rep.note("build_s", round(time.time() - t_start, 1))
    # the torch expectation pinned by numpy, from the formulas alone (a thread: numpy works while the GPU does)
    pinned = {}
    if pin:
        rows = L.pinned_rows(c)
        got = b.exp[torch.from_numpy(rows).to(dev)].cpu().numpy()

        def pin_rows():
            t0 = time.time()
            want = L.host_rows(c, rows)
            badr = np.flatnonzero(want.astype(np.float32) != got)
            pinned["bad"] = (f"the torch expectation differs from numpy's on {badr.size} of {rows.size} pinned rows, first "
                             f"{rows[badr[:4]].tolist()}") if badr.size else ""
            pinned["s"] = round(time.time() - t0, 1)
        th = threading.Thread(target=pin_rows)
        th.start()
    A = capi.CsrMatrix.from_device(c.rows, c.cols, b.rp, b.ci, b.va)          # (spmv_csr_create_device validates)
    try:
        if kind == "spmv":
            _check_handle(c, b, A, rep, torch, dev, capi)
            _check_x_alignment(c, b, A, rep, torch, dev, capi)
    finally:
        A.close()
    if kind in ("spmv", "checked"):
        _run_paths(c, b, kind, rep, torch, dev, capi, sample, paths)
    if kind == "spmm":
        _run_spmm(c, b, rep, torch, dev, capi, sample)
    if pin:
        th.join()
        rep.note("numpy_pin_s", pinned.get("s"))
        if pinned.get("bad", "the numpy pin did not finish"):
            rep.fail(pinned.get("bad", "the numpy pin did not finish"))
    rep.note("peak_device_GiB", round((_start_free[0] - low[0]) / GIB, 2))
    rep.note("case_s", round(time.time() - t_start, 1))


_start_free = [0]


def _check_handle(c, b, A, rep, torch, dev, capi):
    if (A.rows, A.cols, A.nnz) != (c.rows, c.cols, c.nnz):
        rep.fail(f"spmv_csr_dims: {(A.rows, A.cols, A.nnz)}")
    capi.check(capi.lib().spmv_csr_validate(A._h, 0))
    if A.column_range() != (b.col_min, b.col_max):
        rep.fail(f"spmv_csr_column_range: {A.column_range()}, the formulas give {(b.col_min, b.col_max)}")
    # spmv_csr_download returns the bits put in: one array at a time on the host, compared on the device slab by slab
    for what, src, n, arg in (("row_ptr", b.rp, c.rows + 1, 0), ("col_idx", b.ci, c.nnz, 1), ("vals", b.va, c.nnz, 2)):
        host = np.empty(n, np.int32)
        ptrs = [0, 0, 0]
        ptrs[arg] = host.ctypes.data
        capi.check(capi.lib().spmv_csr_download(A._h, *ptrs))
        dv = src.view(torch.int32)
        for s0 in range(0, n, L.SLAB):
            if not torch.equal(torch.from_numpy(host[s0:s0 + L.SLAB]).to(dev), dv[s0:s0 + L.SLAB]):
                rep.fail(f"spmv_csr_download: {what} differs in entries [{s0}, {min(n, s0 + L.SLAB)})")
                break
        del host


def _check_x_alignment(c, b, A, rep, torch, dev, capi):
    """x one float past a 16-byte boundary is refused (SPMV_ERR_INVALID) and y stays untouched."""
    g = Guarded(torch, dev, c.rows, 1)
    g.y.fill_(SENTINEL)
    xb = torch.zeros(min(c.cols, 4096) + 4, dtype=torch.float32, device=dev)
    A.plan(TI)
    try:
        capi.check(capi.lib().spmv_csr_run(A._h, TI, xb.data_ptr() + 4, g.y.data_ptr(), 0))
        rep.fail("spmv_csr_run accepted an x that is not 16-byte aligned")
    except capi.SpmvError as e:
        if e.status != ERR_INVALID or "16-byte" not in str(e):
            rep.fail(f"misaligned x: {e}")
    if not g.untouched(SENTINEL):
        rep.fail("a refused run (misaligned x) wrote to y or its guard bands")


def _run_paths(c, b, kind, rep, torch, dev, capi, sample, only=None):
    g = Guarded(torch, dev, c.rows, 1)
    saved = {}
    libs = [("normal", None)] if kind == "spmv" else [("normal", None), ("checked", capi.CHECKED_LIB_PATH)]
    normal_path = capi.LIB_PATH
    for lib_name, lib_path in libs:
        if lib_path is not None:
            capi.use_library(lib_path)
            capi.debug_bounds()
        for label, v, env, params, want in PATHS:
            if only is not None and label not in only:
                continue
            why = refusal(c, label)
            if kind == "checked" and (v != PA or why is not None):
                continue
            t0 = time.time()
            _set_env(env)
            A = capi.CsrMatrix.from_device(c.rows, c.cols, b.rp, b.ci, b.va)
            try:
                g.y.fill_(SENTINEL)
                err = None
                try:
                    A.plan(v) if params is None else A.plan_set(v, params)
                except capi.SpmvError as e:
                    err = e
                sample()
                if err is not None:
                    if why is None:
                        rep.fail(f"{label}: plan refused where a result is expected: {err}")
                        continue
                    if err.status != ERR_INVALID or why not in str(err):
                        rep.fail(f"{label}: refused, but not with SPMV_ERR_INVALID and a message that holds '{why}': {err}")
                    try:
                        A.run(v, b.x, g.y)
                        rep.fail(f"{label}: a run after the refused plan was accepted")
                    except capi.SpmvError:
                        pass
                    if not g.untouched(SENTINEL):
                        rep.fail(f"{label}: the refused plan wrote to y or its guard bands")
                    A.plan(TI)
                    bad = _two_runs(torch, capi, A, TI, b, g)
                    if bad:
                        rep.fail(f"{label}: SPMV_TILED after the refusal: {bad}")
                    rep.d["paths"][label] = f"refused ({why}); SPMV_TILED on the same handle exact on all rows"
                    continue
                if why is not None:
                    rep.fail(f"{label}: planned where a refusal holding '{why}' is expected: {A.plan_describe(v)}")
                    continue
                desc = A.plan_describe(v)
                bad = _describe_mismatch(desc, want)
                if bad:
                    rep.fail(f"{label}: plan is not the one asked for: {bad}")
                bad = _plan_wanted(c, label, v, A, desc)
                if bad:
                    rep.fail(f"{label}: {bad}")
                bad = _two_runs(torch, capi, A, v, b, g)
                sample()
                if bad:
                    rep.fail(f"{label} ({lib_name}): {bad}")
                    continue
                if lib_name == "checked":
                    viol = capi.debug_bounds()
                    if viol:
                        rep.fail(f"{label}: out-of-bounds accesses [site, count, largest overrun in bytes] {viol}")
                    if not torch.equal(saved[label].view(torch.int32), g.y.view(torch.int32)):
                        rep.fail(f"{label}: the checked build's y differs from the normal library's")
                    rep.d["paths"][label] = "checked build: no violation, y bit-identical, exact on all rows"
                else:
                    if kind == "checked":
                        saved[label] = g.y.clone()
                    rep.d["paths"][label] = f"exact on all rows [{desc[:110]}]"
            finally:
                A.close()
                _set_env({})
                print(f"  {lib_name} {label}: {rep.d['paths'].get(label, 'FAILED')} ({time.time() - t0:.1f} s)", flush=True)
                rep.save()
    if kind == "checked":
        capi.use_library(normal_path)


def _plan_wanted(c, label, v, A, desc):
    """What the plan of this path must look like on this case beyond test_gpu_exact's describe check."""
    name = c.name.split("/")[0]
    if v == AU and name in AUTO_WANT and "/" not in c.name:
        p = A.plan_params(AU)
        variant, layouts = AUTO_WANT[name]
        if p[0] != variant or (layouts and p[6] not in layouts):
            return f"SPMV_AUTO resolved to variant {p[0]} layout {p[6]}, wanted {variant} {layouts}: {desc}"
    if name == "B" and v == TI and label.endswith("_c16") and int(_describe_fields(desc).get("col16_chunks", "0")) <= 0:
        return f"no 16-bit chunks on the band: {desc}"
    if name == "B" and label == "wave" and "block_rows" not in desc:
        return f"SPMV_WAVE did not take the bundles: {desc}"
    return ""


def _two_runs(torch, capi, A, v, b, g):
    """Two runs, into NaN and into the sentinel: both the expectation bit for bit on all rows, the guard bands untouched."""
    for fill in (float("nan"), SENTINEL):
        g.y.fill_(fill)
        A.run(v, b.x, g.y)
        torch.cuda.synchronize()
        if not g.guards_intact():
            return "a run wrote outside y[0, rows)"
        bad = _diff(torch, g.y, b.exp)
        if bad:
            return f"(y filled with {fill}) {bad}"
    return ""


def _run_spmm(c, b, rep, torch, dev, capi, sample):
    A = capi.CsrMatrix.from_device(c.rows, c.cols, b.rp, b.ci, b.va)
    try:
        A.spmm_plan()
        rep.note("spmm_plan", A.spmm_describe())
        X = torch.empty((c.cols, 64), dtype=torch.float32, device=dev)
        L.fill_X(c, torch, dev, X)
        X[~b.referenced] = float("nan")
        Y64 = None
        for k in SPMM_KS:
            Xk = X if k == 64 else X[:, :k].contiguous()
            g = Guarded(torch, dev, c.rows * k, 0)
            Y = g.y.view(c.rows, k)
            for fill in (float("nan"),):          # (every expected entry is finite: an unwritten one stays NaN and differs)
                g.y.fill_(fill)
                A.spmm(Xk, Y)
                torch.cuda.synchronize()
                sample()
                if not g.guards_intact():
                    rep.fail(f"spmm k={k}: a run wrote outside Y")
                if k == 64:
                    for c0 in range(0, 64, 8):          # (8 columns of expectation at a time: X and Y are the large arrays)
                        e = L.expected_columns(b, torch, c0, c0 + 8)
                        if c0 == 0 and not torch.equal(e[:, 0], b.exp):
                            rep.fail("spmm: column 0 of the expectation is not the SpMV expectation")
                        bad = _diff(torch, Y[:, c0:c0 + 8], e)
                        del e
                        torch.cuda.empty_cache()
                        sample()
                        if bad:
                            rep.fail(f"spmm k=64 columns {c0}..{c0 + 7} (Y filled with {fill}): {bad}")
                else:
                    bad = _diff(torch, Y, Y64[:, :k], raw=True)
                    if bad:
                        rep.fail(f"spmm k={k}: columns differ from the k=64 run's (Y filled with {fill}): {bad}")
            if k == 64:
                Y64 = Y
            del g, Y, Xk
            torch.cuda.empty_cache()
            rep.d["paths"][f"spmm/k{k}"] = "every column exact on all rows" if not rep.d["failures"] else "see failures"
            print(f"  spmm k={k} done", flush=True)
            rep.save()
    finally:
        A.close()


def child_main(run_id, out):
    """One giant run in a process of its own: a warm-up (the same case at 1/64: the same kernels' code objects, the
    runtime's pools), then the case, then the memory that must have come back."""
    sys.path.insert(0, os.fspath(ROOT))
    import torch
    import __graft_entry__ as ge
    capi = ge.load_package().capi
    dev = torch.device("cuda:0")
    _, name, kind = next(g for g in GIANT if g[0] == run_id)
    rep = Report(out)
    warm = Report(None)
    run_case(L.case(name, scaled=True), kind, warm, torch, dev, capi, pin=False)
    if warm.d["failures"]:
        rep.fail(f"the warm-up (the case at 1/64) failed: {warm.d['failures'][:3]}")
    del warm
    gc.collect()
    torch.cuda.empty_cache()
    _start_free[0] = _free(torch)
    run_case(L.case(name), kind, rep, torch, dev, capi)
    gc.collect()
    torch.cuda.empty_cache()
    end_free = _free(torch)
    rep.note("free_start_end_MiB", [_start_free[0] // MIB, end_free // MIB])
    if _start_free[0] - end_free > 2 * MIB:
        rep.fail(f"{(_start_free[0] - end_free) / MIB:.1f} MiB of device memory did not come back")
    rep.d["done"] = True
    rep.save()
    print(f"{run_id}: {len(rep.d['failures'])} failure(s), {rep.d['wall_s']} s", flush=True)


# ---- the parent ------------------------------------------------------------------------------------------------------------
_abnormal = []


def _summary(run_id, d):
    lines = [f"{run_id}: wall {d.get('wall_s')} s; " + "; ".join(f"{k}={v}" for k, v in d.get("notes", {}).items())]
    lines += [f"  {k}: {v}" for k, v in d.get("paths", {}).items()]
    return "\n".join(lines)


@pytest.mark.parametrize("name", L.ORDER)
def test_scaled_cases_every_path(pkg, gpu, name):
    """The same formulas at 1/64 (nothing reaches 2^29), in this process: a formula or harness mistake shows here, in
    seconds, before anything giant is allocated.  SpMM on the cases that run it at full size."""
    import torch
    c = L.case(name, scaled=True)
    _start_free[0] = _free(torch)
    rep = Report(None)
    run_case(c, "spmv", rep, torch, gpu, pkg.capi)
    if name in ("A", "B", "E"):
        run_case(c, "spmm", rep, torch, gpu, pkg.capi, pin=False)
    if name in ("A", "C"):
        run_case(c, "checked", rep, torch, gpu, pkg.capi, pin=False)
    print(_summary(name + "/64", rep.d))
    assert not rep.d["failures"], f"{name}/64: {len(rep.d['failures'])} failure(s):\n" + "\n".join(rep.d["failures"])
    assert len([p for p in rep.d["paths"] if not p.startswith("spmm")]) == len(PATHS)


@pytest.mark.parametrize("run_id", [g[0] for g in GIANT])
def test_giant_cases(pkg, gpu, tmp_path, run_id):
    if _abnormal:
        pytest.fail(f"not run: an earlier case ended abnormally ({_abnormal[0]})")
    out = tmp_path / "report.json"
    cmd = [sys.executable, os.fspath(Path(__file__).resolve()), run_id, os.fspath(out)]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[run_id])
        rc, tail = r.returncode, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    except subprocess.TimeoutExpired as e:
        rc, tail = "time limit", str(e.stdout)[-3000:]
    d = json.loads(out.read_text()) if out.exists() else {}
    print(_summary(run_id, d) + f"\n  child: {time.time() - t0:.0f} s of at most {LIMIT[run_id]} s")
    keep = os.environ.get("SPMV_LIMITS_REPORTS")
    if keep and d:
        (Path(keep) / f"{run_id}.json").write_text(json.dumps(d, indent=1))
    if rc != 0 or not d.get("done"):
        _abnormal.append(f"{run_id}: exit {rc}")
        pytest.fail(f"{run_id}: the child ended abnormally (exit {rc}) after {time.time() - t0:.0f} s; its last paths: "
                    f"{list(d.get('paths', {}))[-3:]}\n{tail}")
    assert not d["failures"], f"{run_id}: {len(d['failures'])} failure(s):\n" + "\n".join(d["failures"])
    _, name, kind = next(g for g in GIANT if g[0] == run_id)
    c = L.case(name)
    if kind == "spmv":
        assert set(d["paths"]) == {p[0] for p in PATHS}, "a path was left out"
    elif kind == "checked":
        assert set(d["paths"]) == {p[0] for p in PATHS if p[1] == PA and refusal(c, p[0]) is None} != set()
    else:
        assert set(d["paths"]) == {f"spmm/k{k}" for k in SPMM_KS}


def test_misaligned_x_is_refused_and_y_untouched(pkg, gpu):
    """spmv_csr_run asks 16 bytes of x and only 4 of y (include/spmv_hip.h): x one float past a 16-byte boundary is
    SPMV_ERR_INVALID on every variant and nothing is written; the same x aligned, into a y one float past a boundary, runs."""
    import torch
    capi = pkg.capi
    c = L.case("G", scaled=True)
    b = L.build(c, torch, gpu)
    A = capi.CsrMatrix.from_device(c.rows, c.cols, b.rp, b.ci, b.va)
    g = Guarded(torch, gpu, c.rows, 1)
    xb = torch.zeros(c.cols + 4, dtype=torch.float32, device=gpu)
    xb[1:c.cols + 1] = torch.nan_to_num(b.x, nan=0.0)
    assert xb.data_ptr() % 16 == 0
    for v in (S, WV, WP, VE, AD, TI, PA, AU):
        A.plan(v)
        g.y.fill_(SENTINEL)
        with pytest.raises(capi.SpmvError) as e:
            capi.check(capi.lib().spmv_csr_run(A._h, v, xb.data_ptr() + 4, g.y.data_ptr(), 0))
        assert e.value.status == ERR_INVALID and "16-byte" in str(e.value), v
        torch.cuda.synchronize()
        assert g.untouched(SENTINEL), f"variant {v}: the refused run wrote to y or its guard bands"
        assert _two_runs(torch, capi, A, v, b, g) == "", v
    A.close()


def test_refusal_table_matches_the_cases():
    """The table itself: the refusals the issue's cases are built to meet (no GPU needed, kept beside its table)."""
    want = {"C": set(), "D": {"panel/m4", "panel/m5"}, "E": {"panel/m1", "panel/m2", "panel/m3", "panel/m4", "panel/m5", "xskip"},
            "A": {"panel/m4", "panel/m5"}, "G": {"panel/m1", "panel/m2", "panel/m4", "panel/m5", "xskip"}}
    for name, fam in want.items():
        c = L.case(name)
        got = {p[0].split("_")[0] for p in PATHS if refusal(c, p[0]) is not None}
        if name in ("C", "D"):
            got.discard("xskip")
        assert got == fam, (name, got)


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
