#!/usr/bin/env python3
"""tools/spmm_time.py -- spmv_csr_spmm (k right-hand sides at once) against k back-to-back SPMV_AUTO runs and rocSPARSE.

One JSON line per (workload, k): the plan's time and bytes, the SpMM time, the time of k spmv_csr_run(SPMV_AUTO) calls on
the same data (each column of X copied out to a contiguous x first, outside the timed window), the algorithmic bytes
4 (rows + 1) + 8 nnz + 4 k (cols + rows) and their share of 8 TB/s, and rocsparse_spmm (CSR, row-major dense B and C, loaded
with ctypes as tools/vendor_compare.py loads rocSPARSE) with its largest difference to our Y.  Times: HIP events, warmed up,
median of --reps windows of --iters launches.

    python tools/spmm_time.py [--workloads c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0] [--ks 1,4,8,16,32,64] [--out FILE]

--dtype fp32,bf16[,fp16] times spmv_csr_spmm_16 instead: per (workload, k) the fp32 call and each 16-bit call on the same
numbers (X rounded to the dtype; the fp32 call runs on the fp32 X), in windows that alternate between them in one process,
so that a drift of the device's clocks falls on all alike.  One JSON line each: the median of every call's windows, the
ratio 16-bit / fp32, the spread of the fp32 call's own windows ((max - min) / median: what a ratio has to be read against),
and whether Y of the 16-bit call is, bit for bit, the fp32 call's Y on the widened X rounded by torch.  Appended to
profiles/spmm_16bit.jsonl unless --out names another file; the comparisons above are not run in this mode.

--cols 128,256,512 times spmv_csr_spmm_cols (one call at any k) against what a caller did before it: the loop of narrow
calls over the column blocks of 64, on views of the same X and Y.  Per (workload, k, dtype of --dtype, default fp32,bf16) the
two run in windows that alternate in one process; before the clocks start Y of the call must be, bit for bit, Y of the loop.
One JSON line each -- both medians, their ratio, both spreads ((max - min) / median of the windows) and whether the call is
slower than the loop by more than twice the larger spread -- appended to profiles/spmm_cols.jsonl unless --out names another
file.  Default workloads: configs 2 and 3, band 8192 and uniform.  --lib names another build of the library for an A/B run.
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from vendor_compare import F32, I32, RocSparse  # noqa: E402

PEAK_BPS = 8e12
ROW_ORDER = 0                                          # rocsparse_order_row
SPMM_SIZE, SPMM_PREP, SPMM_COMPUTE = 1, 2, 3           # rocsparse_spmm_stage_*


def timed(fn, iters, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)


DTYPES = {"fp32": "float32", "bf16": "bfloat16", "fp16": "float16"}
OUT_16BIT = ROOT / "profiles" / "spmm_16bit.jsonl"


def interleaved(fns, iters, reps):
    """{name: [ms per call of each of `reps` windows of `iters` launches]}: the windows of the calls alternate."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns.values():
        for _ in range(3):
            fn()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / iters)
    return out


def compare_16bit(kind, label, k, calls, same, iters, reps):
    """The JSON line of one (workload, k): calls = {dtype name: fn}, fp32 among them; same = {dtype name: bool}."""
    w = interleaved(calls, iters, reps)
    med = {n: statistics.median(v) for n, v in w.items()}
    row = dict(call=kind, workload=label, k=k, iters=iters, reps=reps, fp32_ms=round(med["fp32"], 4),
               fp32_spread=round((max(w["fp32"]) - min(w["fp32"])) / med["fp32"], 4))
    for n in calls:
        if n != "fp32":
            row.update({f"{n}_ms": round(med[n], 4), f"{n}_over_fp32": round(med[n] / med["fp32"], 3),
                        f"{n}_spread": round((max(w[n]) - min(w[n])) / med[n], 4), f"{n}_is_fp32_rounded_once": same[n]})
    return row


OUT_COLS = ROOT / "profiles" / "spmm_cols.jsonl"


def cols_sweep(kind, a, emit):
    """--cols of this tool (kind "spmm") and of tools/sddmm_time.py ("sddmm"): one JSON line per (workload, k, dtype)."""
    import torch
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    if a.lib:
        capi.use_library(a.lib)
    dev = torch.device("cuda:0")
    widths = [int(s) for s in a.cols.split(",")]
    dtypes = a.dtype.split(",")
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)      # noqa: E731
    for spec in a.workloads.split(","):
        name, band = spec.split(":")
        w = W.config(name, band=int(band))
        rp = W.row_ptr(w)
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
        A.spmm_plan_cols(max(widths))
        for k in widths:
            blocks = [(c, min(c + 64, k)) for c in range(0, k, 64)]
            for d in dtypes:
                dt = getattr(torch, DTYPES[d])
                gen = torch.Generator(device=dev).manual_seed(k)
                X = torch.randn((w.cols, k), generator=gen, device=dev).to(dt)
                if kind == "spmm":
                    Y, Yl = torch.empty((w.rows, k), dtype=dt, device=dev), torch.empty((w.rows, k), dtype=dt, device=dev)

                    def call():
                        A.spmm_cols(X, Y)

                    def loop():                              # what a caller does without the call: one narrow call per column block
                        for c0, c1 in blocks:
                            A.spmm(X[:, c0:c1], Yl[:, c0:c1])
                    got, want = Y, Yl
                else:
                    U = torch.randn((w.rows, k), generator=gen, device=dev).to(dt)
                    got, want = (torch.empty(nnz, dtype=torch.float32, device=dev) for _ in range(2))
                    tmp = torch.empty(nnz, dtype=torch.float32, device=dev)      # the loop's nnz-sized temporary

                    def call():
                        A.sddmm_cols(U, X, got)

                    def loop():                              # the first block into the result, every further one added by torch
                        for i, (c0, c1) in enumerate(blocks):
                            A.sddmm(U[:, c0:c1], X[:, c0:c1], tmp if i else want)
                            if i:
                                want.add_(tmp)
                # the bit check at the timed size, before the clocks start
                call(), loop()
                torch.cuda.synchronize()
                same = bool(torch.equal(bits(got), bits(want)))
                win = interleaved({"cols": call, "loop": loop}, a.iters, a.reps)
                med = {n: statistics.median(v) for n, v in win.items()}
                spread = {n: (max(v) - min(v)) / med[n] for n, v in win.items()}
                emit(call=f"{kind}_cols", workload=f"{name}_band{band}", k=k, dtype=d, iters=a.iters, reps=a.reps,
                     cols_ms=round(med["cols"], 4), loop_ms=round(med["loop"], 4), cols_over_loop=round(med["cols"] / med["loop"], 3),
                     cols_spread=round(spread["cols"], 4), loop_spread=round(spread["loop"], 4),
                     slower_than_twice_the_spread=bool(med["cols"] - med["loop"] > 2 * max(spread.values()) * med["loop"]),
                     same_bits_as_loop=same, lib=Path(capi.LIB_PATH).name)
                del X, got, want
                if kind == "spmm":
                    del Y, Yl
                else:
                    del U, tmp
                torch.cuda.empty_cache()
        A.close()
        del d_rp, d_ci, d_va
        torch.cuda.empty_cache()


def run_cols(kind, a):
    """The --cols mode of both tools: appends to profiles/spmm_cols.jsonl unless --out names another file."""
    if a.workloads == "c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0":     # (the default: c4's X at these widths does not fit the purpose)
        a.workloads = "c2:8192,c2:0,c3:8192,c3:0"
    if a.dtype == "fp32":
        a.dtype = "fp32,bf16"
    with open(a.out or OUT_COLS, "a") as out:
        def emit(**kv):
            line = json.dumps(kv)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        cols_sweep(kind, a, emit)


def rocsparse_spmm(rs, rows, cols, nnz, d_rp, d_ci, d_va, X, Y, iters, reps):
    """(ms per call, preprocess ms) of rocsparse_spmm with the default algorithm; Y receives its result."""
    import torch
    L = rs.L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    L.rocsparse_create_dnmat_descr.argtypes = [ctypes.POINTER(vp), i64, i64, i64, vp, i32, i32]
    L.rocsparse_destroy_dnmat_descr.argtypes = [vp]
    L.rocsparse_spmm.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t), vp]
    one, zero = ctypes.c_float(1.0), ctypes.c_float(0.0)
    mat, mb, mc = vp(), vp(), vp()
    k = X.shape[1]
    rs._ok(L.rocsparse_create_csr_descr(ctypes.byref(mat), rows, cols, nnz, d_rp.data_ptr(), d_ci.data_ptr(),
                                        d_va.data_ptr(), I32, I32, 0, F32), "create_csr")
    rs._ok(L.rocsparse_create_dnmat_descr(ctypes.byref(mb), cols, k, X.stride(0), X.data_ptr(), F32, ROW_ORDER), "dnmat B")
    rs._ok(L.rocsparse_create_dnmat_descr(ctypes.byref(mc), rows, k, Y.stride(0), Y.data_ptr(), F32, ROW_ORDER), "dnmat C")
    size = ctypes.c_size_t(0)

    def call(stage, buf):
        return L.rocsparse_spmm(rs.h, 111, 111, ctypes.byref(one), mat, mb, ctypes.byref(zero), mc, F32, 0, stage,
                                ctypes.byref(size), buf)
    try:
        rs._ok(call(SPMM_SIZE, None), "spmm buffer_size")
        buf = torch.empty(max(int(size.value), 16), dtype=torch.uint8, device=X.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rs._ok(call(SPMM_PREP, buf.data_ptr()), "spmm preprocess")
        e1.record()
        torch.cuda.synchronize()
        prep = e0.elapsed_time(e1)
        Y.zero_()
        ms = timed(lambda: call(SPMM_COMPUTE, buf.data_ptr()), iters, reps)
        return ms, prep
    finally:
        L.rocsparse_destroy_dnmat_descr(mb)
        L.rocsparse_destroy_dnmat_descr(mc)
        L.rocsparse_destroy_spmat_descr(mat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0")
    ap.add_argument("--ks", default="1,4,8,16,32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--dtype", default="fp32", help="fp32 (the comparisons of the first paragraph), or fp32,bf16[,fp16]")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cols", default=None, help="widths above 64, e.g. 128,256,512: time spmv_csr_spmm_cols against the loop of narrow calls")
    ap.add_argument("--lib", default=None, help="--cols: another build of libspmv_hip.so (tools/build_variant.sh), for an A/B run")
    a = ap.parse_args()
    if a.cols:
        run_cols("spmm", a)
        return
    import torch
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    dev = torch.device("cuda:0")
    dtypes = a.dtype.split(",")
    if any(d not in DTYPES for d in dtypes) or "fp32" not in dtypes:
        ap.error("--dtype lists fp32 and any of bf16, fp16")
    sixteen = [d for d in dtypes if d != "fp32"]
    if sixteen and not a.out:
        a.out = str(OUT_16BIT)
    out = open(a.out, "a") if a.out else None
    rs = None if a.no_rocsparse or sixteen else RocSparse()
    if rs is not None:
        rs._ok(rs.L.rocsparse_set_stream(rs.h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "set_stream")

    def emit(**kv):
        line = json.dumps(kv)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for spec in a.workloads.split(","):
        name, band = spec.split(":")
        w = W.config(name, band=int(band))
        rp = W.row_ptr(w)
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A.spmm_plan()
        plan_ms = (time.perf_counter() - t0) * 1e3
        if not sixteen:
            A.plan(capi.AUTO)
        label = f"{name}_band{band}"
        for k in (int(s) for s in a.ks.split(",")):
            X = torch.randn((w.cols, k), generator=torch.Generator(device=dev).manual_seed(k), device=dev)
            Y = torch.empty((w.rows, k), dtype=torch.float32, device=dev)
            if sixteen:
                X16 = {d: X.to(getattr(torch, DTYPES[d])) for d in sixteen}
                Y16 = {d: torch.empty((w.rows, k), dtype=X16[d].dtype, device=dev) for d in sixteen}
                same = {}
                for d in sixteen:
                    A.spmm(X16[d].to(torch.float32), Y)
                    A.spmm(X16[d], Y16[d])
                    torch.cuda.synchronize()
                    same[d] = bool(torch.equal(Y.to(X16[d].dtype).view(torch.int16), Y16[d].view(torch.int16)))
                calls = {"fp32": lambda: A.spmm(X, Y)}
                calls.update({d: (lambda d=d: A.spmm(X16[d], Y16[d])) for d in sixteen})
                emit(**compare_16bit("spmm", label, k, calls, same, a.iters, a.reps))
                del X, Y, X16, Y16
                torch.cuda.empty_cache()
                continue
            ms = timed(lambda: A.spmm(X, Y), a.iters, a.reps)
            xs = [X[:, c].contiguous() for c in range(k)]
            ys = [torch.empty(w.rows, dtype=torch.float32, device=dev) for _ in range(k)]

            def loop():
                for c in range(k):
                    A.run(capi.AUTO, xs[c], ys[c])
            ms_loop = timed(loop, max(1, a.iters // k), a.reps)
            torch.cuda.synchronize()
            diff_auto = max(float((Y[:, c] - ys[c]).abs().max()) for c in range(k))
            B = 4 * (w.rows + 1) + 8 * nnz + 4 * k * (w.cols + w.rows)
            row = dict(workload=label, k=k, rows=w.rows, cols=w.cols, nnz=nnz, plan_ms=round(plan_ms, 2),
                       plan_bytes=A.spmm_plan_bytes(), plan=A.spmm_describe(), spmm_ms=round(ms, 4),
                       k_auto_runs_ms=round(ms_loop, 4), speedup_vs_k_auto=round(ms_loop / ms, 2),
                       algorithmic_bytes=B, frac_of_8TBs=round(B / (ms * 1e-3) / PEAK_BPS, 3),
                       max_diff_vs_auto=diff_auto, auto_plan=A.plan_describe(capi.AUTO))
            del xs, ys
            if rs is not None:
                Yr = torch.empty_like(Y)
                try:
                    rms, rprep = rocsparse_spmm(rs, w.rows, w.cols, nnz, d_rp, d_ci, d_va, X, Yr, a.iters, a.reps)
                    torch.cuda.synchronize()
                    row.update(rocsparse_ms=round(rms, 4), rocsparse_prep_ms=round(rprep, 2),
                               rocsparse_max_diff=float((Yr - Y).abs().max()))
                except RuntimeError as e:
                    row.update(rocsparse_error=str(e))
                del Yr
            emit(**row)
            del X, Y
            torch.cuda.empty_cache()
        A.close()
        del d_rp, d_ci, d_va
        torch.cuda.empty_cache()
    if rs is not None:
        rs.close()


if __name__ == "__main__":
    main()
