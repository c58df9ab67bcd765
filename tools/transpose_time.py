#!/usr/bin/env python3
"""tools/transpose_time.py -- what spmv_csr_transpose and spmv_csr_transpose_values cost, beside their yardsticks.

One process, one device, warm; the contenders of a workload alternate inside every repetition.  One JSON object per
(workload, contender) goes to stdout and, with --out, to a file (profiles/transpose_time.jsonl), each with the command
line and the commit.

    transpose            spmv_csr_transpose, map kept / not: wall time of the whole call (it allocates T and its
                         temporaries, enqueues, waits and frees the temporaries), effective GB/s over
                         12 nnz + 4 (rows + cols) bytes; destroying T is timed separately
    csr2csc (--vendor)   rocsparse_csr2csc_buffer_size + rocsparse_scsr2csc (rocsparse_action_numeric) on the same device
                         arrays: HIP events around the call alone, outputs and buffer allocated outside the timing
    values               spmv_csr_transpose_values against spmv_calib_stream over 12 nnz bytes (HIP events)
    z = A^T u            SPMV_AUTO on T against SPMV_AUTO on a from_device handle of torch's stable-sort transposition of
                         the same matrix: plan_describe equal, y bit-identical, ms per run of both; with --vendor also
                         rocsparse_spmv with rocsparse_operation_transpose on A, every algorithm that accepts it

    python tools/transpose_time.py [--out FILE] [--reps 10] [--vendor] [--only c2,c4_band8192]
"""
import argparse
import ctypes
import json
import subprocess
import sys
import time
from dataclasses import replace
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

Mi = 1 << 20


def workloads(W):
    c4 = W.CONFIGS["c4"]
    return {
        "c2": (W.config("c2"), None),
        "c3": (W.config("c3"), None),
        "c4_band8192": (W.config("c4", band=8192), None),
        "c4_uniform": (W.config("c4", band=0), None),
        # config 5's shard: 16 Mi rows of a (128 Mi)^2 matrix -- T is tall (128 Mi x 16 Mi)
        "c5_shard": (replace(c4, name="c5", rows=128 * Mi, cols=128 * Mi), 16 * Mi),
    }


def events(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms):
    s = sorted(ms)
    return {"ms_median": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4), "reps": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vendor", action="store_true", help="also time rocSPARSE (loads librocsparse.so)")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    dev = torch.device("cuda:0")
    commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    sink = open(args.out, "a") if args.out else None

    def emit(**kw):
        kw.update(command=" ".join(["python", "tools/transpose_time.py"] + sys.argv[1:]), commit=commit or "unknown",
                  device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    rs = None
    if args.vendor:
        sys.path.insert(0, str(ROOT / "tools"))
        import vendor_compare as VC
        rs = VC.RocSparse()
        L = rs.L
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        L.rocsparse_csr2csc_buffer_size.argtypes = [vp, i32, i32, i32, vp, vp, i32, ctypes.POINTER(ctypes.c_size_t)]
        L.rocsparse_scsr2csc.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp]
        rs._ok(L.rocsparse_set_stream(rs.h, vp(torch.cuda.current_stream().cuda_stream)), "set_stream")

    only = [s for s in args.only.split(",") if s]
    for name, (w, n_local) in workloads(W).items():
        if only and name not in only:
            continue
        rows = n_local or w.rows
        rp = W.row_ptr(w, 0, rows)
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        A = capi.CsrMatrix.from_device(rows, w.cols, d_rp, d_ci, d_va)
        moved = 12 * nnz + 4 * (rows + w.cols)
        base = dict(workload=name, rows=rows, cols=w.cols, nnz=nnz, band=w.band)

        # -- the transpose itself, and the vendor's conversion --------------------------------------------------------------
        A.transpose().close()                                               # warm: code objects, the allocator
        wall = {0: [], 1: []}
        destroy = []
        if rs is not None:
            size = ctypes.c_size_t(0)
            rs._ok(rs.L.rocsparse_csr2csc_buffer_size(rs.h, rows, w.cols, nnz, d_rp.data_ptr(), d_ci.data_ptr(), 1,
                                                      ctypes.byref(size)), "csr2csc_buffer_size")
            buf = torch.empty(max(int(size.value), 16), dtype=torch.uint8, device=dev)
            o_va = torch.empty(nnz, dtype=torch.float32, device=dev)
            o_ri = torch.empty(nnz, dtype=torch.int32, device=dev)
            o_cp = torch.empty(w.cols + 1, dtype=torch.int32, device=dev)

            def vendor():
                rs._ok(rs.L.rocsparse_scsr2csc(rs.h, rows, w.cols, nnz, d_va.data_ptr(), d_rp.data_ptr(), d_ci.data_ptr(),
                                               o_va.data_ptr(), o_ri.data_ptr(), o_cp.data_ptr(), 1, 0, buf.data_ptr()), "scsr2csc")
            vendor()
            torch.cuda.synchronize()
            vendor_ms = []
        for _ in range(args.reps):
            for keep in (1, 0):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T = A.transpose(keep_map=bool(keep))
                wall[keep].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                T.close()
                destroy.append((time.perf_counter() - t0) * 1e3)
            if rs is not None:
                vendor_ms += events(torch, vendor, 1)
        for keep in (1, 0):
            st = stats(wall[keep])
            emit(**base, contender=f"spmv_csr_transpose keep_map={keep}", timing="wall clock of the call (allocations and the wait included)",
                 effective_GBps=round(moved / st["ms_median"] / 1e6, 1), **st)
        emit(**base, contender="spmv_csr_destroy of T", timing="wall clock", **stats(destroy))
        if rs is not None:
            st = stats(vendor_ms)
            emit(**base, contender="rocsparse_scsr2csc numeric", timing="HIP events around the call; buffer and outputs allocated outside",
                 buffer_bytes=int(size.value), effective_GBps=round(moved / st["ms_median"] / 1e6, 1), **st)
            del buf, o_va, o_ri, o_cp

        # -- the values refresh against a stream of the same bytes ------------------------------------------------------------
        T = A.transpose(keep_map=True)
        src = torch.empty(3 * nnz, dtype=torch.float32, device=dev).fill_(1.0)
        snk = torch.zeros(1 << 20, dtype=torch.float32, device=dev)
        T.transpose_values(A)
        capi.calib_stream(src, 12 * nnz, snk)
        tv, ts = [], []
        for _ in range(args.reps):
            tv += events(torch, lambda: T.transpose_values(A), 1)
            ts += events(torch, lambda: capi.calib_stream(src, 12 * nnz, snk), 1)
        sv, ss = stats(tv), stats(ts)
        emit(**base, contender="spmv_csr_transpose_values", timing="HIP events", ratio_to_stream=round(sv["ms_median"] / ss["ms_median"], 3), **sv)
        emit(**base, contender="spmv_calib_stream 12 B per nonzero", timing="HIP events", **ss)
        del src, snk

        # -- z = A^T u: SPMV_AUTO on T and on torch's transposition --------------------------------------------------------------
        perm = torch.sort(d_ci.long(), stable=True).indices
        row_of = torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device=dev), torch.from_numpy(np.diff(rp)).to(dev))
        e_ci, e_va = row_of[perm].contiguous(), d_va[perm].contiguous()
        e_rp = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                          torch.cumsum(torch.bincount(d_ci.long(), minlength=w.cols), 0)]).to(torch.int32)
        del perm, row_of
        R = capi.CsrMatrix.from_device(w.cols, rows, e_rp, e_ci, e_va)
        u = torch.empty(rows, dtype=torch.float32, device=dev)
        capi.synth_x(w.seed, 0, rows, u)
        yt = torch.empty(w.cols, dtype=torch.float32, device=dev)
        yr = torch.empty(w.cols, dtype=torch.float32, device=dev)
        T.plan(capi.AUTO)
        R.plan(capi.AUTO)
        T.run(capi.AUTO, u, yt)
        R.run(capi.AUTO, u, yr)
        torch.cuda.synchronize()
        same_y = bool(torch.equal(yt.view(torch.int32), yr.view(torch.int32)))
        same_plan = T.plan_describe(capi.AUTO) == R.plan_describe(capi.AUTO)
        tt, tr = [], []
        for _ in range(args.reps):
            tt.append(T.time(capi.AUTO, u, yt, 20))
            tr.append(R.time(capi.AUTO, u, yr, 20))
        emit(**base, contender="SPMV_AUTO on T", timing="spmv_csr_time, 20 launches per repetition", plan=T.plan_describe(capi.AUTO),
             same_plan_as_torch_built=same_plan, y_bit_identical_to_torch_built=same_y, **stats(tt))
        emit(**base, contender="SPMV_AUTO on torch's stable-sort transposition", timing="spmv_csr_time, 20 launches per repetition",
             plan=R.plan_describe(capi.AUTO), **stats(tr))
        if rs is not None:
            import vendor_compare as VC
            one, zero = ctypes.c_float(1.0), ctypes.c_float(0.0)
            vx, vy = ctypes.c_void_p(), ctypes.c_void_p()
            rs._ok(rs.L.rocsparse_create_dnvec_descr(ctypes.byref(vx), rows, u.data_ptr(), VC.F32), "dnvec u")
            rs._ok(rs.L.rocsparse_create_dnvec_descr(ctypes.byref(vy), w.cols, yr.data_ptr(), VC.F32), "dnvec z")
            for aname, alg in VC.ALGS.items():
                mat, size = ctypes.c_void_p(), ctypes.c_size_t(0)
                rs._ok(rs.L.rocsparse_create_csr_descr(ctypes.byref(mat), rows, w.cols, nnz, d_rp.data_ptr(), d_ci.data_ptr(),
                                                       d_va.data_ptr(), VC.I32, VC.I32, 0, VC.F32), "create_csr")

                def call(stage, b, mat=mat, alg=alg, size=size):          # 112 = rocsparse_operation_transpose
                    return rs.L.rocsparse_spmv(rs.h, 112, ctypes.byref(one), mat, vx, ctypes.byref(zero), vy, VC.F32, alg, stage,
                                               ctypes.byref(size), b)
                if call(VC.STAGE_SIZE, None) == 0:
                    b = torch.empty(max(int(size.value), 16), dtype=torch.uint8, device=dev)
                    yr.zero_()
                    if call(VC.STAGE_PREP, b.data_ptr()) == 0 and call(VC.STAGE_COMPUTE, b.data_ptr()) == 0:
                        torch.cuda.synchronize()
                        ms = events(torch, lambda: call(VC.STAGE_COMPUTE, b.data_ptr()), args.reps)
                        emit(**base, contender=f"rocsparse_spmv transpose {aname}", timing="HIP events, one launch each", **stats(ms))
                    else:
                        emit(**base, contender=f"rocsparse_spmv transpose {aname}", result="refused by rocSPARSE")
                    del b
                else:
                    emit(**base, contender=f"rocsparse_spmv transpose {aname}", result="refused by rocSPARSE")
                torch.cuda.synchronize()
                rs.L.rocsparse_destroy_spmat_descr(mat)
            rs.L.rocsparse_destroy_dnvec_descr(vx)
            rs.L.rocsparse_destroy_dnvec_descr(vy)
        for h in (R, T, A):
            h.close()
        del d_rp, d_ci, d_va, e_rp, e_ci, e_va, u, yt, yr
        torch.cuda.empty_cache()
    if rs is not None:
        rs.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
