#!/usr/bin/env python3
"""tools/trsv_time.py [--out FILE] [--window-ms 100] [--windows 5] [--only NAME,...] [--thin 64,256,1024,4096 [--sweep-out FILE]]
[--no-rocsparse] -- spmv_csr_trsv against its traffic floor and against rocsparse_spsv.

Workloads, each solved for the lower and for the upper triangle on the matrix's own handle (b of ones): stencil7(200) (8 000 000
rows; the level of a grid point is i + j + k, 598 levels), and config 2 with band 8192 and with uniform columns, given a
dominant diagonal through spmv_csr_add(A, I, 1, 64, UNION).  One JSON line per workload and triangle:

  levels, launches, widest, long_rows, thin_rows, level_cap, plan_bytes      the plan's report
  plan_ms          spmv_csr_trsv_plan: a host clock around the synchronous call (the transpose of the pattern, the peel with
                   its read-backs, the sort by level), median of three
  solve_ms         one solve as enqueued: launches from the host, between two device synchronisations
  graph_ms         the same solve captured once in a graph and replayed
  us_per_launch    graph_ms / launches
  floor_ms         the traffic floor at 8 TB/s: row_ptr, the triangle's col_idx and vals, b read and x written once
                   (4 (rows + 1) + 8 nnz_triangle + 8 rows bytes); over_floor = graph_ms / floor_ms
  rocsparse_prep_ms, rocsparse_ms   rocsparse_spsv on the same arrays (fill mode and non-unit diagonal set on the descriptor):
                   the preprocess stage once, the compute stage in the same windows; vendor_ratio = graph_ms / rocsparse_ms
  rocsparse_close  its x within the host test's bound of ours: |dx_i| <= 1e-5 (|b_i| + sum |v x|) / |d_i|
  rocsparse_error  instead, what the binding or the library refused with
  *_spread         (max - min) / median over the windows

--thin: the same workloads planned with each of these thresholds instead of the default, solve_ms and graph_ms only, one line
per (workload, triangle, threshold) into --sweep-out (profiles/trsv_thin_sweep.jsonl); the default line is not written then.

All sides run in one process in alternating windows of at least --window-ms (at least two calls); a window's figure is its mean
call; the medians of --windows windows are reported.  Needs a device."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

HBM_BYTES_PER_S = 8e12
RTOL = 1e-5
SPSV_SIZE, SPSV_PREP, SPSV_COMPUTE = 1, 2, 3           # rocsparse_spsv_stage_*
FILL_MODE, DIAG_TYPE = 0, 1                            # rocsparse_spmat_attribute


def window(fn, min_s):
    """Mean seconds per call over a window of at least min_s (at least two calls), the device idle before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 2:
            return dt / n


def spread(v):
    return round((max(v) - min(v)) / statistics.median(v), 4)


def row_index(rp):
    return torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), (rp[1:] - rp[:-1]).long())


def copied(h, dev):
    rp = torch.empty(h.rows + 1, dtype=torch.int32, device=dev)
    ci = torch.empty(h.nnz, dtype=torch.int32, device=dev)
    va = torch.empty(h.nnz, dtype=torch.float32, device=dev)
    h.copy_arrays(rp, ci, va)
    torch.cuda.synchronize()
    return rp, ci, va


def workloads(capi, W, dev):
    """name -> callable that gives (rows, device row_ptr, col_idx, vals)."""
    def stencil():
        n, rp, ci, va = W.stencil7(200)
        return n, torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), torch.from_numpy(va).to(dev)

    def config2(band):
        def make():
            w = W.config("c2", band=band)
            rp = W.row_ptr(w)
            nnz = int(rp[-1])
            d_rp = torch.from_numpy(rp).to(dev)
            d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
            d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
            capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
            A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
            eye = capi.CsrMatrix.from_device(w.rows, w.cols, torch.arange(w.rows + 1, dtype=torch.int32, device=dev),
                                             torch.arange(w.rows, dtype=torch.int32, device=dev), torch.ones(w.rows, device=dev))
            S = A.add(eye, 1.0, 64.0, "union")               # the diagonal a synthetic workload lacks
            out = (w.rows,) + copied(S, dev)
            for h in (S, eye, A):
                h.close()
            return out
        return make
    return {"stencil7(200)": stencil, "c2 band 8192 + 64 I": config2(8192), "c2 uniform + 64 I": config2(0)}


class Spsv:
    """rocsparse_spsv on device CSR arrays through ctypes, preprocess and compute apart."""

    def __init__(self, rows, nnz, rp, ci, va, b, x, upper):
        from vendor_compare import F32, I32, RocSparse
        self.rs = RocSparse()
        L = self.L = self.rs.L
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        L.rocsparse_spmat_set_attribute.argtypes = [vp, i32, vp, ctypes.c_size_t]
        L.rocsparse_spsv.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t), vp]
        ok = self.rs._ok
        ok(L.rocsparse_set_stream(self.rs.h, vp(torch.cuda.current_stream().cuda_stream)), "set_stream")
        self.mat, self.vb, self.vx = vp(), vp(), vp()
        ok(L.rocsparse_create_csr_descr(ctypes.byref(self.mat), rows, rows, nnz, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), I32, I32, 0, F32),
           "create_csr")
        fill, diag = i32(1 if upper else 0), i32(0)
        ok(L.rocsparse_spmat_set_attribute(self.mat, FILL_MODE, ctypes.byref(fill), ctypes.sizeof(fill)), "fill mode")
        ok(L.rocsparse_spmat_set_attribute(self.mat, DIAG_TYPE, ctypes.byref(diag), ctypes.sizeof(diag)), "diag type")
        ok(L.rocsparse_create_dnvec_descr(ctypes.byref(self.vb), rows, b.data_ptr(), F32), "dnvec b")
        ok(L.rocsparse_create_dnvec_descr(ctypes.byref(self.vx), rows, x.data_ptr(), F32), "dnvec x")
        self.F32 = F32
        self.one = ctypes.c_float(1.0)
        self.size = ctypes.c_size_t(0)
        ok(self.stage(SPSV_SIZE, None), "spsv buffer_size")
        self.buf = torch.empty(max(int(self.size.value), 16), dtype=torch.uint8, device=x.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok(self.stage(SPSV_PREP, self.buf.data_ptr()), "spsv preprocess")
        torch.cuda.synchronize()
        self.prep_ms = (time.perf_counter() - t0) * 1e3

    def stage(self, stage, buf):
        return self.L.rocsparse_spsv(self.rs.h, 111, ctypes.byref(self.one), self.mat, self.vb, self.vx, self.F32, 0, stage,
                                     ctypes.byref(self.size), buf)

    def compute(self):
        self.rs._ok(self.stage(SPSV_COMPUTE, self.buf.data_ptr()), "spsv compute")

    def close(self):
        self.L.rocsparse_destroy_dnvec_descr(self.vb)
        self.L.rocsparse_destroy_dnvec_descr(self.vx)
        self.L.rocsparse_destroy_spmat_descr(self.mat)
        self.rs.close()


def bound(rp, ci, va, b, x, upper):
    """RTOL * (|b_i| + sum |v x|) / |d_i| per row, with torch's elementwise kernels."""
    row = row_index(rp)
    c = ci.long()
    term = (c > row) if upper else (c < row)
    mag = b.abs().double()
    mag.index_add_(0, row[term], (va[term].abs() * x[c[term]].abs()).double())
    d = torch.zeros_like(mag)
    d.index_add_(0, row[c == row], va[c == row].abs().double())
    return RTOL * mag / d


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trsv.jsonl"))
    ap.add_argument("--sweep-out", default=str(ROOT / "profiles" / "trsv_thin_sweep.jsonl"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--thin", default="")
    ap.add_argument("--no-rocsparse", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    if capi.device_count() < 1:
        print("trsv_time needs a HIP device", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    only = [s for s in args.only.split(",") if s]
    thins = [int(s) for s in args.thin.split(",") if s]
    out = Path(args.sweep_out if thins else args.out)
    lines, ok = [], True
    med = statistics.median
    min_s = args.window_ms / 1e3
    for name, make in workloads(capi, W, dev).items():
        if only and not any(o in name for o in only):
            continue
        rows, rp, ci, va = make()
        A = capi.CsrMatrix.from_device(rows, rows, rp, ci, va)
        b = torch.ones(rows, device=dev)
        x = torch.empty(rows, device=dev)
        row = row_index(rp)
        for uplo in ("lower", "upper"):
            nnz_tri = int(((ci.long() >= row) if uplo == "upper" else (ci.long() <= row)).sum())
            floor = (4 * (rows + 1) + 8 * nnz_tri + 8 * rows) / HBM_BYTES_PER_S * 1e3
            for thin in thins or [0]:
                t_plan = []
                for _ in range(1 if thins else 3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    A.trsv_plan(uplo, thin_rows=thin)
                    t_plan.append((time.perf_counter() - t0) * 1e3)
                info = A.trsv_plan_info(uplo)
                line = {"workload": name, "uplo": uplo, "rows": rows, "nnz": A.nnz, "nnz_triangle": nnz_tri, **info,
                        "plan_bytes": A.trsv_plan_bytes(uplo), "plan_ms": round(med(t_plan), 3)}
                A.trsv(b, x, uplo=uplo)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    A.trsv(b, x, uplo=uplo)
                g.replay()
                torch.cuda.synchronize()
                ours = x.clone()
                spsv = None
                if not thins and not args.no_rocsparse:
                    xr = torch.empty_like(x)
                    try:
                        spsv = Spsv(rows, A.nnz, rp, ci, va, b, xr, uplo == "upper")
                        spsv.compute()
                        torch.cuda.synchronize()
                        line["rocsparse_prep_ms"] = round(spsv.prep_ms, 3)
                        line["rocsparse_close"] = bool(((xr - ours).abs().double() <= bound(rp, ci, va, b, ours, uplo == "upper")).all())
                        ok = ok and line["rocsparse_close"]
                    except (RuntimeError, OSError, AttributeError) as e:
                        line["rocsparse_error"] = str(e).splitlines()[0][:200]
                        spsv = None
                t_solve, t_graph, t_rs = [], [], []
                for _ in range(args.windows):
                    t_solve.append(window(lambda: A.trsv(b, x, uplo=uplo), min_s) * 1e3)
                    t_graph.append(window(g.replay, min_s) * 1e3)
                    if spsv is not None:
                        t_rs.append(window(spsv.compute, min_s) * 1e3)
                line.update({"solve_ms": round(med(t_solve), 4), "solve_spread": spread(t_solve), "graph_ms": round(med(t_graph), 4),
                             "graph_spread": spread(t_graph), "us_per_launch": round(med(t_graph) * 1e3 / max(info["launches"], 1), 3),
                             "floor_ms": round(floor, 4), "over_floor": round(med(t_graph) / floor, 1), "window_ms": args.window_ms,
                             "windows": args.windows})
                if t_rs:
                    line.update({"rocsparse_ms": round(med(t_rs), 4), "rocsparse_spread": spread(t_rs),
                                 "vendor_ratio": round(med(t_graph) / med(t_rs), 2)})
                if spsv is not None:
                    spsv.close()
                del g
                print(json.dumps(line), flush=True)
                lines.append(line)
                out.parent.mkdir(parents=True, exist_ok=True)
                out.write_text("".join(json.dumps(l) + "\n" for l in lines))
        A.close()
        del rp, ci, va, b, x, row
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
