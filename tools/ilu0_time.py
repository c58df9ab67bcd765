#!/usr/bin/env python3
"""tools/ilu0_time.py [--out FILE] [--window-ms 100] [--windows 5] [--only NAME,...] [--no-rocsparse] [--no-krylov] --
spmv_csr_ilu0 against its traffic floor and against rocsparse_scsrilu0, and the Krylov solvers with and without the factor.

Workloads, those of tools/trsv_time.py: stencil7(200) (8 000 000 rows, 598 levels), and config 2 with band 8192 and with uniform
columns, given a dominant diagonal through spmv_csr_add(A, I, 1, 64, UNION).  One JSON line per workload:

  levels, launches, widest, thin_rows, level_cap, plan_bytes   the lower plan's report (launches: its steps + the pivot reset)
  first_ms         spmv_csr_ilu0: a host clock around the synchronous call (the check, the copies, both trsv plans, the factor)
  values_ms        one spmv_csr_ilu0_values as enqueued: launches from the host, between two device synchronisations
  graph_ms         the same captured once in a graph and replayed; us_per_launch = graph_ms / launches
  stream_gbs       the measured rate of a device copy of 1 GiB (bytes read + bytes written per second)
  floor_ms         the traffic floor at that rate: A read once (4 (rows + 1) + 8 nnz bytes) and M written once (4 nnz);
                   over_floor = graph_ms / floor_ms
  pivot            spmv_csr_ilu0_pivot (-1: none)
  rocsparse_analysis_ms, rocsparse_ms   rocsparse_scsrilu0 on the same arrays: the analysis once, the compute in the same
                   windows.  It factors in place, so a window times (copy of A's values + compute) and a second one the copy
                   alone; rocsparse_ms is the difference.  vendor_ratio = graph_ms / rocsparse_ms
  rocsparse_close  on 2000 sampled rows both factors meet the host test's bound (tests/test_ilu0_host.py (a)): |(L U)_ij - a_ij|
                   <= max(1e-5, (terms + 2) 2^-24) (|a_ij| + sum |l_ik u_kj|) in float64; rocsparse_max_rel_diff is the largest
                   |ours - theirs| / |ours| over all entries
  rocsparse_error  instead, what the binding or the library refused with
  krylov           solver, iterations, converged and wall time to ||r|| <= 1e-5 ||b|| (b standard normal, x = 0; the second of
                   two solves, the first warms up), without and with M: PCG on the symmetric stencil (6 / -1 on stencil7(200)'s
                   pattern, its own factor), BiCGStab on the uniform config
  *_spread         (max - min) / median over the windows

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
from trsv_time import spread, window, workloads  # noqa: E402

RTOL = 1e-5


class Csrilu0:
    """rocsparse_scsrilu0 on device CSR arrays through ctypes, analysis and compute apart; `vals` is factored in place."""

    def __init__(self, rows, nnz, rp, ci, vals):
        from vendor_compare import RocSparse
        self.rs = RocSparse()
        L = self.L = self.rs.L
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        L.rocsparse_create_mat_descr.argtypes = [ctypes.POINTER(vp)]
        L.rocsparse_destroy_mat_descr.argtypes = [vp]
        L.rocsparse_create_mat_info.argtypes = [ctypes.POINTER(vp)]
        L.rocsparse_destroy_mat_info.argtypes = [vp]
        L.rocsparse_scsrilu0_buffer_size.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_size_t)]
        L.rocsparse_scsrilu0_analysis.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp]
        L.rocsparse_scsrilu0.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
        ok = self.rs._ok
        ok(L.rocsparse_set_stream(self.rs.h, vp(torch.cuda.current_stream().cuda_stream)), "set_stream")
        self.descr, self.info = vp(), vp()
        ok(L.rocsparse_create_mat_descr(ctypes.byref(self.descr)), "create_mat_descr")
        ok(L.rocsparse_create_mat_info(ctypes.byref(self.info)), "create_mat_info")
        self.args = (rows, nnz, self.descr, vals.data_ptr(), rp.data_ptr(), ci.data_ptr(), self.info)
        size = ctypes.c_size_t(0)
        ok(L.rocsparse_scsrilu0_buffer_size(self.rs.h, *self.args, ctypes.byref(size)), "csrilu0 buffer_size")
        self.buf = torch.empty(max(int(size.value), 16), dtype=torch.uint8, device=vals.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok(L.rocsparse_scsrilu0_analysis(self.rs.h, *self.args, 0, 0, self.buf.data_ptr()), "csrilu0 analysis")   # policies: reuse, auto
        torch.cuda.synchronize()
        self.analysis_ms = (time.perf_counter() - t0) * 1e3

    def compute(self):
        self.rs._ok(self.L.rocsparse_scsrilu0(self.rs.h, *self.args, 0, self.buf.data_ptr()), "csrilu0")

    def close(self):
        self.L.rocsparse_destroy_mat_info(self.info)
        self.L.rocsparse_destroy_mat_descr(self.descr)
        self.rs.close()


def meets_the_bound(rp, ci, va, M, rows_sample):
    """Whether |(L U)_ij - a_ij| <= max(RTOL, (terms + 2) 2^-24) (|a_ij| + sum |l u|) at every stored entry of the sampled rows
    (host arrays; float64)."""
    M = M.astype(np.float64)
    for i in rows_sample:
        lo, hi = rp[i], rp[i + 1]
        cols = ci[lo:hi]
        acc, mag, cnt = np.zeros(hi - lo), np.zeros(hi - lo), np.zeros(hi - lo)
        for t in np.flatnonzero(cols < i):
            k = cols[t]
            krow = ci[rp[k]:rp[k + 1]]
            d = rp[k] + int(np.searchsorted(krow, k))
            q = np.arange(d, rp[k + 1])
            at = np.searchsorted(cols, ci[q])
            hit = at < cols.size
            hit[hit] = cols[at[hit]] == ci[q][hit]
            acc[at[hit]] += M[lo + t] * M[q[hit]]
            mag[at[hit]] += np.abs(M[lo + t] * M[q[hit]])
            cnt[at[hit]] += 1
        up = np.flatnonzero(cols >= i)
        acc[up] += M[lo + up]
        mag[up] += np.abs(M[lo + up])
        cnt[up] += 1
        a = va[lo:hi].astype(np.float64)
        if not np.all(np.abs(acc - a) <= np.maximum(RTOL, (cnt + 2) * 2.0 ** -24) * (np.abs(a) + mag)):
            return False
    return True


def solve_time(solver, A, b, M, maxiter):
    """The second of two solves from x = 0 (the first plans A and warms torch's kernels up), on the first one's state."""
    state = None
    for _ in range(2):
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = solver(A, b, x, M=M, tol=1e-5, maxiter=maxiter, state=state)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        state = res.state
    return {"iterations": res.iterations, "converged": res.converged, "ms": round(ms, 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ilu0.jsonl"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-rocsparse", action="store_true")
    ap.add_argument("--no-krylov", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, W, solvers = pkg.capi, pkg.workloads, pkg.solvers
    if capi.device_count() < 1:
        print("ilu0_time needs a HIP device", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    only = [s for s in args.only.split(",") if s]
    out = Path(args.out)
    lines, ok = [], True
    med = statistics.median
    min_s = args.window_ms / 1e3
    big = torch.empty(1 << 28, dtype=torch.float32, device=dev), torch.empty(1 << 28, dtype=torch.float32, device=dev)
    big[0].zero_()
    t_copy = med([window(lambda: big[1].copy_(big[0]), min_s) for _ in range(3)])
    stream_rate = 2 * big[0].numel() * 4 / t_copy
    del big
    torch.cuda.empty_cache()
    for name, make in workloads(capi, W, dev).items():
        if only and not any(o in name for o in only):
            continue
        rows, rp, ci, va = make()
        A = capi.CsrMatrix.from_device(rows, rows, rp, ci, va)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = A.ilu0()
        first_ms = (time.perf_counter() - t0) * 1e3
        info = M.trsv_plan_info("lower")
        launches = info["launches"] + 1
        floor = (4 * (rows + 1) + 12 * A.nnz) / stream_rate * 1e3
        line = {"workload": name, "rows": rows, "nnz": A.nnz, "levels": info["levels"], "launches": launches, "widest": info["widest"],
                "thin_rows": info["thin_rows"], "level_cap": info["level_cap"], "plan_bytes": M.ilu0_plan_bytes(),
                "first_ms": round(first_ms, 3), "pivot": M.ilu0_pivot()}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            M.ilu0_values(A)
        g.replay()
        torch.cuda.synchronize()
        ours = torch.empty_like(va)
        M.copy_arrays(None, None, ours)
        torch.cuda.synchronize()
        rs, theirs = None, None
        if not args.no_rocsparse:
            try:
                theirs = va.clone()
                rs = Csrilu0(rows, A.nnz, rp, ci, theirs)
                rs.compute()
                torch.cuda.synchronize()
                line["rocsparse_analysis_ms"] = round(rs.analysis_ms, 3)
                line["rocsparse_max_rel_diff"] = float(((theirs - ours).abs() / ours.abs().clamp_min(1e-30)).max())
                sample = np.random.default_rng(1).choice(rows, min(2000, rows), replace=False)
                h_rp, h_ci, h_va = rp.cpu().numpy().astype(np.int64), ci.cpu().numpy(), va.cpu().numpy()
                line["rocsparse_close"] = bool(meets_the_bound(h_rp, h_ci, h_va, ours.cpu().numpy(), sample)
                                               and meets_the_bound(h_rp, h_ci, h_va, theirs.cpu().numpy(), sample))
                del h_rp, h_ci, h_va
                ok = ok and line["rocsparse_close"]
            except (RuntimeError, OSError, AttributeError) as e:
                line["rocsparse_error"] = str(e).splitlines()[0][:200]
                rs = None
        t_values, t_graph, t_rs, t_cp = [], [], [], []

        def vendor():
            theirs.copy_(va)
            rs.compute()

        for _ in range(args.windows):
            t_values.append(window(lambda: M.ilu0_values(A), min_s) * 1e3)
            t_graph.append(window(g.replay, min_s) * 1e3)
            if rs is not None:
                t_rs.append(window(vendor, min_s) * 1e3)
                t_cp.append(window(lambda: theirs.copy_(va), min_s) * 1e3)
        line.update({"values_ms": round(med(t_values), 4), "values_spread": spread(t_values), "graph_ms": round(med(t_graph), 4),
                     "graph_spread": spread(t_graph), "us_per_launch": round(med(t_graph) * 1e3 / launches, 3),
                     "stream_gbs": round(stream_rate / 1e9, 1), "floor_ms": round(floor, 4), "over_floor": round(med(t_graph) / floor, 1),
                     "window_ms": args.window_ms, "windows": args.windows})
        if t_rs:
            rs_ms = med(t_rs) - med(t_cp)
            line.update({"rocsparse_ms": round(rs_ms, 4), "rocsparse_spread": spread(t_rs), "vendor_ratio": round(med(t_graph) / rs_ms, 2)})
        if rs is not None:
            rs.close()
        del g, theirs
        if not args.no_krylov and name.startswith(("stencil7", "c2 uniform")):
            b = torch.from_numpy(np.random.default_rng(2026).standard_normal(rows).astype(np.float32)).to(dev)
            if name.startswith("stencil7"):                    # the symmetric stencil: 6 on the diagonal, -1 off it, and its own factor
                row = torch.repeat_interleave(torch.arange(rows, device=dev), (rp[1:] - rp[:-1]).long())
                va.copy_(torch.where(ci.long() == row, 6.0, -1.0))
                del row
                M.ilu0_values(A)
                solver, label = solvers.pcg, "pcg"
            else:
                solver, label = solvers.bicgstab, "bicgstab"
            line["krylov"] = {"solver": label, "plain": solve_time(solver, A, b, None, 5000), "ilu0": solve_time(solver, A, b, M, 5000)}
            del b
        M.close()
        A.close()
        print(json.dumps(line), flush=True)
        lines.append(line)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(l) + "\n" for l in lines))
        del rp, ci, va, ours
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
