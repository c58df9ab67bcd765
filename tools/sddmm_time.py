#!/usr/bin/env python3
"""tools/sddmm_time.py -- spmv_csr_sddmm against spmv_csr_spmm on the same handle and k, and torch.sparse.sampled_addmm.

One JSON line per (workload, k): the SDDMM time, the time of spmv_csr_spmm on the same handle with the same k (the same
plan, the same gathers of X rows and the same algorithmic bytes 4 (rows + 1) + 8 nnz + 4 k (rows + cols): SpMM reads
col_idx and vals and writes Y, SDDMM reads col_idx and U and writes out; this change leaves kernels_spmm.hip as it was, so
that is the parent commit's kernel), their ratio, the share of 8 TB/s, and -- where the installed torch runs it on a CSR
tensor on this device -- torch.sparse.sampled_addmm(beta = 0) with its largest difference to our result; where it does
not, the line says why.  Times: HIP events, warmed up, median of --reps windows of --iters launches.

    python tools/sddmm_time.py [--workloads c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0] [--ks 1,4,8,16,32,64] [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

PEAK_BPS = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0")
    ap.add_argument("--ks", default="1,4,8,16,32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip torch.sparse.sampled_addmm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

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
        A.spmm_plan()
        label = f"{name}_band{band}"
        for k in (int(s) for s in a.ks.split(",")):
            gen = torch.Generator(device=dev).manual_seed(k)
            U = torch.randn((w.rows, k), generator=gen, device=dev)
            X = torch.randn((w.cols, k), generator=gen, device=dev)
            Y = torch.empty((w.rows, k), dtype=torch.float32, device=dev)
            res = torch.empty(nnz, dtype=torch.float32, device=dev)
            ms = timed(lambda: A.sddmm(U, X, res), a.iters, a.reps)
            ms_spmm = timed(lambda: A.spmm(X, Y), a.iters, a.reps)
            B = 4 * (w.rows + 1) + 8 * nnz + 4 * k * (w.cols + w.rows)
            row = dict(workload=label, k=k, rows=w.rows, cols=w.cols, nnz=nnz, plan=A.spmm_describe(),
                       sddmm_ms=round(ms, 4), spmm_ms=round(ms_spmm, 4), sddmm_over_spmm=round(ms / ms_spmm, 3),
                       algorithmic_bytes=B, frac_of_8TBs=round(B / (ms * 1e-3) / PEAK_BPS, 3))
            if not a.no_torch:
                try:
                    pattern = torch.sparse_csr_tensor(d_rp, d_ci, torch.zeros_like(d_va), size=(w.rows, w.cols))
                    Xt = X.t()
                    r = torch.sparse.sampled_addmm(pattern, U, Xt, beta=0.0)
                    torch.cuda.synchronize()
                    row.update(torch_sampled_addmm_ms=round(timed(lambda: torch.sparse.sampled_addmm(pattern, U, Xt, beta=0.0),
                                                                  max(1, a.iters // 2), a.reps), 4),
                               torch_max_diff=float((r.values() - res).abs().max()))
                    del pattern, r
                except Exception as e:  # noqa: BLE001 -- whatever torch raises here is the finding
                    row.update(torch_sampled_addmm_error=f"{type(e).__name__}: {str(e)[:200]}")
            emit(**row)
            del U, X, Y, res
            torch.cuda.empty_cache()
        A.close()
        del d_rp, d_ci, d_va
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
