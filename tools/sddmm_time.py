#!/usr/bin/env python3
"""tools/sddmm_time.py -- spmv_csr_sddmm against spmv_csr_spmm on the same handle and k, and torch.sparse.sampled_addmm.

One JSON line per (workload, k): the SDDMM time, the time of spmv_csr_spmm on the same handle with the same k (the same
plan, the same gathers of X rows and the same algorithmic bytes 4 (rows + 1) + 8 nnz + 4 k (rows + cols): SpMM reads
col_idx and vals and writes Y, SDDMM reads col_idx and U and writes out; this change leaves kernels_spmm.hip as it was, so
that is the parent commit's kernel), their ratio, the share of 8 TB/s, and -- where the installed torch runs it on a CSR
tensor on this device -- torch.sparse.sampled_addmm(beta = 0) with its largest difference to our result; where it does
not, the line says why.  Times: HIP events, warmed up, median of --reps windows of --iters launches.

    python tools/sddmm_time.py [--workloads c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0] [--ks 1,4,8,16,32,64] [--out FILE]

--dtype fp32,bf16[,fp16] times spmv_csr_sddmm_16 instead, as tools/spmm_time.py --dtype does for SpMM (its interleaved
windows and its JSON line): the fp32 call and each 16-bit call on the same numbers, alternating in one process; out of the
16-bit call must be, bit for bit, the fp32 call's on the widened operands.  Appended to profiles/spmm_16bit.jsonl unless
--out names another file; the comparisons above are not run in this mode.

--cols 128,256,512 times spmv_csr_sddmm_cols as tools/spmm_time.py --cols does for SpMM (its windows, its JSON line, its
output file): against the loop of narrow calls over the column blocks of 64, which also needs an nnz-sized temporary and one
nnz-sized torch add per further block; out of the call must be, bit for bit, the loop's.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
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
    ap.add_argument("--dtype", default="fp32", help="fp32 (the comparisons of the first paragraph), or fp32,bf16[,fp16]")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cols", default=None, help="widths above 64, e.g. 128,256,512: time spmv_csr_sddmm_cols against the loop of narrow calls")
    ap.add_argument("--lib", default=None, help="--cols: another build of libspmv_hip.so, for an A/B run")
    a = ap.parse_args()
    if a.cols:
        from spmm_time import run_cols
        run_cols("sddmm", a)
        return
    import torch
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    dev = torch.device("cuda:0")
    dtypes = a.dtype.split(",")
    sixteen = [d for d in dtypes if d != "fp32"]
    if sixteen:
        from spmm_time import DTYPES, OUT_16BIT, compare_16bit      # (loads rocSPARSE's bindings, not rocSPARSE)
        if any(d not in DTYPES for d in dtypes) or "fp32" not in dtypes:
            ap.error("--dtype lists fp32 and any of bf16, fp16")
        a.out = a.out or str(OUT_16BIT)
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
            if sixteen:
                U16 = {d: U.to(getattr(torch, DTYPES[d])) for d in sixteen}
                X16 = {d: X.to(getattr(torch, DTYPES[d])) for d in sixteen}
                res16 = torch.empty(nnz, dtype=torch.float32, device=dev)
                same = {}
                for d in sixteen:
                    A.sddmm(U16[d].to(torch.float32), X16[d].to(torch.float32), res)
                    A.sddmm(U16[d], X16[d], res16)
                    torch.cuda.synchronize()
                    same[d] = bool(torch.equal(res.view(torch.int32), res16.view(torch.int32)))
                calls = {"fp32": lambda: A.sddmm(U, X, res)}
                calls.update({d: (lambda d=d: A.sddmm(U16[d], X16[d], res16)) for d in sixteen})
                emit(**compare_16bit("sddmm", label, k, calls, same, a.iters, a.reps))
                del U, X, Y, res, res16, U16, X16
                torch.cuda.empty_cache()
                continue
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
