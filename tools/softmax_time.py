#!/usr/bin/env python3
"""tools/softmax_time.py -- spmv_csr_row_softmax and spmv_csr_row_softmax_backward against a pure stream of the same size.

One JSON line per (workload, direction): the time, the algorithmic bytes (forward one read and one write of nnz floats,
8 nnz; backward two reads and one write, 12 nnz; plus row_ptr, 4 (rows + 1)) and their share of 8 TB/s, and as the
yardstick on the same box the time of torch.mul over nnz floats (out = 0.5 * x: 8 bytes per element and nothing else; for
backward torch.mul of two arrays, 12 bytes per element).  Rows of more than 512 nonzeros are read three times forward
and twice backward; the line carries the share of the nonzeros that lie in such rows.
Times: HIP events, warmed up, median of --reps windows of --iters launches.

    python tools/softmax_time.py [--workloads c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0] [--out profiles/softmax_sweep.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
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
        lengths = np.diff(rp)
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
        A.spmm_plan()
        gen = torch.Generator(device=dev).manual_seed(nnz % 1000)
        scores = torch.randn(nnz, generator=gen, device=dev)
        dP = torch.randn(nnz, generator=gen, device=dev)
        P = torch.empty_like(scores)
        dS = torch.empty_like(scores)
        common = dict(workload=f"{name}_band{band}", rows=w.rows, cols=w.cols, nnz=nnz, plan=A.spmm_describe(),
                      nnz_share_in_long_rows=round(float(lengths[lengths > 512].sum()) / max(nnz, 1), 4))
        ms = timed(lambda: A.row_softmax(scores, P, 0.125), a.iters, a.reps)
        mul = timed(lambda: torch.mul(scores, 0.5, out=dS), a.iters, a.reps)
        B = 8 * nnz + 4 * (w.rows + 1)
        emit(direction="forward", softmax_ms=round(ms, 4), algorithmic_bytes=B, frac_of_8TBs=round(B / (ms * 1e-3) / PEAK_BPS, 3),
             torch_mul_ms=round(mul, 4), softmax_over_mul=round(ms / mul, 3), **common)
        ms = timed(lambda: A.row_softmax_backward(P, dP, dS, 0.125), a.iters, a.reps)
        mul = timed(lambda: torch.mul(P, dP, out=dS), a.iters, a.reps)
        B = 12 * nnz + 4 * (w.rows + 1)
        emit(direction="backward", softmax_ms=round(ms, 4), algorithmic_bytes=B, frac_of_8TBs=round(B / (ms * 1e-3) / PEAK_BPS, 3),
             torch_mul_ms=round(mul, 4), softmax_over_mul=round(ms / mul, 3), **common)
        A.close()
        del d_rp, d_ci, d_va, scores, dP, P, dS
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
