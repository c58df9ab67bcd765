#!/usr/bin/env python3
"""tools/spmv_vals16_time.py -- spmv_csr_run_vals16 (bf16 / fp16 matrix values) against spmv_csr_run (fp32 values) under SPMV_TILED.

Both calls run on ONE handle and ONE plan (the plan is a function of the pattern), in one process, in windows that alternate
between them, so that a drift of the device's clocks falls on both alike.  Times: HIP events, the median of --reps windows of
--iters launches each after one window of each side that is thrown away (the clocks ramp up in it); --iters grows to what
fills --window-ms, so that a window of a small matrix is not a measurement of the event pair.  Before the clocks start the
handle's borrowed fp32 values are overwritten with the 16-bit values widened (vals are read live), and y of the 16-bit call
is compared, bit for bit, with y of the fp32 call on them: the contract of include/spmv_hip.h at the timed size.

One JSON line per (workload, dtype): the plan string, both medians, their ratio, the spread of each side's windows
((max - min) / median: what a ratio has to be read against), whether the 16-bit call is not faster than the fp32 call beyond
twice the larger spread, the bytes per nonzero each side streams -- columns plus values, weighted over the plan's chunks: a
chunk with 16-bit columns streams 2 + 4 (fp32 values) or 2 + 2 bytes, a sorted or 32-bit chunk 4 + 4 or 4 + 2 -- and the
bit check.  Appended to profiles/spmv_vals16.jsonl unless --out names another file.

    python tools/spmv_vals16_time.py [--workloads c4:8192,c4:65536,c3:8192,c2:8192,stencil:200] [--dtype bf16,fp16]

Default workloads: config 4 with bands of 8192 and 65 536 columns, configs 3 and 2 with band 8192 and the 7-point stencil on
200^3 unknowns: between them the 16-bit body, the sorted and the mixed launch and the block lists.
"""
import argparse
import json
import re
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from spmm_time import interleaved  # noqa: E402

OUT = ROOT / "profiles" / "spmv_vals16.jsonl"
DTYPES = {"bf16": "bfloat16", "fp16": "float16"}


def _field(plan, name):
    m = re.search(rf"\b{name}=(\d+)", plan)
    return int(m.group(1)) if m else 0


def stream_bytes_per_nnz(plan, value_bytes):
    """Column plus value bytes per nonzero of a TILED run, weighted over the plan's chunks (the ragged last chunk as a whole one)."""
    chunks, c16 = _field(plan, "chunks"), _field(plan, "col16_chunks")
    if not chunks:
        return 0.0
    return round((c16 * (2 + value_bytes) + (chunks - c16) * (4 + value_bytes)) / chunks, 3)


def problem(spec, capi, W, dev):
    """(label, rows, cols, device row_ptr, col_idx, fp32 values, x) of `name:band` or `stencil:n`."""
    import numpy as np
    import torch
    name, arg = spec.split(":")
    if name == "stencil":
        n = int(arg)
        N, rp, ci, va = W.stencil7(n)
        x = np.random.Generator(np.random.PCG64(n)).uniform(-1, 1, size=N).astype(np.float32)
        d_rp, d_ci, d_va, d_x = (torch.from_numpy(a).to(dev) for a in (rp, ci, va, x))
        # (the stencil's own values are a few small integers, all bf16 numbers: general values, so that the conversion rounds)
        d_va = torch.randn(len(ci), generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        return f"stencil7_{n}^3", N, N, d_rp, d_ci, d_va, d_x
    w = W.config(name, band=int(arg))
    rp = W.row_ptr(w)
    nnz = int(rp[-1])
    d_rp = torch.from_numpy(rp).to(dev)
    d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
    d_x = torch.empty(w.cols, dtype=torch.float32, device=dev)
    capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
    capi.synth_x(w.seed, 0, w.cols, d_x)
    return f"{name}_band{arg}", w.rows, w.cols, d_rp, d_ci, d_va, d_x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c4:8192,c4:65536,c3:8192,c2:8192,stencil:200")
    ap.add_argument("--dtype", default="bf16,fp16")
    ap.add_argument("--iters", type=int, default=20, help="launches per window, at least")
    ap.add_argument("--window-ms", type=float, default=100.0, help="a window lasts at least this long")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    dev = torch.device("cuda:0")
    dtypes = a.dtype.split(",")
    if any(d not in DTYPES for d in dtypes):
        ap.error("--dtype lists bf16, fp16")
    with open(a.out, "a") as out:
        for spec in a.workloads.split(","):
            label, rows, cols, d_rp, d_ci, d_va, d_x = problem(spec, capi, W, dev)
            nnz = d_ci.numel()
            master = d_va.clone()                                   # the fp32 values every dtype is converted from
            A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
            A.plan(capi.TILED)
            plan = A.plan_describe(capi.TILED)
            y32 = torch.empty(rows, dtype=torch.float32, device=dev)
            y16 = torch.empty(rows, dtype=torch.float32, device=dev)
            for d in dtypes:
                v16 = master.to(getattr(torch, DTYPES[d]))          # to nearest even
                d_va.copy_(v16)                                     # widened exactly, into the array the handle reads live
                rounded = int((d_va != master).sum())
                y32.fill_(float("nan")), y16.fill_(float("nan"))
                A.run(capi.TILED, d_x, y32)
                A.run_vals16(capi.TILED, v16, d_x, y16)
                torch.cuda.synchronize()
                same = bool(torch.equal(y32.view(torch.int32), y16.view(torch.int32))) and not bool(torch.isnan(y16).any())
                calls = {"fp32": lambda: A.run(capi.TILED, d_x, y32), d: lambda: A.run_vals16(capi.TILED, v16, d_x, y16)}
                first = interleaved(calls, a.iters, 1)               # thrown away; sizes the windows
                iters = max(a.iters, int(a.window_ms / max(first["fp32"][0], 1e-4)) + 1)
                win = interleaved(calls, iters, a.reps)
                med = {n: statistics.median(v) for n, v in win.items()}
                spread = {n: (max(v) - min(v)) / med[n] for n, v in win.items()}
                row = dict(call="spmv_csr_run_vals16", workload=label, dtype=d, rows=rows, cols=cols, nnz=nnz, variant="tiled", plan=plan,
                           iters=iters, reps=a.reps, fp32_ms=round(med["fp32"], 4), vals16_ms=round(med[d], 4),
                           vals16_over_fp32=round(med[d] / med["fp32"], 3), fp32_spread=round(spread["fp32"], 4),
                           vals16_spread=round(spread[d], 4),
                           not_faster_beyond_twice_the_spread=bool(med[d] > med["fp32"] * (1 - 2 * max(spread.values()))),
                           fp32_stream_bytes_per_nnz=stream_bytes_per_nnz(plan, 4), vals16_stream_bytes_per_nnz=stream_bytes_per_nnz(plan, 2),
                           values_rounded=rounded, same_bits_as_fp32_on_widened=same)
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                del v16
            A.close()
            del d_rp, d_ci, d_va, d_x, master, y32, y16
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
