#!/usr/bin/env python3
"""tools/attention_time.py -- FusedSparseAttention against the composed SparseAttention on the same pattern arrays, in one process.

One JSON line per (workload, k = kv): the forward time and the forward-plus-backward time of both holders (HIP events,
warmed up, the two holders' windows alternating, median of --reps windows of enough calls to fill --window-ms), their ratios
fused / composed (below 1: the fused path is faster), and what torch.cuda.max_memory_allocated rises by over one
forward-plus-backward step of each.  The composed holder is sparse_attention.SparseAttention as it stands (SDDMM, row softmax,
SpMM, transpose_values), so it is the yardstick; nothing here sets a threshold.

    python tools/attention_time.py [--workloads c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0] [--ks 16,32,64] [--scale c4=1.0]
                                   [--out profiles/attention_sweep.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed_pair(fa, fb, window_ms, reps, max_iters):
    """Medians of `reps` windows of fa and of fb, alternating; the windows hold the same number of calls."""
    for _ in range(2):
        fa()
        fb()
    one = max(window(fa, 1), window(fb, 1))
    iters = max(1, min(max_iters, int(window_ms / one)))
    a, b = [], []
    for _ in range(reps):
        a.append(window(fa, iters))
        b.append(window(fb, iters))
    return statistics.median(a), statistics.median(b), iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0")
    ap.add_argument("--ks", default="16,32,64")
    ap.add_argument("--scale", default="", help="name=fraction of the rows, e.g. c4=0.5 where the memory does not hold the full size")
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    if capi.device_count() < 1:
        raise SystemExit("attention_time.py needs a HIP device")
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    out = open(a.out, "a") if a.out else None

    def emit(**kv):
        line = json.dumps(kv)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for spec in a.workloads.split(","):
        name, band = spec.split(":")
        w = W.config(name, band=int(band), scale=scales.get(name, 1.0))
        rp = W.row_ptr(w)
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        del d_va
        fused = SA.FusedSparseAttention(w.rows, w.cols, d_rp, d_ci, scale=0.25)
        composed = SA.SparseAttention(w.rows, w.cols, d_rp, d_ci, scale=0.25)
        for k in (int(s) for s in a.ks.split(",")):
            gen = torch.Generator(device=dev).manual_seed(k)
            Q, K, V, dO = (torch.randn((n, k), generator=gen, device=dev) for n in (w.rows, w.cols, w.cols, w.rows))
            q, kk, v = (t.clone().requires_grad_(True) for t in (Q, K, V))

            def forward(att):
                with torch.no_grad():
                    att(Q, K, V)

            def step(att):
                att(q, kk, v).backward(dO)
                q.grad = kk.grad = v.grad = None

            def step_bytes(att):
                step(att)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                step(att)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated() - before

            f_fwd, c_fwd, it_f = timed_pair(lambda: forward(fused), lambda: forward(composed), a.window_ms, a.reps, a.max_iters)
            f_step, c_step, it_s = timed_pair(lambda: step(fused), lambda: step(composed), a.window_ms, a.reps, a.max_iters)
            with torch.no_grad():
                diff = float((fused(Q, K, V) - composed(Q, K, V)).abs().max())
            emit(workload=f"{name}_band{band}", k=k, kv=k, rows=w.rows, cols=w.cols, nnz=nnz, plan=fused.A.spmm_describe(),
                 plan_T=fused.T.spmm_describe(), iters_forward=it_f, iters_step=it_s, reps=a.reps,
                 fused_forward_ms=round(f_fwd, 4), composed_forward_ms=round(c_fwd, 4), forward_ratio=round(f_fwd / c_fwd, 3),
                 fused_step_ms=round(f_step, 4), composed_step_ms=round(c_step, 4), step_ratio=round(f_step / c_step, 3),
                 fused_step_bytes=step_bytes(fused), composed_step_bytes=step_bytes(composed), max_abs_diff_O=diff)
            del Q, K, V, dO, q, kk, v
            torch.cuda.empty_cache()
        fused.close()
        composed.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
