#!/usr/bin/env python3
"""tools/select_time.py [--out FILE] [--window-ms 100] [--windows 5] -- spmv_csr_select_* against the route a user has without it.

Workloads: configs 2 and 3 with band 8192 and with uniform columns, random normal scores.  Calls: select_topk at k = 4, 8, 16
and at k >= the longest row (the copy case), select_threshold at 0 (keeps about half).  One JSON line per (workload, call):

  call_ms         the whole call: allocation, launches and the wait included (a host clock around the synchronous call)
  call_destroy_ms the call and spmv_csr_destroy of its result (the torch route frees into torch's caching allocator)
  stream_ms       device events on the stream around the call: the kernels, the scan's read-back and the allocations between
                  them (no profiler: the kernels alone are not separated from the gaps between them)
  floor_ms        the traffic formula of DESIGN.md section 25 at 8 TB/s
  torch_ms        the torch route on the device: one stable sort of nnz composite keys (row << 32 | descending score key), rank
                  within the row, mask, nonzero, index-select, bincount + cumsum; row_of is made outside the timing
  *_spread        (max - min) / median over the windows

Both sides run in the same process in alternating windows of at least --window-ms; a window's figure is its mean call.  The
torch result is compared with the library's once per line (row_ptr, col_idx and vals equal).  Needs a device."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

HBM_BYTES_PER_S = 8e12


def traffic_bytes(rows, nnz, kept, topk):
    """the scores once per phase that reads them, row_ptr per launch, the cuts written and read, the
    counts written, scanned (read and written) and read, col_idx and vals of the kept nonzeros, 12 bytes written per kept."""
    phases = 2
    b = phases * 4 * nnz + phases * 4 * rows + 4 * rows * 4 + kept * (8 + 12)
    if topk:
        b += 2 * 8 * rows
    return b


def torch_route(rp_long, row_of, ci, va, score, k=None, thr=None):
    nnz = score.numel()
    if k is not None:
        u = score.view(torch.int32).long() & 0xFFFFFFFF
        key = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
        comp = (row_of << 32) | (0xFFFFFFFF - key)
        order = torch.sort(comp, stable=True).indices
        rank = torch.arange(nnz, device=score.device) - rp_long[row_of]
        keep = torch.zeros(nnz, dtype=torch.bool, device=score.device)
        keep[order[rank < k]] = True
    else:
        keep = score >= thr
    pos = keep.nonzero().squeeze(1)
    new_rp = torch.zeros(rp_long.numel(), dtype=torch.int64, device=score.device)
    new_rp[1:] = torch.cumsum(torch.bincount(row_of[pos], minlength=rp_long.numel() - 1), 0)
    return new_rp.int(), ci[pos], va[pos]


def window(fn, min_s, after=None):
    """Mean seconds per call over a window of at least min_s (at least two calls).  after(result): what follows a call
    (destroying its result); returns (mean of fn alone, mean of fn and after)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, alone = 0, 0.0
    while True:
        t1 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        alone += time.perf_counter() - t1
        if after is not None:
            after(r)
        del r
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 2:
            return alone / n, dt / n


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "select.jsonl"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--configs", default="c2,c3")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    if capi.device_count() < 1:
        print("select_time needs a HIP device", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    lines = []
    for cfg in args.configs.split(","):
        for band in (8192, 0):
            w = W.config(cfg, band=band)
            rp = W.row_ptr(w)
            nnz = int(rp[-1])
            d_rp = torch.from_numpy(rp).to(dev)
            d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
            d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
            capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
            A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
            score = torch.randn(nnz, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
            rp_long = d_rp.long()
            row_of = torch.repeat_interleave(torch.arange(w.rows, device=dev), rp_long[1:] - rp_long[:-1])
            longest = int(np.diff(rp).max())
            calls = [(f"topk k={k}", dict(k=k)) for k in (4, 8, 16)] + [(f"topk k={longest} (copy)", dict(k=longest)), ("threshold 0", dict(thr=0.0))]
            for label, kw in calls:
                topk = "k" in kw

                def ours(keep=False):
                    s = A.select_topk(kw["k"], score) if topk else A.select_threshold(kw["thr"], score)
                    if keep:
                        return s
                    s.close()

                def theirs():
                    return torch_route(rp_long, row_of, d_ci, d_va, score, **kw)

                sel = ours(keep=True)                                  # warm, and the two results side by side
                t_rp, t_ci, t_va = theirs()
                g_rp = torch.empty(w.rows + 1, dtype=torch.int32, device=dev)
                g_ci = torch.empty(sel.nnz, dtype=torch.int32, device=dev)
                g_va = torch.empty(sel.nnz, dtype=torch.float32, device=dev)
                sel.copy_arrays(g_rp, g_ci, g_va)
                torch.cuda.synchronize()
                kept = sel.nnz
                same = bool(torch.equal(g_rp, t_rp) and torch.equal(g_ci, t_ci) and torch.equal(g_va.view(torch.int32), t_va.view(torch.int32)))
                sel.close()
                del t_rp, t_ci, t_va, g_rp, g_ci, g_va
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                spans = []
                for _ in range(5):
                    e0.record()
                    s = ours(keep=True)
                    e1.record()
                    s.close()
                    torch.cuda.synchronize()
                    spans.append(e0.elapsed_time(e1))
                a, b = [], []
                a_close = []
                for _ in range(args.windows):
                    alone, both = window(lambda: ours(keep=True), args.window_ms / 1e3, after=lambda s: s.close())
                    a.append(alone * 1e3)
                    a_close.append(both * 1e3)
                    b.append(window(theirs, args.window_ms / 1e3)[1] * 1e3)
                med = statistics.median
                line = {"workload": w.name, "band": band, "rows": w.rows, "nnz": nnz, "call": label, "kept": kept,
                        "call_ms": round(med(a), 4), "call_spread": round((max(a) - min(a)) / med(a), 4),
                        "call_destroy_ms": round(med(a_close), 4), "stream_ms": round(med(spans), 4),
                        "floor_ms": round(traffic_bytes(w.rows, nnz, kept, topk) / HBM_BYTES_PER_S * 1e3, 4),
                        "torch_ms": round(med(b), 4), "torch_spread": round((max(b) - min(b)) / med(b), 4),
                        "call_destroy_spread": round((max(a_close) - min(a_close)) / med(a_close), 4),
                        "speedup": round(med(b) / med(a), 3), "speedup_with_destroy": round(med(b) / med(a_close), 3),
                        "same_result": same,
                        "window_ms": args.window_ms, "windows": args.windows}
                print(json.dumps(line), flush=True)
                lines.append(line)
            A.close()
            del score, row_of, rp_long, d_rp, d_ci, d_va
            torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))
    return 0 if all(l["same_result"] for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
