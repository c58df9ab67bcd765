#!/usr/bin/env python3
"""tools/spgemm_time.py [--out FILE] [--window-ms 100] [--windows 5] [--only NAME,...] -- spmv_csr_spgemm against torch.sparse.mm.

Workloads: A A on config 2 with band 8192 and with uniform columns, A A^T on config 2 with band 8192 (A^T from
spmv_csr_transpose), and A A on config 3's row-length law at 65 536 rows with uniform columns.  One JSON line per workload:

  call_ms          the whole call: allocation, launches, the read-back of the bounds and the waits included (a host clock
                   around the synchronous call)
  call_destroy_ms  the call and spmv_csr_destroy of its result (the torch route frees into torch's caching allocator)
  values_ms        spmv_csr_spgemm_values on a kept plan: the numeric pass alone, between two device synchronisations
  products, nnz_c, compression = products / nnz_c; longest_row_products: the most terms of one row of A
  floor_ms         the traffic floor at 8 TB/s: both operands' col_idx and vals once per term of the product they take part in
                   (8 bytes of b per term; 8 bytes of a per entry of a, read once per term's row walk: 8 nnz(a)), row_ptr of a
                   and the referenced row bounds of b (8 bytes per entry of a), and the result written once (8 nnz_c + 4 rows)
  torch_ms         torch.sparse.mm on sparse_csr tensors of the same arrays on the device, where this torch build offers it;
                   otherwise "torch" holds what it refused with and no ratio is given
  same_pattern, values_close   torch's result against ours, once per line: crow and col indices equal, values within
                   1e-5 * (|a| |b|) entrywise
  *_spread         (max - min) / median over the windows

Both sides run in one process in alternating windows of at least --window-ms (at least two calls); a window's figure is its mean
call; the medians of --windows windows are reported.  Needs a device."""
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
C3_ROWS = 65536      # config 3's law at this size: see DESIGN.md section 26 for the reason


def window(fn, min_s, after=None):
    """Mean seconds per call over a window of at least min_s (at least two calls); after(result) follows a call outside the
    first figure.  Returns (mean of fn alone, mean of fn and after)."""
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


def spread(v):
    return round((max(v) - min(v)) / statistics.median(v), 4)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spgemm.jsonl"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    if capi.device_count() < 1:
        print("spgemm_time needs a HIP device", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    c3 = W.config("c3", band=0, scale=C3_ROWS / W.CONFIGS["c3"].rows)
    jobs = [("c2 band 8192: A A", W.config("c2", band=8192), False), ("c2 uniform: A A", W.config("c2", band=0), False),
            ("c2 band 8192: A A^T", W.config("c2", band=8192), True), (f"c3 law at {C3_ROWS} rows, uniform: A A", c3, False)]
    only = [s for s in args.only.split(",") if s]
    lines = []
    med = statistics.median
    for name, w, with_transpose in jobs:
        if only and not any(o in name for o in only):
            continue
        rp = W.row_ptr(w)
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        A = capi.CsrMatrix.from_device(w.rows, w.cols, d_rp, d_ci, d_va)
        B = A.transpose() if with_transpose else A
        b_rp = torch.empty(B.rows + 1, dtype=torch.int32, device=dev)
        b_ci = torch.empty(B.nnz, dtype=torch.int32, device=dev)
        b_va = torch.empty(B.nnz, dtype=torch.float32, device=dev)
        B.copy_arrays(b_rp, b_ci, b_va)
        torch.cuda.synchronize()
        blen = (b_rp[1:] - b_rp[:-1]).long()
        per_entry = blen[d_ci.long()]
        row_of = torch.repeat_interleave(torch.arange(w.rows, device=dev), (d_rp[1:] - d_rp[:-1]).long())
        longest = int(torch.zeros(w.rows, dtype=torch.long, device=dev).index_add_(0, row_of, per_entry).max())
        del blen, per_entry, row_of

        c = A.spgemm(B, keep_plan=True)                      # warm, and the result the torch side is compared with
        products, nnz_c = c.spgemm_products, c.nnz
        line = {"workload": name, "rows": w.rows, "nnz_a": nnz, "nnz_b": B.nnz, "products": products, "nnz_c": nnz_c,
                "compression": round(products / max(nnz_c, 1), 3), "longest_row_products": longest,
                "plan_bytes": c.spgemm_plan_bytes()}
        theirs = None
        try:
            ta = torch.sparse_csr_tensor(d_rp, d_ci, d_va, size=(w.rows, w.cols))
            tb = torch.sparse_csr_tensor(b_rp, b_ci, b_va, size=(B.rows, B.cols))
            tc = torch.sparse.mm(ta, tb)
            torch.cuda.synchronize()
            g_rp = torch.empty(c.rows + 1, dtype=torch.int32, device=dev)
            g_ci = torch.empty(nnz_c, dtype=torch.int32, device=dev)
            g_va = torch.empty(nnz_c, dtype=torch.float32, device=dev)
            c.copy_arrays(g_rp, g_ci, g_va)
            torch.cuda.synchronize()
            same = tc.crow_indices().numel() == g_rp.numel() and tc.col_indices().numel() == nnz_c \
                and bool(torch.equal(tc.crow_indices().int(), g_rp) and torch.equal(tc.col_indices().int(), g_ci))
            line["same_pattern"] = bool(same)
            if same:
                mag = torch.sparse.mm(torch.sparse_csr_tensor(d_rp, d_ci, d_va.abs(), size=(w.rows, w.cols)),
                                      torch.sparse_csr_tensor(b_rp, b_ci, b_va.abs(), size=(B.rows, B.cols))).values()
                line["values_close"] = bool(((tc.values() - g_va).abs() <= 1e-5 * mag).all())
                del mag
            del tc, g_rp, g_ci, g_va
            theirs = lambda: torch.sparse.mm(ta, tb)         # noqa: E731
        except (RuntimeError, NotImplementedError) as e:
            line["torch"] = f"refused: {str(e).splitlines()[0][:200]}"
            torch.cuda.synchronize()
        a, a_close, v, t = [], [], [], []
        for _ in range(args.windows):
            alone, both = window(lambda: A.spgemm(B), args.window_ms / 1e3, after=lambda r: r.close())
            a.append(alone * 1e3)
            a_close.append(both * 1e3)
            v.append(window(lambda: c.spgemm_values(A, B), args.window_ms / 1e3)[0] * 1e3)
            if theirs is not None:
                t.append(window(theirs, args.window_ms / 1e3)[1] * 1e3)
        floor = (8 * products + 8 * nnz + 8 * nnz + 4 * w.rows + 8 * nnz_c + 4 * w.rows) / HBM_BYTES_PER_S * 1e3
        line.update({"call_ms": round(med(a), 4), "call_spread": spread(a), "call_destroy_ms": round(med(a_close), 4),
                     "call_destroy_spread": spread(a_close), "values_ms": round(med(v), 4), "values_spread": spread(v),
                     "floor_ms": round(floor, 4), "window_ms": args.window_ms, "windows": args.windows})
        if t:
            line.update({"torch_ms": round(med(t), 4), "torch_spread": spread(t), "speedup": round(med(t) / med(a), 3),
                         "speedup_with_destroy": round(med(t) / med(a_close), 3)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        c.close()
        if with_transpose:
            B.close()
        A.close()
        del d_rp, d_ci, d_va, b_rp, b_ci, b_va
        theirs = None
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))
    return 0 if all(l.get("same_pattern", True) and l.get("values_close", True) for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
