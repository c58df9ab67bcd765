#!/usr/bin/env python3
"""tools/add_time.py [--out FILE] [--window-ms 100] [--windows 5] [--only NAME,...] -- spmv_csr_add against torch's own route.

Workloads: A + B (B: the same configuration from another seed) on config 2 and config 3 with band 8192 and with uniform
columns; on config 2 with band 8192 also A + A^T (A^T from spmv_csr_transpose), A UNION the per-row top-8 of A
(spmv_csr_select_topk), A INTERSECT a band mask (64 columns per row inside band 8192, coefficients 1 and 0) and A + B with
B's rows stored in descending column order (the route through the row-sorted view).  One JSON line per workload:

  call_ms          the whole call: the sortedness pass, allocation, launches, the read-backs and the waits included (a host clock
                   around the synchronous call)
  call_destroy_ms  the call and spmv_csr_destroy of its result (the torch route frees into torch's caching allocator)
  values_ms        spmv_csr_add_values on a kept plan: one launch, between two device synchronisations
  nnz_a, nnz_b, nnz_c, terms, plan_bytes
  floor_ms         the traffic floor at 8 TB/s: both operands' row_ptr, col_idx and vals read once and the result written once
                   (8 (nnz_a + nnz_b + nnz_c) + 12 (rows + 1) bytes); over_floor = call_ms / floor_ms
  values_floor_ms  the same for the value pass: the plan and both vals read once, vals written once
                   (4 terms + 4 (nnz_c + 1) + 4 (nnz_a + nnz_b) + 4 nnz_c bytes)
  torch_route      "sparse_csr add" (the sum of two sparse_csr tensors) where this torch build offers it, otherwise "coo cat +
                   coalesce"; the intersection: "isin of 64-bit keys + masked select"; or what torch refused with
  torch_ms         that route on the same arrays on the device
  same_pattern, values_close   torch's result against ours, once per line: row and column indices equal, values within
                   1e-5 * (|alpha a| + |beta b|) entrywise
  *_spread         (max - min) / median over the windows

Both sides run in one process in alternating windows of at least --window-ms (at least two calls); a window's figure is its mean
call; the medians of --windows windows are reported.  Needs a device."""
import argparse
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

HBM_BYTES_PER_S = 8e12


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


def arrays_of(capi, W, w, dev):
    rp = W.row_ptr(w)
    nnz = int(rp[-1])
    d_rp = torch.from_numpy(rp).to(dev)
    d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
    capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
    return d_rp, d_ci, d_va


def copied(h, dev):
    rp = torch.empty(h.rows + 1, dtype=torch.int32, device=dev)
    ci = torch.empty(h.nnz, dtype=torch.int32, device=dev)
    va = torch.empty(h.nnz, dtype=torch.float32, device=dev)
    h.copy_arrays(rp, ci, va)
    torch.cuda.synchronize()
    return rp, ci, va


def row_index(rp):
    return torch.repeat_interleave(torch.arange(rp.numel() - 1, device=rp.device), (rp[1:] - rp[:-1]).long())


def torch_routes(a, b, shape, intersect):
    """[(name, callable -> (row indices or crow, col indices, values, is_csr))] in the order they are tried.  The
    intersection is a membership test of 64-bit keys (torch.isin, which sorts) and a masked select: the product of two sparse
    tensors by a mask of ones would be torch's other route, but on the build this was written against it ended the process
    with SIGFPE at config 2's size, so it is not called here."""
    (a_rp, a_ci, a_va), (b_rp, b_ci, b_va) = a, b
    ia = torch.stack([row_index(a_rp), a_ci.long()])
    ib = torch.stack([row_index(b_rp), b_ci.long()])
    if intersect:
        ka, kb = ia[0] * shape[1] + ia[1], ib[0] * shape[1] + ib[1]

        def isin():
            keep = torch.isin(ka, kb)
            return ia[0][keep], ia[1][keep], a_va[keep], False
        return [("isin of 64-bit keys + masked select", isin)]
    ta = torch.sparse_csr_tensor(a_rp, a_ci, a_va, size=shape)
    tb = torch.sparse_csr_tensor(b_rp, b_ci, b_va, size=shape)

    def csr():
        c = ta + tb
        return c.crow_indices(), c.col_indices(), c.values(), True

    def coo():
        c = torch.sparse_coo_tensor(torch.cat([ia, ib], 1), torch.cat([a_va, b_va]), size=shape).coalesce()
        return c.indices()[0], c.indices()[1], c.values(), False
    return [("sparse_csr add", csr), ("coo cat + coalesce", coo)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "add.jsonl"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    if capi.device_count() < 1:
        print("add_time needs a HIP device", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    jobs = [(f"{cfg} {'band 8192' if band else 'uniform'}: A + B", cfg, band, "other seed") for cfg in ("c2", "c3") for band in (8192, 0)]
    jobs += [("c2 band 8192: A + A^T", "c2", 8192, "transpose"), ("c2 band 8192: A union top-8(A)", "c2", 8192, "top8"),
             ("c2 band 8192: A intersect band mask", "c2", 8192, "mask"), ("c2 band 8192: A + B, B's rows descending", "c2", 8192, "unsorted")]
    only = [s for s in args.only.split(",") if s]
    lines = []
    med = statistics.median
    for name, cfg, band, kind in jobs:
        if only and not any(o in name for o in only):
            continue
        w = W.config(cfg, band=band)
        a = arrays_of(capi, W, w, dev)
        A = capi.CsrMatrix.from_device(w.rows, w.cols, *a)
        alpha, beta, op = 1.0, 1.0, "union"
        made = None
        if kind in ("other seed", "unsorted"):
            b = arrays_of(capi, W, dataclasses.replace(w, seed=w.seed + 1), dev)
            if kind == "unsorted":                        # every row stored back to front
                rp = b[0].long()
                row = row_index(b[0])
                flip = rp[row] + rp[row + 1] - 1 - torch.arange(b[1].numel(), device=dev)
                b = (b[0], b[1][flip].contiguous(), b[2][flip].contiguous())
                del rp, row, flip
        elif kind == "transpose":
            made = A.transpose()
            b = copied(made, dev)
        elif kind == "top8":
            made = A.select_topk(8)
            b = copied(made, dev)
        else:
            b = arrays_of(capi, W, dataclasses.replace(w, seed=w.seed + 2, mean=64), dev)
            beta, op = 0.0, "intersect"
        if made is not None:
            made.close()
        B = capi.CsrMatrix.from_device(w.rows, w.cols, *b)

        c = A.add(B, alpha, beta, op, keep_plan=True)      # warm, and the result the torch side is compared with
        nnz_c, plan_bytes = c.nnz, c.add_plan_bytes()
        terms = (plan_bytes - 4 * (nnz_c + 1)) // 4
        line = {"workload": name, "rows": w.rows, "op": op, "alpha": alpha, "beta": beta, "nnz_a": A.nnz, "nnz_b": B.nnz, "nnz_c": nnz_c,
                "terms": terms, "plan_bytes": plan_bytes}
        theirs = None
        g_rp, g_ci, g_va = copied(c, dev)
        # for the comparison the unsorted operand goes to torch sorted (torch's sparse_csr kernels expect sorted rows)
        tb = b
        if kind == "unsorted":
            sb = B.add(B, 1.0, 0.0, "intersect")           # B with sorted rows
            tb = copied(sb, dev)
            sb.close()
        refused = []
        for route, fn in torch_routes(a, tb, (w.rows, w.cols), op == "intersect"):
            try:
                t_r, t_c, t_v, is_csr = fn()
                torch.cuda.synchronize()
                t_rp = t_r.int() if is_csr else torch.cat([torch.zeros(1, dtype=torch.long, device=dev),
                                                           torch.cumsum(torch.bincount(t_r, minlength=w.rows), 0)]).int()
                same = t_rp.numel() == g_rp.numel() and t_c.numel() == nnz_c and bool(torch.equal(t_rp, g_rp) and torch.equal(t_c.int(), g_ci))
                line["torch_route"] = route
                line["same_pattern"] = bool(same)
                if same:
                    ma = capi.CsrMatrix.from_device(w.rows, w.cols, a[0], a[1], a[2].abs())
                    mb = capi.CsrMatrix.from_device(w.rows, w.cols, b[0], b[1], b[2].abs())
                    mc = ma.add(mb, abs(alpha), abs(beta), op)
                    mag = copied(mc, dev)[2]
                    for h in (mc, ma, mb):
                        h.close()
                    line["values_close"] = bool(((t_v - g_va).abs() <= 1e-5 * mag).all())
                    del mag
                del t_r, t_c, t_v, t_rp
                theirs = fn
                break
            except (RuntimeError, NotImplementedError) as e:
                refused.append(f"{route}: {str(e).splitlines()[0][:160]}")
                torch.cuda.synchronize()
        if refused:
            line["torch_refused"] = refused
        del g_rp, g_ci, g_va
        t_call, t_close, t_vals, t_torch = [], [], [], []
        for _ in range(args.windows):
            alone, both = window(lambda: A.add(B, alpha, beta, op), args.window_ms / 1e3, after=lambda r: r.close())
            t_call.append(alone * 1e3)
            t_close.append(both * 1e3)
            t_vals.append(window(lambda: c.add_values(A, B, alpha, beta), args.window_ms / 1e3)[0] * 1e3)
            if theirs is not None:
                t_torch.append(window(theirs, args.window_ms / 1e3)[1] * 1e3)
        floor = (8 * (A.nnz + B.nnz + nnz_c) + 12 * (w.rows + 1)) / HBM_BYTES_PER_S * 1e3
        vfloor = (4 * terms + 4 * (nnz_c + 1) + 4 * (A.nnz + B.nnz) + 4 * nnz_c) / HBM_BYTES_PER_S * 1e3
        line.update({"call_ms": round(med(t_call), 4), "call_spread": spread(t_call), "call_destroy_ms": round(med(t_close), 4),
                     "call_destroy_spread": spread(t_close), "values_ms": round(med(t_vals), 4), "values_spread": spread(t_vals),
                     "floor_ms": round(floor, 4), "over_floor": round(med(t_call) / floor, 2), "values_floor_ms": round(vfloor, 4),
                     "values_over_floor": round(med(t_vals) / vfloor, 2), "window_ms": args.window_ms, "windows": args.windows})
        if t_torch:
            line.update({"torch_ms": round(med(t_torch), 4), "torch_spread": spread(t_torch), "speedup": round(med(t_torch) / med(t_call), 3),
                         "speedup_with_destroy": round(med(t_torch) / med(t_close), 3)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        for h in (c, B, A):
            h.close()
        del a, b, tb
        theirs = None
        torch.cuda.empty_cache()
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))
    return 0 if all(l.get("same_pattern", True) and l.get("values_close", True) for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
