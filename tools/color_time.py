#!/usr/bin/env python3
"""tools/color_time.py [--out FILE] [--window-ms 100] [--windows 5] [--only NAME,...] [--no-krylov] -- the multicolour ordering on
the workloads of tools/trsv_time.py: stencil7(200) with the symmetric 6 / -1 values, and config 2 + 64 I with band 8192 and with
uniform columns.  One JSON line per workload:

  colors, rounds, launches, largest, smallest, sweep_entries, peak_bytes   spmv_csr_color's report
  color_ms         spmv_csr_color as a whole call (a host clock around the synchronous call)
  stream_gbs       the measured rate of a device copy of 1 GiB (bytes read + bytes written per second)
  color_floor_ms   rounds full sweeps of sweep_entries * 4 bytes at that rate; color_over_floor = color_ms / color_floor_ms
  direct_ms, transpose_ms   spmv_csr_permute(perm, perm) by the direct route and with SPMV_PERMUTE_VIA_TRANSPOSE forced, whole
                   calls (the result destroyed again) in alternating windows, every window listed; direct_wins: direct_ms is below
                   transpose_ms by more than twice the larger (max - min) of the two
  natural / multicolor     for A and for P A P^T: the levels of both triangles, the launches of one ilu0_values and of one
                   ilu0_solve, and each of the two as a replayed graph (values_graph_ms, solve_graph_ms)
  krylov           solver, iterations, converged and wall time to ||r|| <= 1e-5 ||b|| (b standard normal, x = 0; the second of two
                   solves): plain, with the natural ILU(0), and through solvers.multicolor with P A P^T's
  *_spread         (max - min) / median over the windows

Every timed result is checked first, on the device: the colouring is the contract's (every row's colour is the smallest one that no
neighbour of a higher key has), perm sorts the rows by (colour, row), both routes of the permutation give the same bytes, and those
are P A P^T (sorted rows, B's entry i is A's entry map[i] relabelled).  All sides run in one process in alternating windows of at
least --window-ms (at least two calls); the medians of --windows windows are reported.  Needs a device."""
import argparse
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
from ilu0_time import solve_time  # noqa: E402
from trsv_time import row_index, spread, window, workloads  # noqa: E402


def fmix32(h):
    m = 0xFFFFFFFF
    h = h & m
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & m
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def coloring_is_the_contract(rp, ci, color, perm, seed):
    """color[i] = the smallest colour that no neighbour of a higher key has, and perm = the rows by (colour, row)."""
    n = rp.numel() - 1
    row, col = row_index(rp), ci.long()
    a, b = torch.cat([row, col]), torch.cat([col, row])
    key = fmix32(torch.arange(n, device=rp.device) ^ seed)
    keep = key[b] > key[a]                                       # (keys never tie: the row itself drops out)
    a, b = a[keep], b[keep]
    del row, col, keep
    ca, cb = color.long()[a], color.long()[b]
    if bool((ca == cb).any()):
        return False
    below = cb < ca
    width = int(color.max()) + 1
    pairs = torch.unique(a[below] * width + cb[below])             # the distinct (row, smaller colour a higher neighbour has)
    have = torch.bincount(pairs // width, minlength=n)
    if not bool((have == color.long()).all()):
        return False
    want = torch.argsort(color.long() * n + torch.arange(n, device=rp.device))
    return bool((want == perm.long()).all())


def is_papt(A_arrays, B_arrays, bmap, perm):
    rp, ci, va = A_arrays
    brp, bci, bva = B_arrays
    n = rp.numel() - 1
    inv = torch.empty(n, dtype=torch.long, device=rp.device)
    inv[perm.long()] = torch.arange(n, device=rp.device)
    m = bmap.long()
    brow = row_index(brp)
    ok = bool((inv[row_index(rp)[m]] == brow).all()) and bool((inv[ci.long()[m]] == bci.long()).all())
    ok = ok and bool((va.view(torch.int32)[m] == bva.view(torch.int32)).all())
    same = brow[1:] == brow[:-1]
    step = (bci.long()[1:] - bci.long()[:-1])[same]
    tie = (m[1:] - m[:-1])[same]
    return ok and bool(((step > 0) | ((step == 0) & (tie > 0))).all())


def arrays(h, dev):
    rp = torch.empty(h.rows + 1, dtype=torch.int32, device=dev)
    ci = torch.empty(h.nnz, dtype=torch.int32, device=dev)
    va = torch.empty(h.nnz, dtype=torch.float32, device=dev)
    h.copy_arrays(rp, ci, va)
    torch.cuda.synchronize()
    return rp, ci, va


def factor_report(H, r, min_s, windows):
    """Levels, launches and the replayed graphs of ilu0_values and ilu0_solve of H's factor."""
    med = statistics.median
    t0 = time.perf_counter()
    M = H.ilu0()
    first_ms = (time.perf_counter() - t0) * 1e3
    lo, up = M.trsv_plan_info("lower"), M.trsv_plan_info("upper")
    z = torch.empty_like(r)
    gv, gs = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gv):
        M.ilu0_values(H)
    with torch.cuda.graph(gs):
        M.ilu0_solve(r, z)
    tv, ts = [], []
    for _ in range(windows):
        tv.append(window(gv.replay, min_s) * 1e3)
        ts.append(window(gs.replay, min_s) * 1e3)
    rep = {"levels_lower": lo["levels"], "levels_upper": up["levels"], "values_launches": lo["launches"] + 1,
           "solve_launches": lo["launches"] + up["launches"], "ilu0_first_ms": round(first_ms, 3), "values_graph_ms": round(med(tv), 4),
           "values_spread": spread(tv), "solve_graph_ms": round(med(ts), 4), "solve_spread": spread(ts), "pivot": M.ilu0_pivot()}
    del gv, gs
    return M, rep


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "color.jsonl"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-krylov", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, W, solvers = pkg.capi, pkg.workloads, pkg.solvers
    if capi.device_count() < 1:
        print("color_time needs a HIP device", file=sys.stderr)
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
        if name.startswith("stencil7"):                        # the symmetric stencil: 6 on the diagonal, -1 off it
            va.copy_(torch.where(ci.long() == row_index(rp), 6.0, -1.0))
        A = capi.CsrMatrix.from_device(rows, rows, rp, ci, va)
        A.color(args.seed)                                     # (warms the kernels up)
        t_color = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            color, perm, color_ptr, info = A.color(args.seed)
            t_color.append((time.perf_counter() - t0) * 1e3)
        good = coloring_is_the_contract(rp, ci, color, perm, args.seed)
        floor = info["rounds"] * info["sweep_entries"] * 4 / stream_rate * 1e3
        line = {"workload": name, "rows": rows, "nnz": A.nnz, "seed": args.seed, **info, "color_ms": round(med(t_color), 3),
                "color_spread": spread(t_color), "stream_gbs": round(stream_rate / 1e9, 1), "color_floor_ms": round(floor, 4),
                "color_over_floor": round(med(t_color) / floor, 1), "color_is_contract": good}
        torch.cuda.empty_cache()
        # the two routes of the permutation: the same bytes, and those are P A P^T
        Bd, Bt = A.permute(perm, perm, keep_map=True), A.permute(perm, perm, keep_map=True, via_transpose=True)
        ad, at = arrays(Bd, dev), arrays(Bt, dev)
        pos = torch.arange(A.nnz, dtype=torch.int32, device=dev)
        md, mt = Bd.permute_gather(pos), Bt.permute_gather(pos)
        same = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(ad + (md,), at + (mt,)))
        papt = is_papt((rp, ci, va), ad, md, perm)
        line.update({"routes_agree": same, "is_papt": papt})
        good = good and same and papt
        Bd.close()
        Bt.close()
        del ad, at, md, mt, pos
        torch.cuda.empty_cache()
        t_direct, t_transpose = [], []
        for via in (False, True):                              # (one untimed call each: the first large allocations of a route)
            A.permute(perm, perm, via_transpose=via).close()
        for _ in range(args.windows):
            t_direct.append(window(lambda: A.permute(perm, perm).close(), min_s) * 1e3)
            t_transpose.append(window(lambda: A.permute(perm, perm, via_transpose=True).close(), min_s) * 1e3)
        wins = med(t_direct) < med(t_transpose) - 2 * max(max(t_direct) - min(t_direct), max(t_transpose) - min(t_transpose))
        line.update({"direct_ms": round(med(t_direct), 3), "direct_spread": spread(t_direct), "direct_windows": [round(t, 3) for t in t_direct],
                     "transpose_ms": round(med(t_transpose), 3), "transpose_spread": spread(t_transpose),
                     "transpose_windows": [round(t, 3) for t in t_transpose], "direct_wins": bool(wins)})
        # factor and solve, natural and multicolour
        r = torch.from_numpy(np.random.default_rng(2026).standard_normal(rows).astype(np.float32)).to(dev)
        R = solvers.multicolor(A, args.seed)
        Mn, line["natural"] = factor_report(A, r, min_s, args.windows)
        Mc, line["multicolor"] = factor_report(R.matrix, r, min_s, args.windows)
        good = good and line["multicolor"]["levels_lower"] <= info["colors"] and line["multicolor"]["levels_upper"] <= info["colors"]
        if not args.no_krylov and name.startswith(("stencil7", "c2 uniform")):
            solver, label = (solvers.pcg, "pcg") if name.startswith("stencil7") else (solvers.bicgstab, "bicgstab")
            kry = {"solver": label, "plain": solve_time(solver, A, r, None, 5000), "ilu0": solve_time(solver, A, r, Mn, 5000)}
            for _ in range(2):                                 # (the second of two solves, as solve_time)
                x = torch.zeros_like(r)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = R.solve(solver, r, x, M=Mc, tol=1e-5, maxiter=5000)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            kry["multicolor_ilu0"] = {"iterations": res.iterations, "converged": res.converged, "ms": round(ms, 2)}
            line["krylov"] = kry
        line.update({"window_ms": args.window_ms, "windows": args.windows})
        ok = ok and good
        for h in (Mn, Mc):
            h.close()
        R.close()
        A.close()
        print(json.dumps(line), flush=True)
        lines.append(line)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(l) + "\n" for l in lines))
        del rp, ci, va, r, color, perm
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
