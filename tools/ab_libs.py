#!/usr/bin/env python3
"""tools/ab_libs.py CONFIG.json OUT.jsonl -- development aid: several builds of libspmv_hip.so (tools/build_variant.sh, or the
library of another commit copied beside them) and knob settings side by side in ONE process on one device.  Every side is a
library loaded on its own with a handle of its own on the same device arrays; the sides are timed in alternating windows of
>= 100 ms (spmv_csr_time), `rounds` windows per side, forwards and backwards in turn.  One JSON line per workload and side:
median, min, max and spread (max - min) of the window means, whether y equals the first side's as int32, the plan line.
CONFIG = {"rounds": R, "sides": [{"name", "lib", "env": {knob: value}}], "workloads": [{"kind": "c2"|"c3"|"c4"|"c5shard",
"band": n} | {"kind": "stencil7", "n": n}]}; knobs are read when a side's plan is made.  (tools/exp/tiled_chain_ab.json)"""
import ctypes as C
import json
import math
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

KNOBS = ("SPMV_TILED_ORDER", "SPMV_TILED_BLOCK", "SPMV_SORTED_FROM", "SPMV_COL16", "SPMV_BLOCKS")


class Lib:
    def __init__(self, path):
        L = C.CDLL(os.fspath(ROOT / path))
        vp, i64 = C.c_void_p, C.c_int64
        L.spmv_csr_create_device.restype = C.c_int
        L.spmv_csr_create_device.argtypes = [i64, i64, i64, vp, vp, vp, C.POINTER(vp)]
        L.spmv_csr_destroy.argtypes = [vp]
        L.spmv_csr_plan.argtypes = [vp, C.c_int, vp]
        L.spmv_csr_run.argtypes = [vp, C.c_int, vp, vp, vp]
        L.spmv_csr_time.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.POINTER(C.c_float)]
        L.spmv_csr_plan_describe.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        L.spmv_csr_plan_bytes.restype = i64
        L.spmv_csr_plan_bytes.argtypes = [vp, C.c_int]
        L.spmv_last_error.restype = C.c_char_p
        self.order = getattr(L, "spmv_csr_plan_chunk_order", None)
        if self.order is not None:
            self.order.argtypes = [vp, C.c_int]
        self.L = L

    def ck(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}: {self.L.spmv_last_error().decode()}")


def main():
    import torch
    cfg = json.loads(Path(sys.argv[1]).read_text())
    out = open(sys.argv[2], "a")
    pkg = ge.load_package()
    capi, W = pkg.capi, pkg.workloads
    dev = torch.device("cuda:0")
    libs = {}
    for s in cfg["sides"]:
        if s["lib"] not in libs:
            libs[s["lib"]] = Lib(s["lib"])
    rounds = cfg.get("rounds", 9)
    for wl in cfg["workloads"]:
        torch.cuda.empty_cache()
        if wl["kind"] == "stencil7":
            N, rp, ci, va = W.stencil7(wl["n"])
            rows = cols = N
            d_rp, d_ci, d_va = (torch.from_numpy(a).to(dev) for a in (rp, ci, va))
            d_x = torch.rand(N, dtype=torch.float32, device=dev)
            nnz = int(rp[-1])
        else:
            shard = wl["kind"] == "c5shard"
            w = W.c5(8, band=wl["band"]) if shard else W.config(wl["kind"], band=wl["band"])
            n_loc = 16 * W.Mi if shard else w.rows
            rp = W.row_ptr(w, 0, n_loc)
            nnz = int(rp[-1])
            rows, cols = n_loc, w.cols
            d_rp = torch.from_numpy(rp).to(dev)
            d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
            d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
            d_x = torch.empty(cols, dtype=torch.float32, device=dev)
            capi.synth_fill(w.seed, 0, n_loc, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
            capi.synth_x(w.seed, 0, w.cols, d_x)
        d_y = torch.empty(rows, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        v = capi.VARIANTS[wl.get("variant", "auto")]
        sides = []
        y0 = None
        for s in cfg["sides"]:
            lib = libs[s["lib"]]
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(s.get("env", {}))
            h = C.c_void_p()
            lib.ck(lib.L.spmv_csr_create_device(rows, cols, nnz, d_rp.data_ptr(), d_ci.data_ptr(), d_va.data_ptr(), C.byref(h)), "create")
            lib.ck(lib.L.spmv_csr_plan(h, v, None), "plan")
            buf = C.create_string_buffer(512)
            lib.L.spmv_csr_plan_describe(h, v, buf, 512)
            d_y.fill_(float("nan"))
            lib.ck(lib.L.spmv_csr_run(h, v, d_x.data_ptr(), d_y.data_ptr(), None), "run")
            torch.cuda.synchronize()
            y = d_y.view(torch.int32).clone()
            if y0 is None:
                y0 = y
            same = bool(torch.equal(y, y0))
            ms = C.c_float()
            lib.ck(lib.L.spmv_csr_time(h, v, d_x.data_ptr(), d_y.data_ptr(), 5, None, C.byref(ms)), "time")
            iters = max(5, int(math.ceil(120.0 / max(ms.value, 1e-3))))
            sides.append(dict(s=s, lib=lib, h=h, plan=buf.value.decode(), same=same, iters=iters, t=[],
                              order=None if lib.order is None else int(lib.order(h, v)),
                              plan_bytes=int(lib.L.spmv_csr_plan_bytes(h, v))))
        for k in KNOBS:
            os.environ.pop(k, None)
        for r in range(rounds):
            for sd in (sides if r % 2 == 0 else sides[::-1]):
                ms = C.c_float()
                sd["lib"].ck(sd["lib"].L.spmv_csr_time(sd["h"], v, d_x.data_ptr(), d_y.data_ptr(), sd["iters"], None, C.byref(ms)), "time")
                sd["t"].append(ms.value)
        for sd in sides:
            t = np.sort(np.array(sd["t"]))
            rec = dict(workload=wl, side=sd["s"]["name"], lib=sd["s"]["lib"], env=sd["s"].get("env", {}), nnz=nnz,
                       median_ms=round(float(np.median(t)), 5), min_ms=round(float(t[0]), 5), max_ms=round(float(t[-1]), 5),
                       spread_ms=round(float(t[-1] - t[0]), 5), windows=len(t), iters_per_window=sd["iters"],
                       y_equals_first_side=sd["same"], chunk_order=sd["order"], plan_bytes=sd["plan_bytes"], plan=sd["plan"])
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            sd["lib"].L.spmv_csr_destroy(sd["h"])
        del d_rp, d_ci, d_va, d_x, d_y, y0


if __name__ == "__main__":
    main()
