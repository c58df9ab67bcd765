"""GPU (-m gpu): spmv_csr_transpose at the 32-bit edges one handle admits (rows, cols, nnz < 2^31).

The matrices are formula cases of tests/_limits.py, built on the device by _limits.build; a child process per case, the
pattern and the rules of tests/test_gpu_limits.py (run this module as a step of its own, with -x):

    G   3000 x (2^30 + 7)            T has 2^30 + 7 rows: t.row_ptr passes 4 GiB, exclusive_scan_i32 over 2^30 + 8 entries
    F   (2^30 + 2^20 + 5) x 2^18     row numbers >= 2^30 in t.col_idx, ~3 600 nonzeros per row of T
    A   36 864 x 32 768, nearly full two digit passes over 1.18e9 positions, every column ~36 100 times
    D   2^27 x 2^24, hashed columns  three digit passes over 1.17e9 positions
    E   band, nnz = 2^31 - 5         every unsigned 32-bit position

Per case: T = A.transpose(keep_map=True); then, all on the device with torch in slabs of at most 2^26 and int64:
  * structure: T's arrays reach torch one at a time through spmv_csr_download and back to the device slab by slab;
    the differences of t.row_ptr equal bincount(col_idx); inside every row of T t.col_idx is non-decreasing (neighbours
    compared, the positions t.row_ptr names masked); spmv_csr_validate(T); spmv_csr_column_range(T) is (first, last
    non-empty row of A);
  * exact product: u(r) = Case.x(r) and u2(r) = Case.x(3 r + 1) (NaN at A's empty rows), the expectation index_add_ of
    val(k) u(row(k)) in int64; SPMV_TILED and SPMV_SCALAR on T return it bit for bit on all rows (two runs, into NaN and
    into a sentinel; y one float past a 16-byte boundary between guard bands).  Exact because 16 x (longest row of T) <
    2^24, asserted from the device bincount before anything is compared;
  * the map (it has no download call): A's vals rewritten in place to Case.val(k + 12 345), spmv_csr_transpose_values,
    and the product of THOSE values, exactly -- a map entry that points at the wrong nonzero shows;
  * free device memory returns to within 2 MiB.
A child that ends by a signal, an abort or its time limit fails its case; every later case then reports "not run" without
touching the GPU.  Nothing is run twice to see whether a failure repeats."""
import gc
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import _limits as L
from test_gpu_limits import GIB, MIB, SENTINEL, Guarded, Report, _diff, _free, _summary

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TI, S = 5, 0
ORDER = ("G", "F", "A", "D", "E")                     # smallest first
SHIFT = 12_345
# seconds a child may take: max(120, 5 x measured).  Measured on one MI355X (child wall time in s, the warm-up at 1/64 and
# the start of Python included; peak GiB of device memory in the child): G 9 / 33.0, F 5 / 51.4, A 4 / 32.6, D 4 / 33.4,
# E 5 / 67.7 (spmv_csr_transpose itself, map kept: G 0.01 s, F 0.12, A 0.05, D 0.12, E 0.20)
LIMIT = {"G": 120, "F": 120, "A": 120, "D": 120, "E": 120}


def bytes_needed(c):
    """Device bytes a child needs, from the sizes: A (8 nnz + 4 rows), T with its map (12 nnz + 4 cols), the transpose's
    temporaries as include/spmv_hip.h states them (16 nnz + nnz / 4), the plans of T (SPMV_TILED with its 16-bit columns and
    lists, SPMV_SCALAR: 8 nnz at most), _limits.build's x, expectation and mask (5 cols + 4 rows), this module's copies of
    T's arrays and the masks (5 nnz + 8 cols), u and u2 (8 rows), two int64 sums, two expectations and y (28 cols), and the
    slab temporaries (16 int64 arrays of 2^26)."""
    return 50 * c.nnz + 16 * c.rows + 45 * c.cols + 16 * 8 * min(max(c.nnz, c.cols, c.rows), L.SLAB) + (64 << 20)


# ---- the child -------------------------------------------------------------------------------------------------------------
def _to_device(torch, dev, host, dtype):
    out = torch.empty(len(host), dtype=dtype, device=dev)
    for s0 in range(0, len(host), L.SLAB):
        out[s0:s0 + L.SLAB] = torch.from_numpy(host[s0:s0 + L.SLAB]).to(dev)
    return out


def _download(torch, dev, capi, T, which):
    """One array of T through spmv_csr_download: to the host, then back to the device slab by slab."""
    n = T.rows + 1 if which == 0 else T.nnz
    host = np.empty(n, np.int32)
    ptrs = [0, 0, 0]
    ptrs[which] = host.ctypes.data
    capi.check(capi.lib().spmv_csr_download(T._h, *ptrs))
    return _to_device(torch, dev, host, torch.int32)


def _vector(c, torch, dev, mul, add):
    """u(r) = Case.x(mul r + add) as float32 (NaN at the empty rows of the case) and as int64."""
    uf = torch.empty(c.rows, dtype=torch.float32, device=dev)
    ui = torch.empty(c.rows, dtype=torch.int64, device=dev)
    for r0 in range(0, c.rows, L.SLAB):
        r = torch.arange(r0, min(c.rows, r0 + L.SLAB), dtype=torch.int64, device=dev)
        v = c.x(mul * r + add)
        ui[r0:r0 + r.numel()] = v
        f = v.to(torch.float32)
        f[c.length(r) == 0] = float("nan")
        uf[r0:r0 + r.numel()] = f
    return uf, ui


def _expected(c, b, torch, dev, us, shift):
    """z[j] = sum over the nonzeros k of column j of val(k + shift) u(row(k)), int64 over slabs, for every u of us."""
    zs = [torch.zeros(c.cols, dtype=torch.int64, device=dev) for _ in us]
    for k0, k1, lo, hi, ends in L._slabs(b, torch, L.SLAB):
        k = torch.arange(k0, k1, dtype=torch.int64, device=dev)
        r_first, r_end = lo - 1, L._at(b.rp, torch, k1 - 1)
        r = torch.searchsorted(b.rp[r_first:r_end + 1].to(torch.int64), k, right=True) - 1 + r_first
        col = b.ci[k0:k1].to(torch.int64)
        val = c.val(k + shift)
        for z, u in zip(zs, us):
            z.index_add_(0, col, val * u[r])
    return [z.to(torch.float32) for z in zs]


def _products(torch, capi, T, g, vectors, rep, tag):
    for v, vname in ((TI, "SPMV_TILED"), (S, "SPMV_SCALAR")):
        T.plan(v)
        for uname, uf, exp in vectors:
            for fill in (float("nan"), SENTINEL):
                g.y.fill_(fill)
                T.run(v, uf, g.y)
                torch.cuda.synchronize()
                if not g.guards_intact():
                    rep.fail(f"{tag} {vname} {uname}: a run wrote outside y[0, rows)")
                bad = _diff(torch, g.y, exp)
                if bad:
                    rep.fail(f"{tag} {vname} {uname} (y filled with {fill}): {bad}")
        rep.d["paths"][f"{tag}/{vname}"] = "see failures" if rep.d["failures"] else "exact on all rows, both vectors"
        rep.save()


def run_case(c, rep, torch, dev, capi):
    t_start = time.time()
    start_free = _free(torch)
    low = [start_free]

    def sample():
        low[0] = min(low[0], torch.cuda.mem_get_info()[0])

    need = bytes_needed(c)
    rep.note("sizes", f"rows={c.rows} cols={c.cols} nnz={c.nnz} needs={need / GIB:.1f} GiB free={start_free / GIB:.1f} GiB")
    if start_free < need:
        rep.fail(f"{c.name}: {start_free / GIB:.1f} GiB of device memory free, the case needs {need / GIB:.1f} GiB")
        return
    b = L.build(c, torch, dev)
    del b.exp, b.x
    torch.cuda.synchronize()
    rep.note("build_s", round(time.time() - t_start, 1))
    A = capi.CsrMatrix.from_device(c.rows, c.cols, b.rp, b.ci, b.va)
    t0 = time.time()
    T = A.transpose(keep_map=True)
    rep.note("transpose_s", round(time.time() - t0, 2))
    sample()
    try:
        if (T.rows, T.cols, T.nnz) != (c.cols, c.rows, c.nnz):
            rep.fail(f"dims of T: {(T.rows, T.cols, T.nnz)}")
        if T.transpose_map_bytes() != 4 * c.nnz:
            rep.fail(f"transpose_map_bytes: {T.transpose_map_bytes()}")
        capi.check(capi.lib().spmv_csr_validate(T._h, 0))
        first, last = L._at(b.rp, torch, 0) - 1, int(torch.searchsorted(
            b.rp, torch.tensor([c.nnz], dtype=torch.int32, device=dev), right=False).item()) - 1
        if T.column_range() != (first, last):
            rep.fail(f"column_range(T) = {T.column_range()}, the first and last non-empty rows are {(first, last)}")
        # structure: row_ptr against the device bincount
        cnt = torch.zeros(c.cols, dtype=torch.int32, device=dev)
        for k0 in range(0, c.nnz, L.SLAB):
            col = b.ci[k0:k0 + L.SLAB].to(torch.int64)
            cnt.index_add_(0, col, torch.ones(col.numel(), dtype=torch.int32, device=dev))
        longest = int(cnt.max().item())
        rep.note("longest_row_of_T", longest)
        assert 16 * longest < L.EXACT_LIMIT, f"a row of T holds {longest} nonzeros: the products are not exact"
        t_rp = _download(torch, dev, capi, T, 0)
        if int(t_rp[0].item()) != 0 or int(t_rp[-1].item()) != c.nnz:
            rep.fail(f"t.row_ptr[0] = {int(t_rp[0].item())}, t.row_ptr[rows] = {int(t_rp[-1].item())}")
        for j0 in range(0, c.cols, L.SLAB):
            j1 = min(c.cols, j0 + L.SLAB)
            if not torch.equal(t_rp[j0 + 1:j1 + 1] - t_rp[j0:j1], cnt[j0:j1]):
                rep.fail(f"t.row_ptr differences differ from bincount(col_idx) in rows [{j0}, {j1}) of T")
                break
        del cnt
        # structure: col_idx non-decreasing inside every row of T
        starts = torch.zeros(c.nnz + 1, dtype=torch.bool, device=dev)
        for j0 in range(0, c.cols + 1, L.SLAB):
            starts[t_rp[j0:j0 + L.SLAB].to(torch.int64).clamp_(0, c.nnz)] = True
        del t_rp
        t_ci = _download(torch, dev, capi, T, 1)
        sample()
        if int(t_ci.min().item()) < 0 or int(t_ci.max().item()) >= c.rows:
            rep.fail("t.col_idx leaves [0, rows of A)")
        for k0 in range(1, c.nnz, L.SLAB):
            k1 = min(c.nnz, k0 + L.SLAB)
            down = (t_ci[k0:k1] < t_ci[k0 - 1:k1 - 1]) & ~starts[k0:k1]
            if bool(down.any().item()):
                rep.fail(f"t.col_idx decreases inside a row of T near position {k0 + int(down.nonzero()[0, 0].item())}")
                break
        del t_ci, starts
        torch.cuda.empty_cache()
        rep.d["paths"]["structure"] = "see failures" if rep.d["failures"] else "row_ptr = bincount, rows of T sorted, validate, column_range"
        rep.save()
        # exact products, as built and after the values have been rewritten and refreshed through the map
        u1f, u1i = _vector(c, torch, dev, 1, 0)
        u2f, u2i = _vector(c, torch, dev, 3, 1)
        g = Guarded(torch, dev, c.cols, 1)
        for tag, shift in (("as built", 0), ("after transpose_values", SHIFT)):
            if shift:
                for k0 in range(0, c.nnz, L.SLAB):
                    k = torch.arange(k0, min(c.nnz, k0 + L.SLAB), dtype=torch.int64, device=dev)
                    b.va[k0:k0 + k.numel()] = c.val(k + shift).to(torch.float32)
                T.transpose_values(A)
            e1, e2 = _expected(c, b, torch, dev, (u1i, u2i), shift)
            sample()
            _products(torch, capi, T, g, (("u", u1f, e1), ("u2", u2f, e2)), rep, tag)
            sample()
            del e1, e2
    finally:
        T.close()
        A.close()
    rep.note("peak_device_GiB", round((start_free - low[0]) / GIB, 2))
    rep.note("case_s", round(time.time() - t_start, 1))


def child_main(name, out):
    """One case in a process of its own: a warm-up (the case at 1/64), then the case, then the memory that must be back."""
    sys.path.insert(0, os.fspath(ROOT))
    import torch
    import __graft_entry__ as ge
    capi = ge.load_package().capi
    dev = torch.device("cuda:0")
    rep = Report(out)
    warm = Report(None)
    run_case(L.case(name, scaled=True), warm, torch, dev, capi)
    if warm.d["failures"]:
        rep.fail(f"the warm-up (the case at 1/64) failed: {warm.d['failures'][:3]}")
    del warm
    gc.collect()
    torch.cuda.empty_cache()
    start_free = _free(torch)
    run_case(L.case(name), rep, torch, dev, capi)
    gc.collect()
    torch.cuda.empty_cache()
    end_free = _free(torch)
    rep.note("free_start_end_MiB", [start_free // MIB, end_free // MIB])
    if start_free - end_free > 2 * MIB:
        rep.fail(f"{(start_free - end_free) / MIB:.1f} MiB of device memory did not come back")
    rep.d["done"] = True
    rep.save()
    print(f"{name}: {len(rep.d['failures'])} failure(s), {rep.d['wall_s']} s", flush=True)


# ---- the parent ------------------------------------------------------------------------------------------------------------
_abnormal = []


@pytest.mark.parametrize("name", ORDER)
def test_scaled_cases(pkg, gpu, name):
    """The same formulas at 1/64, in this process: a formula or harness mistake shows here before anything giant is allocated."""
    import torch
    rep = Report(None)
    run_case(L.case(name, scaled=True), rep, torch, gpu, pkg.capi)
    print(_summary(name + "/64", rep.d))
    assert not rep.d["failures"], f"{name}/64: {len(rep.d['failures'])} failure(s):\n" + "\n".join(rep.d["failures"])
    assert len(rep.d["paths"]) == 5


@pytest.mark.parametrize("name", ORDER)
def test_giant_cases(pkg, gpu, tmp_path, name):
    if _abnormal:
        pytest.fail(f"not run: an earlier case ended abnormally ({_abnormal[0]})")
    out = tmp_path / "report.json"
    cmd = [sys.executable, os.fspath(Path(__file__).resolve()), name, os.fspath(out)]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[name])
        rc, tail = r.returncode, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    except subprocess.TimeoutExpired as e:
        rc, tail = "time limit", str(e.stdout)[-3000:]
    d = json.loads(out.read_text()) if out.exists() else {}
    print(_summary(name, d) + f"\n  child: {time.time() - t0:.0f} s of at most {LIMIT[name]} s")
    keep = os.environ.get("SPMV_LIMITS_REPORTS")
    if keep and d:
        (Path(keep) / f"transpose_{name}.json").write_text(json.dumps(d, indent=1))
    if rc != 0 or not d.get("done"):
        _abnormal.append(f"{name}: exit {rc}")
        pytest.fail(f"{name}: the child ended abnormally (exit {rc}) after {time.time() - t0:.0f} s; its last steps: "
                    f"{list(d.get('paths', {}))[-3:]}\n{tail}")
    assert not d["failures"], f"{name}: {len(d['failures'])} failure(s):\n" + "\n".join(d["failures"])
    assert len(d["paths"]) == 5, "a step was left out"


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
