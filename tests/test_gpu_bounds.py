"""GPU (-m gpu): the streams of the panel family that read or write past a tile's or a bin's end on purpose stay inside what
their plans allocate.

A kernel can compute the right y while it reads outside its allocation: what it reads past the end counts for nothing, and
the values tests cannot see it -- until the memory behind the array is not mapped.  lib/libspmv_hip_checked.so is the library
compiled with SPMV_CHECK_BOUNDS: the sum launches of both binned flavours (k_bs_sums, k_bin_sums), the scattered product
launch (k_bs_products), the scattered plan's fill (k_bs_group, k_bs_place, k_bs_fill) and the panel sweep's stream (k_panel)
check every access against the array's allocated bytes, record a violation instead of issuing the access, and go on
(csrc/spmv_internal.hpp).  The case list runs in ONE fresh child process bound to that library; the parent then asks, case by
case: no violation, y within the fp64 oracle's bound, and y bit-identical to the normal library's under the same plan (the
instrumentation changes nothing).  The cases aim at the sum launch's read-ahead (it issues two register sets of pieces ahead
of the trip it consumes): a last bin of one piece, empty last bins, a single nonzero, bins of exactly whole pieces."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

# ---- the matrices: host arrays (rows, cols, row_ptr, col_idx, vals, x), built the same way in the child and the parent ----
SYNTH = {"c2/4": ("c2", None, 1 / 4), "c4/16": ("c4", None, 1 / 16), "c4_band1M/16": ("c4", 1000000, 1 / 16)}


def _rows_of(lengths, cols, seed, panel_of=None):
    """CSR with the given row lengths, columns uniform over [0, cols) (sorted per row) -- or, with panel_of(row), inside
    that row's panel of 2^15 columns."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = np.asarray(lengths, np.int64)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    nnz = int(rp[-1])
    if panel_of is None:
        ci = rng.integers(0, cols, size=nnz)
    else:
        rows = np.repeat(np.arange(len(lengths)), lengths)
        ci = panel_of(rows) * 32768 + rng.integers(0, 32768, size=nnz)
    ci = ci.astype(np.int32)
    for r in range(len(lengths)):
        ci[rp[r]:rp[r + 1]].sort()
    va = rng.uniform(-1, 1, size=nnz).astype(np.float32)
    x = rng.uniform(-1, 1, size=cols).astype(np.float32)
    return len(lengths), cols, rp, ci, va, x


def _wide():
    """2^16 x 2^23, 64 nonzeros per row: 256 panels, more than one group of 64 -- the scattered plan's two-pass fill runs
    k_bs_group."""
    rows, cols, per = 1 << 16, 1 << 23, 64
    rng = np.random.Generator(np.random.PCG64(11))
    ci = np.sort(rng.integers(0, cols, size=(rows, per)), axis=1).astype(np.int32).ravel()
    rp = np.arange(0, rows * per + 1, per, dtype=np.int32)
    va = rng.uniform(-1, 1, size=rows * per).astype(np.float32)
    x = rng.uniform(-1, 1, size=cols).astype(np.float32)
    return rows, cols, rp, ci, va, x


# small matrices: with fewer rows than the sum launch keeps wavefronts resident, every bin is one row -- so the row lengths
# ARE the bins' entry counts
SMALL = {
    "last_bin_one_piece": lambda: _rows_of(np.full(1000, 100), 100_000, 1),
    "last_bins_empty": lambda: _rows_of(np.concatenate([np.full(900, 50), np.zeros(100, np.int64)]), 100_000, 2),
    "single_nonzero": lambda: _rows_of([1], 1, 3),
    "single_nonzero_last_row": lambda: _rows_of([0, 0, 0, 0, 1], 70_000, 4),
    "whole_pieces_256": lambda: _rows_of(np.full(600, 256), 200_000, 5),
    "whole_pieces_512": lambda: _rows_of(np.full(300, 512), 200_000, 6),
    # every row alone in its (bin, panel) tile and 256 times in it: a step of the sum launch holds the row 128 times.  Four
    # rows a bin: spare accumulators; sixteen: more than a bin has -- the bin adds with LDS atomics (flagged; mode 4 flags
    # the tiles of bins whose rows need more than 512 spare sums: four rows of 512)
    "spare_rows": lambda: _rows_of(np.full(2048, 256), 64 * 32768, 7, panel_of=lambda r: r % 64),
    "flagged_bins": lambda: _rows_of(np.full(8192, 512), 64 * 32768, 8, panel_of=lambda r: r % 64),
}


def build_matrix(name, orc, pkg):
    if name in SYNTH:
        cfg, band, scale = SYNTH[name]
        w = pkg.workloads.config(cfg, band=band, scale=scale)
        rp = pkg.workloads.row_ptr(w)
        ci, va = orc.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, rp)
        return w.rows, w.cols, rp, ci, va, orc.synth_x(w.seed, 0, w.cols)
    if name == "wide":
        return _wide()
    return SMALL[name]()


# ---- the cases: (matrix, params[6] mode, params[4] rows per bin, environment of the plan) --------------------------------
def _cases():
    out = []
    for m in ("c2/4", "c4/16", "c4_band1M/16", "wide"):
        out += [(m, 5, rows, {}) for rows in (0, 4096, 8192, 16384)]
        out += [(m, 4, rows, {}) for rows in (0, 2048, 4096, 8192)]
        out += [(m, 4, 0, {"SPMV_BINNED_WIDE": wide}) for wide in ("0", "1")]
    out += [("wide", 5, 0, {"SPMV_BS_FILL": "1"})]                     # the one-pass fill (k_bs_fill)
    for m in SMALL:
        out += [(m, 5, rows, {}) for rows in (4096, 16384)]
        out += [(m, 4, 0, {"SPMV_BINNED_WIDE": wide}) for wide in ("0", "1")]
    for m in ("c2/4", "c4_band1M/16", "last_bin_one_piece", "single_nonzero"):
        out += [(m, 1, 0, {"SPMV_PANEL_STEP": step}) for step in ("4", "8")]   # the panel sweep through L2 (k_panel)
    return out


CASES = _cases()


def case_id(c):
    m, mode, rows, env = c
    return f"{m}-mode{mode}-rows{rows}" + "".join(f"-{k}={v}" for k, v in sorted(env.items()))


def plan_and_run(capi, A, d_x, d_y, case):
    """Plan the case on handle A (its environment set while the plan is made) and run it once; y on the host."""
    import torch
    _, mode, rows, env = case
    for k, v in env.items():
        os.environ[k] = v
    try:
        A.plan_set(capi.PANEL, [capi.PANEL, 0, 0, 0, rows, 0, mode, 0])
    finally:
        for k in env:
            os.environ.pop(k, None)
    d_y.fill_(float("nan"))
    A.run(capi.PANEL, d_x, d_y)
    torch.cuda.synchronize()
    return d_y.cpu().numpy().copy()


def _upload(capi, dev, mat):
    import torch
    rows, cols, rp, ci, va, x = mat
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, ci, va, x)]
    d_y = torch.empty(max(rows, 1), dtype=torch.float32, device=dev)
    A = capi.CsrMatrix.from_device(rows, cols, t[0], t[1], t[2])
    return A, t, d_y


def child_main(outdir):
    """The child: every case through the checked library; y_<i>.npy + report.json (violations, plan description) per case."""
    sys.path.insert(0, os.fspath(ROOT))
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    capi = pkg.capi
    capi.use_library(capi.CHECKED_LIB_PATH)
    orc = ge.load_oracle()
    dev = torch.device("cuda:0")
    capi.debug_bounds()                                                  # (a clean table)
    report, cur, held = [], None, None
    for i, case in enumerate(CASES):
        if case[0] != cur:
            if held is not None:
                held[0].close()
            cur = case[0]
            held = _upload(capi, dev, build_matrix(cur, orc, pkg))
        A, t, d_y = held
        y = plan_and_run(capi, A, t[3], d_y, case)
        np.save(Path(outdir) / f"y_{i}.npy", y)
        report.append({"case": case_id(case), "violations": capi.debug_bounds(), "describe": A.plan_describe(capi.PANEL)})
        (Path(outdir) / "report.json").write_text(json.dumps(report, indent=1))
    if held is not None:
        held[0].close()
    print(f"{len(CASES)} cases through the checked library; "
          f"{sum(1 for r in report if r['violations'])} with violations")


@pytest.fixture(scope="module")
def checked_run(pkg, gpu, tmp_path_factory):
    """Run the child once for the module (a timeout, no retry)."""
    assert pkg.capi.CHECKED_LIB_PATH.exists(), f"{pkg.capi.CHECKED_LIB_PATH} missing: build() makes it"
    out = tmp_path_factory.mktemp("bounds")
    r = subprocess.run([sys.executable, os.fspath(Path(__file__).resolve()), os.fspath(out)], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, f"the checked child failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    report = json.loads((out / "report.json").read_text())
    assert [r["case"] for r in report] == [case_id(c) for c in CASES]
    yield out, report
    for v in _held.values():
        v["A"].close()
    _held.clear()


_held = {}


def _matrix(name, oracle, pkg, gpu):
    """The parent's copy of a matrix (host arrays, device upload, fp64 oracle), one at a time: the cases come grouped."""
    if name not in _held:
        for v in _held.values():
            v["A"].close()
        _held.clear()
        mat = build_matrix(name, oracle, pkg)
        A, t, d_y = _upload(pkg.capi, gpu, mat)
        rows, cols, rp, ci, va, x = mat
        y64, mag = oracle.spmv_f64(rp, ci, va, x)
        _held[name] = {"A": A, "t": t, "d_y": d_y, "rows": rows, "y64": y64, "mag": mag}
    return _held[name]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_checked_streams_stay_inside_their_allocations(pkg, oracle, gpu, checked_run, i):
    from _util import assert_close_to_oracle
    out, report = checked_run
    case, rec = CASES[i], report[i]
    assert rec["violations"] == [], f"{rec['case']}: out-of-bounds accesses [site, count, largest overrun in bytes] {rec['violations']}"
    m = _matrix(case[0], oracle, pkg, gpu)
    y = np.load(out / f"y_{i}.npy")[:m["rows"]]
    assert not np.isnan(y).any(), "rows left unwritten"
    assert_close_to_oracle(y, m["y64"], m["mag"], rec["case"])
    y_normal = plan_and_run(pkg.capi, m["A"], m["t"][3], m["d_y"], case)[:m["rows"]]
    assert m["A"].plan_describe(pkg.capi.PANEL) == rec["describe"]
    assert np.array_equal(y.view(np.uint32), y_normal.view(np.uint32)), f"{rec['case']}: the checked build's y differs from the normal one"


@pytest.mark.gpu
def test_bounds_cases_reach_every_path(checked_run):
    """The list is worth its name: both flavours, the scattered sum launch's atomics (flagged bins) and spare accumulators,
    both piece widths of mode 4 and both steps of the panel sweep."""
    _, report = checked_run
    desc = [r["describe"] for r in report]

    def field(d, key):
        return int(d.split(f"{key}=")[1].split()[0])

    scattered = [d for d in desc if d.startswith("binned scattered_products ")]
    assert any(field(d, "flagged_bins") > 0 for d in scattered), "no case reaches a flagged bin (LDS atomics)"
    assert any(field(d, "rows_with_spare_sums") > 0 for d in scattered), "no case reaches spare accumulators"
    binned = [d for d in desc if d.startswith("binned bins=")]
    assert {field(d, "products_per_lane") for d in binned} == {2, 4}
    assert any(field(d, "flagged_tiles") > 0 for d in binned) and any(field(d, "long_rows") > 0 for d in binned)
    assert sum(d.startswith("panel_columns=") for d in desc) == 8


if __name__ == "__main__":
    child_main(sys.argv[1])
