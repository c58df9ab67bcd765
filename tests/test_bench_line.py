"""bench.py as the driver calls it: the pieces that need no GPU here, the whole line on the GPU box.

A plain run times the headline alone (and writes y with --dump-outputs); --full adds the rest.  The full line's roofline
is the north-star's quantity (rocprofv3 FETCH_SIZE / WRITE_SIZE bytes over the kernel time), measured by child passes
inside the run; `python3 bench.py --gpus N` starts its own ranks (the reference drives everything from one process,
its test/main.cpp:3-7)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _csv(path, rows):
    head = ('"Correlation_Id","Dispatch_Id","Agent_Id","Queue_Id","Process_Id","Thread_Id","Grid_Size","Kernel_Id","Kernel_Name",'
            '"Workgroup_Size","LDS_Block_Size","Scratch_Size","VGPR_Count","Accum_VGPR_Count","SGPR_Count","Counter_Name",'
            '"Counter_Value","Start_Timestamp","End_Timestamp"\n')
    with open(path, "w") as f:
        f.write(head)
        for i, (grid, wg, name, counter, value) in enumerate(rows, 1):
            f.write(f'{i},{i},"Agent 2",1,1,1,{grid},1,"{name}",{wg},0,0,8,0,16,"{counter}",{value},{i * 10},{i * 10 + 5}\n')


def test_counter_file_is_cut_at_the_markers(tmp_path):
    """A per-dispatch counter file is attributed to workloads by the marker dispatches (grid / 64 = id), in dispatch
    order, whatever order the rows are written in; rows of another counter are ignored."""
    import bench
    d = tmp_path / "fetch" / "host"
    d.mkdir(parents=True)
    rows = [(64, 64, "spmv::k_marker()", "FETCH_SIZE", 0.0),
            (1 << 20, 256, "spmv::k_calib_stream(a)", "FETCH_SIZE", 512.0),
            (1 << 20, 256, "spmv::k_calib_stream(a)", "FETCH_SIZE", 512.0),
            (300 * 64, 64, "spmv::k_marker()", "FETCH_SIZE", 0.0),
            (4096, 256, "void spmv::k_tiled_mixed<512, false>(x)", "FETCH_SIZE", 1000.0),
            (4096, 256, "spmv::k_carry_fixup(x)", "FETCH_SIZE", 10.0),
            (4096, 256, "void spmv::k_tiled_mixed<512, false>(x)", "WRITE_SIZE", 77.0),
            (4096, 256, "void spmv::k_tiled_mixed<512, false>(x)", "FETCH_SIZE", 1000.0),
            (4096, 256, "spmv::k_carry_fixup(x)", "FETCH_SIZE", 10.0)]
    _csv(d / "1_counter_collection.csv", rows)
    seg = bench.cut_counter_file(tmp_path / "fetch", "FETCH_SIZE")
    assert seg[1]["kib"] == 1024.0 and seg[1]["dispatches"] == 2
    assert seg[300]["kib"] == 2020.0 and seg[300]["dispatches"] == 4
    assert max(seg[300]["kernels"], key=seg[300]["kernels"].get).startswith("void spmv::k_tiled_mixed")


def test_frac_fields_carry_their_flags():
    """No field named *frac* may pass the copy ceiling without the flag that says why."""
    import bench
    alg = 2_348_810_244
    f = bench.rate_fields("auto_", int(0.78 * alg), alg, 0.3192)           # the round-3 headline: 0.92 algorithmic, 0.72 moved
    assert 0.70 < f["auto_frac_hbm"] < 0.74 and "exceeds_copy_ceiling" not in f
    assert f["auto_effective_frac"] > 0.9 and "effective_exceeds_copy_ceiling" in f
    g = bench.rate_fields("auto_", None, alg, 1.0)
    assert "auto_frac_hbm" not in g and "effective_exceeds_copy_ceiling" not in g
    h = bench.rate_fields("auto_", int(7.9 * alg), alg, 2.7)               # counted above what HBM can deliver: flagged
    assert h["auto_frac_hbm"] > 0.79 and "Infinity Cache" in h["exceeds_copy_ceiling"]


def test_replay_only_under_the_same_plan():
    import bench
    tj = json.loads((ROOT / "profiles" / "traffic.json").read_text())
    key, ent = next(iter(tj.items()))
    b, src = bench.replayed_traffic(key, ent["plan"])
    assert b == ent["hbm_bytes_per_launch"] and "replayed" in src
    b, src = bench.replayed_traffic(key, ent["plan"] + " changed=1")
    assert b is None and "another plan" in src


def test_plain_run_leaves_the_rest_to_full():
    """A plain run replays the committed traffic figure and times the headline only; --full measures the traffic in the
    run and adds the extras (N = 1) or the other exchange modes (N > 1); --steps is the number of timed steps."""
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.steps, a.warmup, a.traffic, a.exchange, bench.with_extras(a)) == (False, 7, 2, "replay", "allgather", False)
    f = bench.parse(["--gpus", "1", "--full"])
    assert (f.traffic, f.exchange, bench.with_extras(f)) == ("measure", "all", True)
    assert not bench.with_extras(bench.parse(["--full", "--no-extras"]))
    assert bench.parse(["--gpus", "2"]).traffic == "measure"          # nothing committed to replay for N > 1
    assert bench.parse(["--traffic", "off"]).traffic == "off"
    for bad in (["--steps", "0"], ["--gpus", "2", "--exchange", "all"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_dump_outputs_is_whole_or_a_fixed_sample_within_the_budget(tmp_path):
    """--dump-outputs: a y that fits is written whole; a larger one as the same seeded sample of rows every time, float32,
    within the budget."""
    import torch
    import bench
    small = torch.arange(1000, dtype=torch.float32)
    bench.dump_outputs(tmp_path / "s", torch, small)
    assert [p.name for p in (tmp_path / "s").iterdir()] == ["y.npy"]
    assert np.array_equal(np.load(tmp_path / "s" / "y.npy"), small.numpy())
    big = torch.arange(bench.DUMP_BUDGET_BYTES // 4 + 1, dtype=torch.float32)   # the values are the row numbers (< 2^24)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, torch, big)
        assert [p.name for p in (tmp_path / d).iterdir()] == ["y_sample.npy"]
        assert (tmp_path / d / "y_sample.npy").stat().st_size <= bench.DUMP_BUDGET_BYTES
    a, b = np.load(tmp_path / "a" / "y_sample.npy"), np.load(tmp_path / "b" / "y_sample.npy")
    assert a.dtype == np.float32 and a.size == bench.DUMP_SAMPLE_ROWS and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[-1] < big.numel()             # distinct rows, ascending


def _line(cmd, timeout):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py")] + cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), p.stderr


@pytest.mark.gpu
def test_headline_traffic_is_measured_in_the_run(built, gpu):
    """N = 1, a small matrix of the headline's laws: the two rocprofv3 child passes run before the first GPU call, the
    line's roofline is counters / time, the calibration kernels give the guide's factors (2.0 for 16-byte streams; a
    missing gather is one 128-byte request tallied like a stream's; stores exact)."""
    import shutil
    if shutil.which("rocprofv3") is None and not Path("/opt/rocm/bin/rocprofv3").exists():
        pytest.skip("no rocprofv3 on this box")
    out, err = _line(["--full", "--config", "c2", "--band", "8192", "--no-extras", "--no-cpu-baseline", "--steps", "5", "--warmup", "2"], 900)
    r = out["roofline"]
    assert "measured in this run" in r["traffic_source"], (r["traffic_source"], err[-1500:])
    assert r["traffic"] > 0 and abs(r["frac"] - r["traffic"] / (r["kernel_ms"] * 1e-3) / 8e12) < 2e-3
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-3
    cal = r["calibration"]
    assert 1.9 < cal["read_factor_16B_stream"] < 2.1
    assert 0.9 < cal["write_factor_4B_per_lane"] < 1.1
    assert cal["one_read_factor_valid"] is True, cal
    # c2 band 8192 through the tiled plan reads 16-bit columns: it moves fewer bytes than the CSR-algorithmic count
    assert 0.5 < r["traffic_over_algorithmic"] < 1.2
    assert out["value"] == pytest.approx(r["traffic"] * out["steps"] / (out["ms_per_step"] * out["steps"] * 1e-3) / 1e9, rel=2e-3)
    assert r["effective_frac"] == pytest.approx(out["config"]["algorithmic_bytes_per_gpu"] / (r["kernel_ms"] * 1e-3) / 8e12, abs=2e-3)


@pytest.mark.gpu
def test_bench_starts_its_own_ranks_gloo(built, gpu):
    """`python3 bench.py --gpus 2` with no launcher: two ranks appear, share the one device (the line says so), y is
    exchanged through gloo; the extra exchange modes of --exchange all run under the watchdog."""
    out, err = _line(["--full", "--gpus", "2", "--backend", "gloo", "--no-extras", "--no-cpu-baseline", "--steps", "2", "--warmup", "1",
                      "--rows-per-gpu", str(1 << 20), "--traffic", "off"], 900)
    assert out["n_gpus"] == 2 and "RANKS SHARE DEVICES" in out["config"]["devices"]
    assert out["config"]["launch"] == "bench.py started its own ranks"
    assert out["exchange_only_ms"] is not None
    modes = out["exchange_modes"]
    assert "watchdog" not in modes
    peer = modes["native peer_store (one process, bin/spmv_dist_selftest)"]
    assert "error" not in peer, peer
    assert modes["torch p2p"]["y_bit_identical_to_headline"] is True


@pytest.mark.gpu
def test_bench_starts_its_own_ranks_native(built, gpu):
    """--backend native with fewer devices than ranks: the C++ pipeline with all ranks in one process (peer stores),
    every rank's y bit-identical to the single handle."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one device: the native backend runs one process per GPU over RCCL here")
    out, err = _line(["--gpus", "2", "--backend", "native", "--no-extras", "--no-cpu-baseline", "--steps", "2"], 900)
    assert out["n_gpus"] == 2 and "RANKS SHARE DEVICES" in out["config"]["devices"]
    assert out["rows_differing_from_single_handle"] == 0


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_they_computed(built, gpu, oracle, tmp_path):
    """A plain N = 1 run: exactly --steps timed steps, the headline fields and nothing of --full; --dump-outputs writes the
    y of the timed path, within 1e-5 of the fp64 oracle and bit for bit the same in a second run with the same arguments."""
    from _util import assert_close_to_oracle
    ys = []
    for d in ("a", "b"):
        out, err = _line(["--gpus", "1", "--config", "c2", "--band", "8192", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(tmp_path / d)], 600)
        assert (out["steps"], out["warmup"], out["unit"], out["higher_is_better"], out["dtype"]) == (7, 2, "GB/s", True, "f32")
        assert out["metric"].startswith("fp32 CSR SpMV") and out["value"] > 0 and out["ms_per_step"] > 0
        basis = out["config"]["hbm_bytes_per_gpu"] or out["config"]["algorithmic_bytes_per_gpu"]
        assert out["value"] == pytest.approx(basis / (out["ms_per_step"] * 1e-3) / 1e9, rel=2e-3)
        for key in ("roofline", "cpu_baseline", "other_workloads", "multiply_only_ms", "vendor_dense_slot"):
            assert key not in out, key
        ys.append(np.load(tmp_path / d / "y.npy"))
    pkg = built
    W = pkg.workloads
    w = W.config("c2", band=8192)
    rp = W.row_ptr(w)
    ci, va = oracle.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, rp)
    y64, mag = oracle.spmv_f64(rp, ci, va, oracle.synth_x(w.seed, 0, w.cols))
    assert ys[0].dtype == np.float32 and ys[0].shape == (w.rows,)
    assert_close_to_oracle(ys[0], y64, mag, "bench --dump-outputs")
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32))
