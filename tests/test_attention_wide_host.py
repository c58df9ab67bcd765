"""The wide fused-attention calls without a device (include/spmv_hip.h "Fused attention at head widths up to 128"): the five
symbols are declared, exported and bound with the _bias calls' argument lists, the CsrMatrix methods and the holder's `wide`
argument exist, and a null handle is refused.  The numpy statement of the documented order at V = 32 lanes and steps of
T_wide nonzeros (tests/_attention_wide.py) stays inside the written-down fp64 bound of tests/test_attention_host.py on rows
of 1 to 1600 entries, has the zero-padding property bit for bit, tells every order mistake apart on the data
tests/test_gpu_attention_wide.py runs, and hands expf only arguments whose result any 1-ulp expf gets exactly on every
forward data set of that file.
"""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _attention_bias as AB
import _attention_order as AO
import _attention_wide as AW
import _order_cases as OC

ROOT = Path(__file__).resolve().parent.parent
f32, f64 = np.float32, np.float64
RTOL, EPS = 1e-5, 2.0 ** -24          # (tests/test_attention_host.py)
NAMES = {"spmv_csr_attention_plan_wide": 3, "spmv_csr_attention_max_heads_wide": 3, "spmv_csr_attention_forward_wide": 19,
         "spmv_csr_attention_backward_q_wide": 26, "spmv_csr_attention_backward_kv_wide": 24}      # name -> number of arguments
FORWARD_CASES = ("maxima", "stats_q0", "stats_k0")      # the exact-expf data sets the GPU test runs the forward pass on


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_the_five_symbols_are_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert name in normal and name in checked, f"{name} not exported"
    for p in ("forward", "backward_q", "backward_kv"):      # exactly the _bias call's argument list
        assert capi.SIGNATURES[f"spmv_csr_attention_{p}_wide"] == capi.SIGNATURES[f"spmv_csr_attention_{p}_bias"]
        a = re.search(rf"spmv_csr_attention_{p}_bias\((.*?)\);", header, re.S).group(1)
        b = re.search(rf"spmv_csr_attention_{p}_wide\((.*?)\);", header, re.S).group(1)
        assert re.sub(r"\s+", " ", a) == re.sub(r"\s+", " ", b), f"{p}: the header's argument lists differ"
    assert AW.T_WIDE in (8, 16) and f"T_wide = SPMV_ATTN_WIDE_STEP = {AW.T_WIDE} " in header


def test_the_python_layer_has_the_wide_calls(pkg):
    capi, sa = pkg.capi, pkg.sparse_attention
    for m in ("attention_plan_wide", "attention_max_heads_wide", "attention_forward_wide", "attention_backward_q_wide",
              "attention_backward_kv_wide"):
        assert callable(getattr(capi.CsrMatrix, m, None)), f"CsrMatrix.{m} missing"
    for m in ("attention_forward_wide", "attention_backward_q_wide", "attention_backward_kv_wide"):
        p = inspect.signature(getattr(capi.CsrMatrix, m)).parameters
        assert [n for n in p if n.startswith("bias")] and all(p[n].default is None for n in p if n.startswith("bias")), m
    wide = inspect.signature(sa.FusedSparseAttention.__init__).parameters["wide"]
    assert wide.default is False
    assert sa.MAX_K == 64 and sa.WIDE_MAX_K == 128


def test_the_wide_calls_refuse_a_null_handle(pkg):
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    hs = capi.AttnHeads(heads=1)
    assert lib.spmv_csr_attention_plan_wide(None, 1, None) == capi.ERR_INVALID
    assert "spmv_csr_attention_plan_wide:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_attention_max_heads_wide(None, 128, 128) == capi.ERR_INVALID
    assert "spmv_csr_attention_max_heads_wide:" in lib.spmv_last_error().decode()
    r = lib.spmv_csr_attention_forward_wide(None, C.byref(hs), 1, 0, None, 0, 1.0, 128, p, 128, p, 128, 128, p, 128, p, 128, p, None)
    assert r == capi.ERR_INVALID and "spmv_csr_attention_forward_wide:" in lib.spmv_last_error().decode()
    r = lib.spmv_csr_attention_backward_q_wide(None, C.byref(hs), 1, 0, None, 0, None, 0, 1.0, 128, p, 128, p, 128, 128, p, 128, p, 128, p,
                                               128, p, p, p, 128, None)
    assert r == capi.ERR_INVALID and "spmv_csr_attention_backward_q_wide:" in lib.spmv_last_error().decode()
    r = lib.spmv_csr_attention_backward_kv_wide(None, C.byref(hs), 1, 0, None, 0, 1.0, 128, p, 128, p, 128, 128, p, 128, p, 128, p, p, p,
                                                128, p, 128, None)
    assert r == capi.ERR_INVALID and "spmv_csr_attention_backward_kv_wide:" in lib.spmv_last_error().decode()


# ---- the emulation at V = 32 against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kv", [(128, 128), (97, 66)])
def test_the_emulated_order_at_32_lanes_against_fp64_dense_attention(k, kv):
    """The bound of tests/test_attention_host.py, word for word: it counts additions, rescalings (A / T with T = T_wide) and
    combine steps, none of which is particular to a geometry."""
    V, T = AW.geometry(k, kv)
    assert (V, T) == (32, AW.T_WIDE)
    worst = [0.0, 0.0]
    for L in (1, 2, 7, 8, 9, 16, 17, 64, 511, 512, 513, 1024, 1025, 1600):
        rng = np.random.Generator(np.random.PCG64([L, k, kv]))
        scale = 2.0 ** -3
        q, Kj, Vj, do = (rng.standard_normal(s).astype(f32) for s in ((k,), (L, k), (L, kv), (kv,)))
        o, M, r = AO.forward_row(q, Kj, Vj, scale, V, T)
        dq, delta = AO.backward_q_row(q, Kj, Vj, o, do, M, r, scale, V)
        t = scale * (Kj.astype(f64) @ q.astype(f64))
        D = t.max() - t.min()
        assert D <= 32.0
        p = np.exp(t - t.max())
        p /= p.sum()
        o64 = p @ Vj.astype(f64)
        dp = Vj.astype(f64) @ do.astype(f64)
        dq64 = (scale * p * (dp - p @ dp)) @ Kj.astype(f64)
        A = min(L, AO.PIECE)
        chain = A + -(-A // T) + (-(-L // AO.PIECE) if L > AO.PIECE else 0)
        bound_o = (RTOL + (2 * D + 12 + 2 * chain) * EPS) * (p @ np.abs(Vj).astype(f64))
        mag = (abs(scale) * p * (np.abs(dp) + p @ np.abs(dp))) @ np.abs(Kj).astype(f64)
        bound_q = (RTOL + (2 * D + 2 * kv + 24 + 3 * chain) * EPS) * mag
        ro, rq = np.max(np.abs(o - o64) / bound_o), np.max(np.abs(dq - dq64) / bound_q)
        worst = [max(worst[0], ro), max(worst[1], rq)]
        assert ro <= 1.0, f"L={L} k={k} kv={kv}: O at {ro:.3g} of its bound"
        assert rq <= 1.0, f"L={L} k={k} kv={kv}: dQ at {rq:.3g} of its bound"
        assert M == np.max((f32(scale) * AO.dot(q, Kj, V)).astype(f32))
    print(f"V = 32, T = {T}, k={k} kv={kv}: the emulated order reaches {worst[0]:.3g} (O) and {worst[1]:.3g} (dQ) of the bounds")


# ---- zero padding -----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("k,kv", [(64, 20), (8, 40), (16, 12)])
def test_zero_padding_to_128_changes_no_bit_in_the_emulation(k, kv):
    """Backward passes on caller-made stats and delta with a general bias, and the forward pass on the exact-expf data: the
    outputs of the operands padded to (128, 128) at (V, T) = (32, T_wide) are the narrow geometry's in the original columns
    and +0 in the padded ones."""
    s = OC.p1()
    tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
    rows, keys = AW.one_row_per_length(s.rp), AW.one_row_per_length(tp)[:4]
    d = OC.attention_data("P1", "stats_k0", k, kv)
    d["K"] = OC.randn(77, d["K"].shape)[0]          # (general scores as well: the bias and the caller-made stats keep p finite)
    bias = (OC.randn(78, (s.nnz,))[0] - f32(40.0)).astype(f32)
    bias_t = AB.transposed_bias(s.ci, bias)
    pad = {n: AW.padded(d[n], 128) for n in ("Q", "K", "V", "dO", "O")}
    assert AW.geometry(k, kv) == AO.geometry(k, kv) and AW.geometry(128, 128) == (32, AW.T_WIDE)
    narrow = AW.attention_backward_q(s.rp, s.ci, d["Q"], d["K"], d["V"], d["O"], d["dO"], d["stats"], d["scale"], bias, only=rows)
    wide = AW.attention_backward_q(s.rp, s.ci, pad["Q"], pad["K"], pad["V"], pad["O"], pad["dO"], d["stats"], d["scale"], bias, only=rows)
    assert np.array_equal(_bits(narrow[0]), _bits(wide[0][:, :k])) and not _bits(wide[0][:, k:]).any(), "dQ"
    assert np.array_equal(_bits(narrow[1]), _bits(wide[1])), "delta"
    assert np.array_equal(_bits(narrow[2]), _bits(wide[2])) and np.isfinite(narrow[2]).any(), "dBias"
    nkv = AW.attention_backward_kv(tp, ti, d["Q"], d["K"], d["V"], d["dO"], d["stats"], d["delta"], d["scale"], bias_t, only=keys)
    wkv = AW.attention_backward_kv(tp, ti, pad["Q"], pad["K"], pad["V"], pad["dO"], d["stats"], d["delta"], d["scale"], bias_t, only=keys)
    assert np.array_equal(_bits(nkv[0]), _bits(wkv[0][:, :k])) and not _bits(wkv[0][:, k:]).any(), "dK"
    assert np.array_equal(_bits(nkv[1]), _bits(wkv[1][:, :kv])) and not _bits(wkv[1][:, kv:]).any(), "dV"
    assert np.abs(narrow[0]).max() > 0 and np.abs(nkv[0]).max() > 0
    m = OC.attention_data("P1", "maxima", k, kv)
    on, sn = AW.attention_forward(s.rp, s.ci, m["Q"], m["K"], m["V"], m["scale"], only=rows)
    ow, sw = AW.attention_forward(s.rp, s.ci, AW.padded(m["Q"], 128), AW.padded(m["K"], 128), AW.padded(m["V"], 128), m["scale"], only=rows)
    assert np.array_equal(_bits(on), _bits(ow[:, :kv])) and not _bits(ow[:, kv:]).any() and np.array_equal(_bits(sn), _bits(sw)), "forward"


# ---- the order mistakes and the premise of the bit comparisons -----------------------------------------------------------------------
def test_each_order_mistake_changes_bits_at_32_lanes():
    """On the data of tests/test_gpu_attention_wide.py (P1, stats_q0 with its caller-made stats, (128, 128); the rows it compares): every mistake
    of the order changes bits of dQ or delta, and the three dot-product mistakes -- a sequential sum, an unfused multiply-add,
    the butterfly run m = 1 .. 16 -- differ from the documented order and from one another."""
    s = OC.p1()
    rows = AW.one_row_per_length(s.rp)
    d = OC.attention_data("P1", "stats_q0", 128, 128)        # (Q = 0: p = r_i; K, V, dO, O general, so dQ and delta are)
    run = lambda wrong: AW.attention_backward_q(s.rp, s.ci, d["Q"], d["K"], d["V"], d["O"], d["dO"], d["stats"], d["scale"],      # noqa: E731
                                                wrong=wrong, only=rows)
    right = run(None)
    got = {w: run(w) for w in AW.ORDER_MISTAKES}
    for w, (dq, delta, _) in got.items():
        changed = int((_bits(dq) != _bits(right[0])).sum()) + int((_bits(delta) != _bits(right[1])).sum())
        assert changed > 0, f"{w} changes no bit"
        print(f"{w}: {changed} values of dQ and delta change bits")
    dots = ("sequential", "unfused", "butterfly_low_first")
    for a in dots:
        assert (_bits(got[a][1]) != _bits(right[1])).any(), f"{a}: delta, a dot product over 128 columns, keeps its bits"
        for b in dots:
            if a < b:
                assert (_bits(got[a][1]) != _bits(got[b][1])).any(), f"{a} and {b} give the same delta"
    assert AO.dot is not AW.dot_low_first


@pytest.mark.parametrize("k,kv", AW.WIDTHS)
def test_every_expf_argument_of_the_forward_bit_comparisons_is_exact(k, kv):
    s = OC.p1()
    rows = AW.one_row_per_length(s.rp)
    for case in FORWARD_CASES:
        d = OC.attention_data("P1", case, k, kv)
        for bias in (None, AB.exact_bias(s, 5)):
            with AO.expf_arguments() as log, AO.without_chains():
                AW.attention_forward(s.rp, s.ci, d["Q"], d["K"], d["V"], d["scale"], bias, only=rows)
            assert log and AO.expf_arguments_are_exact(log), f"{case} k={k} kv={kv} bias={bias is not None}"
