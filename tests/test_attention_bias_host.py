"""Fused attention with an additive bias per nonzero, without a device (include/spmv_hip.h "Fused attention with an additive
bias"): the four new symbols are declared, exported and bound; the documented order with the bias (tests/_attention_bias.py:
t = fl(fl(scale * s) + bias[n]), then tests/_attention_order.py word for word; dBias = fl(p * fl(dp - delta))) stays inside
the written-down bound of tests/test_attention_host.py against fp64 attention with bias on rows of 1 to 5000 entries; a bias
of -0.0 gives the unbiased emulation's bits and a bias of -Inf removes a nonzero exactly; and the premises of
tests/test_gpu_attention_bias.py's bit comparisons hold on its very inputs: every expf argument is +-0, at most -128 or -Inf,
and each mistake the bias invites (_attention_bias.MISTAKES) changes bits of an array that test compares.

The bound of dBias, beside those of O and dQ that tests/test_attention_host.py derives: dBias = p (dp - delta) carries p's
error (2 D + 12) 2^-24, the sums of dp and delta (at most kv + 4 roundings each) and two roundings of its own, relative to
p (|dp| + sum p |dp|): RTOL + (2 D + 2 kv + 24) 2^-24, dQ's bound without its chain.  The bias adds one rounding to t, which
is left to RTOL like the fp32 scores themselves.

Only the first two tests need the library (they fail where the four symbols do not exist); the others hold the emulation of
tests/_attention_bias.py to fp64 and to its premises and need nothing but numpy.
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import _attention_bias as AB
import _attention_order as AO
import _order_cases as OC

ROOT = Path(__file__).resolve().parent.parent
RTOL, EPS = 1e-5, 2.0 ** -24
f32, f64 = np.float32, np.float64
NAMES = {"spmv_csr_attention_forward_bias": 19, "spmv_csr_attention_backward_q_bias": 26, "spmv_csr_attention_backward_kv_bias": 24,
         "spmv_csr_transpose_gather": 7}      # name -> number of arguments


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_the_four_symbols_are_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert name in normal and name in checked, f"{name} not exported"
        getattr(capi.lib(), name)
    assert re.search(r"SPMV_ATTN_FP32\s*=\s*0\b", header) and capi.ATTN_FP32 == 0
    for method in ("attention_forward_bias", "attention_backward_q_bias", "attention_backward_kv_bias", "transpose_gather"):
        assert callable(getattr(capi.CsrMatrix, method, None)), f"CsrMatrix.{method} missing"
    import torch
    assert issubclass(pkg.sparse_attention.BiasedFusedSparseAttentionFunction, torch.autograd.Function)


def test_the_bias_calls_refuse_a_null_handle(pkg):
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    hs = capi.AttnHeads(heads=1)
    assert lib.spmv_csr_attention_forward_bias(None, C.byref(hs), 1, 0, p, 0, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, None) == capi.ERR_INVALID
    assert "spmv_csr_attention_forward_bias:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_attention_backward_q_bias(None, C.byref(hs), 1, 0, p, 0, p, 0, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, 4, p, p, p, 4,
                                                  None) == capi.ERR_INVALID
    assert "spmv_csr_attention_backward_q_bias:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_attention_backward_kv_bias(None, C.byref(hs), 1, 0, p, 0, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, p, p, 4, p, 4,
                                                   None) == capi.ERR_INVALID
    assert "spmv_csr_attention_backward_kv_bias:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_transpose_gather(None, 1, p, 0, p, 0, None) == capi.ERR_INVALID
    assert "spmv_csr_transpose_gather:" in lib.spmv_last_error().decode()


# ---- the documented order with bias against fp64 ------------------------------------------------------------------------------
def test_the_emulated_order_with_bias_against_fp64_attention_with_bias():
    worst = [0.0, 0.0, 0.0]
    for L in (1, 2, 7, 8, 9, 16, 17, 64, 511, 512, 513, 1024, 1025, 4100, 5000):
        for k, kv in ((24, 24), (8, 40), (64, 4), (6, 10)):
            rng = np.random.Generator(np.random.PCG64([L, k, kv, 7]))
            V, T = AO.geometry(k, kv)
            scale = 2.0 ** -2
            q, Kj, Vj, do, b = (rng.standard_normal(s).astype(f32) for s in ((k,), (L, k), (L, kv), (kv,), (L,)))
            o, M, r = AB.forward_row(q, Kj, Vj, b, scale, V, T)
            dq, delta, db = AB.backward_q_row(q, Kj, Vj, b, o, do, M, r, scale, V)
            t = scale * (Kj.astype(f64) @ q.astype(f64)) + b.astype(f64)
            D = t.max() - t.min()
            assert D <= 32.0
            p = np.exp(t - t.max())
            p /= p.sum()
            o64 = p @ Vj.astype(f64)
            dp = Vj.astype(f64) @ do.astype(f64)
            g64 = p * (dp - p @ dp)
            dq64 = (scale * g64) @ Kj.astype(f64)
            A = min(L, AO.PIECE)
            chain = A + -(-A // T) + (-(-L // AO.PIECE) if L > AO.PIECE else 0)
            bound_o = (RTOL + (2 * D + 12 + 2 * chain) * EPS) * (p @ np.abs(Vj).astype(f64))
            g_mag = p * (np.abs(dp) + p @ np.abs(dp))
            bound_q = (RTOL + (2 * D + 2 * kv + 24 + 3 * chain) * EPS) * ((abs(scale) * g_mag) @ np.abs(Kj).astype(f64))
            bound_b = (RTOL + (2 * D + 2 * kv + 24) * EPS) * g_mag
            ro, rq = np.max(np.abs(o - o64) / bound_o), np.max(np.abs(dq - dq64) / bound_q)
            rb = np.max(np.abs(db - g64) / bound_b)
            worst = [max(worst[0], ro), max(worst[1], rq), max(worst[2], rb)]
            assert ro <= 1.0, f"L={L} k={k} kv={kv}: O at {ro:.3g} of its bound"
            assert rq <= 1.0, f"L={L} k={k} kv={kv}: dQ at {rq:.3g} of its bound"
            assert rb <= 1.0, f"L={L} k={k} kv={kv}: dBias at {rb:.3g} of its bound"
            assert M == np.max(((f32(scale) * AO.dot(q, Kj, V)).astype(f32) + b).astype(f32))
    print(f"the emulated order with bias reaches {worst[0]:.3g} (O), {worst[1]:.3g} (dQ) and {worst[2]:.3g} (dBias) of the bounds")


def test_a_bias_of_minus_zero_gives_the_unbiased_bits_and_minus_inf_removes_a_nonzero():
    for L, k, kv, scale in ((9, 6, 10, 0.3), (700, 16, 12, -0.7), (40, 4, 4, 0.3)):
        rng = np.random.Generator(np.random.PCG64([L, k, kv, 11]))
        V, T = AO.geometry(k, kv)
        q, Kj, Vj, do = (rng.standard_normal(s).astype(f32) for s in ((k,), (L, k), (L, kv), (kv,)))
        Kj[::5] = 0                                  # s = +0, and t = -0 at the negative scale: -0 + -0 = -0, x + -0 = x
        mz = np.full(L, -0.0, f32)
        o, M, r = AB.forward_row(q, Kj, Vj, mz, scale, V, T)
        o0, M0, r0 = AO.forward_row(q, Kj, Vj, scale, V, T)
        bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)       # noqa: E731
        assert np.array_equal(bits(o), bits(o0)) and bits(M) == bits(M0) and bits(r) == bits(r0)
        assert np.array_equal(bits(AB.score(AO.dot(q, Kj, V), mz, scale)), bits((f32(scale) * AO.dot(q, Kj, V)).astype(f32)))
        dq, delta, db = AB.backward_q_row(q, Kj, Vj, mz, o, do, M, r, scale, V)
        dq0, delta0 = AO.backward_q_row(q, Kj, Vj, o0, do, M0, r0, scale, V)
        assert np.array_equal(bits(dq), bits(dq0)) and bits(delta) == bits(delta0)
        assert np.all(np.isfinite(db))
        dk, dv = AB.backward_kv_row(Kj[0], Vj[0], np.tile(q, (L, 1)), np.tile(do, (L, 1)), mz, np.full(L, M), np.full(L, r),
                                    np.full(L, delta), scale, V)
        dk0, dv0 = AO.backward_kv_row(Kj[0], Vj[0], np.tile(q, (L, 1)), np.tile(do, (L, 1)), np.full(L, M), np.full(L, r),
                                      np.full(L, delta), scale, V)
        assert np.array_equal(bits(dk), bits(dk0)) and np.array_equal(bits(dv), bits(dv0))
        # -Inf on a third of the nonzeros beside a finite maximum: e = +0, p = +0, dBias = +-0, and the row is the row without them
        gone = np.arange(L) % 3 == 1
        b = np.where(gone, -np.inf, rng.standard_normal(L)).astype(f32)
        o, M, r = AB.forward_row(q, Kj, Vj, b, scale, V, T)
        p = AO.probabilities(AB.score(AO.dot(q, Kj, V), b, scale), M, r)
        assert np.all(bits(p[gone]) == 0) and np.isfinite(M) and np.all(np.isfinite(o))
        _, _, db = AB.backward_q_row(q, Kj, Vj, b, o, do, M, r, scale, V)
        assert np.all(db[gone] == 0) and np.any(db[~gone] != 0)
        o_kept, M_kept, _ = AB.forward_row(q, Kj[~gone], Vj[~gone], b[~gone], scale, V, T)
        assert M == M_kept and np.allclose(o, o_kept, rtol=1e-5, atol=1e-6)
        # a NaN or +Inf bias, or a row whose every t is -Inf, behaves as the same t does without a bias: a NaN row
        for bad in (np.nan, np.inf):
            b2 = b.copy()
            b2[0] = bad
            assert np.all(np.isnan(AB.forward_row(q, Kj, Vj, b2, scale, V, T)[0]))
        assert np.all(np.isnan(AB.forward_row(q, Kj, Vj, np.full(L, -np.inf, f32), scale, V, T)[0]))


# ---- the premises of the bit comparisons on the device -------------------------------------------------------------------------
def test_every_expf_argument_of_the_bias_bit_comparisons_is_zero_or_at_most_minus_128():
    total = 0
    for name, case, k, kv in AB.ORDER_SETS:
        s = OC.pattern(name)
        tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
        per, _, _, bias = AB.order_data(name, case, k, kv)
        assert set(np.unique(bias.view(np.uint32)).tolist()) == set(AB.EXACT_BIASES.view(np.uint32).tolist())
        assert len({b.tobytes() for b in bias}) == AB.HEADS, "the bias differs per query head"
        for h, d in enumerate(per):
            with AO.expf_arguments() as log, AO.without_chains():
                want = AB.emulate(s, tp, ti, d, bias[h], kv_pass=case != "maxima")
            assert log and AO.expf_arguments_are_exact(log), f"{name} {case} k={k} kv={kv} head {h}"
            total += sum(x.size for x in log)
            if "stats" in want:
                M = want["stats"][np.diff(s.rp) > 0, 0]
                assert np.all(np.isfinite(M)), "every row keeps a finite t at its maximum"
            x = np.concatenate(log)
            assert np.any(x == -128) and np.any(np.isneginf(x)) and np.any(x == 0)
    print(f"{total} expf arguments, every one +-0, at most -128 or -Inf")


def _differs(a, b):
    return not np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def test_each_mistake_changes_bits_of_a_compared_array():
    """On the inputs of the GPU test: head 1 of the (P1, stats_k0) and (P2, stats_k0) sets and of the forward set (P1, q0); the
    fused multiply-add on the general data of the GPU test's rounding case.  dBias, stats and p feed no chain, so the chains are
    left out where only those are compared (AO.without_chains)."""
    changed = {}
    name, case, k, kv = AB.ORDER_SETS[2]
    assert (name, case) == ("P1", "stats_k0")
    s = OC.pattern(name)
    per, _, _, bias = AB.order_data(name, case, k, kv)
    d, b = per[1], bias[1]
    with AO.without_chains():
        right = AB.attention_backward_q(s.rp, s.ci, d["Q"], d["K"], d["V"], b, d["O"], d["dO"], d["stats"], d["scale"])[2]
        assert not np.any(np.isnan(right)), "every position of [0, nnz) is written"
        for wrong in ("by_column", "neighbour", "before_scaling", "dbias_scaled", "piece_relative"):
            got = AB.attention_backward_q(s.rp, s.ci, d["Q"], d["K"], d["V"], b, d["O"], d["dO"], d["stats"], d["scale"], wrong)[2]
            changed[wrong] = _differs(got, right)
    # the forward pass sees the first three too (stats of the q0 set)
    name, case, k, kv = AB.ORDER_SETS[0]
    s0 = OC.pattern(name)
    per0, _, _, bias0 = AB.order_data(name, case, k, kv)
    with AO.without_chains():
        right = AB.attention_forward(s0.rp, s0.ci, per0[1]["Q"], per0[1]["K"], per0[1]["V"], bias0[1], per0[1]["scale"])[1]
        for wrong in ("by_column", "neighbour"):
            got = AB.attention_forward(s0.rp, s0.ci, per0[1]["Q"], per0[1]["K"], per0[1]["V"], bias0[1], per0[1]["scale"], wrong)[1]
            changed[wrong] = changed[wrong] and _differs(got, right)
    # bias_t not permuted: dK and dV of the P2 set (short transposed rows)
    name, case, k, kv = AB.ORDER_SETS[4]
    s2 = OC.pattern(name)
    tp, ti = AO.transpose_pattern(s2.rows, s2.cols, s2.rp, s2.ci)
    per2, _, _, bias2 = AB.order_data(name, case, k, kv)
    d = per2[1]
    kv_pass = lambda w: AB.attention_backward_kv(tp, ti, d["Q"], d["K"], d["V"], AB.transposed_bias(s2.ci, bias2[1], w), d["dO"],       # noqa: E731
                                                 d["stats"], d["delta"], d["scale"])
    (dk, dv), (dk_w, dv_w) = kv_pass(None), kv_pass("bias_t_unpermuted")
    changed["bias_t_unpermuted"] = _differs(dk, dk_w) and _differs(dv, dv_w)
    # a fused scale * s + b: stats[:, 0] on general data
    sg, Q, K, bg, scale = AB.general_case()
    t = lambda w: np.array([np.max(AB.score(AO.dot(Q[i], K[sg.ci[sg.rp[i]:sg.rp[i + 1]]], 4), bg[sg.rp[i]:sg.rp[i + 1]], scale, w))      # noqa: E731
                            for i in range(sg.rows) if sg.rp[i + 1] > sg.rp[i]], f32)
    changed["fused"] = _differs(t(None), t("fused"))
    assert set(changed) == set(AB.MISTAKES)
    assert all(changed.values()), f"mistakes that change no bit: {[w for w, c in changed.items() if not c]}"

