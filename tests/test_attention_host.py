"""The fused attention entry points without a device (include/spmv_hip.h "Fused attention"): every new symbol is declared,
exported by the normal and the bounds-checked library and bound in capi, the CsrMatrix methods and the fused holder exist,
and a null handle is refused.  A numpy emulation of the documented fp32 order of the three passes (online steps of T
nonzeros, pieces of 512, the combine) is compared with fp64 dense attention on rows of 1 .. 5000 entries, and reproduces the
exact case of tests/test_gpu_fused_attention.py bit for bit.

The emulation (tests/_attention_order.py) rounds every operation to fp32 where the header says so; its fma is the correctly
rounded one and its expf the correctly rounded exponential, which the device's need not be.  That does not matter to the bounds
below, and the exact case has no rounding at all.

The bound of the comparison, per row of L entries with D = max t - min t <= 32: the subtraction puts D 2^-24 into an exponent
and expf gets 2 ulp, in the numerator and in the denominator; the fp32 scores themselves are left to RTOL (as in
tests/test_gpu_sparse_attention.py).  A sum of n terms taken one after the other carries at most n 2^-24 of the sum of its
terms' magnitudes, and a span has A = min(L, 512) additions, ceil(A / T) rescalings and, in a long row, ceil(L / 512) combine
steps: (2 D + 12 + 2 (A + A / T + pieces)) 2^-24 + RTOL relative to sum p |v| for O.  dQ adds the three roundings of ds, the
sums of dp and delta (at most kv + 4 each) and its own chain: RTOL + (2 D + 2 kv + 24 + 3 (A + A / T + pieces)) 2^-24 relative
to the magnitude the GPU tests use, |scale| sum p (|dp| + sum p |dp|) |K|.

The same emulation then runs the rows that tests/test_gpu_fused_attention.py adds for one lane per row, for scales that
round, for masked stretches in long rows and for extreme score profiles (tests/_attention_rows.py), and is held to RTOL
under the GPU tests' normalisation: the documented order itself meets what those tests demand of the kernels.  Three wrong
orders (forward_row's `wrong`) each fail one of these checks, so the rows tell them apart.
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import _attention_rows as R
from _attention_order import (PIECE, backward_kv_row, backward_q_row, dot, f32, f64, fma, forward_row, geometry,  # noqa: F401
                              probabilities)

ROOT = Path(__file__).resolve().parent.parent
RTOL, EPS = 1e-5, 2.0 ** -24
NAMES = {"spmv_csr_attention_plan": 2, "spmv_csr_attention_plan_bytes": 1, "spmv_csr_attention_forward": 14,
         "spmv_csr_attention_backward_q": 19, "spmv_csr_attention_backward_kv": 19}      # name -> number of arguments


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_attention_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    normal, checked = _exports(capi.LIB_PATH), _exports(capi.CHECKED_LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert name in normal, f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in checked, f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
    for name in ("spmv_csr_attention_forward", "spmv_csr_attention_backward_q", "spmv_csr_attention_backward_kv"):
        assert capi.SIGNATURES[name][1][1] is C.c_float, "scale is a float"
    flat = re.sub(r"\s+", " ", header)
    limits = flat[flat.index("Limits of the layouts"):flat.index("tests/test_gpu_limits.py")]
    assert "spmv_csr_attention_forward" in limits
    for method in ("attention_plan", "attention_plan_bytes", "attention_forward", "attention_backward_q", "attention_backward_kv"):
        assert callable(getattr(capi.CsrMatrix, method, None)), f"CsrMatrix.{method} missing"


def test_fused_sparse_attention_imports(pkg):
    import torch
    sa = pkg.sparse_attention
    assert issubclass(sa.FusedSparseAttentionFunction, torch.autograd.Function) and callable(sa.FusedSparseAttention)
    assert issubclass(sa.SparseAttentionFunction, torch.autograd.Function) and callable(sa.SparseAttention)     # (untouched)


def test_attention_refuses_a_null_handle(pkg):
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p -= p % 16
    assert lib.spmv_csr_attention_plan(None, None) == capi.ERR_INVALID
    assert "spmv_csr_attention_plan:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_attention_plan_bytes(None) == capi.ERR_INVALID
    assert lib.spmv_csr_attention_forward(None, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, None) == capi.ERR_INVALID
    assert "spmv_csr_attention_forward:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_attention_backward_q(None, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, 4, p, p, p, 4, None) == capi.ERR_INVALID
    assert "spmv_csr_attention_backward_q:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_attention_backward_kv(None, 1.0, 4, p, 4, p, 4, 4, p, 4, p, 4, p, p, p, 4, p, 4, None) == capi.ERR_INVALID
    assert "spmv_csr_attention_backward_kv:" in lib.spmv_last_error().decode()


# ---- the documented order in fp32: tests/_attention_order.py (shared with the GPU tests that compare bit for bit) -----------
def test_the_emulated_order_against_fp64_dense_attention():
    worst = [0.0, 0.0]
    for L in (1, 2, 7, 8, 9, 16, 17, 64, 511, 512, 513, 1024, 1025, 4100, 5000):
        for k, kv in ((24, 24), (8, 40), (64, 4), (6, 10)):
            rng = np.random.Generator(np.random.PCG64([L, k, kv]))
            V, T = geometry(k, kv)
            scale = 2.0 ** -2
            q, Kj, Vj, do = (rng.standard_normal(s).astype(f32) for s in ((k,), (L, k), (L, kv), (kv,)))
            o, M, r = forward_row(q, Kj, Vj, scale, V, T)
            dq, delta = backward_q_row(q, Kj, Vj, o, do, M, r, scale, V)
            # fp64
            t = scale * (Kj.astype(f64) @ q.astype(f64))
            D = t.max() - t.min()
            assert D <= 32.0
            p = np.exp(t - t.max())
            p /= p.sum()
            o64 = p @ Vj.astype(f64)
            dp = Vj.astype(f64) @ do.astype(f64)
            dq64 = (scale * p * (dp - p @ dp)) @ Kj.astype(f64)
            A = min(L, PIECE)
            chain = A + -(-A // T) + (-(-L // PIECE) if L > PIECE else 0)
            bound_o = (RTOL + (2 * D + 12 + 2 * chain) * EPS) * (p @ np.abs(Vj).astype(f64))
            mag = (abs(scale) * p * (np.abs(dp) + p @ np.abs(dp))) @ np.abs(Kj).astype(f64)
            bound_q = (RTOL + (2 * D + 2 * kv + 24 + 3 * chain) * EPS) * mag
            ro, rq = np.max(np.abs(o - o64) / bound_o), np.max(np.abs(dq - dq64) / bound_q)
            worst = [max(worst[0], ro), max(worst[1], rq)]
            assert ro <= 1.0, f"L={L} k={k} kv={kv}: O at {ro:.3g} of its bound"
            assert rq <= 1.0, f"L={L} k={k} kv={kv}: dQ at {rq:.3g} of its bound"
            assert M == np.max((f32(scale) * dot(q, Kj, V)).astype(f32))
    print(f"the emulated order reaches {worst[0]:.3g} (O) and {worst[1]:.3g} (dQ) of the bounds")


def test_the_emulation_handles_the_special_rows():
    V, T = geometry(8, 8)
    rng = np.random.Generator(np.random.PCG64(3))
    Kj, Vj = rng.standard_normal((30, 8)).astype(f32), rng.standard_normal((30, 8)).astype(f32)
    q = rng.standard_normal(8).astype(f32)
    q[0] = 1.0
    Km = Kj.copy()
    Km[:20, 0] = -np.inf                     # two whole leading steps of -Inf, then a mixed one
    o, M, r = forward_row(q, Km, Vj, 0.25, V, T)
    # (not the bits of the 10 finite entries run alone: those take steps [8][2], these [4 masked + 4][6])
    p = probabilities((f32(0.25) * dot(q, Km, V)).astype(f32), M, r)
    assert np.isfinite(o).all() and np.all(p[:20] == 0) and np.all(p[20:] > 0) and abs(float(p.sum()) - 1) < 1e-6
    # with the finite entries inside one step the masked ones leave the bits alone
    o4, M4, r4 = forward_row(q, Km[:24], Vj[:24], 0.25, V, T)
    o4b, M4b, r4b = forward_row(q, Kj[20:24], Vj[20:24], 0.25, V, T)
    assert o4.tobytes() == o4b.tobytes() and (M4, r4) == (M4b, r4b)
    Km[:, 0] = -np.inf
    assert np.isnan(forward_row(q, Km, Vj, 0.25, V, T)[0]).all()             # a row masked entirely
    qn = q.copy()
    qn[1] = np.nan
    assert np.isnan(forward_row(qn, Kj, Vj, 0.25, V, T)[0]).all()            # a NaN
    Kp = Kj.copy()
    Kp[25, 0] = np.inf
    assert np.isnan(forward_row(q, Kp, Vj, 0.25, V, T)[0]).all()             # a +Inf
    o0, M0, r0 = forward_row(q, Kj[:0], Vj[:0], 0.25, V, T)
    assert not o0.any() and M0 == -np.inf and r0 == 0 and not np.signbit(r0)  # an empty row


def _exact_case(scale):
    """The pattern and data of the GPU exact test: O, dQ, dK and dV of the emulation equal torch's fp64 dense autograd."""
    import torch
    rows, cols, k = 3000, 2000, 8
    rng = np.random.Generator(np.random.PCG64(5))
    lengths = 2 ** rng.integers(0, 5, size=rows)
    lengths[:5] = (1, 2, 4, 8, 16)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ci = np.concatenate([np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lengths]).astype(np.int64)
    row_of = np.repeat(np.arange(rows), lengths)
    ints = lambda seed, shape: np.random.Generator(np.random.PCG64(seed)).integers(-4, 5, size=shape).astype(f32)   # noqa: E731
    V, T = geometry(k, k)
    order = np.argsort(ci, kind="stable")                 # the transposed pattern's storage order
    tp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=cols))])
    for step, zero in enumerate(("Q", "K")):
        Q, K, Vm, dO = ints(10 + step, (rows, k)), ints(20 + step, (cols, k)), ints(30 + step, (cols, k)), ints(40 + step, (rows, k))
        (Q if zero == "Q" else K)[:] = 0
        O, stats, dQ, delta = np.empty((rows, k), f32), np.empty((rows, 2), f32), np.empty((rows, k), f32), np.empty(rows, f32)
        for i in range(rows):
            j = ci[rp[i]:rp[i + 1]]
            O[i], stats[i, 0], stats[i, 1] = forward_row(Q[i], K[j], Vm[j], scale, V, T)
            dQ[i], delta[i] = backward_q_row(Q[i], K[j], Vm[j], O[i], dO[i], stats[i, 0], stats[i, 1], scale, V)
        dK, dV = np.empty((cols, k), f32), np.empty((cols, k), f32)
        for j in range(cols):
            i = row_of[order[tp[j]:tp[j + 1]]]
            dK[j], dV[j] = backward_kv_row(K[j], Vm[j], Q[i], dO[i], stats[i, 0], stats[i, 1], delta[i], scale, V)
        assert np.array_equal(stats[:, 1], (1.0 / lengths).astype(f32)) and not stats[:, 0].any()
        mask = torch.zeros((rows, cols), dtype=torch.bool)
        mask[torch.from_numpy(row_of), torch.from_numpy(ci)] = True
        q, kk, v = (torch.from_numpy(t.astype(f64)).requires_grad_(True) for t in (Q, K, Vm))
        scores = torch.where(mask, (q @ kk.t()) * scale, torch.tensor(float("-inf"), dtype=torch.float64))
        Od = torch.softmax(scores, dim=1) @ v
        Od.backward(torch.from_numpy(dO.astype(f64)))
        for what, got, want in (("O", O, Od.detach()), ("dQ", dQ, q.grad), ("dK", dK, kk.grad), ("dV", dV, v.grad)):
            want = want.numpy()
            assert np.array_equal(want.astype(f32).astype(f64), want), f"{what}: the expectation is not an fp32 number"
            assert np.array_equal(got + f32(0), want.astype(f32) + f32(0)), f"{zero} = 0: {what} differs"
        assert (dQ if zero == "Q" else dK).any() and dV.any() and not (dK if zero == "Q" else dQ).any()


def test_the_emulation_reproduces_the_exact_case():
    _exact_case(2.0 ** -2)


def test_the_emulation_reproduces_the_exact_case_at_a_scale_that_is_no_power_of_two():
    """scale = -0.375: the scores are 0, p = 2^-m and ds a multiple of 2^-11 below 2^8, so nothing is rounded."""
    _exact_case(-0.375)


# ---- the documented order under the acceptance rule of the GPU tests ---------------------------------------------------
# tests/test_gpu_fused_attention.py accepts an error of max(4 x torch's fp32 dense autograd, RTOL) times the magnitudes of
# its _normalised (O: sum p |V|; dQ: |scale| sum p (|dp| + sum p |dp|) |K|; dK, dV alike), against fp64 at the scale the
# kernel receives, fp32(scale).  The checks below hold the emulation of the documented order to RTOL alone on the rows the
# GPU tests add: if the order itself did not meet RTOL there, no kernel could be blamed.
def _row_errors(q, Kj, Vj, do, scale, k, kv, keep=None, floor=0.0, wrong=None, single_query_keys=False):
    """The emulation on one row against fp64 on the entries `keep` (None: all): the normalised errors of O and dQ (and of
    dK, dV where every key has this one query) and the statistics; inf where a value is not finite or beyond the floor at
    magnitude 0."""
    V, T = geometry(k, kv)
    o, M, r = forward_row(q, Kj, Vj, scale, V, T, wrong)
    dq, delta = backward_q_row(q, Kj, Vj, o, do, M, r, scale, V)
    t32 = (f32(scale) * dot(q, Kj, V)).astype(f32)
    sc = float(f32(scale))
    Kr, Vr = (Kj, Vj) if keep is None else (Kj[keep], Vj[keep])
    K64, V64, q64, do64 = Kr.astype(f64), Vr.astype(f64), q.astype(f64), do.astype(f64)
    t = sc * (K64 @ q64)
    p = np.exp(t - t.max())
    p /= p.sum()
    dp = V64 @ do64
    ds = sc * p * (dp - p @ dp)
    ds_abs = abs(sc) * p * (np.abs(dp) + p @ np.abs(dp))

    def err(got, want, mag):
        with np.errstate(invalid="ignore", divide="ignore"):
            got = np.asarray(got, f64)
            if not np.isfinite(got).all() or np.any(np.abs(got[mag == 0]) > floor):
                return np.inf
            live = mag > 0
            return float(np.max(np.maximum(np.abs(got - want)[live] - floor, 0) / mag[live], initial=0.0))

    out = {"O": err(o, p @ V64, p @ np.abs(V64)), "dQ": err(dq, ds @ K64, ds_abs @ np.abs(K64)), "M": M, "r": r, "t": t32,
           "o": o, "dq": dq}
    if single_query_keys:
        assert keep is None
        with np.errstate(invalid="ignore", over="ignore"):
            p32 = probabilities(t32, M, r)
            ds32 = (f32(scale) * (p32 * (dot(do, Vj, V) - delta).astype(f32)).astype(f32)).astype(f32)
            dK, dV = fma(ds32[:, None], q[None], 0.0), fma(p32[:, None], do[None], 0.0)
        out["dK"] = err(dK, ds[:, None] * q64[None], ds_abs[:, None] * np.abs(q64)[None])
        out["dV"] = err(dV, p[:, None] * do64[None], p[:, None] * np.abs(do64)[None])
    return out


def _randn_row(seed, L, k, kv):
    rng = np.random.Generator(np.random.PCG64(seed))
    return tuple(rng.standard_normal(s).astype(f32) for s in ((k,), (L, k), (L, kv), (kv,)))


LENGTHS = (1, 2, 7, 8, 9, 16, 17, 64, 511, 512, 513, 1025, 4100)


def test_the_emulated_order_meets_rtol_at_one_lane():
    """k, kv <= 4: one lane per row, eight nonzeros per step."""
    worst = {"O": 0.0, "dQ": 0.0}
    for k, kv in ((1, 1), (4, 4), (3, 2), (2, 4)):
        assert geometry(k, kv) == (1, 8)
        for L in LENGTHS:
            e = _row_errors(*_randn_row([L, k, kv], L, k, kv), 2.0 ** -2, k, kv)
            assert e["M"] == e["t"].max()
            for w in worst:
                worst[w] = max(worst[w], e[w])
                assert e[w] <= RTOL, f"L={L} k={k} kv={kv}: {w} at {e[w]:.3g}"
    print(f"one lane: the emulated order's normalised error is at most {worst['O']:.3g} (O) and {worst['dQ']:.3g} (dQ)")


def _scales_worst(wrong=None):
    worst = {"O": 0.0, "dQ": 0.0, "M": True}
    for scale in (0.3, -1.7, 0.0, -0.0):
        for k, kv in ((24, 24), (3, 2)):
            for L in (1, 8, 9, 17, 513, 1025, 4100):
                e = _row_errors(*_randn_row([L, k, kv, 7], L, k, kv), scale, k, kv, wrong=wrong)
                worst["M"] &= bool(e["M"] == e["t"].max())
                for w in ("O", "dQ"):
                    worst[w] = max(worst[w], e[w])
                if scale == 0.0 and wrong is None:
                    assert e["M"] == 0 and not e["dq"].any() and e["r"] == f32(1) / f32(L)
    return worst


def test_the_emulated_order_meets_rtol_at_scales_that_round():
    """0.3 and -1.7 are no powers of two: t = scale * s and ds are rounded; a negative scale turns the row
    maximum into the scaled minimum of s; at +0 and -0 every p is 1 / L and dQ is 0."""
    worst = _scales_worst()
    print(f"scales 0.3, -1.7, 0, -0: the emulated order's normalised error is at most {worst['O']:.3g} (O) and "
          f"{worst['dQ']:.3g} (dQ)")
    assert worst["M"], "M is not the maximum of fp32(scale * s)"
    assert worst["O"] <= RTOL and worst["dQ"] <= RTOL


def _extreme_worst(wrong=None, profiles=R.EXTREME_PROFILES):
    worst = {"O": 0.0, "dQ": 0.0, "dK": 0.0, "dV": 0.0}
    rows, _ = R.extreme_rows()
    for k, kv in ((2, 1), (2, 40)):
        for n, (profile, L, first, t) in enumerate(rows):
            if profile not in profiles:
                continue
            rng = np.random.Generator(np.random.PCG64([n, kv]))
            Kj = np.stack([t / R.EXTREME_SCALE, rng.standard_normal(L)], axis=1).astype(f32)
            Vj, do = rng.standard_normal((L, kv)).astype(f32), rng.standard_normal(kv).astype(f32)
            q = np.array([1, 0], f32)
            e = _row_errors(q, Kj, Vj, do, R.EXTREME_SCALE, k, kv, floor=R.ABS_FLOOR, wrong=wrong, single_query_keys=True)
            if wrong is None:
                assert np.array_equal(e["t"].astype(f64), t), "the scores are not exact"
                assert e["M"] == t.max()
            for w in worst:
                worst[w] = max(worst[w], e[w])
    return worst


def test_the_emulated_order_meets_rtol_on_extreme_score_profiles():
    """Rising and falling maxima, spikes of 200, scores near 256: with the absolute floor of 2^-90 for what underflows."""
    worst = _extreme_worst()
    print("extreme profiles: the emulated order's normalised error is at most "
          + ", ".join(f"{worst[w]:.3g} ({w})" for w in worst))
    assert all(v <= RTOL for v in worst.values()), worst


def _special_case(k, kv, scale, seed):
    """K, V of the 2600 keys of _attention_rows (masked keys: K[j][0] = -Inf) and one query with q[0] = q[1] = 1."""
    rng = np.random.Generator(np.random.PCG64([seed, k, kv]))
    K, Vm = rng.standard_normal((R.KEYS, k)).astype(f32), rng.standard_normal((R.KEYS, kv)).astype(f32)
    K[R.is_masked_key(np.arange(R.KEYS)), 0] = -np.inf
    q, do = rng.standard_normal(k).astype(f32), rng.standard_normal(kv).astype(f32)
    q[:2] = 1.0
    return K, Vm, q, do


def _masked_rows_checks(wrong=None):
    """The rows of _attention_rows with a claim of their own, one of each kind; returns what failed (nothing: [])."""
    failed = []
    kinds, lists = R.special_rows()
    worst = 0.0                                  # of O on the straddling rows (their dQ[0] is NaN by IEEE)
    for k, kv in ((8, 12), (3, 4)):
        V, T = geometry(k, kv)
        for scale in (0.25, 0.3):
            K, Vm, q, do = _special_case(k, kv, scale, 89)
            for kind in R.BIT_KINDS + ("straddle", "all_masked"):
                j = lists[int(np.flatnonzero(kinds == kind)[0])]
                fin = ~R.is_masked_key(j)
                o, M, r = forward_row(q, K[j], Vm[j], scale, V, T, wrong)
                if kind == "all_masked":
                    # by the documented order l = 0 and r = 1.0f / l = +Inf, as for a short row masked entirely
                    o1, M1, r1 = forward_row(q, K[j[:9]], Vm[j[:9]], scale, V, T, wrong)
                    if not (np.isnan(o).all() and M == -np.inf and r == np.inf and (M1, r1) == (M, r)):
                        failed.append(f"{kind} k={k} kv={kv} scale={scale}: stats ({M}, {r})")
                    continue
                if kind == "straddle":
                    e = _row_errors(q, K[j], Vm[j], do, scale, k, kv, keep=fin, wrong=wrong)
                    worst = max(worst, e["O"])
                    if not e["O"] <= RTOL:
                        failed.append(f"{kind} k={k} kv={kv} scale={scale}: O at {e['O']:.3g}")
                    continue
                dq, _ = backward_q_row(q, K[j], Vm[j], o, do, M, r, scale, V)
                o2, M2, r2 = forward_row(q, K[j[fin]], Vm[j[fin]], scale, V, T, wrong)
                dq2, _ = backward_q_row(q, K[j[fin]], Vm[j[fin]], o2, do, M2, r2, scale, V)
                same = ((o + f32(0)).tobytes() == (o2 + f32(0)).tobytes() and (M, r) == (M2, r2) and np.isnan(dq[0])
                        and (dq[1:] + f32(0)).tobytes() == (dq2[1:] + f32(0)).tobytes() and np.isfinite(o).all())
                if not same:
                    failed.append(f"{kind} k={k} kv={kv} scale={scale}: not the bits of the finite entries alone")
    return failed, worst


def test_masked_stretches_of_long_rows_leave_the_bits_alone():
    """A masked piece is (m, l, acc) = (-Inf, 0, 0) with w = expf(-Inf - z) = 0 and adds fma(0, 0, l); a piece that holds all
    the finite entries combines with w = expf(0) = 1: O, M, r and dQ[1:] are those of the finite entries alone."""
    failed, worst = _masked_rows_checks()
    print(f"300 masked + 799 finite: the emulated order's normalised error of O is at most {worst:.3g}")
    assert not failed, failed


def test_the_new_rows_tell_wrong_orders_apart():
    """Each mistake of forward_row's `wrong` fails one of the checks above."""
    worst = _extreme_worst("stale_maximum", ("ascending", "ascending_steep"))
    assert not all(v <= RTOL for v in worst.values()), "a stale maximum passes the ascending rows"
    failed, _ = _masked_rows_checks("combine_keeps_minus_inf")
    assert failed and all("all_masked" in f for f in failed), failed
    assert not _scales_worst("maximum_before_scaling")["M"], "a maximum taken before the scaling passes a negative scale"
