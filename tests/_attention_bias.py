"""Fused attention with an additive bias per nonzero (include/spmv_hip.h "Fused attention with an additive bias"), on the
host: the documented order with the bias in numpy, on the primitives of tests/_attention_order.py, the mistakes the bias
invites, a per-nonzero fp64 reference with bias, and the bias data of the bit-for-bit GPU tests.

The score of nonzero n is t = fl(fl(scale * s) + bias[n]); everything after t is _attention_order's, unchanged.  dBias[n] =
fl(p * fl(dp - delta)), and ds = fl(scale * dBias[n]).  The bias is indexed by storage position: bias_t, which the pass on the
transposed pattern reads, is the bias permuted by the stable argsort of col_idx (what spmv_csr_transpose_gather does).
"""
import numpy as np

import _attention_order as AO

f32, f64 = np.float32, np.float64

# each changes bits of a compared array on the inputs of tests/test_gpu_attention_bias.py (tests/test_attention_bias_host.py)
MISTAKES = ("by_column", "neighbour", "before_scaling", "fused", "dbias_scaled", "piece_relative", "bias_t_unpermuted")
EXACT_BIASES = np.array([-0.0, 0.0, -128.0, -256.0, -np.inf], f32)


def score(s, b, scale, wrong=None):
    """t of the scores s with the bias b of their positions."""
    with np.errstate(invalid="ignore", over="ignore"):
        if wrong == "before_scaling":
            return (f32(scale) * (s + b).astype(f32)).astype(f32)
        if wrong == "fused":
            return AO.fma(f32(scale), s, b)
        return ((f32(scale) * s).astype(f32) + b).astype(f32)


def _bias_at(bias, b, e, j, wrong=None):
    if wrong == "by_column":
        return bias[j]
    if wrong == "neighbour":
        return bias[np.minimum(np.arange(b, e) + 1, len(bias) - 1)]
    return bias[b:e]


def forward_row(q, Kj, Vj, bj, scale, V, T, wrong=None):
    """(O row, M, r) of one query with the bias bj of its nonzeros: _attention_order.forward_row on t with the bias."""
    if Kj.shape[0] == 0:
        return np.zeros(Vj.shape[1], f32), f32(-np.inf), f32(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = score(AO.dot(q, Kj, V), bj, scale, wrong)
        parts = [AO.forward_span(t[b:e], Vj[b:e], T) for b, e in AO.spans(len(t))]
        if len(parts) == 1:
            M, l, acc = parts[0]
        else:
            M = np.fmax.reduce(np.array([p[0] for p in parts], f32))
            z = f32(0) if M == -np.inf else M
            l, acc = f32(0), np.zeros(Vj.shape[1], f32)
            for m_p, l_p, acc_p in parts:
                w = AO.expf(m_p - z)
                l, acc = AO.fma(l_p, w, l), AO.fma(acc_p, w, acc)
        r = f32(1) / f32(l)
        return (acc * r).astype(f32), f32(M), f32(r)


def backward_q_row(q, Kj, Vj, bj, o, do, M, r, scale, V, wrong=None):
    """(dQ row, delta, dBias of the row's nonzeros)."""
    if Kj.shape[0] == 0:
        return np.zeros(len(q), f32), f32(0), np.zeros(0, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        delta = AO.dot(do, o[None], V)[0]
        p = AO.probabilities(score(AO.dot(q, Kj, V), bj, scale, wrong), M, r)
        g = (p * (AO.dot(do, Vj, V) - delta).astype(f32)).astype(f32)
        ds = (f32(scale) * g).astype(f32)
    return AO.ordered_fma_sum(ds, Kj), delta, (ds if wrong == "dbias_scaled" else g)


def backward_kv_row(kj, vj, Qi, dOi, bi, Mi, ri, deltai, scale, V, wrong=None):
    """(dK row, dV row) of one key; bi: bias_t of the transposed row's nonzeros."""
    if Qi.shape[0] == 0:
        return np.zeros(len(kj), f32), np.zeros(len(vj), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = AO.probabilities(score(AO.dot(kj, Qi, V), bi, scale, wrong), Mi, ri)
        ds = (f32(scale) * (p * (AO.dot(vj, dOi, V) - deltai).astype(f32)).astype(f32)).astype(f32)
    return AO.ordered_fma_sum(ds, Qi), AO.ordered_fma_sum(p, dOi)


def attention_forward(rp, ci, Q, K, Vm, bias, scale, wrong=None):
    V, T = AO.geometry(Q.shape[1], Vm.shape[1])
    rows = len(rp) - 1
    O, stats = np.zeros((rows, Vm.shape[1]), f32), np.zeros((rows, 2), f32)
    for i in range(rows):
        b, e = rp[i], rp[i + 1]
        j = ci[b:e]
        O[i], stats[i, 0], stats[i, 1] = forward_row(Q[i], K[j], Vm[j], _bias_at(bias, b, e, j, wrong), scale, V, T, wrong)
    return O, stats


def attention_backward_q(rp, ci, Q, K, Vm, bias, O, dO, stats, scale, wrong=None):
    """(dQ, delta, dBias); dBias is NaN where nothing was written (only a mistake leaves such positions)."""
    V, _ = AO.geometry(Q.shape[1], Vm.shape[1])
    rows = len(rp) - 1
    dQ, delta, dB = np.zeros((rows, Q.shape[1]), f32), np.zeros(rows, f32), np.full(len(ci), np.nan, f32)
    for i in range(rows):
        b, e = rp[i], rp[i + 1]
        j = ci[b:e]
        dQ[i], delta[i], g = backward_q_row(Q[i], K[j], Vm[j], _bias_at(bias, b, e, j, wrong), O[i], dO[i], stats[i, 0], stats[i, 1],
                                            scale, V, wrong)
        if wrong == "piece_relative":
            for x, y in AO.spans(e - b):
                dB[b:b + y - x] = g[x:y]
        else:
            dB[b:e] = g
    return dQ, delta, dB


def transposed_bias(ci, bias, wrong=None):
    """bias_t[i] = bias[map[i]]: the map of spmv_csr_transpose is the stable sort of the storage positions by column."""
    if wrong == "bias_t_unpermuted":
        return np.array(bias, f32)
    return np.asarray(bias, f32)[np.argsort(np.asarray(ci, np.int64), kind="stable")]


def attention_backward_kv(tp, ti, Q, K, Vm, bias_t, dO, stats, delta, scale, wrong=None):
    V, _ = AO.geometry(Q.shape[1], Vm.shape[1])
    cols = len(tp) - 1
    dK, dV = np.zeros((cols, K.shape[1]), f32), np.zeros((cols, Vm.shape[1]), f32)
    for j in range(cols):
        x, y = tp[j], tp[j + 1]
        i = ti[x:y]
        dK[j], dV[j] = backward_kv_row(K[j], Vm[j], Q[i], dO[i], bias_t[x:y], stats[i, 0], stats[i, 1], delta[i], scale, V, wrong)
    return dK, dV


def emulate(s, tp, ti, d, bias, wrong=None, kv_pass=True):
    """What the three _bias passes must give on data set d (tests/_order_cases.attention_data) with `bias`: a dict over O,
    stats (not with caller-made stats), dQ, delta, dBias and, with kv_pass, dK and dV."""
    Q, K, V, dO, scale = d["Q"], d["K"], d["V"], d["dO"], d["scale"]
    want = {}
    if "stats" in d:
        O, stats = d["O"], d["stats"]
    else:
        O, stats = attention_forward(s.rp, s.ci, Q, K, V, bias, scale, wrong)
        want["O"], want["stats"] = O, stats
    want["dQ"], want["delta"], want["dBias"] = attention_backward_q(s.rp, s.ci, Q, K, V, bias, O, dO, stats, scale, wrong)
    if kv_pass:
        delta_in = d["delta"] if "stats" in d else want["delta"]
        want["dK"], want["dV"] = attention_backward_kv(tp, ti, Q, K, V, transposed_bias(s.ci, bias, wrong), dO, stats, delta_in,
                                                       scale, wrong)
    return want


def exact_bias(s, seed):
    """A bias per nonzero drawn from EXACT_BIASES whose every non-empty row keeps a +-0: with scores in {+-0, -128} (the data of
    _order_cases) a row's maximum is then finite, every t is a multiple of 128 or -Inf, and so every expf argument is +-0,
    at most -128 or -Inf."""
    rng = np.random.Generator(np.random.PCG64([20250, seed]))
    bias = EXACT_BIASES[rng.integers(0, len(EXACT_BIASES), size=s.nnz)]
    for i in range(s.rows):
        b, e = int(s.rp[i]), int(s.rp[i + 1])
        if e > b:
            bias[b + int(rng.integers(0, e - b))] = f32(0.0) if rng.integers(0, 2) else f32(-0.0)
    return bias


# ---- the per-nonzero reference with bias ------------------------------------------------------------------------------------
def multiset_attention(rp, ci, Q, K, Vm, dO, bias, scale, dtype=f64):
    """_attention_order.multiset_attention with t = scale * s + bias[n], and dBias = p (dp - sum p dp) among the results (its
    magnitude: p (|dp| + sum p |dp|)).  A nonzero whose bias is -Inf has p = 0; a row must keep a finite score."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    rows, cols = len(rp) - 1, K.shape[0]
    Q, K, Vm, dO = (np.asarray(x, f32).astype(dtype) for x in (Q, K, Vm, dO))
    bias = np.asarray(bias, f32).astype(dtype)
    scale = dtype(f32(scale))
    lengths = np.diff(rp)
    row_of = np.repeat(np.arange(rows), lengths)
    full = np.flatnonzero(lengths > 0)
    starts, seg = rp[full], np.repeat(np.arange(full.size), lengths[full])

    def segment_rows(x):
        out = np.zeros((rows, x.shape[1]), dtype)
        out[full] = np.add.reduceat(x, starts, axis=0)
        return out

    def index_add(n, at, x):
        out = np.zeros((n, x.shape[1]), dtype)
        np.add.at(out, at, x)
        return out

    t = scale * np.einsum("nc,nc->n", Q[row_of], K[ci]) + bias
    e = np.exp(t - np.maximum.reduceat(t, starts)[seg])
    p = e / np.add.reduceat(e, starts)[seg]
    dp = np.einsum("nc,nc->n", dO[row_of], Vm[ci])
    dp_abs = np.einsum("nc,nc->n", np.abs(dO[row_of]), np.abs(Vm[ci]))
    g = p * (dp - np.add.reduceat(p * dp, starts)[seg])
    g_abs = p * (dp_abs + np.add.reduceat(p * dp_abs, starts)[seg])
    ds, ds_abs = scale * g, abs(scale) * g_abs
    out = {"O": segment_rows(p[:, None] * Vm[ci]), "dQ": segment_rows(ds[:, None] * K[ci]),
           "dK": index_add(cols, ci, ds[:, None] * Q[row_of]), "dV": index_add(cols, ci, p[:, None] * dO[row_of]), "dBias": g}
    mag = {"O": segment_rows(p[:, None] * np.abs(Vm[ci])), "dQ": segment_rows(ds_abs[:, None] * np.abs(K[ci])),
           "dK": index_add(cols, ci, ds_abs[:, None] * np.abs(Q[row_of])), "dV": index_add(cols, ci, p[:, None] * np.abs(dO[row_of])),
           "dBias": g_abs}
    return out, mag, t


# ---- the data of the bit-for-bit runs (tests/test_gpu_attention_bias.py; premises: tests/test_attention_bias_host.py) ---------
HEADS, GROUP = 4, 2
# _order_cases.GEOMETRIES give V = 1, 4 and 16 only; (8, 8) and (24, 32) add V = 2 and 8 (as tests/test_gpu_attention16.py does),
# where the biased kernels load the bias at another point of the step than their neighbours
GEOMETRIES = ((4, 4), (16, 12), (8, 40), (64, 20), (6, 10), (8, 8), (24, 32))
# (pattern, case of _order_cases.attention_data, k, kv): V = 1, 2, 4, 8 and 16, both load paths, both patterns; the stats_* cases
# run the backward passes on caller-made stats and delta (p is then a general number)
ORDER_SETS = (("P2", "q0", 6, 10), ("P1", "maxima", 64, 20), ("P1", "stats_k0", 16, 12), ("P1", "stats_q0", 8, 40),
              ("P2", "stats_k0", 4, 4), ("P1", "stats_k0", 8, 8), ("P1", "stats_q0", 24, 32))


def order_data(name, case, k, kv):
    """(per query head data, K per K/V head, V per K/V head, bias (HEADS, nnz), one per query head)."""
    import _order_cases as OC
    s = OC.pattern(name)
    per = [OC.attention_data(name, case, k, kv, head=h) for h in range(HEADS)]
    Ks, Vs = [per[c]["K"] for c in range(HEADS // GROUP)], [per[c]["V"] for c in range(HEADS // GROUP)]
    for h, d in enumerate(per):
        d["K"], d["V"] = Ks[h // GROUP], Vs[h // GROUP]
    bias = np.stack([exact_bias(s, sum(map(ord, name + case)) * 64 + h) for h in range(HEADS)])
    return per, Ks, Vs, bias


def general_case():
    """The general data of the rounding-of-t check: P2, k = 16, standard normal Q, K and bias, scale 0.3."""
    import _order_cases as OC
    s = OC.p2()
    Q, K, b = OC.randn(4242, (s.rows, 16), (s.cols, 16), (s.nnz,))
    return s, Q, K, b, 0.3
