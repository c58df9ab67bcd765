"""The documented order of the sums of the lane-group family, in numpy (host only): what include/spmv_hip.h promises for
SpMM, SDDMM, the row softmax's backward pass and the fused attention passes with their _heads and _gqa forms, stated one
rounding at a time, and a per-nonzero reference of attention for arbitrary column lists.  tests/test_attention_host.py holds
the emulation to fp64; tests/test_gpu_order.py holds the kernels to the emulation bit for bit.

Every operation is rounded to fp32 where the header says so.  fma(a, b, c) is the correctly rounded one (below); expf is the
correctly rounded exponential, which the device library's is not (1 ulp): bit comparisons therefore use data whose every
expf argument is +-0, at most -128 or -Inf, where any 1-ulp expf returns exactly 1 or 0 (expf_arguments records them).

The per-nonzero reference (multiset_attention) works on the stored nonzeros and segment sums over row_ptr, never through a
dense mask: a key that a row lists twice counts twice in the softmax, is gathered twice into O and appears twice in the
transposed row.
"""
import contextlib
from fractions import Fraction

import numpy as np

PIECE = 512
f32, f64 = np.float32, np.float64


def geometry(k, kv):
    """(V, T): lanes per row and nonzeros per step."""
    slices, V = (max(k, kv) + 3) // 4, 1
    while V < slices:
        V *= 2
    return V, max(V, 8)


# ---- fma ---------------------------------------------------------------------------------------------------------------
def fma_twice_rounded(a, b, c):
    """fp32(fp64(a) * fp64(b) + c): the product is exact in fp64, the sum is rounded to fp64 and then to fp32.  Wrong by one
    ulp where the fp64 sum lands exactly on the midpoint of two fp32 numbers although the exact sum does not."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _round_exactly(a, b, c, near):
    """The fp32 number nearest to a * b + c in exact arithmetic (ties to even), among `near` and its two neighbours."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    best = None
    for cand in (np.nextafter(near, f32(-np.inf)), near, np.nextafter(near, f32(np.inf))):
        if not np.isfinite(cand):
            continue
        d = abs(Fraction(float(cand)) - exact)
        even = int(np.asarray(cand, f32).view(np.uint32)) & 1 == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, cand, even)
    return best[1]


def fma(a, b, c):
    """The correctly rounded fp32 fma.  fp64(a * b) is exact; where the fp64 sum is not an fp32 midpoint (its low 29 mantissa
    bits are not 1000...0) the second rounding cannot cross a midpoint and fp32(fp64 sum) is right.  On a midpoint, and in
    fp32's subnormal range where the midpoints lie elsewhere, exact arithmetic decides."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)
        out = r.astype(f32)
    flat = np.ascontiguousarray(r).reshape(-1)
    tie = ((flat.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | ((np.abs(flat) < 2.0 ** -125) & (flat != 0))
    tie &= np.isfinite(flat)
    if tie.any():
        A, B, Cc = (np.broadcast_to(np.asarray(x, f64), r.shape).reshape(-1) for x in (a, b, c))
        fixed = out.reshape(-1).copy()
        for n in np.flatnonzero(tie):
            if np.isfinite(fixed[n]):
                fixed[n] = _round_exactly(A[n], B[n], Cc[n], fixed[n])
        out = fixed.reshape(r.shape)
    return out if out.ndim else f32(out)


def expf(x):
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(x, f32)
        for log in _EXPF_LOGS:
            log.append(np.array(x, f32).reshape(-1))
        return np.exp(x.astype(f64)).astype(f32)


_EXPF_LOGS = []


@contextlib.contextmanager
def expf_arguments():
    """Collects every argument the emulation hands to expf inside the block: a list of fp32 arrays."""
    log = []
    _EXPF_LOGS.append(log)
    try:
        yield log
    finally:
        _EXPF_LOGS.remove(log)


def expf_arguments_are_exact(log):
    """Every recorded argument is +-0, at most -128 or -Inf: any expf of 1 ulp returns exactly 1 or exactly 0 there."""
    x = np.concatenate(log) if log else np.zeros(0, f32)
    return bool(np.all((x == 0) | (x <= -128)))


def dot(a, B, V, wrong=None):
    """a . B[n] for every row n of B in the documented order: lane partials by fma from +0, then the xor butterfly.
    wrong: "unfused" rounds every product before it is added; "sequential" adds the lane partials one after the other."""
    B = np.asarray(B, f32).reshape(-1, len(a))
    p = np.zeros((B.shape[0], V), f32)
    for c in range(len(a)):
        if wrong == "unfused":
            p[:, c // 4] = p[:, c // 4] + (f32(a[c]) * B[:, c]).astype(f32)
        else:
            p[:, c // 4] = fma(a[c], B[:, c], p[:, c // 4])
    if wrong == "sequential":
        acc = p[:, 0].copy()
        for s in range(1, V):
            acc = acc + p[:, s]
        return acc
    lane, m = np.arange(V), V // 2
    with np.errstate(invalid="ignore"):
        while m:
            p = p + p[:, lane ^ m]
            m //= 2
    return p[:, 0]


def spans(n):
    return [(0, n)] if n <= PIECE else [(b, min(b + PIECE, n)) for b in range(0, n, PIECE)]


WRONG = ("stale_maximum", "combine_keeps_minus_inf", "maximum_before_scaling")      # see forward_row
# mistakes of the order alone (the values stay right to fp32 precision): tests/test_attention_order_host.py shows that each
# changes bits on the inputs of tests/test_gpu_order.py
ORDER_MISTAKES = ("reversed", "pieces_last_to_first", "sequential", "unfused")


_SKIP_CHAINS = []


@contextlib.contextmanager
def without_chains():
    """Inside the block the sums over a row's nonzeros (acc, dQ, dK, dV) are left out: they feed no expf, so the arguments
    that expf_arguments records are the full emulation's, at a fraction of its time.  The outputs are then meaningless."""
    _SKIP_CHAINS.append(True)
    try:
        yield
    finally:
        _SKIP_CHAINS.pop()


def _chain(w, X, wrong=None):
    """acc = fma(w[n], X[n], acc) over the rows of X in storage order from +0."""
    acc = np.zeros(X.shape[1], f32)
    if _SKIP_CHAINS:
        return acc
    order = range(len(w) - 1, -1, -1) if wrong == "reversed" else range(len(w))
    for n in order:
        acc = (acc + (f32(w[n]) * X[n]).astype(f32)).astype(f32) if wrong == "unfused" else fma(w[n], X[n], acc)
    return acc


def forward_span(t, Vj, T, wrong=None, s=None, scale=None):
    m, l, acc = f32(-np.inf), f32(0), np.zeros(Vj.shape[1], f32)
    if wrong == "reversed":
        t, Vj = t[::-1], Vj[::-1]
    with np.errstate(invalid="ignore", over="ignore"):
        for kb in range(0, len(t), T):
            tt = t[kb:kb + T]
            mn = np.fmax(m, np.fmax.reduce(tt))
            if wrong == "maximum_before_scaling":
                mn = np.fmax(m, f32(f32(scale) * np.fmax.reduce(s[kb:kb + T])))
            z = f32(0) if mn == -np.inf else mn
            if wrong == "stale_maximum" and m != -np.inf:
                z = m
            a, e = expf(m - z), expf(tt - z)
            l, acc = f32(l * a), (acc * a).astype(f32)
            for i in range(len(tt)):
                l = f32(l + e[i])
                if _SKIP_CHAINS:
                    continue
                if wrong == "unfused":
                    acc = (acc + (e[i] * Vj[kb + i]).astype(f32)).astype(f32)
                else:
                    acc = fma(e[i], Vj[kb + i], acc)
            m = mn
    return m, l, acc


def forward_row(q, Kj, Vj, scale, V, T, wrong=None):
    """(O row, M, r) of one query whose keys are the rows of Kj, Vj in storage order.  wrong: None is the documented order;
    the others are mistakes an online softmax invites, kept to show that the rows of the tests tell them apart:
    "stale_maximum" takes a step's exponentials against the maximum before the step, "combine_keeps_minus_inf" leaves out
    the combine's z = 0 for M = -Inf, "maximum_before_scaling" takes the maximum over s and scales it afterwards; and the
    ORDER_MISTAKES, which keep the values and change the order."""
    assert wrong is None or wrong in WRONG or wrong in ORDER_MISTAKES
    n = Kj.shape[0]
    if n == 0:
        return np.zeros(Vj.shape[1], f32), f32(-np.inf), f32(0)
    dot_wrong = wrong if wrong in ("sequential", "unfused") else None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = dot(q, Kj, V, dot_wrong)
        t = (f32(scale) * s).astype(f32)
        parts = [forward_span(t[b:e], Vj[b:e], T, wrong, s[b:e], scale) for b, e in spans(n)]
        if len(parts) == 1:
            M, l, acc = parts[0]
        else:
            M = np.fmax.reduce(np.array([p[0] for p in parts], f32))
            z = f32(0) if M == -np.inf and wrong != "combine_keeps_minus_inf" else M
            l, acc = f32(0), np.zeros(Vj.shape[1], f32)
            for m_p, l_p, acc_p in (parts[::-1] if wrong == "pieces_last_to_first" else parts):
                w = expf(m_p - z)
                if wrong == "unfused":
                    l, acc = f32(l + f32(l_p * w)), (acc + (acc_p * w).astype(f32)).astype(f32)
                else:
                    l, acc = fma(l_p, w, l), fma(acc_p, w, acc)
        r = f32(1) / f32(l)
        return (acc * r).astype(f32), f32(M), f32(r)


def probabilities(t, M, r):
    with np.errstate(invalid="ignore", over="ignore"):
        return (expf((t - M).astype(f32)) * r).astype(f32)


def ordered_fma_sum(w, X, wrong=None):
    """sum of w[n] X[n] over the spans of a row: fma in storage order from +0, the spans added in piece order from +0."""
    parts = [_chain(w[b:e], X[b:e], wrong) for b, e in spans(len(w))]
    if len(parts) == 1:
        return parts[0]
    acc = np.zeros(X.shape[1], f32)
    for p in (parts[::-1] if wrong == "pieces_last_to_first" else parts):
        acc = (acc + p).astype(f32)
    return acc


def backward_q_row(q, Kj, Vj, o, do, M, r, scale, V, wrong=None):
    """(dQ row, delta) of one query."""
    if Kj.shape[0] == 0:
        return np.zeros(len(q), f32), f32(0)
    dot_wrong = wrong if wrong in ("sequential", "unfused") else None
    with np.errstate(invalid="ignore", over="ignore"):
        delta = dot(do, o[None], V, dot_wrong)[0]
        p = probabilities((f32(scale) * dot(q, Kj, V, dot_wrong)).astype(f32), M, r)
        ds = (f32(scale) * (p * (dot(do, Vj, V, dot_wrong) - delta).astype(f32)).astype(f32)).astype(f32)
    return ordered_fma_sum(ds, Kj, wrong), delta


def backward_kv_row(kj, vj, Qi, dOi, Mi, ri, deltai, scale, V, wrong=None):
    """(dK row, dV row) of one key whose queries are the rows of Qi, dOi in the transposed pattern's storage order."""
    if Qi.shape[0] == 0:
        return np.zeros(len(kj), f32), np.zeros(len(vj), f32)
    dot_wrong = wrong if wrong in ("sequential", "unfused") else None
    with np.errstate(invalid="ignore", over="ignore"):
        p = probabilities((f32(scale) * dot(kj, Qi, V, dot_wrong)).astype(f32), Mi, ri)
        ds = (f32(scale) * (p * (dot(vj, dOi, V, dot_wrong) - deltai).astype(f32)).astype(f32)).astype(f32)
    return ordered_fma_sum(ds, Qi, wrong), ordered_fma_sum(p, dOi, wrong)


# ---- whole patterns ------------------------------------------------------------------------------------------------------
def transpose_pattern(rows, cols, rp, ci):
    """(row_ptr, col_idx) of the transposed pattern as spmv_csr_transpose builds it: row j lists the nonzeros whose column is
    j in ascending storage position (a stable sort by column), so a key listed twice gives a query listed twice."""
    ci = np.asarray(ci, np.int64)
    order = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    tp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=cols))])
    return tp.astype(np.int64), row_of[order]


def _rows(n, only):
    return range(n) if only is None else only


def attention_forward(rp, ci, Q, K, Vm, scale, wrong=None, only=None):
    """(O, stats) of every query in the documented order (only: the queries to compute; the other rows stay 0)."""
    V, T = geometry(Q.shape[1], Vm.shape[1])
    rows = len(rp) - 1
    O, stats = np.zeros((rows, Vm.shape[1]), f32), np.zeros((rows, 2), f32)
    for i in _rows(rows, only):
        j = ci[rp[i]:rp[i + 1]]
        O[i], stats[i, 0], stats[i, 1] = forward_row(Q[i], K[j], Vm[j], scale, V, T, wrong)
    return O, stats


def attention_backward_q(rp, ci, Q, K, Vm, O, dO, stats, scale, wrong=None, only=None):
    """(dQ, delta) of every query."""
    V, _ = geometry(Q.shape[1], Vm.shape[1])
    rows = len(rp) - 1
    dQ, delta = np.zeros((rows, Q.shape[1]), f32), np.zeros(rows, f32)
    for i in _rows(rows, only):
        j = ci[rp[i]:rp[i + 1]]
        dQ[i], delta[i] = backward_q_row(Q[i], K[j], Vm[j], O[i], dO[i], stats[i, 0], stats[i, 1], scale, V, wrong)
    return dQ, delta


def attention_backward_kv(tp, ti, Q, K, Vm, dO, stats, delta, scale, wrong=None, only=None):
    """(dK, dV) of every key; (tp, ti) is the transposed pattern."""
    V, _ = geometry(Q.shape[1], Vm.shape[1])
    cols = len(tp) - 1
    dK, dV = np.zeros((cols, K.shape[1]), f32), np.zeros((cols, Vm.shape[1]), f32)
    for j in _rows(cols, only):
        i = ti[tp[j]:tp[j + 1]]
        dK[j], dV[j] = backward_kv_row(K[j], Vm[j], Q[i], dO[i], stats[i, 0], stats[i, 1], delta[i], scale, V, wrong)
    return dK, dV


def gqa_fold(per_head, from_zero=False):
    """dK_c = (..((dK^(0) + dK^(1)) + dK^(2)) ..): fp32 additions in head order, starting from head 0's value.
    from_zero is the mistake of starting from +0: it turns a -0 of head 0 into +0."""
    acc = np.zeros_like(per_head[0]) if from_zero else np.array(per_head[0], f32)
    for x in (per_head if from_zero else per_head[1:]):
        acc = (acc + x).astype(f32)
    return acc


def spmm(rp, ci, vals, X, wrong=None, only=None):
    """Y = A X in the documented order: per output column acc = fma(v, x, acc) in storage order from +0; a row of more than
    512 nonzeros per piece of 512, the partial sums added in piece order from +0."""
    rows = len(rp) - 1
    Y = np.zeros((rows, X.shape[1]), f32)
    for i in _rows(rows, only):
        b, e = rp[i], rp[i + 1]
        Y[i] = ordered_fma_sum(vals[b:e], X[ci[b:e]], wrong)
    return Y


def sddmm(rp, ci, U, X, wrong=None):
    """out[n] = U[i] . X[j] in the documented order: four-column lane partials by fma from +0, then the xor butterfly."""
    V, _ = geometry(U.shape[1], 1)
    out = np.empty(len(ci), f32)
    for i in range(len(rp) - 1):
        b, e = rp[i], rp[i + 1]
        if e > b:
            out[b:e] = dot(U[i], X[ci[b:e]], V, wrong)
    return out


def _piece_sum(x, wrong=None):
    """One piece of a row sum (include/spmv_hip.h "Row softmax"): lane l of 64 adds terms l, l + 64, ... from +0, then the
    xor butterfly (_softmax.ordered_sum on at most 512 terms); "sequential" adds the terms one after the other instead."""
    import _softmax as S
    if wrong == "sequential":
        acc = f32(0)
        for v in x:
            acc = f32(acc + v)
        return acc
    return S.ordered_sum(x)


def row_sum(x, wrong=None):
    """The sum of a row's fp32 terms in the documented order: per piece of 512, the pieces added in piece order from +0."""
    x = np.asarray(x, f32)
    if wrong == "reversed":
        x = x[::-1]
    parts = [_piece_sum(x[b:e], wrong) for b, e in spans(len(x))]
    if len(parts) == 1:
        return parts[0]
    acc = f32(0)
    for p in (parts[::-1] if wrong == "pieces_last_to_first" else parts):
        acc = f32(acc + p)
    return acc


def softmax_backward(rp, P, dP, scale, wrong=None):
    """dS[n] = scale * (P[n] * (dP[n] - dot)), three roundings; dot = the row's sum of fp32(P * dP) in the order of row_sum.
    The header has no fma here, so the mistake that corresponds to "unfused" elsewhere is the contracted one: wrong =
    "unfused" stands for P * (dP - dot) computed as fma(P, dP, -fp32(P * dot))."""
    dS = np.full(len(P), np.nan, f32)
    s = f32(scale)
    for i in range(len(rp) - 1):
        b, e = rp[i], rp[i + 1]
        if e == b:
            continue
        p, dp = P[b:e], dP[b:e]
        d = row_sum((p * dp).astype(f32), wrong)
        if wrong == "unfused":
            dS[b:e] = (s * fma(p, dp, -(p * d).astype(f32))).astype(f32)
        else:
            dS[b:e] = (s * (p * (dp - d).astype(f32)).astype(f32)).astype(f32)
    return dS


# ---- the per-nonzero reference -------------------------------------------------------------------------------------------
def multiset_attention(rp, ci, Q, K, Vm, dO, scale, dtype=f64):
    """Attention and its gradients on the stored nonzeros, in `dtype` throughout: scores per nonzero, a segment softmax over
    row_ptr, O and dQ by segment sums, dK and dV by index_add over the nonzeros.  No dense mask: a key listed twice in a row
    is two nonzeros.  Returns (results, magnitudes, t): dicts over O, dQ, dK, dV -- the magnitudes are the sums of the
    absolute values the GPU tests divide errors by (O: sum p |V|; dQ: |scale| sum p (|dp| + sum p |dp|) |K|; dK, dV alike)
    -- and the scaled scores.  Empty rows give zero rows."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    rows, cols = len(rp) - 1, K.shape[0]
    Q, K, Vm, dO = (np.asarray(x, f32).astype(dtype) for x in (Q, K, Vm, dO))
    scale = dtype(f32(scale))                                   # what the kernel receives
    lengths = np.diff(rp)
    row_of = np.repeat(np.arange(rows), lengths)
    full = np.flatnonzero(lengths > 0)
    starts, seg = rp[full], np.repeat(np.arange(full.size), lengths[full])
    zero = lambda n, w: np.zeros((n, w), dtype)                 # noqa: E731

    def segment_rows(x):
        out = zero(rows, x.shape[1])
        if len(ci):
            out[full] = np.add.reduceat(x, starts, axis=0)
        return out

    def index_add(n, at, x):
        out = zero(n, x.shape[1])
        np.add.at(out, at, x)
        return out

    t = scale * np.einsum("nc,nc->n", Q[row_of], K[ci])
    if len(ci) == 0:
        z = {"O": zero(rows, Vm.shape[1]), "dQ": zero(rows, Q.shape[1]), "dK": zero(cols, Q.shape[1]), "dV": zero(cols, Vm.shape[1])}
        return z, {w: x.copy() for w, x in z.items()}, t
    e = np.exp(t - np.maximum.reduceat(t, starts)[seg])
    p = e / np.add.reduceat(e, starts)[seg]
    dp = np.einsum("nc,nc->n", dO[row_of], Vm[ci])
    dp_abs = np.einsum("nc,nc->n", np.abs(dO[row_of]), np.abs(Vm[ci]))
    ds = scale * p * (dp - np.add.reduceat(p * dp, starts)[seg])
    ds_abs = abs(scale) * p * (dp_abs + np.add.reduceat(p * dp_abs, starts)[seg])
    out = {"O": segment_rows(p[:, None] * Vm[ci]), "dQ": segment_rows(ds[:, None] * K[ci]),
           "dK": index_add(cols, ci, ds[:, None] * Q[row_of]), "dV": index_add(cols, ci, p[:, None] * dO[row_of])}
    mag = {"O": segment_rows(p[:, None] * np.abs(Vm[ci])), "dQ": segment_rows(ds_abs[:, None] * np.abs(K[ci])),
           "dK": index_add(cols, ci, ds_abs[:, None] * np.abs(Q[row_of])), "dV": index_add(cols, ci, p[:, None] * np.abs(dO[row_of]))}
    return out, mag, t


def score_spread(rp, t):
    """max over the rows of D = max t - min t."""
    rp = np.asarray(rp, np.int64)
    full = np.flatnonzero(np.diff(rp) > 0)
    if full.size == 0:
        return 0.0
    return float(np.max(np.maximum.reduceat(t, rp[full]) - np.minimum.reduceat(t, rp[full])))
