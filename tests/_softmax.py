"""What the row-softmax tests share (host only, numpy): the recipe their expectation comes from, the parity bound of the
documented order of the sums, and an emulation of that order in fp32.

The order (include/spmv_hip.h "Row softmax"): a piece is a whole row of at most 512 entries or entries [512 j, 512 j + 512)
of a longer row; lane l of 64 adds the piece's terms l, l + 64, ... ascending from +0, the 64 partials are combined with the
xor butterfly m = 32 .. 1, and the pieces' sums are added in piece order from +0.
"""
import numpy as np

PIECE, LANES = 512, 64
SCALES = (1.0, 0.125, -2.0)
EPS = 2.0 ** -24


def chain(L):
    """A(L): the longest chain of fp32 additions the documented order has for a row of L entries."""
    L = np.asarray(L, np.int64)
    return -(-np.minimum(L, PIECE) // LANES) + 6 + np.where(L > PIECE, -(-L // PIECE), 0)


def _segments(rp):
    rp = np.asarray(rp, np.int64)
    lengths = np.diff(rp)
    full = np.flatnonzero(lengths > 0)
    return rp, lengths, full, np.repeat(np.arange(full.size), lengths[full])


def scaled(scores, scale):
    """t = scale * scores with one fp32 rounding."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.float32(scale) * np.asarray(scores, np.float32)).astype(np.float32)


def recipe(rp, scores, scale):
    """(ref, D, L) per entry: the softmax of every row with t in fp32 and everything else in fp64; D = max t - min t of the
    entry's row and L its length."""
    rp, lengths, full, seg = _segments(rp)
    t = scaled(scores, scale).astype(np.float64)
    if t.size == 0:
        return t, t, np.zeros(0, np.int64)
    starts = rp[full]
    with np.errstate(over="ignore", invalid="ignore"):
        M = np.fmax.reduceat(t, starts)
        m = np.fmin.reduceat(t, starts)
        e = np.exp(t - M[seg])
        S = np.add.reduceat(e, starts)
        return e / S[seg], (M - m)[seg], lengths[full][seg]


def parity_bound(ref, D, L):
    """|out - ref| <= (2 D + 12 + A(L)) 2^-24 ref: the subtraction puts D 2^-24 into the exponent and expf gets 2 ulp, in
    the numerator and in the denominator; the sum of positive terms adds A 2^-24, the reciprocal and the product one each."""
    return (2.0 * D + 12.0 + chain(L)) * EPS * ref


def backward_recipe(rp, P, dP, scale):
    """(ref, mag) per entry in fp64: dS = scale P (dP - dot) and |scale| |P| (|dP| + sum over the row of |P dP|)."""
    rp, lengths, full, seg = _segments(rp)
    P, dP = np.asarray(P, np.float64), np.asarray(dP, np.float64)
    if P.size == 0:
        return P, P
    starts = rp[full]
    dot = np.add.reduceat(P * dP, starts)
    mag = np.add.reduceat(np.abs(P * dP), starts)
    return scale * P * (dP - dot[seg]), abs(scale) * np.abs(P) * (np.abs(dP) + mag[seg])


def backward_bound(mag, L):
    return (chain(L) + 4.0) * EPS * mag + 1e-37


def clipped_scores(rng, n, scale):
    """Normal scores of spread 4 / |scale|, clipped so that D = max t - min t <= 32 in every row."""
    lim = np.float32(15.9 / abs(scale))
    return np.clip(rng.standard_normal(n).astype(np.float32) * np.float32(4.0 / abs(scale)), -lim, lim)


# ---- the documented order in fp32 ------------------------------------------------------------------------------------
def ordered_sum(x):
    """The sum of the fp32 terms x of one row in the documented order."""
    x = np.asarray(x, np.float32)
    pieces = -(-x.size // PIECE)
    pad = np.zeros(pieces * PIECE, np.float32)
    pad[:x.size] = x
    pad = pad.reshape(pieces, PIECE // LANES, LANES)
    q = np.zeros((pieces, LANES), np.float32)
    for j in range(PIECE // LANES):
        q = q + pad[:, j]
    lane = np.arange(LANES)
    m = LANES // 2
    while m:
        q = q + q[:, lane ^ m]
        m //= 2
    acc = np.float32(0.0)
    if pieces == 1:
        return q[0, 0]
    for s in q[:, 0]:
        acc = np.float32(acc + s)
    return acc


def emulate_row(scores, scale):
    """One row's softmax in the documented fp32 order, with a correctly rounded exp."""
    t = scaled(scores, scale)
    M = np.max(t)
    e = np.exp((t - M).astype(np.float32).astype(np.float64)).astype(np.float32)
    r = np.float32(1.0) / ordered_sum(e)
    return (e * r).astype(np.float32)
