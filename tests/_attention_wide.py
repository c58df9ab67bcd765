"""The wide fused-attention calls (include/spmv_hip.h "Fused attention at head widths up to 128") on the host: the documented
order at V = 32 lanes in steps of T_wide nonzeros, in numpy, on the row functions of tests/_attention_order.py and
tests/_attention_bias.py, which take (V, T) as arguments; only their geometry() and their loops over a pattern assume
T = max(V, 8).  T_wide is read from the header, the one place that states it.

Also here: one row per row length of a pattern (the emulation at width 128 is slow, and a row's result depends on its column
list alone), zero padding, and the butterfly run from the lowest level up, a mistake that only a group of more than two
lanes can make and that "sequential" does not stand for.
"""
import contextlib
import re
from pathlib import Path

import numpy as np

import _attention_bias as AB
import _attention_order as AO

f32 = np.float32
HEADER = Path(__file__).resolve().parent.parent / "include" / "spmv_hip.h"
T_WIDE = int(re.search(r"^#define SPMV_ATTN_WIDE_STEP (\d+)$", HEADER.read_text(), re.M).group(1))
V_WIDE = 32
WIDTHS = ((128, 128), (65, 65), (68, 128), (128, 4), (4, 100), (97, 66))
ORDER_MISTAKES = AO.ORDER_MISTAKES + ("butterfly_low_first",)


def geometry(k, kv):
    """(V, T) of a _wide call: 32 lanes in steps of T_wide above width 64, the other calls' geometry up to it."""
    return (V_WIDE, T_WIDE) if max(k, kv) > 64 else AO.geometry(k, kv)


def dot_low_first(a, B, V, wrong=None):
    """AO.dot with the butterfly's levels run m = 1, 2, .., V / 2: the same pairs at every level, in the wrong order."""
    B = np.asarray(B, f32).reshape(-1, len(a))
    p = np.zeros((B.shape[0], V), f32)
    for c in range(len(a)):
        p[:, c // 4] = AO.fma(a[c], B[:, c], p[:, c // 4])
    lane, m = np.arange(V), 1
    with np.errstate(invalid="ignore"):
        while m < V:
            p = p + p[:, lane ^ m]
            m *= 2
    return p[:, 0]


@contextlib.contextmanager
def _mistake(wrong):
    """The `wrong` the row functions of _attention_order understand; "butterfly_low_first" swaps their dot for the block."""
    if wrong != "butterfly_low_first":
        yield wrong
        return
    keep, AO.dot = AO.dot, dot_low_first
    try:
        yield None
    finally:
        AO.dot = keep


def _rows(n, only):
    return range(n) if only is None else only


def attention_forward(rp, ci, Q, K, Vm, scale, bias=None, wrong=None, only=None):
    """(O, stats) of the queries `only` (all: None) in the documented order of a _wide call; bias: per nonzero, or None."""
    V, T = geometry(Q.shape[1], Vm.shape[1])
    rows = len(rp) - 1
    O, stats = np.zeros((rows, Vm.shape[1]), f32), np.zeros((rows, 2), f32)
    with _mistake(wrong) as w:
        for i in _rows(rows, only):
            b, e = rp[i], rp[i + 1]
            j = ci[b:e]
            if bias is None:
                O[i], stats[i, 0], stats[i, 1] = AO.forward_row(Q[i], K[j], Vm[j], scale, V, T, w)
            else:
                O[i], stats[i, 0], stats[i, 1] = AB.forward_row(Q[i], K[j], Vm[j], bias[b:e], scale, V, T)
    return O, stats


def attention_backward_q(rp, ci, Q, K, Vm, O, dO, stats, scale, bias=None, wrong=None, only=None):
    """(dQ, delta, dBias) of the queries `only`; dBias is NaN where no row was computed, and None without a bias."""
    V, _ = geometry(Q.shape[1], Vm.shape[1])
    rows = len(rp) - 1
    dQ, delta = np.zeros((rows, Q.shape[1]), f32), np.zeros(rows, f32)
    dB = None if bias is None else np.full(len(ci), np.nan, f32)
    with _mistake(wrong) as w:
        for i in _rows(rows, only):
            b, e = rp[i], rp[i + 1]
            j = ci[b:e]
            if bias is None:
                dQ[i], delta[i] = AO.backward_q_row(Q[i], K[j], Vm[j], O[i], dO[i], stats[i, 0], stats[i, 1], scale, V, w)
            else:
                dQ[i], delta[i], dB[b:e] = AB.backward_q_row(Q[i], K[j], Vm[j], bias[b:e], O[i], dO[i], stats[i, 0], stats[i, 1], scale, V)
    return dQ, delta, dB


def attention_backward_kv(tp, ti, Q, K, Vm, dO, stats, delta, scale, bias_t=None, wrong=None, only=None):
    """(dK, dV) of the keys `only`; (tp, ti) is the transposed pattern, bias_t the bias in its storage order."""
    V, _ = geometry(Q.shape[1], Vm.shape[1])
    cols = len(tp) - 1
    dK, dV = np.zeros((cols, K.shape[1]), f32), np.zeros((cols, Vm.shape[1]), f32)
    with _mistake(wrong) as w:
        for j in _rows(cols, only):
            x, y = tp[j], tp[j + 1]
            i = ti[x:y]
            if bias_t is None:
                dK[j], dV[j] = AO.backward_kv_row(K[j], Vm[j], Q[i], dO[i], stats[i, 0], stats[i, 1], delta[i], scale, V, w)
            else:
                dK[j], dV[j] = AB.backward_kv_row(K[j], Vm[j], Q[i], dO[i], bias_t[x:y], stats[i, 0], stats[i, 1], delta[i], scale, V)
    return dK, dV


def one_row_per_length(rp, extra=()):
    """The first row of every row length of the pattern (and the rows `extra`), ascending: every step and piece boundary
    once."""
    lengths = np.diff(np.asarray(rp, np.int64))
    first = {}
    for i, n in enumerate(lengths.tolist()):
        first.setdefault(n, i)
    return sorted(set(first.values()) | {int(x) for x in extra})


def padded(a, w):
    """a with zero columns up to width w."""
    out = np.zeros((a.shape[0], w), f32)
    out[:, :a.shape[1]] = a
    return out
