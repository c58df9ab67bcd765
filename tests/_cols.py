"""The documented order of spmv_csr_spmm_cols and spmv_csr_sddmm_cols (include/spmv_hip.h "SpMM and SDDMM at any k"), in numpy
(host only), on top of tests/_attention_order.py, which states the order of the narrow calls.

Column tile t of a call at width k is the columns [64t, 64t + k_t), k_t = min(64, k - 64t).
  SpMM    every tile is _attention_order.spmm on that column block: a column's bits are the narrow call's.
  SDDMM   r_t = _attention_order.sddmm on U[:, tile t], X[:, tile t] (lane partials by fma from +0, then the xor butterfly, at
          width k_t), and out = (..((r_0 + r_1) + r_2) .. + r_(m-1)): fp32 additions in tile order from r_0's value.

sddmm(wrong=...) are the mistakes a tiled kernel invites; tests/test_cols_host.py shows that each changes bits on the data of
tests/test_gpu_cols.py:
  "reversed"        the tiles folded last to first (the same sum with two tiles: fp32 addition is commutative)
  "from_zero"       the fold started from +0: a result whose every tile is -0 becomes +0
  "carried"         a lane's partial carried from one tile into the next (one fma chain over all the lane's columns, 64 apart),
                    one butterfly at the end
  "butterfly_128"   tiles of 128 columns, each reduced by one butterfly over 32 lanes, folded in order
"""
import functools

import numpy as np

import _attention_order as AO
import _exact as E
import _order_cases as OC

TILE = 64
WRONG = ("reversed", "from_zero", "carried", "butterfly_128")
f32 = np.float32


def tiles(k, width=TILE):
    return [(c, min(c + width, k)) for c in range(0, k, width)]


def spmm(rp, ci, vals, X, only=None):
    return np.concatenate([AO.spmm(rp, ci, vals, X[:, a:b], only=only) for a, b in tiles(X.shape[1])], axis=1)


def fold(parts, wrong=None):
    """The tiles' results added in fp32 in tile order, from tile 0's value."""
    if wrong == "reversed":
        parts = parts[::-1]
    with np.errstate(invalid="ignore", over="ignore"):
        if wrong == "from_zero":
            acc = np.zeros_like(parts[0])
            for x in parts:
                acc = (acc + x).astype(f32)
            return acc
        acc = np.array(parts[0], f32)
        for x in parts[1:]:
            acc = (acc + x).astype(f32)
        return acc


def _carried_dot(u, B):
    """16 lane partials, lane s one fma chain over its columns 4s .. 4s+3 of every tile in turn, then one butterfly."""
    p = np.zeros((B.shape[0], TILE // 4), f32)
    for c in range(len(u)):
        s = (c % TILE) // 4
        p[:, s] = AO.fma(u[c], B[:, c], p[:, s])
    lane, m = np.arange(TILE // 4), TILE // 8
    with np.errstate(invalid="ignore"):
        while m:
            p = p + p[:, lane ^ m]
            m //= 2
    return p[:, 0]


def sddmm(rp, ci, U, X, wrong=None):
    assert wrong is None or wrong in WRONG
    k = U.shape[1]
    if wrong == "carried":
        out = np.empty(len(ci), f32)
        for i in range(len(rp) - 1):
            b, e = rp[i], rp[i + 1]
            if e > b:
                out[b:e] = _carried_dot(U[i], np.asarray(X[ci[b:e]], f32))
        return out
    if wrong == "butterfly_128":
        return fold(tile_results(rp, ci, U, X, 2 * TILE))
    return fold(tile_results(rp, ci, U, X), wrong)


def tile_results(rp, ci, U, X, width=TILE):
    """[r_0, .., r_(m-1)]: the narrow call's results per tile (fold adds them)."""
    return [AO.sddmm(rp, ci, U[:, a:b], X[:, a:b]) for a, b in tiles(U.shape[1], width)]


# ---- the patterns and the data the host and the device tests share ------------------------------------------------------------
WIDTHS = (65, 128, 129, 130, 192, 257)
K_MAX = max(WIDTHS)
PATTERNS = ("P1", "P2", "P1T")


@functools.lru_cache(maxsize=None)
def pattern(name):
    """P1 and P2 of tests/_order_cases.py, and "P1T": P1 transposed as spmv_csr_transpose builds it (every row in pieces)."""
    if name != "P1T":
        return OC.pattern(name)
    s = OC.pattern("P1")
    tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
    return E.Structure(s.cols, s.rows, tp, ti)


@functools.lru_cache(maxsize=None)
def data(name):
    """(structure, vals, U, X): random normal fp32, U and X K_MAX columns wide.  A test at width k takes the leading k columns,
    so the full tiles' references are shared among the widths (treat the arrays as read-only)."""
    s = pattern(name)
    vals, U, X = OC.randn([2200, PATTERNS.index(name)], (s.nnz,), (s.rows, K_MAX), (s.cols, K_MAX))
    return s, vals, U, X


@functools.lru_cache(maxsize=None)
def tile_reference(name, a, b):
    s, _, U, X = data(name)
    return AO.sddmm(s.rp, s.ci, U[:, a:b], X[:, a:b])


def sddmm_reference(name, k, wrong=None):
    """sddmm of data(name) at width k in the documented order (the tiles' results cached)."""
    return fold([tile_reference(name, a, b) for a, b in tiles(k)], wrong)


@functools.lru_cache(maxsize=None)
def spmm_reference(name):
    """spmm of data(name) at K_MAX columns: column c is the reference of every call that contains it (batch invariance)."""
    s, vals, _, X = data(name)
    return spmm(s.rp, s.ci, vals, X)


def neg_zero_rows(s, count=6):
    """Rows of the structure s (tests/_exact.Structure) with at least one nonzero, spread over its lengths: the rows whose
    every result is made -0 by minus_zero."""
    full = np.flatnonzero(np.diff(s.rp) > 0)
    return full[np.linspace(0, full.size - 1, count).astype(np.int64)]


def minus_zero(s, U, X):
    """U, X changed in place so that every product of the rows neg_zero_rows(s) underflows to -0 in every column: U = -2^-100
    there and X = 2^-100 in every row those rows list.  Each lane partial is then fma(-2^-100, 2^-100, +-0) = -0, each tile's
    butterfly -0 + -0 = -0 (every tile of a k that is a multiple of 64 is full: all 16 lanes hold -0), and the fold from tile
    0's value gives -0 where the fold from +0 gives +0.  Returns the storage positions of those rows' nonzeros."""
    tiny = f32(2.0 ** -100)
    where = []
    for i in neg_zero_rows(s):
        b, e = s.rp[i], s.rp[i + 1]
        U[i] = -tiny
        X[s.ci[b:e]] = tiny
        where.append(np.arange(b, e))
    return np.concatenate(where)
