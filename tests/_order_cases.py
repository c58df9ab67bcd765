"""The patterns and data sets that tests/test_gpu_order.py runs on the device, tests/test_attention_order_host.py checks on
the host and tests/test_gpu_attention_multigraph.py shares (host only, numpy).

P1 ("multigraph"): about 200 queries on 40 keys, columns drawn with replacement and left unsorted, so keys repeat inside
rows; rows that list one key L times; rows whose leading stretch comes from keys [0, 20) only (the "low" keys of the
rising-maxima data).  Every key is listed more than 512 times, so every row of the transpose goes in pieces, with
repeated queries inside.  P2: about 300 queries on 2600 keys, columns without replacement, then _exact.shuffled (unsorted,
about 1/8 duplicates); its transposed rows are short.

Fused-attention data keeps every expf argument in {+-0, <= -128, -Inf} (tests/_attention_order.py says why):
  q0       Q = 0; K, V, dO random.  Every score is +0, every e is 1.
  k0       K = 0; Q, V, dO random.
  maxima   Q = e_0, K[:, 0] = -256 for the low keys and 0 for the others, scale 0.5: t is -128 or 0.  A step or a whole
           piece of low keys before a high one arrives makes the forward pass rescale with alpha = 0 and the combine weigh a
           piece with w_p = 0.
  stats_q0, stats_k0   Q = 0 or K = 0 and caller-made stats = (0, r_i), O and delta: p = r_i exactly, a different number at
           every nonzero of a transposed row, so the backward chains multiply general numbers.
"""
import functools

import numpy as np

import _exact as E

f32 = np.float32
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 16, 17, 33, 63, 64, 65, 100, 511, 512, 513, 700, 1025, 1537)
ONE_KEY = (1, 8, 512, 513)                       # rows that list one key L times
LOW_FIRST = ((9, 8), (17, 16), (33, 24), (65, 40), (513, 512), (700, 600), (1025, 1024), (1537, 520))   # (length, low prefix)
P1_KEYS, P1_LOW = 40, 20
GEOMETRIES = ((4, 4), (16, 12), (8, 40), (64, 20), (6, 10))
CASES = ("q0", "k0", "maxima", "stats_q0", "stats_k0")
SCALE = {"q0": 0.3, "k0": 0.3, "maxima": 0.5, "stats_q0": 0.3, "stats_k0": -0.7}


@functools.lru_cache(maxsize=None)
def p1():
    rng = np.random.Generator(np.random.PCG64(20240))
    rows = [rng.integers(0, P1_KEYS, size=n) for n in LENGTHS]
    rows += [np.full(n, 3 + 7 * i) for i, n in enumerate(ONE_KEY)]
    for n, low in LOW_FIRST:
        rows.append(np.concatenate([rng.integers(0, P1_LOW, size=low), rng.integers(0, P1_KEYS, size=n - low)]))
        rows.append(np.concatenate([rng.integers(P1_LOW, P1_KEYS, size=low), rng.integers(0, P1_LOW, size=n - low)]))
    rows += [np.zeros(0, np.int64)] * 3
    while len(rows) < 200:
        rows.append(rng.integers(0, P1_KEYS, size=int(rng.integers(20, 140))))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    s = E.Structure(len(rows), P1_KEYS, rp, np.concatenate(rows))
    assert np.bincount(s.ci, minlength=P1_KEYS).min() > 512, "every transposed row must go in pieces"
    assert set(LENGTHS) <= set(np.diff(s.rp).tolist())
    return s


@functools.lru_cache(maxsize=None)
def p2():
    rng = np.random.Generator(np.random.PCG64(20241))
    lengths = [n for n in LENGTHS if n <= 1025]
    while len(lengths) < 300:
        lengths.append(int(rng.integers(0, 12)))
    lengths = np.array(lengths)[rng.permutation(len(lengths))]
    rp = np.concatenate([[0], np.cumsum(lengths)])
    ci = np.concatenate([np.sort(rng.choice(2600, size=int(n), replace=False)) for n in lengths if n])
    s, _ = E.shuffled(E.Structure(len(lengths), 2600, rp, ci), "order_p2")
    assert np.bincount(s.ci, minlength=2600).max() <= 512
    return s


def pattern(name):
    return {"P1": p1, "P2": p2}[name]()


def randn(seed, *shapes):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.standard_normal(s).astype(f32) for s in shapes]


def _seed(*parts):
    return [sum(map(ord, p)) if isinstance(p, str) else int(p) for p in parts]


def spmm_data(name, k):
    s = pattern(name)
    vals, X = randn(_seed("spmm", name, k), (s.nnz,), (s.cols, k))
    return s, vals, X


def sddmm_data(name, k):
    s = pattern(name)
    U, X = randn(_seed("sddmm", name, k), (s.rows, k), (s.cols, k))
    return s, U, X


def softmax_data(name):
    s = pattern(name)
    P, dP = randn(_seed("softmax", name), (s.nnz,), (s.nnz,))
    return s, P, dP


def neg_zero_key():
    """P2 with minus_zero: every gradient of this key (the one most queries list) is -0 in every head (see attention_data)."""
    return int(np.argmax(np.bincount(p2().ci, minlength=2600)))


def attention_data(name, case, k, kv, head=0, minus_zero=False):
    """dict(Q, K, V, dO, scale) and, for the stats_* cases, the caller-made O, stats and delta.
    minus_zero (stats_k0 on P2): the queries that list neg_zero_key() get r = 2^-100, dO = -2^-100, Q = 2^-100 and delta = 1000 with the
    sign of the scale,
    so p dO and ds Q underflow to -0 at every nonzero of that key: its dK and dV are -0, which a sum started from +0 loses."""
    s = pattern(name)
    Q, K, V, dO, O = randn(_seed(name, case, k, kv, head), (s.rows, k), (s.cols, k), (s.cols, kv), (s.rows, kv), (s.rows, kv))
    d = dict(Q=Q, K=K, V=V, dO=dO, scale=SCALE[case])
    if case in ("q0", "stats_q0"):
        Q[:] = 0
    elif case in ("k0", "stats_k0"):
        K[:] = 0
    elif case == "maxima":
        assert name == "P1"
        Q[:] = 0
        Q[:, 0] = 1
        K[:, 0] = np.where(np.arange(s.cols) < P1_LOW, -256.0, 0.0)
    if case.startswith("stats"):
        rng = np.random.Generator(np.random.PCG64(_seed("stats", name, case, k, kv, head)))
        r = rng.uniform(0.25, 2.0, size=s.rows).astype(f32)
        d["stats"] = np.stack([np.zeros(s.rows, f32), r], axis=1)
        d["delta"] = rng.standard_normal(s.rows).astype(f32)
        d["O"] = O
        if minus_zero:
            assert case == "stats_k0" and name == "P2"
            i = np.unique(s.row_of[s.ci == neg_zero_key()])
            assert i.size >= 2
            tiny = f32(2.0 ** -100)
            d["stats"][i, 1], d["dO"][i], d["Q"][i], d["delta"][i] = tiny, -tiny, tiny, np.copysign(1000.0, SCALE[case])
    return d
