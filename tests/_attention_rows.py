"""Rows that tests/test_gpu_fused_attention.py and tests/test_attention_host.py both run the fused attention passes on
(host only, numpy): the extreme score profiles and the pattern of masked, NaN and +Inf keys in long rows.

Extreme scores.  Q_i = (1, 0) and K[j][0] = t_j / scale with scale = 2^-2 and t a multiple of 0.5 below 2^10, so every
score t_j = scale * (Q_i . K_j) is exact in fp32 and the profile itself costs no accuracy.  Each row owns a range of keys,
so its scores lie in storage order as the profile says.

Special rows.  2600 keys: [0, 1200) masked, [1200, 2000) finite, [2000, 2600) masked (a row's columns are sorted, so masked
stretches lie before and after the finite one).  The kinds of rows are SPECIAL_KINDS below; special_rows() says which keys
each row lists, which rows are NaN rows and which keys those touch.
"""
import numpy as np

# ---- extreme score profiles --------------------------------------------------------------------------------------------
EXTREME_SCALE = 2.0 ** -2
EXTREME_LENGTHS = (1, 2, 7, 8, 9, 16, 17, 511, 512, 513, 1025)
EXTREME_PROFILES = ("ascending", "ascending_steep", "descending", "descending_steep", "spike_last", "spike_first",
                    "alternating", "near_256")
ABS_FLOOR = 2.0 ** -90     # a flushed probability loses at most 2^-126, times |K| <= 2^13, |dp| <= 2^8 and 2^11 entries


def extreme_scores(profile, n, rng):
    """The n scores t of one row in storage order (float64; multiples of 0.5, |t| < 2^10)."""
    i = np.arange(n, dtype=np.float64)
    small = rng.integers(-8, 9, size=n) * 0.5           # [-4, 4]
    if profile == "ascending":
        t = 0.5 * i
    elif profile == "ascending_steep":                  # a step of 8 raises the maximum by 128 or more: a = expf(m - z) = 0
        t = np.minimum(16.0 * i, 1008.0) + 0.5 * (i % 2)
    elif profile == "descending":
        t = (0.5 * i)[::-1].copy()
    elif profile == "descending_steep":
        t = (np.minimum(16.0 * i, 1008.0) + 0.5 * (i % 2))[::-1].copy()
    elif profile == "spike_last":                       # at 513 entries the maximum is the single nonzero of the last piece
        t = small
        t[-1] = 200.0
    elif profile == "spike_first":
        t = small
        t[0] = 200.0
    elif profile == "alternating":
        t = np.where(i % 2 == 0, 0.0, -200.0)
    elif profile == "near_256":                         # a softmax that forgot the maximum overflows here
        t = 256.0 + small
    else:
        raise KeyError(profile)
    assert np.all(t * 2 == np.round(t * 2)) and np.abs(t).max() < 1024
    return t


def extreme_rows(seed=71):
    """[(profile, length, first key, scores)] for every profile and length, and the number of keys; row r owns the keys
    [first, first + length)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, first = [], 0
    for profile in EXTREME_PROFILES:
        for n in EXTREME_LENGTHS:
            rows.append((profile, n, first, extreme_scores(profile, n, rng)))
            first += n
    return rows, first


# ---- masked, NaN and +Inf keys in long rows ----------------------------------------------------------------------------
KEYS, FINITE_LO, FINITE_HI = 2600, 1200, 2000
KEY_MASKED0, KEY_A, KEY_B = 0, 1200, 1201           # the keys that about 700 short rows list: long transposed rows
BAD_LO = 1450                                       # the finite keys of the NaN rows come from [BAD_LO, FINITE_HI)
KEY_INF = 1999                                      # K[KEY_INF][1] = +Inf
SPECIAL_KINDS = {
    "lead512": "512 leading masked + 300 finite: the bits of the 300 finite alone",
    "lead1024": "1024 leading masked + 600 finite: the bits of the 600 finite alone",
    "trail512": "512 finite + 512 trailing masked: the bits of the 512 finite alone",
    "trail300": "300 finite + 512 trailing masked: the bits of the 300 finite alone",
    "straddle": "300 leading masked + the 799 finite keys but KEY_INF: the pieces straddle the boundary",
    "all_masked": "1100 masked entries: a NaN row",
    "nan_long": "a long row with a NaN in Q",
    "inf_short": "a short row that lists the +Inf key",
    "inf_long": "a long row that lists the +Inf key",
    "shared": "a short row that lists keys 0 (masked), 1200 and 1201 and a few finite keys",
    "shared_nan": "the one short row with a NaN in Q: it lists key 1201 but neither key 0 nor key 1200",
    "ordinary": "3 masked + 5 finite entries",
    "empty": "no entry",
}
BIT_KINDS = ("lead512", "lead1024", "trail512", "trail300")       # rows with a bit-level claim against their finite twin
NAN_KINDS = ("all_masked", "nan_long", "inf_short", "inf_long", "shared_nan")
Q_NAN_KINDS = ("nan_long", "shared_nan")                          # Q[row][2] = NaN


def is_masked_key(j):
    j = np.asarray(j)
    return (j < FINITE_LO) | (j >= FINITE_HI)


def special_rows(seed=83, shared=700, ordinary=200):
    """(kinds, lists): the kind of every row and its sorted keys.  The NaN rows avoid keys 0 and 1200 and take their finite
    keys from [BAD_LO, FINITE_HI), so most finite keys stay comparable; only the inf_* rows list KEY_INF."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lead = np.arange(1, FINITE_LO)                                                  # masked keys before the finite ones, not 0
    trail = np.arange(FINITE_HI, KEYS)
    finite = np.setdiff1d(np.arange(FINITE_LO, FINITE_HI), [KEY_A, KEY_B, KEY_INF])  # 797 keys
    bad_finite = finite[finite >= BAD_LO]                                           # 549 keys
    pick = lambda pool, n: np.sort(rng.choice(pool, size=n, replace=False))         # noqa: E731
    cat = lambda *parts: np.sort(np.concatenate(parts)).astype(np.int64)            # noqa: E731
    rows = []
    for _ in range(3):
        rows.append(("lead512", cat(pick(lead, 512), pick(finite, 300))))
        rows.append(("lead1024", cat(pick(lead, 1024), pick(finite, 600))))
        rows.append(("trail512", cat(pick(finite, 512), pick(trail, 512))))
        rows.append(("trail300", cat(pick(finite, 300), pick(trail, 512))))
        rows.append(("straddle", cat(pick(lead, 300), finite, [KEY_A, KEY_B])))      # every finite key but KEY_INF: 799
    for _ in range(2):
        rows.append(("all_masked", cat(pick(np.concatenate([lead, trail]), 1100))))
        rows.append(("nan_long", cat(pick(bad_finite, 530))))
        rows.append(("inf_short", cat(pick(bad_finite, 6), [KEY_INF])))
        rows.append(("inf_long", cat(pick(bad_finite, 530), [KEY_INF])))
    for n in range(shared):
        if n == shared // 2:
            rows.append(("shared_nan", cat([KEY_B], pick(bad_finite, 4))))
        else:
            rows.append(("shared", cat([KEY_MASKED0, KEY_A, KEY_B], pick(finite, int(rng.integers(1, 5))))))
    for _ in range(ordinary):
        rows.append(("ordinary", cat(pick(lead, 2), pick(finite, 5), pick(trail, 1))))
    for _ in range(12):
        rows.append(("empty", np.zeros(0, np.int64)))
    rows = [rows[i] for i in rng.permutation(len(rows))]       # the long rows lie scattered among the short ones
    kinds = np.array([k for k, _ in rows])
    lists = [l for _, l in rows]
    for kind, l in rows:
        assert len(np.unique(l)) == len(l)
        if kind in NAN_KINDS:
            assert KEY_MASKED0 not in l and KEY_A not in l
        if kind not in ("inf_short", "inf_long"):
            assert KEY_INF not in l
    assert set(kinds) == set(SPECIAL_KINDS)
    return kinds, lists
