"""The host half of tests/test_gpu_order.py (no device): the premises its bit comparisons rest on.

fma       the emulation's fma is the correctly rounded one: on operands whose fp64 sum lands exactly on an fp32 midpoint,
          above and below the exact sum, the twice-rounded formula is off by one ulp and the new one matches exact arithmetic.
expf      on every data set of the GPU test (tests/_order_cases.py: every case at every geometry, on P1, and the P2 runs) each
          argument the emulation hands to expf is +-0, at most -128 or -Inf, so any expf of 1 ulp returns exactly 1 or 0 and the
          host's correctly rounded expf stands for the device's.
mistakes  a reversed storage order, pieces added last to first, a sequential sum in place of the butterfly, an unfused
          multiply-add and a GQA fold from +0 each change at least one bit of each array the GPU test compares, on these very
          inputs.  A row's outputs are a function of that row alone, so the mistakes are run on a sample of the rows (every
          length and every special row of P1 is in it; 6 of the 40 keys): a bit that changes in the sample changes in the
          array.  EXEMPT lists the pairings that cannot change by construction, with the reason, and the test asserts that they
          indeed do not: the list claims no more than is true.
multiset  the per-nonzero reference equals dense masked attention where no key repeats, and counts a repeated key twice.
"""
from fractions import Fraction

import numpy as np

import _attention_order as AO
import _order_cases as OC

f32, f64 = np.float32, np.float64


def _exact_fma(a, b, c):
    """a * b + c in exact arithmetic, rounded once to fp32 (ties to even) by searching the neighbours of the fp64 value."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = f32(float(exact))
    cands = [np.nextafter(near, f32(-np.inf)), near, np.nextafter(near, f32(np.inf))]
    dist = [abs(Fraction(float(x)) - exact) for x in cands]
    best = min(dist)
    winners = [x for x, d in zip(cands, dist) if d == best]
    if len(winners) > 1:
        winners = [x for x in winners if int(np.asarray(x, f32).view(np.uint32)) & 1 == 0]
    return winners[0]


def test_fma_is_correctly_rounded_on_fp32_ties_in_both_directions():
    """c + a b with a b = -+2^-24 (1 - 2^-44): the exact sum lies 2^-68 beside the midpoint of two fp32 numbers, fp64 rounds
    it onto the midpoint, and the second rounding goes to the even neighbour, the wrong one in both constructions."""
    a = f32(1 + 2.0 ** -22)
    below = f32((1 - 2.0 ** -22) * 2.0 ** -24)                  # a * below = 2^-24 (1 - 2^-44)
    cases = [(a, below, f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23)),        # just below 1 + 3 2^-24: down to the odd 1 + 2^-23
             (a, -below, f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23)),       # just above 1 + 2^-24: up to the odd 1 + 2^-23
             (a, -below, f32(-1 - 2.0 ** -23), f32(-1 - 2.0 ** -23))]     # the mirror image of the first
    seen = set()
    for x, y, c, want in cases:
        old, new, exact = AO.fma_twice_rounded(x, y, c), AO.fma(x, y, c), _exact_fma(x, y, c)
        r64 = f64(x) * f64(y) + f64(c)
        assert int(np.asarray(r64).view(np.uint64)) & 0x1FFFFFFF == 0x10000000, "the fp64 sum is not an fp32 midpoint"
        assert new == exact == want, (x, y, c, new, exact)
        assert old != new and abs(float(old) - float(new)) == 2.0 ** -23, "the twice-rounded formula was expected to miss"
        seen.add(float(old) > float(new))
    assert seen == {True, False}, "one construction must round too far up and one too far down"
    # vectors, scalars and broadcasting, with ties and ordinary operands mixed
    rng = np.random.Generator(np.random.PCG64(1))
    X, Y, Cc = (rng.standard_normal(1000).astype(f32) for _ in range(3))
    X[::100], Y[::100], Cc[::100] = a, below, f32(1 + 2.0 ** -23)
    got = AO.fma(X, Y, Cc)
    assert got.dtype == np.float32 and all(got[n] == _exact_fma(X[n], Y[n], Cc[n]) for n in range(1000))
    assert np.all(got[::100] == f32(1 + 2.0 ** -23)) and np.all(AO.fma_twice_rounded(X, Y, Cc)[::100] != got[::100])
    assert AO.fma(X[:, None], Y[None, :3], f32(0.5)).shape == (1000, 3) and isinstance(AO.fma(a, below, f32(1)), np.float32)
    # products that underflow keep their sign, as IEEE says (the GQA data relies on it)
    tiny = f32(2.0 ** -100)
    assert np.signbit(AO.fma(tiny, -tiny, f32(0))) and AO.fma(tiny, -tiny, f32(0)) == 0
    assert np.signbit(AO.fma(tiny, -tiny, -f32(0))) and not np.signbit(AO.fma(f32(0), f32(-1), f32(0)))


# ---- the expf arguments ---------------------------------------------------------------------------------------------------
def _fused_sets():
    sets = [("P1", case, k, kv) for case in OC.CASES for k, kv in OC.GEOMETRIES]       # (the odd-ld run uses the (16, 12) data)
    return sets + [("P2", case, 8, 40) for case in ("q0", "stats_k0")]


def _emulate(s, tp, ti, case, d, wrong=None, rows=None, keys=None):
    """test_gpu_order.emulate (a test module is not imported): the arrays the GPU test compares on data set d."""
    Q, K, V, dO, scale = d["Q"], d["K"], d["V"], d["dO"], d["scale"]
    want = {}
    if case.startswith("stats"):
        O, stats = d["O"], d["stats"]
    else:
        O, stats = AO.attention_forward(s.rp, s.ci, Q, K, V, scale, wrong, rows)
        want["O"], want["stats"] = O, stats
    want["dQ"], want["delta"] = AO.attention_backward_q(s.rp, s.ci, Q, K, V, O, dO, stats, scale, wrong, rows)
    if case != "maxima":
        delta_in = d["delta"] if case.startswith("stats") else want["delta"]
        want["dK"], want["dV"] = AO.attention_backward_kv(tp, ti, Q, K, V, dO, stats, delta_in, scale, wrong, keys)
    return want


def test_every_expf_argument_of_the_bit_comparisons_is_zero_or_at_most_minus_128():
    """The sums over the nonzeros feed no expf and are left out here (AO.without_chains): the arguments are the full run's."""
    total = 0
    for name, case, k, kv in _fused_sets():
        s = OC.pattern(name)
        tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
        with AO.expf_arguments() as log, AO.without_chains():
            _emulate(s, tp, ti, case, OC.attention_data(name, case, k, kv))
        assert log and AO.expf_arguments_are_exact(log), f"{name} {case} k={k} kv={kv}: an expf argument outside {{0, <= -128, -Inf}}"
        x = np.concatenate(log)
        total += x.size
        if case == "maxima":
            assert np.any(x == -128) and np.any(x == 0) and np.any(np.isneginf(x)), "the maxima data must rescale"
    for name, case, k, kv, minus_zero in (("P1", "stats_k0", 16, 12, False), ("P1", "stats_q0", 8, 40, False), ("P2", "stats_k0", 16, 12, True)):
        s = OC.pattern(name)
        tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
        for h in range(4):
            with AO.expf_arguments() as log, AO.without_chains():
                _emulate(s, tp, ti, case, OC.attention_data(name, case, k, kv, head=h, minus_zero=minus_zero))
            assert log and AO.expf_arguments_are_exact(log), f"gqa {name} {case} head {h}"
            total += sum(x.size for x in log)
    print(f"{total} expf arguments, every one +-0, at most -128 or -Inf")
    # the check itself tells general data apart
    s = OC.p2()
    Q, K, V = OC.randn(5, (s.rows, 8), (s.cols, 8), (s.cols, 8))
    with AO.expf_arguments() as log, AO.without_chains():
        AO.attention_forward(s.rp, s.ci, Q, K, V, 0.3, only=range(20))
    assert not AO.expf_arguments_are_exact(log)


# ---- every mistake is visible ---------------------------------------------------------------------------------------------
def _sample(s):
    """Rows of P1 that cover every length of LENGTHS, every one-key row and low-first rows in steps and in pieces; 3 keys."""
    lengths = np.diff(s.rp)
    rows, seen = [], set()
    for i in np.argsort(lengths, kind="stable"):
        if lengths[i] not in seen or (i % 9 == 0 and lengths[i] <= 140):
            rows.append(int(i))
            seen.add(int(lengths[i]))
    one_key = [i for i in range(s.rows) if lengths[i] and len(set(s.ci[s.rp[i]:s.rp[i + 1]].tolist())) == 1]
    low_first = [i for i in range(s.rows) if lengths[i] in (17, 513, 1025) and (s.ci[s.rp[i]:s.rp[i] + 8] < OC.P1_LOW).all()]
    return sorted(set(rows + one_key + low_first)), [7, 17, 24]      # (17 and 24: more than 1024 queries, three pieces)


def _differs(a, b, fold=True):
    a, b = (np.ascontiguousarray(x, f32) for x in (a, b))
    if fold:
        a, b = a + f32(0), b + f32(0)
    return bool(np.any(a.view(np.uint32) != b.view(np.uint32)))


# (mistake, array) -> why no input can make the pairing visible while every expf argument stays in {0, <= -128, -Inf}
EXEMPT = {
    (m, "stats"): "M is a maximum and l a count of ones: both exact in any order" for m in AO.ORDER_MISTAKES
}
EXEMPT.update({
    ("unfused", "O"): "every multiplier of the forward chains (e, alpha, w_p) is exactly 0 or 1, so each product is exact",
    ("sequential", "O"): "the only butterfly before O is the score's, and the scores are +-0 or exact",
    ("sequential", "dV"): "dV = sum p dO takes p from the scores, which are +-0 or exact; no other dot product enters",
})


def test_every_mistake_changes_bits_of_every_array_the_gpu_test_compares():
    s = OC.p1()
    tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
    rows, keys = _sample(s)
    assert {int(n) for n in np.diff(s.rp)[rows]} >= set(OC.LENGTHS) and np.diff(tp)[keys].max() > 2 * AO.PIECE
    k, kv = 16, 12                                              # four lanes: a butterfly of two levels
    changed = {}                                                # (mistake, array) -> the cases in which it changes
    for case in OC.CASES:
        d = OC.attention_data("P1", case, k, kv)
        right = _emulate(s, tp, ti, case, d, None, rows, keys)
        for m in AO.ORDER_MISTAKES:
            wrong = _emulate(s, tp, ti, case, d, m, rows, keys)
            for w in right:
                if _differs(right[w], wrong[w]):
                    changed.setdefault((m, w), []).append(case)
    for m in AO.ORDER_MISTAKES:
        for w in ("O", "stats", "delta", "dQ", "dK", "dV"):
            if (m, w) in EXEMPT:
                assert (m, w) not in changed, f"{m} changes {w} after all ({changed.get((m, w))}): it is no exemption"
            else:
                assert changed.get((m, w)), f"{m} changes no bit of {w} on any data set: the inputs are too tame"
    # the strongest pin on the backward chains: with caller-made stats every chain mistake shows in its own array
    for m in ("reversed", "pieces_last_to_first", "unfused"):
        assert "stats_q0" in changed[(m, "dQ")] and "stats_k0" in changed[(m, "dK")] and "stats_k0" in changed[(m, "dV")], m
    # the rescale and the combine are live in the maxima data: O there depends on the order of the pieces and of the steps
    assert "maxima" in changed[("reversed", "O")] and "maxima" in changed[("pieces_last_to_first", "O")]
    print("changed:", {f"{m}/{w}": c for (m, w), c in sorted(changed.items())})


def test_every_mistake_changes_bits_of_spmm_sddmm_and_softmax_backward():
    s, vals, X = OC.spmm_data("P1", 13)
    rows, _ = _sample(s)
    right = AO.spmm(s.rp, s.ci, vals, X, only=rows)
    for m in ("reversed", "pieces_last_to_first", "unfused"):             # (SpMM has no butterfly)
        assert _differs(right, AO.spmm(s.rp, s.ci, vals, X, m, only=rows)), f"spmm: {m}"
    for k in (13, 24, 40, 64):                                            # (k <= 4 is one lane: no butterfly; 3 and 4 fuse alike)
        s, U, Xs = OC.sddmm_data("P1", k)
        right = AO.sddmm(s.rp[:41], s.ci, U, Xs)[:s.rp[40]]
        for m in ("sequential", "unfused"):                               # (a dot product has no storage order and no pieces)
            if k == 13 and m == "sequential":
                continue                                                  # (two partials after the first level: one addition either way)
            assert _differs(right, AO.sddmm(s.rp[:41], s.ci, U, Xs, m)[:s.rp[40]]), f"sddmm k={k}: {m}"
    for k in (3, 4):
        s, U, Xs = OC.sddmm_data("P1", k)
        assert _differs(AO.sddmm(s.rp[:41], s.ci, U, Xs)[:s.rp[40]], AO.sddmm(s.rp[:41], s.ci, U, Xs, "unfused")[:s.rp[40]]), f"sddmm k={k}"
    s, P, dP = OC.softmax_data("P1")
    for scale in (1.0, 0.3, -0.7):
        right = AO.softmax_backward(s.rp, P, dP, scale)
        for m in AO.ORDER_MISTAKES:
            assert _differs(right, AO.softmax_backward(s.rp, P, dP, scale, m)), f"softmax backward scale={scale}: {m}"


def test_a_gqa_fold_from_plus_zero_is_visible_only_where_a_gradient_is_minus_zero():
    """x + 0 = x for every x but -0.  A transposed row in pieces is added from +0 and is never -0, so on P1 the fold from +0
    cannot be seen; on P2 the data gives one key -0 in every head, and there the two folds differ, in dK_c and in dV_c."""
    k, kv = 16, 12
    s = OC.p2()
    tp, ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
    j = OC.neg_zero_key()
    single = []
    for h in range(2):
        d = OC.attention_data("P2", "stats_k0", k, kv, head=h, minus_zero=True)
        d0 = OC.attention_data("P2", "stats_k0", k, kv, head=0, minus_zero=True)       # (K and V of K/V head 0)
        Kc, Vc = d0["K"], d0["V"]
        single.append(AO.attention_backward_kv(tp, ti, d["Q"], Kc, Vc, d["dO"], d["stats"], d["delta"], d["scale"], only=[j, j + 1]))
    for w, name in ((0, "dK"), (1, "dV")):
        right, wrong = AO.gqa_fold([x[w] for x in single]), AO.gqa_fold([x[w] for x in single], from_zero=True)
        assert np.all(right[j] == 0) and np.all(np.signbit(right[j])) and not np.any(np.signbit(wrong[j])), name
        assert _differs(right, wrong, fold=False) and not _differs(right, wrong, fold=True), name
        assert np.any(right[j + 1] != 0) or tp[j + 2] == tp[j + 1]
    # P1: every transposed row is a sum of pieces from +0
    s1 = OC.p1()
    assert np.bincount(s1.ci, minlength=s1.cols).min() > AO.PIECE
    assert not np.signbit(AO.ordered_fma_sum(np.full(600, f32(2.0 ** -100)), np.full((600, 2), -f32(2.0 ** -100)))).any()


# ---- the per-nonzero reference ------------------------------------------------------------------------------------------
def test_the_multiset_reference_is_dense_attention_where_no_key_repeats_and_counts_a_repeated_key_twice():
    rng = np.random.Generator(np.random.PCG64(9))
    rows, cols, k, kv = 30, 50, 6, 5
    lengths = rng.integers(0, 12, size=rows)
    lengths[:2] = 0, 1
    rp = np.concatenate([[0], np.cumsum(lengths)])
    ci = np.concatenate([rng.permutation(cols)[:n] for n in lengths])           # unsorted, no repeats
    Q, K, V, dO = OC.randn(10, (rows, k), (cols, k), (cols, kv), (rows, kv))
    got, mag, _ = AO.multiset_attention(rp, ci, Q, K, V, dO, 0.3)
    mask = np.zeros((rows, cols), bool)
    mask[np.repeat(np.arange(rows), lengths), ci] = True
    sc = f64(f32(0.3))
    S = np.where(mask, sc * (Q.astype(f64) @ K.astype(f64).T), -np.inf)
    with np.errstate(invalid="ignore"):
        P = np.exp(S - S.max(1, keepdims=True, initial=-1e300, where=mask))
    P = np.where(mask, P, 0.0)
    P /= np.where(P.sum(1, keepdims=True) > 0, P.sum(1, keepdims=True), 1.0)
    dP = dO.astype(f64) @ V.astype(f64).T
    dS = sc * P * (dP - (P * dP).sum(1, keepdims=True))
    for w, want in (("O", P @ V), ("dQ", dS @ K), ("dK", dS.T @ Q), ("dV", P.T @ dO)):
        assert np.allclose(got[w], want, rtol=1e-12, atol=1e-14), w
    assert not got["O"][0].any() and not got["dQ"][0].any() and np.array_equal(got["O"][1], V[ci[0]].astype(f64))
    # a row that lists key a three times and key b once: O = (3 V_a + V_b) / 4 with Q = 0; a dense mask would give the half sum
    rp2, ci2 = np.array([0, 4]), np.array([7, 2, 7, 7])
    got2, _, _ = AO.multiset_attention(rp2, ci2, np.zeros((1, k), f32), K, V, dO[:1], 0.3)
    assert np.allclose(got2["O"][0], (3 * V[7].astype(f64) + V[2]) / 4) and not np.allclose(got2["O"][0], (V[7].astype(f64) + V[2]) / 2)
    assert np.allclose(got2["dV"][7], 0.75 * dO[0]) and np.allclose(got2["dV"][2], 0.25 * dO[0])
    # the same function in fp32 is the yardstick of the GPU test
    got32, _, _ = AO.multiset_attention(rp, ci, Q, K, V, dO, 0.3, dtype=f32)
    assert got32["O"].dtype == np.float32 and np.allclose(got32["O"], got["O"], rtol=1e-4, atol=1e-5)
