"""Fused and composed attention on unsorted rows and repeated keys, with the device's own expf (include/spmv_hip.h "Fused
attention": rows need not be sorted, a column may repeat, and a row's output is a pure function of its column list in
storage order).  The other attention tests build their rows sorted and without repeats and compare with a dense boolean
mask, which cannot express a key that a row lists twice.  Here the reference is the per-nonzero one of
tests/_attention_order.py (multiset_attention): scores per stored nonzero, a segment softmax over row_ptr, segment sums for O
and dQ, index_add over the nonzeros for dK and dV; a key listed twice counts twice in the softmax, is gathered twice into O
and appears twice in the transposed row that backward_kv walks.

Patterns: tests/_order_cases.py.  P1 is a multigraph (40 keys, columns with replacement, rows that list one key up to 513
times, every transposed row in pieces with repeated queries); P2 is shuffled with duplicates and has short transposed rows.

exact       Q = 0 (and once K = 0), integer V and dO in [-4, 4], k = kv = 8, rows of power-of-two length 1 .. 16 drawn with
            replacement from 6 keys: O, dQ, dK and dV equal the fp64 per-nonzero reference bit for bit.  One row lists key 4
            three times and key 1 once: O = (3 V_4 + V_1) / 4.  A dense mask, for which a key is listed or not, would give
            the half sum (V_4 + V_1) / 2 there.
general     normal Q, K, V, dO at (k, kv) = (24, 24), (8, 40), (4, 4) and scales 2^-2 and 0.3, on three paths: the three
            fused passes directly, FusedSparseAttention through autograd (heads="loop" and "batched" at 4 query heads on 2
            K/V heads) and the composed SparseAttention through autograd.  The project's rule: the error divided by the
            magnitude of the chain taken with absolute values is at most max(4 x the same reference run in fp32 under the
            same normalisation, RTOL); both figures are printed.  D = max t - min t <= 32 in every row is checked on the host.
identities  a row that lists one key L times has O equal to that V row (the general rule) and stats[i][0] equal to its
            single score bit for bit; shuffling the nonzeros inside the rows leaves stats[:, 0] bit-identical; the batched
            (GQA) holder and the loop holder give the same bits.
"""
import numpy as np
import pytest

import _attention_order as AO
import _exact as E
import _order_cases as OC
from _util import RTOL

pytestmark = pytest.mark.gpu

GUARD, GUARD_N = 3.0e35, 4096
f32, f64 = np.float32, np.float64
WHATS = ("O", "dQ", "dK", "dV")


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _guarded(gpu, rows, w):
    import torch
    buf = torch.full((2 * GUARD_N + rows * w,), GUARD, dtype=torch.float32, device=gpu)
    out = buf[GUARD_N:GUARD_N + rows * w].view(rows, w)
    out.fill_(float("nan"))
    return buf, out


def _folded(a):
    return (np.ascontiguousarray(a, f32) + f32(0)).view(np.uint32)


class Handles:
    def __init__(self, pkg, s, gpu):
        import torch
        self.keep = (_dev(gpu, s.rp), _dev(gpu, s.ci), torch.zeros(s.nnz, dtype=torch.float32, device=gpu))
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=False)
        self.A.attention_plan()
        self.T.attention_plan()

    def close(self):
        self.T.close()
        self.A.close()


def _run(h, gpu, Q, K, V, dO, scale):
    """The three passes into NaN-filled outputs between guard bands; numpy results."""
    import torch
    A, T = h.A, h.T
    k, kv = Q.shape[1], V.shape[1]
    Q, K, V, dO = (_dev(gpu, x) for x in (Q, K, V, dO))
    made = [_guarded(gpu, n, w) for n, w in ((A.rows, kv), (A.rows, 2), (A.rows, 1), (A.rows, k), (A.cols, k), (A.cols, kv))]
    O, stats, delta, dQ, dK, dV = (o for _, o in made)
    delta = delta.reshape(-1)
    A.attention_forward(Q, K, V, O, stats, scale)
    A.attention_backward_q(Q, K, V, O, dO, stats, delta, dQ, scale)
    T.attention_backward_kv(Q, K, V, dO, stats, delta, dK, dV, scale)
    torch.cuda.synchronize()
    for buf, _ in made:
        assert bool((buf[:GUARD_N] == GUARD).all()) and bool((buf[-GUARD_N:] == GUARD).all()), "a pass wrote outside its output"
    return {n: t.cpu().numpy() for n, t in (("O", O), ("stats", stats), ("delta", delta), ("dQ", dQ), ("dK", dK), ("dV", dV))}


# ---- exact ---------------------------------------------------------------------------------------------------------------
KEY_A, KEY_B = 4, 1


def _exact_pattern():
    rng = np.random.Generator(np.random.PCG64(61))
    lengths = [1, 2, 4, 8, 16] * 4
    rows = [rng.integers(0, 6, size=n) for n in lengths]
    rows[2] = np.array([KEY_A, KEY_B, KEY_A, KEY_A])
    rp = np.concatenate([[0], np.cumsum(lengths)])
    s = E.Structure(len(rows), 6, rp, np.concatenate(rows))
    assert any(len(set(r.tolist())) < len(r) for r in rows) and any(np.any(np.diff(r) < 0) for r in rows)
    return s


def test_attention_on_repeated_keys_is_exact_against_the_per_nonzero_reference(pkg, gpu):
    s = _exact_pattern()
    h = Handles(pkg, s, gpu)
    ints = lambda seed, shape: np.random.Generator(np.random.PCG64(seed)).integers(-4, 5, size=shape).astype(f32)       # noqa: E731
    for step, zero in enumerate(("Q", "K")):
        Q, K, V, dO = ints(10 + step, (s.rows, 8)), ints(20 + step, (6, 8)), ints(30 + step, (6, 8)), ints(40 + step, (s.rows, 8))
        (Q if zero == "Q" else K)[:] = 0
        got = _run(h, gpu, Q, K, V, dO, 0.25)
        want, _, _ = AO.multiset_attention(s.rp, s.ci, Q, K, V, dO, 0.25)
        for w in WHATS:
            assert np.array_equal(want[w].astype(f32).astype(f64), want[w]), f"{w}: the expectation is not an fp32 number"
            assert np.array_equal(_folded(got[w]), _folded(want[w].astype(f32))), f"{zero} = 0: {w} differs from the per-nonzero reference"
        assert (got["dQ"] if zero == "Q" else got["dK"]).any() and got["dV"].any() and not (got["dK"] if zero == "Q" else got["dQ"]).any()
        # key 4 three times and key 1 once: three quarters and one quarter, not the halves of a dense mask
        assert np.array_equal(got["O"][2], ((3 * V[KEY_A].astype(f64) + V[KEY_B]) / 4).astype(f32))
        assert not np.array_equal(got["O"][2], ((V[KEY_A].astype(f64) + V[KEY_B]) / 2).astype(f32))
        assert np.array_equal(got["stats"][:, 1], (1.0 / np.diff(s.rp)).astype(f32))
    h.close()


# ---- general -------------------------------------------------------------------------------------------------------------
def _errors(tag, got, r64, r32, mag):
    """The rule of the attention tests on every output of `got`: prints our figure beside the yardstick's."""
    for w in WHATS:
        if w not in got:
            continue
        g, live = np.asarray(got[w], f64), mag[w] > 0
        assert live.any(), f"{tag} {w}: nothing to compare"
        assert np.all(g[~live] == 0), f"{tag} {w}: a value where nothing contributes"
        ours = float(np.max(np.abs(g - r64[w])[live] / mag[w][live]))
        yard = float(np.max(np.abs(r32[w].astype(f64) - r64[w])[live] / mag[w][live]))
        print(f"{tag} {w}: normalised error {ours:.3g}, the per-nonzero reference in fp32 {yard:.3g}")
        assert ours <= max(4.0 * yard, RTOL), f"{tag} {w}: {ours:.3g} against {yard:.3g} of the fp32 per-nonzero reference"


def _references(s, Q, K, V, dO, scale):
    r64, mag, t = AO.multiset_attention(s.rp, s.ci, Q, K, V, dO, scale)
    r32, _, _ = AO.multiset_attention(s.rp, s.ci, Q, K, V, dO, scale, dtype=f32)
    D = AO.score_spread(s.rp, t)
    assert D <= 32.0, f"D = {D}: choose another seed"
    return r64, r32, mag


GENERAL = [(name, k, kv, scale) for name in ("P1", "P2") for k, kv in ((24, 24), (8, 40), (4, 4)) for scale in (0.25, 0.3)]


@pytest.mark.parametrize("name,k,kv,scale", GENERAL, ids=[f"{n}-k{k}-kv{kv}-scale{sc}" for n, k, kv, sc in GENERAL])
def test_attention_on_unsorted_rows_and_repeated_keys_against_the_per_nonzero_reference(pkg, gpu, name, k, kv, scale):
    import torch
    s = OC.pattern(name)
    tag = f"{name} k={k} kv={kv} scale={scale}"
    heads, kv_heads = 4, 2
    seed = [sum(map(ord, name)), k, kv, int(scale * 100)]
    Qh, dOh = OC.randn(seed + [1], (heads, s.rows, k), (heads, s.rows, kv))
    Kh, Vh = OC.randn(seed + [2], (kv_heads, s.cols, k), (kv_heads, s.cols, kv))
    refs = [_references(s, Qh[y], Kh[y // 2], Vh[y // 2], dOh[y], scale) for y in range(heads)]
    # the three fused passes directly (head 0's data)
    h = Handles(pkg, s, gpu)
    got = _run(h, gpu, Qh[0], Kh[0], Vh[0], dOh[0], scale)
    _errors(f"{tag} fused passes", got, *refs[0])
    lengths = np.diff(s.rp)
    assert not got["O"][lengths == 0].any() and not got["dQ"][lengths == 0].any()
    # a row that lists one key L times: O is that V row, and the row maximum is the single score SDDMM gives
    one_key = [i for i in range(s.rows) if lengths[i] > 1 and len(set(s.ci[s.rp[i]:s.rp[i + 1]].tolist())) == 1]
    if name == "P1":
        assert sorted(lengths[one_key].tolist()) == [8, 512, 513]
        S = torch.empty(s.nnz, dtype=torch.float32, device=gpu)
        h.A.sddmm(_dev(gpu, Qh[0]), _dev(gpu, Kh[0]), S)
        t = (torch.tensor(scale, dtype=torch.float32, device=gpu) * S).cpu().numpy()
        for i in one_key:
            j = int(s.ci[s.rp[i]])
            v64, mag = Vh[0][j].astype(f64), np.abs(Vh[0][j]).astype(f64)
            yard = float(np.max(np.abs(refs[0][1]["O"][i] - v64)[mag > 0] / mag[mag > 0]))
            ours = float(np.max(np.abs(got["O"][i] - v64)[mag > 0] / mag[mag > 0]))
            print(f"{tag} one key {lengths[i]} times: O against the V row {ours:.3g}, the fp32 reference {yard:.3g}")
            assert ours <= max(4.0 * yard, RTOL)
            assert got["stats"][i, 0].view(np.uint32) == t[s.rp[i]].view(np.uint32), "the row maximum is not the single score"
            assert len(set(t[s.rp[i]:s.rp[i + 1]].view(np.uint32).tolist())) == 1
    # shuffling the nonzeros inside the rows leaves the row maxima bit-identical
    rng = np.random.Generator(np.random.PCG64(seed + [3]))
    order = np.lexsort((rng.random(s.nnz), s.row_of))
    s2 = E.Structure(s.rows, s.cols, s.rp, s.ci[order])
    assert np.any(s2.ci != s.ci)
    h2 = Handles(pkg, s2, gpu)
    got2 = _run(h2, gpu, Qh[0], Kh[0], Vh[0], dOh[0], scale)
    assert np.array_equal(got2["stats"][:, 0].view(np.uint32), got["stats"][:, 0].view(np.uint32)), "stats[:, 0] depends on the order"
    _errors(f"{tag} fused passes, rows shuffled again", got2, *refs[0])
    h2.close()
    h.close()
    # the composed SparseAttention through autograd (head 0's data)
    d_rp, d_ci = _dev(gpu, s.rp), _dev(gpu, s.ci)
    composed = pkg.sparse_attention.SparseAttention(s.rows, s.cols, d_rp, d_ci, scale=scale)
    Qc, Kc, Vc = (_dev(gpu, x).requires_grad_(True) for x in (Qh[0], Kh[0], Vh[0]))
    Oc = composed(Qc, Kc, Vc)
    Oc.backward(_dev(gpu, dOh[0]))
    torch.cuda.synchronize()
    _errors(f"{tag} composed", {"O": Oc.detach().cpu().numpy(), "dQ": Qc.grad.cpu().numpy(), "dK": Kc.grad.cpu().numpy(),
                                 "dV": Vc.grad.cpu().numpy()}, *refs[0])
    composed.close()
    # FusedSparseAttention through autograd: 4 query heads on 2 K/V heads, one after the other and in one launch per kernel
    r64 = {w: np.stack([r[0][w] for r in refs]) for w in ("O", "dQ")}
    r32 = {w: np.stack([r[1][w] for r in refs]) for w in ("O", "dQ")}
    mag = {w: np.stack([r[2][w] for r in refs]) for w in ("O", "dQ")}
    for w in ("dK", "dV"):          # a K/V head's gradient is the sum over its two query heads
        r64[w] = np.stack([refs[2 * c][0][w] + refs[2 * c + 1][0][w] for c in range(kv_heads)])
        r32[w] = np.stack([refs[2 * c][1][w] + refs[2 * c + 1][1][w] for c in range(kv_heads)])
        mag[w] = np.stack([refs[2 * c][2][w] + refs[2 * c + 1][2][w] for c in range(kv_heads)])
    results = {}
    for mode in ("loop", "batched"):
        att = pkg.sparse_attention.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=scale, heads=mode)
        Q, K, V = (_dev(gpu, x).requires_grad_(True) for x in (Qh, Kh, Vh))
        O = att(Q, K, V)
        O.backward(_dev(gpu, dOh))
        torch.cuda.synchronize()
        results[mode] = {"O": O.detach().cpu().numpy(), "dQ": Q.grad.cpu().numpy(), "dK": K.grad.cpu().numpy(), "dV": V.grad.cpu().numpy()}
        assert results[mode]["dK"].shape == (kv_heads, s.cols, k) and results[mode]["O"].shape == (heads, s.rows, kv)
        _errors(f"{tag} holder heads={mode}", results[mode], r64, r32, mag)
        att.close()
    for w in WHATS:
        assert np.array_equal(np.ascontiguousarray(results["loop"][w]).view(np.uint32), np.ascontiguousarray(results["batched"][w]).view(np.uint32)), \
            f"{tag}: the batched holder's {w} differs from the loop holder's in a bit"
