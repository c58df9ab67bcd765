"""The fused attention passes on the GPU (spmv_csr_attention_forward / _backward_q / _backward_kv, include/spmv_hip.h "Fused
attention") and sparse_attention.FusedSparseAttention on top of them.  Every direct run of the passes writes into NaN-filled
outputs between guard bands of 4096 floats (and guard columns where ld exceeds the width) that must stay untouched.

exact       the pattern and data of test_gpu_sparse_attention's exact test (row lengths 1 .. 16, powers of two; integer V and
            dO; Q = 0 or K = 0): O, dQ, dK and dV equal torch's fp64 dense autograd bit for bit (+0 and -0 folded), at
            scale = 2^-2 and at -0.375, where nothing is rounded either.
scores      stats[:, 0] is bit for bit the row maximum of fp32(scale * A.sddmm(Q, K)), at 16, 8 and 1 lanes per row and at
            scales 2^-2, 0.3 and -0.7 (there the scaled minimum of the scores).
general     three patterns (short rows; rows of 512 .. 4100 beside short ones; 3000 queries on 48 keys, whose transposed rows
            lie on both sides of 512) times four (k, kv), one of them also with every ld % 4 != 0.  The error of O divided by
            P |V| and the gradients' errors divided by the magnitudes of test_gpu_sparse_attention are each at most
            max(4 x torch's fp32 dense autograd under the same normalisation, RTOL): another order of the sums at equal
            precision may differ by a small factor.  The composed SparseAttention's figures are printed beside the fused ones.
            Four more (k, kv) with k, kv <= 4 run one lane per row (no plan order, no shuffle, 8 column indices per lane), on
            both load paths; two patterns run at scales 0.3 and -1.7 as well (t and ds are rounded there; the reference
            takes fp32(scale), what the kernel receives).
zero        scale = +0 and -0: dQ = dK = 0, stats[:, 0] = 0, O and dV by the general rule (every p is 1 / L).
masks       keys masked with K[j, 0] = -Inf (Q[:, 0] = 1): rows whose first 20 entries are masked, rows masked entirely, a row
            with a NaN, empty rows.  The reference is the dense autograd of the pattern WITHOUT the masked entries and with a
            finite K.  One deviation is IEEE's, not the kernel's: dQ[i][0] of a row that lists a masked key is 0 * -Inf = NaN
            in every implementation (torch's dense autograd and the composed path included), so that column is checked to be
            NaN there and everything else against the reference.
special     tests/_attention_rows.py's rows on 2600 keys with masked stretches on both sides of the finite keys: 512 or 1024
            leading or 512 trailing masked entries leave the bits of O, stats and dQ[:, 1:] to the finite entries alone
            (whole masked pieces in the combine), masked entries across a piece boundary pass the general rule, long rows
            that are masked entirely or hold a NaN or a +Inf are NaN rows, and three keys that 700 queries list run in
            pieces on the transposed handle: the masked one gets dK = dV = 0, the one a NaN row lists NaN, the third is
            compared.  Once with 4 lanes per row, once with 1.
invariance  40 rows of 1 .. 700 entries give the same bits of O, stats and dQ among short rows, among rows of 300, as a row
            block with a rebased row_ptr, with strided operands and on the 4-byte load path; at 8 lanes per row and at 1.
extreme     tests/_attention_rows.py's score profiles, every score exact: maxima that rise or fall at every step (by 0.5, or
            by 128 and more so that the rescaling factor underflows), a spike of 200 first or last (at 513 entries the only
            nonzero of the last piece), 0 and -200 in turn, scores near 256; lengths 1 .. 1025.  The general rule with an
            absolute floor of 2^-90 for what underflows; every output finite.
heads       three heads as column blocks of (rows, 24) tensors: no copy, and the bits of three single-head calls.
memory      a forward plus backward step of the fused holder allocates less than 4 nnz bytes; the composed holder more.
graph       the three passes captured on one stream and replayed with new data in place: the bits of the eager run.
refusals    k or kv of 0 or 65, an ld below the width, a misaligned pointer, a scale that is not finite, a missing plan and a
            transposed handle of the wrong shape are refused and launch nothing.
"""
import ctypes as C

import numpy as np
import pytest

import _attention_rows as R
import _exact as E
from _util import RTOL

pytestmark = pytest.mark.gpu

GUARD, GUARD_N = 3.0e35, 4096
SCALE = 2.0 ** -2


def _bits(t):
    import torch
    return (t + 0.0).contiguous().view(torch.int32)


def _raw_bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _ints(gpu, seed, shape):
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(-4, 5, size=shape).astype(np.float32)).to(gpu)


def _pow2_pattern(rows, cols, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = 2 ** rng.integers(0, 5, size=rows)
    lengths[:5] = (1, 2, 4, 8, 16)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    return E.Structure(rows, cols, rp, ci)


def _rows_pattern(lengths, cols, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = np.asarray(lengths, np.int64)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    parts = [np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lengths if n]
    return E.Structure(len(lengths), cols, rp, np.concatenate(parts).astype(np.int32))


def _mask(s, gpu, keep=None):
    import torch
    m = torch.zeros((s.rows, s.cols), dtype=torch.bool, device=gpu)
    r, c = s.row_of, s.ci.astype(np.int64)
    if keep is not None:
        r, c = r[keep], c[keep]
    m[torch.from_numpy(r).to(gpu), torch.from_numpy(c).to(gpu)] = True
    return m


def _dense_autograd(mask, scale, Q, K, V, dO, dtype):
    """(O, dQ, dK, dV, P) of the masked softmax attention by torch's dense autograd in `dtype`; a row without a key gives
    a zero row of O and no gradient."""
    import torch
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (Q, K, V))
    full = mask.any(1)
    scores = torch.where(mask, (q @ k.t()) * scale, torch.tensor(float("-inf"), dtype=dtype, device=mask.device))
    P = torch.zeros_like(scores)
    P[full] = torch.softmax(scores[full], dim=1)
    O = P @ v
    O.backward(dO.to(dtype))
    return O.detach(), q.grad, k.grad, v.grad, P.detach()


# ---- guarded outputs and the direct run of the three passes ----------------------------------------------------------
def _guarded(gpu, rows, w, ld=None):
    """(buffer, rows x w view of leading dimension ld filled with NaN, between guard bands and beside guard columns)."""
    import torch
    ld = ld or w
    buf = torch.full((2 * GUARD_N + rows * ld,), GUARD, dtype=torch.float32, device=gpu)
    out = buf[GUARD_N:GUARD_N + rows * ld].view(rows, ld)[:, :w]
    out.fill_(float("nan"))
    return buf, out


def _intact(buf, rows, w, ld):
    body = buf[GUARD_N:GUARD_N + rows * ld].view(rows, ld)
    return (bool((buf[:GUARD_N] == GUARD).all()) and bool((buf[GUARD_N + rows * ld:] == GUARD).all())
            and bool((body[:, w:] == GUARD).all()))


def _strided(t, ld):
    """A copy of t with leading dimension ld; the columns past its width hold NaN."""
    import torch
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float32, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


class Handles:
    def __init__(self, pkg, s, gpu, plan=True):
        import torch
        self.keep = (torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu),
                     torch.zeros(s.nnz, dtype=torch.float32, device=gpu))
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=False)
        if plan:
            self.A.attention_plan()
            self.T.attention_plan()

    def close(self):
        self.T.close()
        self.A.close()


def _run(h, Q, K, V, dO, scale, ld=None):
    """The three passes into guarded outputs; ld: width -> leading dimension of every output (None: the width)."""
    import torch
    A, T = h.A, h.T
    k, kv = Q.shape[1], V.shape[1]
    made = []

    def out(rows, w, wide=True):
        l = ld(w) if ld and wide else w
        buf, o = _guarded(Q.device, rows, w, l)
        made.append((buf, rows, w, l))
        return o

    O, stats, delta = out(A.rows, kv), out(A.rows, 2, False), out(A.rows, 1, False).reshape(-1)
    dQ, dK, dV = out(A.rows, k), out(A.cols, k), out(A.cols, kv)
    A.attention_forward(Q, K, V, O, stats, scale)
    A.attention_backward_q(Q, K, V, O, dO, stats, delta, dQ, scale)
    T.attention_backward_kv(Q, K, V, dO, stats, delta, dK, dV, scale)
    torch.cuda.synchronize()
    assert all(_intact(*m) for m in made), "a pass wrote outside its output"
    return dict(O=O, stats=stats, delta=delta, dQ=dQ, dK=dK, dV=dV)


def _randn(gpu, seed, *shapes):
    import torch
    gen = torch.Generator(device=gpu).manual_seed(seed)
    return [torch.randn(s, generator=gen, device=gpu, dtype=torch.float32) for s in shapes]


# ---- exact -----------------------------------------------------------------------------------------------------------
def _exact(pkg, gpu, SCALE):
    import torch
    s = _pow2_pattern(3000, 2000, 5)
    assert set(np.diff(s.rp)) == {1, 2, 4, 8, 16}
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    att = pkg.sparse_attention.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE)
    composed = pkg.sparse_attention.SparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE)
    h = Handles(pkg, s, gpu)
    mask = _mask(s, gpu)
    for step, zero in enumerate(("Q", "K", "Q", "K")):       # the second pair: new data, no new plan
        Q, K = _ints(gpu, 10 + step, (s.rows, 8)), _ints(gpu, 20 + step, (s.cols, 8))
        V, dO = _ints(gpu, 30 + step, (s.cols, 8)), _ints(gpu, 40 + step, (s.rows, 8))
        (Q if zero == "Q" else K).zero_()
        Q.requires_grad_(True), K.requires_grad_(True), V.requires_grad_(True)
        O = att(Q, K, V)
        O.backward(dO)
        torch.cuda.synchronize()
        Od, dQd, dKd, dVd, P = _dense_autograd(mask, SCALE, Q, K, V, dO, torch.float64)
        direct = _run(h, Q.detach(), K.detach(), V.detach(), dO, SCALE)
        for what, got, want in (("O", O.detach(), Od), ("dQ", Q.grad, dQd), ("dK", K.grad, dKd), ("dV", V.grad, dVd)):
            assert got.shape == want.shape and got.dtype == torch.float32
            assert torch.equal(want.to(torch.float32).to(torch.float64), want), f"{what}: the expectation is not an fp32 number"
            assert torch.equal(_bits(got), _bits(want.to(torch.float32))), f"step {step} ({zero} = 0): {what} differs"
            assert torch.equal(_bits(direct[what]), _bits(got)), f"step {step}: the direct run's {what} differs from the holder's"
        assert bool((Q.grad if zero == "K" else K.grad).eq(0).all())
        assert bool((K.grad if zero == "K" else Q.grad).ne(0).any()) and bool(V.grad.ne(0).any())
        # delta = sum_c dO O equals the composed path's sum over the row of P dP exactly on this data
        dP = torch.where(mask, dO.double() @ V.detach().double().t(), torch.zeros((), dtype=torch.float64, device=gpu))
        assert torch.equal(direct["delta"].double(), (P * dP).sum(1))
        # the values are the composed path's
        Qc, Kc, Vc = (t.detach().clone().requires_grad_(True) for t in (Q, K, V))
        Oc = composed(Qc, Kc, Vc)
        Oc.backward(dO)
        for got, want in ((O.detach(), Oc.detach()), (Q.grad, Qc.grad), (K.grad, Kc.grad), (V.grad, Vc.grad)):
            assert torch.equal(_bits(got), _bits(want))
    # only some of the gradients asked for
    Q, K, V = _ints(gpu, 50, (s.rows, 8)).zero_(), _ints(gpu, 51, (s.cols, 8)), _ints(gpu, 52, (s.cols, 8)).requires_grad_(True)
    att(Q, K, V).backward(dO)
    torch.cuda.synchronize()
    assert Q.grad is None and K.grad is None
    assert torch.equal(_bits(V.grad), _bits(_dense_autograd(mask, SCALE, Q, K, V, dO, torch.float64)[3].to(torch.float32)))
    Q.requires_grad_(True), V.requires_grad_(False)
    att(Q, K, V).backward(dO)
    assert Q.grad is not None and K.grad is None and V.grad is not None      # (V.grad: the earlier one, untouched)
    for a in (att, composed, h):
        a.close()


def test_fused_attention_exact_against_dense_fp64_autograd(pkg, gpu):
    _exact(pkg, gpu, SCALE)


def test_fused_attention_exact_at_a_scale_that_is_no_power_of_two(pkg, gpu):
    """scale = -0.375: the scores are 0 (or -0), p = 2^-m and ds a multiple of 2^-11 below 2^8, so every intermediate is
    still an fp32 number and the bits are the fp64 autograd's; the composed path's as well."""
    _exact(pkg, gpu, -0.375)


# ---- the scores are SDDMM's ------------------------------------------------------------------------------------------
def test_fused_attention_row_maximum_is_the_sddmm_scores(pkg, gpu):
    import torch
    rows, cols, per = 512, 300, 24
    s = _rows_pattern([per] * rows, cols, 7)
    h = Handles(pkg, s, gpu)
    for k, kv in ((20, 20), (3, 4)):                         # (3, 4): one lane per row
        Q, K, V, dO = _randn(gpu, 3, (rows, k), (cols, k), (cols, kv), (rows, kv))
        S = torch.empty(s.nnz, dtype=torch.float32, device=gpu)
        h.A.sddmm(Q, K, S)
        assert bool((S.view(rows, per).max(1).values > 0).all()) and bool((S.view(rows, per).min(1).values < 0).all())
        # 0.3 and -0.7: t = scale * s is rounded; at -0.7 the maximum of t is the scaled minimum of s
        for scale in (SCALE, 0.3, -0.7):
            got = _run(h, Q, K, V, dO, scale)
            t = torch.tensor(scale, dtype=torch.float32, device=gpu) * S
            assert t.dtype == torch.float32
            assert torch.equal(_raw_bits(got["stats"][:, 0]), _raw_bits(t.view(rows, per).max(1).values)), f"k={k} scale={scale}"
            if scale < 0:
                assert torch.equal(got["stats"][:, 0], torch.tensor(scale, dtype=torch.float32, device=gpu) * S.view(rows, per).min(1).values)
            if k != 20:
                continue
            # ... and on a wider group than SDDMM's for this k (kv = 40: V = 16 against 8)
            V2, dO2 = _randn(gpu, 4, (cols, 40), (rows, 40))
            got2 = _run(h, Q, K, V2, dO2, scale)
            assert torch.equal(_raw_bits(got2["stats"][:, 0]), _raw_bits(got["stats"][:, 0]))
    h.close()


# ---- general ---------------------------------------------------------------------------------------------------------
def _keys48():
    s = _rows_pattern([8] * 3000, 48, 0)
    per_key = np.bincount(s.ci, minlength=48)
    assert per_key.min() <= 512 < per_key.max(), "the transposed pattern must have rows on both sides of 512"
    return s


def _general_structure(name, pkg, oracle):
    return _keys48() if name == "keys48" else E.structure(name, pkg, oracle)


def _normalised(mask, scale, Q, K, V, dO, P):
    """The magnitudes the errors are divided by: O's P |V| and the gradients' as in test_gpu_sparse_attention."""
    import torch
    aQ, aK, aV, adO = (x.detach().double().abs() for x in (Q, K, V, dO))
    dP_abs = torch.where(mask, adO @ aV.t(), torch.zeros((), dtype=torch.float64, device=Q.device))
    dS_abs = abs(scale) * P * (dP_abs + (P * dP_abs).sum(1, keepdim=True))
    return {"O": P @ aV, "dQ": dS_abs @ aK, "dK": dS_abs.t() @ aQ, "dV": P.t() @ adO}


def _check_general(tag, got, mask, scale, Q, K, V, dO, other=None, rows=None, cols=None, whats=("O", "dQ", "dK", "dV")):
    """got[what] against the fp64 dense autograd, yardstick torch's fp32 dense autograd; `other`: results printed beside.
    rows / cols: boolean selections of the queries / keys that are compared (None: all); whats: the outputs compared."""
    import torch
    *r64, P = _dense_autograd(mask, scale, Q, K, V, dO, torch.float64)
    r64 = dict(zip(("O", "dQ", "dK", "dV"), r64))
    r32 = dict(zip(("O", "dQ", "dK", "dV"), _dense_autograd(mask, scale, Q, K, V, dO, torch.float32)))
    mags = _normalised(mask, scale, Q, K, V, dO, P)
    for what in whats:
        sel = rows if what in ("O", "dQ") else cols
        pick = (lambda t: t) if sel is None else (lambda t: t[sel])
        g, g64, g32, mag = pick(got[what]), pick(r64[what]), pick(r32[what]), pick(mags[what])
        live = mag > 0
        assert bool(live.any()), f"{tag} {what}: nothing to compare"
        assert bool((g[~live] == 0).all()), f"{tag} {what}: a value where nothing contributes"
        ours = float(((g.double() - g64).abs()[live] / mag[live]).max())
        yard = float(((g32.double() - g64).abs()[live] / mag[live]).max())
        beside = ""
        if other is not None:
            beside = f", composed {float(((pick(other[what]).double() - g64).abs()[live] / mag[live]).max()):.3g}"
        print(f"{tag} {what}: normalised error fused {ours:.3g}{beside}, torch fp32 dense autograd {yard:.3g}")
        assert ours <= max(4.0 * yard, RTOL), f"{tag} {what}: {ours:.3g} against {yard:.3g} of torch's fp32 dense autograd"


# (1, 1): contiguous ld = 1, the 4-byte path; (4, 4): ld = 4, the 16-byte path; all four new ones: one lane per row
GENERAL = [(24, 24, False), (8, 40, False), (64, 4, False), (6, 10, False), (6, 10, True),
           (1, 1, False), (4, 4, False), (3, 2, False), (2, 4, True)]
# scales that are no power of two (t and ds are rounded), one of them negative (the row maximum is the minimum of s)
GENERAL_CASES = [(name, k, kv, o, SCALE) for k, kv, o in GENERAL for name in ("odd_last_chunk", "wave_pipe_thresholds", "keys48")]
GENERAL_CASES += [(name, k, kv, False, scale) for scale in (0.3, -1.7) for k, kv in ((24, 24), (3, 2))
                  for name in ("wave_pipe_thresholds", "keys48")]


@pytest.mark.parametrize("name,k,kv,odd_ld,SCALE", GENERAL_CASES,
                         ids=[f"{n}-k{k}-kv{kv}{'-oddld' if o else ''}{'' if sc == SCALE else f'-scale{sc}'}"
                              for n, k, kv, o, sc in GENERAL_CASES])
def test_fused_attention_general_against_dense_autograd(pkg, oracle, gpu, name, k, kv, odd_ld, SCALE):
    import torch
    SCALE_REF = float(np.float32(SCALE))                       # what the kernel receives
    s = _general_structure(name, pkg, oracle)
    h = Handles(pkg, s, gpu)
    if name == "wave_pipe_thresholds":
        assert "long_rows=5 " in h.A.spmm_describe()                 # 513, 1024, 1025, 1028, 4100 go in pieces; 512 does not
    if name == "keys48":
        assert "long_rows=0 " in h.A.spmm_describe() and "long_rows=0 " not in h.T.spmm_describe()
    mask = _mask(s, gpu)
    Q, K, V, dO = _randn(gpu, len(name) + 64 * k + kv, (s.rows, k), (s.cols, k), (s.cols, kv), (s.rows, kv))
    ld = None
    ins = (Q, K, V, dO)
    if odd_ld:
        ld = lambda w: w + 1 if (w + 1) % 4 else w + 2       # noqa: E731
        ins = tuple(_strided(t, ld(t.shape[1])) for t in ins)
        assert all(t.stride(0) % 4 != 0 for t in ins)
    got = _run(h, *ins, SCALE, ld)
    if odd_ld:
        assert all(got[w].stride(0) % 4 != 0 for w in ("O", "dQ", "dK", "dV"))
    # the composed path on the same data, for the figures beside
    other = None
    if k == 24 and kv == 24 or odd_ld:
        att = pkg.sparse_attention.SparseAttention(s.rows, s.cols, h.keep[0], h.keep[1], scale=SCALE)
        Qc, Kc, Vc = (t.detach().clone().requires_grad_(True) for t in (Q, K, V))
        Oc = att(Qc, Kc, Vc)
        Oc.backward(dO)
        other = {"O": Oc.detach(), "dQ": Qc.grad, "dK": Kc.grad, "dV": Vc.grad}
        att.close()
    _check_general(f"{name} k={k} kv={kv}{' odd ld' if odd_ld else ''} scale={SCALE}", got, mask, SCALE_REF, Q, K, V, dO, other)
    L = torch.from_numpy(np.diff(s.rp)).to(gpu)
    assert bool((got["O"][L == 0] == 0).all()) and bool((got["dQ"][L == 0] == 0).all())
    assert bool((got["stats"][L == 0, 0] == float("-inf")).all()) and bool((got["stats"][L == 0, 1] == 0).all())
    h.close()


@pytest.mark.parametrize("scale", [0.0, -0.0], ids=["plus0", "minus0"])
def test_fused_attention_at_scale_zero(pkg, oracle, gpu, scale):
    """A scale of +0 or -0 is finite, so it is accepted: every p is 1 / L, O is the row mean of V, dQ = dK = 0."""
    import torch
    k, kv = 8, 12
    s = E.structure("wave_pipe_thresholds", pkg, oracle)
    h = Handles(pkg, s, gpu)
    assert "long_rows=5 " in h.A.spmm_describe()
    Q, K, V, dO = _randn(gpu, 97, (s.rows, k), (s.cols, k), (s.cols, kv), (s.rows, kv))
    got = _run(h, Q, K, V, dO, scale)
    assert bool((got["dQ"] == 0).all()) and bool((got["dK"] == 0).all())
    _check_general(f"scale={scale}", got, _mask(s, gpu), scale, Q, K, V, dO, whats=("O", "dV"))
    L = torch.from_numpy(np.diff(s.rp)).to(gpu)
    assert bool((got["stats"][L > 0, 0] == 0).all()) and bool((got["stats"][L == 0, 0] == float("-inf")).all())
    h.close()


# ---- masks -----------------------------------------------------------------------------------------------------------
def test_fused_attention_masked_keys_nan_rows_and_empty_rows(pkg, gpu):
    import torch
    rng = np.random.Generator(np.random.PCG64(17))
    cols, n_masked, k, kv = 400, 100, 8, 12                  # keys 0 .. 99 are masked; columns are sorted, so they come first
    kinds = rng.choice(4, size=600, p=[0.55, 0.25, 0.1, 0.1])  # 0 ordinary, 1 first 20 masked, 2 all masked, 3 empty
    kinds[:4] = (0, 1, 2, 3)
    parts = []
    for kind in kinds:
        lo = {0: 3, 1: 20, 2: 10, 3: 0}[kind]
        hi = {0: 5, 1: 4, 2: 0, 3: 0}[kind]           # (the finite entries of a row fall into one step of 8, see below)
        parts.append(np.concatenate([np.sort(rng.choice(n_masked, size=lo, replace=False)),
                                     n_masked + np.sort(rng.choice(cols - n_masked, size=hi, replace=False))]))
    rp = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    s = E.Structure(len(kinds), cols, rp, np.concatenate(parts).astype(np.int32))
    nan_row = int(np.flatnonzero(kinds == 0)[3])
    h = Handles(pkg, s, gpu)
    Q, K, V, dO = _randn(gpu, 23, (s.rows, k), (cols, k), (cols, kv), (s.rows, kv))
    Q[:, 0] = 1.0
    K_ref = K.clone()
    K_ref[:n_masked, 0] = 0.0
    K[:n_masked, 0] = float("-inf")
    Q[nan_row, 1] = float("nan")
    got = _run(h, Q, K, V, dO, SCALE)
    kinds_t = torch.from_numpy(kinds).to(gpu)
    bad_rows = (kinds_t == 2)
    bad_rows[nan_row] = True
    # fully masked rows and the NaN row are NaN throughout
    assert bool(got["O"][bad_rows].isnan().all()) and bool(got["dQ"][bad_rows].isnan().all())
    # empty rows: a zero row of O and no gradient
    assert bool((got["O"][kinds_t == 3] == 0).all()) and bool((got["dQ"][kinds_t == 3] == 0).all())
    # the keys a NaN row refers to carry its NaN; the others must not
    touched = torch.zeros(cols, dtype=torch.bool, device=gpu)
    for r in bad_rows.nonzero().flatten().tolist():
        touched[torch.from_numpy(s.ci[s.rp[r]:s.rp[r + 1]].astype(np.int64)).to(gpu)] = True
    assert bool(got["dV"][touched].isnan().all()) and bool(got["dK"][touched].isnan().all())
    assert not bool(got["dV"][~touched].isnan().any()) and not bool(got["dK"][~touched].isnan().any())
    # everything else: the dense autograd of the pattern without the masked entries (and without the NaN rows), finite K
    Qr = Q.clone()
    Qr[nan_row, 1] = 0.0
    keep = (s.ci >= n_masked) & ~np.isin(s.row_of, bad_rows.nonzero().flatten().cpu().numpy())
    mask = _mask(s, gpu, keep)
    good = ~bad_rows
    dq0 = got["dQ"][:, 0].clone()
    lists_masked = torch.from_numpy(np.isin(kinds, (0, 1))).to(gpu) & good
    assert bool(dq0[lists_masked].isnan().all()), "0 * -Inf is NaN by IEEE"
    fixed = dict(got)
    fixed["dQ"] = got["dQ"].clone()
    ref_dq = _dense_autograd(mask, SCALE, Qr, K_ref, V, dO, torch.float64)[1]
    fixed["dQ"][:, 0] = torch.where(lists_masked, ref_dq[:, 0].float(), dq0)        # (that column is checked above)
    assert bool(got["O"][good].isfinite().all()) and bool(fixed["dQ"][good].isfinite().all())
    _check_general("masks", fixed, mask, SCALE, Qr, K_ref, V, dO, rows=good, cols=~touched)
    # masked entries contribute exactly nothing: the same rows without their masked entries give the same bits of O
    keep_all = s.ci >= n_masked
    lengths2 = np.bincount(s.row_of[keep_all], minlength=s.rows)
    s2 = E.Structure(s.rows, cols, np.concatenate([[0], np.cumsum(lengths2)]).astype(np.int32), s.ci[keep_all])
    h2 = Handles(pkg, s2, gpu)
    got2 = _run(h2, Q, K, V, dO, SCALE)
    # (a row of kind 1 keeps its 4 finite entries: one step; with its 20 masked entries it takes three steps of 8 whose first
    # two are all -Inf and whose third holds the finite ones, so the documented order gives the same bits either way)
    live = good & (kinds_t != 3)
    assert bool((kinds_t[live] == 1).any())
    assert torch.equal(_bits(got["O"][live]), _bits(got2["O"][live]))
    assert torch.equal(_raw_bits(got["stats"][live]), _raw_bits(got2["stats"][live]))
    assert torch.equal(_bits(got["dQ"][live][:, 1:]), _bits(got2["dQ"][live][:, 1:]))
    is_masked = torch.arange(cols, device=gpu) < n_masked
    assert torch.equal(_bits(got["dV"][~touched & ~is_masked]), _bits(got2["dV"][~touched & ~is_masked]))
    assert torch.equal(_bits(got["dK"][~touched & ~is_masked]), _bits(got2["dK"][~touched & ~is_masked]))
    assert bool((got["dV"][~touched & is_masked] == 0).all()) and bool((got["dK"][~touched & is_masked] == 0).all())
    assert bool((~touched & is_masked).any())
    h.close()
    h2.close()


@pytest.mark.parametrize("k,kv", [(8, 12), (3, 4)], ids=["k8-kv12", "k3-kv4"])
def test_fused_attention_special_values_in_long_rows(pkg, gpu, k, kv):
    """The rows of _attention_rows.special_rows: masked stretches before and after the finite keys of rows in pieces, long
    rows that are masked entirely or hold a NaN or a +Inf, and keys 0 (masked), 1200 and 1201 that some 700 queries list,
    so the transposed handle runs them in pieces as well.  (3, 4) is one lane per row."""
    import torch
    kinds, lists = R.special_rows()
    cols = R.KEYS
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    s = E.Structure(len(lists), cols, rp, np.concatenate(lists).astype(np.int32))
    h = Handles(pkg, s, gpu)
    n_long = int((np.diff(rp) > 512).sum())
    assert n_long >= 20 and f"long_rows={n_long} " in h.A.spmm_describe()
    per_key = np.bincount(s.ci, minlength=cols)
    assert all(per_key[j] > 512 for j in (R.KEY_MASKED0, R.KEY_A, R.KEY_B))
    assert f"long_rows={int((per_key > 512).sum())} " in h.T.spmm_describe() and "long_rows=0 " not in h.T.spmm_describe()
    is_kind = lambda *names: torch.from_numpy(np.isin(kinds, names)).to(gpu)       # noqa: E731
    is_masked = torch.from_numpy(R.is_masked_key(np.arange(cols))).to(gpu)
    Q, K, V, dO = _randn(gpu, 101 + k, (s.rows, k), (cols, k), (cols, kv), (s.rows, kv))
    Q[:, 0] = 1.0
    Q[:, 1] = 1.0
    K_ref = K.clone()
    K_ref[is_masked, 0] = 0.0
    K_ref[R.KEY_INF, 1] = 0.0
    K[is_masked, 0] = float("-inf")
    K[R.KEY_INF, 1] = float("inf")
    Qr = Q.clone()
    Q[is_kind(*R.Q_NAN_KINDS), 2] = float("nan")
    got = _run(h, Q, K, V, dO, SCALE)
    bad_rows, good = is_kind(*R.NAN_KINDS), ~is_kind(*R.NAN_KINDS)
    for kind in R.NAN_KINDS:
        assert bool(got["O"][is_kind(kind)].isnan().all()) and bool(got["dQ"][is_kind(kind)].isnan().all()), kind
    # a row masked entirely, long or short: l = 0, so stats = (-Inf, 1.0f / 0 = +Inf)
    assert bool((got["stats"][is_kind("all_masked"), 0] == float("-inf")).all())
    assert bool((got["stats"][is_kind("all_masked"), 1] == float("inf")).all())
    assert bool((got["O"][is_kind("empty")] == 0).all()) and bool((got["dQ"][is_kind("empty")] == 0).all())
    # the keys a NaN row refers to carry its NaN; the others must not
    touched_np = np.zeros(cols, bool)
    touched_np[np.concatenate([lists[r] for r in np.flatnonzero(np.isin(kinds, R.NAN_KINDS))])] = True
    assert touched_np[R.KEY_B] and touched_np[R.KEY_INF] and not touched_np[R.KEY_A] and not touched_np[R.KEY_MASKED0]
    touched = torch.from_numpy(touched_np).to(gpu)
    assert bool(got["dV"][touched].isnan().all()) and bool(got["dK"][touched].isnan().all())
    assert not bool(got["dV"][~touched].isnan().any()) and not bool(got["dK"][~touched].isnan().any())
    # a masked key contributes nothing, also through the pieces of the transposed handle and their sum (key 0)
    assert bool((~touched & is_masked).sum() > 100)
    assert bool((got["dV"][~touched & is_masked] == 0).all()) and bool((got["dK"][~touched & is_masked] == 0).all())
    assert bool((got["dV"][R.KEY_MASKED0] == 0).all()) and bool((got["dK"][R.KEY_MASKED0] == 0).all())
    # everything else: the dense autograd of the pattern without the masked entries (and without the NaN rows), finite K
    keep = ~R.is_masked_key(s.ci) & ~np.isin(kinds, R.NAN_KINDS)[s.row_of]
    mask = _mask(s, gpu, keep)
    lists_masked = torch.from_numpy(np.array([bool(R.is_masked_key(l).any()) for l in lists])).to(gpu) & good
    assert bool(lists_masked[is_kind(*R.BIT_KINDS, "straddle", "shared", "ordinary")].all())
    dq0 = got["dQ"][:, 0].clone()
    assert bool(dq0[lists_masked].isnan().all()), "0 * -Inf is NaN by IEEE"
    fixed = dict(got)
    fixed["dQ"] = got["dQ"].clone()
    ref_dq = _dense_autograd(mask, SCALE, Qr, K_ref, V, dO, torch.float64)[1]
    fixed["dQ"][:, 0] = torch.where(lists_masked, ref_dq[:, 0].float(), dq0)        # (that column is checked above)
    assert bool(got["O"][good].isfinite().all()) and bool(fixed["dQ"][good].isfinite().all())
    assert bool((~touched)[R.KEY_A])                                                 # key 1200: a long transposed row, compared
    _check_general(f"special k={k} kv={kv}", fixed, mask, SCALE, Qr, K_ref, V, dO, rows=good, cols=~touched)
    # masked stretches contribute exactly nothing: the same rows without their masked entries give the same bits
    keep_all = ~R.is_masked_key(s.ci)
    lengths2 = np.bincount(s.row_of[keep_all], minlength=s.rows)
    s2 = E.Structure(s.rows, cols, np.concatenate([[0], np.cumsum(lengths2)]).astype(np.int32), s.ci[keep_all])
    h2 = Handles(pkg, s2, gpu)
    got2 = _run(h2, Q, K, V, dO, SCALE)
    # (a leading stretch of 512 or 1024 masked entries is one or two whole pieces, (m, l, acc) = (-Inf, 0, 0) with w = 0, and
    # the finite entries keep their piece boundaries; 512 finite entries are one piece with w = expf(0) = 1 or, alone, a row
    # of one span; trailing masked entries in a piece add e = 0.  An ordinary row is one step of 8 either way.)
    for kind in R.BIT_KINDS + ("ordinary",):
        live = is_kind(kind)
        assert bool(live.any())
        assert torch.equal(_bits(got["O"][live]), _bits(got2["O"][live])), kind
        assert torch.equal(_raw_bits(got["stats"][live]), _raw_bits(got2["stats"][live])), kind
        assert torch.equal(_bits(got["dQ"][live][:, 1:]), _bits(got2["dQ"][live][:, 1:])), kind
    h.close()
    h2.close()


# ---- invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kv", [(12, 20), (3, 2)], ids=["k12-kv20", "k3-kv2"])
def test_fused_attention_rows_do_not_depend_on_their_placement(pkg, gpu, k, kv):
    """(3, 2) is one lane per row: there placement changes a lane's neighbours in its wavefront, and the contiguous operands
    (ld = 3 and 2) already take the 4-byte path, so "strided operands" is its 16-byte run."""
    import torch
    cols = 900
    rng = np.random.Generator(np.random.PCG64(29))
    lengths = np.concatenate([[1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 511, 512, 513, 700], rng.integers(1, 701, size=26)])
    assert len(lengths) == 40
    lists = [np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lengths]
    Qs, dOs = _randn(gpu, 31, (40, k), (40, kv))
    K, V = _randn(gpu, 32, (cols, k), (cols, kv))

    def placement(filler_len, gap):
        """The 40 rows, `gap` filler rows of `filler_len` entries before each; returns (structure, positions)."""
        parts, pos = [], []
        for l in lists:
            for _ in range(gap):
                parts.append(np.sort(rng.choice(cols, size=filler_len, replace=False)))
            pos.append(len(parts))
            parts.append(l)
        rp = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
        return E.Structure(len(parts), cols, rp, np.concatenate(parts).astype(np.int32)), np.array(pos)

    def run(s, pos, strided=False, odd=False):
        h = Handles(pkg, s, gpu)
        Q, dO = _randn(gpu, 33 + s.rows, (s.rows, k), (s.rows, kv))
        at = torch.from_numpy(pos).to(gpu)
        Q[at], dO[at] = Qs, dOs
        ins, ld = (Q, K, V, dO), None
        if strided:
            ld = (lambda w: w + 5 if (w + 5) % 4 else w + 6) if odd else (lambda w: (w + 11) // 4 * 4)
            ins = tuple(_strided(t, ld(t.shape[1])) for t in ins)
            assert all((t.stride(0) % 4 != 0) == odd for t in ins)
        got = _run(h, *ins, SCALE, ld)
        h.close()
        return {w: got[w][at].contiguous() for w in ("O", "stats", "dQ")}

    base = run(*placement(3, 5))
    block = E.Structure(40, cols, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), np.concatenate(lists).astype(np.int32))
    for tag, other in (("among rows of 300", run(*placement(300, 2))),
                       ("a row block with a rebased row_ptr", run(block, np.arange(40))),
                       ("strided operands", run(*placement(3, 5), strided=True)),
                       ("the 4-byte load path", run(*placement(3, 5), strided=True, odd=True))):
        for w in ("O", "stats", "dQ"):
            assert torch.equal(_raw_bits(base[w]), _raw_bits(other[w])), f"{w} differs {tag}"


# ---- extreme score profiles ------------------------------------------------------------------------------------------
def _check_with_floor(tag, got, mask, scale, Q, K, V, dO, floor):
    """_check_general's rule with an absolute floor: |error| <= max(4 x yard, RTOL) x magnitude + floor, the yardstick's error
    taken beyond the same floor.  For rows whose probabilities underflow: their magnitudes go down to 1e-84, and the device's
    fp64 softmax returns 0 for a probability below fp32's normal range (seen: exp(-88) = 6e-39 comes out as 0), where the
    kernels keep a subnormal.  So at magnitude 0 the rule is the floor alone, not an exact zero."""
    import torch
    *r64, P = _dense_autograd(mask, scale, Q, K, V, dO, torch.float64)
    r64 = dict(zip(("O", "dQ", "dK", "dV"), r64))
    r32 = dict(zip(("O", "dQ", "dK", "dV"), _dense_autograd(mask, scale, Q, K, V, dO, torch.float32)))
    mags = _normalised(mask, scale, Q, K, V, dO, P)
    for what in ("O", "dQ", "dK", "dV"):
        g, g64, g32, mag = got[what], r64[what], r32[what], mags[what]
        assert bool(g.isfinite().all()), f"{tag} {what}: not finite"
        live = mag > 0
        assert bool(live.any())
        assert bool((g[~live].abs() <= floor).all()), f"{tag} {what}: a value beyond the floor where nothing contributes"
        beyond = lambda x: ((x.double() - g64).abs()[live] - floor).clamp(min=0) / mag[live]      # noqa: E731
        ours, yard = float(beyond(g).max()), float(beyond(g32).max())
        print(f"{tag} {what}: normalised error beyond 2^-90 fused {ours:.3g}, torch fp32 dense autograd {yard:.3g}")
        assert ours <= max(4.0 * yard, RTOL), f"{tag} {what}: {ours:.3g} against {yard:.3g} of torch's fp32 dense autograd"


@pytest.mark.parametrize("k,kv", [(2, 1), (2, 40)], ids=["k2-kv1", "k2-kv40"])
def test_fused_attention_extreme_score_profiles(pkg, gpu, k, kv):
    """The rows of _attention_rows.extreme_rows, every score exact: maxima that rise at every step (a = expf(m - z) down to
    0, where (l, acc) restart) or fall, a spike of 200 as the last entry (at 513 the single nonzero of the last piece) or
    the first, 0 and -200 in turn, scores near 256.  (2, 1): one lane, steps of 8; (2, 40): 16 lanes, steps of 16."""
    import torch
    rows, cols = R.extreme_rows()
    lengths = [n for _, n, _, _ in rows]
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    s = E.Structure(len(rows), cols, rp, np.arange(cols, dtype=np.int32))         # row r owns the keys [rp[r], rp[r + 1])
    assert [first for _, _, first, _ in rows] == rp[:-1].tolist()
    h = Handles(pkg, s, gpu)
    assert f"long_rows={sum(n > 512 for n in lengths)} " in h.A.spmm_describe() and "long_rows=0 " in h.T.spmm_describe()
    Q, K, V, dO = _randn(gpu, 103 + kv, (s.rows, k), (cols, k), (cols, kv), (s.rows, kv))
    Q[:, 0], Q[:, 1] = 1.0, 0.0
    t = torch.from_numpy(np.concatenate([t for _, _, _, t in rows])).to(gpu)
    K[:, 0] = (t / R.EXTREME_SCALE).float()
    assert torch.equal(K[:, 0].double() * R.EXTREME_SCALE, t)
    got = _run(h, Q, K, V, dO, R.EXTREME_SCALE)
    S = torch.empty(s.nnz, dtype=torch.float32, device=gpu)
    h.A.sddmm(Q, K, S)
    assert torch.equal(S.double() * R.EXTREME_SCALE, t), "the scores are not exact"
    want_max = torch.tensor([float(t.max()) for _, _, _, t in rows], dtype=torch.float32, device=gpu)
    assert torch.equal(got["stats"][:, 0], want_max)
    _check_with_floor(f"extreme k={k} kv={kv}", got, _mask(s, gpu), R.EXTREME_SCALE, Q, K, V, dO, R.ABS_FLOOR)
    h.close()


# ---- heads -----------------------------------------------------------------------------------------------------------
def test_fused_attention_heads_as_column_blocks_without_a_copy(pkg, gpu, monkeypatch):
    import torch
    s = _rows_pattern(np.random.Generator(np.random.PCG64(41)).integers(0, 30, size=700), 500, 43)
    heads, k = 3, 8
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    att = pkg.sparse_attention.FusedSparseAttention(s.rows, s.cols, d_rp, d_ci, scale=SCALE)
    Qf, Kf, Vf, dOf = _randn(gpu, 47, (s.rows, heads * k), (s.cols, heads * k), (s.cols, heads * k), (s.rows, heads * k))
    split = lambda t: t.view(t.shape[0], heads, k).transpose(0, 1)         # noqa: E731  (heads, n, k), strides (k, heads k, 1)
    seen = []
    real = pkg.capi.CsrMatrix.attention_forward
    monkeypatch.setattr(pkg.capi.CsrMatrix, "attention_forward",
                        lambda self, Q, K, V, *a, **kw: (seen.append((Q.data_ptr(), K.data_ptr(), V.data_ptr())), real(self, Q, K, V, *a, **kw))[1])
    Q3, K3, V3 = (split(t).requires_grad_(True) for t in (Qf, Kf, Vf))
    O3 = att(Q3, K3, V3)
    O3.backward(split(dOf))
    torch.cuda.synchronize()
    assert seen == [(Qf.data_ptr() + 4 * k * h, Kf.data_ptr() + 4 * k * h, Vf.data_ptr() + 4 * k * h) for h in range(heads)]
    assert O3.shape == (heads, s.rows, k)
    for h in range(heads):
        q, kk, v = (t[:, h * k:(h + 1) * k].clone().requires_grad_(True) for t in (Qf, Kf, Vf))
        o = att(q, kk, v)
        o.backward(dOf[:, h * k:(h + 1) * k])
        torch.cuda.synchronize()
        for got, want in ((O3[h].detach(), o.detach()), (Q3.grad[h], q.grad), (K3.grad[h], kk.grad), (V3.grad[h], v.grad)):
            assert torch.equal(_raw_bits(got), _raw_bits(want)), f"head {h}"
    att.close()


# ---- memory ----------------------------------------------------------------------------------------------------------
def test_fused_attention_step_allocates_less_than_one_array_of_nnz_floats(pkg, gpu):
    import torch
    rows = cols = 2000
    s = _rows_pattern([128] * rows, cols, 53)
    cap = 4 * s.nnz
    assert s.nnz == 256_000 and cap == 1_024_000
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    Q, K, V, dO = _randn(gpu, 59, (rows, 8), (cols, 8), (cols, 8), (rows, 8))

    def step_bytes(att):
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        att(q, k, v).backward(dO)                         # warm-up
        q.grad = k.grad = v.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        att(q, k, v).backward(dO)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    fused = pkg.sparse_attention.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=SCALE)
    composed = pkg.sparse_attention.SparseAttention(rows, cols, d_rp, d_ci, scale=SCALE)
    got, ref = step_bytes(fused), step_bytes(composed)
    print(f"one step: fused {got} bytes, composed {ref} bytes, 4 nnz = {cap}")
    assert got < cap, f"the fused step allocates {got} bytes, 4 nnz = {cap}"
    assert ref > cap, "the composed path was expected to keep an array of nnz floats"
    fused.close()
    composed.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------
def test_fused_attention_is_graph_capturable(pkg, oracle, gpu):
    import torch
    s = E.structure("wave_pipe_thresholds", pkg, oracle)
    h = Handles(pkg, s, gpu)
    k, kv = 16, 24
    data = [_randn(gpu, 61 + i, (s.rows, k), (s.cols, k), (s.cols, kv), (s.rows, kv)) for i in range(3)]
    eager = [_run(h, *d, SCALE) for d in data]
    Q, K, V, dO = (t.clone() for t in data[0])
    made = [_guarded(gpu, n, w) for n, w in ((s.rows, kv), (s.rows, 2), (s.rows, 1), (s.rows, k), (s.cols, k), (s.cols, kv))]
    O, stats, delta, dQ, dK, dV = (o for _, o in made)
    delta = delta.reshape(-1)
    torch.cuda.synchronize()                                 # (every kernel has run once before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # (one capture stream; the calls take the current stream)
        h.A.attention_forward(Q, K, V, O, stats, SCALE)
        h.A.attention_backward_q(Q, K, V, O, dO, stats, delta, dQ, SCALE)
        h.T.attention_backward_kv(Q, K, V, dO, stats, delta, dK, dV, SCALE)
    for i in (1, 2):
        for dst, src in zip((Q, K, V, dO), data[i]):
            dst.copy_(src)
        for _, o in made:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for w, t in (("O", O), ("stats", stats), ("delta", delta), ("dQ", dQ), ("dK", dK), ("dV", dV)):
            assert torch.equal(_raw_bits(t), _raw_bits(eager[i][w])), f"replay {i}: {w} differs from the eager run"
    assert all(_intact(buf, o.shape[0], o.shape[1], o.shape[1]) for buf, o in made)
    h.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_fused_attention_refusals_launch_nothing(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    s = _rows_pattern([5] * 64, 40, 67)
    h = Handles(pkg, s, gpu)
    unplanned = Handles(pkg, s, gpu, plan=False)
    wide = lambda n: torch.ones((n, 72), dtype=torch.float32, device=gpu)       # noqa: E731
    Q, K, V, dO, O_in = wide(s.rows), wide(s.cols), wide(s.cols), wide(s.rows), wide(s.rows)
    stats_in, delta_in = torch.zeros((s.rows, 2), device=gpu), torch.zeros(s.rows, device=gpu)
    outs = {n: torch.full((r, 72), 7.0, dtype=torch.float32, device=gpu) for n, r in
            (("O", s.rows), ("dQ", s.rows), ("dK", s.cols), ("dV", s.cols), ("stats", s.rows), ("delta", s.rows))}
    st = capi._stream_handle()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)       # noqa: E731

    def call(which, hd, scale=1.0, k=8, kv=8, ld=72, off=None):
        """One call with every ld = `ld`; off = (operand name, bytes) shifts that pointer."""
        o = lambda name, t: p(t, off[1] if off and off[0] == name else 0)      # noqa: E731
        if which == "forward":
            return lib.spmv_csr_attention_forward(hd._h, scale, k, o("Q", Q), ld, o("K", K), ld, kv, o("V", V), ld,
                                                  o("O", outs["O"]), ld, o("stats", outs["stats"]), st)
        if which == "backward_q":
            return lib.spmv_csr_attention_backward_q(hd._h, scale, k, o("Q", Q), ld, o("K", K), ld, kv, o("V", V), ld,
                                                     o("O", O_in), ld, o("dO", dO), ld, o("stats", stats_in),
                                                     o("delta", outs["delta"]), o("dQ", outs["dQ"]), ld, st)
        return lib.spmv_csr_attention_backward_kv(hd._h, scale, k, o("Q", Q), ld, o("K", K), ld, kv, o("V", V), ld,
                                                  o("dO", dO), ld, o("stats", stats_in), o("delta", delta_in),
                                                  o("dK", outs["dK"]), ld, o("dV", outs["dV"]), ld, st)

    handle = {"forward": h.A, "backward_q": h.A, "backward_kv": h.T}
    for which, hd in handle.items():
        name = f"spmv_csr_attention_{which}"
        cases = [dict(k=0), dict(k=65), dict(kv=0), dict(kv=65), dict(k=8, kv=8, ld=7), dict(k=12, kv=8, ld=11),
                 dict(off=("Q", 4)), dict(off=("V", 8)), dict(scale=float("inf")), dict(scale=float("nan"))]
        cases.append(dict(off=("O" if which == "forward" else "dQ" if which == "backward_q" else "dV", 4)))
        for kw in cases:
            assert call(which, hd, **kw) == capi.ERR_INVALID, f"{which} {kw}"
            assert lib.spmv_last_error().decode().startswith(name + ":"), lib.spmv_last_error()
        missing = unplanned.T if which == "backward_kv" else unplanned.A
        assert call(which, missing) == capi.ERR_NOT_PLANNED
        assert name in lib.spmv_last_error().decode()
    # a transposed handle of the wrong shape: the Python binding checks the operands against the handle it is given
    q, kk, v = torch.ones((s.rows, 8), device=gpu), torch.ones((s.cols, 8), device=gpu), torch.ones((s.cols, 8), device=gpu)
    with pytest.raises(ValueError):
        h.A.attention_backward_kv(q, kk, v, q, stats_in, delta_in, outs["dK"][:, :8], outs["dV"][:, :8])
    with pytest.raises(ValueError):
        h.T.attention_forward(q, kk, v, outs["O"][:, :8], outs["stats"][:, :2].contiguous())
    with pytest.raises(ValueError):
        h.A.attention_forward(q, kk, v, outs["O"][:, :8], outs["stats"][:, :2].contiguous(), float("inf"))
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs.values()), "a refused call wrote to an output"
    # the holder refuses what the composed holder refuses
    att = pkg.sparse_attention.FusedSparseAttention(s.rows, s.cols, h.keep[0], h.keep[1])
    z = lambda r, c: torch.zeros((r, c), dtype=torch.float32, device=gpu)       # noqa: E731
    for a, b, c in ((z(s.rows, 65), z(s.cols, 65), z(s.cols, 8)), (z(s.rows, 8), z(s.cols, 8), z(s.cols, 65)),
                    (z(s.rows + 1, 8), z(s.cols, 8), z(s.cols, 8)), (z(s.rows, 8), z(s.cols, 4), z(s.cols, 8)),
                    (z(s.rows, 8).double(), z(s.cols, 8), z(s.cols, 8)), (z(s.rows, 8), z(s.cols, 8), torch.zeros((3, s.cols, 8), device=gpu))):
        with pytest.raises(ValueError):
            att(a, b, c)
    with pytest.raises(ValueError):
        pkg.sparse_attention.FusedSparseAttention(s.rows, s.cols, h.keep[0], h.keep[1], scale=float("nan"))
    att.close()
    h.close()
    unplanned.close()
