"""The documented order of the sums, on the device, bit for bit (include/spmv_hip.h: "the order of the sums is part of the
interface" for SpMM, SDDMM, the row softmax and the fused attention passes with their _heads and _gqa forms).

Every test runs a kernel on general data (standard normal floats, so that the order of the additions decides the last bit)
and compares every output value with the numpy statement of the documented order in tests/_attention_order.py: raw bits with
+0 and -0 folded, no tolerance, nothing left out.  The other GPU tests cannot see a wrong order: exact data gives the same
bits in any order, a tolerance admits any order at fp32 precision, and invariance compares a kernel with itself.
tests/test_attention_order_host.py shows on these very inputs that a reversed storage order, pieces added last to first, a
sequential sum in place of the butterfly, an unfused multiply-add and a GQA fold from +0 each change bits.

Patterns and data: tests/_order_cases.py.  P1 has unsorted rows with repeated keys, rows that list one key up to 513
times, lengths on both sides of every step and piece boundary, and a transpose whose 40 rows all go in pieces; P2 is
shuffled with duplicates and has short transposed rows.

spmm        Y[i][c]: the fma chain in storage order from +0, pieces of 512 added in piece order from +0; k = 1, 13, 64.
sddmm       out[n]: four-column lane partials, then the xor butterfly; k = 1, 3, 4, 13, 24, 40, 64.
softmax     row_softmax_backward's dS[n]: 64 strided partials, the butterfly, the pieces, then three roundings; scales 1,
            0.3 and -0.7.
attention   the three fused passes at (k, kv) = (4, 4) (one lane), (16, 12), (8, 40) (kv > k: T comes from kv), (64, 20)
            and (6, 10) (the 4-byte load path), and (16, 12) again with every ld % 4 != 0, on the five data sets of
            _order_cases: O, stats, delta, dQ, dK and dV (the stats_* sets: delta, dQ, dK, dV from caller-made O, stats and
            delta; maxima: the forward pass and backward_q).
gqa         four query heads on two K/V heads with the caller-made-stats data: dK_c and dV_c are the fold of two single-head
            emulations in head order from head 0's value, O-side outputs the single-head ones; group = 1 (the _heads call on
            expanded K, V) gives the unfolded emulations.  On P1 every transposed row is added from +0 in piece order, so no
            gradient is -0 there and a fold from +0 would give the same bits; on P2 one key's gradients are -0 in every head
            (products that underflow), and there dK_c and dV_c are compared without folding the zeros.

Not here: spmv_csr_row_softmax and the fused forward pass on general scores.  Their bits depend on the device library's
expf, of which the header promises 1 ulp and not the correctly rounded value, and the host cannot reproduce that.  The fused
passes are therefore run on data whose every expf argument is +-0, at most -128 or -Inf (e and alpha are then exactly 1 or
0 under any expf of 1 ulp; the host test asserts the premise), which leaves the multipliers of the forward chains at 0 or
1: the forward pass is pinned as a chain of additions, its rescale and combine by the maxima data, and the multiply-add
chains by the backward passes, where p = r_i is a general number.  tests/test_gpu_attention_multigraph.py covers the live
expf within a tolerance.
"""
import numpy as np
import pytest

import _attention_order as AO
import _order_cases as OC

pytestmark = pytest.mark.gpu

GUARD, GUARD_N = 3.0e35, 4096
f32 = np.float32


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


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


class Outputs:
    """NaN-filled outputs between guard bands; check() asserts the bands and the guard columns are untouched."""

    def __init__(self, gpu, ld=None):
        self.gpu, self.ld, self.made = gpu, ld, []

    def matrix(self, rows, w, wide=True):
        ld = self.ld(w) if self.ld and wide else w
        buf, out = _guarded(self.gpu, rows, w, ld)
        self.made.append((buf, rows, w, ld))
        return out

    def heads(self, heads, rows, w):
        return self.matrix(heads * rows, w, wide=False).view(heads, rows, w)

    def check(self):
        import torch
        torch.cuda.synchronize()
        assert all(_intact(*m) for m in self.made), "a kernel wrote outside its output"


def _strided(t, ld):
    """A copy of t with leading dimension ld; the columns past its width hold NaN."""
    import torch
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float32, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _folded(a):
    return (np.ascontiguousarray(a, f32) + f32(0)).view(np.uint32)


def _same_bits(tag, got, want, fold=True):
    """Every value of `got` (a device tensor) has the bits of `want` (numpy); returns how many were compared."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, tag
    g, w = (_folded(got), _folded(want)) if fold else (np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    bad = np.flatnonzero((g != w).reshape(-1))
    if bad.size:
        n = int(bad[0])
        raise AssertionError(f"{tag}: {bad.size} of {g.size} values differ from the documented order in a bit; the first at flat index "
                             f"{n}: {got.reshape(-1)[n]!r} ({g.reshape(-1)[n]:#010x}) against {want.reshape(-1)[n]!r} ({w.reshape(-1)[n]:#010x})")
    return int(g.size)


class Handles:
    def __init__(self, pkg, s, gpu, vals=None, heads=1, transposed=True):
        import torch
        v = torch.zeros(s.nnz, dtype=torch.float32, device=gpu) if vals is None else _dev(gpu, vals)
        self.keep = (_dev(gpu, s.rp), _dev(gpu, s.ci), v)
        self.A = pkg.capi.CsrMatrix.from_device(s.rows, s.cols, *self.keep)
        self.T = self.A.transpose(keep_map=False) if transposed else None
        for h in (self.A, self.T):
            if h is not None:
                h.attention_plan_heads(heads)
        self.tp, self.ti = AO.transpose_pattern(s.rows, s.cols, s.rp, s.ci)
        if transposed:
            # the emulation walks the transposed rows in the order spmv_csr_transpose gives them
            rp_t, ci_t, _ = self.T.download()
            assert np.array_equal(rp_t, self.tp) and np.array_equal(ci_t, self.ti)

    def close(self):
        if self.T is not None:
            self.T.close()
        self.A.close()


# ---- SpMM, SDDMM, softmax backward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("P1", 1), ("P1", 13), ("P1", 64), ("P2", 13)])
def test_spmm_has_the_documented_order(pkg, gpu, name, k):
    s, vals, X = OC.spmm_data(name, k)
    h = Handles(pkg, s, gpu, vals, transposed=False)
    assert ("long_rows=0 " not in h.A.spmm_describe())
    out = Outputs(gpu)
    Y = out.matrix(s.rows, k)
    h.A.spmm(_dev(gpu, X), Y)
    out.check()
    n = _same_bits(f"spmm {name} k={k}", Y, AO.spmm(s.rp, s.ci, vals, X))
    print(f"spmm {name} k={k}: {n} values compared bit for bit")
    h.close()


@pytest.mark.parametrize("name,k", [("P1", k) for k in (1, 3, 4, 13, 24, 40, 64)] + [("P2", 13)])
def test_sddmm_has_the_documented_order(pkg, gpu, name, k):
    s, U, X = OC.sddmm_data(name, k)
    h = Handles(pkg, s, gpu, transposed=False)
    out = Outputs(gpu)
    got = out.matrix(1, s.nnz).reshape(-1)
    h.A.sddmm(_dev(gpu, U), _dev(gpu, X), got)
    out.check()
    n = _same_bits(f"sddmm {name} k={k}", got, AO.sddmm(s.rp, s.ci, U, X))
    print(f"sddmm {name} k={k}: {n} values compared bit for bit")
    h.close()


@pytest.mark.parametrize("name", ["P1", "P2"])
@pytest.mark.parametrize("scale", [1.0, 0.3, -0.7])
def test_softmax_backward_has_the_documented_order(pkg, gpu, name, scale):
    s, P, dP = OC.softmax_data(name)
    h = Handles(pkg, s, gpu, transposed=False)
    out = Outputs(gpu)
    dS = out.matrix(1, s.nnz).reshape(-1)
    h.A.row_softmax_backward(_dev(gpu, P), _dev(gpu, dP), dS, scale)
    out.check()
    n = _same_bits(f"softmax backward {name} scale={scale}", dS, AO.softmax_backward(s.rp, P, dP, scale))
    print(f"softmax backward {name} scale={scale}: {n} values compared bit for bit")
    h.close()


# ---- fused attention -----------------------------------------------------------------------------------------------------
def emulate(s, tp, ti, case, d, wrong=None, rows=None, keys=None):
    """What the passes must give on data set d of `case`: a dict over the arrays the test compares."""
    Q, K, V, dO, scale = d["Q"], d["K"], d["V"], d["dO"], d["scale"]
    want = {}
    if case.startswith("stats"):
        O, stats, delta_in = d["O"], d["stats"], d["delta"]
    else:
        O, stats = AO.attention_forward(s.rp, s.ci, Q, K, V, scale, wrong, rows)
        want["O"], want["stats"] = O, stats
    want["dQ"], want["delta"] = AO.attention_backward_q(s.rp, s.ci, Q, K, V, O, dO, stats, scale, wrong, rows)
    if case != "maxima":
        delta_in = d["delta"] if case.startswith("stats") else want["delta"]
        want["dK"], want["dV"] = AO.attention_backward_kv(tp, ti, Q, K, V, dO, stats, delta_in, scale, wrong, keys)
    return want


FUSED = [("P1", case, k, kv, False) for case in OC.CASES for k, kv in OC.GEOMETRIES]
FUSED += [("P1", case, 16, 12, True) for case in OC.CASES]
FUSED += [("P2", case, 8, 40, False) for case in ("q0", "stats_k0")]


@pytest.mark.parametrize("name,case,k,kv,odd_ld", FUSED, ids=[f"{n}-{c}-k{k}-kv{kv}{'-oddld' if o else ''}" for n, c, k, kv, o in FUSED])
def test_fused_attention_has_the_documented_order(pkg, gpu, name, case, k, kv, odd_ld):
    s = OC.pattern(name)
    d = OC.attention_data(name, case, k, kv)
    h = Handles(pkg, s, gpu)
    if name == "P1":
        assert f"long_rows={s.cols} " in h.T.spmm_describe(), "every transposed row of P1 goes in pieces"
    ld = (lambda w: w + 1 if (w + 1) % 4 else w + 2) if odd_ld else None
    put = (lambda a: _strided(_dev(gpu, a), ld(a.shape[1]))) if odd_ld else (lambda a: _dev(gpu, a))
    Q, K, V, dO = (put(d[n]) for n in ("Q", "K", "V", "dO"))
    if odd_ld:
        assert all(t.stride(0) % 4 != 0 for t in (Q, K, V, dO))
    out = Outputs(gpu, ld)
    scale = d["scale"]
    got = {}
    if case.startswith("stats"):
        O, stats = put(d["O"]), _dev(gpu, d["stats"])
    else:
        O, stats = out.matrix(s.rows, kv), out.matrix(s.rows, 2, False)
        h.A.attention_forward(Q, K, V, O, stats, scale)
        got["O"], got["stats"] = O, stats
    got["delta"], got["dQ"] = out.matrix(s.rows, 1, False).reshape(-1), out.matrix(s.rows, k)
    h.A.attention_backward_q(Q, K, V, O, dO, stats, got["delta"], got["dQ"], scale)
    if case != "maxima":
        got["dK"], got["dV"] = out.matrix(s.cols, k), out.matrix(s.cols, kv)
        delta_in = _dev(gpu, d["delta"]) if case.startswith("stats") else got["delta"]
        h.T.attention_backward_kv(Q, K, V, dO, stats, delta_in, got["dK"], got["dV"], scale)
    out.check()
    want = emulate(s, h.tp, h.ti, case, d)
    assert set(want) == set(got)
    counts = {w: _same_bits(f"{name} {case} k={k} kv={kv}{' odd ld' if odd_ld else ''}: {w}", got[w], want[w])
              for w in ("O", "stats", "delta", "dQ", "dK", "dV") if w in want}
    print(f"fused attention {name} {case} k={k} kv={kv}{' odd ld' if odd_ld else ''}: values compared bit for bit: "
          + ", ".join(f"{w} {n}" for w, n in counts.items()))
    h.close()


# ---- the _heads and _gqa forms ---------------------------------------------------------------------------------------------
HEADS, GROUP = 4, 2
GQA = [("P1", "stats_k0", 16, 12, False), ("P1", "stats_q0", 8, 40, False), ("P2", "stats_k0", 16, 12, True)]


def gqa_data(name, case, k, kv, minus_zero):
    """Per query head Q, dO, O, stats and delta of attention_data(head = h); K and V of K/V head c from head = c."""
    per = [OC.attention_data(name, case, k, kv, head=h, minus_zero=minus_zero) for h in range(HEADS)]
    return per, [per[c]["K"] for c in range(HEADS // GROUP)], [per[c]["V"] for c in range(HEADS // GROUP)]


def gqa_emulate(s, tp, ti, per, Ks, Vs, wrong=None, rows=None, keys=None):
    """Per query head (dQ, delta, dK, dV) of the single-head emulation with K, V of head h // GROUP."""
    single = []
    for hq, d in enumerate(per):
        K, V = Ks[hq // GROUP], Vs[hq // GROUP]
        dQ, delta = AO.attention_backward_q(s.rp, s.ci, d["Q"], K, V, d["O"], d["dO"], d["stats"], d["scale"], wrong, rows)
        dK, dV = AO.attention_backward_kv(tp, ti, d["Q"], K, V, d["dO"], d["stats"], d["delta"], d["scale"], wrong, keys)
        single.append(dict(dQ=dQ, delta=delta, dK=dK, dV=dV))
    return single


@pytest.mark.parametrize("name,case,k,kv,minus_zero", GQA, ids=[f"{n}-{c}-k{k}-kv{kv}" for n, c, k, kv, _ in GQA])
def test_gqa_folds_the_heads_in_the_documented_order(pkg, gpu, name, case, k, kv, minus_zero):
    import torch
    s = OC.pattern(name)
    per, Ks, Vs = gqa_data(name, case, k, kv, minus_zero)
    scale = per[0]["scale"]
    h = Handles(pkg, s, gpu, heads=HEADS)
    stack = lambda arrays: _dev(gpu, np.stack(arrays))           # noqa: E731
    Q, dO, O, stats, delta_in = (stack([d[n] for d in per]) for n in ("Q", "dO", "O", "stats", "delta"))
    K2, V2 = stack(Ks), stack(Vs)
    single = gqa_emulate(s, h.tp, h.ti, per, Ks, Vs)
    fold = lambda w, c: AO.gqa_fold([single[c * GROUP + i][w] for i in range(GROUP)])       # noqa: E731
    # grouped: four query heads on two K/V heads
    out = Outputs(gpu)
    delta, dQ = out.heads(HEADS, s.rows, 1).view(HEADS, s.rows), out.heads(HEADS, s.rows, k)
    dK, dV = out.heads(HEADS // GROUP, s.cols, k), out.heads(HEADS // GROUP, s.cols, kv)
    h.A.attention_backward_q_gqa(Q, K2, V2, O, dO, stats, delta, dQ, scale)
    h.T.attention_backward_kv_gqa(Q, K2, V2, dO, stats, delta_in, dK, dV, scale)
    out.check()
    n = 0
    for hq in range(HEADS):
        n += _same_bits(f"gqa head {hq}: dQ", dQ[hq], single[hq]["dQ"]) + _same_bits(f"gqa head {hq}: delta", delta[hq], single[hq]["delta"])
    for c in range(HEADS // GROUP):
        # (minus_zero: -0 must survive the fold, so the zeros are not folded in the comparison)
        n += _same_bits(f"gqa K/V head {c}: dK", dK[c], fold("dK", c), fold=not minus_zero)
        n += _same_bits(f"gqa K/V head {c}: dV", dV[c], fold("dV", c), fold=not minus_zero)
    if minus_zero:
        j = OC.neg_zero_key()
        assert np.all(np.signbit(dK[:, j].cpu().numpy())) and np.all(np.signbit(dV[:, j].cpu().numpy())), "the -0 key"
        assert not np.any(np.signbit(AO.gqa_fold([single[0]["dV"], single[1]["dV"]], from_zero=True)[j]))
    # group = 1: the _heads call on expanded K, V gives the unfolded single-head results
    K4, V4 = K2.repeat_interleave(GROUP, 0), V2.repeat_interleave(GROUP, 0)
    out1 = Outputs(gpu)
    delta1, dQ1 = out1.heads(HEADS, s.rows, 1).view(HEADS, s.rows), out1.heads(HEADS, s.rows, k)
    dK1, dV1 = out1.heads(HEADS, s.cols, k), out1.heads(HEADS, s.cols, kv)
    h.A.attention_backward_q_heads(Q, K4, V4, O, dO, stats, delta1, dQ1, scale)
    h.T.attention_backward_kv_heads(Q, K4, V4, dO, stats, delta_in, dK1, dV1, scale)
    out1.check()
    for hq in range(HEADS):
        for w, t in (("dQ", dQ1), ("delta", delta1), ("dK", dK1), ("dV", dV1)):
            n += _same_bits(f"heads (group = 1) head {hq}: {w}", t[hq], single[hq][w], fold=not minus_zero)
    assert torch.isfinite(dK).all() and torch.isfinite(dV).all()
    print(f"gqa {name} {case} k={k} kv={kv}: {n} values compared bit for bit")
    h.close()
