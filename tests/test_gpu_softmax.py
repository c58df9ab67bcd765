"""spmv_csr_row_softmax and spmv_csr_row_softmax_backward (include/spmv_hip.h "Row softmax") on the GPU.  Every forward
run goes into out filled with NaN, into out filled with a sentinel and in place; every backward run into NaN, into the
sentinel, over P and over dP: all must agree bit for bit.  Every output lies one float past a 16-byte boundary between two
bands of 4096 guard floats that must stay untouched.  What is checked:

  uniform rows   the 21 matrices of tests/_exact.py, every row one constant (-3e4, -1, 0, 7.5, 3e4 by row), scale in 1,
                 0.125, -2: every result is fp32(1) / fp32(L) bit for bit (exp(0) = 1, a sum of L < 2^24 ones is exact in
                 any order, 1 * r = r).  With scale = 0.3 the same holds only if t = scale * s is rounded before the
                 maximum is subtracted (a fused multiply-subtract leaves the rounding error of t in the exponent).
  masks          every entry -Inf with probability 1/2; rows with only the first or only the last entry kept, rows fully
                 masked, whole plan pieces of the long rows masked: fp32(1 / count) at kept entries, the bits of +0 at
                 masked ones, NaN across a fully masked row.
  non-finite     a NaN, a +Inf or an overflowing scale * s makes its row NaN; every other row keeps its exact result.
  parity         random scores with D = max t - min t <= 32 per row on six structures: within (2 D + 12 + A(L)) 2^-24 ref
                 of the fp64 recipe of tests/_softmax.py, entry by entry.
  invariance     two handles; the same rows among different neighbours (short ones, rows of 33 .. 64, rows of 300) in three
                 matrices; a row-block handle (row_ptr rebased, arrays at + first_nnz) against the whole matrix.
  backward       integers in [-4, 4], scale in 1, 0.25, -2, against int64 (every order is exact: the dot is at most 16 L and
                 every result below 2^24), +0 and -0 folded; normal floats within (A(L) + 4) 2^-24 |scale| |P| (|dP| +
                 sum |P dP|) + 1e-37 of fp64.
  composition    sddmm into the borrowed vals, the softmax in place, values_changed, spmm: against fp64.
  2^30           nnz just above 2^30, uniform rows by a closed formula, in place, checked on the device; then backward.
  graph          forward and backward captured after the plan, replayed with new data: exact.
  refusals       every status of the header's list, the output untouched (the refusal under another current device only
                 where a second device is visible); the wrapper's ValueErrors; rows = 0 and nnz = 0 return OK.
"""
import ctypes as C

import numpy as np
import pytest

import _exact as E
import _softmax as SM
from _util import RTOL

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1.2345e30)
GUARD, GUARD_N = np.float32(3.0e35), 4096
CONSTANTS = np.array([-3e4, -1.0, 0.0, 7.5, 3e4], np.float32)
BWD_SCALES = (1.0, 0.25, -2.0)
PARITY = sorted(E.SYNTH) + ["one_row_spanning_30_chunks", "wave_pipe_thresholds", "lengths_around_short_threshold"]


def _guarded(gpu, nnz):
    """(buffer, the nnz floats one float past a 16-byte boundary between its two guard bands)."""
    import torch
    buf = torch.full((2 * GUARD_N + nnz + 1,), float(GUARD), dtype=torch.float32, device=gpu)
    out = buf[GUARD_N + 1:GUARD_N + 1 + nnz]
    assert buf.data_ptr() % 16 == 0 and (nnz == 0 or out.data_ptr() % 16 == 4)
    return buf, out


def _guards_intact(buf, nnz):
    return bool((buf[:GUARD_N + 1] == float(GUARD)).all()) and bool((buf[GUARD_N + 1 + nnz:] == float(GUARD)).all())


def _mismatches(out, exp, fold_zeros=False):
    """Entries of out that are not the expectation's bits (a NaN is expected wherever exp holds one)."""
    import torch
    a, b = (out + 0.0, exp + 0.0) if fold_zeros else (out, exp)
    ok = torch.where(torch.isnan(exp), torch.isnan(out), a.view(torch.int32) == b.view(torch.int32))
    return int((~ok).sum().item())


class _Dev:
    """One pattern on the device (a borrowing handle, planned) and the run sets of one case."""

    def __init__(self, capi, gpu, rows, cols, rp, ci):
        import torch
        self.gpu, self.rows, self.nnz = gpu, rows, int(rp[-1])
        self.d_rp = torch.from_numpy(np.ascontiguousarray(rp, np.int32)).to(gpu)
        self.d_ci = torch.from_numpy(np.ascontiguousarray(ci, np.int32)).to(gpu)
        self.d_va = torch.full((self.nnz,), float("nan"), dtype=torch.float32, device=gpu)      # never read
        self.A = capi.CsrMatrix.from_device(rows, cols, self.d_rp, self.d_ci, self.d_va)
        self.A.spmm_plan()

    @classmethod
    def of(cls, capi, gpu, s):
        return cls(capi, gpu, s.rows, s.cols, s.rp, s.ci)

    def _agree(self, runs, what):
        import torch
        torch.cuda.synchronize()
        bad = [f"the {tag} run wrote outside its array" for tag, buf, _ in runs if not _guards_intact(buf, self.nnz)]
        first = runs[0][2].view(torch.int32)
        for tag, _, out in runs[1:]:
            d = int((out.view(torch.int32) != first).sum().item())
            if d:
                bad.append(f"{what}: {d} entries unwritten or different between the {runs[0][0]} and the {tag} run")
        return runs[0][2], bad

    def forward(self, scores, scale):
        """Into NaN, into the sentinel and in place; returns (out, complaints)."""
        runs = []
        for tag, fill in (("nan", float("nan")), ("sentinel", float(SENTINEL))):
            buf, out = _guarded(self.gpu, self.nnz)
            out.fill_(fill)
            self.A.row_softmax(scores, out, scale)
            runs.append((tag, buf, out))
        buf, out = _guarded(self.gpu, self.nnz)
        out.copy_(scores)
        self.A.row_softmax(out, out, scale)
        runs.append(("in-place", buf, out))
        return self._agree(runs, "forward")

    def backward(self, P, dP, scale):
        """Into NaN, into the sentinel, over P and over dP; returns (dS, complaints)."""
        runs = []
        for tag, fill in (("nan", float("nan")), ("sentinel", float(SENTINEL))):
            buf, out = _guarded(self.gpu, self.nnz)
            out.fill_(fill)
            self.A.row_softmax_backward(P, dP, out, scale)
            runs.append((tag, buf, out))
        buf, out = _guarded(self.gpu, self.nnz)
        out.copy_(P)
        self.A.row_softmax_backward(out, dP, out, scale)
        runs.append(("over-P", buf, out))
        buf, out = _guarded(self.gpu, self.nnz)
        out.copy_(dP)
        self.A.row_softmax_backward(P, out, out, scale)
        runs.append(("over-dP", buf, out))
        return self._agree(runs, "backward")

    def close(self):
        self.A.close()


def _to(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu)


def _lengths(s):
    return np.diff(s.rp).astype(np.int64)


def _row_constants(s, salt=0):
    """One constant per row, spread over CONSTANTS by the row number."""
    return CONSTANTS[(np.arange(s.rows) + salt) % CONSTANTS.size][s.row_of]


def _one_over(count):
    with np.errstate(divide="ignore"):
        return np.float32(1.0) / count.astype(np.float32)


# ---- forward, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.MATRICES)
def test_softmax_uniform_rows_are_one_over_the_length(pkg, oracle, gpu, name):
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    exp = _to(gpu, _one_over(_lengths(s))[s.row_of])
    scores = _to(gpu, _row_constants(s))
    failures = []
    for scale in SM.SCALES + (0.3,):
        out, bad = dev.forward(scores, scale)
        n = _mismatches(out, exp)
        if n:
            bad.append(f"{n} of {s.nnz} entries are not fp32(1) / fp32(L)")
        failures += [f"scale={scale}: {b}" for b in bad]
    dev.close()
    assert not failures, f"{name}:\n" + "\n".join(failures)


def _masked_case(s, scale, salt):
    """(scores, expectation): masked entries hold the infinity that scale turns into -Inf."""
    rng = np.random.Generator(np.random.PCG64([sum(map(ord, "mask")), salt, s.nnz]))
    L = _lengths(s)
    start = s.rp[:-1].astype(np.int64)
    pos = np.arange(s.nnz, dtype=np.int64) - start[s.row_of]          # position inside the row
    keep = rng.random(s.nnz) >= 0.5
    long_row = (L > SM.PIECE)[s.row_of]
    keep &= ~(long_row & ((pos // SM.PIECE) % 3 == 0))                # whole plan pieces, the first one included
    kind = (np.arange(s.rows) % 7)[s.row_of]
    keep = np.where(kind == 1, pos == 0, keep)                        # only the first entry kept
    keep = np.where(kind == 2, pos == L[s.row_of] - 1, keep)          # only the last
    keep = np.where(kind == 3, False, keep)                           # the row fully masked
    count = np.add.reduceat(keep.astype(np.int64), start[L > 0]) if s.nnz else np.zeros(0, np.int64)
    per_row = np.zeros(s.rows, np.int64)
    per_row[L > 0] = count
    scores = np.where(keep, _row_constants(s, salt), np.float32(-np.inf if scale > 0 else np.inf)).astype(np.float32)
    with np.errstate(divide="ignore"):
        exp = np.where(keep, _one_over(per_row)[s.row_of], np.float32(0.0)).astype(np.float32)
    exp[(per_row == 0)[s.row_of]] = np.nan
    return scores, exp


@pytest.mark.parametrize("name", E.MATRICES)
def test_softmax_masked_entries(pkg, oracle, gpu, name):
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    failures = []
    for salt, scale in enumerate(SM.SCALES):
        scores, exp = _masked_case(s, scale, salt)
        out, bad = dev.forward(_to(gpu, scores), scale)
        n = _mismatches(out, _to(gpu, exp))
        if n:
            bad.append(f"{n} of {s.nnz} entries differ (1 / count where kept, +0 where masked, NaN in a masked row)")
        failures += [f"scale={scale}: {b}" for b in bad]
    dev.close()
    assert not failures, f"{name}:\n" + "\n".join(failures)


@pytest.mark.parametrize("name", ["lengths_around_short_threshold", "long_row_between_short_rows", "wave_pipe_thresholds",
                                  "rows_exactly_chunk_aligned", "odd_last_chunk"])
def test_softmax_nonfinite_rows_are_nan_and_the_others_exact(pkg, oracle, gpu, name):
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    rng = np.random.Generator(np.random.PCG64([len(name), 9]))
    L = _lengths(s)
    full = np.flatnonzero(L > 0)
    scale = -2.0
    # -2 * -3e38 overflows to +Inf; -2 * -Inf is +Inf; the constants stay finite
    poisons = np.array([np.nan, -np.inf, -3e38], np.float32)
    bad_rows = np.unique(np.concatenate([rng.choice(full, size=max(1, full.size // 5), replace=False), [int(np.argmax(L))]]))
    scores = _row_constants(s).copy()
    for i, r in enumerate(bad_rows):
        at = int(s.rp[r]) + (int(L[r]) - 1 if i % 4 == 0 else int(rng.integers(0, L[r])))    # the last entry or anywhere
        scores[at] = poisons[i % 3]
    exp = _one_over(L)[s.row_of]
    exp[np.isin(s.row_of, bad_rows)] = np.nan
    out, bad = dev.forward(_to(gpu, scores), scale)
    n = _mismatches(out, _to(gpu, exp))
    dev.close()
    assert not bad and n == 0, f"{name}: {bad}; {n} entries differ (NaN in {bad_rows.size} rows, 1 / L elsewhere)"


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_softmax_parity_with_the_fp64_recipe(pkg, oracle, gpu, name):
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    for i, scale in enumerate(SM.SCALES):
        rng = np.random.Generator(np.random.PCG64([len(name), 21 + i]))
        scores = SM.clipped_scores(rng, s.nnz, scale)
        ref, D, L = SM.recipe(s.rp, scores, scale)
        assert D.max() <= 32.0 and ref.min() >= 1e-17
        out, bad = dev.forward(_to(gpu, scores), scale)
        assert not bad, (name, scale, bad)
        ratio = np.abs(out.cpu().numpy().astype(np.float64) - ref) / SM.parity_bound(ref, D, L)
        print(f"{name} scale={scale}: largest error / bound = {ratio.max():.3g}")
        assert ratio.max() <= 1.0, f"{name} scale={scale}: {int((ratio > 1).sum())} entries outside the bound, worst {ratio.max():.3g}"
    dev.close()


# ---- invariance ------------------------------------------------------------------------------------------------------------
PROBES = (1, 2, 3, 5, 17, 31, 32, 33, 64, 65, 129, 300, 512, 513, 1024, 2000)


def _among(neighbours, probes, rng):
    """Row lengths: every probe row between runs of 70 neighbour rows; returns (lengths, the probes' row numbers)."""
    lengths, where = [], []
    for p in probes:
        lengths += [int(v) for v in rng.choice(neighbours, size=70)]
        where.append(len(lengths))
        lengths.append(p)
    lengths += [int(v) for v in rng.choice(neighbours, size=5)]
    return np.array(lengths, np.int64), where


def test_softmax_a_row_does_not_depend_on_its_neighbours(pkg, gpu):
    rng = np.random.Generator(np.random.PCG64(2025))
    data = {p: rng.standard_normal(p).astype(np.float32) * 3 for p in PROBES}
    grads = {p: rng.standard_normal(p).astype(np.float32) for p in PROBES}
    results = []
    for neighbours, order in (([0, 1, 2, 3, 4], PROBES), (list(range(33, 65)), PROBES[::-1]), ([300], PROBES[3:] + PROBES[:3])):
        lengths, where = _among(neighbours, order, rng)
        rp = np.concatenate([[0], np.cumsum(lengths)])
        nnz = int(rp[-1])
        scores, dP = rng.standard_normal(nnz).astype(np.float32), rng.standard_normal(nnz).astype(np.float32)
        for p, r in zip(order, where):
            scores[rp[r]:rp[r + 1]] = data[p]
            dP[rp[r]:rp[r + 1]] = grads[p]
        dev = _Dev(pkg.capi, gpu, len(lengths), 4096, rp, np.zeros(nnz, np.int32))
        out, bad = dev.forward(_to(gpu, scores), 0.7)
        assert not bad, bad
        dS, bad = dev.backward(out, _to(gpu, dP), 0.7)
        assert not bad, bad
        out, dS = out.cpu().numpy(), dS.cpu().numpy()
        results.append({p: (out[rp[r]:rp[r + 1]].tobytes(), dS[rp[r]:rp[r + 1]].tobytes()) for p, r in zip(order, where)})
        dev.close()
    for p in PROBES:
        assert results[0][p] == results[1][p] == results[2][p], f"a row of {p} entries changes with its neighbours"


@pytest.mark.parametrize("name", ["wave_pipe_thresholds", "c3_powerlaw"])
def test_softmax_two_handles_and_a_row_block_agree(pkg, oracle, gpu, name):
    import torch
    capi = pkg.capi
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(capi, gpu, s)
    gen = torch.Generator(device=gpu).manual_seed(7)
    scores = torch.randn(s.nnz, generator=gen, device=gpu, dtype=torch.float32) * 3
    dP = torch.randn(s.nnz, generator=gen, device=gpu, dtype=torch.float32)
    out, bad = dev.forward(scores, -2.0)
    assert not bad, bad
    dS, bad = dev.backward(out, dP, -2.0)
    assert not bad, bad
    other = _Dev.of(capi, gpu, s)
    out2, _ = other.forward(scores, -2.0)
    dS2, _ = other.backward(out, dP, -2.0)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), "two handles differ (forward)"
    assert torch.equal(dS2.view(torch.int32), dS.view(torch.int32)), "two handles differ (backward)"
    other.close()
    # the rows [r0, r1) as a handle of their own: row_ptr rebased, every array at + first_nnz
    r0 = next(r for r in range(s.rows // 9, s.rows) if s.rp[r] % 4)      # the block's arrays start off a 16-byte boundary
    r1 = s.rows - s.rows // 7
    lo, hi = int(s.rp[r0]), int(s.rp[r1])
    block = _Dev(capi, gpu, r1 - r0, s.cols, s.rp[r0:r1 + 1].astype(np.int64) - lo, s.ci[lo:hi])
    assert block.nnz == hi - lo and scores[lo:].data_ptr() % 16 != 0
    b_out = torch.full((hi - lo,), float("nan"), dtype=torch.float32, device=gpu)
    block.A.row_softmax(scores[lo:hi], b_out, -2.0)
    b_dS = torch.full((hi - lo,), float("nan"), dtype=torch.float32, device=gpu)
    block.A.row_softmax_backward(out[lo:hi], dP[lo:hi], b_dS, -2.0)
    whole = scores.clone()                   # and in place inside the whole array: nothing outside [lo, hi) changes
    block.A.row_softmax(whole[lo:hi], whole[lo:hi], -2.0)
    torch.cuda.synchronize()
    assert torch.equal(b_out.view(torch.int32), out[lo:hi].view(torch.int32)), "the row block differs from the whole matrix"
    assert torch.equal(b_dS.view(torch.int32), dS[lo:hi].view(torch.int32)), "the row block differs (backward)"
    assert torch.equal(whole[lo:hi].view(torch.int32), out[lo:hi].view(torch.int32))
    assert torch.equal(whole[:lo], scores[:lo]) and torch.equal(whole[hi:], scores[hi:])
    block.close()
    dev.close()


# ---- backward ----------------------------------------------------------------------------------------------------------------
def _int_pair(name, nnz):
    rng = np.random.Generator(np.random.PCG64([sum(map(ord, name)), 31]))
    return rng.integers(-4, 5, size=nnz), rng.integers(-4, 5, size=nnz)


def _int_backward(s, P, dP):
    """P (dP - dot) per entry in int64."""
    L = _lengths(s)
    dot = np.zeros(s.rows, np.int64)
    if s.nnz:
        dot[L > 0] = np.add.reduceat(P * dP, s.rp[:-1].astype(np.int64)[L > 0])
    res = P * (dP - dot[s.row_of])
    assert res.size == 0 or np.abs(res).max() < E.EXACT_LIMIT
    return res


@pytest.mark.parametrize("name", E.MATRICES)
def test_softmax_backward_exact_on_integers(pkg, oracle, gpu, name):
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    P, dP = _int_pair(name, s.nnz)
    res = _int_backward(s, P, dP)
    failures = []
    for scale in BWD_SCALES:
        dS, bad = dev.backward(_to(gpu, P), _to(gpu, dP), scale)
        n = _mismatches(dS, _to(gpu, scale * res.astype(np.float64)), fold_zeros=True)
        if n:
            bad.append(f"{n} of {s.nnz} entries differ from the int64 expectation")
        failures += [f"scale={scale}: {b}" for b in bad]
    dev.close()
    assert not failures, f"{name}:\n" + "\n".join(failures)


@pytest.mark.parametrize("name", PARITY)
def test_softmax_backward_parity_with_fp64(pkg, oracle, gpu, name):
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    L = _lengths(s)[s.row_of]
    for i, scale in enumerate(BWD_SCALES):
        rng = np.random.Generator(np.random.PCG64([len(name), 41 + i]))
        P, dP = rng.standard_normal(s.nnz).astype(np.float32), rng.standard_normal(s.nnz).astype(np.float32)
        ref, mag = SM.backward_recipe(s.rp, P, dP, scale)
        dS, bad = dev.backward(_to(gpu, P), _to(gpu, dP), scale)
        assert not bad, (name, scale, bad)
        ratio = np.abs(dS.cpu().numpy().astype(np.float64) - ref) / SM.backward_bound(mag, L)
        print(f"{name} scale={scale}: largest error / bound = {ratio.max():.3g}")
        assert ratio.max() <= 1.0, f"{name} scale={scale}: {int((ratio > 1).sum())} entries outside the bound, worst {ratio.max():.3g}"
    dev.close()


# ---- composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd_last_chunk", "wave_pipe_thresholds"])
def test_sddmm_softmax_spmm_compose(pkg, oracle, gpu, name):
    import torch
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    rng = np.random.Generator(np.random.PCG64([len(name), 51]))
    k, kv, scale = 8, 5, 2.0 ** -4
    Q, K = rng.integers(-2, 3, size=(s.rows, k)), rng.integers(-2, 3, size=(s.cols, k))
    V = rng.standard_normal((s.cols, kv)).astype(np.float32)
    dev.A.sddmm(_to(gpu, Q), _to(gpu, K), dev.d_va)                   # the handle's own borrowed vals
    dev.A.row_softmax(dev.d_va, dev.d_va, scale)
    dev.A.values_changed()
    O = torch.full((s.rows, kv), float("nan"), dtype=torch.float32, device=gpu)
    dev.A.spmm(_to(gpu, V), O)
    torch.cuda.synchronize()
    scores = np.einsum("nc,nc->n", Q[s.row_of], K[s.ci]).astype(np.float32)       # exact, and so is scale * scores
    ref, D, L = SM.recipe(s.rp, scores, scale)
    rel = SM.parity_bound(np.ones_like(ref), D, L) + RTOL
    terms = ref[:, None] * V[s.ci].astype(np.float64)
    want, bound = np.zeros((s.rows, kv)), np.zeros((s.rows, kv))
    np.add.at(want, s.row_of, terms)
    np.add.at(bound, s.row_of, rel[:, None] * np.abs(terms))
    err = np.abs(O.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= bound + 1e-37), f"{name}: {int((err > bound + 1e-37).sum())} entries of O outside the bound"
    dev.close()


# ---- beyond 2^30 nonzeros --------------------------------------------------------------------------------------------------------
def test_softmax_nnz_beyond_2_to_30(pkg, gpu):
    """4 n passes 2^32: rows of 64 nonzeros, nnz = 2^30 + 64, every row one constant; in place; every entry checked."""
    import torch
    per, rows = 64, (1 << 24) + 1
    nnz = rows * per
    assert (1 << 30) < nnz < (1 << 31)
    d_rp = (torch.arange(rows + 1, device=gpu, dtype=torch.int64) * per).to(torch.int32)
    d_ci = torch.zeros(nnz, dtype=torch.int32, device=gpu)               # (never read by these calls)
    buf = torch.empty(nnz, dtype=torch.float32, device=gpu)
    row_const = ((torch.arange(rows, device=gpu, dtype=torch.int64) * 5) % 9 - 4).to(torch.float32)
    buf.view(rows, per).copy_(row_const[:, None].expand(rows, per))
    A = pkg.capi.CsrMatrix.from_device(rows, 4096, d_rp, d_ci, buf)
    A.spmm_plan()
    A.row_softmax(buf, buf, -2.0)
    torch.cuda.synchronize()
    assert bool((buf == 1.0 / per).all()), f"{int((buf != 1.0 / per).sum())} entries are not 1 / 64"
    # backward over dP: dP one integer per row, so dot = 64 * (c / 64) = c and every dS is a zero
    dP = torch.empty(nnz, dtype=torch.float32, device=gpu)
    dP.view(rows, per).copy_(row_const[:, None].expand(rows, per))
    A.row_softmax_backward(buf, dP, dP, 0.25)
    torch.cuda.synchronize()
    assert bool((dP == 0).all()), f"{int((dP != 0).sum())} entries of dS are not zero"
    assert bool((buf == 1.0 / per).all())
    A.close()


# ---- graph capture -----------------------------------------------------------------------------------------------------------------
def test_softmax_graph_capture(pkg, oracle, gpu):
    import torch
    name = "wave_pipe_thresholds"
    s = E.structure(name, pkg, oracle)
    dev = _Dev.of(pkg.capi, gpu, s)
    sc, out = torch.zeros(s.nnz, device=gpu), torch.full((s.nnz,), float("nan"), device=gpu)
    P, dP, dS = torch.zeros(s.nnz, device=gpu), torch.zeros(s.nnz, device=gpu), torch.full((s.nnz,), float("nan"), device=gpu)
    dev.A.row_softmax(sc, out, 0.125)                       # (every kernel has run once before the capture)
    dev.A.row_softmax_backward(P, dP, dS, 0.25)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.A.row_softmax(sc, out, 0.125)
        dev.A.row_softmax_backward(P, dP, dS, 0.25)
    Pi, dPi = _int_pair(name, s.nnz)
    res = _int_backward(s, Pi, dPi)
    sc.copy_(_to(gpu, _row_constants(s)))
    P.copy_(_to(gpu, Pi))
    dP.copy_(_to(gpu, dPi))
    g.replay()
    torch.cuda.synchronize()
    assert _mismatches(out, _to(gpu, _one_over(_lengths(s))[s.row_of])) == 0
    assert _mismatches(dS, _to(gpu, 0.25 * res.astype(np.float64)), fold_zeros=True) == 0
    scores, exp = _masked_case(s, 0.125, 5)
    sc.copy_(_to(gpu, scores))
    P.copy_(_to(gpu, -dPi))
    dP.copy_(_to(gpu, Pi))
    out.fill_(float("nan"))
    dS.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _mismatches(out, _to(gpu, exp)) == 0
    assert _mismatches(dS, _to(gpu, 0.25 * _int_backward(s, -dPi, Pi).astype(np.float64)), fold_zeros=True) == 0
    dev.close()


# ---- refusals and edges ----------------------------------------------------------------------------------------------------------------
def test_softmax_refusals_leave_the_output_untouched(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    s = E.structure("lengths_around_short_threshold", pkg, oracle)
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    d_va = torch.zeros(s.nnz, dtype=torch.float32, device=gpu)
    A = capi.CsrMatrix.from_device(s.rows, s.cols, d_rp, d_ci, d_va)
    x = torch.ones(s.nnz + 4, dtype=torch.float32, device=gpu)
    out = torch.full((s.nnz + 4,), float(SENTINEL), dtype=torch.float32, device=gpu)
    before = out.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, op = x.data_ptr(), out.data_ptr()
    fwd, bwd = lib.spmv_csr_row_softmax, lib.spmv_csr_row_softmax_backward

    def named(rc, status, name):
        assert rc == status, (name, rc)
        assert name + (":" if status == capi.ERR_INVALID else " ") in lib.spmv_last_error().decode()

    named(fwd(A._h, 1.0, xp, op, st), capi.ERR_NOT_PLANNED, "spmv_csr_row_softmax")           # before the plan
    named(bwd(A._h, 1.0, xp, xp, op, st), capi.ERR_NOT_PLANNED, "spmv_csr_row_softmax_backward")
    A.spmm_plan()
    for scale in (float("inf"), float("-inf"), float("nan")):
        named(fwd(A._h, scale, xp, op, st), capi.ERR_INVALID, "spmv_csr_row_softmax")
        named(bwd(A._h, scale, xp, xp, op, st), capi.ERR_INVALID, "spmv_csr_row_softmax_backward")
    for a, b in ((None, op), (xp, None), (xp + 2, op), (xp, op + 1), (xp + 3, op + 3)):
        named(fwd(A._h, 1.0, a, b, st), capi.ERR_INVALID, "spmv_csr_row_softmax")
    for a, b, c in ((None, xp, op), (xp, None, op), (xp, xp, None), (xp + 2, xp, op), (xp, xp + 1, op), (xp, xp, op + 2)):
        named(bwd(A._h, 1.0, a, b, c, st), capi.ERR_INVALID, "spmv_csr_row_softmax_backward")
    named(fwd(None, 1.0, xp, op, st), capi.ERR_INVALID, "spmv_csr_row_softmax")
    named(bwd(None, 1.0, xp, xp, op, st), capi.ERR_INVALID, "spmv_csr_row_softmax_backward")
    if torch.cuda.device_count() >= 2:                    # another current device than the handle's
        with torch.cuda.device(1):
            named(fwd(A._h, 1.0, xp, op, None), capi.ERR_INVALID, "spmv_csr_row_softmax")
            named(bwd(A._h, 1.0, xp, xp, op, None), capi.ERR_INVALID, "spmv_csr_row_softmax_backward")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32))
    # the wrapper checks before it calls
    good, o = x[:s.nnz], out[:s.nnz]
    for bad in (x[:s.nnz - 1], x[:s.nnz].double(), torch.cat([x, x])[:2 * s.nnz:2],
                x[:s.nnz].view(1, -1), None):
        with pytest.raises(ValueError):
            A.row_softmax(bad, o)
        with pytest.raises(ValueError):
            A.row_softmax(good, bad)
        with pytest.raises(ValueError):
            A.row_softmax_backward(bad, good, o)
        with pytest.raises(ValueError):
            A.row_softmax_backward(good, bad, o)
        with pytest.raises(ValueError):
            A.row_softmax_backward(good, good, bad)
    with pytest.raises(ValueError):
        A.row_softmax(good, o, scale=float("inf"))
    with pytest.raises(ValueError):
        A.row_softmax_backward(good, good, o, scale=float("nan"))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32))
    L = _lengths(s)[s.row_of]
    o2 = torch.full((s.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    A.row_softmax(good, o2, scale=3.0)                   # and the good calls, 4-byte aligned views included
    torch.cuda.synchronize()
    assert torch.equal(o2, _to(gpu, _one_over(L)))
    A.row_softmax_backward(x[1:s.nnz + 1], x[3:s.nnz + 3], out[1:s.nnz + 1], scale=1.0)
    torch.cuda.synchronize()
    assert torch.equal(out[0], before[0]) and torch.equal(out[s.nnz + 1:], before[s.nnz + 1:])
    assert torch.equal(out[1:s.nnz + 1], _to(gpu, (1.0 - L).astype(np.float32)))       # 1 * (1 - L)
    A.close()


@pytest.mark.parametrize("rows,cols", [(0, 10), (5, 0), (7, 9)])
def test_softmax_empty_shapes(pkg, gpu, rows, cols):
    import torch
    capi = pkg.capi
    d_rp = torch.zeros(rows + 1, dtype=torch.int32, device=gpu)
    d_ci = torch.zeros(1, dtype=torch.int32, device=gpu)[:0]
    d_va = torch.zeros(1, dtype=torch.float32, device=gpu)[:0]
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    e = torch.empty(0, dtype=torch.float32, device=gpu)
    A.row_softmax(e, e)
    A.row_softmax_backward(e, e, e)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert capi.lib().spmv_csr_row_softmax(A._h, 1.0, None, None, st) == capi.OK
    assert capi.lib().spmv_csr_row_softmax(A._h, 1.0, 2, 6, st) == capi.OK                # whatever the pointers are
    assert capi.lib().spmv_csr_row_softmax_backward(A._h, 1.0, None, 2, None, st) == capi.OK
    torch.cuda.synchronize()
    A.close()
