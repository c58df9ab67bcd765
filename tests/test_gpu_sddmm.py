"""spmv_csr_sddmm (out[n] = U[row(n), :k] . X[col(n), :k], include/spmv_hip.h "SDDMM") on the GPU.  What is checked:

  exact          the 21 matrices of tests/_exact.py in four forms (exact, subnormal, dilated with every unreferenced X row
                 NaN / +Inf / -Inf, unsorted with duplicates); U and X hold integers in [-4, 4], the U rows scaled by
                 2^e[row] (|sum| <= 1024: every order is exact), the expectation is int64 arithmetic.  k in KS with (ldu,
                 ldx) drawn from k, k + 3 and k rounded up to 4, mixed pairs included; the columns [k, ld) hold NaN, and so
                 do the U rows of empty rows.  out must match bit for bit (+0 and -0 folded).  Each case runs twice, into
                 out filled with NaN and with a sentinel: the two agree.  out lies one float past a 16-byte boundary
                 between two bands of 4096 guard floats that every run must leave untouched.  Equal (row, column) pairs of
                 the unsorted form get equal bits because both match the one expectation.
  padding        every k in 1 .. 63 that is not a multiple of 4, ld rounded up to 4 (the fast path), NaN in [k, ld).
  non-finite     Inf * 0 and +Inf + -Inf inside a dot give NaN; per entry the class of an fp64 numpy dot, finite ones exact.
  invariance     random normal floats on c3_powerlaw, k in 1, 13, 64: the same bits for every (ldu, ldx), two runs, two
                 handles; the nonzeros shuffled inside rows permute out the same way; NaN in every row of U and X that a
                 probe set of nonzeros does not touch leaves those nonzeros' bits; T.sddmm(X, U) == A.sddmm(U, X)[perm].
  parity         the three synthetic structures, random floats, k = 13: within _util.RTOL sum|terms| of the fp64 dot (the
                 project's bound; a 64-term fp32 dot stays under it by 64 2^-24 = 3.8e-6).
  4 GiB, 2^30    X of 2^24 + 3 rows and U of 2^24 + 3 rows at k = 64, nnz just above 2^30 at k = 4: integer data by closed
                 formulas, built and checked on the device.
  graph          captured after spmm_plan, replayed with new U and X: exact.
  refusals       a call before the plan, k = 0 / 65, ldu < k, ldx < k, misaligned U / X: the documented status, out
                 untouched; the wrapper's ValueErrors; rows = 0, cols = 0, nnz = 0 return OK.
  borrowed vals  SDDMM writes the handle's own vals, then values_changed, then spmm multiplies with them: exact.
"""
import ctypes as C

import numpy as np
import pytest

import _exact as E
from _util import RTOL

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 13, 16, 31, 32, 33, 64)      # SpMM's
KINDS = ("exact", "subnormal", "poison", "unsorted")
SENTINEL = np.float32(-1.2345e30)
GUARD, GUARD_N = np.float32(3.0e35), 4096


def _lds(k):
    return sorted({k, k + 3, (k + 3) // 4 * 4})


def _ld_pairs(k):
    lds = _lds(k)
    return sorted({(ld, ld) for ld in lds} | {(lds[-1], lds[0]), (lds[0], lds[-1]), (lds[1 % len(lds)], lds[-1])})


def _bits(t):
    import torch
    return (t + 0.0).view(torch.int32)      # (+0 folds -0: an exact zero sum may carry either sign)


def _ints(name, n, salt):
    rng = np.random.Generator(np.random.PCG64([sum(map(ord, name)), salt]))
    return rng.integers(-4, 5, size=(n, 64)).astype(np.int32)


def _padded(M64, k, ld):
    """(n, ld) device tensor: columns [0, k) of M64, NaN behind them; returns the (n, k) view the wrapper takes."""
    import torch
    P = torch.full((M64.shape[0], ld), float("nan"), dtype=torch.float32, device=M64.device)
    P[:, :k] = M64[:, :k]
    return P[:, :k]


class _Sddmm:
    """One pattern on the device (a borrowing handle, planned) and the checks of one run pair."""

    def __init__(self, capi, gpu, s):
        import torch
        self.gpu, self.s = gpu, s
        self.d_rp = torch.from_numpy(s.rp).to(gpu)
        self.d_ci = torch.from_numpy(s.ci).to(gpu)
        self.d_va = torch.full((s.nnz,), float("nan"), dtype=torch.float32, device=gpu)    # never read
        self.A = capi.CsrMatrix.from_device(s.rows, s.cols, self.d_rp, self.d_ci, self.d_va)
        self.A.spmm_plan()
        self.row_of = torch.from_numpy(s.row_of).to(gpu)
        self.col_of = self.d_ci.to(torch.int64)

    def int_dots(self, Ui, Xi, k):
        """int64 sum over c < k of Ui[row(n), c] * Xi[col(n), c] per nonzero (device; Ui, Xi int32 device tensors)."""
        import torch
        out = torch.zeros(self.s.nnz, dtype=torch.int64, device=self.gpu)
        for n0 in range(0, self.s.nnz, 1 << 20):
            sl = slice(n0, n0 + (1 << 20))
            out[sl] = (Ui[self.row_of[sl], :k].to(torch.int64) * Xi[self.col_of[sl], :k].to(torch.int64)).sum(1)
        return out

    def run_pair(self, U64, X64, k, ldu, ldx):
        """Runs k columns with these leading dimensions into NaN and into the sentinel; returns (out, complaints)."""
        import torch
        nnz = self.s.nnz
        U, X = _padded(U64, k, ldu), _padded(X64, k, ldx)
        outs, bufs = [], []
        for fill in (float("nan"), float(SENTINEL)):
            buf = torch.full((2 * GUARD_N + nnz + 1,), float(GUARD), dtype=torch.float32, device=self.gpu)
            out = buf[GUARD_N + 1:GUARD_N + 1 + nnz]        # one float past a 16-byte boundary
            assert buf.data_ptr() % 16 == 0 and (nnz == 0 or out.data_ptr() % 16 == 4)
            out.fill_(fill)
            self.A.sddmm(U, X, out)
            outs.append(out)
            bufs.append(buf)
        torch.cuda.synchronize()
        bad = []
        for buf in bufs:
            if not (bool((buf[:GUARD_N + 1] == float(GUARD)).all()) and bool((buf[GUARD_N + 1 + nnz:] == float(GUARD)).all())):
                bad.append("a run wrote outside out")
        d = (outs[0].view(torch.int32) != outs[1].view(torch.int32)).sum().item()
        if d:
            bad.append(f"{d} entries unwritten or different between two runs")
        return outs[0], bad

    def close(self):
        self.A.close()


def _scaled(sums, exps):
    """fp32 of int64 sums (device) times 2^exps (numpy per nonzero, or one int), through float64 on the host."""
    import torch
    h = np.ldexp(sums.cpu().numpy().astype(np.float64), exps).astype(np.float32)
    return torch.from_numpy(h).to(sums.device)


def _sweep(dev, U64, X64, Ui, Xi, exps, label):
    failures = []
    for k in KS:
        exp = _scaled(dev.int_dots(Ui, Xi, k), exps)
        for ldu, ldx in _ld_pairs(k):
            out, bad = dev.run_pair(U64, X64, k, ldu, ldx)
            n = int((_bits(out) != _bits(exp)).sum().item())
            if n:
                bad.append(f"{n} of {out.numel()} entries differ from the expectation")
            if bad:
                failures.append(f"{label} k={k} ldu={ldu} ldx={ldx}: " + "; ".join(bad))
    return failures


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", E.MATRICES)
def test_sddmm_exact_every_nonzero(pkg, oracle, gpu, name, kind):
    import torch
    s = E.structure(name, pkg, oracle)
    if kind == "unsorted":
        s, _ = E.shuffled(s, name)
    Ui_h, Xi_h = _ints(name + kind, s.rows, 1), _ints(name + kind, s.cols, 2)
    e_row = np.random.Generator(np.random.PCG64([len(name), 3])).integers(-40, 41, size=s.rows)
    empty = np.diff(s.rp) == 0
    Ui, Xi = torch.from_numpy(Ui_h).to(gpu), torch.from_numpy(Xi_h).to(gpu)
    if kind == "subnormal":
        U_h = np.ldexp(Ui_h.astype(np.float64), E.SUB_VAL_EXP).astype(np.float32)
        X_h = np.ldexp(Xi_h.astype(np.float64), E.SUB_X_EXP).astype(np.float32)
        exps = E.SUB_VAL_EXP + E.SUB_X_EXP
    else:
        U_h = np.ldexp(Ui_h.astype(np.float64), e_row[:, None]).astype(np.float32)
        X_h = Xi_h.astype(np.float32)
        exps = e_row[s.row_of]
    U_h[empty] = np.nan                                   # the U row of an empty row never reaches a result
    U64 = torch.from_numpy(U_h).to(gpu)
    failures = []
    if kind == "poison":
        dev = _Sddmm(pkg.capi, gpu, E.dilate(s))
        Xi_d = torch.zeros((2 * s.cols + 1, 64), dtype=torch.int32, device=gpu)
        Xi_d[1::2] = Xi
        for tag, p in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            Xd = np.full((2 * s.cols + 1, 64), p, np.float32)
            Xd[1::2] = X_h
            failures += _sweep(dev, U64, torch.from_numpy(Xd).to(gpu), Ui, Xi_d, exps, f"poison_{tag}")
    else:
        dev = _Sddmm(pkg.capi, gpu, s)
        failures += _sweep(dev, U64, torch.from_numpy(X_h).to(gpu), Ui, Xi, exps, kind)
    dev.close()
    assert not failures, f"{name}/{kind}: {len(failures)} failing case(s):\n" + "\n".join(failures[:20])


def test_sddmm_padding_every_k_on_the_fast_path(pkg, oracle, gpu):
    import torch
    name = "not_multiple_of_anything"
    s = E.structure(name, pkg, oracle)
    dev = _Sddmm(pkg.capi, gpu, s)
    Ui, Xi = torch.from_numpy(_ints(name, s.rows, 4)).to(gpu), torch.from_numpy(_ints(name, s.cols, 5)).to(gpu)
    U64, X64 = Ui.to(torch.float32), Xi.to(torch.float32)
    failures = []
    for k in (k for k in range(1, 64) if k % 4):
        ld = (k + 3) // 4 * 4
        exp = dev.int_dots(Ui, Xi, k).to(torch.float32)
        out, bad = dev.run_pair(U64, X64, k, ld, ld + 4)            # both multiples of 4: 16-byte loads over the NaN
        if int((_bits(out) != _bits(exp)).sum().item()):
            bad.append("differs from the expectation")
        if bad:
            failures.append(f"k={k}: " + "; ".join(bad))
    dev.close()
    assert not failures, "\n".join(failures)


def test_sddmm_nonfinite_classes(pkg, oracle, gpu):
    import torch
    name = "odd_last_chunk"
    s = E.structure(name, pkg, oracle)
    dev = _Sddmm(pkg.capi, gpu, s)
    rng = np.random.Generator(np.random.PCG64(77))
    U_h, X_h = _ints(name, s.rows, 6).astype(np.float32), _ints(name, s.cols, 7).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan], np.float32)
    ru, rx = rng.choice(s.rows, 300, replace=False), rng.choice(s.cols, 300, replace=False)
    U_h[ru, rng.integers(0, 64, 300)] = np.resize(special, 300)          # Inf * 0 wherever the other side holds a zero
    X_h[rx, rng.integers(0, 64, 300)] = np.resize(special, 300)
    X_h[rx[:100], 0] = np.inf                                             # +Inf and -Inf inside one dot: these X rows under
    X_h[rx[:100], 1] = -np.inf                                            # U rows whose columns 0 and 1 have the same sign
    U64, X64 = torch.from_numpy(U_h).to(gpu), torch.from_numpy(X_h).to(gpu)
    seen = set()
    for k in (5, 13, 64):
        with np.errstate(invalid="ignore", over="ignore"):
            ref = np.einsum("nc,nc->n", U_h[s.row_of, :k].astype(np.float64), X_h[s.ci, :k].astype(np.float64))
        seen |= {"nan"} if np.isnan(ref).any() else set()
        seen |= {"inf"} if np.isinf(ref).any() else set()
        for ldu, ldx in _ld_pairs(k):
            out, bad = dev.run_pair(U64, X64, k, ldu, ldx)
            assert not bad, (k, ldu, ldx, bad)
            got = out.cpu().numpy()
            fin = np.isfinite(ref)
            assert np.array_equal(got[fin], ref[fin].astype(np.float32)), f"k={k}: finite entries differ"
            assert np.array_equal(np.isnan(got), np.isnan(ref)), f"k={k}: NaN where the fp64 dot has none, or the reverse"
            inf = np.isinf(ref)
            assert np.array_equal(got[inf], ref[inf].astype(np.float32)), f"k={k}: infinities differ"
    assert seen == {"nan", "inf"}
    dev.close()


# ---- invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 13, 64])
def test_sddmm_order_of_sums_is_a_function_of_the_operands(pkg, oracle, gpu, k):
    import torch
    capi = pkg.capi
    s = E.structure("c3_powerlaw", pkg, oracle)
    dev = _Sddmm(capi, gpu, s)
    gen = torch.Generator(device=gpu).manual_seed(100 + k)
    U64 = torch.randn((s.rows, 64), generator=gen, device=gpu, dtype=torch.float32)
    X64 = torch.randn((s.cols, 64), generator=gen, device=gpu, dtype=torch.float32)

    def run(A, U, X, nnz=s.nnz):
        out = torch.full((nnz,), float("nan"), dtype=torch.float32, device=gpu)
        A.sddmm(U, X, out)
        torch.cuda.synchronize()
        return out.view(torch.int32)

    base = run(dev.A, U64[:, :k].contiguous(), X64[:, :k].contiguous())
    assert not torch.isnan(base.view(torch.float32)).any()
    lds = _lds(k)
    for ldu in lds:
        for ldx in lds:
            assert torch.equal(run(dev.A, _padded(U64, k, ldu), _padded(X64, k, ldx)), base), f"ldu={ldu} ldx={ldx} differs"
    assert torch.equal(run(dev.A, _padded(U64, k, lds[-1]), _padded(X64, k, lds[-1])), base), "two runs differ"
    B = capi.CsrMatrix.from_device(s.rows, s.cols, dev.d_rp, dev.d_ci, dev.d_va)
    B.spmm_plan()
    assert torch.equal(run(B, _padded(U64, k, lds[0]), _padded(X64, k, lds[-1])), base), "two handles differ"
    B.close()
    # the nonzeros shuffled inside their rows: out is permuted the same way (position and piece do not matter)
    rng = np.random.Generator(np.random.PCG64(k))
    order = np.lexsort((rng.random(s.nnz), s.row_of))
    d_ci2 = torch.from_numpy(s.ci[order]).to(gpu)
    S = capi.CsrMatrix.from_device(s.rows, s.cols, dev.d_rp, d_ci2, dev.d_va)
    S.spmm_plan()
    assert torch.equal(run(S, _padded(U64, k, lds[-1]), _padded(X64, k, lds[-1])), base[torch.from_numpy(order).to(gpu)]), \
        "shuffled rows are not the same numbers permuted"
    S.close()
    # NaN in every row of U and X the probe does not touch
    probe = np.unique(np.concatenate([rng.integers(0, s.nnz, size=500), [0, s.nnz - 1]]))
    Up = torch.full_like(U64, float("nan"))
    Xp = torch.full_like(X64, float("nan"))
    ru, rx = torch.from_numpy(np.unique(s.row_of[probe])).to(gpu), torch.from_numpy(np.unique(s.ci[probe]).astype(np.int64)).to(gpu)
    Up[ru], Xp[rx] = U64[ru], X64[rx]
    d_probe = torch.from_numpy(probe).to(gpu)
    assert torch.equal(run(dev.A, _padded(Up, k, lds[-1]), _padded(Xp, k, lds[-1]))[d_probe], base[d_probe]), \
        "a probed nonzero changes with NaN in rows it does not touch"
    # the operands trade places on the transposed pattern
    T = dev.A.transpose()
    T.spmm_plan()
    perm = torch.from_numpy(np.argsort(s.ci, kind="stable")).to(gpu)
    assert torch.equal(run(T, _padded(X64, k, lds[-1]), _padded(U64, k, lds[0])), base[perm]), "T.sddmm(X, U) != A.sddmm(U, X)[perm]"
    T.close()
    dev.close()


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.SYNTH))
def test_sddmm_parity_with_fp64(pkg, oracle, gpu, name):
    import torch
    s = E.structure(name, pkg, oracle)
    dev = _Sddmm(pkg.capi, gpu, s)
    k = 13
    gen = torch.Generator(device=gpu).manual_seed(13)
    U = torch.randn((s.rows, 16), generator=gen, device=gpu, dtype=torch.float32)[:, :k]
    X = torch.randn((s.cols, 16), generator=gen, device=gpu, dtype=torch.float32)[:, :k]
    out = torch.full((s.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    dev.A.sddmm(U, X, out)
    torch.cuda.synchronize()
    worst = 0.0
    for n0 in range(0, s.nnz, 1 << 20):
        sl = slice(n0, n0 + (1 << 20))
        terms = U[dev.row_of[sl]].to(torch.float64) * X[dev.col_of[sl]].to(torch.float64)
        err = (out[sl].to(torch.float64) - terms.sum(1)).abs()
        bound = RTOL * terms.abs().sum(1) + 1e-37
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), f"{name}: {int((~(err <= bound)).sum())} entries outside {RTOL:g} sum|terms| from {n0} on"
    print(f"{name}: largest error / bound = {worst:.3g}")
    dev.close()


# ---- beyond 4 GiB and 2^30 nonzeros -------------------------------------------------------------------------------------
def _x_formula(j, c):
    return ((j * 7 + c * 13) % 9) - 4


def _u_formula(i, c):
    return ((i * 5 + c * 3) % 9) - 4


def _fill(t, formula):
    """t[r, c] = formula(r, c), in slabs on the device."""
    import torch
    cc = torch.arange(t.shape[1], device=t.device, dtype=torch.int64)
    for r0 in range(0, t.shape[0], 1 << 20):
        r = torch.arange(r0, min(t.shape[0], r0 + (1 << 20)), device=t.device, dtype=torch.int64)[:, None]
        t[r0:r0 + r.shape[0]] = formula(r, cc).to(torch.float32)


def _check_formula(out, row_of, col_of, k, slab):
    """out[n] == sum over c < k of u(row(n), c) x(col(n), c) for every n (row_of, col_of: callables of a position slab)."""
    import torch
    cc = torch.arange(k, device=out.device, dtype=torch.int64)
    for n0 in range(0, out.numel(), slab):
        n = torch.arange(n0, min(out.numel(), n0 + slab), device=out.device, dtype=torch.int64)
        want = (_u_formula(row_of(n)[:, None], cc) * _x_formula(col_of(n)[:, None], cc)).sum(1).to(torch.float32)
        bad = int((out[n0:n0 + n.numel()] != want).sum().item())
        assert bad == 0, f"{bad} entries differ in the slab from {n0} on"


def test_sddmm_x_beyond_4gib(pkg, gpu):
    import torch
    cols, k, rows, per = (1 << 24) + 3, 64, 1 << 17, 4
    rng = np.random.Generator(np.random.PCG64(2024))
    ci = rng.integers(0, cols, size=(rows, per)).astype(np.int64)
    ci[0] = (0, cols - 1, cols - 2, 1)
    ci[-1] = (cols - 1, cols - 1, 0, cols - 3)       # a repeated column
    ci[1:1000, 0] = cols - 1 - rng.integers(0, 1 << 16, size=999)
    d_ci = torch.from_numpy(ci.reshape(-1).astype(np.int32)).to(gpu)
    d_rp = torch.arange(rows + 1, device=gpu, dtype=torch.int32) * per
    X = torch.empty((cols, k), dtype=torch.float32, device=gpu)             # 4.3 GB
    U = torch.empty((rows, k), dtype=torch.float32, device=gpu)
    _fill(X, _x_formula)
    _fill(U, _u_formula)
    out = torch.full((rows * per,), float("nan"), dtype=torch.float32, device=gpu)
    A = pkg.capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, out)         # (vals is never read: out stands in)
    A.spmm_plan()
    A.sddmm(U, X, out)
    torch.cuda.synchronize()
    col64 = d_ci.to(torch.int64)
    _check_formula(out, lambda n: n // per, lambda n: col64[n], k, 1 << 19)
    A.close()


def test_sddmm_u_beyond_4gib(pkg, gpu):
    import torch
    rows, cols, k = (1 << 24) + 3, 4096, 64
    r = torch.arange(rows, device=gpu, dtype=torch.int64)
    lengths = 1 + r % 2
    lengths[(r % 5 == 0) & (r < rows - 65536)] = 0                   # empty rows, but the last 65 536 are not
    rp = torch.zeros(rows + 1, dtype=torch.int64, device=gpu)
    rp[1:] = torch.cumsum(lengths, 0)
    nnz = int(rp[-1].item())
    row_of = torch.repeat_interleave(r, lengths)
    del r, lengths
    n = torch.arange(nnz, device=gpu, dtype=torch.int64)
    d_ci = ((n * 2654435761) % cols).to(torch.int32)
    del n
    U = torch.empty((rows, k), dtype=torch.float32, device=gpu)             # 4.3 GB
    X = torch.empty((cols, k), dtype=torch.float32, device=gpu)
    _fill(U, _u_formula)
    _fill(X, _x_formula)
    out = torch.full((nnz,), float("nan"), dtype=torch.float32, device=gpu)
    A = pkg.capi.CsrMatrix.from_device(rows, cols, rp.to(torch.int32), d_ci, out)
    A.spmm_plan()
    A.sddmm(U, X, out)
    torch.cuda.synchronize()
    _check_formula(out, lambda p: row_of[p], lambda p: (p * 2654435761) % cols, k, 1 << 20)
    A.close()


def test_sddmm_nnz_beyond_2_to_30(pkg, gpu):
    """4 n passes 2^32 in col_idx and out: rows of 64 nonzeros, nnz = 2^30 + 64, k = 4; every entry checked."""
    import torch
    per, k, cols = 64, 4, 4096
    rows = (1 << 24) + 1
    nnz = rows * per
    assert (1 << 30) < nnz < (1 << 31)
    d_rp = (torch.arange(rows + 1, device=gpu, dtype=torch.int64) * per).to(torch.int32)
    d_ci = torch.empty(nnz, dtype=torch.int32, device=gpu)
    for n0 in range(0, nnz, 1 << 26):
        n = torch.arange(n0, min(nnz, n0 + (1 << 26)), device=gpu, dtype=torch.int64)
        d_ci[n0:n0 + n.numel()] = ((n * 2654435761) % cols).to(torch.int32)
    del n
    U = torch.empty((rows, k), dtype=torch.float32, device=gpu)
    X = torch.empty((cols, k), dtype=torch.float32, device=gpu)
    _fill(U, _u_formula)
    _fill(X, _x_formula)
    out = torch.full((nnz,), float("nan"), dtype=torch.float32, device=gpu)
    A = pkg.capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, out)
    A.spmm_plan()
    A.sddmm(U, X, out)
    torch.cuda.synchronize()
    _check_formula(out, lambda n: n // per, lambda n: (n * 2654435761) % cols, k, 1 << 24)
    A.close()


# ---- graph capture, borrowed vals ------------------------------------------------------------------------------------------
def _small(pkg, oracle, gpu, name, k):
    import torch
    s = E.structure(name, pkg, oracle)
    dev = _Sddmm(pkg.capi, gpu, s)
    Ui = torch.from_numpy(_ints(name, s.rows, 8)).to(gpu)[:, :k].contiguous()
    Xi = torch.from_numpy(_ints(name, s.cols, 9)).to(gpu)[:, :k].contiguous()
    return s, dev, Ui, Xi


def test_sddmm_graph_capture(pkg, oracle, gpu):
    import torch
    s, dev, Ui, Xi = _small(pkg, oracle, gpu, "wave_pipe_thresholds", 24)
    want = dev.int_dots(Ui, Xi, 24).to(torch.float32)
    Ug, Xg = torch.zeros_like(Ui, dtype=torch.float32), torch.zeros_like(Xi, dtype=torch.float32)
    out = torch.full((s.nnz,), float("nan"), dtype=torch.float32, device=gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.A.sddmm(Ug, Xg, out)
    Ug.copy_(Ui)
    Xg.copy_(Xi)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    Xg.copy_(-2 * Xi)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, -2 * want)
    dev.close()


def test_sddmm_into_borrowed_vals_then_spmm(pkg, oracle, gpu):
    import torch
    import scipy.sparse as sp
    s, dev, Ui, Xi = _small(pkg, oracle, gpu, "odd_last_chunk", 8)
    dev.A.sddmm(Ui.to(torch.float32), Xi.to(torch.float32), dev.d_va)       # the handle's own borrowed vals
    dev.A.values_changed()
    X2 = torch.from_numpy(_ints("odd_last_chunk", s.cols, 10)).to(gpu)[:, :5].contiguous()
    Y = torch.full((s.rows, 5), float("nan"), dtype=torch.float32, device=gpu)
    dev.A.spmm(X2.to(torch.float32), Y)
    torch.cuda.synchronize()
    vals = dev.int_dots(Ui, Xi, 8).cpu().numpy()
    assert np.array_equal(dev.d_va.cpu().numpy(), vals.astype(np.float32))
    A = sp.csr_matrix((vals.astype(np.float64), s.ci.copy(), s.rp.copy()), shape=(s.rows, s.cols))
    want = A @ X2.cpu().numpy().astype(np.float64)
    assert np.abs(want).max() < E.EXACT_LIMIT
    assert np.array_equal(Y.cpu().numpy(), want.astype(np.float32))
    dev.close()


# ---- refusals and edges ---------------------------------------------------------------------------------------------------
def test_sddmm_refusals_leave_out_untouched(pkg, oracle, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    s = E.structure("many_tiny_rows", pkg, oracle)
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    d_va = torch.zeros(s.nnz, dtype=torch.float32, device=gpu)
    A = capi.CsrMatrix.from_device(s.rows, s.cols, d_rp, d_ci, d_va)
    U = torch.ones((s.rows, 72), dtype=torch.float32, device=gpu)
    X = torch.ones((s.cols, 72), dtype=torch.float32, device=gpu)
    out = torch.full((s.nnz,), float(SENTINEL), dtype=torch.float32, device=gpu)
    before = out.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    up, xp, op = U.data_ptr(), X.data_ptr(), out.data_ptr()
    assert lib.spmv_csr_sddmm(A._h, 4, up, 72, xp, 72, op, st) == capi.ERR_NOT_PLANNED     # before the plan
    assert "spmv_csr_sddmm" in lib.spmv_last_error().decode()
    A.spmm_plan()
    for k, ldu, ldx, uo, xo in ((0, 72, 72, 0, 0), (65, 72, 72, 0, 0), (8, 7, 72, 0, 0), (8, 72, 7, 0, 0),
                                (8, 72, 72, 4, 0), (8, 72, 72, 0, 8)):
        rc = lib.spmv_csr_sddmm(A._h, k, up + uo, ldu, xp + xo, ldx, op, st)
        assert rc == capi.ERR_INVALID, (k, ldu, ldx, uo, xo, rc)
        assert "spmv_csr_sddmm" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_sddmm(A._h, 8, up, 72, xp, 72, None, st) == capi.ERR_INVALID            # no out, nnz > 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32))
    # the wrapper checks before it calls
    with pytest.raises(ValueError):
        A.sddmm(U[:, 0], X[:, :1], out)                          # U not 2-D
    with pytest.raises(ValueError):
        A.sddmm(U[:, :4], X[:, :4].double(), out)                # X not float32
    with pytest.raises(ValueError):
        A.sddmm(torch.ones((4, s.rows), device=gpu).t(), X[:, :4], out)   # column-strided
    with pytest.raises(ValueError):
        A.sddmm(U[:-1, :4], X[:, :4], out)                       # U rows != rows
    with pytest.raises(ValueError):
        A.sddmm(U[:, :4], X[:-1, :4], out)                       # X rows != cols
    with pytest.raises(ValueError):
        A.sddmm(U[:, :4], X[:, :8], out)                         # two widths
    with pytest.raises(ValueError):
        A.sddmm(U[:, :4], X[:, :4], out[:-1])                    # out too short
    with pytest.raises(ValueError):
        A.sddmm(U[:, :4], X[:, :4], torch.cat([out, out])[::2])  # out strided
    with pytest.raises(ValueError):
        A.sddmm(U[:, :4], X[:, :4], out.view(1, -1))             # out not 1-D
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32))
    A.sddmm(U[:, :4], X[:, :4], out)                             # and the good call
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 4.0))
    A.close()


@pytest.mark.parametrize("rows,cols,nnz", [(0, 10, 0), (5, 0, 0), (7, 9, 0)])
def test_sddmm_empty_shapes(pkg, gpu, rows, cols, nnz):
    import torch
    capi = pkg.capi
    d_rp = torch.zeros(rows + 1, dtype=torch.int32, device=gpu)
    d_ci = torch.zeros(1, dtype=torch.int32, device=gpu)[:0]
    d_va = torch.zeros(1, dtype=torch.float32, device=gpu)[:0]
    A = capi.CsrMatrix.from_device(rows, cols, d_rp, d_ci, d_va)
    A.spmm_plan()
    for k in (1, 5, 64):
        U = torch.ones((rows, k), dtype=torch.float32, device=gpu)
        X = torch.ones((cols, k), dtype=torch.float32, device=gpu)
        A.sddmm(U, X, torch.empty(0, dtype=torch.float32, device=gpu))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert capi.lib().spmv_csr_sddmm(A._h, k, None if rows == 0 else U.data_ptr(), k, None if cols == 0 else X.data_ptr(), k,
                                         None, st) == capi.OK
    torch.cuda.synchronize()
    A.close()
