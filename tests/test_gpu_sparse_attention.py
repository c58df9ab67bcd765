"""sparse_attention.SparseAttention on the GPU: O = softmax_rows(scale * Q K^T at the pattern) V and its gradients, on
spmv_csr_sddmm, spmv_csr_row_softmax(_backward), spmv_csr_spmm and the transposed handle.

exact      a pattern whose every row length is a power of two between 1 and 16; V and the upstream gradient dO integers in
           [-4, 4], k = kv = 8, scale = 2^-2.  With Q = 0 (K integer) or K = 0 (Q integer) every score is 0, so P = 2^-m
           exactly and O, dV, dQ and dK are sums of at most 22 significant bits: every order is exact, and all four must
           equal torch's own fp64 dense autograd of the same masked softmax attention bit for bit (+0 and -0 folded).
           Q = 0 exercises dQ and dV, K = 0 exercises dK.  A second pass with new data runs without a new plan.
general    two patterns of tests/_exact.py, random normal Q, K and V, k = 24.  O is within (_util.RTOL + the parity bound
           of the softmax, (2 D + 12 + A(L)) 2^-24) * sum |P v| of fp64 (the rounding of the fp32 scores themselves, at most
           7 2^-24 sum |q k| scale in the exponent, is left to RTOL).  Every gradient's error against the fp64 dense
           autograd, divided by the fp64 magnitude of the same chain taken with absolute values, is at most 4 times what
           torch's own fp32 dense autograd shows on the same data under the same normalisation, and not held below RTOL:
           a different order of the sums at equal precision may differ by a small factor.  Both figures are printed.
refusals   k = 65, wrong shapes and a scale that is not finite raise ValueError.
"""
import numpy as np
import pytest

import _exact as E
import _softmax as SM
from _util import RTOL

pytestmark = pytest.mark.gpu


def _bits(t):
    import torch
    return (t + 0.0).view(torch.int32)


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


def _mask(s, gpu):
    import torch
    m = torch.zeros((s.rows, s.cols), dtype=torch.bool, device=gpu)
    m[torch.from_numpy(s.row_of).to(gpu), torch.from_numpy(s.ci.astype(np.int64)).to(gpu)] = True
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


def _attention(pkg, s, gpu, scale):
    import torch
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    return pkg.sparse_attention.SparseAttention(s.rows, s.cols, d_rp, d_ci, scale=scale)


def test_sparse_attention_exact_against_dense_fp64_autograd(pkg, gpu):
    import torch
    s = _pow2_pattern(3000, 2000, 5)
    assert set(np.diff(s.rp)) == {1, 2, 4, 8, 16}
    att = _attention(pkg, s, gpu, 2.0 ** -2)
    plans = (att.A.spmm_describe(), att.T.spmm_describe())
    mask = _mask(s, gpu)
    for step, zero in enumerate(("Q", "K", "Q", "K")):       # the second pair: new data, no new plan
        Q, K = _ints(gpu, 10 + step, (s.rows, 8)), _ints(gpu, 20 + step, (s.cols, 8))
        V, dO = _ints(gpu, 30 + step, (s.cols, 8)), _ints(gpu, 40 + step, (s.rows, 8))
        (Q if zero == "Q" else K).zero_()
        Q.requires_grad_(True), K.requires_grad_(True), V.requires_grad_(True)
        O = att(Q, K, V)
        O.backward(dO)
        torch.cuda.synchronize()
        Od, dQd, dKd, dVd, _ = _dense_autograd(mask, att.scale, Q, K, V, dO, torch.float64)
        for what, got, want in (("O", O.detach(), Od), ("dQ", Q.grad, dQd), ("dK", K.grad, dKd), ("dV", V.grad, dVd)):
            assert got.shape == want.shape and got.dtype == torch.float32
            assert torch.equal(want.to(torch.float32).to(torch.float64), want), f"{what}: the expectation is not an fp32 number"
            assert torch.equal(_bits(got), _bits(want.to(torch.float32))), f"step {step} ({zero} = 0): {what} differs"
        assert bool((Q.grad if zero == "K" else K.grad).eq(0).all())
        assert bool((K.grad if zero == "K" else Q.grad).ne(0).any()) and bool(V.grad.ne(0).any())
    assert (att.A.spmm_describe(), att.T.spmm_describe()) == plans
    # only some of the gradients asked for
    Q, K, V = _ints(gpu, 50, (s.rows, 8)).zero_(), _ints(gpu, 51, (s.cols, 8)), _ints(gpu, 52, (s.cols, 8)).requires_grad_(True)
    att(Q, K, V).backward(dO)
    torch.cuda.synchronize()
    assert Q.grad is None and K.grad is None
    assert torch.equal(_bits(V.grad), _bits(_dense_autograd(mask, att.scale, Q, K, V, dO, torch.float64)[3].to(torch.float32)))
    # refusals
    z = lambda r, c: torch.zeros((r, c), dtype=torch.float32, device=gpu)       # noqa: E731
    for q, k, v in ((z(s.rows, 65), z(s.cols, 65), z(s.cols, 8)), (z(s.rows, 8), z(s.cols, 8), z(s.cols, 65)),
                    (z(s.rows + 1, 8), z(s.cols, 8), z(s.cols, 8)), (z(s.rows, 8), z(s.cols - 1, 8), z(s.cols, 8)),
                    (z(s.rows, 8), z(s.cols, 8), z(s.rows + 7, 8)), (z(s.rows, 8), z(s.cols, 4), z(s.cols, 8)),
                    (z(s.rows, 8).double(), z(s.cols, 8), z(s.cols, 8)), (z(s.rows, 8), z(s.cols, 8), z(s.cols, 8)[:, 0])):
        with pytest.raises(ValueError):
            att(q, k, v)
    with pytest.raises(ValueError):
        pkg.sparse_attention.SparseAttention(s.rows, s.cols, att.A._keep[0], att.A._keep[1], scale=float("inf"))
    att.close()


@pytest.mark.parametrize("name", ["odd_last_chunk", "wave_pipe_thresholds"])
def test_sparse_attention_general_against_dense_autograd(pkg, oracle, gpu, name):
    import torch
    s = E.structure(name, pkg, oracle)
    k, scale = 24, 2.0 ** -2
    att = _attention(pkg, s, gpu, scale)
    mask = _mask(s, gpu)
    gen = torch.Generator(device=gpu).manual_seed(len(name))
    Q, K, V = (torch.randn((n, k), generator=gen, device=gpu, dtype=torch.float32).requires_grad_(True)
               for n in (s.rows, s.cols, s.cols))
    dO = torch.randn((s.rows, k), generator=gen, device=gpu, dtype=torch.float32)
    O = att(Q, K, V)
    O.backward(dO)
    torch.cuda.synchronize()
    O64, dQ64, dK64, dV64, P = _dense_autograd(mask, scale, Q, K, V, dO, torch.float64)
    _, dQ32, dK32, dV32, _ = _dense_autograd(mask, scale, Q, K, V, dO, torch.float32)
    # O: RTOL and the softmax's parity bound, relative to sum |P v|
    t = torch.where(mask, (Q.detach().double() @ K.detach().double().t()) * scale, torch.tensor(float("nan"), dtype=torch.float64, device=gpu))
    L = mask.sum(1)
    D = torch.where(L > 0, torch.nan_to_num(t, nan=-1e300).max(1).values - torch.nan_to_num(t, nan=1e300).min(1).values, torch.zeros_like(L, dtype=torch.float64))
    assert float(D.max()) <= 32.0
    chain = torch.from_numpy(SM.chain(L.cpu().numpy()).astype(np.float64)).to(gpu)
    rel = RTOL + (2.0 * D + 12.0 + chain) * SM.EPS
    err = (O.detach().double() - O64).abs()
    bound = rel[:, None] * (P @ V.detach().double().abs()) + 1e-37
    assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} entries of O outside the bound"
    assert bool((O.detach()[L == 0] == 0).all())
    # the gradients: error / the magnitude of the chain taken with absolute values, against torch's fp32 dense autograd
    aQ, aK, aV, adO = (x.detach().double().abs() for x in (Q, K, V, dO))
    dP_abs = torch.where(mask, adO @ aV.t(), torch.zeros((), dtype=torch.float64, device=gpu))
    dS_abs = abs(scale) * P * (dP_abs + (P * dP_abs).sum(1, keepdim=True))
    mags = {"dQ": dS_abs @ aK, "dK": dS_abs.t() @ aQ, "dV": P.t() @ adO}
    for what, got, g32, g64 in (("dQ", Q.grad, dQ32, dQ64), ("dK", K.grad, dK32, dK64), ("dV", V.grad, dV32, dV64)):
        mag = mags[what]
        live = mag > 0
        assert bool((got[~live] == 0).all()), f"{what}: a gradient where nothing contributes"
        ours = float(((got.double() - g64).abs()[live] / mag[live]).max())
        yard = float(((g32.double() - g64).abs()[live] / mag[live]).max())
        print(f"{name} {what}: normalised error {ours:.3g}, torch fp32 dense autograd {yard:.3g}")
        assert ours <= max(4.0 * yard, RTOL), f"{name} {what}: {ours:.3g} against {yard:.3g} of torch's fp32 dense autograd"
    att.close()
