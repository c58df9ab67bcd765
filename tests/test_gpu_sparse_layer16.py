"""sparse_layer.SparseLayer / SparseMatmul on bf16 and fp16 activations: X, Y, dY and dX in the 16-bit dtype, ``vals`` and
dvals float32, on spmv_csr_spmm_16 (forward), spmv_csr_transpose_values + spmv_csr_spmm_16 on A^T (dX) and spmv_csr_sddmm_16
(dvals).

Small integers that are exact in the dtype (values, X and the upstream gradient in [-4, 4], K = 16) on the two patterns of
tests/test_gpu_sparse_layer.py, so every fp32 sum of every order is an exact integer below 2^24 (|Y| <= 4100 * 16): Y and dX
must equal the dense float64 torch autograd on the widened operands converted once to the dtype -- that one rounding is the
whole difference -- and dvals the same autograd's as float32, all bit for bit (+0 and -0 folded, as the fp32 test folds them).
Two steps with ``vals`` rewritten in place and no new plan; the layer's results equal the direct CsrMatrix calls; a float32 X
on the same layer still gives float32 results; mixed dtypes raise ValueError."""
import numpy as np
import pytest

import _exact as E

pytestmark = pytest.mark.gpu

K = 16
NAMES = ("odd_last_chunk", "wave_pipe_thresholds")


def _dtypes():
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16}


def _bits(t):
    """The bits with -0 folded into +0 (int16 for a 16-bit tensor, int32 for float32)."""
    import torch
    return (t + 0.0).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _ints(gpu, seed, shape, dtype, nonzero=False):
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(1, 5, size=shape) * rng.choice([-1, 1], size=shape) if nonzero else rng.integers(-4, 5, size=shape)
    t = torch.from_numpy(a.astype(np.float32)).to(gpu).to(dtype)
    assert torch.equal(t.to(torch.float32).cpu(), torch.from_numpy(a.astype(np.float32))), "exact in the dtype"
    return t


@pytest.fixture(scope="module")
def reference(pkg, oracle, gpu):
    """(Y, dX, dvals) in float64 of Y = A X with upstream gradient G, by a dense matrix and torch's own autograd: computed
    once per (pattern, vals, X, G), shared by both dtypes (their operands are the same integers) and left unchanged."""
    import torch
    cache = {}

    def get(name, key, vals, X, G):
        if (name, key) not in cache:
            s = E.structure(name, pkg, oracle)
            v = vals.detach().to(torch.float64).requires_grad_(True)
            x = X.detach().to(torch.float64).requires_grad_(True)
            r = torch.from_numpy(s.row_of).to(gpu)
            c = torch.from_numpy(s.ci.astype(np.int64)).to(gpu)
            D = torch.zeros((s.rows, s.cols), dtype=torch.float64, device=gpu).index_put((r, c), v, accumulate=True)
            Y = D @ x
            Y.backward(G.to(torch.float64))
            assert float(Y.detach().abs().max()) < 2 ** 24 and float(x.grad.abs().max()) < 2 ** 24
            cache[(name, key)] = (Y.detach().cpu(), x.grad.cpu(), v.grad.cpu())
        return [t.to(gpu) for t in cache[(name, key)]]

    return get


@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
@pytest.mark.parametrize("name", NAMES)
def test_sparse_layer_16bit_matches_dense_autograd(pkg, oracle, gpu, reference, name, fmt):
    import torch
    SL = pkg.sparse_layer
    dt, f32 = _dtypes()[fmt], torch.float32
    s = E.structure(name, pkg, oracle)
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    vals = _ints(gpu, 1, s.nnz, f32, nonzero=True).requires_grad_(True)
    layer = SL.SparseLayer(s.rows, s.cols, d_rp, d_ci, vals)
    plans = (layer.A.spmm_describe(), layer.T.spmm_describe(), layer.A.spmm_plan_bytes(), layer.T.spmm_plan_bytes())
    for step in range(2):
        X = _ints(gpu, 10 + step, (s.cols, K), dt).requires_grad_(True)
        G = _ints(gpu, 20 + step, (s.rows, K), dt)
        vals.grad = None
        Y = layer(X)
        Y.backward(G)
        torch.cuda.synchronize()
        assert Y.dtype == dt and X.grad.dtype == dt and vals.grad.dtype == f32 and vals.dtype == f32
        assert Y.shape == (s.rows, K) and X.grad.shape == X.shape and vals.grad.shape == vals.shape
        Yd, dXd, dvd = reference(name, step, vals, X, G)
        assert torch.equal(_bits(Y.detach()), _bits(Yd.to(dt))), f"step {step}: Y differs"           # the one rounding
        assert torch.equal(_bits(X.grad), _bits(dXd.to(dt))), f"step {step}: dX differs"
        assert torch.equal(_bits(vals.grad), _bits(dvd.to(f32))), f"step {step}: dvals differs"
        # the layer is the three direct calls
        Y2 = torch.empty((s.rows, K), dtype=dt, device=gpu)
        dX2 = torch.empty((s.cols, K), dtype=dt, device=gpu)
        dv2 = torch.empty(s.nnz, dtype=f32, device=gpu)
        layer.A.spmm(X.detach(), Y2)
        layer.T.transpose_values(layer.A)
        layer.T.spmm(G, dX2)
        layer.A.sddmm(G, X.detach(), dv2)
        torch.cuda.synchronize()
        assert torch.equal(Y2.view(torch.int16), Y.detach().view(torch.int16))
        assert torch.equal(dX2.view(torch.int16), X.grad.view(torch.int16))
        assert torch.equal(dv2.view(torch.int32), vals.grad.view(torch.int32))
        # an optimizer step: the borrowed values rewritten in place, no new plan
        vals.data.copy_(_ints(gpu, 30 + step, s.nnz, f32, nonzero=True))
    assert (layer.A.spmm_describe(), layer.T.spmm_describe(), layer.A.spmm_plan_bytes(), layer.T.spmm_plan_bytes()) == plans
    # a float32 X on the same layer still gives float32 results, the same numbers (they are exact)
    X32 = X.detach().to(f32).requires_grad_(True)
    vals.grad = None
    Y32 = layer(X32)
    Y32.backward(G.to(f32))
    torch.cuda.synchronize()
    assert Y32.dtype == f32 and X32.grad.dtype == f32 and vals.grad.dtype == f32
    Yd, dXd, dvd = reference(name, "f32", vals, X32, G)
    assert torch.equal(_bits(Y32.detach()), _bits(Yd.to(f32))) and torch.equal(_bits(X32.grad), _bits(dXd.to(f32)))
    assert torch.equal(_bits(vals.grad), _bits(dvd.to(f32)))
    # an unaligned 16-bit X (rows of 17 elements from an odd one) is copied, not refused
    wide = torch.zeros((s.cols, K + 1), dtype=dt, device=gpu)
    wide[:, 1:] = X.detach()
    assert wide[:, 1:].data_ptr() % 8 != 0
    assert torch.equal(layer(wide[:, 1:]).detach().view(torch.int16), layer(X.detach()).detach().view(torch.int16))
    # mixed dtypes
    other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
    Yo = layer(X.detach().clone().requires_grad_(True))
    for bad in (other, f32):
        with pytest.raises(ValueError, match="dY is"):
            SL.SparseMatmul.backward(Yo.grad_fn, G.to(bad))
    with pytest.raises(ValueError):
        layer.A.spmm(X.detach(), torch.empty((s.rows, K), dtype=other, device=gpu))
    with pytest.raises(ValueError):
        layer.A.sddmm(G, X.detach().to(other), torch.empty(s.nnz, dtype=f32, device=gpu))
    with pytest.raises(ValueError):
        layer.A.sddmm(G, X.detach(), torch.empty(s.nnz, dtype=dt, device=gpu))
    with pytest.raises(ValueError):
        layer(torch.zeros((s.cols, 65), dtype=dt, device=gpu))
    with pytest.raises(ValueError):
        layer(torch.zeros((s.cols, K), dtype=torch.float64, device=gpu))
    layer.close()
