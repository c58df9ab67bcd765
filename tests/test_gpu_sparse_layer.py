"""sparse_layer.SparseLayer / SparseMatmul on the GPU: Y = A X with A's values a torch leaf, on spmv_csr_spmm (forward),
spmv_csr_transpose_values + spmv_csr_spmm on A^T (dX) and spmv_csr_sddmm (dvals).

Integer data (values, X and the upstream gradient in [-4, 4], k = 24) on two patterns of tests/_exact.py, so that every sum
of every order is exact in fp32 (|Y| <= 4100 * 16, far below 2^24): Y, dX and dvals must equal the dense float64 torch
autograd of the same product bit for bit after the cast (+0 and -0 folded).  Then vals.data is rewritten in place, as an
optimizer step does, and a second forward and backward is exact again without a new plan.  Batches wider than 64 columns
are refused with ValueError."""
import numpy as np
import pytest

import _exact as E

pytestmark = pytest.mark.gpu

K = 24


def _bits(t):
    import torch
    return (t + 0.0).view(torch.int32)


def _ints(gpu, seed, shape, nonzero=False):
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(1, 5, size=shape) * rng.choice([-1, 1], size=shape) if nonzero else rng.integers(-4, 5, size=shape)
    return torch.from_numpy(a.astype(np.float32)).to(gpu)


def _dense_autograd(s, gpu, vals, X, G):
    """(Y, dX, dvals) of Y = A X with upstream gradient G, by a dense float64 matrix and torch's own autograd."""
    import torch
    v = vals.detach().to(torch.float64).requires_grad_(True)
    x = X.detach().to(torch.float64).requires_grad_(True)
    r = torch.from_numpy(s.row_of).to(gpu)
    c = torch.from_numpy(s.ci.astype(np.int64)).to(gpu)
    D = torch.zeros((s.rows, s.cols), dtype=torch.float64, device=gpu).index_put((r, c), v, accumulate=True)
    Y = D @ x
    Y.backward(G.to(torch.float64))
    return Y.detach().to(torch.float32), x.grad.to(torch.float32), v.grad.to(torch.float32)


@pytest.mark.parametrize("name", ["odd_last_chunk", "wave_pipe_thresholds"])
def test_sparse_layer_matches_dense_autograd(pkg, oracle, gpu, name):
    import torch
    SL = pkg.sparse_layer
    s = E.structure(name, pkg, oracle)
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    vals = _ints(gpu, 1, s.nnz, nonzero=True).requires_grad_(True)
    layer = SL.SparseLayer(s.rows, s.cols, d_rp, d_ci, vals)
    plans = (layer.A.spmm_describe(), layer.T.spmm_describe())
    for step in range(2):
        X = _ints(gpu, 10 + step, (s.cols, K)).requires_grad_(True)
        G = _ints(gpu, 20 + step, (s.rows, K))
        vals.grad = None
        Y = layer(X)
        Y.backward(G)
        torch.cuda.synchronize()
        Yd, dXd, dvd = _dense_autograd(s, gpu, vals, X, G)
        assert Y.shape == (s.rows, K) and X.grad.shape == X.shape and vals.grad.shape == vals.shape
        assert torch.equal(_bits(Y.detach()), _bits(Yd)), f"step {step}: Y differs"
        assert torch.equal(_bits(X.grad), _bits(dXd)), f"step {step}: dX differs"
        assert torch.equal(_bits(vals.grad), _bits(dvd)), f"step {step}: dvals differs"
        # an optimizer step: the borrowed values rewritten in place, no new plan
        vals.data.copy_(_ints(gpu, 30 + step, s.nnz, nonzero=True))
    assert (layer.A.spmm_describe(), layer.T.spmm_describe()) == plans
    # only one of the two gradients asked for
    Xn = _ints(gpu, 40, (s.cols, K))
    vals.grad = None
    layer(Xn).backward(G)
    torch.cuda.synchronize()
    assert Xn.grad is None and torch.equal(_bits(vals.grad), _bits(_dense_autograd(s, gpu, vals, Xn, G)[2]))
    with pytest.raises(ValueError):
        layer(torch.zeros((s.cols, 65), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        layer(torch.zeros((s.cols + 1, 8), dtype=torch.float32, device=gpu))
    layer.close()
