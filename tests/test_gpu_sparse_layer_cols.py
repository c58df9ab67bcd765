"""SparseLayer(k_max=192) on the GPU: a batch of up to 192 columns through spmv_csr_spmm_cols and spmv_csr_sddmm_cols, judged bit
for bit by the default layer (the narrow calls) run per block of 64 columns, on pattern P2 of tests/_order_cases.py, in fp32
and bf16: Y and dX block by block, dvals as the fp32 fold of the blocks' dvals in block order.  An in-place update of vals is
followed without a new plan; 193 columns are refused, and the default layer still refuses 65."""
import numpy as np
import pytest

import _cols as CO

pytestmark = pytest.mark.gpu

K_MAX = 192


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def layers(pkg, gpu):
    import torch
    s, vals, _, _ = CO.data("P2")
    d_rp, d_ci = torch.from_numpy(s.rp).to(gpu), torch.from_numpy(s.ci).to(gpu)
    v_wide = torch.from_numpy(vals).to(gpu).requires_grad_()
    v_narrow = torch.from_numpy(vals).to(gpu).requires_grad_()
    wide = pkg.sparse_layer.SparseLayer(s.rows, s.cols, d_rp, d_ci, v_wide, k_max=K_MAX)
    narrow = pkg.sparse_layer.SparseLayer(s.rows, s.cols, d_rp, d_ci, v_narrow)
    yield s, wide, narrow
    wide.close()
    narrow.close()


def _run(layer, X, dY):
    """(Y, dX, dvals) of one forward and backward."""
    layer.vals.grad = None
    X = X.detach().clone().requires_grad_()
    Y = layer(X)
    Y.backward(dY)
    return Y.detach(), X.grad, layer.vals.grad.clone()


def _compare(s, wide, narrow, X, dY, what):
    import torch
    k = X.shape[1]
    Y, dX, dvals = _run(wide, X, dY)
    assert Y.dtype == X.dtype and dX.dtype == X.dtype and dvals.dtype == torch.float32
    parts = []
    for a, b in CO.tiles(k):
        Yb, dXb, dvb = _run(narrow, X[:, a:b].contiguous(), dY[:, a:b].contiguous())
        assert np.array_equal(_bits(Y[:, a:b]), _bits(Yb)), f"{what}: Y differs from the default layer on columns [{a}, {b})"
        assert np.array_equal(_bits(dX[:, a:b]), _bits(dXb)), f"{what}: dX differs from the default layer on columns [{a}, {b})"
        parts.append(dvb.cpu().numpy())
    want = CO.fold(parts)
    assert not np.isnan(want).any()
    assert np.array_equal(dvals.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{what}: dvals is not the fold of the blocks' dvals"
    return Y


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
@pytest.mark.parametrize("k", (65, 130, K_MAX))
def test_wide_layer_is_the_default_layer_block_by_block(layers, gpu, k, dtype):
    import torch
    s, wide, narrow = layers
    g = torch.Generator(device=gpu).manual_seed(2400 + k)
    X = torch.randn((s.cols, k), generator=g, device=gpu).to(getattr(torch, dtype))
    dY = torch.randn((s.rows, k), generator=g, device=gpu).to(getattr(torch, dtype))
    _compare(s, wide, narrow, X, dY, f"{dtype} k = {k}")


def test_an_in_place_update_of_vals_is_followed_without_a_new_plan(layers, gpu):
    import torch
    s, wide, narrow = layers
    g = torch.Generator(device=gpu).manual_seed(2401)
    X = torch.randn((s.cols, 130), generator=g, device=gpu)
    dY = torch.randn((s.rows, 130), generator=g, device=gpu)
    before = _compare(s, wide, narrow, X, dY, "before the update")
    bytes_before = wide.A.spmm_plan_bytes()
    try:
        with torch.no_grad():
            for layer in (wide, narrow):
                layer.vals.mul_(-0.75).add_(0.125)
        after = _compare(s, wide, narrow, X, dY, "after the update")
        assert not torch.equal(before, after), "the forward pass did not follow the new values"
        assert wide.A.spmm_plan_bytes() == bytes_before
    finally:
        with torch.no_grad():
            for layer in (wide, narrow):
                layer.vals.copy_(torch.from_numpy(CO.data("P2")[1]).to(gpu))


def test_width_limits(layers, gpu):
    import torch
    s, wide, narrow = layers
    with pytest.raises(ValueError, match="193 columns"):
        wide(torch.zeros((s.cols, K_MAX + 1), device=gpu))
    with pytest.raises(ValueError, match="65 columns"):
        narrow(torch.zeros((s.cols, 65), device=gpu))
    assert wide(torch.zeros((s.cols, 1), device=gpu)).shape == (s.rows, 1)
