"""Y = A X as a differentiable torch operation, on the three primitives of include/spmv_hip.h that a sparse layer needs:

    forward    Y     = A X                 spmv_csr_spmm on A
    backward   dX    = A^T dY              spmv_csr_spmm on T = transpose(A), its values refreshed by spmv_csr_transpose_values
               dvals = (dY X^T) at A's pattern     spmv_csr_sddmm on A

Plumbing that shows the primitives compose, not a framework: one device, a batch of k <= 64 columns -- or, for a layer made
with ``k_max``, of up to k_max columns through the _cols calls of the same primitives (spmv_csr_spmm_cols and
spmv_csr_sddmm_cols: column tiles of 64 in one call, every column's bits the narrow call's).  X may be float32, or
bfloat16 or float16 (the _16 calls of the same primitives): Y and dX then have X's dtype, rounded once at their store, while
``vals`` and dvals stay float32 and every sum is the fp32 call's.  Every product runs in the HIP library; there is no torch
fallback.
"""
from __future__ import annotations

import torch

from . import capi

MAX_K = 64


_DTYPES_16 = (torch.bfloat16, torch.float16)


def _operand(t, name: str, rows: int, like=None, max_k=None):
    """t as the library takes it: 2-D float32 (or bfloat16 / float16), stride(1) == 1, stride(0) >= k, 16-byte aligned (a
    16-bit tensor: 8-byte), copied if it is not.  like: the tensor whose dtype t must share (dY against X).  max_k: the
    layer's k_max (None: MAX_K, the narrow calls)."""
    max_k = MAX_K if max_k is None else max_k
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or (t.dtype != torch.float32 and t.dtype not in _DTYPES_16):
        raise ValueError(f"SparseMatmul: {name} must be a 2-D float32 tensor")
    if like is not None and t.dtype != like.dtype:
        raise ValueError(f"SparseMatmul: {name} is {t.dtype}, X was {like.dtype}")
    if t.shape[0] != rows:
        raise ValueError(f"SparseMatmul: {name} has {t.shape[0]} rows, the matrix needs {rows}")
    if not 1 <= t.shape[1] <= max_k:
        raise ValueError(f"SparseMatmul: {name} has {t.shape[1]} columns (1 <= k <= {max_k})")
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.data_ptr() % (8 if t.dtype in _DTYPES_16 else 16) == 0:
        return t
    return torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)


class SparseMatmul(torch.autograd.Function):
    """``SparseMatmul.apply(layer, vals, X)`` = A X with A's values ``vals`` (the leaf ``layer`` borrows)."""

    @staticmethod
    def forward(ctx, layer, vals, X):
        X = _operand(X, "X", layer.A.cols, max_k=layer.k_max)
        Y = torch.empty((layer.A.rows, X.shape[1]), dtype=X.dtype, device=X.device)
        layer._forward(X, Y)
        ctx.layer = layer
        ctx.save_for_backward(X)
        return Y

    @staticmethod
    def backward(ctx, dY):
        layer = ctx.layer
        X, = ctx.saved_tensors
        dY = _operand(dY, "dY", layer.A.rows, like=X, max_k=layer.k_max)
        dvals = dX = None
        if ctx.needs_input_grad[1]:
            dvals = torch.empty(layer.A.nnz, dtype=torch.float32, device=dY.device)
            layer._dvals(dY, X, dvals)
        if ctx.needs_input_grad[2]:
            dX = torch.empty((layer.A.cols, dY.shape[1]), dtype=dY.dtype, device=dY.device)
            layer.T.transpose_values(layer.A)      # A's values as they are now
            layer._dx(dY, dX)
        return None, dvals, dX


class SparseLayer:
    """A rows x cols CSR matrix whose values are a torch leaf.  Borrows ``row_ptr``, ``col_idx`` (int32) and ``vals``
    (float32, may require grad), all on one device; owns the handle of A, of T = A^T (with the map that refreshes T's
    values) and both SpMM plans.  The pattern is fixed; ``vals`` may be updated in place (an optimizer step): the next
    forward and backward follow the new values without a new plan.  X may be float32, bfloat16 or float16 from one call to
    the next; ``vals`` and its gradient are float32 always.  ``k_max`` (an int from 1 to capi.COLS_MAX_K): the layer takes
    1 .. k_max columns, both handles are planned with spmm_plan_cols(k_max) and forward, dX and dvals go through the _cols
    calls; None (the default) is the layer of the narrow calls, 1 .. MAX_K columns."""

    def __init__(self, rows: int, cols: int, row_ptr, col_idx, vals, k_max=None):
        if k_max is not None and (isinstance(k_max, bool) or not isinstance(k_max, int) or not 1 <= k_max <= capi.COLS_MAX_K):
            raise ValueError(f"SparseLayer: k_max must be None or an int in [1, {capi.COLS_MAX_K}], not {k_max!r}")
        self.k_max = k_max
        self.vals = vals
        self.A = capi.CsrMatrix.from_device(rows, cols, row_ptr, col_idx, vals)
        self.T = self.A.transpose(keep_map=True)
        # the narrow calls or the _cols calls, chosen here once: what SparseMatmul runs for Y, dvals and dX
        if k_max is None:
            self.A.spmm_plan()
            self.T.spmm_plan()
            self._forward, self._dvals, self._dx = self.A.spmm, self.A.sddmm, self.T.spmm
        else:
            self.A.spmm_plan_cols(k_max)
            self.T.spmm_plan_cols(k_max)
            self._forward, self._dvals, self._dx = self.A.spmm_cols, self.A.sddmm_cols, self.T.spmm_cols

    def __call__(self, X):
        return SparseMatmul.apply(self, self.vals, X)

    def pruned(self, k: int) -> "SparseLayer":
        """A new SparseLayer on the per-row top-k of ``|vals|`` (spmv_csr_select_topk with SPMV_SELECT_ABS: magnitude pruning,
        ties to the earlier nonzero, rows in their storage order).  Its ``row_ptr`` and ``col_idx`` are fresh device tensors
        and its ``vals`` a fresh leaf (requires_grad as the parent's) filled by select_gather; ``.selection`` is the select
        handle with its map, so a caller can bring optimizer state along the same way
        (``new.selection.select_gather(state, new_state)``) or scatter a gradient back.  The parent layer is untouched."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"SparseLayer.pruned: k = {k!r} (an int >= 1)")
        sel = self.A.select_topk(k, abs=True, keep_map=True)
        dev = self.vals.device
        row_ptr = torch.empty(sel.rows + 1, dtype=torch.int32, device=dev)
        col_idx = torch.empty(sel.nnz, dtype=torch.int32, device=dev)
        vals = torch.empty(sel.nnz, dtype=torch.float32, device=dev)
        sel.copy_arrays(row_ptr, col_idx)
        sel.select_gather(self.vals.detach(), vals)
        vals.requires_grad_(self.vals.requires_grad)
        layer = SparseLayer(sel.rows, sel.cols, row_ptr, col_idx, vals, k_max=self.k_max)
        layer.selection = sel
        return layer

    def composed(self, first: "SparseLayer") -> "SparseLayer":
        """A new SparseLayer on ``self.A @ first.A`` (spmv_csr_spgemm), so that ``new(X)`` approximates ``self(first(X))`` --
        two layers without an activation between them folded into one; the sums are taken in another order, so the bits
        differ.  Its ``row_ptr`` and ``col_idx`` are fresh device tensors (copy_arrays) and its ``vals`` a fresh leaf
        (requires_grad as this layer's); ``k_max`` is this layer's.  No gradient flows to the parents, which are untouched."""
        if not isinstance(first, SparseLayer):
            raise ValueError("SparseLayer.composed: first must be a SparseLayer")
        if self.A.cols != first.A.rows:
            raise ValueError(f"SparseLayer.composed: self is {self.A.rows} x {self.A.cols}, first is {first.A.rows} x {first.A.cols} "
                             "(self's columns must be first's rows)")
        prod = self.A.spgemm(first.A)
        try:
            dev = self.vals.device
            row_ptr = torch.empty(prod.rows + 1, dtype=torch.int32, device=dev)
            col_idx = torch.empty(prod.nnz, dtype=torch.int32, device=dev)
            vals = torch.empty(prod.nnz, dtype=torch.float32, device=dev)
            prod.copy_arrays(row_ptr, col_idx, vals)
            torch.cuda.current_stream().synchronize()      # the copies are done before the product's arrays are freed
            rows, cols = prod.rows, prod.cols
        finally:
            prod.close()
        vals.requires_grad_(self.vals.requires_grad)
        return SparseLayer(rows, cols, row_ptr, col_idx, vals, k_max=self.k_max)

    def _on_sum(self, c) -> "SparseLayer":
        """A new layer on fresh copies of the arrays of the sum handle ``c`` (vals a fresh leaf, requires_grad as this layer's)."""
        dev = self.vals.device
        row_ptr = torch.empty(c.rows + 1, dtype=torch.int32, device=dev)
        col_idx = torch.empty(c.nnz, dtype=torch.int32, device=dev)
        vals = torch.empty(c.nnz, dtype=torch.float32, device=dev)
        c.copy_arrays(row_ptr, col_idx, vals)
        torch.cuda.current_stream().synchronize()      # the copies are done before the sum's arrays may be freed
        vals.requires_grad_(self.vals.requires_grad)
        return SparseLayer(c.rows, c.cols, row_ptr, col_idx, vals, k_max=self.k_max)

    def grown(self, row_ptr, col_idx) -> "SparseLayer":
        """A new SparseLayer on the union of this layer's pattern with the given one (int32 device tensors of rows + 1 and of
        nnz' elements; spmv_csr_add(A, G, 1, 0, SPMV_ADD_UNION)): the counterpart of :meth:`pruned`.  The old values are carried
        bit for bit (this layer's rows must be free of repeated columns for that: a repeated column's values are added), the
        new positions start at +0, the rows come out sorted.  Its ``vals`` is a fresh leaf (requires_grad as the parent's);
        ``.growth`` is the sum handle with its plan, so optimizer state follows: ``new.growth.add_values(old.A, G, 1, 0)`` with
        a handle on the state in place of the values, or ``new.growth.add_gather(0, new_state, old_state)`` back.  The parent
        layer is untouched."""
        for name, t in (("row_ptr", row_ptr), ("col_idx", col_idx)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() \
                    or t.device != self.vals.device:
                raise ValueError(f"SparseLayer.grown: {name} must be a contiguous 1-D int32 tensor on {self.vals.device}")
        if row_ptr.numel() != self.A.rows + 1:
            raise ValueError(f"SparseLayer.grown: row_ptr holds {row_ptr.numel()} elements, the layer has {self.A.rows} rows")
        zeros = torch.zeros(col_idx.numel(), dtype=torch.float32, device=self.vals.device)
        G = capi.CsrMatrix.from_device(self.A.rows, self.A.cols, row_ptr, col_idx, zeros)
        try:
            growth = self.A.add(G, 1.0, 0.0, "union", keep_plan=True)
        finally:
            G.close()
        layer = self._on_sum(growth)
        layer.growth = growth
        return layer

    def summed(self, other: "SparseLayer", alpha: float = 1.0, beta: float = 1.0) -> "SparseLayer":
        """A new SparseLayer on ``alpha * self.A + beta * other.A`` (spmv_csr_add on the union of the two patterns), so that
        ``new(X)`` approximates ``alpha * self(X) + beta * other(X)``; the sums are taken in another order, so the bits differ.
        Its arrays are fresh device tensors and its ``vals`` a fresh leaf (requires_grad as this layer's); ``k_max`` is this
        layer's.  No gradient flows to the parents, which are untouched."""
        if not isinstance(other, SparseLayer):
            raise ValueError("SparseLayer.summed: other must be a SparseLayer")
        if (self.A.rows, self.A.cols) != (other.A.rows, other.A.cols):
            raise ValueError(f"SparseLayer.summed: self is {self.A.rows} x {self.A.cols}, other is {other.A.rows} x {other.A.cols}")
        c = self.A.add(other.A, alpha, beta, "union")
        try:
            return self._on_sum(c)
        finally:
            c.close()

    def close(self) -> None:
        for name in ("selection", "growth"):
            h = getattr(self, name, None)
            if h is not None:
                h.close()
        self.T.close()
        self.A.close()
