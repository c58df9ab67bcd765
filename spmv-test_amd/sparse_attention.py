"""O = softmax_rows(scale * (Q K^T at the pattern)) V as a differentiable torch operation, on the primitives of
include/spmv_hip.h that a sparse (or graph) attention needs, all on one pattern, one SpMM plan and one transposed handle:

    forward    S  = Q K^T at A's pattern          spmv_csr_sddmm on A, into the work buffer A borrows as vals
               P  = softmax of scale * S per row  spmv_csr_row_softmax, in place
               O  = P V                           spmv_csr_spmm on A
    backward   dV = P^T dO                        spmv_csr_transpose_values + spmv_csr_spmm on T = transpose(A)
               dP = dO V^T at the pattern         spmv_csr_sddmm on A, into the work buffer
               dS = scale * P * (dP - sum P dP)   spmv_csr_row_softmax_backward, dS over dP
               dQ = dS K                          spmv_csr_spmm on A
               dK = dS^T Q                        spmv_csr_transpose_values + spmv_csr_spmm on T

Plumbing that shows the primitives compose, not a framework: fp32, one device, one head, k and kv <= 64.  Every product
and the softmax run in the HIP library; there is no torch fallback.  The only temporaries of nnz floats are the work
buffer and the clone of P that the backward pass needs.

FusedSparseAttention is the same operation on the three fused passes (spmv_csr_attention_forward, _backward_q on A and
_backward_kv on T = transpose(A), include/spmv_hip.h "Fused attention"): nothing of nnz floats is written, saved or read
but col_idx, so one holder serves any number of heads: one after the other (heads="loop", the default) or all in one launch
per kernel (heads="batched": spmv_csr_attention_*_heads).  Both give the same bits.  Grouped-query heads (GQA: K and V
with H_kv heads, H % H_kv == 0) run on spmv_csr_attention_*_gqa: K and V are not expanded, dK and dV come back per K/V head.
Q, K and V may also be all torch.bfloat16 or all torch.float16 (spmv_csr_attention_*_16: 16-bit storage, fp32 sums, every output
rounded once); O and the gradients then have that dtype, stats and delta stay float32.  The composed SparseAttention is fp32 only.
FusedSparseAttention(..., bias=True) adds a float32 number per nonzero (and head) to the score before the softmax, with its
gradient (spmv_csr_attention_*_bias): of nnz size a step then holds the bias, its copy in T's order and dBias, nothing else.
"""
from __future__ import annotations

import math

import torch

from . import capi

MAX_K = 64
WIDE_MAX_K = 128     # a FusedSparseAttention made with wide=True (spmv_csr_attention_*_wide)
FUSED_DTYPES = (torch.float32, torch.bfloat16, torch.float16)      # what the fused passes take (all matrices of a call alike)


def _operand(t, name: str, rows: int, k=None, dtypes=(torch.float32,), max_k: int = MAX_K):
    """t as the library takes it: 2-D float32 (or another of `dtypes`), stride(1) == 1, stride(0) >= k, aligned to four
    elements: 16 bytes of floats, 8 of 16-bit elements (copied if it is not)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in dtypes:
        raise ValueError(f"SparseAttention: {name} must be a 2-D {' or '.join(str(d).replace('torch.', '') for d in dtypes)} tensor")
    if t.shape[0] != rows:
        raise ValueError(f"SparseAttention: {name} has {t.shape[0]} rows, the pattern needs {rows}")
    if not 1 <= t.shape[1] <= max_k:
        raise ValueError(f"SparseAttention: {name} has {t.shape[1]} columns (1 <= k <= {max_k})")
    if k is not None and t.shape[1] != k:
        raise ValueError(f"SparseAttention: {name} has {t.shape[1]} columns, its partner has {k}")
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.data_ptr() % (4 * t.element_size()) == 0:
        return t
    return torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)


class SparseAttentionFunction(torch.autograd.Function):
    """``SparseAttentionFunction.apply(att, Q, K, V)`` = softmax_rows(att.scale * Q K^T at the pattern) V."""

    @staticmethod
    def forward(ctx, att, Q, K, V):
        A = att.A
        Q = _operand(Q, "Q", A.rows)
        K = _operand(K, "K", A.cols, Q.shape[1])
        V = _operand(V, "V", A.cols)
        A.sddmm(Q, K, att.work)
        A.row_softmax(att.work, att.work, att.scale)
        A.values_changed()
        O = torch.empty((A.rows, V.shape[1]), dtype=torch.float32, device=V.device)
        A.spmm(V, O)
        ctx.att = att
        ctx.save_for_backward(Q, K, V, att.work.clone())
        return O

    @staticmethod
    def backward(ctx, dO):
        att = ctx.att
        A, T, W = att.A, att.T, att.work
        Q, K, V, P = ctx.saved_tensors
        dO = _operand(dO, "dO", A.rows, V.shape[1])
        dQ = dK = dV = None
        if ctx.needs_input_grad[3]:
            W.copy_(P)
            A.values_changed()
            T.transpose_values(A)
            dV = torch.empty_like(V, memory_format=torch.contiguous_format)
            T.spmm(dO, dV)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            A.sddmm(dO, V, W)                                   # dP
            A.row_softmax_backward(P, W, W, att.scale)          # dS over dP
            A.values_changed()
            if ctx.needs_input_grad[1]:
                dQ = torch.empty_like(Q, memory_format=torch.contiguous_format)
                A.spmm(K, dQ)
            if ctx.needs_input_grad[2]:
                T.transpose_values(A)
                dK = torch.empty_like(K, memory_format=torch.contiguous_format)
                T.spmm(Q, dK)
        return None, dQ, dK, dV


class SparseAttention:
    """One attention pattern of rows queries by cols keys.  Borrows ``row_ptr`` and ``col_idx`` (int32, one device); owns
    the work buffer of nnz floats that A borrows as its values, T = A^T (with the map that refreshes T's values) and both
    SpMM plans.  ``att(Q, K, V)``: Q rows x k, K cols x k, V cols x kv, k and kv <= 64; a query without keys (an empty
    row) gets a zero row of O.  Calls of one holder are stream-ordered: they share the work buffer and the plans' scratch."""

    def __init__(self, rows: int, cols: int, row_ptr, col_idx, scale: float = 1.0):
        if not math.isfinite(scale):
            raise ValueError(f"SparseAttention: scale = {scale} is not finite")
        self.scale = float(scale)
        self.work = torch.zeros(int(col_idx.numel()), dtype=torch.float32, device=col_idx.device)
        self.A = capi.CsrMatrix.from_device(rows, cols, row_ptr, col_idx, self.work)
        self.T = self.A.transpose(keep_map=True)
        self.A.spmm_plan()
        self.T.spmm_plan()

    def __call__(self, Q, K, V):
        return SparseAttentionFunction.apply(self, Q, K, V)

    def close(self) -> None:
        self.T.close()
        self.A.close()


def topk_pattern(A, Q, K, k: int, scale: float = 1.0):
    """The k best keys of every query among the candidates of ``A`` (a capi.CsrMatrix of queries x keys): the scores
    ``scale * Q K^T`` at A's pattern (spmv_csr_sddmm: one head, float32, Q rows x w and K cols x w with w <= MAX_K), then
    ``A.select_topk(k, score)`` -- ties go to the earlier candidate, a NaN score ranks last, rows keep A's storage order.
    Returns ``(row_ptr, col_idx)`` as int32 device tensors, ready for ``FusedSparseAttention(rows, cols, row_ptr, col_idx,
    ...)``.  The selection is a discrete choice: no gradient flows through it (Q and K are read detached); the attention
    on the returned pattern differentiates with respect to Q, K and V as usual.  A's values are not read."""
    if not isinstance(A, capi.CsrMatrix):
        raise ValueError("topk_pattern: A must be a capi.CsrMatrix (the candidate pattern)")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"topk_pattern: k = {k!r} (an int >= 1)")
    if not math.isfinite(scale):
        raise ValueError(f"topk_pattern: scale = {scale} is not finite")
    if not isinstance(Q, torch.Tensor) or not isinstance(K, torch.Tensor):
        raise ValueError("topk_pattern: Q and K must be 2-D float32 tensors")
    Q = _operand(Q.detach(), "Q", A.rows)
    K = _operand(K.detach(), "K", A.cols, Q.shape[1])
    A.spmm_plan()
    score = torch.empty(A.nnz, dtype=torch.float32, device=Q.device)
    A.sddmm(Q, K, score)
    if scale != 1.0:
        score.mul_(float(scale))
    sel = A.select_topk(k, score)
    row_ptr = torch.empty(sel.rows + 1, dtype=torch.int32, device=Q.device)
    col_idx = torch.empty(sel.nnz, dtype=torch.int32, device=Q.device)
    sel.copy_arrays(row_ptr, col_idx)
    torch.cuda.current_stream().synchronize()      # the copies read sel's arrays, which close() frees
    sel.close()
    return row_ptr, col_idx


def _combined_pattern(who: str, A, B, op: str):
    for name, m in (("A", A), ("B", B)):
        if not isinstance(m, capi.CsrMatrix):
            raise ValueError(f"{who}: {name} must be a capi.CsrMatrix")
    if (A.rows, A.cols) != (B.rows, B.cols):
        raise ValueError(f"{who}: A is {A.rows} x {A.cols}, B is {B.rows} x {B.cols}")
    c = A.add(B, 0.0, 0.0, op)                      # (coefficients of 0: the patterns alone, no value of A or B is read)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        row_ptr = torch.empty(c.rows + 1, dtype=torch.int32, device=dev)
        col_idx = torch.empty(c.nnz, dtype=torch.int32, device=dev)
        c.copy_arrays(row_ptr, col_idx)
        torch.cuda.current_stream().synchronize()      # the copies read c's arrays, which close() frees
    finally:
        c.close()
    return row_ptr, col_idx


def union_pattern(A, B):
    """The union of two patterns of queries x keys (capi.CsrMatrix handles of one shape; spmv_csr_add with SPMV_ADD_UNION):
    a local band with the per-row top-k of :func:`topk_pattern` with a few global columns, two at a time.  Returns ``(row_ptr,
    col_idx)`` as fresh int32 device tensors with sorted, duplicate-free rows, ready for ``FusedSparseAttention``.  No value
    of A or B is read."""
    return _combined_pattern("union_pattern", A, B, "union")


def mask_pattern(A, M):
    """The positions of A that M has too (spmv_csr_add with SPMV_ADD_INTERSECT): a candidate pattern under a causal or block
    mask.  Returns ``(row_ptr, col_idx)`` as :func:`union_pattern` does."""
    return _combined_pattern("mask_pattern", A, M, "intersect")


def _fused_operand(t, name: str, rows: int, k=None):
    """A 2-D operand as _operand takes it, or (heads, rows, k): every head t[h] must itself be acceptable to the library
    (a column block of a (rows, heads * k) tensor with k % 4 == 0 is); otherwise the whole tensor is copied once into
    rows padded to a multiple of 4 elements, so that every head starts on a boundary of four elements (16 bytes of floats, 8
    of 16-bit elements)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        return _operand(t, name, rows, k, FUSED_DTYPES)
    if t.shape[0] < 1:
        raise ValueError(f"SparseAttention: {name} has no heads")
    _operand(t[0], name, rows, k, FUSED_DTYPES)       # (dtype and shape)
    w, align = t.shape[2], 4 * t.element_size()
    if all(t.stride(2) == 1 and t.stride(1) >= w and t[h].data_ptr() % align == 0 for h in range(t.shape[0])):
        return t
    return _heads_empty(t.shape[0], rows, w, t.device, t.dtype).copy_(t)


def _batched_operand(t, name: str, rows: int, k=None, max_k: int = MAX_K):
    """A (heads, rows, k) operand as one _heads call takes it: stride(2) == 1, stride(1) >= k, head 0 on a boundary of four
    elements (16 bytes of floats, 8 of 16-bit elements) and, with more than one head, a head stride that is a multiple of 4
    elements (0: one head shared by all).  Stacked heads and the column blocks of a (rows, heads * k) tensor with k % 4 == 0
    are; anything else is copied once."""
    if t.shape[0] < 1:
        raise ValueError(f"SparseAttention: {name} has no heads")
    _operand(t[0], name, rows, k, FUSED_DTYPES, max_k)       # (dtype and shape)
    w = t.shape[2]
    if t.stride(2) == 1 and t.stride(1) >= w and t.data_ptr() % (4 * t.element_size()) == 0 \
            and (t.shape[0] == 1 or t.stride(0) % 4 == 0):
        return t
    return _heads_empty(t.shape[0], rows, w, t.device, t.dtype).copy_(t)


def _heads_empty(heads: int, rows: int, w: int, device, dtype=torch.float32):
    """(heads, rows, w) of `dtype` whose every head starts on a boundary of four elements (rows padded to a multiple of 4
    elements if need be)."""
    return torch.empty((heads, rows, (w + 3) // 4 * 4), dtype=dtype, device=device)[:, :, :w]


class FusedSparseAttentionFunction(torch.autograd.Function):
    """``FusedSparseAttentionFunction.apply(att, Q, K, V)``: as SparseAttentionFunction, 2-D operands or (heads, n, width)
    ones; K and V may hold H_kv heads with H % H_kv == 0 (grouped-query heads: query head h reads K[h // g], V[h // g],
    g = H // H_kv).  Saved for backward: Q, K, V, O and stats (2 floats per query and head)."""

    @staticmethod
    def forward(ctx, att, Q, K, V):
        A = att.A
        if len({t.dim() if isinstance(t, torch.Tensor) else -1 for t in (Q, K, V)}) != 1:
            raise ValueError("SparseAttention: Q, K and V must all be 2-D or all (heads, n, width)")
        one_launch = att.heads == "batched" and isinstance(Q, torch.Tensor) and Q.dim() == 3
        operand = _batched_operand if one_launch else _fused_operand
        Q = operand(Q, "Q", A.rows)
        K = operand(K, "K", A.cols, Q.shape[-1])
        V = operand(V, "V", A.cols)
        for name, t in (("K", K), ("V", V)):
            if t.dtype != Q.dtype:
                raise ValueError(f"SparseAttention: {name} is {t.dtype}, Q is {Q.dtype} (Q, K and V share one dtype)")
        kv = V.shape[-1]
        if Q.dim() == 3:
            heads = Q.shape[0]
            if K.shape[0] != V.shape[0] or heads % K.shape[0] != 0:
                raise ValueError(f"SparseAttention: Q has {heads} heads, K {K.shape[0]} and V {V.shape[0]}")
            g = heads // K.shape[0]
            O = _heads_empty(heads, A.rows, kv, V.device, V.dtype)
            stats = torch.empty((heads, A.rows, 2), dtype=torch.float32, device=V.device)
            chunks = att.head_chunks(heads, Q.shape[-1], kv, g) if one_launch else None
            if chunks and g == 1:
                for lo, hi in chunks:
                    A.attention_forward_heads(Q[lo:hi], K[lo:hi], V[lo:hi], O[lo:hi], stats[lo:hi], att.scale)
            elif chunks:
                for lo, hi in chunks:
                    A.attention_forward_gqa(Q[lo:hi], K[lo // g:hi // g], V[lo // g:hi // g], O[lo:hi], stats[lo:hi], att.scale)
            else:
                for h in range(heads):
                    A.attention_forward(Q[h], K[h // g], V[h // g], O[h], stats[h], att.scale)
        else:
            O = torch.empty((A.rows, kv), dtype=V.dtype, device=V.device)
            stats = torch.empty((A.rows, 2), dtype=torch.float32, device=V.device)
            A.attention_forward(Q, K, V, O, stats, att.scale)
        ctx.att = att
        ctx.save_for_backward(Q, K, V, O, stats)
        return O

    @staticmethod
    def backward(ctx, dO):
        att = ctx.att
        A, T = att.A, att.T
        Q, K, V, O, stats = ctx.saved_tensors
        need_q, need_k, need_v = ctx.needs_input_grad[1:4]
        if not (need_q or need_k or need_v):
            return None, None, None, None
        batched = Q.dim() == 3
        one_launch = batched and att.heads == "batched"
        dO = (_batched_operand if one_launch else _fused_operand)(dO, "dO", A.rows, V.shape[-1])
        if batched and dO.shape[0] != Q.shape[0]:
            raise ValueError(f"SparseAttention: dO has {dO.shape[0]} heads, Q {Q.shape[0]}")
        if dO.dtype != Q.dtype:
            raise ValueError(f"SparseAttention: dO is {dO.dtype}, Q is {Q.dtype}")

        def like(t):
            return _heads_empty(*t.shape, t.device, t.dtype) if batched else torch.empty(t.shape, dtype=t.dtype, device=t.device)

        # backward_q also makes delta, which backward_kv reads: it runs whichever gradient is asked for
        dQ = like(Q)
        delta = torch.empty(O.shape[:-1], dtype=torch.float32, device=O.device)
        dK = like(K) if need_k or need_v else None
        dV = like(V) if need_k or need_v else None
        g = Q.shape[0] // K.shape[0] if batched else 1
        chunks = att.head_chunks(Q.shape[0], Q.shape[-1], V.shape[-1], g) if one_launch else None
        if chunks:
            for lo, hi in chunks:
                at = lambda t, lo=lo, hi=hi: t[lo:hi]       # noqa: E731
                kv = lambda t, lo=lo // g, hi=hi // g: t[lo:hi]       # noqa: E731  (the chunk's K/V heads)
                if g == 1:
                    A.attention_backward_q_heads(at(Q), at(K), at(V), at(O), at(dO), at(stats), at(delta), at(dQ), att.scale)
                    if dK is not None:
                        T.attention_backward_kv_heads(at(Q), at(K), at(V), at(dO), at(stats), at(delta), at(dK), at(dV), att.scale)
                    continue
                A.attention_backward_q_gqa(at(Q), kv(K), kv(V), at(O), at(dO), at(stats), at(delta), at(dQ), att.scale)
                if dK is not None:
                    T.attention_backward_kv_gqa(at(Q), kv(K), kv(V), at(dO), at(stats), at(delta), kv(dK), kv(dV), att.scale)
            return None, dQ if need_q else None, dK if need_k else None, dV if need_v else None
        heads = range(Q.shape[0]) if batched else (None,)
        if g > 1 and dK is not None and Q.dtype != torch.float32:
            # 16-bit grouped-query heads: the sum over the heads of a group is fp32 and rounded once, so it stays in the kernel:
            # one _gqa call per K/V head instead of per-head calls added here (which would round every head's dK and dV first)
            att.plan_heads(g)
            for h in heads:
                A.attention_backward_q(Q[h], K[h // g], V[h // g], O[h], dO[h], stats[h], delta[h], dQ[h], att.scale)
            for c in range(K.shape[0]):
                qs = slice(c * g, c * g + g)
                T.attention_backward_kv_gqa(Q[qs], K[c:c + 1], V[c:c + 1], dO[qs], stats[qs], delta[qs], dK[c:c + 1], dV[c:c + 1],
                                            att.scale)
            return None, dQ if need_q else None, dK if need_k else None, dV if need_v else None
        # grouped-query heads: the heads of a group after the first write into dKh, dVh, which are then added to the group's
        # dK, dV: fp32 adds in head order, starting from the first head's value (what the _gqa call does in its kernel)
        dKh, dVh = (like(K[:1])[0], like(V[:1])[0]) if g > 1 and dK is not None else (None, None)
        for h in heads:
            at = (lambda t: t) if h is None else (lambda t, h=h: t[h])
            kv = (lambda t: t) if h is None else (lambda t, c=h // g: t[c])
            A.attention_backward_q(at(Q), kv(K), kv(V), at(O), at(dO), at(stats), at(delta), at(dQ), att.scale)
            if dK is None:
                continue
            first = h is None or h % g == 0
            T.attention_backward_kv(at(Q), kv(K), kv(V), at(dO), at(stats), at(delta), kv(dK) if first else dKh,
                                    kv(dV) if first else dVh, att.scale)
            if not first:
                torch.add(kv(dK), dKh, out=kv(dK))
                torch.add(kv(dV), dVh, out=kv(dV))
        return None, dQ if need_q else None, dK if need_k else None, dV if need_v else None


class BiasedFusedSparseAttentionFunction(torch.autograd.Function):
    """``BiasedFusedSparseAttentionFunction.apply(att, Q, K, V, bias)`` = softmax_rows(att.scale * Q K^T + bias at the pattern) V
    on the three _bias passes: operands as FusedSparseAttentionFunction takes them (a 2-D call is one head), bias float32
    (nnz,) -- one for all heads -- or (heads, nnz), in the storage order of the pattern.  Saved for backward: Q, K, V, O,
    stats and bias.  Backward makes bias_t (the bias in T's order, one gather) only when dK or dV is asked for, and dBias
    (heads, nnz) only when the bias requires grad; a shared bias gets dBias summed over the heads.
    On a holder made with wide=True every pass is the _wide call instead: widths up to WIDE_MAX_K, and bias may be None (no
    bias: the unbiased kernels)."""

    @staticmethod
    def _runs(att, heads: int, k: int, kv: int, g: int):
        """[(lo, hi)]: whole groups of query heads per _bias call: as many as fit one launch ("batched"), or one group ("loop")"""
        runs = att.head_chunks(heads, k, kv, g) if att.heads == "batched" else None
        if runs is None:
            att.plan_heads(g)
            runs = [(lo, lo + g) for lo in range(0, heads, g)]
        return runs

    @staticmethod
    def forward(ctx, att, Q, K, V, bias):
        A = att.A
        if len({t.dim() if isinstance(t, torch.Tensor) else -1 for t in (Q, K, V)}) != 1 or Q.dim() not in (2, 3):
            raise ValueError("SparseAttention: Q, K and V must all be 2-D or all (heads, n, width)")
        flat = Q.dim() == 2
        if flat:
            Q, K, V = Q[None], K[None], V[None]
        max_k = WIDE_MAX_K if att.wide else MAX_K
        Q = _batched_operand(Q, "Q", A.rows, None, max_k)
        K = _batched_operand(K, "K", A.cols, Q.shape[-1], max_k)
        V = _batched_operand(V, "V", A.cols, None, max_k)
        for name, t in (("K", K), ("V", V)):
            if t.dtype != Q.dtype:
                raise ValueError(f"SparseAttention: {name} is {t.dtype}, Q is {Q.dtype} (Q, K and V share one dtype)")
        heads, kv = Q.shape[0], V.shape[-1]
        if K.shape[0] != V.shape[0] or heads % K.shape[0] != 0:
            raise ValueError(f"SparseAttention: Q has {heads} heads, K {K.shape[0]} and V {V.shape[0]}")
        if bias is None and att.wide:
            pass
        elif not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) not in ((A.nnz,), (heads, A.nnz)):
            raise ValueError(f"SparseAttention: bias must be a float32 tensor of ({A.nnz},) or ({heads}, {A.nnz})")
        bias = bias if bias is None or bias.stride(-1) == 1 else bias.contiguous()
        g = heads // K.shape[0]
        O = _heads_empty(heads, A.rows, kv, V.device, V.dtype)
        stats = torch.empty((heads, A.rows, 2), dtype=torch.float32, device=V.device)
        for lo, hi in BiasedFusedSparseAttentionFunction._runs(att, heads, Q.shape[-1], kv, g):
            b = bias if bias is None or bias.dim() == 1 else bias[lo:hi]
            if att.wide:
                A.attention_forward_wide(Q[lo:hi], K[lo // g:hi // g], V[lo // g:hi // g], O[lo:hi], stats[lo:hi], b, att.scale)
            else:
                A.attention_forward_bias(Q[lo:hi], K[lo // g:hi // g], V[lo // g:hi // g], b, O[lo:hi], stats[lo:hi], att.scale)
        ctx.att, ctx.flat = att, flat
        ctx.save_for_backward(Q, K, V, O, stats, bias)
        return O[0] if flat else O

    @staticmethod
    def backward(ctx, dO):
        att = ctx.att
        A, T = att.A, att.T
        Q, K, V, O, stats, bias = ctx.saved_tensors
        need_q, need_k, need_v, need_b = ctx.needs_input_grad[1:5]
        if not (need_q or need_k or need_v or need_b):
            return None, None, None, None, None
        dO = _batched_operand(dO[None] if ctx.flat else dO, "dO", A.rows, V.shape[-1], WIDE_MAX_K if att.wide else MAX_K)
        if dO.shape[0] != Q.shape[0] or dO.dtype != Q.dtype:
            raise ValueError(f"SparseAttention: dO is {dO.dtype} with {dO.shape[0]} heads, Q {Q.dtype} with {Q.shape[0]}")
        heads, g = Q.shape[0], Q.shape[0] // K.shape[0]
        shared = bias is not None and bias.dim() == 1
        # backward_q also makes delta, which backward_kv reads: it runs whichever gradient is asked for
        dQ = _heads_empty(*Q.shape, Q.device, Q.dtype)
        delta = torch.empty(O.shape[:-1], dtype=torch.float32, device=O.device)
        dBias = torch.empty((heads, A.nnz), dtype=torch.float32, device=O.device) if need_b else None
        dK = dV = bias_t = None
        if need_k or need_v:
            dK, dV = _heads_empty(*K.shape, K.device, K.dtype), _heads_empty(*V.shape, V.device, V.dtype)
            if bias is not None:
                bias_t = torch.empty_like(bias)
                T.transpose_gather(bias, bias_t)
        for lo, hi in BiasedFusedSparseAttentionFunction._runs(att, heads, Q.shape[-1], V.shape[-1], g):
            at = lambda t, lo=lo, hi=hi: t[lo:hi]       # noqa: E731
            kv = lambda t, lo=lo // g, hi=hi // g: t[lo:hi]       # noqa: E731  (the run's K/V heads)
            per_head = (lambda b: b) if shared or bias is None else at
            if att.wide:
                A.attention_backward_q_wide(at(Q), kv(K), kv(V), at(O), at(dO), at(stats), at(delta), at(dQ), per_head(bias),
                                            at(dBias) if need_b else None, att.scale)
                if dK is not None:
                    T.attention_backward_kv_wide(at(Q), kv(K), kv(V), at(dO), at(stats), at(delta), kv(dK), kv(dV), per_head(bias_t),
                                                 att.scale)
                continue
            A.attention_backward_q_bias(at(Q), kv(K), kv(V), per_head(bias), at(O), at(dO), at(stats), at(delta), at(dQ),
                                        at(dBias) if need_b else None, att.scale)
            if dK is not None:
                T.attention_backward_kv_bias(at(Q), kv(K), kv(V), per_head(bias_t), at(dO), at(stats), at(delta),
                                             kv(dK), kv(dV), att.scale)
        if need_b and shared:
            dBias = dBias[0] if heads == 1 else dBias.sum(0)
        one = (lambda t: t[0]) if ctx.flat else (lambda t: t)
        return None, one(dQ) if need_q else None, one(dK) if need_k else None, one(dV) if need_v else None, dBias


class FusedSparseAttention:
    """One attention pattern of rows queries by cols keys on the fused passes.  Borrows ``row_ptr`` and ``col_idx`` (int32,
    one device); owns T = A^T (pattern only: no map) and both attention plans.  ``att(Q, K, V)``: Q rows x k, K cols x k,
    V cols x kv, k and kv <= 64, or (heads, rows, k), (heads, cols, k), (heads, cols, kv): with ``heads="loop"`` (the default)
    the heads run one after the other on the same A and T; a head that is a strided view with stride(1) == 1 on a 16-byte
    boundary goes in without a copy.  With ``heads="batched"`` all heads of a 3-D call run in one launch per kernel
    (spmv_csr_attention_*_heads): the plans grow to the head count on first use (an allocation: not inside a graph capture),
    stacked heads and column blocks of a (n, heads * k) tensor with k % 4 == 0 go in without a copy, and a head count beyond
    a launch limit is split into the fewest chunks that fit.  Both modes give the same bits; 2-D operands behave alike in
    both.  Grouped-query heads (GQA): K and V may carry H_kv heads with H % H_kv == 0; query head h then reads K[h // g] and
    V[h // g], g = H // H_kv, without a copy, and dK and dV come back (H_kv, cols, width).  "batched" issues one
    spmv_csr_attention_*_gqa call per pass (the kernel adds the heads' dK, dV), in chunks of whole groups; where fewer than
    g heads fit one launch that call runs by the loop.  "loop" runs the per-head calls on K[h // g] and adds each head's dK, dV
    into its group's in head order, starting from the first head's value: the same bits again.  Any other head mismatch is a
    ValueError.  16-bit operands: Q, K and V all torch.bfloat16 or all torch.float16 run on spmv_csr_attention_*_16 in every
    layout above (alignment and strides then count 2-byte elements: a head starts on an 8-byte boundary); O, the saved O and
    the gradients have that dtype, stats and delta stay float32; every output is the fp32 result rounded once, so with
    grouped K/V "loop" leaves the sum over a group's heads to one _gqa call per K/V head.  A query without keys gets a zero row of O.  Calls of one holder are stream-ordered (the plans' scratch).  The
    values array that handle creation still asks for is allocated once here and never read.
    ``bias=True``: ``att(Q, K, V, bias)`` adds ``bias`` -- float32 (nnz,), shared by all heads, or (heads, nnz), in the storage
    order of ``col_idx`` -- to the scaled scores before the softmax and is differentiable in it
    (BiasedFusedSparseAttentionFunction); T then keeps its map (4 bytes per nonzero), which brings the bias into T's order in
    backward.  Every layout and dtype above works; "loop" runs one call per K/V head, "batched" as many groups as fit.
    ``wide=True``: k and kv up to 128 (WIDE_MAX_K) on spmv_csr_attention_*_wide, with or without ``bias=True``, in both
    ``heads`` modes, with grouped-query heads and 16-bit tensors: both handles are planned wide and every pass is a _wide call,
    one per K/V head ("loop") or as many groups as fit a launch ("batched").  Up to width 64 those are the calls above bit for
    bit.  The default is the holder described above, unchanged."""

    def __init__(self, rows: int, cols: int, row_ptr, col_idx, scale: float = 1.0, heads: str = "loop", bias: bool = False,
                 wide: bool = False):
        if heads not in ("loop", "batched"):
            raise ValueError(f"SparseAttention: heads = {heads!r} (\"loop\" or \"batched\")")
        if not math.isfinite(scale):
            raise ValueError(f"SparseAttention: scale = {scale} is not finite")
        self.heads = heads
        self.scale = float(scale)
        self.max_heads = None       # a cap on the heads of one launch below the library's (None: the library's limit)
        self._planned = 1
        vals = torch.zeros(int(col_idx.numel()), dtype=torch.float32, device=col_idx.device)
        self.A = capi.CsrMatrix.from_device(rows, cols, row_ptr, col_idx, vals)
        self.bias = bool(bias)
        self.wide = bool(wide)
        self.T = self.A.transpose(keep_map=self.bias)
        self.A.attention_plan()
        self.T.attention_plan()
        if self.wide:
            self.A.attention_plan_wide(1)
            self.T.attention_plan_wide(1)

    def __call__(self, Q, K, V, bias=None):
        if self.bias != (bias is not None):
            raise ValueError("SparseAttention: a holder made with bias=True takes att(Q, K, V, bias), any other att(Q, K, V)")
        if bias is not None or self.wide:
            return BiasedFusedSparseAttentionFunction.apply(self, Q, K, V, bias)
        return FusedSparseAttentionFunction.apply(self, Q, K, V)

    def head_chunks(self, heads: int, k: int, kv: int, group: int = 1):
        """[(lo, hi)]: the fewest runs of heads that each fit one launch on A and on T at these widths (the library says how
        many fit: spmv_csr_attention_max_heads).  Grows both plans to the largest run.  With ``group`` > 1 (grouped-query
        heads) a run is whole groups; None when not even one group fits a launch (the caller then runs the heads in a loop)."""
        if self.wide:
            fit = min(self.A.attention_max_heads_wide(k, kv), self.T.attention_max_heads_wide(k, kv))
        else:
            fit = min(self.A.attention_max_heads(k, kv), self.T.attention_max_heads(k, kv))
        fit = max(1, min(fit, self.max_heads or fit))      # (not even one: the call itself says why)
        if group > 1:
            if fit < group:
                return None
            n = -(-heads // (fit // group * group))
            size = -(-(heads // group) // n) * group
        else:
            n = -(-heads // fit)
            size = -(-heads // n)
        self.plan_heads(size)
        return [(lo, min(lo + size, heads)) for lo in range(0, heads, size)]

    def plan_heads(self, heads: int) -> None:
        """Grow both plans to `heads` heads of one launch (an allocation: not inside a graph capture)."""
        if heads > self._planned:
            plan = "attention_plan_wide" if self.wide else "attention_plan_heads"
            getattr(self.A, plan)(heads)
            getattr(self.T, plan)(heads)
            self._planned = heads

    def close(self) -> None:
        self.T.close()
        self.A.close()
