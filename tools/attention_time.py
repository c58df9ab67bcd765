#!/usr/bin/env python3
"""tools/attention_time.py -- FusedSparseAttention against the composed SparseAttention on the same pattern arrays, in one process.

One JSON line per (workload, k = kv): the forward time and the forward-plus-backward time of both holders (HIP events,
warmed up, the two holders' windows alternating, median of --reps windows of enough calls to fill --window-ms), their ratios
fused / composed (below 1: the fused path is faster), and what torch.cuda.max_memory_allocated rises by over one
forward-plus-backward step of each.  The composed holder is sparse_attention.SparseAttention as it stands (SDDMM, row softmax,
SpMM, transpose_values), so it is the yardstick; nothing here sets a threshold.

    python tools/attention_time.py [--workloads c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0] [--ks 16,32,64] [--scale c4=1.0]
                                   [--out profiles/attention_sweep.jsonl]

--heads H[,H..]: the other comparison.  On the same (H, n, w) tensors and the same pattern, FusedSparseAttention(heads="loop")
(one call per head and pass: the behaviour before the _heads calls existed) against FusedSparseAttention(heads="batched") (all
heads in one launch per kernel), by the same protocol.  One JSON line per (pattern, k = kv, H): both times, their ratio
batched / loop (below 1: one launch is faster), the lowest and highest window of each, and whether O and the three gradients
of the two holders are equal bit for bit.  The patterns: bandNxM = N queries and N keys, query i listing the M consecutive
keys around i (a sliding window), or a config as above; "@H" after a pattern runs it at that head count only.

    python tools/attention_time.py --heads 8,16 [--workloads band4096x64,...,c2:8192@8] [--ks 16,64]
                                   [--out profiles/attention_heads.jsonl]

--gqa G[,G..]: grouped-query heads.  On the same patterns as --heads, with H = 16 query heads (--gqa-heads) on H / G K/V heads,
FusedSparseAttention(heads="batched") two ways in one process, the windows alternating: on the grouped K and V (the _gqa
calls: K and V are not expanded, the kernel adds the heads' dK and dV), and on K and V expanded with repeat_interleave inside
the timed window, with autograd's sum of dK and dV (what a caller did before the _gqa calls existed).  And backward_kv alone:
one attention_backward_kv_gqa call against one attention_backward_kv_heads call on the expanded K and V (G per-head passes per
K/V head into H sets of dK and dV, which nobody sums here).  One JSON line per (pattern, k = kv, G): the medians, the ratios
grouped / expanded (below 1: grouped is faster), the lowest and highest window of each and the bytes a forward-plus-backward
step allocates.  Nothing here sets a threshold.

    python tools/attention_time.py --gqa 2,4,8 [--workloads band4096x64,...] [--ks 16,64] [--out profiles/attention_gqa.jsonl]

--dtype bf16[,fp16]: 16-bit operands.  On the same pattern arrays two FusedSparseAttention holders, one called on float32 Q, K, V
and dO and one on the same numbers in the 16-bit dtype (spmv_csr_attention_*_16), by the same protocol: the windows alternating,
median of --reps, the lowest and highest window of each.  One JSON line per (workload, k = kv, dtype): forward and
forward-plus-backward time of both, the ratios 16-bit / fp32 (below 1: 16-bit is faster), and the bytes a step allocates.  The
fp32 path is the yardstick; nothing here sets a threshold.

    python tools/attention_time.py --dtype bf16,fp16 [--workloads c2:8192,c2:0,c3:8192,c3:0] [--ks 16,32,64]
                                   [--out profiles/attention_16bit.jsonl]

--bias: the additive bias per nonzero.  On the same pattern arrays, in one process, the windows alternating, median of --reps:
FusedSparseAttention(bias=True) called with a float32 bias of nnz numbers that requires grad (spmv_csr_attention_*_bias; the
step includes the gather to T's order and dBias) against the unbiased FusedSparseAttention, the yardstick, and against the
composed SparseAttention path with the bias added to the scaled scores by torch (SDDMM, mul and add on nnz floats, row softmax,
SpMM; backward with dBias).  One JSON line per (workload, k = kv): the medians, the ratios biased / unbiased and
biased / composed (below 1: the biased fused path is faster), the lowest and highest window of each, the bytes a step
allocates.  Nothing here sets a threshold.

    python tools/attention_time.py --bias [--workloads c2:8192,c2:0,c3:8192,c3:0] [--ks 16,32,64]
                                   [--out profiles/attention_bias.jsonl]
--wide: the holder made with wide=True at k = kv = 128 (spmv_csr_attention_*_wide) against the unchanged holder at k = kv = 64
on the same pattern arrays, float32 and 16-bit operands (wide_main).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed_windows(fa, fb, window_ms, reps, max_iters):
    """`reps` windows of fa and of fb, alternating; the windows hold the same number of calls."""
    for _ in range(2):
        fa()
        fb()
    one = max(window(fa, 1), window(fb, 1))
    iters = max(1, min(max_iters, int(window_ms / one)))
    a, b = [], []
    for _ in range(reps):
        a.append(window(fa, iters))
        b.append(window(fb, iters))
    return a, b, iters


def timed_pair(fa, fb, window_ms, reps, max_iters):
    """Medians of the windows of timed_windows."""
    a, b, iters = timed_windows(fa, fb, window_ms, reps, max_iters)
    return statistics.median(a), statistics.median(b), iters


HEADS_WORKLOADS = "band4096x64,band4096x256,band16384x64,band16384x256,band65536x64,band65536x256,c2:8192@8"


def heads_pattern(spec, capi, W, dev, scales):
    """(name, rows, cols, row_ptr, col_idx) on the device of bandNxM (query i lists the M consecutive keys around i) or of
    a config name:band."""
    import torch
    if spec.startswith("band"):
        n, m = (int(v) for v in spec[4:].split("x"))
        start = (torch.arange(n, device=dev) - m // 2).clamp(0, n - m)
        ci = (start[:, None] + torch.arange(m, device=dev)[None, :]).to(torch.int32).reshape(-1).contiguous()
        rp = (torch.arange(n + 1, device=dev) * m).to(torch.int32)
        return spec, n, n, rp, ci
    name, band = spec.split(":")
    w = W.config(name, band=int(band), scale=scales.get(name, 1.0))
    rp = W.row_ptr(w)
    nnz = int(rp[-1])
    d_rp = torch.from_numpy(rp).to(dev)
    d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
    capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
    return f"{name}_band{band}", w.rows, w.cols, d_rp, d_ci


def heads_main(a, emit):
    """The loop over the heads against one launch for all heads (see the module docstring)."""
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    all_heads = [int(h) for h in a.heads.split(",")]
    for spec in (a.workloads or HEADS_WORKLOADS).split(","):
        spec, _, only = spec.partition("@")
        name, rows, cols, d_rp, d_ci = heads_pattern(spec, capi, W, dev, scales)
        loop = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25, heads="loop")
        batched = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25, heads="batched")
        for H in ([int(only)] if only else all_heads):
            for k in (int(s) for s in a.ks.split(",")):
                gen = torch.Generator(device=dev).manual_seed(k)
                Q, K, V, dO = (torch.randn((H, n, k), generator=gen, device=dev) for n in (rows, cols, cols, rows))
                q, kk, v = (t.clone().requires_grad_(True) for t in (Q, K, V))

                def forward(att):
                    with torch.no_grad():
                        att(Q, K, V)

                def step(att):
                    att(q, kk, v).backward(dO)
                    q.grad = kk.grad = v.grad = None

                def results(att):
                    O = att(q, kk, v)
                    O.backward(dO)
                    out = [t.detach().clone() for t in (O, q.grad, kk.grad, v.grad)]
                    q.grad = kk.grad = v.grad = None
                    return out

                same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(results(loop), results(batched)))
                l_f, b_f, it_f = timed_windows(lambda: forward(loop), lambda: forward(batched), a.window_ms, a.reps, a.max_iters)
                l_s, b_s, it_s = timed_windows(lambda: step(loop), lambda: step(batched), a.window_ms, a.reps, a.max_iters)
                med, r4 = statistics.median, lambda x: round(x, 4)      # noqa: E731
                emit(workload=name, heads=H, k=k, kv=k, rows=rows, cols=cols, nnz=int(d_ci.numel()), plan=loop.A.spmm_describe(),
                     plan_T=loop.T.spmm_describe(), iters_forward=it_f, iters_step=it_s, reps=a.reps,
                     loop_forward_ms=r4(med(l_f)), batched_forward_ms=r4(med(b_f)), forward_ratio=round(med(b_f) / med(l_f), 3),
                     loop_forward_windows=[r4(min(l_f)), r4(max(l_f))], batched_forward_windows=[r4(min(b_f)), r4(max(b_f))],
                     loop_step_ms=r4(med(l_s)), batched_step_ms=r4(med(b_s)), step_ratio=round(med(b_s) / med(l_s), 3),
                     loop_step_windows=[r4(min(l_s)), r4(max(l_s))], batched_step_windows=[r4(min(b_s)), r4(max(b_s))],
                     equal_bits=same)
                del Q, K, V, dO, q, kk, v
                torch.cuda.empty_cache()
        loop.close()
        batched.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


def gqa_main(a, emit):
    """Grouped K and V against K and V expanded by the caller (see the module docstring)."""
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    H = a.gqa_heads
    med, r4 = statistics.median, lambda x: round(x, 4)      # noqa: E731
    for spec in (a.workloads or HEADS_WORKLOADS).split(","):
        spec = spec.partition("@")[0]
        name, rows, cols, d_rp, d_ci = heads_pattern(spec, capi, W, dev, scales)
        att = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25, heads="batched")
        for G in (int(g) for g in a.gqa.split(",")):
            for k in (int(s) for s in a.ks.split(",")):
                gen = torch.Generator(device=dev).manual_seed(k)
                Q, K, V, dO = (torch.randn((h, n, k), generator=gen, device=dev)
                               for h, n in ((H, rows), (H // G, cols), (H // G, cols), (H, rows)))
                q, kk, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
                expand = lambda t: t.repeat_interleave(G, dim=0)      # noqa: E731

                def forward(grouped):
                    with torch.no_grad():
                        att(Q, K, V) if grouped else att(Q, expand(K), expand(V))

                def step(grouped):
                    (att(q, kk, v) if grouped else att(q, expand(kk), expand(v))).backward(dO)
                    q.grad = kk.grad = v.grad = None

                def step_bytes(grouped):
                    step(grouped)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    step(grouped)
                    torch.cuda.synchronize()
                    return torch.cuda.max_memory_allocated() - before

                def results(grouped):
                    O = att(q, kk, v) if grouped else att(q, expand(kk), expand(v))
                    O.backward(dO)
                    out = [t.detach().clone() for t in (O, q.grad, kk.grad, v.grad)]
                    q.grad = kk.grad = v.grad = None
                    return out

                rg, re = results(True), results(False)
                same_O = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(rg[:2], re[:2]))
                diff = max(float((x - y).abs().max()) for x, y in zip(rg[2:], re[2:]))
                g_f, e_f, it_f = timed_windows(lambda: forward(True), lambda: forward(False), a.window_ms, a.reps, a.max_iters)
                g_s, e_s, it_s = timed_windows(lambda: step(True), lambda: step(False), a.window_ms, a.reps, a.max_iters)
                # backward_kv alone, on the operands of one step (the plans cover H heads after the steps above)
                with torch.no_grad():
                    O = att(Q, K, V)
                stats, delta = torch.empty((H, rows, 2), device=dev), torch.empty((H, rows), device=dev)
                dQ = torch.empty_like(Q)
                att.A.attention_forward_gqa(Q, K, V, O, stats, att.scale)
                att.A.attention_backward_q_gqa(Q, K, V, O, dO, stats, delta, dQ, att.scale)
                Ke, Ve = expand(K), expand(V)
                dKg, dVg, dKe, dVe = torch.empty_like(K), torch.empty_like(V), torch.empty_like(Ke), torch.empty_like(Ve)
                g_kv, e_kv, it_kv = timed_windows(
                    lambda: att.T.attention_backward_kv_gqa(Q, K, V, dO, stats, delta, dKg, dVg, att.scale),
                    lambda: att.T.attention_backward_kv_heads(Q, Ke, Ve, dO, stats, delta, dKe, dVe, att.scale),
                    a.window_ms, a.reps, a.max_iters)
                emit(workload=name, heads=H, group=G, k=k, kv=k, rows=rows, cols=cols, nnz=int(d_ci.numel()),
                     plan=att.A.spmm_describe(), plan_T=att.T.spmm_describe(), iters_forward=it_f, iters_step=it_s,
                     iters_backward_kv=it_kv, reps=a.reps,
                     grouped_forward_ms=r4(med(g_f)), expanded_forward_ms=r4(med(e_f)), forward_ratio=round(med(g_f) / med(e_f), 3),
                     grouped_forward_windows=[r4(min(g_f)), r4(max(g_f))], expanded_forward_windows=[r4(min(e_f)), r4(max(e_f))],
                     grouped_step_ms=r4(med(g_s)), expanded_step_ms=r4(med(e_s)), step_ratio=round(med(g_s) / med(e_s), 3),
                     grouped_step_windows=[r4(min(g_s)), r4(max(g_s))], expanded_step_windows=[r4(min(e_s)), r4(max(e_s))],
                     grouped_backward_kv_ms=r4(med(g_kv)), per_head_backward_kv_ms=r4(med(e_kv)),
                     backward_kv_ratio=round(med(g_kv) / med(e_kv), 3),
                     grouped_backward_kv_windows=[r4(min(g_kv)), r4(max(g_kv))],
                     per_head_backward_kv_windows=[r4(min(e_kv)), r4(max(e_kv))],
                     grouped_step_bytes=step_bytes(True), expanded_step_bytes=step_bytes(False),
                     equal_bits_O_dQ=same_O, max_abs_diff_dK_dV=diff)
                del Q, K, V, dO, q, kk, v, Ke, Ve, dKg, dVg, dKe, dVe, O, stats, delta, dQ, rg, re
                torch.cuda.empty_cache()
        att.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


def dtype_main(a, emit):
    """16-bit operands against float32 ones on the fused passes (see the module docstring)."""
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    dtypes = {"bf16": torch.bfloat16, "fp16": torch.float16}
    med, r4 = statistics.median, lambda x: round(x, 4)      # noqa: E731
    for spec in (a.workloads or "c2:8192,c2:0,c3:8192,c3:0").split(","):
        name, rows, cols, d_rp, d_ci = heads_pattern(spec.partition("@")[0], capi, W, dev, scales)
        wide = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25)
        narrow = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25)
        for k in (int(s) for s in a.ks.split(",")):
            for dname in a.dtype.split(","):
                gen = torch.Generator(device=dev).manual_seed(k)
                ops32 = [torch.randn((n, k), generator=gen, device=dev) for n in (rows, cols, cols, rows)]
                ops16 = [t.to(dtypes[dname]) for t in ops32]
                ops32 = [t.float() for t in ops16]                      # (the same numbers on both sides)
                sets = {}
                for att, (Q, K, V, dO) in ((wide, ops32), (narrow, ops16)):
                    sets[att] = (Q, K, V, dO) + tuple(t.clone().requires_grad_(True) for t in (Q, K, V))

                def forward(att):
                    Q, K, V = sets[att][:3]
                    with torch.no_grad():
                        att(Q, K, V)

                def step(att):
                    dO, q, kk, v = sets[att][3:]
                    att(q, kk, v).backward(dO)
                    q.grad = kk.grad = v.grad = None

                def step_bytes(att):
                    step(att)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    step(att)
                    torch.cuda.synchronize()
                    return torch.cuda.max_memory_allocated() - before

                n_f, w_f, it_f = timed_windows(lambda: forward(narrow), lambda: forward(wide), a.window_ms, a.reps, a.max_iters)
                n_s, w_s, it_s = timed_windows(lambda: step(narrow), lambda: step(wide), a.window_ms, a.reps, a.max_iters)
                with torch.no_grad():
                    diff = float((narrow(*ops16[:3]).float() - wide(*ops32[:3])).abs().max())
                emit(workload=name, dtype=dname, k=k, kv=k, rows=rows, cols=cols, nnz=int(d_ci.numel()), plan=wide.A.spmm_describe(),
                     plan_T=wide.T.spmm_describe(), iters_forward=it_f, iters_step=it_s, reps=a.reps,
                     narrow_forward_ms=r4(med(n_f)), fp32_forward_ms=r4(med(w_f)), forward_ratio=round(med(n_f) / med(w_f), 3),
                     narrow_forward_windows=[r4(min(n_f)), r4(max(n_f))], fp32_forward_windows=[r4(min(w_f)), r4(max(w_f))],
                     narrow_step_ms=r4(med(n_s)), fp32_step_ms=r4(med(w_s)), step_ratio=round(med(n_s) / med(w_s), 3),
                     narrow_step_windows=[r4(min(n_s)), r4(max(n_s))], fp32_step_windows=[r4(min(w_s)), r4(max(w_s))],
                     narrow_step_bytes=step_bytes(narrow), fp32_step_bytes=step_bytes(wide), max_abs_diff_O=diff)
                del ops32, ops16, sets
                torch.cuda.empty_cache()
        wide.close()
        narrow.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


def wide_main(a, emit):
    """--wide: FusedSparseAttention(wide=True) at k = kv = 128 (spmv_csr_attention_*_wide on lane groups of 32) against the
    unchanged FusedSparseAttention at k = kv = 64, the yardstick, on the same pattern arrays in one process, float32 and (--dtype,
    default bf16) 16-bit operands; the windows alternate, median of --reps with the lowest and the highest kept.  A pass gathers
    twice the bytes per nonzero at twice the width, so the expectation is a ratio of 2.0."""
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    dtypes = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
    med, r4 = statistics.median, lambda x: round(x, 4)      # noqa: E731
    for spec in (a.workloads or "c2:8192,c2:0,c3:8192,c3:0").split(","):
        name, rows, cols, d_rp, d_ci = heads_pattern(spec.partition("@")[0], capi, W, dev, scales)
        wide = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.125, wide=True)
        narrow = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.125)
        for dname in ["fp32"] + (a.dtype or "bf16").split(","):
            sets = {}
            for att, k in ((wide, 128), (narrow, 64)):
                gen = torch.Generator(device=dev).manual_seed(k)
                Q, K, V, dO = (torch.randn((n, k), generator=gen, device=dev).to(dtypes[dname]) for n in (rows, cols, cols, rows))
                sets[att] = (Q, K, V, dO) + tuple(t.clone().requires_grad_(True) for t in (Q, K, V))

            def forward(att):
                Q, K, V = sets[att][:3]
                with torch.no_grad():
                    att(Q, K, V)

            def step(att):
                dO, q, kk, v = sets[att][3:]
                att(q, kk, v).backward(dO)
                q.grad = kk.grad = v.grad = None

            w_f, n_f, it_f = timed_windows(lambda: forward(wide), lambda: forward(narrow), a.window_ms, a.reps, a.max_iters)
            w_s, n_s, it_s = timed_windows(lambda: step(wide), lambda: step(narrow), a.window_ms, a.reps, a.max_iters)
            emit(workload=name, dtype=dname, rows=rows, cols=cols, nnz=int(d_ci.numel()), plan=wide.A.spmm_describe(),
                 plan_T=wide.T.spmm_describe(), iters_forward=it_f, iters_step=it_s, reps=a.reps,
                 wide128_forward_ms=r4(med(w_f)), narrow64_forward_ms=r4(med(n_f)), forward_ratio=round(med(w_f) / med(n_f), 3),
                 wide128_forward_windows=[r4(min(w_f)), r4(max(w_f))], narrow64_forward_windows=[r4(min(n_f)), r4(max(n_f))],
                 wide128_step_ms=r4(med(w_s)), narrow64_step_ms=r4(med(n_s)), step_ratio=round(med(w_s) / med(n_s), 3),
                 wide128_step_windows=[r4(min(w_s)), r4(max(w_s))], narrow64_step_windows=[r4(min(n_s)), r4(max(n_s))])
            del sets
            torch.cuda.empty_cache()
        wide.close()
        narrow.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


def bias_main(a, emit):
    """The biased fused holder against the unbiased one and against the composed path with a torch add (see the module docstring)."""
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    med, r4 = statistics.median, lambda x: round(x, 4)      # noqa: E731

    class ComposedBias(torch.autograd.Function):
        """SparseAttentionFunction with bias added to the scaled scores by torch; dBias is dS with respect to t."""

        @staticmethod
        def forward(ctx, att, Q, K, V, bias):
            A = att.A
            A.sddmm(Q, K, att.work)
            att.work.mul_(att.scale).add_(bias)
            A.row_softmax(att.work, att.work, 1.0)
            A.values_changed()
            O = torch.empty((A.rows, V.shape[1]), dtype=torch.float32, device=V.device)
            A.spmm(V, O)
            ctx.att = att
            ctx.save_for_backward(Q, K, V, att.work.clone())
            return O

        @staticmethod
        def backward(ctx, dO):
            att = ctx.att
            A, T, Wk = att.A, att.T, att.work
            Q, K, V, P = ctx.saved_tensors
            dO = dO.contiguous()
            Wk.copy_(P)
            A.values_changed()
            T.transpose_values(A)
            dV = torch.empty_like(V)
            T.spmm(dO, dV)
            A.sddmm(dO, V, Wk)
            A.row_softmax_backward(P, Wk, Wk, 1.0)
            dB = Wk.clone()
            Wk.mul_(att.scale)
            A.values_changed()
            dQ, dK = torch.empty_like(Q), torch.empty_like(K)
            A.spmm(K, dQ)
            T.transpose_values(A)
            T.spmm(Q, dK)
            return None, dQ, dK, dV, dB

    for spec in (a.workloads or "c2:8192,c2:0,c3:8192,c3:0").split(","):
        name, rows, cols, d_rp, d_ci = heads_pattern(spec.partition("@")[0], capi, W, dev, scales)
        nnz = int(d_ci.numel())
        biased = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25, bias=True)
        plain = SA.FusedSparseAttention(rows, cols, d_rp, d_ci, scale=0.25)
        composed = SA.SparseAttention(rows, cols, d_rp, d_ci, scale=0.25)
        for k in (int(s) for s in a.ks.split(",")):
            gen = torch.Generator(device=dev).manual_seed(k)
            Q, K, V, dO = (torch.randn((n, k), generator=gen, device=dev) for n in (rows, cols, cols, rows))
            B = torch.randn((nnz,), generator=gen, device=dev)
            q, kk, v, b = (t.clone().requires_grad_(True) for t in (Q, K, V, B))
            calls = {"biased": lambda *x: biased(*x), "plain": lambda Q, K, V, B: plain(Q, K, V),
                     "composed": lambda *x: ComposedBias.apply(composed, *x)}

            def forward(which):
                with torch.no_grad():
                    calls[which](Q, K, V, B)

            def step(which):
                calls[which](q, kk, v, b).backward(dO)
                q.grad = kk.grad = v.grad = b.grad = None

            def step_bytes(which):
                step(which)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                step(which)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated() - before

            with torch.no_grad():
                diff = float((calls["biased"](Q, K, V, B) - calls["composed"](Q, K, V, B)).abs().max())
            b_f, p_f, it_f = timed_windows(lambda: forward("biased"), lambda: forward("plain"), a.window_ms, a.reps, a.max_iters)
            b_s, p_s, it_s = timed_windows(lambda: step("biased"), lambda: step("plain"), a.window_ms, a.reps, a.max_iters)
            b_f2, c_f, _ = timed_windows(lambda: forward("biased"), lambda: forward("composed"), a.window_ms, a.reps, a.max_iters)
            b_s2, c_s, _ = timed_windows(lambda: step("biased"), lambda: step("composed"), a.window_ms, a.reps, a.max_iters)
            emit(workload=name, k=k, kv=k, rows=rows, cols=cols, nnz=nnz, plan=plain.A.spmm_describe(), plan_T=plain.T.spmm_describe(),
                 iters_forward=it_f, iters_step=it_s, reps=a.reps,
                 biased_forward_ms=r4(med(b_f)), unbiased_forward_ms=r4(med(p_f)), forward_ratio=round(med(b_f) / med(p_f), 3),
                 biased_forward_windows=[r4(min(b_f)), r4(max(b_f))], unbiased_forward_windows=[r4(min(p_f)), r4(max(p_f))],
                 biased_step_ms=r4(med(b_s)), unbiased_step_ms=r4(med(p_s)), step_ratio=round(med(b_s) / med(p_s), 3),
                 biased_step_windows=[r4(min(b_s)), r4(max(b_s))], unbiased_step_windows=[r4(min(p_s)), r4(max(p_s))],
                 composed_forward_ms=r4(med(c_f)), forward_ratio_to_composed=round(med(b_f2) / med(c_f), 3),
                 composed_step_ms=r4(med(c_s)), step_ratio_to_composed=round(med(b_s2) / med(c_s), 3),
                 biased_step_bytes=step_bytes("biased"), unbiased_step_bytes=step_bytes("plain"), composed_step_bytes=step_bytes("composed"),
                 max_abs_diff_O_to_composed=diff)
            del Q, K, V, dO, B, q, kk, v, b
            torch.cuda.empty_cache()
        biased.close()
        plain.close()
        composed.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=None, help="default: c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0; with --heads: " + HEADS_WORKLOADS)
    ap.add_argument("--ks", default=None, help="default: 16,32,64; with --heads: 16,64")
    ap.add_argument("--heads", default=None, help="H[,H..]: time heads=\"loop\" against heads=\"batched\" at these head counts")
    ap.add_argument("--gqa", default=None, help="G[,G..]: time grouped K/V against K/V expanded with repeat_interleave at these group sizes")
    ap.add_argument("--gqa-heads", type=int, default=16, help="query heads of the --gqa runs")
    ap.add_argument("--dtype", default=None, help="bf16[,fp16]: time 16-bit operands against float32 ones on the fused passes")
    ap.add_argument("--bias", action="store_true", help="time FusedSparseAttention(bias=True) against the unbiased and the composed path")
    ap.add_argument("--wide", action="store_true", help="time FusedSparseAttention(wide=True) at k = kv = 128 against the unchanged holder at 64")
    ap.add_argument("--scale", default="", help="name=fraction of the rows, e.g. c4=0.5 where the memory does not hold the full size")
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    capi, W, SA = pkg.capi, pkg.workloads, pkg.sparse_attention
    if capi.device_count() < 1:
        raise SystemExit("attention_time.py needs a HIP device")
    dev = torch.device("cuda:0")
    scales = dict((s.split("=")[0], float(s.split("=")[1])) for s in a.scale.split(",") if s)
    out = open(a.out, "a") if a.out else None

    def emit(**kv):
        line = json.dumps(kv)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if a.wide:
        wide_main(a, emit)
        return
    if a.bias:
        a.ks = a.ks or "16,32,64"
        bias_main(a, emit)
        return
    if a.dtype:
        a.ks = a.ks or "16,32,64"
        dtype_main(a, emit)
        return
    if a.gqa:
        a.ks = a.ks or "16,64"
        gqa_main(a, emit)
        return
    if a.heads:
        a.ks = a.ks or "16,64"
        heads_main(a, emit)
        return
    a.workloads, a.ks = a.workloads or "c2:8192,c2:0,c3:8192,c3:0,c4:8192,c4:0", a.ks or "16,32,64"
    for spec in a.workloads.split(","):
        name, band = spec.split(":")
        w = W.config(name, band=int(band), scale=scales.get(name, 1.0))
        rp = W.row_ptr(w)
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(rp).to(dev)
        d_ci = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_va = torch.empty(nnz, dtype=torch.float32, device=dev)
        capi.synth_fill(w.seed, 0, w.rows, w.rows, w.cols, w.band, d_rp, d_ci, d_va)
        del d_va
        fused = SA.FusedSparseAttention(w.rows, w.cols, d_rp, d_ci, scale=0.25)
        composed = SA.SparseAttention(w.rows, w.cols, d_rp, d_ci, scale=0.25)
        for k in (int(s) for s in a.ks.split(",")):
            gen = torch.Generator(device=dev).manual_seed(k)
            Q, K, V, dO = (torch.randn((n, k), generator=gen, device=dev) for n in (w.rows, w.cols, w.cols, w.rows))
            q, kk, v = (t.clone().requires_grad_(True) for t in (Q, K, V))

            def forward(att):
                with torch.no_grad():
                    att(Q, K, V)

            def step(att):
                att(q, kk, v).backward(dO)
                q.grad = kk.grad = v.grad = None

            def step_bytes(att):
                step(att)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                step(att)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated() - before

            f_fwd, c_fwd, it_f = timed_pair(lambda: forward(fused), lambda: forward(composed), a.window_ms, a.reps, a.max_iters)
            f_step, c_step, it_s = timed_pair(lambda: step(fused), lambda: step(composed), a.window_ms, a.reps, a.max_iters)
            with torch.no_grad():
                diff = float((fused(Q, K, V) - composed(Q, K, V)).abs().max())
            emit(workload=f"{name}_band{band}", k=k, kv=k, rows=w.rows, cols=w.cols, nnz=nnz, plan=fused.A.spmm_describe(),
                 plan_T=fused.T.spmm_describe(), iters_forward=it_f, iters_step=it_s, reps=a.reps,
                 fused_forward_ms=round(f_fwd, 4), composed_forward_ms=round(c_fwd, 4), forward_ratio=round(f_fwd / c_fwd, 3),
                 fused_step_ms=round(f_step, 4), composed_step_ms=round(c_step, 4), step_ratio=round(f_step / c_step, 3),
                 fused_step_bytes=step_bytes(fused), composed_step_bytes=step_bytes(composed), max_abs_diff_O=diff)
            del Q, K, V, dO, q, kk, v
            torch.cuda.empty_cache()
        fused.close()
        composed.close()
        del d_rp, d_ci
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
