// kernels_attention.hip -- O = softmax_rows(scale * Q K^T at the pattern) V and its gradients in three row-parallel passes
// that never store a score, a probability or their gradients (spmv_csr_attention_forward, spmv_csr_attention_backward_q,
// spmv_csr_attention_backward_kv, include/spmv_hip.h "Fused attention").  Of nnz size only col_idx is read, once per pass.
//
// The lane groups, their steps and the plan are lane_group.hpp's, with V = pow2 >= ceil(max(k, kv) / 4): 1 to 16 up to width 64,
// and through the _wide entry points alone V = 32 for widths 65 to 128, in steps of kWideStep = 8 nonzeros that the lanes
// sub < 8 of the group own (a scratch slot of 260 floats per piece there: at_slots, AttnPlan::d_scratch_wide).  Lane s keeps
// columns [4s, 4s+4) of the row's own operands in registers (Q_i; dO_i; K_j and V_j on the transposed handle).  Per step a
// lane issues all its gathers (2 T slices, and on the transposed handle the 12 bytes stats[2i], stats[2i+1], delta[i] per
// nonzero, loaded by the lane that owns the nonzero) and only then computes.  The scores of a step go through
// reduce_scatter; the lane that ends up with a score turns it into e, p or ds and broadcasts that.
//
// The order of the fp32 operations (the header states it; tests/test_attention_host.py emulates it).  Nothing below is
// contracted by the compiler (fp contract is off in this file): an fma is one where fmaf is written, and nowhere else.
//   score    s = spmv_csr_sddmm's number for k: the dot product of lane_group.hpp, which also says why a V wider than SDDMM's
//            for this k (kv > k) changes no bit.  dp = dO_i . V_j likewise over kv.  t = scale * s (rounded).
//   forward  a span is a whole row of at most 512 nonzeros or a plan piece; m = -Inf, l = +0, acc = +0; per step of T:
//              m' = max(m, the step's t)  (fmaxf: a NaN is ignored here);  z = m' == -Inf ? 0 : m'
//              a = expf(m - z);  e_t = expf(t_t - z);  l = l * a;  acc[c] = acc[c] * a
//              for t in storage order:  l = l + e_t;  acc[c] = fma(e_t, V[j_t][c], acc[c])
//            a row of one span: r = 1.0f / l, O[c] = acc[c] * r, stats = (m, r).  A row in pieces: M = max m_p,
//            z = M == -Inf ? 0 : M, then from +0 in piece order w_p = expf(m_p - z), l = fma(l_p, w_p, l),
//            acc[c] = fma(acc_p[c], w_p, acc[c]); r, O and stats = (M, r) as above.  An empty row: O = 0, stats = (-Inf, +0).
//   p        = expf(t - M_i) * r_i in both backward passes (t - M_i rounded, then the product)
//   delta_i  d_s = +0, d_s = fma(dO[i][c], O[i][c], d_s) over the lane's columns below kv, then the xor butterfly
//   ds       = scale * (p * (dp - delta_i))   (three roundings)
//   dQ_i[c]  = fma(ds, K[j][c], dQ_i[c]) over the span in storage order from +0; the spans of a row added in piece order from +0
//   dV_j[c]  = fma(p, dO[i][c], dV_j[c]),  dK_j[c] = fma(ds, Q[i][c], dK_j[c])  over T's span likewise
// So a row's outputs are a function of its column list in storage order, its operands, k, kv and scale: not of any ld, of
// the 16-byte or 4-byte load path, of the row's place or neighbours, of a rebased row_ptr or of the handle.  (T depends on
// V, hence on max(k, kv) only.)
//
// Heads.  Every kernel serves one query head of a launch: head = blockIdx.z * gridDim.y + blockIdx.y (query_head).  The grid's
// y extent is the group g of query heads that share one K/V head and z is that K/V head, so no kernel divides: it advances K
// and V by z x stride and every other base by head x stride once at entry (at_head; wave-uniform) and uses the slice of the
// scratch at head x pieces x kAtSlots.  The _heads calls launch with g = 1 (y extent 1, the head in z), a call of one head
// is the same kernel at a grid of y = z = 1 with every stride 0: head y of a call is that call on the advanced pointers bit
// for bit.  (k_attn_add_pieces takes no K or V and keeps the head in a 2-D grid's y; query_head reads that alike.)
//
// Grouped-query heads (the _gqa calls).  Forward, backward_q and every *_pieces kernel are the kernels above at g > 1.  Only
// backward_kv's sum over the heads of a group is new: k_attn_bwd_kv_rows_gqa (a lane group keeps K_j, V_j and walks its row of T
// once per query head of the group) and k_attn_add_pieces_gqa (the long rows) form, per K/V head c,
//   dK_c = (..((dK^(0) + dK^(1)) + dK^(2)) .. + dK^(g-1)),  dV_c alike,
// with dK^(i), dV^(i) the single-head numbers of query head c g + i (spans from +0, a long row's pieces in piece order from
// +0), added in head order from head 0's value, not from +0.  g = 1 adds nothing: the _heads bits.
//
// Element types.  Every kernel, span function and launch function takes the element type E of the matrices (Q, K, V, O, dO, dQ, dK,
// dV) as its last template argument: float (the nine fp32 entry points) or 16-bit storage (bf16, fp16: the _16 entry points).
// The text above is E = float.  With 16-bit E nothing of the order changes: a step's gathered slices wait packed as loaded
// (slice_t<E>, 2 registers per slice) and are widened exactly to fp32 at each use (widen, widen_again), the row's own operands
// are widened once (load_wide), every sum above is the same fp32 operation, and store_slice rounds an output to E once, to
// nearest even.  stats, delta, the scratch and the LDS slots of k_attn_bwd_kv_rows_gqa hold floats whatever E is.  So a 16-bit
// call is, bit for bit, the fp32 call on the widened operands with O, dQ, dK and dV rounded once.
//
// The additive bias (the _bias entry points; include/spmv_hip.h "Fused attention with an additive bias").  The spans take a
// compile-time BIAS switch; off, they are the code above.  On, t = (scale * s) + bias[n], two roundings, where n is the nonzero's
// position in the storage order of the handle the pass runs on (backward_kv: the transposed handle's, bias_t); everything after
// t is the order above.  The lane that ends up with the score of a nonzero after reduce_scatter loads its bias (4 coalesced
// bytes per nonzero, none past the span's end, with the step's gathers or after reduce_scatter: kBiasEarly) and, in
// backward_q, stores dBias[n] = p * (dp - delta), whose product with scale is ds: every position once, no atomics.  The bias
// pointers are one more kernel argument (AttnBias), the only element of the argument pack that ends each of the seven kernels
// that run a span: k_attn_fwd_rows<V, VEC, E, AttnBias> is the biased kernel, k_attn_fwd_rows<V, VEC, E> with its empty pack the
// unbiased one, whose AttnArgsT, kernarg segment and code hold nothing of the bias.
//
// The scratch of the long rows (AttnPlan): per head, kAtSlots floats per piece: [0] m_p, [1] l_p, [4, 132) up to 128 partial sums
// (forward acc_p[kv]; backward_q dQ_p[k]; backward_kv dK_p[k] at 4 and dV_p[kv] at 68).
#include <initializer_list>
#include "lane_group.hpp"

#pragma clang fp contract(off)

#ifdef SPMV_ATTN_WIDE_STEP      // (include/spmv_hip.h states the step of the wide calls: its bits are part of the interface)
static_assert(spmv::kWideStep == SPMV_ATTN_WIDE_STEP, "lane_group.hpp and include/spmv_hip.h disagree on T_wide");
#endif

namespace spmv {

namespace {

constexpr int kAtSlots = 132;     // floats of scratch per piece
constexpr int kAtSums = 4;        // where a piece's partial sums start (16-byte aligned)
constexpr int kAtSums2 = 68;      // the second set of backward_kv (dV)
// V = 32 (the _wide entry points at 64 < max(k, kv) <= 128) has a scratch of its own (AttnPlan::d_scratch_wide): per head and
// piece [0] m_p, [1] l_p, [4, 132) up to 128 partial sums, [132, 260) backward_kv's second 128
constexpr int kAtSlotsWide = 4 + 2 * 128;
constexpr int kAtSums2Wide = 4 + 128;
template <int V>
constexpr int at_slots = V > 16 ? kAtSlotsWide : kAtSlots;
template <int V>
constexpr int at_sums2 = V > 16 ? kAtSums2Wide : kAtSums2;

// the query head of the block: blockIdx.y within its group of gridDim.y heads, the group (= the K/V head) in blockIdx.z
__device__ __forceinline__ int64_t query_head() { return (int64_t)blockIdx.z * gridDim.y + blockIdx.y; }

// the operands of the block's head: every base advanced once, by a wave-uniform number (scalar work); K and V by the K/V
// head, everything else by the query head
template <typename E>
__device__ __forceinline__ AttnArgsT<E> at_head(AttnArgsT<E> a)
{
    const int64_t y = query_head(), c = blockIdx.z;
    a.Q += y * a.hq, a.K += c * a.hk, a.V += c * a.hv, a.O += y * a.ho, a.dO += y * a.hdo;
    a.stats_in += y * a.hstats_in, a.delta_in += y * a.hdelta_in;
    a.out0 += y * a.h0, a.out1 += y * a.h1, a.stats += y * a.hstats, a.delta += y * a.hdelta;
#if defined(__HIP_DEVICE_COMPILE__)
    // each base is formed here, not where it is first used: its stride and the head then stop occupying scalar registers
    // (an empty statement per pointer, so that one a pass does not use still disappears)
    asm("" : "+s"(a.Q));
    asm("" : "+s"(a.K));
    asm("" : "+s"(a.V));
    asm("" : "+s"(a.O));
    asm("" : "+s"(a.dO));
    asm("" : "+s"(a.stats_in));
    asm("" : "+s"(a.delta_in));
    asm("" : "+s"(a.out0));
    asm("" : "+s"(a.out1));
    asm("" : "+s"(a.stats));
    asm("" : "+s"(a.delta));
#endif
    return a;
}

// the scratch of the block's head: query head y owns the slice at y * pieces * kAtSlots (formed at entry like the bases above)
template <int V>
__device__ __forceinline__ float *at_head_scratch(const GroupPieces &g)
{
    float *s = g.scratch + query_head() * g.npieces * at_slots<V>;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(s));
#endif
    return s;
}

// A kernel that runs a span ends in an argument pack `B... bb`: empty, or one AttnBias (BIAS = sizeof...(B) == 1), which
// bias_of(bb...) reads.  The instantiation with the empty pack has neither the argument nor any code for it.
__device__ __forceinline__ AttnBias bias_of() { return AttnBias{}; }
__device__ __forceinline__ AttnBias bias_of(AttnBias b) { return b; }

// the bias of the block's query head (formed at entry like the bases above).  A null dbias stays null.
__device__ __forceinline__ AttnBias at_head(AttnBias b)
{
    const int64_t y = query_head();
    b.bias += y * b.hbias;
    b.dbias = b.dbias ? b.dbias + y * b.hdbias : nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(b.bias));
    asm("" : "+s"(b.dbias));
#endif
    return b;
}

// The bias of the step's nonzeros kb + i V + sub, one coalesced 4-byte load per nonzero by the lane that ends up with its
// score (0 past the end e, and in a lane that owns no nonzero of a step narrower than the group: no load).  A span issues it with the step's gathers (kBiasEarly) or, where that costs the kernel
// a register it does not have, after reduce_scatter; the bits are the same.
template <int V>
__device__ __forceinline__ void load_bias(const float *__restrict__ bias, int64_t kb, int64_t e, int sub, float (&bl)[LaneGeom<V>::L])
{
#pragma unroll
    for (int i = 0; i < LaneGeom<V>::L; ++i) {
        const int64_t n = kb + (int64_t)i * V + sub;
        bl[i] = LaneGeom<V>::owner(sub) && n < e ? bias[n] : 0.0f;
    }
}

// where the early load would cost the kernel a wave per SIMD or a spill (profiles/lane_group_resource_usage.md, "with bias")
template <int PASS, int V, typename E>
constexpr bool kBiasEarly = PASS == kPassForward     ? !(kIs16<E> && V <= 2)
                            : PASS == kPassBackwardQ ? !((kIs16<E> && V == 1) || V == 4 || V == 8)
                                                     : !(V == 1 || (V == 8 && !kIs16<E>));

// The waves per SIMD asked of a kernel with a bias: the unbiased instantiation's, where the compiler then fits the bias's
// registers without scratch (1: no floor; elsewhere a floor only turns registers into scratch, and without a bias nothing is
// asked).  This table and kBiasEarly above are read off one compiler's register allocation: `python
// tools/attention_bias_resources.py` compiles this file, prints every biased instantiation beside its unbiased one (the
// table of profiles/lane_group_resource_usage.md) and fails on scratch, so run it after a change to a span or a new ROCm and
// move the entries with what it shows.
enum BiasKernel { kBiasBwdQRows, kBiasBwdKvRows };
template <BiasKernel KERNEL, int V, bool VEC, typename E, typename... B>
constexpr int bias_waves()
{
    if (sizeof...(B) == 0) return 1;
    if (KERNEL == kBiasBwdQRows) return V == 8 && !VEC && std::is_same<E, bf16>::value ? 5 : 1;
    return V == 1 && !VEC && kIs16<E> ? 4 : 1;       // kBiasBwdKvRows
}
#if defined(__HIP_DEVICE_COMPILE__)
#define SPMV_BIAS_WAVES(KERNEL) __attribute__((amdgpu_waves_per_eu(bias_waves<KERNEL, V, VEC, E, B...>())))
#else
#define SPMV_BIAS_WAVES(KERNEL)
#endif

// ---- forward: (m, l, acc) of the nonzeros [b, e) of the group's row.  All lanes of a group call it with the same b, e. ----
// BIAS (here and in the two spans below): the score of nonzero n is t = (scale * s) + bias[n], two roundings.
template <int V, bool VEC, typename E, bool BIAS = false>
__device__ __forceinline__ void fwd_span(int lane, int64_t b, int64_t e, const AttnArgsT<E> &a, float4 q,
                                         const int32_t *__restrict__ col_idx, int c0, float &m, float &l, float4 &acc,
                                         const float *__restrict__ bias = nullptr)
{
    constexpr bool kEarly = kBiasEarly<kPassForward, V, E>;
    constexpr int T = LaneGeom<V>::T, L = LaneGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int nk = a.k - c0, nv = a.kv - c0;
    m = -INFINITY;
    l = 0.0f;
    acc = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        group_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        [[maybe_unused]] float bl[L];
        if constexpr (BIAS && kEarly) load_bias<V>(bias, kb, e, sub, bl);
        slice_t<E> xk[T], xv[T];      // as loaded: 16-bit elements stay packed until they are used
#pragma unroll
        for (int t = 0; t < T; ++t) xk[t] = (nk > 0 && kb + t < e) ? load_slice<VEC>(a.K, a.ldk, ct[t], c0, a.k) : zero_slice<E>();
#pragma unroll
        for (int t = 0; t < T; ++t) xv[t] = (nv > 0 && kb + t < e) ? load_slice<VEC>(a.V, a.ldv, ct[t], c0, a.kv) : zero_slice<E>();
        float p[T];
#pragma unroll
        for (int t = 0; t < T; ++t) p[t] = dot_partial(q, widen<E>(xk[t]), nk);
        reduce_scatter<V, T>(p, sub, gbase);
        if constexpr (BIAS && !kEarly) load_bias<V>(bias, kb, e, sub, bl);
        float tl[L], sm = -INFINITY;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const bool in = LaneGeom<V>::owner(sub) && kb + i * V + sub < e;
            if constexpr (BIAS) tl[i] = in ? a.scale * p[i * V] + bl[i] : -INFINITY;
            else tl[i] = in ? a.scale * p[i * V] : -INFINITY;
            sm = fmaxf(sm, tl[i]);
        }
        const float mn = fmaxf(m, group_max<V>(sm));
        const float z = mn == -INFINITY ? 0.0f : mn;
        const float alpha = expf(m - z);
        float el[L], et[T];
#pragma unroll
        for (int i = 0; i < L; ++i) el[i] = expf(tl[i] - z);
        group_bcast<V, T>(el, et, gbase);
        l = l * alpha;
        acc.x = acc.x * alpha;
        acc.y = acc.y * alpha;
        acc.z = acc.z * alpha;
        acc.w = acc.w * alpha;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {
                l = l + et[t];
                const float4 wv = widen<E>(xv[t]);
                acc.x = fmaf(et[t], wv.x, acc.x);
                acc.y = fmaf(et[t], wv.y, acc.y);
                acc.z = fmaf(et[t], wv.z, acc.z);
                acc.w = fmaf(et[t], wv.w, acc.w);
            }
        }
        m = mn;
    }
}

__device__ __forceinline__ float4 scaled4(float4 a, float r) { return make_float4(a.x * r, a.y * r, a.z * r, a.w * r); }

__device__ __forceinline__ void store_stats(float *stats, int64_t r, float m, float rinv)
{
    *reinterpret_cast<float2 *>(stats + 2 * r) = make_float2(m, rinv);
}

// Each of the seven kernels that run a span is one template for both: <V, VEC, E> is the unbiased kernel, <V, VEC, E, AttnBias>
// takes the bias as one more argument and hands that of the block's query head to the span (bias_of above).
template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) void k_attn_fwd_rows(GroupRows g, AttnArgsT<E> a0, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1;
    const AttnArgsT<E> a = at_head(a0);
    [[maybe_unused]] const float *bias = nullptr;
    if constexpr (BIAS) bias = at_head(bias_of(bb...)).bias;
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = group_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    if (e == b) {
        if (c0 < a.kv) store_slice<VEC>(a.out0 + r * a.ld0 + c0, zero4(), c0, a.kv);
        if (sub == 0) store_stats(a.stats, r, -INFINITY, 0.0f);
        return;
    }
    const float4 q = c0 < a.k ? load_wide<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    float m, l;
    float4 acc;
    fwd_span<V, VEC, E, BIAS>(lane, b, e, a, q, g.col_idx, c0, m, l, acc, bias);
    const float rinv = 1.0f / l;
    if (c0 < a.kv) store_slice<VEC>(a.out0 + r * a.ld0 + c0, scaled4(acc, rinv), c0, a.kv);
    if (sub == 0) store_stats(a.stats, r, m, rinv);
}

template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) void k_attn_fwd_pieces(GroupPieces g, AttnArgsT<E> a0, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1;
    const AttnArgsT<E> a = at_head(a0);
    [[maybe_unused]] const float *bias = nullptr;
    if constexpr (BIAS) bias = at_head(bias_of(bb...)).bias;
    float *const scratch = at_head_scratch<V>(g);
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    int lo;
    const int64_t p = group_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    const float4 q = c0 < a.k ? load_wide<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    float m, l;
    float4 acc;
    fwd_span<V, VEC, E, BIAS>(lane, b, e, a, q, g.col_idx, c0, m, l, acc, bias);
    float *s = scratch + p * at_slots<V>;
    if (sub == 0) *reinterpret_cast<float2 *>(s) = make_float2(m, l);
    if (c0 < a.kv) *reinterpret_cast<float4 *>(s + kAtSums + c0) = acc;
}

// a group per long row: the pieces' (m_p, l_p, acc_p) folded in piece order
template <int V, bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_attn_fwd_combine(GroupPieces g, AttnArgsT<E> a0)
{
    const AttnArgsT<E> a = at_head(a0);
    const int sub = threadIdx.x & (V - 1), c0 = 4 * sub;
    const int64_t i = (int64_t)blockIdx.x * (kBlock / V) + threadIdx.x / V;
    if (i >= g.n_long) return;
    const int64_t r = g.long_row[i];
    const int f = g.long_first[i], n = g.long_first[i + 1];
    const float *scratch = at_head_scratch<V>(g);
    float M = -INFINITY;
    for (int p = f; p < n; ++p) M = fmaxf(M, scratch[(int64_t)p * at_slots<V>]);
    const float z = M == -INFINITY ? 0.0f : M;
    float l = 0.0f;
    float4 acc = zero4();
    for (int p = f; p < n; ++p) {
        const float *s = scratch + (int64_t)p * at_slots<V>;
        const float w = expf(s[0] - z);
        l = fmaf(s[1], w, l);
        if (c0 < a.kv) {
            const float4 x = *reinterpret_cast<const float4 *>(s + kAtSums + c0);
            acc.x = fmaf(x.x, w, acc.x);
            acc.y = fmaf(x.y, w, acc.y);
            acc.z = fmaf(x.z, w, acc.z);
            acc.w = fmaf(x.w, w, acc.w);
        }
    }
    const float rinv = 1.0f / l;
    if (c0 < a.kv) store_slice<VEC>(a.out0 + r * a.ld0 + c0, scaled4(acc, rinv), c0, a.kv);
    if (sub == 0) store_stats(a.stats, r, M, rinv);
}

// ---- backward_q: dQ of the nonzeros [b, e) of row i, whose q, dO slice g, (M, rinv) and delta the group holds -------------
// BIAS: the lane that forms p (dp - delta) of a nonzero also stores it to dbias at the nonzero's position (if dbias is not null)
template <int V, bool VEC, typename E, bool BIAS = false>
__device__ __forceinline__ float4 bwdq_span(int lane, int64_t b, int64_t e, const AttnArgsT<E> &a, float4 q, float4 g, float M,
                                            float rinv, float delta, const int32_t *__restrict__ col_idx, int c0,
                                            const float *__restrict__ bias = nullptr, float *__restrict__ dbias = nullptr)
{
    constexpr bool kEarly = kBiasEarly<kPassBackwardQ, V, E>;
    constexpr int T = LaneGeom<V>::T, L = LaneGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int nk = a.k - c0, nv = a.kv - c0;
    float4 dq = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        group_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        [[maybe_unused]] float bl[L];
        if constexpr (BIAS && kEarly) load_bias<V>(bias, kb, e, sub, bl);
        slice_t<E> xk[T], xv[T];      // as loaded: 16-bit elements stay packed until they are used
#pragma unroll
        for (int t = 0; t < T; ++t) xk[t] = (nk > 0 && kb + t < e) ? load_slice<VEC>(a.K, a.ldk, ct[t], c0, a.k) : zero_slice<E>();
#pragma unroll
        for (int t = 0; t < T; ++t) xv[t] = (nv > 0 && kb + t < e) ? load_slice<VEC>(a.V, a.ldv, ct[t], c0, a.kv) : zero_slice<E>();
        float ps[T], pd[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            ps[t] = dot_partial(q, widen<E>(xk[t]), nk);
            pd[t] = dot_partial(g, widen<E>(xv[t]), nv);
        }
        reduce_scatter<V, T>(ps, sub, gbase);
        reduce_scatter<V, T>(pd, sub, gbase);
        if constexpr (BIAS && !kEarly) load_bias<V>(bias, kb, e, sub, bl);
        float dl[L], dt[T];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            if constexpr (BIAS) {
                const float t = a.scale * ps[i * V] + bl[i];
                const float p = expf(t - M) * rinv;
                const float db = p * (pd[i * V] - delta);
                const int64_t n = kb + (int64_t)i * V + sub;
                if constexpr (T < V) {
                    if (dbias && sub < T && n < e) dbias[n] = db;
                } else {
                    if (dbias && n < e) dbias[n] = db;
                }
                dl[i] = a.scale * db;
            } else {
                const float t = a.scale * ps[i * V];
                const float p = expf(t - M) * rinv;
                dl[i] = a.scale * (p * (pd[i * V] - delta));
            }
        }
        group_bcast<V, T>(dl, dt, gbase);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {
                const float4 wk = widen_again<E>(xk[t]);
                dq.x = fmaf(dt[t], wk.x, dq.x);
                dq.y = fmaf(dt[t], wk.y, dq.y);
                dq.z = fmaf(dt[t], wk.z, dq.z);
                dq.w = fmaf(dt[t], wk.w, dq.w);
            }
        }
    }
    return dq;
}

// delta of row r (every lane of the group gets it) and the row's dO slice
template <int V, bool VEC, typename E>
__device__ __forceinline__ float at_delta(const AttnArgsT<E> &a, int64_t r, int c0, float4 &g)
{
    float4 o = zero4();
    g = zero4();
    if (c0 < a.kv) {
        g = load_wide<VEC>(a.dO, a.lddo, r, c0, a.kv);
        o = load_wide<VEC>(a.O, a.ldo, r, c0, a.kv);
    }
    return group_sum<V>(dot_partial(g, o, a.kv - c0));
}

template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) SPMV_BIAS_WAVES(kBiasBwdQRows) void k_attn_bwd_q_rows(GroupRows g, AttnArgsT<E> a0, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1;
    const AttnArgsT<E> a = at_head(a0);
    [[maybe_unused]] AttnBias bi{};
    if constexpr (BIAS) bi = at_head(bias_of(bb...));
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = group_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    if (e == b) {
        if (c0 < a.k) store_slice<VEC>(a.out0 + r * a.ld0 + c0, zero4(), c0, a.k);
        if (sub == 0) a.delta[r] = 0.0f;
        return;
    }
    float4 go;
    const float delta = at_delta<V, VEC, E>(a, r, c0, go);
    const float4 q = c0 < a.k ? load_wide<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    const float2 st = *reinterpret_cast<const float2 *>(a.stats_in + 2 * r);
    const float4 dq = bwdq_span<V, VEC, E, BIAS>(lane, b, e, a, q, go, st.x, st.y, delta, g.col_idx, c0, bi.bias, bi.dbias);
    if (c0 < a.k) store_slice<VEC>(a.out0 + r * a.ld0 + c0, dq, c0, a.k);
    if (sub == 0) a.delta[r] = delta;
}

template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_q_pieces(GroupPieces g, AttnArgsT<E> a0, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1;
    const AttnArgsT<E> a = at_head(a0);
    [[maybe_unused]] AttnBias bi{};
    if constexpr (BIAS) bi = at_head(bias_of(bb...));
    float *const scratch = at_head_scratch<V>(g);
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    int lo;
    const int64_t p = group_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    float4 go;
    const float delta = at_delta<V, VEC, E>(a, r, c0, go);      // (every piece of the row computes the same bits)
    const float4 q = c0 < a.k ? load_wide<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    const float2 st = *reinterpret_cast<const float2 *>(a.stats_in + 2 * r);
    const float4 dq = bwdq_span<V, VEC, E, BIAS>(lane, b, e, a, q, go, st.x, st.y, delta, g.col_idx, c0, bi.bias, bi.dbias);
    if (c0 < a.k) *reinterpret_cast<float4 *>(scratch + p * at_slots<V> + kAtSums + c0) = dq;
    if (sub == 0 && p == g.long_first[lo]) a.delta[r] = delta;
}

// a group per long row: out[row][c] = the pieces' partial sums at scratch offset `off`, added in piece order from +0
// (hout: floats from one head's out to the next)
template <int V, bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_attn_add_pieces(GroupPieces g, int off, E *__restrict__ out, int64_t ld, int w,
                                                            int64_t hout)
{
    const int sub = threadIdx.x & (V - 1), c0 = 4 * sub;
    const int64_t i = (int64_t)blockIdx.x * (kBlock / V) + threadIdx.x / V;
    if (i >= g.n_long || c0 >= w) return;
    const float *scratch = at_head_scratch<V>(g);
    out += query_head() * hout;
    float4 acc = zero4();
    for (int p = g.long_first[i]; p < g.long_first[i + 1]; ++p) {
        const float4 x = *reinterpret_cast<const float4 *>(scratch + (int64_t)p * at_slots<V> + off + c0);
        acc.x = acc.x + x.x;
        acc.y = acc.y + x.y;
        acc.z = acc.z + x.z;
        acc.w = acc.w + x.w;
    }
    store_slice<VEC>(out + (int64_t)g.long_row[i] * ld + c0, acc, c0, w);
}

// ---- backward_kv on the transposed pattern: (dK, dV) of the nonzeros [b, e) of row j, whose K and V slices the group holds
// BIAS: `bias` is in the transposed handle's storage order (spmv_csr_transpose_gather made it)
template <int V, bool VEC, typename E, bool BIAS = false>
__device__ __forceinline__ void bwdkv_span(int lane, int64_t b, int64_t e, const AttnArgsT<E> &a, float4 kj, float4 vj,
                                           const int32_t *__restrict__ col_idx, int c0, float4 &dk, float4 &dv,
                                           const float *__restrict__ bias = nullptr)
{
    constexpr bool kEarly = kBiasEarly<kPassBackwardKV, V, E>;
#if defined(__HIP_DEVICE_COMPILE__)
    // one lane per row on the 4-byte path: the pass is out of scalar registers (106), so the bias base waits in vector ones
    if constexpr (BIAS && V == 1 && !VEC) asm("" : "+v"(bias));
#endif
    constexpr int T = LaneGeom<V>::T, L = LaneGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int nk = a.k - c0, nv = a.kv - c0;
    dk = zero4();
    dv = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        group_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        float2 st[L];
        float de[L];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const bool in = LaneGeom<V>::owner(sub) && kb + i * V + sub < e;
            st[i] = in ? *reinterpret_cast<const float2 *>(a.stats_in + 2 * (int64_t)c[i]) : make_float2(0.0f, 0.0f);
            de[i] = in ? a.delta_in[c[i]] : 0.0f;
        }
        [[maybe_unused]] float bl[L];
        if constexpr (BIAS && kEarly) load_bias<V>(bias, kb, e, sub, bl);
        slice_t<E> xq[T], xg[T];
#pragma unroll
        for (int t = 0; t < T; ++t) xq[t] = (nk > 0 && kb + t < e) ? load_slice<VEC>(a.Q, a.ldq, ct[t], c0, a.k) : zero_slice<E>();
#pragma unroll
        for (int t = 0; t < T; ++t) xg[t] = (nv > 0 && kb + t < e) ? load_slice<VEC>(a.dO, a.lddo, ct[t], c0, a.kv) : zero_slice<E>();
        float ps[T], pd[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            ps[t] = dot_partial(kj, widen<E>(xq[t]), nk);
            pd[t] = dot_partial(vj, widen<E>(xg[t]), nv);
        }
        reduce_scatter<V, T>(ps, sub, gbase);
        reduce_scatter<V, T>(pd, sub, gbase);
        if constexpr (BIAS && !kEarly) load_bias<V>(bias, kb, e, sub, bl);
        float pl[L], dl[L], pt[T], dt[T];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            float t = a.scale * ps[i * V];
            if constexpr (BIAS) t = t + bl[i];
            pl[i] = expf(t - st[i].x) * st[i].y;
            dl[i] = a.scale * (pl[i] * (pd[i * V] - de[i]));
        }
        group_bcast<V, T>(pl, pt, gbase);
        group_bcast<V, T>(dl, dt, gbase);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {
                const float4 wg = widen_again<E>(xg[t]);
                dv.x = fmaf(pt[t], wg.x, dv.x);
                dv.y = fmaf(pt[t], wg.y, dv.y);
                dv.z = fmaf(pt[t], wg.z, dv.z);
                dv.w = fmaf(pt[t], wg.w, dv.w);
                const float4 wq = widen_again<E>(xq[t]);
                dk.x = fmaf(dt[t], wq.x, dk.x);
                dk.y = fmaf(dt[t], wq.y, dk.y);
                dk.z = fmaf(dt[t], wq.z, dk.z);
                dk.w = fmaf(dt[t], wq.w, dk.w);
            }
        }
    }
}

template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) SPMV_BIAS_WAVES(kBiasBwdKvRows) void k_attn_bwd_kv_rows(GroupRows g, AttnArgsT<E> a0, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1;
    const AttnArgsT<E> a = at_head(a0);
    [[maybe_unused]] const float *bias = nullptr;
    if constexpr (BIAS) bias = at_head(bias_of(bb...)).bias;
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = group_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    float4 dk = zero4(), dv = zero4();
    if (e > b) {
        const float4 kj = c0 < a.k ? load_wide<VEC>(a.K, a.ldk, r, c0, a.k) : zero4();
        const float4 vj = c0 < a.kv ? load_wide<VEC>(a.V, a.ldv, r, c0, a.kv) : zero4();
        bwdkv_span<V, VEC, E, BIAS>(lane, b, e, a, kj, vj, g.col_idx, c0, dk, dv, bias);
    }
    if (c0 < a.k) store_slice<VEC>(a.out0 + r * a.ld0 + c0, dk, c0, a.k);
    if (c0 < a.kv) store_slice<VEC>(a.out1 + r * a.ld1 + c0, dv, c0, a.kv);
}

template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_kv_pieces(GroupPieces g, AttnArgsT<E> a0, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1;
    const AttnArgsT<E> a = at_head(a0);
    [[maybe_unused]] const float *bias = nullptr;
    if constexpr (BIAS) bias = at_head(bias_of(bb...)).bias;
    float *const scratch = at_head_scratch<V>(g);
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    int lo;
    const int64_t p = group_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    const float4 kj = c0 < a.k ? load_wide<VEC>(a.K, a.ldk, r, c0, a.k) : zero4();
    const float4 vj = c0 < a.kv ? load_wide<VEC>(a.V, a.ldv, r, c0, a.kv) : zero4();
    float4 dk, dv;
    bwdkv_span<V, VEC, E, BIAS>(lane, b, e, a, kj, vj, g.col_idx, c0, dk, dv, bias);
    float *s = scratch + p * at_slots<V>;
    if (c0 < a.k) *reinterpret_cast<float4 *>(s + kAtSums + c0) = dk;
    if (c0 < a.kv) *reinterpret_cast<float4 *>(s + at_sums2<V> + c0) = dv;
}


__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// What a lane of k_attn_bwd_kv_rows_gqa needs only between two heads waits in LDS while the next head's span runs: N 16-byte
// slots of the lane's own (slot n of lane t at [n * kBlock + t]).  Only the owning lane reads and writes them, so there is no
// barrier; park_fence keeps the compiler from forwarding a parked value in a register instead.  Slots 0 and 1 hold the four
// head strides (every V: 8 KiB per workgroup); at V = 16 slots 2 to 5 hold the dK sum, the dV sum, the row's two output
// addresses and its bounds (b, e) as well (24 KiB).
template <int N>
__device__ __forceinline__ float4 *park_lds()
{
    __shared__ float4 park[N * kBlock];
    return park + threadIdx.x;
}

template <int N, typename X>
__device__ __forceinline__ void park_put(int slot, X x)
{
    static_assert(sizeof(X) == 16, "a slot is 16 bytes");
    __builtin_memcpy(park_lds<N>() + slot * kBlock, &x, 16);
}

template <int N, typename X>
__device__ __forceinline__ X park_get(int slot)
{
    X x;
    __builtin_memcpy(&x, park_lds<N>() + slot * kBlock, 16);
    return x;
}

__device__ __forceinline__ void park_fence() { asm volatile("" ::: "memory"); }

struct Strides2 {
    int64_t a, b;
};
template <typename E>
struct Pointers2 {
    E *k, *v;
};

// a number every lane of the wavefront holds alike, as a scalar again
__device__ __forceinline__ int64_t uniform64(int64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
#else
    return x;
#endif
}

// backward_kv of a group of `group` query heads that share K/V head c = blockIdx.y (grid: row blocks x K/V heads): the lane
// group holds K_j, V_j of its row of T once, walks the row once per query head c * group + i from +0 (bwdkv_span: the
// per-head numbers) and adds the heads' results in head order, starting from head 0's.  The per-head kernel leaves few
// registers free (k_attn_bwd_kv_rows: up to 104 SGPRs; at V = 16 247 to 254 of the 256 VGPRs that two waves per SIMD allow),
// so the head strides, and at V = 16 the running sums, the row's output addresses and its bounds, wait in LDS (park_lds).
// With a bias (<..., AttnBias>) each query head of the group uses its own: the bias base advances per head like Q's, its
// stride waits in one more slot (the last).
template <int V, bool VEC, typename E, typename... B>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_kv_rows_gqa(GroupRows g, AttnArgsT<E> a, int group, B... bb)
{
    constexpr bool BIAS = sizeof...(B) == 1, kPark = V == 16;
    constexpr int N = (kPark ? 6 : 2) + BIAS;
    [[maybe_unused]] const AttnBias bi = bias_of(bb...);
    [[maybe_unused]] const float *bias = nullptr;
    if constexpr (BIAS) {
        bias = bi.bias + (int64_t)blockIdx.y * group * bi.hbias;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("" : "+s"(bias));
#endif
    }
    {
        const int64_t c = blockIdx.y, y0 = c * group;
        a.K += c * a.hk, a.V += c * a.hv, a.out0 += c * a.h0, a.out1 += c * a.h1;
        a.Q += y0 * a.hq, a.dO += y0 * a.hdo, a.stats_in += y0 * a.hstats_in, a.delta_in += y0 * a.hdelta_in;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("" : "+s"(a.K));      // (as at_head: the bases are formed here; c and the K/V strides are dead from here on)
        asm("" : "+s"(a.V));
        asm("" : "+s"(a.out0));
        asm("" : "+s"(a.out1));
        asm("" : "+s"(a.Q));
        asm("" : "+s"(a.dO));
        asm("" : "+s"(a.stats_in));
        asm("" : "+s"(a.delta_in));
#endif
    }
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = group_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    Pointers2<E> out{a.out0 + r * a.ld0 + c0, a.out1 + r * a.ld1 + c0};
    float4 dk = zero4(), dv = zero4();
    if (e > b) {
        const float4 kj = c0 < a.k ? load_wide<VEC>(a.K, a.ldk, r, c0, a.k) : zero4();
        const float4 vj = c0 < a.kv ? load_wide<VEC>(a.V, a.ldv, r, c0, a.kv) : zero4();
        park_put<N>(0, Strides2{a.hq, a.hdo});
        park_put<N>(1, Strides2{a.hstats_in, a.hdelta_in});
        if constexpr (BIAS) park_put<N>(N - 1, Strides2{bi.hbias, 0});
        if constexpr (kPark) {
            park_put<N>(4, out);
            park_put<N>(5, Strides2{b, e});
        }
        float4 sk = zero4(), sv = zero4();
        for (int left = group;;) {
            park_fence();
            if constexpr (kPark) {
                const Strides2 be = park_get<N, Strides2>(5);
                bwdkv_span<V, VEC, E, BIAS>(lane, be.a, be.b, a, kj, vj, g.col_idx, c0, dk, dv, bias);
            } else {
                bwdkv_span<V, VEC, E, BIAS>(lane, b, e, a, kj, vj, g.col_idx, c0, dk, dv, bias);
            }
            if (left != group) {
                if constexpr (kPark) sk = park_get<N, float4>(2), sv = park_get<N, float4>(3);
                dk = add4(sk, dk);
                dv = add4(sv, dv);
            }
            if (--left == 0) break;
            if constexpr (kPark) {
                park_put<N>(2, dk);
                park_put<N>(3, dv);
            } else {
                sk = dk, sv = dv;
            }
            const Strides2 s0 = park_get<N, Strides2>(0), s1 = park_get<N, Strides2>(1);
            a.Q += uniform64(s0.a), a.dO += uniform64(s0.b), a.stats_in += uniform64(s1.a), a.delta_in += uniform64(s1.b);
            if constexpr (BIAS) bias += uniform64(park_get<N, Strides2>(N - 1).a);
        }
        if constexpr (kPark) out = park_get<N, Pointers2<E>>(4);
    }
    if (c0 < a.k) store_slice<VEC>(out.k, dk, c0, a.k);
    if (c0 < a.kv) store_slice<VEC>(out.v, dv, c0, a.kv);
}

// a group per long row of T and K/V head c = blockIdx.y: for each query head c * group + i its pieces' partial sums at scratch
// offset `off`, added in piece order from +0 (k_attn_add_pieces' number), then the heads in head order from head 0's
template <int V, bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_attn_add_pieces_gqa(GroupPieces g, int off, E *__restrict__ out, int64_t ld, int w,
                                                                int64_t hout, int group)
{
    const int sub = threadIdx.x & (V - 1), c0 = 4 * sub;
    const int64_t i = (int64_t)blockIdx.x * (kBlock / V) + threadIdx.x / V;
    if (i >= g.n_long || c0 >= w) return;
    const int64_t c = blockIdx.y, slice = (int64_t)g.npieces * at_slots<V>;
    const float *scratch = g.scratch + c * group * slice;
    float4 acc = zero4();
    for (int y = 0; y < group; ++y, scratch += slice) {
        float4 sum = zero4();
        for (int p = g.long_first[i]; p < g.long_first[i + 1]; ++p)
            sum = add4(sum, *reinterpret_cast<const float4 *>(scratch + (int64_t)p * at_slots<V> + off + c0));
        acc = y ? add4(acc, sum) : sum;
    }
    store_slice<VEC>(out + c * hout + (int64_t)g.long_row[i] * ld + c0, acc, c0, w);
}

// one grid per kernel for all heads: x is what a call of one head launches, y the query head within its group of `group`, z
// the group (the K/V head); group = 1 for the _heads calls.  gqa (backward_kv only): the _gqa call, which sums the heads of a
// group (k_attn_bwd_kv_rows_gqa, k_attn_add_pieces_gqa; also at group = 1).
// bb: the call's bias (a _bias entry point) or null.  The seven kernels that run a span are launched through with_bias: each
// once, with *bb as its last argument (the <..., AttnBias> instantiation) or without one.
template <int PASS, int V, bool VEC, typename E>
int launch_attn_v(const spmv_csr &h, const AttnArgsT<E> &a, const AttnBias *bb, int heads, int group, bool gqa, const char *what,
                  hipStream_t s)
{
    const SpmmPlan &p = h.plan_spmm;
    const int64_t nblocks = group_head_blocks(what, h, V, heads);
    if (nblocks < 0) return SPMV_ERR_INVALID;
    const GroupRows g = group_rows(h, V, nblocks);
    const unsigned kv_heads = (unsigned)(heads / group);
    const dim3 grid((unsigned)nblocks, (unsigned)group, kv_heads), block(kBlock);
    const auto with_bias = [&](auto launch) { bb ? launch(*bb) : launch(); };
    with_bias([&](auto... bias) {
        if constexpr (PASS == kPassForward) hipLaunchKernelGGL((k_attn_fwd_rows<V, VEC, E, decltype(bias)...>), grid, block, 0, s, g, a, bias...);
        else if constexpr (PASS == kPassBackwardQ) hipLaunchKernelGGL((k_attn_bwd_q_rows<V, VEC, E, decltype(bias)...>), grid, block, 0, s, g, a, bias...);
        else if (gqa) hipLaunchKernelGGL((k_attn_bwd_kv_rows_gqa<V, VEC, E, decltype(bias)...>), dim3((unsigned)nblocks, kv_heads), block, 0, s, g, a, group, bias...);
        else hipLaunchKernelGGL((k_attn_bwd_kv_rows<V, VEC, E, decltype(bias)...>), grid, block, 0, s, g, a, bias...);
    });
    SPMV_LAUNCHED("k_attn_*_rows");
    if (!p.n_long) return SPMV_OK;
    const GroupPieces q = group_pieces(h, V > 16 ? h.plan_attn.d_scratch_wide.get() : h.plan_attn.d_scratch.get());
    const dim3 pgrid(group_grid(p.pieces, V).x, (unsigned)group, kv_heads), lgrid(group_grid(p.n_long, V).x, (unsigned)heads);
    if constexpr (PASS == kPassForward) {
        with_bias([&](auto... bias) { hipLaunchKernelGGL((k_attn_fwd_pieces<V, VEC, E, decltype(bias)...>), pgrid, block, 0, s, q, a, bias...); });
        SPMV_LAUNCHED("k_attn_fwd_pieces");
        hipLaunchKernelGGL((k_attn_fwd_combine<V, VEC, E>), dim3(lgrid.x, (unsigned)group, kv_heads), block, 0, s, q, a);
        SPMV_LAUNCHED("k_attn_fwd_combine");
    } else if constexpr (PASS == kPassBackwardQ) {
        with_bias([&](auto... bias) { hipLaunchKernelGGL((k_attn_bwd_q_pieces<V, VEC, E, decltype(bias)...>), pgrid, block, 0, s, q, a, bias...); });
        SPMV_LAUNCHED("k_attn_bwd_q_pieces");
        hipLaunchKernelGGL((k_attn_add_pieces<V, VEC, E>), lgrid, block, 0, s, q, kAtSums, a.out0, a.ld0, a.k, a.h0);
        SPMV_LAUNCHED("k_attn_add_pieces");
    } else {
        with_bias([&](auto... bias) { hipLaunchKernelGGL((k_attn_bwd_kv_pieces<V, VEC, E, decltype(bias)...>), pgrid, block, 0, s, q, a, bias...); });
        SPMV_LAUNCHED("k_attn_bwd_kv_pieces");
        if (gqa) {
            const dim3 cgrid(lgrid.x, kv_heads);
            hipLaunchKernelGGL((k_attn_add_pieces_gqa<V, VEC, E>), cgrid, block, 0, s, q, kAtSums, a.out0, a.ld0, a.k, a.h0, group);
            SPMV_LAUNCHED("k_attn_add_pieces_gqa");
            hipLaunchKernelGGL((k_attn_add_pieces_gqa<V, VEC, E>), cgrid, block, 0, s, q, at_sums2<V>, a.out1, a.ld1, a.kv, a.h1, group);
            SPMV_LAUNCHED("k_attn_add_pieces_gqa");
            return SPMV_OK;
        }
        hipLaunchKernelGGL((k_attn_add_pieces<V, VEC, E>), lgrid, block, 0, s, q, kAtSums, a.out0, a.ld0, a.k, a.h0);
        SPMV_LAUNCHED("k_attn_add_pieces");
        hipLaunchKernelGGL((k_attn_add_pieces<V, VEC, E>), lgrid, block, 0, s, q, at_sums2<V>, a.out1, a.ld1, a.kv, a.h1);
        SPMV_LAUNCHED("k_attn_add_pieces");
    }
    return SPMV_OK;
}

template <int PASS, typename E>
int launch_attn(const spmv_csr &h, const AttnArgsT<E> &a, const AttnBias *bb, int heads, int group, bool gqa, bool vec, const char *what,
                hipStream_t s)
{
    if (h.rows == 0) return SPMV_OK;
    const int slices = ((a.k > a.kv ? a.k : a.kv) + 3) / 4;
    // the sixth geometry, V = 32 in steps of kWideStep: only a _wide entry point admits such widths (capi.hip), and it has made
    // sure of the wide scratch (plan_attention_wide)
    if (slices > 16)
        return vec ? launch_attn_v<PASS, 32, true, E>(h, a, bb, heads, group, gqa, what, s)
                   : launch_attn_v<PASS, 32, false, E>(h, a, bb, heads, group, gqa, what, s);
    return dispatch_lanes(slices, [&](auto v) {
        constexpr int V = decltype(v)::value;
        return vec ? launch_attn_v<PASS, V, true, E>(h, a, bb, heads, group, gqa, what, s)
                   : launch_attn_v<PASS, V, false, E>(h, a, bb, heads, group, gqa, what, s);
    });
}

bool vec4(std::initializer_list<int64_t> lds)
{
    for (int64_t ld : lds)
        if (ld % 4 != 0) return false;
    return true;
}

}  // namespace

// The attention plan: the SpMM plan (made here if it is missing) and the scratch of the long rows' pieces, a slice of
// pieces * kAtSlots floats per head.  It only grows; the scratch it replaces may still be read by work on `s`, so that is
// waited for before the old block goes.
int plan_attention_heads(spmv_csr &h, int heads, hipStream_t s)
{
    if (int rc = plan_spmm(h, s)) return rc;
    if (h.plan_attn.ready && h.plan_attn.heads >= heads) return SPMV_OK;
    DevPtr<float> scratch;
    if (h.plan_spmm.n_long) SPMV_HIP_TRY(scratch.alloc((size_t)heads * (size_t)h.plan_spmm.pieces * kAtSlots));
    if (h.plan_attn.ready) SPMV_HIP_TRY(hipStreamSynchronize(s));
    h.plan_attn.d_scratch = std::move(scratch);     // (the wide scratch, if there is one, stays)
    h.plan_attn.heads = heads;
    h.plan_attn.ready = true;
    return SPMV_OK;
}

// The plan of the _wide entry points: the plan above for `heads` heads and, for V = 32, a scratch of its own of pieces *
// kAtSlotsWide floats per head, a separate allocation that grows like the other (the narrow scratch keeps its layout).
int plan_attention_wide(spmv_csr &h, int heads, hipStream_t s)
{
    if (int rc = plan_attention_heads(h, heads, s)) return rc;
    if (h.plan_attn.wide_heads >= heads) return SPMV_OK;
    DevPtr<float> scratch;
    if (h.plan_spmm.n_long) SPMV_HIP_TRY(scratch.alloc((size_t)heads * (size_t)h.plan_spmm.pieces * kAtSlotsWide));
    if (h.plan_attn.wide_heads) SPMV_HIP_TRY(hipStreamSynchronize(s));
    h.plan_attn.d_scratch_wide = std::move(scratch);
    h.plan_attn.wide_heads = heads;
    return SPMV_OK;
}

int plan_attention(spmv_csr &h, hipStream_t s) { return plan_attention_heads(h, 1, s); }

int64_t attention_plan_bytes(const spmv_csr &h)
{
    if (!h.plan_attn.ready) return 0;
    const int64_t floats = (int64_t)h.plan_attn.heads * kAtSlots + (int64_t)h.plan_attn.wide_heads * kAtSlotsWide;
    return spmm_plan_bytes(h) + (h.plan_spmm.n_long ? floats * h.plan_spmm.pieces * 4 : 0);
}

int attention_max_heads(const spmv_csr &h, int width)
{
    if (width > 64) return (int)group_max_heads(h, 32);     // (the _wide entry points only)
    return dispatch_lanes((width + 3) / 4, [&](auto v) { return (int)group_max_heads(h, decltype(v)::value); });
}

// One call of any of the entry points (arguments checked by capi.hip, which also fills `a`): `heads` query heads, `group`
// of them per K/V head (1 for the _heads calls and a call of one head).  sum_group (backward_kv only): a _gqa call, which sums the
// heads of a group in the kernel, at group = 1 too.  The vector load path (16 bytes of floats, 8 bytes of 16-bit elements)
// needs every ld the pass uses to be a multiple of 4.
namespace {
template <typename E>
int launch_attention_e(AttnPass pass, const spmv_csr &h, const AttnArgsT<E> &a, const AttnBias *bb, int heads, int group, bool sum_group,
                       const char *what, hipStream_t s)
{
    switch (pass) {
        case kPassForward: return launch_attn<kPassForward>(h, a, bb, heads, group, false, vec4({a.ldq, a.ldk, a.ldv, a.ld0}), what, s);
        case kPassBackwardQ:
            return launch_attn<kPassBackwardQ>(h, a, bb, heads, group, false, vec4({a.ldq, a.ldk, a.ldv, a.ldo, a.lddo, a.ld0}), what, s);
        case kPassBackwardKV:
            return launch_attn<kPassBackwardKV>(h, a, bb, heads, group, sum_group, vec4({a.ldq, a.ldk, a.ldv, a.lddo, a.ld0, a.ld1}), what, s);
    }
    return SPMV_ERR_INVALID;
}
}  // namespace

int launch_attention(AttnPass pass, const spmv_csr &h, const AttnArgs &a, const AttnBias *bb, int heads, int group, bool sum_group,
                     const char *what, hipStream_t s)
{
    return launch_attention_e(pass, h, a, bb, heads, group, sum_group, what, s);
}

// the _16 entry points: the same kernels on 16-bit matrices
int launch_attention(AttnPass pass, const spmv_csr &h, const AttnArgsT<bf16> &a, const AttnBias *bb, int heads, int group, bool sum_group,
                     const char *what, hipStream_t s)
{
    return launch_attention_e(pass, h, a, bb, heads, group, sum_group, what, s);
}

int launch_attention(AttnPass pass, const spmv_csr &h, const AttnArgsT<fp16> &a, const AttnBias *bb, int heads, int group, bool sum_group,
                     const char *what, hipStream_t s)
{
    return launch_attention_e(pass, h, a, bb, heads, group, sum_group, what, s);
}

}  // namespace spmv
