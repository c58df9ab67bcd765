// kernels_attention.hip -- O = softmax_rows(scale * Q K^T at the pattern) V and its gradients in three row-parallel passes
// that never store a score, a probability or their gradients (spmv_csr_attention_forward, spmv_csr_attention_backward_q,
// spmv_csr_attention_backward_kv, include/spmv_hip.h "Fused attention").  Of nnz size only col_idx is read, once per pass.
//
// The geometry is kernels_spmm.hip's and kernels_sddmm.hip's, and so is the plan (SpmmPlan: the order of the rows, the
// pieces of the rows of more than 512 nonzeros).  A group of V = pow2 >= ceil(max(k, kv) / 4) lanes owns one row of the
// pattern (or one plan piece): lane s keeps columns [4s, 4s+4) of the row's own operands in registers (Q_i; dO_i; K_j and
// V_j on the transposed handle) and reads the same columns of every row the CSR row refers to.  A group walks its row in
// steps of T = max(V, 8) nonzeros: it loads the step's col_idx coalesced, broadcasts them inside the group, issues all
// gathers of the step (2 T slices per lane, and on the transposed handle the 12 bytes stats[2i], stats[2i+1], delta[i]
// per nonzero, loaded by the lane that owns the nonzero), and only then computes.  The scores of a step go through
// SDDMM's reduce-scatter; the lane that ends up with a score turns it into e, p or ds and broadcasts that.
//
// The order of the fp32 operations (the header states it; tests/test_attention_host.py emulates it).  Nothing below is
// contracted by the compiler (fp contract is off in this file): an fma is one where fmaf is written, and nowhere else.
//   score    s = spmv_csr_sddmm's number for k: p_s = +0, p_s = fma(a[c], b[c], p_s) over the lane's columns below k, then
//            the xor butterfly m = V/2 .. 1.  V may be wider than SDDMM's for this k (kv > k): the extra lanes hold +0, a
//            partial is never -0, so the extra levels add +0 to a number that is not -0.  dp = dO_i . V_j likewise over kv.
//            t = scale * s (rounded).
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
// The scratch of the long rows (AttnPlan): kAtSlots floats per piece: [0] m_p, [1] l_p, [4, 132) up to 128 partial sums
// (forward acc_p[kv]; backward_q dQ_p[k]; backward_kv dK_p[k] at 4 and dV_p[kv] at 68).  Addresses are 64-bit; no buffer
// descriptor and no range check is relied on.  With an ld % 4 != 0 the kernels read and store 4-byte elements below k / kv.
#include <initializer_list>
#include "spmv_internal.hpp"

#pragma clang fp contract(off)

namespace spmv {

namespace {

constexpr int kAtBlock = 256;     // 4 wavefronts
constexpr int kAtSlots = 132;     // floats of scratch per piece
constexpr int kAtSums = 4;        // where a piece's partial sums start (16-byte aligned)
constexpr int kAtSums2 = 68;      // the second set of backward_kv (dV)

// the operands of the three passes (by value; a pass reads what it needs)
struct AttnArgs {
    float scale;
    int k, kv;
    const float *Q;   int64_t ldq;
    const float *K;   int64_t ldk;
    const float *V;   int64_t ldv;
    const float *O;   int64_t ldo;     // backward_q
    const float *dO;  int64_t lddo;    // backward
    const float *stats_in;             // backward
    const float *delta_in;             // backward_kv
    float *out0;      int64_t ld0;     // forward O; backward_q dQ; backward_kv dK
    float *out1;      int64_t ld1;     // backward_kv dV
    float *stats;                      // forward
    float *delta;                      // backward_q
};

// the rows and pieces of a launch
struct AttnRows {
    int64_t rows, nblocks;
    int row_cap;
    const int32_t *order, *row_ptr, *col_idx;
};
struct AttnPieces {
    int npieces, n_long;
    const int32_t *long_row, *long_first, *piece_k0, *piece_len, *col_idx;
    float *scratch;
};

// block b of the grid takes item at_xcd_item(b, n): as spmm_xcd_item, each XCD gets one contiguous range of row blocks
__device__ __forceinline__ int64_t at_xcd_item(int64_t bid, int64_t n)
{
    const int64_t q = n / kXcds, rem = n % kXcds;
    const int64_t j = bid % kXcds, idx = bid / kXcds;
    return j * q + (j < rem ? j : rem) + idx;
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// the four columns [c0, c0+4) of row j of a row-major matrix (c0 < w); VEC: one 16-byte load, else the columns below w only
template <bool VEC>
__device__ __forceinline__ float4 at_slice(const float *__restrict__ M, int64_t ld, int64_t j, int c0, int w)
{
    const float *p = M + j * ld + c0;
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    float4 r = zero4();
    r.x = p[0];
    if (c0 + 1 < w) r.y = p[1];
    if (c0 + 2 < w) r.z = p[2];
    if (c0 + 3 < w) r.w = p[3];
    return r;
}

// the columns [c0, c0+4) below w of one output row (c0 < w)
template <bool VEC>
__device__ __forceinline__ void at_store(float *__restrict__ p, float4 a, int c0, int w)
{
    if (VEC && c0 + 4 <= w) {
        *reinterpret_cast<float4 *>(p) = a;
        return;
    }
    p[0] = a.x;
    if (c0 + 1 < w) p[1] = a.y;
    if (c0 + 2 < w) p[2] = a.z;
    if (c0 + 3 < w) p[3] = a.w;
}

// the lane's partial of a dot product: fma over its n1 = w - c0 columns (at most 4) from +0; +0 for an idle lane
__device__ __forceinline__ float at_partial(float4 u, float4 x, int n1)
{
    float a = 0.0f;
    if (n1 > 0) {
        a = fmaf(u.x, x.x, a);
        if (n1 > 1) a = fmaf(u.y, x.y, a);
        if (n1 > 2) a = fmaf(u.z, x.z, a);
        if (n1 > 3) a = fmaf(u.w, x.w, a);
    }
    return a;
}

// the xor butterfly over the group as a reduce-scatter (kernels_sddmm.hip): of results i*V + [0, V) lane `sub` ends with
// result i*V + sub in p[i*V]; the bits are the full butterfly's
template <int V, int T>
__device__ __forceinline__ void at_reduce_scatter(float (&p)[T], int sub)
{
#pragma unroll
    for (int i = 0; i < T / V; ++i) {
#pragma unroll
        for (int m = V / 2; m >= 1; m /= 2) {
            const bool up = (sub & m) != 0;
#pragma unroll
            for (int j = 0; j < m; ++j) {
                const float lo = p[i * V + j], hi = p[i * V + j + m];
                const float keep = up ? hi : lo, send = up ? lo : hi;
                p[i * V + j] = keep + __shfl_xor(send, m);
            }
        }
    }
}

// what lane `sub` holds for nonzero i*V + sub, in every lane of the group
template <int V, int T>
__device__ __forceinline__ void at_bcast(const float (&w)[T / V], float (&wt)[T], int gbase)
{
#pragma unroll
    for (int t = 0; t < T; ++t) wt[t] = V == 1 ? w[t] : __shfl(w[t / V], gbase + t % V);
}

template <int V>
__device__ __forceinline__ float at_group_max(float x)
{
#pragma unroll
    for (int m = V / 2; m >= 1; m /= 2) x = fmaxf(x, __shfl_xor(x, m));
    return x;
}

template <int V>
__device__ __forceinline__ float at_group_sum(float x)
{
#pragma unroll
    for (int m = V / 2; m >= 1; m /= 2) x = x + __shfl_xor(x, m);
    return x;
}

// the step's column indices: lane `sub` loads nonzeros kb + i*V + sub (0 past the end), every lane gets all T
template <int V, int T>
__device__ __forceinline__ void at_columns(int64_t kb, int64_t e, int sub, int gbase, const int32_t *__restrict__ col_idx,
                                           int32_t (&c)[T / V], int32_t (&ct)[T])
{
#pragma unroll
    for (int i = 0; i < T / V; ++i) {
        const int64_t n = kb + (int64_t)i * V + sub;
        c[i] = n < e ? col_idx[n] : 0;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) ct[t] = V == 1 ? c[t] : __shfl(c[t / V], gbase + t % V);
}

template <int V>
struct AtGeom {
    static constexpr int T = V > 8 ? V : 8;   // nonzeros per step
    static constexpr int L = T / V;           // of which a lane owns L
};

// ---- forward: (m, l, acc) of the nonzeros [b, e) of the group's row.  All lanes of a group call it with the same b, e. ----
template <int V, bool VEC>
__device__ __forceinline__ void fwd_span(int lane, int64_t b, int64_t e, const AttnArgs &a, float4 q,
                                         const int32_t *__restrict__ col_idx, int c0, float &m, float &l, float4 &acc)
{
    constexpr int T = AtGeom<V>::T, L = AtGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int nk = a.k - c0, nv = a.kv - c0;
    m = -INFINITY;
    l = 0.0f;
    acc = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        at_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        float4 xk[T], xv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) xk[t] = (nk > 0 && kb + t < e) ? at_slice<VEC>(a.K, a.ldk, ct[t], c0, a.k) : zero4();
#pragma unroll
        for (int t = 0; t < T; ++t) xv[t] = (nv > 0 && kb + t < e) ? at_slice<VEC>(a.V, a.ldv, ct[t], c0, a.kv) : zero4();
        float p[T];
#pragma unroll
        for (int t = 0; t < T; ++t) p[t] = at_partial(q, xk[t], nk);
        at_reduce_scatter<V, T>(p, sub);
        float tl[L], sm = -INFINITY;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            tl[i] = kb + i * V + sub < e ? a.scale * p[i * V] : -INFINITY;
            sm = fmaxf(sm, tl[i]);
        }
        const float mn = fmaxf(m, at_group_max<V>(sm));
        const float z = mn == -INFINITY ? 0.0f : mn;
        const float alpha = expf(m - z);
        float el[L], et[T];
#pragma unroll
        for (int i = 0; i < L; ++i) el[i] = expf(tl[i] - z);
        at_bcast<V, T>(el, et, gbase);
        l = l * alpha;
        acc.x = acc.x * alpha;
        acc.y = acc.y * alpha;
        acc.z = acc.z * alpha;
        acc.w = acc.w * alpha;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {
                l = l + et[t];
                acc.x = fmaf(et[t], xv[t].x, acc.x);
                acc.y = fmaf(et[t], xv[t].y, acc.y);
                acc.z = fmaf(et[t], xv[t].z, acc.z);
                acc.w = fmaf(et[t], xv[t].w, acc.w);
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

// the row of slot `threadIdx.x / V` of the block, or -1 (group-uniform: a group never splits here)
template <int V>
__device__ __forceinline__ int64_t at_row(const AttnRows &g)
{
    const int64_t slot = at_xcd_item(blockIdx.x, g.nblocks) * (kAtBlock / V) + threadIdx.x / V;
    if (slot >= g.rows) return -1;
    return g.order ? g.order[slot] : slot;
}

// the piece of the group and the index of its long row: long_first[lo] <= p < long_first[lo + 1]
template <int V>
__device__ __forceinline__ int64_t at_piece(const AttnPieces &g, int &lo)
{
    const int64_t p = (int64_t)blockIdx.x * (kAtBlock / V) + threadIdx.x / V;
    if (p >= g.npieces) return -1;
    int hi = g.n_long;
    lo = 0;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (g.long_first[mid] <= p) lo = mid;
        else hi = mid;
    }
    return p;
}

template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_fwd_rows(AttnRows g, AttnArgs a)
{
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = at_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    if (e == b) {
        if (c0 < a.kv) at_store<VEC>(a.out0 + r * a.ld0 + c0, zero4(), c0, a.kv);
        if (sub == 0) store_stats(a.stats, r, -INFINITY, 0.0f);
        return;
    }
    const float4 q = c0 < a.k ? at_slice<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    float m, l;
    float4 acc;
    fwd_span<V, VEC>(lane, b, e, a, q, g.col_idx, c0, m, l, acc);
    const float rinv = 1.0f / l;
    if (c0 < a.kv) at_store<VEC>(a.out0 + r * a.ld0 + c0, scaled4(acc, rinv), c0, a.kv);
    if (sub == 0) store_stats(a.stats, r, m, rinv);
}

template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_fwd_pieces(AttnPieces g, AttnArgs a)
{
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    int lo;
    const int64_t p = at_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    const float4 q = c0 < a.k ? at_slice<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    float m, l;
    float4 acc;
    fwd_span<V, VEC>(lane, b, e, a, q, g.col_idx, c0, m, l, acc);
    float *s = g.scratch + p * kAtSlots;
    if (sub == 0) *reinterpret_cast<float2 *>(s) = make_float2(m, l);
    if (c0 < a.kv) *reinterpret_cast<float4 *>(s + kAtSums + c0) = acc;
}

// a group per long row: the pieces' (m_p, l_p, acc_p) folded in piece order
template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_fwd_combine(AttnPieces g, AttnArgs a)
{
    const int sub = threadIdx.x & (V - 1), c0 = 4 * sub;
    const int64_t i = (int64_t)blockIdx.x * (kAtBlock / V) + threadIdx.x / V;
    if (i >= g.n_long) return;
    const int64_t r = g.long_row[i];
    const int f = g.long_first[i], n = g.long_first[i + 1];
    float M = -INFINITY;
    for (int p = f; p < n; ++p) M = fmaxf(M, g.scratch[(int64_t)p * kAtSlots]);
    const float z = M == -INFINITY ? 0.0f : M;
    float l = 0.0f;
    float4 acc = zero4();
    for (int p = f; p < n; ++p) {
        const float *s = g.scratch + (int64_t)p * kAtSlots;
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
    if (c0 < a.kv) at_store<VEC>(a.out0 + r * a.ld0 + c0, scaled4(acc, rinv), c0, a.kv);
    if (sub == 0) store_stats(a.stats, r, M, rinv);
}

// ---- backward_q: dQ of the nonzeros [b, e) of row i, whose q, dO slice g, (M, rinv) and delta the group holds -------------
template <int V, bool VEC>
__device__ __forceinline__ float4 bwdq_span(int lane, int64_t b, int64_t e, const AttnArgs &a, float4 q, float4 g, float M,
                                            float rinv, float delta, const int32_t *__restrict__ col_idx, int c0)
{
    constexpr int T = AtGeom<V>::T, L = AtGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int nk = a.k - c0, nv = a.kv - c0;
    float4 dq = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        at_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        float4 xk[T], xv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) xk[t] = (nk > 0 && kb + t < e) ? at_slice<VEC>(a.K, a.ldk, ct[t], c0, a.k) : zero4();
#pragma unroll
        for (int t = 0; t < T; ++t) xv[t] = (nv > 0 && kb + t < e) ? at_slice<VEC>(a.V, a.ldv, ct[t], c0, a.kv) : zero4();
        float ps[T], pd[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            ps[t] = at_partial(q, xk[t], nk);
            pd[t] = at_partial(g, xv[t], nv);
        }
        at_reduce_scatter<V, T>(ps, sub);
        at_reduce_scatter<V, T>(pd, sub);
        float dl[L], dt[T];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const float t = a.scale * ps[i * V];
            const float p = expf(t - M) * rinv;
            dl[i] = a.scale * (p * (pd[i * V] - delta));
        }
        at_bcast<V, T>(dl, dt, gbase);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {
                dq.x = fmaf(dt[t], xk[t].x, dq.x);
                dq.y = fmaf(dt[t], xk[t].y, dq.y);
                dq.z = fmaf(dt[t], xk[t].z, dq.z);
                dq.w = fmaf(dt[t], xk[t].w, dq.w);
            }
        }
    }
    return dq;
}

// delta of row r (every lane of the group gets it) and the row's dO slice
template <int V, bool VEC>
__device__ __forceinline__ float at_delta(const AttnArgs &a, int64_t r, int c0, float4 &g)
{
    float4 o = zero4();
    g = zero4();
    if (c0 < a.kv) {
        g = at_slice<VEC>(a.dO, a.lddo, r, c0, a.kv);
        o = at_slice<VEC>(a.O, a.ldo, r, c0, a.kv);
    }
    return at_group_sum<V>(at_partial(g, o, a.kv - c0));
}

template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_bwd_q_rows(AttnRows g, AttnArgs a)
{
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = at_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    if (e == b) {
        if (c0 < a.k) at_store<VEC>(a.out0 + r * a.ld0 + c0, zero4(), c0, a.k);
        if (sub == 0) a.delta[r] = 0.0f;
        return;
    }
    float4 go;
    const float delta = at_delta<V, VEC>(a, r, c0, go);
    const float4 q = c0 < a.k ? at_slice<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    const float2 st = *reinterpret_cast<const float2 *>(a.stats_in + 2 * r);
    const float4 dq = bwdq_span<V, VEC>(lane, b, e, a, q, go, st.x, st.y, delta, g.col_idx, c0);
    if (c0 < a.k) at_store<VEC>(a.out0 + r * a.ld0 + c0, dq, c0, a.k);
    if (sub == 0) a.delta[r] = delta;
}

template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_bwd_q_pieces(AttnPieces g, AttnArgs a)
{
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    int lo;
    const int64_t p = at_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    float4 go;
    const float delta = at_delta<V, VEC>(a, r, c0, go);      // (every piece of the row computes the same bits)
    const float4 q = c0 < a.k ? at_slice<VEC>(a.Q, a.ldq, r, c0, a.k) : zero4();
    const float2 st = *reinterpret_cast<const float2 *>(a.stats_in + 2 * r);
    const float4 dq = bwdq_span<V, VEC>(lane, b, e, a, q, go, st.x, st.y, delta, g.col_idx, c0);
    if (c0 < a.k) *reinterpret_cast<float4 *>(g.scratch + p * kAtSlots + kAtSums + c0) = dq;
    if (sub == 0 && p == g.long_first[lo]) a.delta[r] = delta;
}

// a group per long row: out[row][c] = the pieces' partial sums at scratch offset `off`, added in piece order from +0
template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_add_pieces(AttnPieces g, int off, float *__restrict__ out, int64_t ld, int w)
{
    const int sub = threadIdx.x & (V - 1), c0 = 4 * sub;
    const int64_t i = (int64_t)blockIdx.x * (kAtBlock / V) + threadIdx.x / V;
    if (i >= g.n_long || c0 >= w) return;
    float4 acc = zero4();
    for (int p = g.long_first[i]; p < g.long_first[i + 1]; ++p) {
        const float4 x = *reinterpret_cast<const float4 *>(g.scratch + (int64_t)p * kAtSlots + off + c0);
        acc.x = acc.x + x.x;
        acc.y = acc.y + x.y;
        acc.z = acc.z + x.z;
        acc.w = acc.w + x.w;
    }
    at_store<VEC>(out + (int64_t)g.long_row[i] * ld + c0, acc, c0, w);
}

// ---- backward_kv on the transposed pattern: (dK, dV) of the nonzeros [b, e) of row j, whose K and V slices the group holds
template <int V, bool VEC>
__device__ __forceinline__ void bwdkv_span(int lane, int64_t b, int64_t e, const AttnArgs &a, float4 kj, float4 vj,
                                           const int32_t *__restrict__ col_idx, int c0, float4 &dk, float4 &dv)
{
    constexpr int T = AtGeom<V>::T, L = AtGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int nk = a.k - c0, nv = a.kv - c0;
    dk = zero4();
    dv = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        at_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        float2 st[L];
        float de[L];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const bool in = kb + i * V + sub < e;
            st[i] = in ? *reinterpret_cast<const float2 *>(a.stats_in + 2 * (int64_t)c[i]) : make_float2(0.0f, 0.0f);
            de[i] = in ? a.delta_in[c[i]] : 0.0f;
        }
        float4 xq[T], xg[T];
#pragma unroll
        for (int t = 0; t < T; ++t) xq[t] = (nk > 0 && kb + t < e) ? at_slice<VEC>(a.Q, a.ldq, ct[t], c0, a.k) : zero4();
#pragma unroll
        for (int t = 0; t < T; ++t) xg[t] = (nv > 0 && kb + t < e) ? at_slice<VEC>(a.dO, a.lddo, ct[t], c0, a.kv) : zero4();
        float ps[T], pd[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            ps[t] = at_partial(kj, xq[t], nk);
            pd[t] = at_partial(vj, xg[t], nv);
        }
        at_reduce_scatter<V, T>(ps, sub);
        at_reduce_scatter<V, T>(pd, sub);
        float pl[L], dl[L], pt[T], dt[T];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const float t = a.scale * ps[i * V];
            pl[i] = expf(t - st[i].x) * st[i].y;
            dl[i] = a.scale * (pl[i] * (pd[i * V] - de[i]));
        }
        at_bcast<V, T>(pl, pt, gbase);
        at_bcast<V, T>(dl, dt, gbase);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {
                dv.x = fmaf(pt[t], xg[t].x, dv.x);
                dv.y = fmaf(pt[t], xg[t].y, dv.y);
                dv.z = fmaf(pt[t], xg[t].z, dv.z);
                dv.w = fmaf(pt[t], xg[t].w, dv.w);
                dk.x = fmaf(dt[t], xq[t].x, dk.x);
                dk.y = fmaf(dt[t], xq[t].y, dk.y);
                dk.z = fmaf(dt[t], xq[t].z, dk.z);
                dk.w = fmaf(dt[t], xq[t].w, dk.w);
            }
        }
    }
}

template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_bwd_kv_rows(AttnRows g, AttnArgs a)
{
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    const int64_t r = at_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    float4 dk = zero4(), dv = zero4();
    if (e > b) {
        const float4 kj = c0 < a.k ? at_slice<VEC>(a.K, a.ldk, r, c0, a.k) : zero4();
        const float4 vj = c0 < a.kv ? at_slice<VEC>(a.V, a.ldv, r, c0, a.kv) : zero4();
        bwdkv_span<V, VEC>(lane, b, e, a, kj, vj, g.col_idx, c0, dk, dv);
    }
    if (c0 < a.k) at_store<VEC>(a.out0 + r * a.ld0 + c0, dk, c0, a.k);
    if (c0 < a.kv) at_store<VEC>(a.out1 + r * a.ld1 + c0, dv, c0, a.kv);
}

template <int V, bool VEC>
__global__ __launch_bounds__(kAtBlock) void k_attn_bwd_kv_pieces(AttnPieces g, AttnArgs a)
{
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (V - 1), c0 = 4 * sub;
    int lo;
    const int64_t p = at_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    const float4 kj = c0 < a.k ? at_slice<VEC>(a.K, a.ldk, r, c0, a.k) : zero4();
    const float4 vj = c0 < a.kv ? at_slice<VEC>(a.V, a.ldv, r, c0, a.kv) : zero4();
    float4 dk, dv;
    bwdkv_span<V, VEC>(lane, b, e, a, kj, vj, g.col_idx, c0, dk, dv);
    float *s = g.scratch + p * kAtSlots;
    if (c0 < a.k) *reinterpret_cast<float4 *>(s + kAtSums + c0) = dk;
    if (c0 < a.kv) *reinterpret_cast<float4 *>(s + kAtSums2 + c0) = dv;
}

#define AT_LAUNCHED(name)                                                                                     \
    if (hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return hip_fail(e_, name, __FILE__, __LINE__)

enum { kPassForward = 0, kPassBackwardQ = 1, kPassBackwardKV = 2 };

template <int PASS, int V, bool VEC>
int launch_attn_v(const spmv_csr &h, const AttnArgs &a, const char *what, hipStream_t s)
{
    const SpmmPlan &p = h.plan_spmm;
    constexpr int kPerBlock = kAtBlock / V;
    const int64_t nblocks = (h.rows + kPerBlock - 1) / kPerBlock;
    // (a launch carries fewer than 2^32 work-items, as in launch_spmm_v: rows x lanes per row < 2^32)
    if (nblocks * kAtBlock >= (1LL << 32)) {
        set_error("%s: %lld rows x %d lanes per row reach the launch limit of 2^32 work-items", what, (long long)h.rows, V);
        return SPMV_ERR_INVALID;
    }
    const AttnRows g{h.rows, nblocks, p.row_cap, V == 1 ? nullptr : p.d_order.get(), h.d_row_ptr, h.d_col_idx};
    const dim3 grid((unsigned)nblocks), block(kAtBlock);
    if constexpr (PASS == kPassForward) hipLaunchKernelGGL((k_attn_fwd_rows<V, VEC>), grid, block, 0, s, g, a);
    else if constexpr (PASS == kPassBackwardQ) hipLaunchKernelGGL((k_attn_bwd_q_rows<V, VEC>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((k_attn_bwd_kv_rows<V, VEC>), grid, block, 0, s, g, a);
    AT_LAUNCHED("k_attn_*_rows");
    if (!p.n_long) return SPMV_OK;
    const AttnPieces q{p.pieces, p.n_long, p.d_long_row.get(), p.d_long_first.get(), p.d_piece_k0.get(), p.d_piece_len.get(),
                       h.d_col_idx, h.plan_attn.d_scratch.get()};
    const dim3 pgrid((unsigned)((p.pieces + kPerBlock - 1) / kPerBlock)), lgrid((unsigned)((p.n_long + kPerBlock - 1) / kPerBlock));
    if constexpr (PASS == kPassForward) {
        hipLaunchKernelGGL((k_attn_fwd_pieces<V, VEC>), pgrid, block, 0, s, q, a);
        AT_LAUNCHED("k_attn_fwd_pieces");
        hipLaunchKernelGGL((k_attn_fwd_combine<V, VEC>), lgrid, block, 0, s, q, a);
        AT_LAUNCHED("k_attn_fwd_combine");
    } else if constexpr (PASS == kPassBackwardQ) {
        hipLaunchKernelGGL((k_attn_bwd_q_pieces<V, VEC>), pgrid, block, 0, s, q, a);
        AT_LAUNCHED("k_attn_bwd_q_pieces");
        hipLaunchKernelGGL((k_attn_add_pieces<V, VEC>), lgrid, block, 0, s, q, kAtSums, a.out0, a.ld0, a.k);
        AT_LAUNCHED("k_attn_add_pieces");
    } else {
        hipLaunchKernelGGL((k_attn_bwd_kv_pieces<V, VEC>), pgrid, block, 0, s, q, a);
        AT_LAUNCHED("k_attn_bwd_kv_pieces");
        hipLaunchKernelGGL((k_attn_add_pieces<V, VEC>), lgrid, block, 0, s, q, kAtSums, a.out0, a.ld0, a.k);
        AT_LAUNCHED("k_attn_add_pieces");
        hipLaunchKernelGGL((k_attn_add_pieces<V, VEC>), lgrid, block, 0, s, q, kAtSums2, a.out1, a.ld1, a.kv);
        AT_LAUNCHED("k_attn_add_pieces");
    }
    return SPMV_OK;
}

template <int PASS, bool VEC>
int launch_attn_vec(const spmv_csr &h, const AttnArgs &a, const char *what, hipStream_t s)
{
    const int slices = ((a.k > a.kv ? a.k : a.kv) + 3) / 4;
    if (slices <= 1) return launch_attn_v<PASS, 1, VEC>(h, a, what, s);
    if (slices <= 2) return launch_attn_v<PASS, 2, VEC>(h, a, what, s);
    if (slices <= 4) return launch_attn_v<PASS, 4, VEC>(h, a, what, s);
    if (slices <= 8) return launch_attn_v<PASS, 8, VEC>(h, a, what, s);
    return launch_attn_v<PASS, 16, VEC>(h, a, what, s);
}

template <int PASS>
int launch_attn(const spmv_csr &h, const AttnArgs &a, bool vec, const char *what, hipStream_t s)
{
    if (h.rows == 0) return SPMV_OK;
    return vec ? launch_attn_vec<PASS, true>(h, a, what, s) : launch_attn_vec<PASS, false>(h, a, what, s);
}

bool vec4(std::initializer_list<int64_t> lds)
{
    for (int64_t ld : lds)
        if (ld % 4 != 0) return false;
    return true;
}

}  // namespace

// The attention plan: the SpMM plan (made here if it is missing) and the scratch of the long rows' pieces.
int plan_attention(spmv_csr &h, hipStream_t s)
{
    if (int rc = plan_spmm(h, s)) return rc;
    if (h.plan_attn.ready) return SPMV_OK;
    AttnPlan p;
    if (h.plan_spmm.n_long) SPMV_HIP_TRY(p.d_scratch.alloc((size_t)h.plan_spmm.pieces * kAtSlots));
    p.ready = true;
    h.plan_attn = std::move(p);
    return SPMV_OK;
}

int64_t attention_plan_bytes(const spmv_csr &h)
{
    if (!h.plan_attn.ready) return 0;
    return spmm_plan_bytes(h) + (h.plan_spmm.n_long ? (int64_t)h.plan_spmm.pieces * kAtSlots * 4 : 0);
}

// arguments checked by the callers in capi.hip
int launch_attention_forward(const spmv_csr &h, float scale, int k, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                             int kv, const float *V, int64_t ldv, float *O, int64_t ldo, float *stats, hipStream_t s)
{
    AttnArgs a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = Q, a.ldq = ldq, a.K = K, a.ldk = ldk, a.V = V, a.ldv = ldv;
    a.out0 = O, a.ld0 = ldo, a.stats = stats;
    return launch_attn<kPassForward>(h, a, vec4({ldq, ldk, ldv, ldo}), "spmv_csr_attention_forward", s);
}

int launch_attention_backward_q(const spmv_csr &h, float scale, int k, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                                int kv, const float *V, int64_t ldv, const float *O, int64_t ldo, const float *dO,
                                int64_t lddo, const float *stats, float *delta, float *dQ, int64_t lddq, hipStream_t s)
{
    AttnArgs a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = Q, a.ldq = ldq, a.K = K, a.ldk = ldk, a.V = V, a.ldv = ldv, a.O = O, a.ldo = ldo, a.dO = dO, a.lddo = lddo;
    a.stats_in = stats, a.delta = delta, a.out0 = dQ, a.ld0 = lddq;
    return launch_attn<kPassBackwardQ>(h, a, vec4({ldq, ldk, ldv, ldo, lddo, lddq}), "spmv_csr_attention_backward_q", s);
}

int launch_attention_backward_kv(const spmv_csr &t, float scale, int k, const float *Q, int64_t ldq, const float *K,
                                 int64_t ldk, int kv, const float *V, int64_t ldv, const float *dO, int64_t lddo,
                                 const float *stats, const float *delta, float *dK, int64_t lddk, float *dV, int64_t lddv,
                                 hipStream_t s)
{
    AttnArgs a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = Q, a.ldq = ldq, a.K = K, a.ldk = ldk, a.V = V, a.ldv = ldv, a.dO = dO, a.lddo = lddo;
    a.stats_in = stats, a.delta_in = delta, a.out0 = dK, a.ld0 = lddk, a.out1 = dV, a.ld1 = lddv;
    return launch_attn<kPassBackwardKV>(t, a, vec4({ldq, ldk, ldv, lddo, lddk, lddv}), "spmv_csr_attention_backward_kv", s);
}

}  // namespace spmv
