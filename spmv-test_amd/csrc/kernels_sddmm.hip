// kernels_sddmm.hip -- out[n] = U[row(n), :k] . X[col(n), :k] for every stored nonzero n of a CSR handle, k <= 64
// (spmv_csr_sddmm, include/spmv_hip.h "SDDMM"): the dense-dense product U X^T sampled at the handle's pattern.  Any k in
// column tiles of 64: spmv_csr_sddmm_cols (sddmm_span_cols below).
//
// The lane groups, their steps and the plan are lane_group.hpp's.  U is rows rows of ldu floats (row-major), X cols rows
// of ldx floats.  Lane s of a row's group loads columns [4s, 4s+4) of the row's U row once and keeps them in registers;
// per step the group issues all T slice gathers of X, forms T lane partials, reduces each across the group and stores
// the step's T results coalesced (lane `sub` stores positions kb + i*V + sub).  vals is never read.  Results are
// independent of one another: the pieces of a long row write straight into out, there is no partial buffer and no
// combine launch.
//
// The order of the fp32 operations of out[n] is fixed by k alone: the dot product of lane_group.hpp (dot_partial, then
// the xor butterfly as reduce_scatter).  Nothing depends on ldu, ldx, the load path, the nonzero's position in its row,
// the row's length, the pieces or other rows; and fma(u, x, p) == fma(x, u, p), so the operands may trade places
// (T.sddmm(X, U) on the transposed pattern).
//
// Element types.  Every kernel here takes the element type E of U and X as its last template argument: float
// (spmv_csr_sddmm) or 16-bit storage (bf16, fp16: spmv_csr_sddmm_16).  With 16-bit E the row's U slice is widened once
// (load_wide) and stays in registers as floats, a step's gathered X slices wait packed as loaded (slice_t<E>) and are
// widened exactly where dot_partial multiplies them, and every operation above is the same fp32 operation: out, which is
// float always, holds the bits of the fp32 call on the widened operands.
#include "lane_group.hpp"

namespace spmv {

namespace {

// the results of the nonzeros [b, e) of the group's row (or piece), whose U slice is u.  All lanes of a group call it
// with the same b, e; lanes with c0 >= k load nothing and contribute +0 (their shuffles still run).
template <int V, bool VEC, typename E>
__device__ __forceinline__ void sddmm_span(int lane, int64_t b, int64_t e, float4 u, const int32_t *__restrict__ col_idx,
                                           const E *__restrict__ X, int64_t ldx, float *__restrict__ out, int c0, int k)
{
    constexpr int T = LaneGeom<V>::T, L = LaneGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const int n1 = k - c0;               // the lane's columns below k: min(n1, 4)
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        group_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        slice_t<E> xt[T];
        float p[T];
#pragma unroll
        for (int t = 0; t < T; ++t) xt[t] = (n1 > 0 && kb + t < e) ? load_slice<VEC>(X, ldx, ct[t], c0, k) : zero_slice<E>();
#pragma unroll
        for (int t = 0; t < T; ++t) p[t] = dot_partial(u, widen_again<E>(xt[t]), n1);    // (no slice widened before its turn)
        reduce_scatter<V, T>(p, sub);
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int64_t n = kb + (int64_t)i * V + sub;
            if (n < e) out[n] = p[i * V];
        }
    }
}

// The same at any k (spmv_csr_sddmm_cols), a group of kColsV = 16 lanes whatever k is.  The group walks a step's T = 16
// nonzeros once and loops over the column tiles inside the step: per tile t the lane's U slice of that tile (reloaded per
// step: 16 bytes from a row the group keeps reading, against the step's 16 gathers of X), the T gathers of X, dot_partial
// at the tile's width k_t and the butterfly -- the very number r_t the narrow call gives for U[:, tile t], X[:, tile t] at
// k_t -- and then acc = r_0, acc = acc + r_t in tile order: one fp32 addition per further tile, never a partial carried
// from one tile's lanes into the next butterfly.  One coalesced store per step, as above.
template <bool VEC, typename E>
__device__ __forceinline__ void sddmm_span_cols(int lane, int64_t r, int64_t b, int64_t e, const int32_t *__restrict__ col_idx,
                                                const E *__restrict__ U, int64_t ldu, const E *__restrict__ X, int64_t ldx,
                                                float *__restrict__ out, int k)
{
    constexpr int V = kColsV, T = LaneGeom<V>::T, L = LaneGeom<V>::L;
    static_assert(L == 1, "one result per lane and step");
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1), c0 = 4 * sub;
    const int m = cols_tiles(k);
    const E *__restrict__ urow = U + r * ldu;
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L], ct[T];
        group_columns<V, T>(kb, e, sub, gbase, col_idx, c, ct);
        float acc = 0.0f;
        for (int tile = 0; tile < m; ++tile) {
            const int kt = min(kColsTile, k - kColsTile * tile), n1 = kt - c0;
            const E *__restrict__ Xt = X + (int64_t)kColsTile * tile;
            const float4 u = n1 > 0 ? load_wide<VEC>(urow + (int64_t)kColsTile * tile, 0, 0, c0, kt) : zero4();
            slice_t<E> xt[T];
            float p[T];
#pragma unroll
            for (int t = 0; t < T; ++t) xt[t] = (n1 > 0 && kb + t < e) ? load_slice<VEC>(Xt, ldx, ct[t], c0, kt) : zero_slice<E>();
#pragma unroll
            for (int t = 0; t < T; ++t) p[t] = dot_partial(u, widen_again<E>(xt[t]), n1);
            reduce_scatter<V, T>(p, sub);
            acc = tile == 0 ? p[0] : acc + p[0];      // (from r_0's value, not from +0: a -0 stays -0)
        }
        const int64_t n = kb + sub;
        if (n < e) out[n] = acc;
    }
}

// the operands of a launch (by value); E: the element type of U and X, whose ld count elements of E
template <typename E>
struct SddmmArgs {
    const E *U;
    int64_t ldu;
    const E *X;
    int64_t ldx;
    float *out;
    int k;
};

// a group of V lanes per row; rows of more than row_cap nonzeros are left to the pieces
template <int V, bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_sddmm_rows(GroupRows g, SddmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1), c0 = 4 * (lane & (V - 1));
    const int64_t r = group_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e == b || e - b > g.row_cap) return;   // (the U row of an empty row is not even loaded)
    const float4 u = c0 < a.k ? load_wide<VEC>(a.U, a.ldu, r, c0, a.k) : zero4();
    sddmm_span<V, VEC, E>(lane, b, e, u, g.col_idx, a.X, a.ldx, a.out, c0, a.k);
}

// a group of V lanes per piece of a long row
template <int V, bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_sddmm_pieces(GroupPieces g, SddmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1), c0 = 4 * (lane & (V - 1));
    int lo;
    const int64_t p = group_piece<V>(g, lo);
    if (p < 0) return;
    const int64_t r = g.long_row[lo];
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    const float4 u = c0 < a.k ? load_wide<VEC>(a.U, a.ldu, r, c0, a.k) : zero4();
    sddmm_span<V, VEC, E>(lane, b, e, u, g.col_idx, a.X, a.ldx, a.out, c0, a.k);
}

// the two kernels of spmv_csr_sddmm_cols: a group of kColsV lanes per row, and per piece of a long row (a.k: any width)
template <bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_sddmm_cols_rows(GroupRows g, SddmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = group_row<kColsV>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e == b || e - b > g.row_cap) return;
    sddmm_span_cols<VEC, E>(lane, r, b, e, g.col_idx, a.U, a.ldu, a.X, a.ldx, a.out, a.k);
}

template <bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void k_sddmm_cols_pieces(GroupPieces g, SddmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1);
    int lo;
    const int64_t p = group_piece<kColsV>(g, lo);
    if (p < 0) return;
    const int64_t b = g.piece_k0[p];
    sddmm_span_cols<VEC, E>(lane, g.long_row[lo], b, b + g.piece_len[p], g.col_idx, a.U, a.ldu, a.X, a.ldx, a.out, a.k);
}

template <bool VEC, typename E>
int launch_sddmm_cols_v(const spmv_csr &h, const SddmmArgs<E> &a, hipStream_t s)
{
    constexpr int V = kColsV;
    const int64_t nblocks = group_row_blocks("spmv_csr_sddmm_cols", h, V);
    if (nblocks < 0) return SPMV_ERR_INVALID;
    hipLaunchKernelGGL((k_sddmm_cols_rows<VEC, E>), dim3((unsigned)nblocks), dim3(kBlock), 0, s, group_rows(h, V, nblocks), a);
    SPMV_LAUNCHED("k_sddmm_cols_rows");
    if (!h.plan_spmm.n_long) return SPMV_OK;
    hipLaunchKernelGGL((k_sddmm_cols_pieces<VEC, E>), group_grid(h.plan_spmm.pieces, V), dim3(kBlock), 0, s, group_pieces(h, nullptr), a);
    SPMV_LAUNCHED("k_sddmm_cols_pieces");
    return SPMV_OK;
}

template <typename E>
int launch_sddmm_cols_e(const spmv_csr &h, int k, const E *U, int64_t ldu, const E *X, int64_t ldx, float *out, hipStream_t s)
{
    if (h.rows == 0 || h.nnz == 0) return SPMV_OK;
    const SddmmArgs<E> a{U, ldu, X, ldx, out, k};
    return ldu % 4 == 0 && ldx % 4 == 0 ? launch_sddmm_cols_v<true, E>(h, a, s) : launch_sddmm_cols_v<false, E>(h, a, s);
}

template <int V, bool VEC, typename E>
int launch_sddmm_v(const spmv_csr &h, const SddmmArgs<E> &a, hipStream_t s)
{
    const int64_t nblocks = group_row_blocks(kIs16<E> ? "spmv_csr_sddmm_16" : "spmv_csr_sddmm", h, V);
    if (nblocks < 0) return SPMV_ERR_INVALID;
    hipLaunchKernelGGL((k_sddmm_rows<V, VEC, E>), dim3((unsigned)nblocks), dim3(kBlock), 0, s, group_rows(h, V, nblocks), a);
    SPMV_LAUNCHED("k_sddmm_rows");
    if (!h.plan_spmm.n_long) return SPMV_OK;
    hipLaunchKernelGGL((k_sddmm_pieces<V, VEC, E>), group_grid(h.plan_spmm.pieces, V), dim3(kBlock), 0, s,
                       group_pieces(h, nullptr), a);
    SPMV_LAUNCHED("k_sddmm_pieces");
    return SPMV_OK;
}

template <typename E>
int launch_sddmm_e(const spmv_csr &h, int k, const E *U, int64_t ldu, const E *X, int64_t ldx, float *out, hipStream_t s)
{
    if (h.rows == 0 || h.nnz == 0) return SPMV_OK;
    const SddmmArgs<E> a{U, ldu, X, ldx, out, k};
    const bool vec = ldu % 4 == 0 && ldx % 4 == 0;
    return dispatch_lanes((k + 3) / 4, [&](auto v) {
        constexpr int V = decltype(v)::value;
        return vec ? launch_sddmm_v<V, true, E>(h, a, s) : launch_sddmm_v<V, false, E>(h, a, s);
    });
}

}  // namespace

// arguments checked by spmv_csr_sddmm: 1 <= k <= 64, ld >= k, U / X 16-byte aligned, the SpMM plan made
int launch_sddmm(const spmv_csr &h, int k, const float *U, int64_t ldu, const float *X, int64_t ldx, float *out, hipStream_t s)
{
    return launch_sddmm_e<float>(h, k, U, ldu, X, ldx, out, s);
}

// and by spmv_csr_sddmm_16: the same with U / X 8-byte aligned and every ld in 16-bit elements
int launch_sddmm(const spmv_csr &h, int k, const bf16 *U, int64_t ldu, const bf16 *X, int64_t ldx, float *out, hipStream_t s)
{
    return launch_sddmm_e<bf16>(h, k, U, ldu, X, ldx, out, s);
}

int launch_sddmm(const spmv_csr &h, int k, const fp16 *U, int64_t ldu, const fp16 *X, int64_t ldx, float *out, hipStream_t s)
{
    return launch_sddmm_e<fp16>(h, k, U, ldu, X, ldx, out, s);
}

// arguments checked by spmv_csr_sddmm_cols: 1 <= k <= SPMV_COLS_MAX_K, ld >= k, U / X aligned for E, the _cols plan covers k
int launch_sddmm_cols(const spmv_csr &h, int k, const float *U, int64_t ldu, const float *X, int64_t ldx, float *out, hipStream_t s)
{
    return launch_sddmm_cols_e<float>(h, k, U, ldu, X, ldx, out, s);
}

int launch_sddmm_cols(const spmv_csr &h, int k, const bf16 *U, int64_t ldu, const bf16 *X, int64_t ldx, float *out, hipStream_t s)
{
    return launch_sddmm_cols_e<bf16>(h, k, U, ldu, X, ldx, out, s);
}

int launch_sddmm_cols(const spmv_csr &h, int k, const fp16 *U, int64_t ldu, const fp16 *X, int64_t ldx, float *out, hipStream_t s)
{
    return launch_sddmm_cols_e<fp16>(h, k, U, ldu, X, ldx, out, s);
}

}  // namespace spmv
