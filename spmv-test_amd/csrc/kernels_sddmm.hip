// kernels_sddmm.hip -- out[n] = U[row(n), :k] . X[col(n), :k] for every stored nonzero n of a CSR handle, k <= 64
// (spmv_csr_sddmm, include/spmv_hip.h "SDDMM"): the dense-dense product U X^T sampled at the handle's pattern.  Any k in
// column tiles of 64: spmv_csr_sddmm_cols (sddmm_span_cols below; the COLS instantiations of the two kernels, which differ
// from the narrow ones in that one call).  launch_sddmm<E> is the one way in for the three entry points of an element type.
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
// (COLS: the kernel of spmv_csr_sddmm_cols, V = kColsV and a.k any width)
template <int V, bool VEC, typename E, bool COLS = false>
__global__ __launch_bounds__(kBlock) void k_sddmm_rows(GroupRows g, SddmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1), c0 = 4 * (lane & (V - 1));
    const int64_t r = group_row<V>(g);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e == b || e - b > g.row_cap) return;   // (the U row of an empty row is not even loaded)
    if constexpr (COLS) {
        sddmm_span_cols<VEC, E>(lane, r, b, e, g.col_idx, a.U, a.ldu, a.X, a.ldx, a.out, a.k);
    } else {
        const float4 u = c0 < a.k ? load_wide<VEC>(a.U, a.ldu, r, c0, a.k) : zero4();
        sddmm_span<V, VEC, E>(lane, b, e, u, g.col_idx, a.X, a.ldx, a.out, c0, a.k);
    }
}

// a group of V lanes per piece of a long row (COLS: as above)
template <int V, bool VEC, typename E, bool COLS = false>
__global__ __launch_bounds__(kBlock) void k_sddmm_pieces(GroupPieces g, SddmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1), c0 = 4 * (lane & (V - 1));
    int lo;
    const int64_t p = group_piece<V>(g, lo);
    if (p < 0) return;
    // (the three loads in this order: with long_row first the COLS instantiations schedule differently)
    const int64_t b = g.piece_k0[p], r = g.long_row[lo], e = b + g.piece_len[p];
    if constexpr (COLS) {
        sddmm_span_cols<VEC, E>(lane, r, b, e, g.col_idx, a.U, a.ldu, a.X, a.ldx, a.out, a.k);
    } else {
        const float4 u = c0 < a.k ? load_wide<VEC>(a.U, a.ldu, r, c0, a.k) : zero4();
        sddmm_span<V, VEC, E>(lane, b, e, u, g.col_idx, a.X, a.ldx, a.out, c0, a.k);
    }
}

// the two launches of a call; who: the entry point, for a refusal
template <int V, bool VEC, typename E, bool COLS>
int launch_sddmm_v(const spmv_csr &h, const char *who, const SddmmArgs<E> &a, hipStream_t s)
{
    const int64_t nblocks = group_row_blocks(who, h, V);
    if (nblocks < 0) return SPMV_ERR_INVALID;
    hipLaunchKernelGGL((k_sddmm_rows<V, VEC, E, COLS>), dim3((unsigned)nblocks), dim3(kBlock), 0, s, group_rows(h, V, nblocks), a);
    SPMV_LAUNCHED("k_sddmm_rows");
    if (!h.plan_spmm.n_long) return SPMV_OK;
    hipLaunchKernelGGL((k_sddmm_pieces<V, VEC, E, COLS>), group_grid(h.plan_spmm.pieces, V), dim3(kBlock), 0, s,
                       group_pieces(h, nullptr), a);
    SPMV_LAUNCHED("k_sddmm_pieces");
    return SPMV_OK;
}

}  // namespace

// Arguments checked by capi.hip (product_args): ld >= k, U / X aligned for E, and 1 <= k <= 64 with the SpMM plan made or, with
// `cols`, 1 <= k <= SPMV_COLS_MAX_K with the _cols plan covering k.  V = pow2 >= ceil(k / 4), or kColsV whatever k is.
template <typename E>
int launch_sddmm(const spmv_csr &h, const char *who, bool cols, int k, const E *U, int64_t ldu, const E *X, int64_t ldx, float *out,
                 hipStream_t s)
{
    if (h.rows == 0 || h.nnz == 0) return SPMV_OK;
    const SddmmArgs<E> a{U, ldu, X, ldx, out, k};
    const bool vec = ldu % 4 == 0 && ldx % 4 == 0;
    if (cols) return vec ? launch_sddmm_v<kColsV, true, E, true>(h, who, a, s) : launch_sddmm_v<kColsV, false, E, true>(h, who, a, s);
    return dispatch_lanes((k + 3) / 4, [&](auto v) {
        constexpr int V = decltype(v)::value;
        return vec ? launch_sddmm_v<V, true, E, false>(h, who, a, s) : launch_sddmm_v<V, false, E, false>(h, who, a, s);
    });
}

template int launch_sddmm(const spmv_csr &, const char *, bool, int, const float *, int64_t, const float *, int64_t, float *, hipStream_t);
template int launch_sddmm(const spmv_csr &, const char *, bool, int, const bf16 *, int64_t, const bf16 *, int64_t, float *, hipStream_t);
template int launch_sddmm(const spmv_csr &, const char *, bool, int, const fp16 *, int64_t, const fp16 *, int64_t, float *, hipStream_t);

}  // namespace spmv
