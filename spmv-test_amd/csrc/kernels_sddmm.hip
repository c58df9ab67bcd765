// kernels_sddmm.hip -- out[n] = U[row(n), :k] . X[col(n), :k] for every stored nonzero n of a CSR handle, k <= 64
// (spmv_csr_sddmm, include/spmv_hip.h "SDDMM"): the dense-dense product U X^T sampled at the handle's pattern.
//
// The geometry is kernels_spmm.hip's, and so is the plan (SpmmPlan: the order of the rows, the pieces of the long rows).
// U is rows rows of ldu floats (row-major), X cols rows of ldx floats.  A group of V = pow2 >= ceil(k/4) lanes owns one
// row of the pattern (or one plan piece of a row of more than 512 nonzeros): lane s of the group loads columns [4s, 4s+4)
// of the row's U row once and keeps them in registers, and reads the same columns of every X row the CSR row refers to
// (one 16-byte slice per nonzero where ldu % 4 == 0 and ldx % 4 == 0).  A group walks its row in steps of T = max(V, 8)
// nonzeros: it loads the step's col_idx coalesced, broadcasts them inside the group with shuffles, issues all T slice
// gathers, forms T lane partials, reduces each across the group and stores the step's T results coalesced (lane `sub`
// stores positions kb + i*V + sub).  vals is never read.  Results are independent of one another: the pieces of a long
// row write straight into out, there is no partial buffer and no combine launch.
//
// The order of the fp32 operations of out[n] is fixed by k alone:
//   1. lane s: p_s = +0, then p_s = fma(U[i][c], X[j][c], p_s) for c = 4s, 4s+1, 4s+2, 4s+3 while c < k (a column >= k
//      is skipped, not multiplied by zero; a lane whose slice starts at or past k keeps p_s = +0);
//   2. the V partials are added in the xor-butterfly m = V/2, V/4, ..., 1: p_s <- p_s + p_(s xor m).
// Step 2 runs as a reduce-scatter (after the exchange at distance m a lane keeps only the half of the step's results
// whose index has the lane's bit m: V - 1 shuffles per V results instead of V log2 V); each result goes through the
// very additions of the full butterfly, and fp32 addition is commutative, so the bits are the butterfly's.  Nothing
// depends on ldu, ldx, the load path, the nonzero's position in its row, the row's length, the pieces or other rows;
// and fma(u, x, p) == fma(x, u, p), so the operands may trade places (T.sddmm(X, U) on the transposed pattern).
//
// Addresses are 64-bit (U and X may exceed 4 GiB, 4 n passes 2^32 in col_idx and out from nnz = 2^30 on); no buffer
// descriptor and no range check is relied on.  With ld % 4 != 0 the kernels read 4-byte elements, columns below k only.
#include "spmv_internal.hpp"

namespace spmv {

namespace {

constexpr int kSddmmBlock = 256;    // 4 wavefronts

// block b of the grid takes item sddmm_xcd_item(b, n): blocks are dealt round-robin over the 8 XCDs, so each XCD gets
// one contiguous range of row blocks (as spmm_xcd_item: neighbouring rows share lines of X in that XCD's L2)
__device__ __forceinline__ int64_t sddmm_xcd_item(int64_t bid, int64_t n)
{
    const int64_t q = n / kXcds, rem = n % kXcds;
    const int64_t j = bid % kXcds, idx = bid / kXcds;
    return j * q + (j < rem ? j : rem) + idx;
}

// the four columns [c0, c0+4) of row j of a row-major matrix (c0 < k); VEC: one 16-byte load (ld % 4 == 0), else the
// columns below k only
template <bool VEC>
__device__ __forceinline__ float4 sddmm_slice(const float *__restrict__ M, int64_t ld, int64_t j, int c0, int k)
{
    const float *p = M + j * ld + c0;
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.x = p[0];
    if (c0 + 1 < k) r.y = p[1];
    if (c0 + 2 < k) r.z = p[2];
    if (c0 + 3 < k) r.w = p[3];
    return r;
}

// the results of the nonzeros [b, e) of the group's row (or piece), whose U slice is u.  All lanes of a group call it
// with the same b, e; lanes with c0 >= k load nothing and contribute +0 (their shuffles still run).
template <int V, bool VEC>
__device__ __forceinline__ void sddmm_span(int lane, int64_t b, int64_t e, float4 u, const int32_t *__restrict__ col_idx,
                                           const float *__restrict__ X, int64_t ldx, float *__restrict__ out, int c0, int k)
{
    constexpr int T = V > 8 ? V : 8;     // nonzeros per step: T slice gathers in flight per lane
    constexpr int L = T / V;             // of which each lane of the group loads L column indices and stores L results
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const bool active = c0 < k;
    const int n1 = k - c0;               // the lane's columns below k: min(n1, 4)
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int64_t n = kb + (int64_t)i * V + sub;
            c[i] = n < e ? col_idx[n] : 0;
        }
        int32_t ct[T];
        float4 xt[T];
        float p[T];
#pragma unroll
        for (int t = 0; t < T; ++t) ct[t] = V == 1 ? c[t] : __shfl(c[t / V], gbase + t % V);
#pragma unroll
        for (int t = 0; t < T; ++t)
            xt[t] = (active && kb + t < e) ? sddmm_slice<VEC>(X, ldx, ct[t], c0, k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            float a = 0.0f;
            if (active) {
                a = fmaf(u.x, xt[t].x, a);
                if (n1 > 1) a = fmaf(u.y, xt[t].y, a);
                if (n1 > 2) a = fmaf(u.z, xt[t].z, a);
                if (n1 > 3) a = fmaf(u.w, xt[t].w, a);
            }
            p[t] = a;
        }
        // the xor-butterfly over the group as a reduce-scatter: of results i*V + [0, V) lane `sub` ends with i*V + sub
#pragma unroll
        for (int i = 0; i < L; ++i) {
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
            const int64_t n = kb + (int64_t)i * V + sub;
            if (n < e) out[n] = p[i * V];
        }
    }
}

// a group of V lanes per row, the rows taken in `order` (null: in row order); rows of more than `row_cap` nonzeros are
// left to the pieces
template <int V, bool VEC>
__global__ __launch_bounds__(kSddmmBlock) void k_sddmm_rows(int64_t rows, int64_t nblocks, int row_cap,
                                                            const int32_t *__restrict__ order,
                                                            const int32_t *__restrict__ row_ptr,
                                                            const int32_t *__restrict__ col_idx, const float *__restrict__ U,
                                                            int64_t ldu, const float *__restrict__ X, int64_t ldx,
                                                            float *__restrict__ out, int k)
{
    constexpr int kRowsPerBlock = kSddmmBlock / V;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t blk = sddmm_xcd_item(blockIdx.x, nblocks);
    const int64_t slot = blk * kRowsPerBlock + threadIdx.x / V;
    if (slot >= rows) return;   // (group-uniform: a group never splits here)
    const int64_t r = order ? order[slot] : slot;
    const int64_t b = row_ptr[r], e = row_ptr[r + 1];
    if (e == b || e - b > row_cap) return;   // (the U row of an empty row is not even loaded)
    const int c0 = 4 * (lane & (V - 1));
    const float4 u = c0 < k ? sddmm_slice<VEC>(U, ldu, r, c0, k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    sddmm_span<V, VEC>(lane, b, e, u, col_idx, X, ldx, out, c0, k);
}

// a group of V lanes per piece of a long row; the piece's row is the last long row whose first piece is <= p
template <int V, bool VEC>
__global__ __launch_bounds__(kSddmmBlock) void k_sddmm_pieces(int npieces, int n_long, const int32_t *__restrict__ long_row,
                                                              const int32_t *__restrict__ long_first,
                                                              const int32_t *__restrict__ piece_k0,
                                                              const int32_t *__restrict__ piece_len,
                                                              const int32_t *__restrict__ col_idx, const float *__restrict__ U,
                                                              int64_t ldu, const float *__restrict__ X, int64_t ldx,
                                                              float *__restrict__ out, int k)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t p = (int64_t)blockIdx.x * (kSddmmBlock / V) + threadIdx.x / V;
    if (p >= npieces) return;
    int lo = 0, hi = n_long;      // long_first[lo] <= p < long_first[hi]  (long_first[0] = 0, long_first[n_long] = npieces)
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (long_first[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int64_t r = long_row[lo];
    const int64_t b = piece_k0[p], e = b + piece_len[p];
    const int c0 = 4 * (lane & (V - 1));
    const float4 u = c0 < k ? sddmm_slice<VEC>(U, ldu, r, c0, k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    sddmm_span<V, VEC>(lane, b, e, u, col_idx, X, ldx, out, c0, k);
}

template <int V, bool VEC>
int launch_sddmm_v(const spmv_csr &h, int k, const float *U, int64_t ldu, const float *X, int64_t ldx, float *out,
                   hipStream_t s)
{
    const SpmmPlan &p = h.plan_spmm;
    constexpr int kRowsPerBlock = kSddmmBlock / V;
    const int64_t nblocks = (h.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    // (a launch carries fewer than 2^32 work-items, as in launch_spmm_v: rows x lanes per row < 2^32)
    if (nblocks * kSddmmBlock >= (1LL << 32)) {
        set_error("spmv_csr_sddmm: %lld rows x %d lanes per row reach the launch limit of 2^32 work-items", (long long)h.rows, V);
        return SPMV_ERR_INVALID;
    }
    hipLaunchKernelGGL((k_sddmm_rows<V, VEC>), dim3((unsigned)nblocks), dim3(kSddmmBlock), 0, s, h.rows, nblocks, p.row_cap,
                       V == 1 ? nullptr : p.d_order.get(), h.d_row_ptr, h.d_col_idx, U, ldu, X, ldx, out, k);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "k_sddmm_rows", __FILE__, __LINE__);
    if (!p.n_long) return SPMV_OK;
    constexpr int kPiecesPerBlock = kSddmmBlock / V;
    hipLaunchKernelGGL((k_sddmm_pieces<V, VEC>), dim3((unsigned)((p.pieces + kPiecesPerBlock - 1) / kPiecesPerBlock)),
                       dim3(kSddmmBlock), 0, s, p.pieces, p.n_long, p.d_long_row.get(), p.d_long_first.get(),
                       p.d_piece_k0.get(), p.d_piece_len.get(), h.d_col_idx, U, ldu, X, ldx, out, k);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "k_sddmm_pieces", __FILE__, __LINE__);
    return SPMV_OK;
}

template <bool VEC>
int launch_sddmm_vec(const spmv_csr &h, int k, const float *U, int64_t ldu, const float *X, int64_t ldx, float *out,
                     hipStream_t s)
{
    const int slices = (k + 3) / 4;
    if (slices <= 1) return launch_sddmm_v<1, VEC>(h, k, U, ldu, X, ldx, out, s);
    if (slices <= 2) return launch_sddmm_v<2, VEC>(h, k, U, ldu, X, ldx, out, s);
    if (slices <= 4) return launch_sddmm_v<4, VEC>(h, k, U, ldu, X, ldx, out, s);
    if (slices <= 8) return launch_sddmm_v<8, VEC>(h, k, U, ldu, X, ldx, out, s);
    return launch_sddmm_v<16, VEC>(h, k, U, ldu, X, ldx, out, s);
}

}  // namespace

// arguments checked by spmv_csr_sddmm: 1 <= k <= 64, ld >= k, U / X 16-byte aligned, the SpMM plan made
int launch_sddmm(const spmv_csr &h, int k, const float *U, int64_t ldu, const float *X, int64_t ldx, float *out, hipStream_t s)
{
    if (h.rows == 0 || h.nnz == 0) return SPMV_OK;
    if (ldu % 4 == 0 && ldx % 4 == 0) return launch_sddmm_vec<true>(h, k, U, ldu, X, ldx, out, s);
    return launch_sddmm_vec<false>(h, k, U, ldu, X, ldx, out, s);
}

}  // namespace spmv
