// kernels_spmm.hip -- Y = A X for k <= 64 right-hand sides at once (spmv_csr_spmm, include/spmv_hip.h "SpMM").
//
// X is cols rows of ldx floats (row-major), Y rows rows of ldy floats.  A group of V = pow2 >= ceil(k/4) lanes owns one
// row of A: lane s of the group holds columns [4s, 4s+4) of Y's row in four accumulators and reads the same columns of
// every X row the CSR row refers to (one 16-byte slice per nonzero where ldx % 4 == 0).  A group walks its row in steps
// of T = max(V, 8) nonzeros: the group loads the step's (col_idx, vals) coalesced, broadcasts them inside the group with
// shuffles, issues all T slice gathers and only then multiplies and adds, one nonzero after the other.
//
// The order of the fp32 additions of column c is fixed by the row alone: acc = fma(v, x, acc) over the row's nonzeros in
// storage order, from +0 -- the same for every V, every ld and every position of c in the batch (batch invariance).  Rows
// longer than kSpmmRowCap nonzeros are cut by the plan into pieces of kSpmmPiece nonzeros (plan-fixed boundaries); a
// group sums each piece the same way into a partial of 64 floats, and k_spmm_combine adds a row's partials in piece
// order (from +0).  Nothing here depends on k but how many columns are computed and stored.
//
// Addresses are 64-bit (X and Y may exceed 4 GiB: c4 at k = 64 is 4.3 GB each), so the 32-bit range of buffer descriptors
// does not arise.  A lane whose slice starts at or past k does nothing; the last slice of a k that is not a multiple of 4
// reads its 16-byte block whole when ldx % 4 == 0 (the block holds X[j*ldx + k-1], inside the caller's row) and stores
// only the columns below k.  With ld % 4 != 0 the kernels read and store 4-byte elements, columns below k only.
#include <algorithm>
#include <numeric>
#include <vector>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

constexpr int kSpmmBlock = 256;     // 4 wavefronts
constexpr int kSpmmRowCap = 512;    // rows of more nonzeros go in pieces
constexpr int kSpmmPiece = 512;     // nonzeros of a piece
constexpr int kSpmmMaxK = 64;       // columns of a piece's partial (the scratch is sized for k = 64 at plan time)
constexpr int kSpmmSortRows = 4096; // the plan orders the rows of each block of this many by length (a wave's rows alike)

// block b of the grid takes item spmm_xcd_item(b, n): blocks are dealt round-robin over the 8 XCDs, so each XCD gets one
// contiguous range of row blocks (neighbouring rows share lines of X in that XCD's L2)
__device__ __forceinline__ int64_t spmm_xcd_item(int64_t bid, int64_t n)
{
    const int64_t q = n / kXcds, rem = n % kXcds;
    const int64_t j = bid % kXcds, idx = bid / kXcds;
    return j * q + (j < rem ? j : rem) + idx;
}

// the four columns [c0, c0+4) of X row j (c0 < k); VEC: one 16-byte load (ldx % 4 == 0), else the columns below k only
template <bool VEC>
__device__ __forceinline__ float4 load_slice(const float *__restrict__ X, int64_t ldx, int32_t j, int c0, int k)
{
    const float *p = X + (int64_t)j * ldx + c0;
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.x = p[0];
    if (c0 + 1 < k) r.y = p[1];
    if (c0 + 2 < k) r.z = p[2];
    if (c0 + 3 < k) r.w = p[3];
    return r;
}

// the columns [c0, c0+4) below k of one row of Y (vector stores only)
template <bool VEC>
__device__ __forceinline__ void store_slice(float *__restrict__ p, float4 a, int c0, int k)
{
    if (VEC && c0 + 4 <= k) {
        *reinterpret_cast<float4 *>(p) = a;
        return;
    }
    p[0] = a.x;
    if (c0 + 1 < k) p[1] = a.y;
    if (c0 + 2 < k) p[2] = a.z;
    if (c0 + 3 < k) p[3] = a.w;
}

// sum over the nonzeros [b, e) of the group's row (or piece) of vals[n] * X[col_idx[n]][c0 .. c0+3], in storage order.
// All lanes of a group call it with the same b, e; lanes with c0 >= k load and add nothing (their shuffles still run).
template <int V, bool VEC>
__device__ __forceinline__ float4 row_dot(int lane, int64_t b, int64_t e, const int32_t *__restrict__ col_idx,
                                          const float *__restrict__ vals, const float *__restrict__ X, int64_t ldx, int c0,
                                          int k)
{
    constexpr int T = V > 8 ? V : 8;     // nonzeros per step: T slice gathers in flight per lane
    constexpr int L = T / V;             // of which each lane of the group loads L
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const bool active = c0 < k;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int64_t kb = b; kb < e; kb += T) {
        int32_t c[L];
        float v[L];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int64_t n = kb + (int64_t)i * V + sub;
            c[i] = n < e ? col_idx[n] : 0;
            v[i] = n < e ? vals[n] : 0.0f;
        }
        int32_t ct[T];
        float vt[T];
        float4 xt[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (V == 1) {
                ct[t] = c[t];
                vt[t] = v[t];
            } else {
                ct[t] = __shfl(c[t / V], gbase + t % V);
                vt[t] = __shfl(v[t / V], gbase + t % V);
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
            xt[t] = (active && kb + t < e) ? load_slice<VEC>(X, ldx, ct[t], c0, k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {     // (a slot past the end adds nothing: not even +0, which would turn an acc of -0 into +0)
                acc.x = fmaf(vt[t], xt[t].x, acc.x);
                acc.y = fmaf(vt[t], xt[t].y, acc.y);
                acc.z = fmaf(vt[t], xt[t].z, acc.z);
                acc.w = fmaf(vt[t], xt[t].w, acc.w);
            }
        }
    }
    return acc;
}

// a group of V lanes per row, the rows taken in `order` (null: in row order); rows of more than kSpmmRowCap nonzeros are
// left to the pieces and the combine
template <int V, bool VEC>
__global__ __launch_bounds__(kSpmmBlock) void k_spmm_rows(int64_t rows, int64_t nblocks, const int32_t *__restrict__ order,
                                                          const int32_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col_idx, const float *__restrict__ vals,
                                                          const float *__restrict__ X, int64_t ldx, float *__restrict__ Y,
                                                          int64_t ldy, int k)
{
    constexpr int kRowsPerBlock = kSpmmBlock / V;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t blk = spmm_xcd_item(blockIdx.x, nblocks);
    const int64_t slot = blk * kRowsPerBlock + threadIdx.x / V;
    if (slot >= rows) return;   // (group-uniform: a group never splits here)
    const int64_t r = order ? order[slot] : slot;
    const int64_t b = row_ptr[r], e = row_ptr[r + 1];
    if (e - b > kSpmmRowCap) return;
    const int c0 = 4 * (lane & (V - 1));
    const float4 acc = row_dot<V, VEC>(lane, b, e, col_idx, vals, X, ldx, c0, k);
    if (c0 < k) store_slice<VEC>(Y + r * ldy + c0, acc, c0, k);
}

// a group of V lanes per piece of a long row: partial[p][0 .. 4V) (the scratch holds kSpmmMaxK floats per piece)
template <int V, bool VEC>
__global__ __launch_bounds__(kSpmmBlock) void k_spmm_pieces(int npieces, const int32_t *__restrict__ piece_k0,
                                                            const int32_t *__restrict__ piece_len,
                                                            const int32_t *__restrict__ col_idx, const float *__restrict__ vals,
                                                            const float *__restrict__ X, int64_t ldx,
                                                            float *__restrict__ partial, int k)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t p = (int64_t)blockIdx.x * (kSpmmBlock / V) + threadIdx.x / V;
    if (p >= npieces) return;
    const int64_t b = piece_k0[p], e = b + piece_len[p];
    const int c0 = 4 * (lane & (V - 1));
    const float4 acc = row_dot<V, VEC>(lane, b, e, col_idx, vals, X, ldx, c0, k);
    if (c0 < k) *reinterpret_cast<float4 *>(partial + p * kSpmmMaxK + c0) = acc;
}

// one thread per (long row, column < k): the row's partials added in piece order
__global__ __launch_bounds__(kSpmmBlock) void k_spmm_combine(int n_long, const int32_t *__restrict__ long_row,
                                                             const int32_t *__restrict__ long_first,
                                                             const float *__restrict__ partial, float *__restrict__ Y,
                                                             int64_t ldy, int k)
{
    const int64_t t = (int64_t)blockIdx.x * kSpmmBlock + threadIdx.x;
    const int64_t i = t / k;
    const int c = (int)(t % k);
    if (i >= n_long) return;
    float acc = 0.0f;
    for (int p = long_first[i]; p < long_first[i + 1]; ++p) acc += partial[(int64_t)p * kSpmmMaxK + c];
    Y[(int64_t)long_row[i] * ldy + c] = acc;
}

}  // namespace

// The plan: the rows of more than kSpmmRowCap nonzeros and their pieces, in row order -- a function of row_ptr alone.
// Reads row_ptr back to the host once and waits for the stream (not graph-capturable; spmv_csr_spmm is).
int plan_spmm(spmv_csr &h, hipStream_t s)
{
    if (h.plan_spmm.ready) return SPMV_OK;
    h.plan_spmm = SpmmPlan{};
    std::vector<int32_t> rp((size_t)h.rows + 1);
    SPMV_HIP_TRY(hipMemcpyAsync(rp.data(), h.d_row_ptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> lr, lf, k0, ln;
    for (int64_t r = 0; r < h.rows; ++r) {
        const int32_t b = rp[(size_t)r], e = rp[(size_t)r + 1];
        if (e - b <= kSpmmRowCap) continue;
        lr.push_back((int32_t)r);
        lf.push_back((int32_t)k0.size());
        for (int64_t q = b; q < e; q += kSpmmPiece) {   // (64 bits: q + kSpmmPiece passes INT_MAX on a row that ends near it)
            k0.push_back((int32_t)q);
            ln.push_back((int32_t)(e - q < kSpmmPiece ? e - q : kSpmmPiece));
        }
    }
    lf.push_back((int32_t)k0.size());
    // the rows of every block of kSpmmSortRows, stably by length: the 64 / V rows a wavefront walks side by side end at
    // nearly the same step, and the block's rows still share their window of X.  V = 1 (k <= 4) keeps the row order:
    // there each lane streams its own row's col_idx / vals, and neighbouring rows keep those loads on neighbouring lines
    // (measured: 2x faster at k = 1 and 4 on configs 3 and 4; from V = 2 on the sorted order wins, up to 2.5x)
    std::vector<int32_t> order((size_t)h.rows);
    std::iota(order.begin(), order.end(), 0);
    for (int64_t r0 = 0; r0 < h.rows; r0 += kSpmmSortRows) {
        const int64_t r1 = std::min<int64_t>(h.rows, r0 + kSpmmSortRows);
        std::stable_sort(order.begin() + r0, order.begin() + r1, [&](int32_t a, int32_t b) {
            return rp[(size_t)a + 1] - rp[(size_t)a] < rp[(size_t)b + 1] - rp[(size_t)b];
        });
    }
    SpmmPlan p;
    p.n_long = (int)lr.size();
    p.pieces = (int)k0.size();
    DevPtr<int32_t> d_ord, d_lr, d_lf, d_k0, d_ln;
    SPMV_HIP_TRY(d_ord.alloc(order.size()));
    SPMV_HIP_TRY(hipMemcpyAsync(d_ord.get(), order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, s));
    DevPtr<float> d_part;
    SPMV_HIP_TRY(d_lr.alloc(lr.size()));
    SPMV_HIP_TRY(d_lf.alloc(lf.size()));
    SPMV_HIP_TRY(d_k0.alloc(k0.size()));
    SPMV_HIP_TRY(d_ln.alloc(ln.size()));
    SPMV_HIP_TRY(d_part.alloc((size_t)p.pieces * kSpmmMaxK));
    if (p.n_long) {
        SPMV_HIP_TRY(hipMemcpyAsync(d_lr.get(), lr.data(), sizeof(int32_t) * lr.size(), hipMemcpyHostToDevice, s));
        SPMV_HIP_TRY(hipMemcpyAsync(d_k0.get(), k0.data(), sizeof(int32_t) * k0.size(), hipMemcpyHostToDevice, s));
        SPMV_HIP_TRY(hipMemcpyAsync(d_ln.get(), ln.data(), sizeof(int32_t) * ln.size(), hipMemcpyHostToDevice, s));
    }
    SPMV_HIP_TRY(hipMemcpyAsync(d_lf.get(), lf.data(), sizeof(int32_t) * lf.size(), hipMemcpyHostToDevice, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));     // (the host vectors die with this call)
    p.d_order = std::move(d_ord);
    p.d_long_row = std::move(d_lr);
    p.d_long_first = std::move(d_lf);
    p.d_piece_k0 = std::move(d_k0);
    p.d_piece_len = std::move(d_ln);
    p.d_partial = std::move(d_part);
    p.row_cap = kSpmmRowCap;
    p.piece_len = kSpmmPiece;
    p.ready = true;
    h.plan_spmm = std::move(p);
    return SPMV_OK;
}

int64_t spmm_plan_bytes(const spmv_csr &h)
{
    const SpmmPlan &p = h.plan_spmm;
    if (!p.ready) return 0;
    return h.rows * 4 + (int64_t)p.n_long * 4 + ((int64_t)p.n_long + 1) * 4 + (int64_t)p.pieces * 8 + (int64_t)p.pieces * kSpmmMaxK * 4;
}

template <int V, bool VEC>
static int launch_spmm_v(const spmv_csr &h, int k, const float *X, int64_t ldx, float *Y, int64_t ldy, hipStream_t s)
{
    const SpmmPlan &p = h.plan_spmm;
    constexpr int kRowsPerBlock = kSpmmBlock / V;
    const int64_t nblocks = (h.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    // (a launch carries fewer than 2^32 work-items -- the runtime passes grid x block on in 32 bits and a larger product wraps
    // silently: rows x lanes per row < 2^32 -- any handle up to k = 8, rows < 2^30 / 2^29 / 2^28 up to k = 16 / 32 / 64)
    if (nblocks * kSpmmBlock >= (1LL << 32)) {
        set_error("spmv_csr_spmm: %lld rows x %d lanes per row reach the launch limit of 2^32 work-items", (long long)h.rows, V);
        return SPMV_ERR_INVALID;
    }
    hipLaunchKernelGGL((k_spmm_rows<V, VEC>), dim3((unsigned)nblocks), dim3(kSpmmBlock), 0, s, h.rows, nblocks,
                       V == 1 ? nullptr : p.d_order, h.d_row_ptr,
                       h.d_col_idx, h.d_vals, X, ldx, Y, ldy, k);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "k_spmm_rows", __FILE__, __LINE__);
    if (!p.n_long) return SPMV_OK;
    constexpr int kPiecesPerBlock = kSpmmBlock / V;
    hipLaunchKernelGGL((k_spmm_pieces<V, VEC>), dim3((unsigned)((p.pieces + kPiecesPerBlock - 1) / kPiecesPerBlock)),
                       dim3(kSpmmBlock), 0, s, p.pieces, p.d_piece_k0, p.d_piece_len, h.d_col_idx, h.d_vals, X, ldx,
                       p.d_partial, k);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "k_spmm_pieces", __FILE__, __LINE__);
    const int64_t threads = (int64_t)p.n_long * k;
    hipLaunchKernelGGL(k_spmm_combine, dim3((unsigned)((threads + kSpmmBlock - 1) / kSpmmBlock)), dim3(kSpmmBlock), 0, s,
                       p.n_long, p.d_long_row, p.d_long_first, p.d_partial, Y, ldy, k);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, "k_spmm_combine", __FILE__, __LINE__);
    return SPMV_OK;
}

template <bool VEC>
static int launch_spmm_vec(const spmv_csr &h, int k, const float *X, int64_t ldx, float *Y, int64_t ldy, hipStream_t s)
{
    const int slices = (k + 3) / 4;
    if (slices <= 1) return launch_spmm_v<1, VEC>(h, k, X, ldx, Y, ldy, s);
    if (slices <= 2) return launch_spmm_v<2, VEC>(h, k, X, ldx, Y, ldy, s);
    if (slices <= 4) return launch_spmm_v<4, VEC>(h, k, X, ldx, Y, ldy, s);
    if (slices <= 8) return launch_spmm_v<8, VEC>(h, k, X, ldx, Y, ldy, s);
    return launch_spmm_v<16, VEC>(h, k, X, ldx, Y, ldy, s);
}

// arguments checked by spmv_csr_spmm: 1 <= k <= 64, ld >= k, X / Y 16-byte aligned, the plan made
int launch_spmm(const spmv_csr &h, int k, const float *X, int64_t ldx, float *Y, int64_t ldy, hipStream_t s)
{
    if (h.rows == 0) return SPMV_OK;
    if (ldx % 4 == 0 && ldy % 4 == 0) return launch_spmm_vec<true>(h, k, X, ldx, Y, ldy, s);
    return launch_spmm_vec<false>(h, k, X, ldx, Y, ldy, s);
}

}  // namespace spmv
