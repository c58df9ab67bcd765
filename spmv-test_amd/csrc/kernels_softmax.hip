// kernels_softmax.hip -- the softmax of every row of a CSR pattern and its backward (spmv_csr_row_softmax,
// spmv_csr_row_softmax_backward, include/spmv_hip.h "Row softmax"): the step between the SDDMM that makes the scores of
// a sparse attention and the SpMM that applies them.  Every array holds nnz floats in the handle's storage order; only
// row_ptr and the SpMM plan's long rows are read, never col_idx or vals.
//
// Geometry.  A wavefront owns 64 consecutive rows (a workgroup of 256 threads 256 rows, dealt per XCD as the SpMM blocks
// are: xcd_item64 of lane_group.hpp).  Lane l loads the bounds of row r0 + l; the longest of the 64 rows (rows of more than row_cap nonzeros count as
// empty here) decides how the wavefront walks them:
//   at most 64   groups of G = pow2 >= that length lanes, one row per group, 64 / G rows per pass, one element per lane:
//                the rows are contiguous in storage, so a pass loads a nearly contiguous span;
//   more         the whole wavefront per row, lane l holding elements l, l + 64, ... (at most 8: row_cap <= 512).
// Either way a row is read once, held in registers and written once.  G depends on the wavefront's own rows only, and
// the two walks give the same bits (below), so a row's result does not depend on its neighbours.
// Rows of more than row_cap nonzeros go by the plan's pieces (<= 512 nonzeros, one wavefront each) in three reads: the
// pieces' maxima, the row's maximum, the pieces' sums of exp(t - M), the row's sum, then the store (backward: the pieces'
// dots, the row's dot, the store).  The scratch is the plan's d_partial, 64 floats per piece, of which slots 0 .. 3 of a
// piece are used: [0] the piece's maximum (backward: its dot), [1] its sum, and in the row's FIRST piece [2] the row's
// maximum (backward: dot) and [3] the row's sum.
//
// The order of the fp32 operations (the header states it; tests/test_softmax_host.py emulates it).  A "piece" is a whole
// row of at most 512 entries or a plan piece; x_0 .. x_(len-1) its terms (forward: e = expf(t - M); backward: the rounded
// products P dP):
//   q_l = +0;  q_l = q_l + x_(l + 64 j) for j = 0, 1, ... while l + 64 j < len              (l = 0 .. 63)
//   for m = 32, 16, ..., 1:  q_l = q_l + q_(l xor m);      the piece's sum is q_0
// and the sums of the pieces of a long row are added in piece order from +0.  A lane past the piece holds +0 (-Inf for the
// maximum), and q_l is never -0, so the butterfly levels at m >= G add +0 to a number that is not -0: a group of G < 64
// lanes that runs the levels m = G/2 .. 1 only has the full butterfly's bits.  Nothing is contracted into an fma
// (fp contract is off in this file): t = scale * s is rounded before M is subtracted.
//
// Aliasing: out may be scores, dS may be P or dP (the identical pointer): every element is read by the lane that writes it,
// and in the three-read walk the stores come in the last launch.  Hence no __restrict__ on these arrays.
// Addresses are 64-bit; no buffer descriptor and no range check is relied on.
#include "lane_group.hpp"

#pragma clang fp contract(off)

namespace spmv {

namespace {

constexpr int kSmBlock = 256;                 // 4 wavefronts
constexpr int kSmWaves = kSmBlock / kWave;
constexpr int kSmPiece = 512;                 // the most nonzeros a wavefront holds in registers
constexpr int kSmRegs = kSmPiece / kWave;     // 8 per lane
constexpr int kSmSlots = 64;                  // floats of plan scratch per piece (SpmmPlan::d_partial)

// the xor-butterfly m = G/2 .. 1 inside every group of G lanes (G a power of two, wavefront-uniform)
__device__ __forceinline__ float group_sum(float q, int G)
{
#pragma unroll
    for (int m = kWave / 2; m >= 1; m /= 2)
        if (m < G) q = q + __shfl_xor(q, m);
    return q;
}

__device__ __forceinline__ float group_max(float q, int G)
{
#pragma unroll
    for (int m = kWave / 2; m >= 1; m /= 2)
        if (m < G) q = fmaxf(q, __shfl_xor(q, m));
    return q;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int m = kWave / 2; m >= 1; m /= 2) {
        const int o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// ---- one piece in the registers of one wavefront: element l + 64 j of [b, b + len) in slot j of lane l ---------------
__device__ __forceinline__ void piece_scaled(const float *x, int64_t b, int len, int lane, float scale, float (&t)[kSmRegs])
{
#pragma unroll
    for (int j = 0; j < kSmRegs; ++j) {
        const int i = lane + j * kWave;
        t[j] = i < len ? scale * x[b + i] : -INFINITY;
    }
}

__device__ __forceinline__ float piece_max(const float (&t)[kSmRegs])
{
    float m = t[0];
#pragma unroll
    for (int j = 1; j < kSmRegs; ++j) m = fmaxf(m, t[j]);
    return group_max(m, kWave);
}

// e = expf(t - M) in place (+0 past the piece); returns the piece's sum
__device__ __forceinline__ float piece_exp_sum(float (&t)[kSmRegs], int len, int lane, float M)
{
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < kSmRegs; ++j) {
        t[j] = lane + j * kWave < len ? expf(t[j] - M) : 0.0f;
        q = q + t[j];
    }
    return group_sum(q, kWave);
}

__device__ __forceinline__ void piece_store_scaled(float *out, int64_t b, int len, int lane, const float (&e)[kSmRegs], float r)
{
#pragma unroll
    for (int j = 0; j < kSmRegs; ++j) {
        const int i = lane + j * kWave;
        if (i < len) out[b + i] = e[j] * r;
    }
}

__device__ __forceinline__ float piece_dot(const float *P, const float *dP, int64_t b, int len, int lane, float (&p)[kSmRegs],
                                           float (&g)[kSmRegs])
{
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < kSmRegs; ++j) {
        const int i = lane + j * kWave;
        p[j] = i < len ? P[b + i] : 0.0f;
        g[j] = i < len ? dP[b + i] : 0.0f;
        const float prod = p[j] * g[j];
        q = q + (i < len ? prod : 0.0f);
    }
    return group_sum(q, kWave);
}

__device__ __forceinline__ void piece_store_backward(float *dS, int64_t b, int len, int lane, const float (&p)[kSmRegs],
                                                     const float (&g)[kSmRegs], float dot, float scale)
{
#pragma unroll
    for (int j = 0; j < kSmRegs; ++j) {
        const int i = lane + j * kWave;
        if (i < len) dS[b + i] = scale * (p[j] * (g[j] - dot));
    }
}

// the bounds of the wavefront's 64 rows, one per lane (a row of more than row_cap nonzeros, or past the matrix: len 0);
// returns the longest length
__device__ __forceinline__ int wave_rows(int64_t r0, int64_t rows, int row_cap, const int32_t *__restrict__ row_ptr, int lane,
                                         int &b, int &len)
{
    const int64_t r = r0 + lane;
    b = 0;
    len = 0;
    if (r < rows) {
        b = row_ptr[r];
        const int l = row_ptr[r + 1] - b;
        len = l > row_cap ? 0 : l;
    }
    return wave_max(len);
}

// ---- rows of at most row_cap nonzeros ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kSmBlock) void k_softmax_rows(int64_t rows, int64_t nblocks, int row_cap,
                                                           const int32_t *__restrict__ row_ptr, float scale, const float *x,
                                                           float *out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r0 = xcd_item64(blockIdx.x, nblocks) * kSmBlock + (threadIdx.x / kWave) * kWave;
    if (r0 >= rows) return;     // (wavefront-uniform, as every branch around a shuffle below)
    int b, len;
    const int lmax = wave_rows(r0, rows, row_cap, row_ptr, lane, b, len);
    if (lmax == 0) return;
    if (lmax <= kWave) {
        int G = 1, sh = 0;
        while (G < lmax) G *= 2, ++sh;
        const int sub = lane & (G - 1), per = kWave / G;
        for (int pass = 0; pass < G && r0 + pass * per < rows; ++pass) {
            const int src = pass * per + (lane >> sh);
            const int64_t rb = __shfl(b, src);
            const int rl = __shfl(len, src);
            const bool valid = sub < rl;
            const float t = valid ? scale * x[rb + sub] : -INFINITY;
            const float M = group_max(t, G);
            const float e = valid ? expf(t - M) : 0.0f;
            const float S = group_sum(0.0f + e, G);
            const float r = 1.0f / S;
            if (valid) out[rb + sub] = e * r;
        }
    } else {
        for (int i = 0; i < kWave && r0 + i < rows; ++i) {
            const int64_t rb = __shfl(b, i);
            const int rl = __shfl(len, i);
            if (rl == 0) continue;
            float t[kSmRegs];
            piece_scaled(x, rb, rl, lane, scale, t);
            const float M = piece_max(t);
            const float S = piece_exp_sum(t, rl, lane, M);
            piece_store_scaled(out, rb, rl, lane, t, 1.0f / S);
        }
    }
}

__global__ __launch_bounds__(kSmBlock) void k_softmax_bwd_rows(int64_t rows, int64_t nblocks, int row_cap,
                                                               const int32_t *__restrict__ row_ptr, float scale, const float *P,
                                                               const float *dP, float *dS)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r0 = xcd_item64(blockIdx.x, nblocks) * kSmBlock + (threadIdx.x / kWave) * kWave;
    if (r0 >= rows) return;
    int b, len;
    const int lmax = wave_rows(r0, rows, row_cap, row_ptr, lane, b, len);
    if (lmax == 0) return;
    if (lmax <= kWave) {
        int G = 1, sh = 0;
        while (G < lmax) G *= 2, ++sh;
        const int sub = lane & (G - 1), per = kWave / G;
        for (int pass = 0; pass < G && r0 + pass * per < rows; ++pass) {
            const int src = pass * per + (lane >> sh);
            const int64_t rb = __shfl(b, src);
            const int rl = __shfl(len, src);
            const bool valid = sub < rl;
            const float p = valid ? P[rb + sub] : 0.0f;
            const float g = valid ? dP[rb + sub] : 0.0f;
            const float prod = p * g;
            const float dot = group_sum(0.0f + (valid ? prod : 0.0f), G);
            if (valid) dS[rb + sub] = scale * (p * (g - dot));
        }
    } else {
        for (int i = 0; i < kWave && r0 + i < rows; ++i) {
            const int64_t rb = __shfl(b, i);
            const int rl = __shfl(len, i);
            if (rl == 0) continue;
            float p[kSmRegs], g[kSmRegs];
            const float dot = piece_dot(P, dP, rb, rl, lane, p, g);
            piece_store_backward(dS, rb, rl, lane, p, g, dot, scale);
        }
    }
}

// ---- rows of more than row_cap nonzeros: one wavefront per plan piece ------------------------------------------------------
// the first piece of the long row that holds piece p: long_first[lo] <= p < long_first[lo + 1]
__device__ __forceinline__ int64_t first_piece_of(int p, int n_long, const int32_t *__restrict__ long_first)
{
    int lo = 0, hi = n_long;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (long_first[mid] <= p) lo = mid;
        else hi = mid;
    }
    return long_first[lo];
}

enum { kPieceMax = 0, kPieceSum = 1, kPieceStore = 2 };

template <int STEP>
__global__ __launch_bounds__(kSmBlock) void k_softmax_pieces(int npieces, int n_long, const int32_t *__restrict__ long_first,
                                                             const int32_t *__restrict__ piece_k0,
                                                             const int32_t *__restrict__ piece_len, float scale, const float *x,
                                                             float *out, float *partial)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int p = blockIdx.x * kSmWaves + threadIdx.x / kWave;
    if (p >= npieces) return;
    const int64_t b = piece_k0[p];
    const int len = piece_len[p];
    float t[kSmRegs];
    piece_scaled(x, b, len, lane, scale, t);
    if (STEP == kPieceMax) {
        const float m = piece_max(t);
        if (lane == 0) partial[(int64_t)p * kSmSlots + 0] = m;
        return;
    }
    const int64_t f = first_piece_of(p, n_long, long_first);
    const float M = partial[f * kSmSlots + 2];
    const float s = piece_exp_sum(t, len, lane, M);
    if (STEP == kPieceSum) {
        if (lane == 0) partial[(int64_t)p * kSmSlots + 1] = s;
        return;
    }
    const float S = partial[f * kSmSlots + 3];
    piece_store_scaled(out, b, len, lane, t, 1.0f / S);
}

template <bool STORE>
__global__ __launch_bounds__(kSmBlock) void k_softmax_bwd_pieces(int npieces, int n_long, const int32_t *__restrict__ long_first,
                                                                 const int32_t *__restrict__ piece_k0,
                                                                 const int32_t *__restrict__ piece_len, float scale,
                                                                 const float *P, const float *dP, float *dS, float *partial)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int p = blockIdx.x * kSmWaves + threadIdx.x / kWave;
    if (p >= npieces) return;
    const int64_t b = piece_k0[p];
    const int len = piece_len[p];
    float pv[kSmRegs], g[kSmRegs];
    const float d = piece_dot(P, dP, b, len, lane, pv, g);
    if (!STORE) {
        if (lane == 0) partial[(int64_t)p * kSmSlots + 0] = d;
        return;
    }
    const float dot = partial[first_piece_of(p, n_long, long_first) * kSmSlots + 2];
    piece_store_backward(dS, b, len, lane, pv, g, dot, scale);
}

// one thread per long row: slot `src` of its pieces folded in piece order (the maximum from -Inf, the sum from +0) into
// slot `dst` of its first piece
template <bool MAX>
__global__ __launch_bounds__(kSmBlock) void k_softmax_fold(int n_long, const int32_t *__restrict__ long_first, float *partial,
                                                           int src, int dst)
{
    const int i = blockIdx.x * kSmBlock + threadIdx.x;
    if (i >= n_long) return;
    const int f = long_first[i], l = long_first[i + 1];
    float acc = MAX ? -INFINITY : 0.0f;
    for (int p = f; p < l; ++p) {
        const float v = partial[(int64_t)p * kSmSlots + src];
        acc = MAX ? fmaxf(acc, v) : acc + v;
    }
    partial[(int64_t)f * kSmSlots + dst] = acc;
}

int check_plan(const SpmmPlan &p, const char *what)
{
    if (p.row_cap > kSmPiece || p.piece_len > kSmPiece) {   // (a wavefront holds a row or a piece in 8 registers per lane)
        set_error("%s: the plan's row_cap = %d or piece_len = %d exceeds %d", what, p.row_cap, p.piece_len, kSmPiece);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

}  // namespace

// arguments checked by spmv_csr_row_softmax: the pointers, a finite scale, the SpMM plan made
int launch_row_softmax(const spmv_csr &h, float scale, const float *scores, float *out, hipStream_t s)
{
    if (h.rows == 0 || h.nnz == 0) return SPMV_OK;
    const SpmmPlan &p = h.plan_spmm;
    if (int rc = check_plan(p, "spmv_csr_row_softmax")) return rc;
    const int64_t nblocks = (h.rows + kSmBlock - 1) / kSmBlock;      // (rows < 2^31: fewer than 2^23 blocks)
    hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)nblocks), dim3(kSmBlock), 0, s, h.rows, nblocks, p.row_cap, h.d_row_ptr,
                       scale, scores, out);
    SPMV_LAUNCHED("k_softmax_rows");
    if (!p.n_long) return SPMV_OK;
    const dim3 pg((unsigned)((p.pieces + kSmWaves - 1) / kSmWaves)), lg((unsigned)((p.n_long + kSmBlock - 1) / kSmBlock));
    const int32_t *lf = p.d_long_first.get(), *k0 = p.d_piece_k0.get(), *ln = p.d_piece_len.get();
    float *part = p.d_partial.get();
    hipLaunchKernelGGL(k_softmax_pieces<kPieceMax>, pg, dim3(kSmBlock), 0, s, p.pieces, p.n_long, lf, k0, ln, scale, scores, out, part);
    SPMV_LAUNCHED("k_softmax_pieces<max>");
    hipLaunchKernelGGL(k_softmax_fold<true>, lg, dim3(kSmBlock), 0, s, p.n_long, lf, part, 0, 2);
    SPMV_LAUNCHED("k_softmax_fold<max>");
    hipLaunchKernelGGL(k_softmax_pieces<kPieceSum>, pg, dim3(kSmBlock), 0, s, p.pieces, p.n_long, lf, k0, ln, scale, scores, out, part);
    SPMV_LAUNCHED("k_softmax_pieces<sum>");
    hipLaunchKernelGGL(k_softmax_fold<false>, lg, dim3(kSmBlock), 0, s, p.n_long, lf, part, 1, 3);
    SPMV_LAUNCHED("k_softmax_fold<sum>");
    hipLaunchKernelGGL(k_softmax_pieces<kPieceStore>, pg, dim3(kSmBlock), 0, s, p.pieces, p.n_long, lf, k0, ln, scale, scores, out, part);
    SPMV_LAUNCHED("k_softmax_pieces<store>");
    return SPMV_OK;
}

int launch_row_softmax_backward(const spmv_csr &h, float scale, const float *P, const float *dP, float *dS, hipStream_t s)
{
    if (h.rows == 0 || h.nnz == 0) return SPMV_OK;
    const SpmmPlan &p = h.plan_spmm;
    if (int rc = check_plan(p, "spmv_csr_row_softmax_backward")) return rc;
    const int64_t nblocks = (h.rows + kSmBlock - 1) / kSmBlock;
    hipLaunchKernelGGL(k_softmax_bwd_rows, dim3((unsigned)nblocks), dim3(kSmBlock), 0, s, h.rows, nblocks, p.row_cap, h.d_row_ptr,
                       scale, P, dP, dS);
    SPMV_LAUNCHED("k_softmax_bwd_rows");
    if (!p.n_long) return SPMV_OK;
    const dim3 pg((unsigned)((p.pieces + kSmWaves - 1) / kSmWaves)), lg((unsigned)((p.n_long + kSmBlock - 1) / kSmBlock));
    const int32_t *lf = p.d_long_first.get(), *k0 = p.d_piece_k0.get(), *ln = p.d_piece_len.get();
    float *part = p.d_partial.get();
    hipLaunchKernelGGL(k_softmax_bwd_pieces<false>, pg, dim3(kSmBlock), 0, s, p.pieces, p.n_long, lf, k0, ln, scale, P, dP, dS, part);
    SPMV_LAUNCHED("k_softmax_bwd_pieces<dot>");
    hipLaunchKernelGGL(k_softmax_fold<false>, lg, dim3(kSmBlock), 0, s, p.n_long, lf, part, 0, 2);
    SPMV_LAUNCHED("k_softmax_fold<dot>");
    hipLaunchKernelGGL(k_softmax_bwd_pieces<true>, pg, dim3(kSmBlock), 0, s, p.pieces, p.n_long, lf, k0, ln, scale, P, dP, dS, part);
    SPMV_LAUNCHED("k_softmax_bwd_pieces<store>");
    return SPMV_OK;
}

}  // namespace spmv
