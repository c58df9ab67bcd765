// kernels_permute.hip -- spmv_csr_permute / _values / _gather and spmv_permute_vector (include/spmv_hip.h "the multicolour
// ordering"): B = P A Q^T as a new handle.  New index r holds old index perm[r]: row r of B is row row_perm[r] of A, and an
// entry in column j of A lands in column inv_col[j] (col_perm[inv_col[j]] = j).  Inside a row of B the entries ascend by
// (new column, storage position in A), so the result does not depend on the route, on timing or on the lane that did the work.
//
//   0. k_perm_invert / k_perm_verify: inv[p] = the smallest index i with perm[i] = p (an integer minimum per mark, independent
//      of arrival order); an index whose entry is out of range or whose mark another index holds is an integer minimum too.
//      For a permutation inv is its inverse.
//   Direct route:
//   1. k_perm_lengths   B's row lengths (scan_offsets_i32 makes them row_ptr), the longest row, how many rows hold 9 .. 64
//                       entries, and the list of the rows of more than 64 (its order reaches no output).
//   2. k_perm_rank<G>   a group of G lanes per row of at most G entries (G = 8, then 64 for what is left): a lane per entry,
//                       the others' new columns through __shfl, rank = the entries with a smaller (column, position).
//   3. k_perm_bitonic   a workgroup per row of 65 .. 4096 entries: the 64-bit keys column << 32 | position in LDS, padded to
//                       a power of two with ~0, sorted by a bitonic network.
//   Route via the transpose (the flag, and every call with a row of more than 4096 entries): relabel the columns, transpose
//   (kernels_transpose.hip, with its map), relabel its columns (A's rows) by the inverse row permutation, transpose again and
//   compose the two maps.  Two stable sorts by the library's own code: linear in nnz whatever the row lengths.
//
// The atomics: integer minima and maxima on words that hold the same value whatever the order of arrival, a counter, and the
// place of a row in the list of long rows.  None returns a value that reaches B.  Positions are unsigned 32-bit (nnz < 2^31).
// Every access is predicated on its array's own length; permutations that were never verified move nothing outside the arrays.
#include <climits>
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

constexpr int kPermSmall = 8;              // rows of at most this many entries: a group of 8 lanes
constexpr int kPermLong = 4096;            // rows of more entries send the call through the transpose
enum { kPsLongest = 0, kPsMid = 1, kPsLong = 2, kPsWords = 8 };   // the direct route's state: the longest row above 8 entries, rows of 9 .. 64, rows above 64

struct PermRow { uint32_t lo, hi; };

__device__ __forceinline__ PermRow perm_row(const int32_t *rp, int64_t row, uint32_t nnz)
{
    const uint32_t hi = min((uint32_t)rp[row + 1], nnz), lo = min((uint32_t)rp[row], hi);
    return PermRow{lo, hi};
}

// the old row of new row r, or -1 where the permutation's entry is out of range
__device__ __forceinline__ int64_t perm_old(const int32_t *perm, int64_t r, int64_t n)
{
    const int64_t p = perm ? (int64_t)perm[r] : r;
    return p >= 0 && p < n ? p : -1;
}

// the new column of old column j (0xffffffff where j or the inverse's entry is out of range: it sorts behind every column)
__device__ __forceinline__ uint32_t perm_newcol(const int32_t *inv_col, int j, int64_t cols)
{
    if (j < 0 || (int64_t)j >= cols) return 0xffffffffu;
    const int c = inv_col ? inv_col[j] : j;
    return c >= 0 && (int64_t)c < cols ? (uint32_t)c : 0xffffffffu;
}

// ---- 0. the permutations ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_perm_invert(int64_t n, const int32_t *__restrict__ perm, int32_t *__restrict__ inv)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int p = perm[i];
    if (p >= 0 && (int64_t)p < n) atomicMin(&inv[p], (int32_t)i);
}

__global__ __launch_bounds__(kBlock) void k_perm_verify(int64_t n, const int32_t *__restrict__ perm, const int32_t *__restrict__ inv,
                                                        int32_t *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int p = perm[i];
    if (p < 0 || (int64_t)p >= n || inv[p] != (int32_t)i) atomicMin(bad, (int32_t)i);
}

// ---- 1. the row lengths ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_perm_lengths(int64_t rows, uint32_t nnz, const int32_t *__restrict__ rp,
                                                         const int32_t *__restrict__ row_perm, int32_t *__restrict__ len,
                                                         int32_t *__restrict__ longs, int32_t *__restrict__ st)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    const int64_t old = perm_old(row_perm, r, rows);
    int32_t n = 0;
    if (old >= 0) {
        const PermRow a = perm_row(rp, old, nnz);
        n = (int32_t)(a.hi - a.lo);
    }
    len[r] = n;
    if (n > kPermSmall) atomicMax(&st[kPsLongest], n);
    if (n > kPermSmall && n <= kWave) atomicAdd(&st[kPsMid], 1);
    if (n > kWave) {
        const int32_t at = atomicAdd(&st[kPsLong], 1);
        if (at >= 0 && (int64_t)at < rows) longs[at] = (int32_t)r;
    }
}

struct PermArgs {
    int64_t rows, cols;
    uint32_t nnz;                              // of A and of B
    const int32_t *rp, *ci;                    // A
    const uint32_t *va;                        // A's values as bits
    const int32_t *row_perm, *inv_col;         // null: the identity
    const int32_t *brp;                        // B
    int32_t *bci;
    uint32_t *bva, *map;                       // map null: not kept
};

__device__ __forceinline__ void perm_store(const PermArgs &p, uint64_t at, uint32_t col, uint32_t pos)
{
    if (at >= p.nnz) return;
    p.bci[at] = (int32_t)col;
    p.bva[at] = pos < p.nnz ? p.va[pos] : 0u;
    if (p.map) p.map[at] = pos;
}

// ---- 2. short rows: a group of G lanes per row, the rows of lo_len < entries <= G ----------------------------------------------
template <int G>
__global__ __launch_bounds__(kBlock) void k_perm_rank(PermArgs p, int lo_len)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int g0 = lane & ~(G - 1), t = lane & (G - 1);
    const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int64_t old = r < p.rows ? perm_old(p.row_perm, r, p.rows) : -1;
    PermRow a{0, 0};
    uint32_t b0 = 0, b1 = 0;
    if (old >= 0) {
        a = perm_row(p.rp, old, p.nnz);
        b1 = min((uint32_t)p.brp[r + 1], p.nnz);
        b0 = min((uint32_t)p.brp[r], b1);
    }
    int n = (int)min(a.hi - a.lo, b1 - b0);
    if (n <= lo_len || n > G) n = 0;                        // (another launch's row, or none)
    const uint32_t col = t < n ? perm_newcol(p.inv_col, p.ci[a.lo + (uint32_t)t], p.cols) : 0xffffffffu;
    int rank = 0;
#pragma unroll
    for (int u = 0; u < G; ++u) {                           // every lane of the wavefront takes every step
        const uint32_t other = (uint32_t)__shfl((int)col, g0 + u);
        if (u < n && (other < col || (other == col && u < t))) ++rank;
    }
    if (t < n) perm_store(p, (uint64_t)b0 + (uint32_t)rank, col, a.lo + (uint32_t)t);
}

// ---- 3. rows of 65 .. 4096 entries: one workgroup, a bitonic network over the keys in LDS -----------------------------------
__global__ __launch_bounds__(kBlock) void k_perm_bitonic(PermArgs p, const int32_t *__restrict__ longs, int32_t n_long)
{
    __shared__ uint64_t s_key[kPermLong];
    if ((int64_t)blockIdx.x >= (int64_t)n_long) return;
    const int64_t r = longs[blockIdx.x];
    if (r < 0 || r >= p.rows) return;
    const int64_t old = perm_old(p.row_perm, r, p.rows);
    if (old < 0) return;
    const PermRow a = perm_row(p.rp, old, p.nnz);
    const uint32_t b1 = min((uint32_t)p.brp[r + 1], p.nnz), b0 = min((uint32_t)p.brp[r], b1);
    const uint32_t n = min(a.hi - a.lo, b1 - b0);
    if (n > (uint32_t)kPermLong) return;                     // (the host sends such a call through the transpose)
    uint32_t width = kWave;
    while (width < n) width <<= 1;
    const int tid = (int)threadIdx.x;
    for (uint32_t i = (uint32_t)tid; i < width; i += kBlock)
        s_key[i] = i < n ? ((uint64_t)perm_newcol(p.inv_col, p.ci[a.lo + i], p.cols) << 32) | (a.lo + i) : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= width; k <<= 1) {
        for (uint32_t j = k >> 1; j >= 1; j >>= 1) {
            for (uint32_t i = (uint32_t)tid; i < width; i += kBlock) {
                const uint32_t q = i ^ j;
                if (q > i) {
                    const uint64_t x = s_key[i], y = s_key[q];
                    if (((i & k) == 0) == (x > y)) { s_key[i] = y; s_key[q] = x; }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = (uint32_t)tid; i < n; i += kBlock) perm_store(p, (uint64_t)b0 + i, (uint32_t)(s_key[i] >> 32), (uint32_t)s_key[i]);
}

// ---- the route via the transpose ---------------------------------------------------------------------------------------------
// out[k] = relabel[in[k]] (relabel null: in[k]); an entry outside [0, n) stays as it is.  `out` may be `in` itself.
__global__ __launch_bounds__(kBlock) void k_perm_relabel(int64_t nnz, int64_t n, const int32_t *in, const int32_t *__restrict__ relabel, int32_t *out)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= nnz) return;
    const int j = in[k];
    out[k] = (relabel && j >= 0 && (int64_t)j < n) ? relabel[j] : j;
}

// map[i] = first[map[i]], in place
__global__ __launch_bounds__(kBlock) void k_perm_compose(int64_t n, const uint32_t *__restrict__ first, uint32_t *map)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = map[i];
    map[i] = (int64_t)m < n ? first[m] : 0xffffffffu;
}

__global__ __launch_bounds__(kBlock) void k_perm_vector(int64_t n, const int32_t *__restrict__ perm, bool inverse, const uint32_t *__restrict__ src,
                                                        uint32_t *__restrict__ dst)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int p = perm[r];
    if (p < 0 || (int64_t)p >= n) return;
    if (inverse) dst[p] = src[r];
    else dst[r] = src[p];
}

unsigned perm_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int perm_fail(const char *msg)
{
    set_error("spmv_csr_permute: %s", msg);
    return SPMV_ERR_INVALID;
}

// inv = the inverse of perm (n entries) on the device; *bad_word takes the first index that makes perm no permutation
int perm_inverse(const int32_t *perm, int64_t n, DevPtr<int32_t> &inv, int32_t *bad_word, hipStream_t s)
{
    SPMV_HIP_TRY(inv.alloc((size_t)n));
    if (n == 0) return SPMV_OK;
    SPMV_HIP_TRY(hipMemsetAsync(inv.get(), 0x7f, sizeof(int32_t) * (size_t)n, s));      // 0x7f7f7f7f: above every index
    hipLaunchKernelGGL(k_perm_invert, dim3(perm_blocks(n)), dim3(kBlock), 0, s, n, perm, inv.get());
    if (int rc = check_launch("k_perm_invert")) return rc;
    hipLaunchKernelGGL(k_perm_verify, dim3(perm_blocks(n)), dim3(kBlock), 0, s, n, perm, (const int32_t *)inv.get(), bad_word);
    return check_launch("k_perm_verify");
}

int perm_finish(const spmv_csr &a, DevPtr<int32_t> &rp, DevPtr<int32_t> &ci, DevPtr<float> &va, DevPtr<uint32_t> &map, bool keep_map,
                spmv_csr_t **out)
{
    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) return perm_fail("out of host memory");
    h->rows = a.rows; h->cols = a.cols; h->nnz = a.nnz;
    h->device = a.device;
    h->d_row_ptr = rp; h->d_col_idx = ci; h->d_vals = va;
    h->own_row_ptr = std::move(rp); h->own_col_idx = std::move(ci); h->own_vals = std::move(va);
    if (keep_map) {
        h->map.words = std::move(map);
        h->map.parent_len = a.nnz;
        h->map.maker = MapMaker::permute;
    }
    *out = h;
    return SPMV_OK;
}

// B through two transposes; inv_row / inv_col null: the identity
int permute_via_transpose(const spmv_csr &a, const int32_t *inv_row, const int32_t *inv_col, bool keep_map, hipStream_t s, spmv_csr_t **out)
{
    const int64_t nnz = a.nnz;
    // A with its columns relabelled; its transpose lists every new column's entries in A's storage order
    DevPtr<int32_t> ci1;
    SPMV_HIP_TRY(ci1.alloc((size_t)nnz));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_perm_relabel, dim3(perm_blocks(nnz)), dim3(kBlock), 0, s, nnz, a.cols, a.d_col_idx, inv_col, ci1.get());
        if (int rc = check_launch("k_perm_relabel")) return rc;
    }
    spmv_csr a1;
    a1.rows = a.rows; a1.cols = a.cols; a1.nnz = nnz; a1.device = a.device;
    a1.d_row_ptr = a.d_row_ptr; a1.d_col_idx = ci1; a1.d_vals = a.d_vals;
    spmv_csr_t *t1 = nullptr;
    if (int rc = transpose(a1, true, s, &t1)) return rc;
    SPMV_HIP_TRY(ci1.reset());
    // ... whose columns (A's rows) become B's rows; its transpose lists every row of B by (new column, position in A)
    int rc = SPMV_OK;
    if (nnz > 0 && inv_row) {
        hipLaunchKernelGGL(k_perm_relabel, dim3(perm_blocks(nnz)), dim3(kBlock), 0, s, nnz, a.rows, (const int32_t *)t1->own_col_idx.get(), inv_row,
                           t1->own_col_idx.get());
        rc = check_launch("k_perm_relabel");
    }
    spmv_csr_t *b = nullptr;
    if (rc == SPMV_OK) rc = transpose(*t1, true, s, &b);
    if (rc == SPMV_OK && keep_map && nnz > 0) {
        // b's map holds positions of t1: through t1's map they are positions of A
        hipLaunchKernelGGL(k_perm_compose, dim3(perm_blocks(nnz)), dim3(kBlock), 0, s, nnz, (const uint32_t *)t1->map.words.get(),
                           b->map.words.get());
        rc = check_launch("k_perm_compose");
    }
    if (rc == SPMV_OK && hipStreamSynchronize(s) != hipSuccess) rc = perm_fail("the stream failed");
    (void)spmv_csr_destroy(t1);
    if (rc != SPMV_OK) {
        if (b) (void)spmv_csr_destroy(b);
        return rc;
    }
    if (keep_map) b->map.maker = MapMaker::permute;      // b's own map, now of positions of A: relabelled, not moved
    else b->map = PosMap();
    *out = b;
    return SPMV_OK;
}

// B by the direct route; *longest takes the longest row, and above kPermLong entries nothing is made (the caller's other route)
int permute_direct(const spmv_csr &a, const int32_t *row_perm, const int32_t *inv_col, bool keep_map, hipStream_t s, spmv_csr_t **out,
                   int64_t *longest)
{
    const int64_t rows = a.rows, cols = a.cols, nnz = a.nnz;
    DevPtr<int32_t> rp, ci, longs, d_st;
    DevPtr<float> va;
    DevPtr<uint32_t> map;
    int32_t st[kPsWords] = {};
    SPMV_HIP_TRY(d_st.alloc(kPsWords));
    SPMV_HIP_TRY(hipMemsetAsync(d_st.get(), 0, sizeof st, s));
    SPMV_HIP_TRY(rp.alloc((size_t)rows + 1));
    SPMV_HIP_TRY(longs.alloc((size_t)rows));
    int32_t total = 0;
    if (rows > 0) {
        hipLaunchKernelGGL(k_perm_lengths, dim3(perm_blocks(rows)), dim3(kBlock), 0, s, rows, (uint32_t)nnz, a.d_row_ptr, row_perm, rp.get(), longs.get(),
                           d_st.get());
        if (int rc = check_launch("k_perm_lengths")) return rc;
        SPMV_HIP_TRY(hipMemcpyAsync(st, d_st.get(), sizeof st, hipMemcpyDeviceToHost, s));
        if (int rc = scan_offsets_i32(rp.get(), rows, d_st.get() + 7, true, s, &total)) return rc;  // (waits for s: st has arrived)
    } else {
        SPMV_HIP_TRY(hipMemsetAsync(rp.get(), 0, sizeof(int32_t), s));
    }
    if ((int64_t)total != nnz) return perm_fail("the rows of a do not hold nnz entries (the arrays are not a valid CSR)");
    *longest = st[kPsLongest];
    if (st[kPsLongest] > kPermLong) return SPMV_OK;
    SPMV_HIP_TRY(ci.alloc((size_t)nnz));
    SPMV_HIP_TRY(va.alloc((size_t)nnz));
    if (keep_map) SPMV_HIP_TRY(map.alloc((size_t)nnz));
    const PermArgs args{rows, cols, (uint32_t)nnz, a.d_row_ptr, a.d_col_idx, (const uint32_t *)a.d_vals, row_perm, inv_col, rp.get(), ci.get(),
                        (uint32_t *)va.get(), keep_map ? map.get() : nullptr};
    if (rows > 0 && nnz > 0) {
        hipLaunchKernelGGL(k_perm_rank<kPermSmall>, dim3(perm_blocks(rows * kPermSmall)), dim3(kBlock), 0, s, args, 0);
        if (int rc = check_launch("k_perm_rank<8>")) return rc;
        if (st[kPsMid] > 0) {
            hipLaunchKernelGGL(k_perm_rank<kWave>, dim3(perm_blocks(rows * kWave)), dim3(kBlock), 0, s, args, kPermSmall);
            if (int rc = check_launch("k_perm_rank<64>")) return rc;
        }
        const int64_t n_long = st[kPsLong] < 0 ? 0 : (st[kPsLong] > rows ? rows : st[kPsLong]);
        if (n_long > 0) {
            hipLaunchKernelGGL(k_perm_bitonic, dim3((unsigned)n_long), dim3(kBlock), 0, s, args, (const int32_t *)longs.get(), (int32_t)n_long);
            if (int rc = check_launch("k_perm_bitonic")) return rc;
        }
    }
    SPMV_HIP_TRY(hipStreamSynchronize(s));   // the temporaries are freed on return
    return perm_finish(a, rp, ci, va, map, keep_map, out);
}

}  // namespace

int permute(const spmv_csr &a, const int32_t *row_perm, const int32_t *col_perm, bool keep_map, bool via_transpose, hipStream_t s, spmv_csr_t **out)
{
    const int64_t rows = a.rows, cols = a.cols;
    DevPtr<int32_t> inv_row, inv_col, d_bad;
    int32_t bad[2] = {INT32_MAX, INT32_MAX};
    SPMV_HIP_TRY(d_bad.alloc(2));
    SPMV_HIP_TRY(hipMemcpyAsync(d_bad.get(), bad, sizeof bad, hipMemcpyHostToDevice, s));
    if (row_perm)
        if (int rc = perm_inverse(row_perm, rows, inv_row, d_bad.get(), s)) return rc;
    if (col_perm)
        if (int rc = perm_inverse(col_perm, cols, inv_col, d_bad.get() + 1, s)) return rc;
    SPMV_HIP_TRY(hipMemcpyAsync(bad, d_bad.get(), sizeof bad, hipMemcpyDeviceToHost, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    for (int side = 0; side < 2; ++side) {
        if (bad[side] == INT32_MAX) continue;
        set_error("spmv_csr_permute: %s is no permutation of 0 .. %lld: the entry at index %d is out of range or repeats an earlier one",
                  side ? "d_col_perm" : "d_row_perm", (long long)((side ? cols : rows) - 1), bad[side]);
        return SPMV_ERR_INVALID;
    }
    const int32_t *irow = row_perm ? inv_row.get() : nullptr, *icol = col_perm ? inv_col.get() : nullptr;
    if (!via_transpose) {
        int64_t longest = 0;
        spmv_csr_t *b = nullptr;
        if (int rc = permute_direct(a, row_perm, icol, keep_map, s, &b, &longest)) return rc;
        if (b) { *out = b; return SPMV_OK; }
    }
    return permute_via_transpose(a, irow, icol, keep_map, s, out);
}

int permute_vector(const int32_t *perm, int64_t n, bool inverse, const float *src, float *dst, hipStream_t s)
{
    if (n <= 0) return SPMV_OK;
    hipLaunchKernelGGL(k_perm_vector, dim3(perm_blocks(n)), dim3(kBlock), 0, s, n, perm, inverse, (const uint32_t *)src, (uint32_t *)dst);
    return check_launch("k_perm_vector");
}

}  // namespace spmv
