// kernels_spgemm.hip -- spmv_csr_spgemm / spmv_csr_spgemm_values (include/spmv_hip.h "the sparse product"): C = A B for two
// CSR handles as a new handle that owns its arrays.  The pattern is structural and every row of C sorted and duplicate-free;
// the value of entry (i, j) is one fma chain over its terms in ascending (storage position s of A's row, storage position q
// of B's row).  Nothing here depends on the order in which anything arrives: there is no hash table and no compare-and-swap
// at all -- a row's distinct columns come out of a sort --, the only atomic is an integer LDS add whose result is not used,
// and no float atomic.
//
// A row of A has a product BOUND, the sum of the lengths of the rows of B it refers to (its number of terms; 64-bit).  The
// host reads the bounds back once (8 bytes per row of A, no pass over the nonzeros) and sorts the rows into classes:
// bound 0 (nothing to do), bound <= kSpgSlots[c] (SPMV_SPGEMM_CLASS_SLOTS: the smallest such c), and oversized.
//
//   1. k_spg_bound      a lane per row of A: the bound
//   2. k_spg_sym<T>     a wavefront per row of class T: the columns of all its terms into T words of LDS, a bitonic sort
//                       of the next power of two, the distinct ones counted (WRITE = false) or stored to C (WRITE = true)
//      k_spg_big_sort   a workgroup of 1024 per oversized row: the same in a scratch of pow2 >= bound words of global
//      k_spg_big_write  memory, which stays sorted for the pass that stores the distinct columns
//   3. k_spg_total + scan_offsets_i32: the total as a 64-bit number (refused from 2^31 on), then C's row_ptr
//   4. k_spg_num<W>     a wavefront per row (the first call and spmv_csr_spgemm_values alike): a window of W consecutive
//                       entries of C's sorted row staged in LDS beside W sums; the wavefront walks s in order and inside
//                       it q in order, 64 terms a step; a term finds its entry by bisection.  The lanes of a step touch
//                       distinct entries unless B's row repeats a column: a tag per entry (hashed into 256 words) tells,
//                       and only then the lanes of the step add one after the other in lane order.  A row of more than W
//                       entries takes ceil(D / W) windows, each a walk over all its terms (classes above 4096 and
//                       oversized rows: W = 16384, the windows dealt over 32 wavefronts).
//
// Positions are unsigned 32-bit (nnz < 2^31), scratch offsets 64-bit.  Every access is predicated on its array's own
// length: nothing here relies on slack behind an array.
#include <climits>
#include <memory>
#include <new>
#include "spmv_internal.hpp"

#ifndef SPG_DYNAMIC_LDS
#define SPG_DYNAMIC_LDS(name) extern __shared__ int name[]
#endif

namespace spmv {

namespace {

constexpr int kSpgClasses = 4;
constexpr int kSpgSlots[kSpgClasses] = {SPMV_SPGEMM_CLASS_SLOTS};
constexpr int kSpgWindow = 16384;               // entries of C a wavefront holds at once for the rows beyond class 4096
constexpr int kSpgWindowSplit = 32;             // ... whose windows are dealt over this many wavefronts (blockIdx.y)
constexpr int kSpgBigBlock = 1024;              // work-items of the workgroup that sorts an oversized row in global memory
constexpr int kSpgTags = 256;                   // words of a wavefront's collision tags
constexpr int kSpgPad = INT_MAX;                // sorts behind every column (a column is at most 2^31 - 2)
constexpr int64_t kSpgBigMax = (int64_t)1 << 30;   // the largest bound of an oversized row (its scratch is indexed in 32 bits)
static_assert(kSpgSlots[0] == 64 && kSpgSlots[1] == 512 && kSpgSlots[2] == 4096 && kSpgSlots[3] == 32768,
              "the launch table below is written for these classes");

struct SpgOperands {
    int64_t b_rows;
    uint32_t a_nnz, b_nnz;
    const int32_t *a_rp, *a_ci;
    const float *a_va;
    const int32_t *b_rp, *b_ci;
    const float *b_va;
};

__device__ __forceinline__ int spg_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// the LDS (or global) writes of the wavefront's lanes before it are seen by its lanes after it
__device__ __forceinline__ void spg_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ __forceinline__ uint32_t spg_pow2(uint32_t n)
{
    uint32_t p = 2;
    while (p < n) p <<= 1;
    return p;
}

// Row `row` of A, by one wavefront: f(b0, bl, av) once per entry s in ascending s, with the first position and the length
// of B's row a.col_idx[s] (length 0 where the column or B's row_ptr is out of range) and a.vals[s]; all wavefront-uniform.
// The lanes load 64 entries' worth at once and hand them round.
template <bool VALS, typename F>
__device__ __forceinline__ void spg_walk(const SpgOperands &o, int64_t row, int lane, F f)
{
    const uint32_t s0 = (uint32_t)o.a_rp[row], s1 = min((uint32_t)o.a_rp[row + 1], o.a_nnz);
    for (uint32_t sb = s0; sb < s1; sb += kWave) {
        const uint32_t s = sb + (uint32_t)lane;
        uint32_t b0 = 0u;
        int bl = 0;
        float av = 0.0f;
        if (s < s1) {
            const int64_t c = o.a_ci[s];
            if (VALS) av = o.a_va[s];
            if (c >= 0 && c < o.b_rows) {
                const uint32_t lo = (uint32_t)o.b_rp[c], hi = (uint32_t)o.b_rp[c + 1];
                if (lo <= hi && hi <= o.b_nnz) {
                    b0 = lo;
                    bl = (int)(hi - lo);
                }
            }
        }
        const int n = (int)min((uint32_t)kWave, s1 - sb);
        for (int i = 0; i < n; ++i) f((uint32_t)__shfl((int)b0, i), __shfl(bl, i), VALS ? __shfl(av, i) : 0.0f);
    }
}

// ascending bitonic sort of keys[0, P), P a power of two >= 2, by `STRIDE` work-items of which I am `me`
template <int STRIDE, typename Sync>
__device__ __forceinline__ void spg_bitonic(int *keys, uint32_t P, int me, Sync sync)
{
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t p = (uint32_t)me; p < P / 2; p += STRIDE) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const int x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0)) {
                    keys[i] = y;
                    keys[l] = x;
                }
            }
            sync();
        }
}

// ---- 1. the bounds ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_spg_bound(SpgOperands o, int64_t rows, int64_t *__restrict__ bounds)
{
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    const uint32_t s0 = (uint32_t)o.a_rp[row], s1 = min((uint32_t)o.a_rp[row + 1], o.a_nnz);
    int64_t sum = 0;
    for (uint32_t s = s0; s < s1; ++s) {
        const int64_t c = o.a_ci[s];
        if (c < 0 || c >= o.b_rows) continue;
        const uint32_t lo = (uint32_t)o.b_rp[c], hi = (uint32_t)o.b_rp[c + 1];
        if (lo <= hi && hi <= o.b_nnz) sum += (int64_t)(hi - lo);
    }
    bounds[row] = sum;
}

// ---- 2. the symbolic pass, rows of a class -------------------------------------------------------------------------------
// WRITE = false: dst = the counts (row_ptr before its scan), dst[row] = distinct columns.  WRITE = true: dst = C's row_ptr.
template <int T, int WAVES, bool WRITE>
__global__ __launch_bounds__(WAVES * kWave) void k_spg_sym(SpgOperands o, const int32_t *__restrict__ list, int64_t nlist,
                                                           int32_t *__restrict__ dst, int32_t *__restrict__ c_ci, uint32_t c_nnz)
{
    SPG_DYNAMIC_LDS(lds);
    const int lane = spg_lane(), w = (int)(threadIdx.x >> 6);
    int *keys = lds + w * T;
    const int64_t item = (int64_t)blockIdx.x * WAVES + w;
    if (item >= nlist) return;                      // wavefront-uniform; the kernel has no workgroup barrier
    const int64_t row = list[item];
    uint32_t t = 0u;
    spg_walk<false>(o, row, lane, [&](uint32_t b0, int bl, float) {
        for (int q = lane; q < bl; q += kWave)
            if (t + (uint32_t)q < (uint32_t)T) keys[t + (uint32_t)q] = o.b_ci[b0 + (uint32_t)q];
        t += (uint32_t)bl;
    });
    const uint32_t bound = min(t, (uint32_t)T), P = spg_pow2(bound);
    for (uint32_t i = bound + (uint32_t)lane; i < P; i += kWave) keys[i] = kSpgPad;
    spg_wave_sync();
    spg_bitonic<kWave>(keys, P, lane, [] { spg_wave_sync(); });
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
    const uint32_t base = WRITE ? (uint32_t)dst[row] : 0u;
    int cnt = 0, prev_last = -1;                    // (no column is negative)
    for (uint32_t i0 = 0; i0 < bound; i0 += kWave) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool ok = i < bound;
        const int v = ok ? keys[i] : kSpgPad;
        const int pv = (ok && lane > 0) ? keys[i - 1] : prev_last;
        const bool first = ok && v != pv;
        const uint64_t bal = __ballot(first);
        if (WRITE) {
            const uint32_t d = base + (uint32_t)cnt + (uint32_t)__popcll(bal & below);
            if (first && d < c_nnz) c_ci[d] = v;
        }
        cnt += (int)__popcll(bal);
        prev_last = __shfl(v, kWave - 1);
    }
    if (!WRITE && lane == 0) dst[row] = cnt;
}

// ---- 2'. the symbolic pass, oversized rows: a workgroup of 1024 per row, the sort in global memory --------------------------
// off[i] .. off[i + 1]: row list[i]'s power-of-two words of the scratch
__global__ __launch_bounds__(kSpgBigBlock) void k_spg_big_sort(SpgOperands o, const int32_t *__restrict__ list, const int64_t *__restrict__ off,
                                                         int32_t *__restrict__ scratch, int32_t *__restrict__ counts)
{
    __shared__ int s_cnt;
    const int tid = (int)threadIdx.x, lane = spg_lane();
    const int64_t row = list[blockIdx.x];
    int32_t *scr = scratch + off[blockIdx.x];
    const uint32_t P = (uint32_t)(off[blockIdx.x + 1] - off[blockIdx.x]);
    if (tid == 0) s_cnt = 0;
    uint64_t t = 0;
    spg_walk<false>(o, row, lane, [&](uint32_t b0, int bl, float) {
        for (int q = tid; q < bl; q += kSpgBigBlock)
            if (t + (uint64_t)q < P) scr[t + (uint64_t)q] = o.b_ci[b0 + (uint32_t)q];
        t += (uint64_t)bl;
    });
    for (uint64_t i = t + (uint64_t)tid; i < P; i += kSpgBigBlock) scr[i] = kSpgPad;
    __syncthreads();
    spg_bitonic<kSpgBigBlock>(scr, P, tid, [] { __syncthreads(); });
    int local = 0;
    for (uint32_t i = (uint32_t)tid; i < P; i += kSpgBigBlock) {
        const int v = scr[i];
        if (v != kSpgPad && (i == 0 || scr[i - 1] != v)) ++local;
    }
    if (local) atomicAdd(&s_cnt, local);            // (an integer sum; the result of the atomic is not used)
    __syncthreads();
    if (tid == 0) counts[row] = s_cnt;
}

__global__ __launch_bounds__(kSpgBigBlock) void k_spg_big_write(const int32_t *__restrict__ list, const int64_t *__restrict__ off,
                                                          const int32_t *__restrict__ scratch, const int32_t *__restrict__ c_rp,
                                                          int32_t *__restrict__ c_ci, uint32_t c_nnz)
{
    constexpr int kWaves = kSpgBigBlock / kWave;
    __shared__ int s_first[2][kWaves];
    const int tid = (int)threadIdx.x, lane = spg_lane(), w = tid >> 6;
    const int64_t row = list[blockIdx.x];
    const int32_t *scr = scratch + off[blockIdx.x];
    const uint32_t P = (uint32_t)(off[blockIdx.x + 1] - off[blockIdx.x]);
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
    const uint32_t base = (uint32_t)c_rp[row];
    uint32_t run = 0u;
    int par = 0;
    for (uint32_t i0 = 0; i0 < P; i0 += kSpgBigBlock, par ^= 1) {
        const uint32_t i = i0 + (uint32_t)tid;
        const int v = i < P ? scr[i] : kSpgPad;
        const bool first = v != kSpgPad && (i == 0 || scr[i - 1] != v);
        const uint64_t bal = __ballot(first);
        if (lane == 0) s_first[par][w] = (int)__popcll(bal);
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
            const uint32_t n = (uint32_t)s_first[par][q];
            if (q < w) before += n;
            all += n;
        }
        const uint32_t d = base + run + before + (uint32_t)__popcll(bal & below);
        if (first && d < c_nnz) c_ci[d] = v;
        run += all;
        // (the next step writes the other half of s_first, and the one after it comes a barrier later)
    }
}

// ---- 3. the total of the counts as a 64-bit number ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_spg_total(const int32_t *__restrict__ counts, int64_t rows, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s_sum[kBlock];
    const int tid = (int)threadIdx.x;
    unsigned long long sum = 0ull;
    for (int64_t r = tid; r < rows; r += kBlock) sum += (unsigned long long)(uint32_t)counts[r];
    s_sum[tid] = sum;
    __syncthreads();
    for (int o = kBlock / 2; o >= 1; o >>= 1) {
        if (tid < o) s_sum[tid] += s_sum[tid + o];
        __syncthreads();
    }
    if (tid == 0) *total = s_sum[0];
}

// ---- 4. the numeric pass ------------------------------------------------------------------------------------------------------
// which lanes of the step hold an entry that NO other lane of the step holds (the scheme of lone_in_step, spmv_internal.hpp:
// two entries in one of the 256 tag words both count as shared -- conservative, never wrong)
__device__ __forceinline__ bool spg_lone(int *tags, bool valid, int key, int lane)
{
    int *tag = tags + (key & (kSpgTags - 1));
    int first = lane, second = kWave;
    if (valid) __hip_atomic_store(tag, lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    spg_wave_sync();
    if (valid) first = __hip_atomic_load(tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    spg_wave_sync();
    if (valid && first != lane) __hip_atomic_store(tag, kWave, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    spg_wave_sync();
    if (valid) second = __hip_atomic_load(tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    spg_wave_sync();
    return valid && second == lane;
}

template <int W, int WAVES>
__global__ __launch_bounds__(WAVES * kWave) void k_spg_num(SpgOperands o, const int32_t *__restrict__ list, int64_t nlist,
                                                           const int32_t *__restrict__ c_rp, const int32_t *__restrict__ c_ci,
                                                           float *__restrict__ c_va, uint32_t c_nnz)
{
    SPG_DYNAMIC_LDS(lds);
    const int lane = spg_lane(), w = (int)(threadIdx.x >> 6);
    int *keys = lds + w * (2 * W + kSpgTags);
    float *acc = reinterpret_cast<float *>(keys + W);
    int *tags = keys + 2 * W;
    const int64_t item = (int64_t)blockIdx.x * WAVES + w;
    if (item >= nlist) return;                      // wavefront-uniform; the kernel has no workgroup barrier
    const int64_t row = list[item];
    const uint32_t cs = (uint32_t)c_rp[row], ce = min((uint32_t)c_rp[row + 1], c_nnz);
    // (the windows of a row are independent: block y of the grid takes every gridDim.y-th of them)
    for (uint32_t w0 = cs + blockIdx.y * (uint32_t)W; w0 < ce; w0 += gridDim.y * (uint32_t)W) {
        const int n = (int)min((uint32_t)W, ce - w0);
        for (int i = lane; i < n; i += kWave) {
            keys[i] = c_ci[w0 + (uint32_t)i];
            acc[i] = 0.0f;
        }
        spg_wave_sync();
        const int key_lo = keys[0], key_hi = keys[n - 1];
        spg_walk<true>(o, row, lane, [&](uint32_t b0, int bl, float av) {
            for (int q0 = 0; q0 < bl; q0 += kWave) {
                const int q = q0 + lane;
                const bool ok = q < bl;
                const int j = ok ? o.b_ci[b0 + (uint32_t)q] : 0;
                const float bv = ok ? o.b_va[b0 + (uint32_t)q] : 0.0f;
                const bool in = ok && j >= key_lo && j <= key_hi;
                if (__ballot(in) == 0) continue;
                // the first entry of the window that is not below j
                int lo = 0, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (keys[mid] < j) lo = mid + 1;
                    else hi = mid;
                }
                const bool hit = in && lo < n && keys[lo] == j;
                const bool lone = spg_lone(tags, hit, lo, lane);
                if (__ballot(hit && !lone) == 0) {
                    if (hit) acc[lo] = __builtin_fmaf(av, bv, acc[lo]);
                } else {
                    // B's row repeats a column inside this step (or two entries share a tag word): in lane order
                    for (uint64_t m = __ballot(hit); m != 0; m &= m - 1) {
                        if (lane == __builtin_ctzll(m)) acc[lo] = __builtin_fmaf(av, bv, acc[lo]);
                        spg_wave_sync();
                    }
                }
                spg_wave_sync();
            }
        });
        for (int i = lane; i < n; i += kWave) c_va[w0 + (uint32_t)i] = acc[i];
        spg_wave_sync();
    }
}

template <int T, int WAVES, bool WRITE>
int spg_launch_sym(int device, const SpgOperands &o, const int32_t *list, int64_t nlist, int32_t *dst, int32_t *c_ci, uint32_t c_nnz,
                   hipStream_t s)
{
    if (nlist <= 0) return SPMV_OK;
    const size_t lds = sizeof(int) * (size_t)T * WAVES;
    static LdsOptIn optin;
    if (int rc = optin.ensure(reinterpret_cast<const void *>(&k_spg_sym<T, WAVES, WRITE>), device, (int)lds)) return rc;
    hipLaunchKernelGGL((k_spg_sym<T, WAVES, WRITE>), dim3((unsigned)((nlist + WAVES - 1) / WAVES)), dim3(WAVES * kWave), lds, s, o, list,
                       nlist, dst, c_ci, c_nnz);
    return check_launch("k_spg_sym");
}

template <bool WRITE>
int spg_sym_classes(int device, const SpgOperands &o, const int32_t *order, const int64_t *cls, int32_t *dst, int32_t *c_ci,
                    uint32_t c_nnz, hipStream_t s)
{
    if (int rc = spg_launch_sym<64, 4, WRITE>(device, o, order + cls[0], cls[1] - cls[0], dst, c_ci, c_nnz, s)) return rc;
    if (int rc = spg_launch_sym<512, 4, WRITE>(device, o, order + cls[1], cls[2] - cls[1], dst, c_ci, c_nnz, s)) return rc;
    if (int rc = spg_launch_sym<4096, 4, WRITE>(device, o, order + cls[2], cls[3] - cls[2], dst, c_ci, c_nnz, s)) return rc;
    return spg_launch_sym<32768, 1, WRITE>(device, o, order + cls[3], cls[4] - cls[3], dst, c_ci, c_nnz, s);
}

template <int W, int WAVES>
int spg_launch_num(int device, const SpgOperands &o, const int32_t *list, int64_t nlist, const int32_t *c_rp, const int32_t *c_ci,
                   float *c_va, uint32_t c_nnz, hipStream_t s, int split = 1)
{
    if (nlist <= 0) return SPMV_OK;
    const size_t lds = sizeof(int) * (size_t)(2 * W + kSpgTags) * WAVES;
    static LdsOptIn optin;
    if (int rc = optin.ensure(reinterpret_cast<const void *>(&k_spg_num<W, WAVES>), device, (int)lds)) return rc;
    hipLaunchKernelGGL((k_spg_num<W, WAVES>), dim3((unsigned)((nlist + WAVES - 1) / WAVES), (unsigned)split), dim3(WAVES * kWave), lds, s, o,
                       list, nlist, c_rp, c_ci, c_va, c_nnz);
    return check_launch("k_spg_num");
}

SpgOperands spg_operands(const spmv_csr &a, const spmv_csr &b)
{
    return SpgOperands{b.rows, (uint32_t)a.nnz, (uint32_t)b.nnz, a.d_row_ptr, a.d_col_idx, a.d_vals, b.d_row_ptr, b.d_col_idx, b.d_vals};
}

// the numeric pass over the plan's row lists: at most four launches, no allocation, no wait
int spg_numeric(const SpgemmPlan &p, int device, const SpgOperands &o, const int32_t *c_rp, const int32_t *c_ci, float *c_va,
                uint32_t c_nnz, hipStream_t s)
{
    const int32_t *order = p.d_order.get();
    const int64_t *cls = p.cls;
    if (int rc = spg_launch_num<64, 4>(device, o, order + cls[0], cls[1] - cls[0], c_rp, c_ci, c_va, c_nnz, s)) return rc;
    if (int rc = spg_launch_num<512, 4>(device, o, order + cls[1], cls[2] - cls[1], c_rp, c_ci, c_va, c_nnz, s)) return rc;
    if (int rc = spg_launch_num<4096, 1>(device, o, order + cls[2], cls[3] - cls[2], c_rp, c_ci, c_va, c_nnz, s)) return rc;
    // class 32768 and the oversized rows stand side by side in the list
    return spg_launch_num<kSpgWindow, 1>(device, o, order + cls[3], cls[5] - cls[3], c_rp, c_ci, c_va, c_nnz, s, kSpgWindowSplit);
}

}  // namespace

int64_t spgemm_plan_bytes(const spmv_csr &c) { return c.plan_spgemm.ready ? 4 * c.plan_spgemm.cls[kSpgClasses + 1] : 0; }

// Device memory while the call runs, beside C's own arrays (4 (a.rows + 1) + 8 nnz(C) bytes): 8 a.rows (the bounds, freed before
// C's col_idx and vals are allocated) + 4 listed (the row lists: the plan; listed = rows of A with at least one product) + 8
// (n_over + 1) + 4 sum of pow2ceil(bound) over the n_over oversized rows (their sort scratch) + 16 + what scan_offsets_i32 takes
// for a.rows counts (4 bytes per 4096 rows).
int spgemm(const spmv_csr &a, const spmv_csr &b, bool keep_plan, hipStream_t s, spmv_csr_t **out, int64_t *products)
{
    const int64_t rows = a.rows;
    const SpgOperands o = spg_operands(a, b);
    SpgemmPlan plan;
    DevPtr<int32_t> rp, ci, total32, scratch;
    DevPtr<float> va;
    DevPtr<int64_t> bounds, over_off;
    DevPtr<unsigned long long> total64;
    std::unique_ptr<int64_t[]> hb, h_off;
    std::unique_ptr<int32_t[]> h_order;
    int64_t total_products = 0, n_over = 0, scratch_words = 0;
    int64_t *cls = plan.cls;                       // cls[c] .. cls[c + 1]: the rows of class c in the list; class 4: oversized
    for (int c = 0; c <= kSpgClasses + 1; ++c) cls[c] = 0;
    SPMV_HIP_TRY(rp.alloc((size_t)rows + 1));
    SPMV_HIP_TRY(hipMemsetAsync(rp.get(), 0, sizeof(int32_t) * ((size_t)rows + 1), s));
    if (rows > 0) {
        SPMV_HIP_TRY(bounds.alloc((size_t)rows));
        hipLaunchKernelGGL(k_spg_bound, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, o, rows, bounds.get());
        if (int rc = check_launch("k_spg_bound")) return rc;
        hb.reset(new (std::nothrow) int64_t[(size_t)rows]);
        if (!hb) { set_error("spmv_csr_spgemm: out of host memory"); return SPMV_ERR_INVALID; }
        SPMV_HIP_TRY(hipMemcpyAsync(hb.get(), bounds.get(), sizeof(int64_t) * (size_t)rows, hipMemcpyDeviceToHost, s));
        SPMV_HIP_TRY(hipStreamSynchronize(s));
        SPMV_HIP_TRY(bounds.reset());
        auto class_of = [](int64_t bound) {
            for (int c = 0; c < kSpgClasses; ++c)
                if (bound <= kSpgSlots[c]) return c;
            return kSpgClasses;
        };
        int64_t count[kSpgClasses + 1] = {};
        for (int64_t r = 0; r < rows; ++r) {
            total_products += hb[r];
            if (hb[r] <= 0) continue;
            const int c = class_of(hb[r]);
            ++count[c];
            if (c == kSpgClasses && hb[r] > kSpgBigMax) {
                set_error("spmv_csr_spgemm: row %lld of a has %lld products (a row takes at most 2^30)", (long long)r, (long long)hb[r]);
                return SPMV_ERR_INVALID;
            }
        }
        for (int c = 0; c <= kSpgClasses; ++c) cls[c + 1] = cls[c] + count[c];
        const int64_t listed = cls[kSpgClasses + 1];
        n_over = count[kSpgClasses];
        h_order.reset(new (std::nothrow) int32_t[(size_t)listed + 1]);
        h_off.reset(new (std::nothrow) int64_t[(size_t)n_over + 1]);
        if (!h_order || !h_off) { set_error("spmv_csr_spgemm: out of host memory"); return SPMV_ERR_INVALID; }
        int64_t at[kSpgClasses + 1];
        for (int c = 0; c <= kSpgClasses; ++c) at[c] = cls[c];
        h_off[0] = 0;
        for (int64_t r = 0, k = 0; r < rows; ++r) {
            if (hb[r] <= 0) continue;
            const int c = class_of(hb[r]);
            h_order[at[c]++] = (int32_t)r;
            if (c == kSpgClasses) {
                h_off[k + 1] = h_off[k] + (int64_t)spg_pow2((uint32_t)hb[r]);
                ++k;
            }
        }
        scratch_words = h_off[n_over];
        SPMV_HIP_TRY(plan.d_order.alloc((size_t)listed));
        if (listed > 0)
            SPMV_HIP_TRY(hipMemcpyAsync(plan.d_order.get(), h_order.get(), sizeof(int32_t) * (size_t)listed, hipMemcpyHostToDevice, s));
        if (n_over > 0) {
            SPMV_HIP_TRY(over_off.alloc((size_t)n_over + 1));
            SPMV_HIP_TRY(hipMemcpyAsync(over_off.get(), h_off.get(), sizeof(int64_t) * ((size_t)n_over + 1), hipMemcpyHostToDevice, s));
            SPMV_HIP_TRY(scratch.alloc((size_t)scratch_words));
        }
    }
    if (products) *products = total_products;      // (a number of its own: a refusal below leaves it set)
    const int32_t *order = plan.d_order.get();
    int32_t nnz_c = 0;
    if (rows > 0) {
        if (int rc = spg_sym_classes<false>(a.device, o, order, cls, rp.get(), nullptr, 0u, s)) return rc;
        if (n_over > 0) {
            hipLaunchKernelGGL(k_spg_big_sort, dim3((unsigned)n_over), dim3(kSpgBigBlock), 0, s, o, order + cls[kSpgClasses],
                               (const int64_t *)over_off.get(), scratch.get(), rp.get());
            if (int rc = check_launch("k_spg_big_sort")) return rc;
        }
        SPMV_HIP_TRY(total64.alloc(1));
        SPMV_HIP_TRY(total32.alloc(1));
        hipLaunchKernelGGL(k_spg_total, dim3(1), dim3(kBlock), 0, s, (const int32_t *)rp.get(), rows, total64.get());
        if (int rc = check_launch("k_spg_total")) return rc;
        unsigned long long total = 0ull;
        SPMV_HIP_TRY(hipMemcpyAsync(&total, total64.get(), sizeof total, hipMemcpyDeviceToHost, s));
        SPMV_HIP_TRY(hipStreamSynchronize(s));
        if (total > (unsigned long long)INT32_MAX) {
            set_error("spmv_csr_spgemm: the product has %llu nonzeros (a handle holds fewer than 2^31)", total);
            return SPMV_ERR_INVALID;
        }
        if (int rc = scan_offsets_i32(rp.get(), rows, total32.get(), true, s, &nnz_c)) return rc;
    }
    SPMV_HIP_TRY(ci.alloc((size_t)nnz_c));
    SPMV_HIP_TRY(va.alloc((size_t)nnz_c));
    if (nnz_c > 0) {
        if (int rc = spg_sym_classes<true>(a.device, o, order, cls, rp.get(), ci.get(), (uint32_t)nnz_c, s)) return rc;
        if (n_over > 0) {
            hipLaunchKernelGGL(k_spg_big_write, dim3((unsigned)n_over), dim3(kSpgBigBlock), 0, s, order + cls[kSpgClasses],
                               (const int64_t *)over_off.get(), (const int32_t *)scratch.get(), (const int32_t *)rp.get(), ci.get(),
                               (uint32_t)nnz_c);
            if (int rc = check_launch("k_spg_big_write")) return rc;
        }
        if (int rc = spg_numeric(plan, a.device, o, rp.get(), ci.get(), va.get(), (uint32_t)nnz_c, s)) return rc;
    }
    SPMV_HIP_TRY(hipStreamSynchronize(s));         // the scratch and the host lists are freed on return

    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("spmv_csr_spgemm: out of host memory"); return SPMV_ERR_INVALID; }
    h->rows = a.rows; h->cols = b.cols; h->nnz = nnz_c;
    h->device = a.device;
    h->d_row_ptr = rp; h->d_col_idx = ci; h->d_vals = va;
    h->own_row_ptr = std::move(rp); h->own_col_idx = std::move(ci); h->own_vals = std::move(va);
    if (keep_plan) {
        plan.ready = true;
        plan.inner = a.cols;
        plan.a_nnz = a.nnz;
        plan.b_nnz = b.nnz;
        h->plan_spgemm = std::move(plan);
    }
    *out = h;
    return SPMV_OK;
}

int spgemm_values(spmv_csr &c, const spmv_csr &a, const spmv_csr &b, hipStream_t s)
{
    if (c.nnz <= 0) return SPMV_OK;
    return spg_numeric(c.plan_spgemm, c.device, spg_operands(a, b), c.d_row_ptr, c.d_col_idx, c.own_vals.get(), (uint32_t)c.nnz, s);
}

}  // namespace spmv
