// kernels_color.hip -- spmv_csr_color (include/spmv_hip.h "the multicolour ordering"): the greedy colouring of the symmetrised
// pattern of a square handle in descending key order (Jones-Plassmann), key(i) = fmix32(i ^ seed).  color[i] is the smallest
// colour that no neighbour of a higher key has; a row can take its colour as soon as those neighbours have theirs, so the rows
// colour in rounds: round(i) = 1 + the largest round among the neighbours of a higher key.
//
//   1. the other direction of the graph: transpose(a) (kernels_transpose.hip); a row's neighbours are its entries in both.
//   2. the rounds.  rnd[i] = 0 while row i is uncoloured, else the round that coloured it.  Round R visits the list of the
//      uncoloured rows.  A neighbour j of a higher key counts as coloured only when 1 <= rnd[j] < R: then an EARLIER round wrote
//      color[j] and rnd[j], before a kernel boundary or before a workgroup barrier.  A row that finds all of them coloured
//      writes color[i], then rnd[i] = R; rnd[j] == R, read while its writer runs, counts as uncoloured, so which rows a round
//      colours does not depend on timing.  Every other row is appended to the next list: the one atomic, an integer counter
//      that decides the row's place in a list whose order reaches no output.
//      k_color_round   a grid over the list, 64 consecutive entries per wavefront: a lane per row of at most
//                      SPMV_COLOR_SERIAL_MAX neighbour entries, then the wavefront together for each longer row among them
//                      (lanes stride over the entries, the mask of forbidden colours is OR-combined across the lanes).
//      k_color_small   the same for a list of at most kBlock rows: ONE workgroup runs round after round with __syncthreads()
//                      between them, kColorRoundsMax at the most, the list in LDS.
//      The mask holds the 64 colours from `base` on; when all 64 are taken the window moves up by 64 and the row is scanned
//      again, entries / 64 + 1 times at the most (a row has no more forbidden colours than entries).
//   3. perm / color_ptr: the transpose of the rows x colours pattern with the one entry (i, color[i]) per row -- the library's
//      stable sort, as kernels_trsv.hip orders the rows by level.
//
// No flag, no spin, no grid barrier, no cooperative launch.  Positions are unsigned 32-bit (nnz < 2^31).  Every access is
// predicated on its array's own length: a handle that was never validated gives an unspecified colouring or a refusal inside
// the arrays, and every loop ends.
#include <climits>
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

constexpr int kColorRoundsMax = 1024;      // rounds one k_color_small launch runs at the most
enum { kCsNext = 0, kCsRounds = 1, kCsWords = 8 };   // the words of the loop's state: the next list's size, the rounds a small launch ran

struct ColorRow { uint32_t lo, hi; };

__device__ __forceinline__ ColorRow color_row(const int32_t *rp, int64_t row, uint32_t nnz)
{
    const uint32_t hi = min((uint32_t)rp[row + 1], nnz), lo = min((uint32_t)rp[row], hi);
    return ColorRow{lo, hi};
}

__host__ __device__ __forceinline__ uint32_t color_key(uint32_t i, uint32_t seed)
{
    uint32_t h = i ^ seed;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

struct ColorArgs {
    int64_t rows;
    uint32_t nnz, tnnz, seed;
    const int32_t *rp, *ci;       // a
    const int32_t *trp, *tci;     // its transpose
    int32_t *color, *rnd;         // (read while other rows write theirs: never __restrict__)
};

// entry e of row i's neighbour list (a's row, then the transpose's): the mask bit it forbids in the window from `base`, or
// `blocked` where it is a neighbour of a higher key that no earlier round coloured
__device__ __forceinline__ void color_visit(const ColorArgs &a, int j, int i, uint32_t ki, int32_t round, int32_t base, uint64_t &mask, bool &blocked)
{
    if (j == i || j < 0 || (int64_t)j >= a.rows) return;
    if (color_key((uint32_t)j, a.seed) <= ki) return;
    const int32_t r = __atomic_load_n(&a.rnd[j], __ATOMIC_RELAXED);
    if (r < 1 || r >= round) { blocked = true; return; }
    const int64_t d = (int64_t)__atomic_load_n(&a.color[j], __ATOMIC_RELAXED) - base;
    if (d >= 0 && d < 64) mask |= 1ull << d;
}

__device__ __forceinline__ void color_take(const ColorArgs &a, int i, int32_t c, int32_t round)
{
    __atomic_store_n(&a.color[i], c, __ATOMIC_RELAXED);
    __atomic_store_n(&a.rnd[i], round, __ATOMIC_RELAXED);
}

// The rows at positions base + lane < end of the list (list null: the row is its position).  append(row) takes a row that
// stays uncoloured.  Every lane of the wavefront comes here together.
template <class Append>
__device__ __forceinline__ void color_wave(const ColorArgs &a, const int32_t *list, int64_t base, int64_t end, int lane, int32_t round,
                                           const Append &append)
{
    const int64_t pos = base + lane;
    const int row = pos < end ? (list ? list[pos] : (int)pos) : -1;
    const bool have = row >= 0 && (int64_t)row < a.rows;
    ColorRow ra{0, 0}, rt{0, 0};
    if (have) {
        ra = color_row(a.rp, row, a.nnz);
        rt = color_row(a.trp, row, a.tnnz);
    }
    const uint64_t len = (uint64_t)(ra.hi - ra.lo) + (rt.hi - rt.lo);
    const bool is_long = have && len > SPMV_COLOR_SERIAL_MAX;
    if (have && !is_long) {
        const uint32_t ki = color_key((uint32_t)row, a.seed);
        uint64_t mask = 0;
        bool blocked = false;
        for (uint32_t s = ra.lo; s < ra.hi && !blocked; ++s) color_visit(a, a.ci[s], row, ki, round, 0, mask, blocked);
        for (uint32_t s = rt.lo; s < rt.hi && !blocked; ++s) color_visit(a, a.tci[s], row, ki, round, 0, mask, blocked);
        // (at most SPMV_COLOR_SERIAL_MAX < 64 forbidden colours: the first window has a free one)
        if (!blocked && mask != ~0ull) color_take(a, row, (int32_t)__ffsll((unsigned long long)~mask) - 1, round);
        else append(row);
    }
    for (uint64_t m = __ballot(is_long); m != 0; m &= m - 1) {
        const int src = __ffsll((unsigned long long)m) - 1;
        const int lrow = __shfl(row, src);
        const uint32_t a0 = (uint32_t)__shfl((int)ra.lo, src), a1 = (uint32_t)__shfl((int)ra.hi, src);
        const uint32_t t0 = (uint32_t)__shfl((int)rt.lo, src), t1 = (uint32_t)__shfl((int)rt.hi, src);
        const uint64_t na = a1 - a0, n = na + (t1 - t0);
        const uint32_t ki = color_key((uint32_t)lrow, a.seed);
        const uint64_t passes = n / 64 + 1;
        int32_t got = -1;
        bool stuck = false;
        for (uint64_t pass = 0; pass < passes; ++pass) {
            const int32_t window = (int32_t)(pass * 64);
            uint64_t mask = 0;
            bool blocked = false;
            for (uint64_t e = (uint64_t)lane; e < n; e += kWave) {
                const int j = e < na ? a.ci[a0 + (uint32_t)e] : a.tci[t0 + (uint32_t)(e - na)];
                color_visit(a, j, lrow, ki, round, window, mask, blocked);
            }
            if (__ballot(blocked) != 0) { stuck = true; break; }             // (the same word for every lane)
            uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
#pragma unroll
            for (int w = kWave / 2; w >= 1; w >>= 1) {                         // lanes l < w: mask[l] |= mask[l + w]
                mlo |= (uint32_t)__shfl_down((int)mlo, w);
                mhi |= (uint32_t)__shfl_down((int)mhi, w);
            }
            const uint64_t all = ((uint64_t)(uint32_t)__shfl((int)mhi, 0) << 32) | (uint32_t)__shfl((int)mlo, 0);
            if (all != ~0ull) { got = window + (int32_t)__ffsll((unsigned long long)~all) - 1; break; }
        }
        if (lane == 0) {
            if (!stuck && got >= 0) color_take(a, lrow, got, round);
            else append(lrow);
        }
    }
}

// one round over a list of n rows: a wavefront per 64 of them
__global__ __launch_bounds__(kBlock) void k_color_round(ColorArgs a, const int32_t *__restrict__ list, int64_t n, int32_t round,
                                                        int32_t *__restrict__ next, int32_t *__restrict__ n_next)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int64_t base = (int64_t)blockIdx.x * kBlock + (threadIdx.x - (unsigned)lane);
    if (base >= n) return;                                 // (a whole wavefront)
    color_wave(a, list, base, n, lane, round, [&](int i) {
        const int32_t at = atomicAdd(n_next, 1);
        if (at >= 0 && (int64_t)at < a.rows) next[at] = i;
    });
}

// One workgroup: the list of n <= kBlock rows (null: the rows 0 .. n - 1), round after round from `round0` while rows are left,
// kColorRoundsMax rounds at the most.  Leaves what is left in `list` (when there is one) and in st its size and the rounds run.
__global__ __launch_bounds__(kBlock) void k_color_small(ColorArgs a, int32_t *list, int32_t n, int32_t round0, int32_t *__restrict__ st)
{
    __shared__ int32_t s_list[2][kBlock];
    __shared__ int32_t s_n[2];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
    if (n > kBlock) n = kBlock;
    if (tid < n) s_list[0][tid] = list ? list[tid] : tid;
    if (tid == 0) { s_n[0] = n; s_n[1] = 0; }
    __syncthreads();
    int w = 0, rounds = 0;
    for (int it = 0; it < kColorRoundsMax; ++it) {
        const int m = s_n[w];
        if (m < 1 || m > kBlock) break;                    // (the same word for every work-item: they leave together)
        color_wave(a, s_list[w], (int64_t)(tid - lane), (int64_t)m, lane, round0 + it, [&](int i) {
            const int32_t at = atomicAdd(&s_n[w ^ 1], 1);
            if (at >= 0 && at < kBlock) s_list[w ^ 1][at] = i;
        });
        __syncthreads();
        if (tid == 0) s_n[w] = 0;                          // the round after the next appends here
        ++rounds;
        w ^= 1;
        __syncthreads();
    }
    const int left = min(max(s_n[w], 0), kBlock);
    if (list && tid < left) list[tid] = s_list[w][tid];
    if (tid == 0) {
        st[kCsNext] = left;
        st[kCsRounds] = rounds;
    }
}

__global__ __launch_bounds__(kBlock) void k_color_iota(int64_t n, int32_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

unsigned color_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int color_fail(const char *msg)
{
    set_error("spmv_csr_color: %s", msg);
    return SPMV_ERR_INVALID;
}

// what transpose() holds at its peak for a matrix of nnz entries and tcols rows of the result, the result included
int64_t color_transpose_peak(int64_t nnz, int64_t trows)
{
    const int64_t tiles = (nnz + 4095) / 4096;
    return 4 * (trows + 1) + 8 * nnz + 16 * nnz + 1024 * tiles + 16;
}

}  // namespace

int color(const spmv_csr &a, uint32_t seed, hipStream_t s, int32_t *d_color, int32_t *d_perm, int32_t *color_ptr, int cap, int64_t info[8])
{
    const int64_t rows = a.rows;
    int64_t colors = 0, rounds = 0, launches = 0, largest = 0, smallest = 0, peak = 0;
    if (rows > 0) {
        spmv_csr_t *tr = nullptr;
        if (int rc = transpose(a, false, s, &tr)) return rc;
        peak = color_transpose_peak(a.nnz, a.cols);
        const int64_t at_bytes = 4 * (rows + 1) + 8 * a.nnz;
        int rc = SPMV_OK;
        {
            DevPtr<int32_t> rnd, fr[2], d_st;
            hipError_t e = rnd.alloc((size_t)rows);
            if (e == hipSuccess) e = fr[0].alloc((size_t)rows);
            if (e == hipSuccess) e = fr[1].alloc((size_t)rows);
            if (e == hipSuccess) e = d_st.alloc(kCsWords);
            if (e == hipSuccess) e = hipMemsetAsync(rnd.get(), 0, sizeof(int32_t) * (size_t)rows, s);
            if (e == hipSuccess) e = hipMemsetAsync(d_st.get(), 0, sizeof(int32_t) * kCsWords, s);
            if (at_bytes + 12 * rows + 32 > peak) peak = at_bytes + 12 * rows + 32;
            const ColorArgs args{rows, (uint32_t)a.nnz, (uint32_t)tr->nnz, seed, a.d_row_ptr, a.d_col_idx, tr->d_row_ptr, tr->d_col_idx, d_color, rnd.get()};
            // every trip colours at least the row of the largest key that is left, so there are `rows` trips at the most
            int cur = -1;                                  // the buffer of the list; -1: the rows themselves
            int64_t n = rows;
            int32_t st[kCsWords] = {};
            for (int64_t trip = 0; rc == SPMV_OK && e == hipSuccess && n > 0 && trip < rows; ++trip) {
                const int64_t before = n;
                int32_t *list = cur < 0 ? nullptr : fr[cur].get();
                if (n <= kBlock) {
                    hipLaunchKernelGGL(k_color_small, dim3(1), dim3(kBlock), 0, s, args, list, (int32_t)n, (int32_t)(rounds + 1), d_st.get());
                    rc = check_launch("k_color_small");
                    if (rc == SPMV_OK) e = hipMemcpyAsync(st, d_st.get(), sizeof st, hipMemcpyDeviceToHost, s);
                    if (rc == SPMV_OK && e == hipSuccess) e = hipStreamSynchronize(s);
                    if (rc == SPMV_OK && e == hipSuccess) {
                        rounds += st[kCsRounds];
                        n = st[kCsNext];
                        if (n > 0 && !list) rc = color_fail("rows are left that no list holds");      // (kColorRoundsMax rounds of kBlock rows at the most colour them all)
                    }
                } else {
                    const int nxt = cur < 0 ? 0 : cur ^ 1;
                    e = hipMemsetAsync(d_st.get() + kCsNext, 0, sizeof(int32_t), s);
                    if (e == hipSuccess) {
                        hipLaunchKernelGGL(k_color_round, dim3(color_blocks(n)), dim3(kBlock), 0, s, args, (const int32_t *)list, n,
                                           (int32_t)(rounds + 1), fr[nxt].get(), d_st.get() + kCsNext);
                        rc = check_launch("k_color_round");
                    }
                    if (rc == SPMV_OK && e == hipSuccess) e = hipMemcpyAsync(st, d_st.get(), sizeof(int32_t), hipMemcpyDeviceToHost, s);
                    if (rc == SPMV_OK && e == hipSuccess) e = hipStreamSynchronize(s);
                    if (rc == SPMV_OK && e == hipSuccess) {
                        rounds += 1;
                        n = st[kCsNext];
                        cur = nxt;
                    }
                }
                ++launches;
                if (rc == SPMV_OK && e == hipSuccess && (n < 0 || n >= before)) rc = color_fail("a round coloured no row (the arrays are not a valid CSR)");
            }
            if (rc == SPMV_OK && e != hipSuccess) rc = hip_fail(e, "spmv_csr_color: the rounds", __FILE__, __LINE__);
            if (rc == SPMV_OK && n != 0) rc = color_fail("rows are left uncoloured");
        }
        (void)spmv_csr_destroy(tr);
        if (rc) return rc;

        // perm / color_ptr: the stable sort of the rows by colour, as the transpose of a rows x colours pattern
        DevPtr<int32_t> iota, range;
        DevPtr<float> zeros;
        SPMV_HIP_TRY(iota.alloc((size_t)rows + 1));
        SPMV_HIP_TRY(zeros.alloc((size_t)rows));
        SPMV_HIP_TRY(range.alloc(2));
        SPMV_HIP_TRY(hipMemsetAsync(zeros.get(), 0, sizeof(float) * (size_t)rows, s));
        hipLaunchKernelGGL(k_color_iota, dim3(color_blocks(rows + 1)), dim3(kBlock), 0, s, rows + 1, iota.get());
        if (int rc2 = check_launch("k_color_iota")) return rc2;
        spmv_csr by_color;
        by_color.rows = rows; by_color.cols = rows; by_color.nnz = rows; by_color.device = a.device;
        by_color.d_row_ptr = iota; by_color.d_col_idx = d_color; by_color.d_vals = zeros;
        if (int rc2 = launch_column_range(by_color, range.get(), s)) return rc2;
        int32_t r2[2] = {0, -1};
        SPMV_HIP_TRY(hipMemcpyAsync(r2, range.get(), sizeof r2, hipMemcpyDeviceToHost, s));
        SPMV_HIP_TRY(hipStreamSynchronize(s));
        if (r2[0] < 0 || r2[1] < 0 || (int64_t)r2[1] >= rows) return color_fail("a colour outside [0, rows)");
        colors = (int64_t)r2[1] + 1;
        by_color.cols = colors;
        spmv_csr_t *sorted = nullptr;
        if (int rc2 = transpose(by_color, false, s, &sorted)) return rc2;
        if (8 * rows + 4 + color_transpose_peak(rows, colors) > peak) peak = 8 * rows + 4 + color_transpose_peak(rows, colors);
        int32_t *cp = new (std::nothrow) int32_t[(size_t)colors + 1];
        int rc3 = SPMV_OK;
        if (!cp || sorted->rows != colors || sorted->nnz != rows) rc3 = color_fail("the rows did not sort by colour");
        if (rc3 == SPMV_OK && hipMemcpyAsync(cp, sorted->d_row_ptr, sizeof(int32_t) * ((size_t)colors + 1), hipMemcpyDeviceToHost, s) != hipSuccess) rc3 = SPMV_ERR_HIP;
        if (rc3 == SPMV_OK && d_perm &&
            hipMemcpyAsync(d_perm, sorted->d_col_idx, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToDevice, s) != hipSuccess) rc3 = SPMV_ERR_HIP;
        if (rc3 == SPMV_OK && hipStreamSynchronize(s) != hipSuccess) rc3 = SPMV_ERR_HIP;
        (void)spmv_csr_destroy(sorted);
        if (rc3 == SPMV_ERR_HIP) set_error("spmv_csr_color: a copy of the sorted rows failed");
        if (rc3 == SPMV_OK && (cp[0] != 0 || (int64_t)cp[colors] != rows)) rc3 = color_fail("the colours do not cover the rows");
        if (rc3 == SPMV_OK) {
            smallest = rows;
            for (int64_t c = 0; c < colors; ++c) {
                const int64_t m = (int64_t)cp[c + 1] - cp[c];
                if (m > largest) largest = m;
                if (m < smallest) smallest = m;
            }
            if (color_ptr)
                for (int64_t c = 0; c <= colors && c < (int64_t)cap; ++c) color_ptr[c] = cp[c];
        }
        delete[] cp;
        if (rc3) return rc3;
    } else if (color_ptr && cap > 0) {
        color_ptr[0] = 0;
    }
    if (info) {
        const int64_t v[8] = {colors, rounds, launches, largest, smallest, rows > 0 ? 2 * a.nnz : 0, peak, 0};
        for (int i = 0; i < 8; ++i) info[i] = v[i];
    }
    return SPMV_OK;
}

}  // namespace spmv
