// kernels_trsv.hip -- spmv_csr_trsv_plan / spmv_csr_trsv (include/spmv_hip.h "the triangular solve"): x = T^-1 b for the lower
// or the upper triangle of a square handle, LEVEL-SCHEDULED.  level[i] = 0 for a row without terms, else 1 + the largest level
// of its terms' columns; the rows of one level need only rows of earlier levels, so a level is one launch and the launches of a
// solve follow each other on one stream.  Nothing on the solve path waits for a value another workgroup writes: there is no
// flag, no atomic, no grid barrier and no cooperative launch, the only waits are kernel boundaries and __syncthreads() inside
// the one workgroup of a merged launch, and every loop bound is a kernel argument or comes from the plan's arrays.
//
// The plan (a function of the pattern alone):
//   1. k_trsv_scan     a lane per row: the diagonal's position and how often it occurs, the row's terms.  Rows without terms
//                      are the first frontier; the first row whose diagonal is missing or repeated is an integer minimum.
//   2. Kahn's peel over the dependents, which are the rows of transpose(h) (kernels_transpose.hip) restricted to the triangle:
//      k_trsv_peel        a lane per row of the frontier takes one off the term counter of every dependent; the lane that
//                         takes the last one gives the dependent its level and appends it to the next frontier.
//      k_trsv_peel_small  the same for frontiers of at most kBlock rows: ONE workgroup peels level after level with
//                         __syncthreads() between them, until a frontier is empty or larger (a bidiagonal chain does not cost
//                         one launch and one read-back per row).
//      The integer atomics decide who appends a row and where in the frontier it stands, nothing else: a frontier's ORDER
//      reaches no array of the plan, only level[] does, and level[i] is the number of the peel that emptied row i's counter.
//   3. order / level_ptr: the transpose of the rows x levels pattern with the one entry (i, level[i]) per row -- a stable sort
//      by level, so every level lists its rows ascending; its row_ptr is level_ptr and its col_idx is order.
//   4. the rows of more than SPMV_TRSV_SERIAL_MAX terms ("long"): where each one's terms are (scan_offsets_i32 of their
//      counts, k_trsv_terms: a lane per long row lists the storage positions, ascending), and bit 31 of their entry of order.
//   5. the steps, on the host from level_ptr: a level of more than thin rows is a grid launch, a run of thinner levels one
//      workgroup's, cut every SPMV_TRSV_LEVEL_CAP levels.
//
// The solve: k_trsv_level (a grid over one level) and k_trsv_levels (one workgroup over a run of levels) share trsv_wave: 64
// consecutive rows of the level's list, a lane per row for the short rows (one serial chain over the row's storage, as
// SPMV_SCALAR), then the wavefront together for each long row among them (64 strided chains over the plan's term list and the
// combine p[l] += p[l + w], w = 32 .. 1).  In a merged launch x is written to global memory and read by other wavefronts of the
// same workgroup after __syncthreads(): workgroup scope, one CU.  b and x may be the same array (row i reads b[i] before it
// writes x[i], and nobody else touches either), so neither is __restrict__.
//
// Positions are unsigned 32-bit (nnz < 2^31).  Every access is predicated on its array's own length: nothing here relies on
// slack behind an array, and a handle that was never validated gives an unspecified result or a refusal inside the arrays.
#include <climits>
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

constexpr int kPeelMax = 4096;         // levels one k_trsv_peel_small launch peels at the most
// the words of the plan builder's state
enum { kStSize0 = 0, kStSize1 = 1, kStLevels = 2, kStRetired = 3, kStCur = 4, kStBad = 5, kStLong = 6, kStWords = 8 };

struct TrsvRow { uint32_t lo, hi; };      // positions [lo, hi) of a row, hi <= nnz, lo <= hi

__device__ __forceinline__ TrsvRow trsv_row(const int32_t *rp, int64_t row, uint32_t nnz)
{
    const uint32_t hi = min((uint32_t)rp[row + 1], nnz), lo = min((uint32_t)rp[row], hi);
    return TrsvRow{lo, hi};
}

// is column c a term of row i?  (a column outside [0, rows) is none)
__device__ __forceinline__ bool trsv_term(int c, int i, bool upper, int64_t rows) { return upper ? (c > i && (int64_t)c < rows) : (c >= 0 && c < i); }

// ---- 1. the rows' diagonals and terms ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_trsv_scan(int64_t rows, uint32_t nnz, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                      bool upper, int32_t *__restrict__ diag, int32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ lcount, int32_t *__restrict__ level, int32_t *__restrict__ front,
                                                      int32_t *__restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows) return;
    const TrsvRow r = trsv_row(rp, i, nnz);
    int32_t dpos = -1, ndiag = 0, nt = 0;
    for (uint32_t s = r.lo; s < r.hi; ++s) {
        const int c = ci[s];
        if (c == (int)i) {
            if (ndiag == 0) dpos = (int32_t)s;
            ++ndiag;
        } else if (trsv_term(c, (int)i, upper, rows)) {
            ++nt;
        }
    }
    diag[i] = dpos;
    cnt[i] = nt;
    lcount[i] = nt > SPMV_TRSV_SERIAL_MAX ? nt : 0;
    level[i] = 0;
    if (ndiag != 1) atomicMin(&st[kStBad], (int32_t)i);
    if (nt > SPMV_TRSV_SERIAL_MAX) atomicAdd(&st[kStLong], 1);
    if (nt == 0) {
        const int32_t at = atomicAdd(&st[kStSize0], 1);
        if (at >= 0 && (int64_t)at < rows) front[at] = (int32_t)i;
    }
}

// ---- 2. Kahn's peel ------------------------------------------------------------------------------------------------------------
// the transpose's rows: the dependents of column c are t_ci[t_rp[c] .. t_rp[c + 1]) on the far side of the diagonal
struct TrsvDeps {
    const int32_t *rp, *ci;
    uint32_t nnz;
    int64_t rows;
    bool upper;
};

// row c leaves: one off the counter of each of its dependents; whoever empties a counter appends that row (level `lvl`)
template <class Append>
__device__ __forceinline__ void trsv_release(const TrsvDeps &t, int c, int32_t *cnt, int32_t *level, int32_t lvl, const Append &append)
{
    if (c < 0 || (int64_t)c >= t.rows) return;
    const TrsvRow r = trsv_row(t.rp, c, t.nnz);
    for (uint32_t q = r.lo; q < r.hi; ++q) {
        const int i = t.ci[q];
        if (i < 0 || (int64_t)i >= t.rows || !trsv_term(c, i, t.upper, t.rows)) continue;
        if (atomicSub(&cnt[i], 1) == 1) {
            level[i] = lvl;
            append(i);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_trsv_peel(TrsvDeps t, const int32_t *__restrict__ front, int32_t n_front, int32_t lvl,
                                                      int32_t *__restrict__ cnt, int32_t *__restrict__ level, int32_t *__restrict__ next,
                                                      int32_t *__restrict__ n_next)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)n_front) return;
    trsv_release(t, front[k], cnt, level, lvl, [&](int i) {
        const int32_t at = atomicAdd(n_next, 1);
        if (at >= 0 && (int64_t)at < t.rows) next[at] = i;
    });
}

// One workgroup: the frontier (n_front <= kBlock rows of level lvl0 - 1, in buffer `cur` of fr) and every later one while it
// holds 1 .. kBlock rows, kPeelMax peels at the most.  A small frontier lives in LDS; every frontier is also written to its
// global buffer, where the host's next launch finds the one this launch stops at.  Leaves in st: the buffer and the size of
// that frontier, the peels done and the rows they retired.
__global__ __launch_bounds__(kBlock) void k_trsv_peel_small(TrsvDeps t, int32_t *fr0, int32_t *fr1, int cur, int32_t n_front, int32_t lvl0,
                                                            int32_t *__restrict__ cnt, int32_t *__restrict__ level, int32_t *__restrict__ st)
{
    __shared__ int32_t s_front[2][kBlock];
    __shared__ int32_t s_n[2];
    const int tid = (int)threadIdx.x;
    if (n_front > kBlock) n_front = kBlock;
    if (tid < n_front) s_front[0][tid] = (cur ? fr1 : fr0)[tid];
    if (tid == 0) { s_n[0] = n_front; s_n[1] = 0; }
    __syncthreads();
    int w = 0, peels = 0, retired = 0;
    for (int it = 0; it < kPeelMax; ++it) {
        const int n = s_n[w];
        if (n < 1 || n > kBlock) break;                    // (the same word for every work-item: they leave together)
        int32_t *next = (cur ^ 1) ? fr1 : fr0;
        if (tid < n)
            trsv_release(t, s_front[w][tid], cnt, level, lvl0 + it, [&](int i) {
                const int32_t at = atomicAdd(&s_n[w ^ 1], 1);
                if (at >= 0 && at < kBlock) s_front[w ^ 1][at] = i;
                if (at >= 0 && (int64_t)at < t.rows) next[at] = i;
            });
        __syncthreads();
        if (tid == 0) s_n[w] = 0;                          // the next peel appends here
        retired += n;
        ++peels;
        cur ^= 1;
        w ^= 1;
        __syncthreads();
    }
    if (tid == 0) {
        st[kStCur] = cur;
        st[cur ? kStSize1 : kStSize0] = s_n[w];
        st[kStLevels] = peels;
        st[kStRetired] = retired;
    }
}

// ---- 3. the rows x levels pattern whose transpose sorts the rows by level -------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_trsv_iota(int64_t n, int32_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

// ---- 4. the long rows' terms, and their mark in order -----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_trsv_terms(int64_t rows, uint32_t nnz, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       bool upper, const int32_t *__restrict__ lstart, uint32_t *__restrict__ lterm,
                                                       uint32_t n_terms)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows) return;
    uint32_t t = (uint32_t)lstart[i];
    const uint32_t t1 = min((uint32_t)lstart[i + 1], n_terms);
    if (t >= t1) return;
    const TrsvRow r = trsv_row(rp, i, nnz);
    for (uint32_t s = r.lo; s < r.hi && t < t1; ++s)
        if (trsv_term(ci[s], (int)i, upper, rows)) lterm[t++] = s;
}

__global__ __launch_bounds__(kBlock) void k_trsv_mark(int64_t rows, const int32_t *__restrict__ lstart, int32_t *__restrict__ order)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= rows) return;
    const int32_t i = order[p];
    if (i >= 0 && (int64_t)i < rows && lstart[i + 1] > lstart[i]) order[p] = (int32_t)((uint32_t)i | 0x80000000u);
}

// ---- the solve -----------------------------------------------------------------------------------------------------------------------
struct TrsvArgs {
    int64_t rows;
    uint32_t nnz, n_terms;
    const int32_t *rp, *ci;
    const float *va;
    const int32_t *order, *level_ptr, *diag, *lstart;
    const uint32_t *lterm;
    const float *b;
    float *x;
    bool upper, unit;
};

// the rows at positions base + lane < end of the level's list
__device__ __forceinline__ void trsv_wave(const TrsvArgs &a, int64_t base, int64_t end, int lane)
{
    const int64_t pos = base + lane;
    const uint32_t word = pos < end ? (uint32_t)a.order[pos] : 0xffffffffu;
    const int row = (int)(word & 0x7fffffffu);
    const bool have = pos < end && (int64_t)row < a.rows;
    const bool is_long = have && (word >> 31) != 0u;
    if (have && !is_long) {
        const TrsvRow r = trsv_row(a.rp, row, a.nnz);
        float s = 0.0f, d = 1.0f;
        for (uint32_t k = r.lo; k < r.hi; ++k) {
            const int c = a.ci[k];
            if (c == row) {
                if (!a.unit) d = a.va[k];
            } else if (trsv_term(c, row, a.upper, a.rows)) {
                s = __builtin_fmaf(a.va[k], a.x[c], s);
            }
        }
        const float num = a.b[row] - s;
        a.x[row] = a.unit ? num : num / d;
    }
    for (uint64_t m = __ballot(is_long); m != 0; m &= m - 1) {
        const int src = __ffsll((unsigned long long)m) - 1;
        const int lrow = __shfl(row, src);
        const uint32_t t0 = (uint32_t)a.lstart[lrow], t1 = min((uint32_t)a.lstart[lrow + 1], a.n_terms);
        float p = 0.0f;
        for (uint64_t t = (uint64_t)t0 + (uint32_t)lane; t < t1; t += kWave) {
            const uint32_t k = a.lterm[t];
            if (k >= a.nnz) continue;
            const int c = a.ci[k];
            if (c < 0 || (int64_t)c >= a.rows) continue;
            p = __builtin_fmaf(a.va[k], a.x[c], p);
        }
#pragma unroll
        for (int w = kWave / 2; w >= 1; w >>= 1) p += __shfl_down(p, w);     // lanes l < w: p[l] += p[l + w]
        if (lane == 0) {
            float d = 1.0f;
            const int32_t dp = a.diag[lrow];
            if (!a.unit && dp >= 0 && (uint32_t)dp < a.nnz) d = a.va[dp];
            const float num = a.b[lrow] - p;
            a.x[lrow] = a.unit ? num : num / d;
        }
    }
}

// one level, positions [p0, p1) of order: a wavefront per 64 rows
__global__ __launch_bounds__(kBlock) void k_trsv_level(TrsvArgs a, int64_t p0, int64_t p1)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int64_t base = p0 + ((int64_t)blockIdx.x * kBlock + (threadIdx.x - (unsigned)lane));
    if (base >= p1) return;                                // (a whole wavefront)
    trsv_wave(a, base, p1, lane);
}

// the levels [k0, k1), one workgroup: level after level, __syncthreads() between them
__global__ __launch_bounds__(kBlock) void k_trsv_levels(TrsvArgs a, int32_t k0, int32_t k1)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int64_t first = (int64_t)(threadIdx.x - (unsigned)lane);
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t p1 = min((int64_t)(uint32_t)a.level_ptr[k + 1], a.rows), p0 = min((int64_t)(uint32_t)a.level_ptr[k], p1);
        for (int64_t base = p0 + first; base < p1; base += kBlock) trsv_wave(a, base, p1, lane);
        __syncthreads();
    }
}

unsigned trsv_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int trsv_fail(const char *msg)
{
    set_error("spmv_csr_trsv_plan: %s", msg);
    return SPMV_ERR_INVALID;
}

}  // namespace

int64_t trsv_plan_bytes(const TrsvPlan &p, int64_t rows)
{
    return p.ready ? 4 * rows + 4 * rows + 4 * (p.levels + 1) + 4 * (rows + 1) + 4 * p.long_terms : 0;
}

// Device memory while the call runs, beside the plan (see trsv_plan_bytes): the transpose of the pattern (12 nnz + 4 (rows + 1)
// bytes and, while it is made, the transpose's own temporaries), the term counters, the levels and the two frontiers (16 rows)
// and 32 bytes of state; then, the pattern's transpose freed, the rows x levels pattern (4 (rows + 1) + 4 rows, the levels
// being its columns), its transpose's values (4 rows; order and level_ptr are the plan's) and that transpose's temporaries.
int trsv_plan(spmv_csr &h, bool upper, int thin_rows, hipStream_t s)
{
    const int64_t rows = h.rows;
    const uint32_t nnz = (uint32_t)h.nnz;
    TrsvPlan p;
    p.thin = thin_rows > 0 ? thin_rows : SPMV_TRSV_THIN_DEFAULT;
    p.cap = SPMV_TRSV_LEVEL_CAP;
    SPMV_HIP_TRY(p.d_diag.alloc((size_t)rows));
    SPMV_HIP_TRY(p.d_lstart.alloc((size_t)rows + 1));
    int64_t levels = 0;
    int32_t st[kStWords] = {0, 0, 0, 0, 0, INT32_MAX, 0, 0};
    if (rows > 0) {
        DevPtr<int32_t> cnt, level, fr[2], d_st;
        SPMV_HIP_TRY(cnt.alloc((size_t)rows));
        SPMV_HIP_TRY(level.alloc((size_t)rows));
        SPMV_HIP_TRY(fr[0].alloc((size_t)rows));
        SPMV_HIP_TRY(fr[1].alloc((size_t)rows));
        SPMV_HIP_TRY(d_st.alloc(kStWords));
        SPMV_HIP_TRY(hipMemcpyAsync(d_st.get(), st, sizeof st, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_trsv_scan, dim3(trsv_blocks(rows)), dim3(kBlock), 0, s, rows, nnz, h.d_row_ptr, h.d_col_idx, upper, p.d_diag.get(),
                           cnt.get(), p.d_lstart.get(), level.get(), fr[0].get(), d_st.get());
        if (int rc = check_launch("k_trsv_scan")) return rc;
        SPMV_HIP_TRY(hipMemcpyAsync(st, d_st.get(), sizeof st, hipMemcpyDeviceToHost, s));
        SPMV_HIP_TRY(hipStreamSynchronize(s));
        p.bad_diag_row = st[kStBad] == INT32_MAX ? -1 : st[kStBad];
        p.long_rows = st[kStLong];

        spmv_csr_t *tr = nullptr;
        if (int rc = transpose(h, false, s, &tr)) return rc;
        const TrsvDeps deps{tr->d_row_ptr, tr->d_col_idx, (uint32_t)tr->nnz, rows, upper};
        // the peel: every trip of this loop retires a frontier of at least one row, so there are `rows` trips at the most
        int cur = 0;
        int64_t n_front = st[kStSize0], retired = 0;
        int rc = SPMV_OK;
        for (int64_t trip = 0; rc == SPMV_OK && n_front > 0 && retired < rows && trip < rows; ++trip) {
            if (n_front > rows) n_front = rows;
            const int64_t before = retired;
            hipError_t e = hipSuccess;
            if (n_front <= kBlock) {
                hipLaunchKernelGGL(k_trsv_peel_small, dim3(1), dim3(kBlock), 0, s, deps, fr[0].get(), fr[1].get(), cur, (int32_t)n_front,
                                   (int32_t)(levels + 1), cnt.get(), level.get(), d_st.get());
                rc = check_launch("k_trsv_peel_small");
                if (rc == SPMV_OK) e = hipMemcpyAsync(st, d_st.get(), sizeof st, hipMemcpyDeviceToHost, s);
                if (rc == SPMV_OK && e == hipSuccess) e = hipStreamSynchronize(s);
                if (rc == SPMV_OK && e == hipSuccess) {
                    cur = st[kStCur] & 1;
                    levels += st[kStLevels];
                    retired += st[kStRetired];
                    n_front = st[cur ? kStSize1 : kStSize0];
                }
            } else {
                int32_t *n_next = d_st.get() + (cur ? kStSize0 : kStSize1);
                e = hipMemsetAsync(n_next, 0, sizeof(int32_t), s);
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(k_trsv_peel, dim3(trsv_blocks(n_front)), dim3(kBlock), 0, s, deps, (const int32_t *)fr[cur].get(),
                                       (int32_t)n_front, (int32_t)(levels + 1), cnt.get(), level.get(), fr[cur ^ 1].get(), n_next);
                    rc = check_launch("k_trsv_peel");
                }
                int32_t got = 0;
                if (rc == SPMV_OK && e == hipSuccess) e = hipMemcpyAsync(&got, n_next, sizeof got, hipMemcpyDeviceToHost, s);
                if (rc == SPMV_OK && e == hipSuccess) e = hipStreamSynchronize(s);
                if (rc == SPMV_OK && e == hipSuccess) {
                    levels += 1;
                    retired += n_front;
                    n_front = got;
                    cur ^= 1;
                }
            }
            if (rc == SPMV_OK && e != hipSuccess) rc = hip_fail(e, "spmv_csr_trsv_plan: the peel", __FILE__, __LINE__);
            if (rc == SPMV_OK && retired <= before) rc = trsv_fail("a peel retired no row (the arrays are not a valid CSR)");
        }
        (void)spmv_csr_destroy(tr);
        if (rc) return rc;
        if (retired != rows || levels < 1 || levels > rows)
            return trsv_fail("the levels do not close: rows are left whose terms never resolve (the arrays are not a valid CSR)");

        // order / level_ptr: the stable sort of the rows by level, as the transpose of a rows x levels pattern
        DevPtr<int32_t> iota;
        DevPtr<float> zeros;
        SPMV_HIP_TRY(fr[0].reset());
        SPMV_HIP_TRY(fr[1].reset());
        SPMV_HIP_TRY(cnt.reset());
        SPMV_HIP_TRY(iota.alloc((size_t)rows + 1));
        SPMV_HIP_TRY(zeros.alloc((size_t)rows));
        SPMV_HIP_TRY(hipMemsetAsync(zeros.get(), 0, sizeof(float) * (size_t)rows, s));
        hipLaunchKernelGGL(k_trsv_iota, dim3(trsv_blocks(rows + 1)), dim3(kBlock), 0, s, rows + 1, iota.get());
        if (int rc2 = check_launch("k_trsv_iota")) return rc2;
        spmv_csr by_level;
        by_level.rows = rows; by_level.cols = levels; by_level.nnz = rows; by_level.device = h.device;
        by_level.d_row_ptr = iota; by_level.d_col_idx = level; by_level.d_vals = zeros;
        spmv_csr_t *sorted = nullptr;
        if (int rc2 = transpose(by_level, false, s, &sorted)) return rc2;
        if (sorted->rows != levels || sorted->nnz != rows || !sorted->own_row_ptr || !sorted->own_col_idx) {
            (void)spmv_csr_destroy(sorted);
            return trsv_fail("the rows did not sort by level");
        }
        p.d_level_ptr = std::move(sorted->own_row_ptr);
        p.d_order = std::move(sorted->own_col_idx);
        (void)spmv_csr_destroy(sorted);

        // the long rows
        int32_t n_terms = 0;
        if (int rc2 = scan_offsets_i32(p.d_lstart.get(), rows, d_st.get(), true, s, &n_terms)) return rc2;
        if (n_terms < 0) return trsv_fail("the long rows hold 2^31 terms or more");
        p.long_terms = n_terms;
        SPMV_HIP_TRY(p.d_lterm.alloc((size_t)n_terms));
        if (n_terms > 0) {
            hipLaunchKernelGGL(k_trsv_terms, dim3(trsv_blocks(rows)), dim3(kBlock), 0, s, rows, nnz, h.d_row_ptr, h.d_col_idx, upper,
                               (const int32_t *)p.d_lstart.get(), p.d_lterm.get(), (uint32_t)n_terms);
            if (int rc2 = check_launch("k_trsv_terms")) return rc2;
            hipLaunchKernelGGL(k_trsv_mark, dim3(trsv_blocks(rows)), dim3(kBlock), 0, s, rows, (const int32_t *)p.d_lstart.get(), p.d_order.get());
            if (int rc2 = check_launch("k_trsv_mark")) return rc2;
        }
    } else {
        SPMV_HIP_TRY(p.d_level_ptr.alloc(1));
        SPMV_HIP_TRY(p.d_order.alloc(0));
        SPMV_HIP_TRY(p.d_lterm.alloc(0));
        SPMV_HIP_TRY(hipMemsetAsync(p.d_level_ptr.get(), 0, sizeof(int32_t), s));
        SPMV_HIP_TRY(hipMemsetAsync(p.d_lstart.get(), 0, sizeof(int32_t), s));
    }
    p.levels = levels;

    // the steps, from the host's copy of level_ptr
    p.level_ptr = new (std::nothrow) int32_t[(size_t)levels + 1];
    p.steps = new (std::nothrow) TrsvStep[(size_t)levels + 1];
    if (!p.level_ptr || !p.steps) return trsv_fail("out of host memory");
    SPMV_HIP_TRY(hipMemcpyAsync(p.level_ptr, p.d_level_ptr.get(), sizeof(int32_t) * ((size_t)levels + 1), hipMemcpyDeviceToHost, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    if (p.level_ptr[0] != 0 || (int64_t)p.level_ptr[levels] != rows) return trsv_fail("the levels do not cover the rows");
    for (int64_t k = 0; k < levels; ++k) {
        const int64_t n = (int64_t)p.level_ptr[k + 1] - p.level_ptr[k];
        if (n < 1) return trsv_fail("an empty level");
        if (n > p.widest) p.widest = n;
    }
    for (int64_t k = 0; k < levels;) {
        TrsvStep &step = p.steps[p.nsteps++];
        step.first = (int32_t)k;
        if ((int64_t)p.level_ptr[k + 1] - p.level_ptr[k] > p.thin) {
            step.merged = false;
            ++k;
        } else {
            step.merged = true;
            const int64_t stop = k + p.cap < levels ? k + p.cap : levels;
            while (k < stop && (int64_t)p.level_ptr[k + 1] - p.level_ptr[k] <= p.thin) ++k;
        }
        step.last = (int32_t)k;
    }
    p.ready = true;
    h.plan_trsv[upper ? 1 : 0] = std::move(p);
    return SPMV_OK;
}

int trsv_solve(const spmv_csr &h, bool upper, bool unit, const float *b, float *x, hipStream_t s)
{
    const TrsvPlan &p = h.plan_trsv[upper ? 1 : 0];
    const TrsvArgs a{h.rows, (uint32_t)h.nnz, (uint32_t)p.long_terms, h.d_row_ptr, h.d_col_idx, h.d_vals, p.d_order.get(), p.d_level_ptr.get(),
                     p.d_diag.get(), p.d_lstart.get(), p.d_lterm.get(), b, x, upper, unit};
    for (int64_t i = 0; i < p.nsteps; ++i) {
        const TrsvStep &step = p.steps[i];
        if (step.merged) {
            hipLaunchKernelGGL(k_trsv_levels, dim3(1), dim3(kBlock), 0, s, a, step.first, step.last);
            if (int rc = check_launch("k_trsv_levels")) return rc;
        } else {
            const int64_t p0 = p.level_ptr[step.first], p1 = p.level_ptr[step.first + 1];
            hipLaunchKernelGGL(k_trsv_level, dim3(trsv_blocks(p1 - p0)), dim3(kBlock), 0, s, a, p0, p1);
            if (int rc = check_launch("k_trsv_level")) return rc;
        }
    }
    return SPMV_OK;
}

}  // namespace spmv
