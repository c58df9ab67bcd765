// kernels_ilu0.hip -- spmv_csr_ilu0 / _values / _solve / _pivot (include/spmv_hip.h "the incomplete factorisation"): M = ILU(0)
// of a square handle with sorted rows and a stored diagonal, on A's pattern, L (unit lower) and U (upper) in ONE handle.
//
// Row i of the factor needs the finished rows k < i with (i, k) stored: the dependency graph of the LOWER triangle.  So the
// lower TrsvPlan of the factor handle (kernels_trsv.hip: order, level_ptr, the diagonal's positions, the steps) is the schedule
// of the factorisation too, and nothing is analysed here.  As for the solve, nothing waits for a value another workgroup
// writes: no flag, no spin, no grid barrier and no cooperative launch; the only waits are kernel boundaries and __syncthreads()
// inside the one workgroup of a merged launch, and every loop bound is a kernel argument or comes from row_ptr or the plan.
//
// k_ilu0_level (a grid over one level) and k_ilu0_levels (one workgroup over a run of thin levels) share ilu0_wave: 64
// consecutive rows of the level's list.  Bit 31 of an entry of order is the solve's mark and is masked: here a row is long when
// it STORES more than SPMV_ILU0_SERIAL_MAX entries.
//   short row  one lane: copies a's row into M, then walks the contract as written.  All of the row's traffic is one lane's, so
//              program order is the only order needed.
//   long row   the wavefront, one row after the other (__ballot): position r of the row BELONGS to lane (r - lo) % 64 for the
//              whole row.  The owners copy a's row.  At step p (column k < i) the owner of p divides and __shfl's l; every lane
//              then visits its own positions r > p and looks column ci[r] up in row k beyond the diagonal by bisection.  No value
//              of row i is read by another lane than the one that wrote it, so there is no LDS staging, no fence and no cap on
//              the row's length; every entry sees its terms in ascending k because p ascends for the whole wavefront.
// Values of EARLIER rows (row k's, and the pivots) were written by other wavefronts before a kernel boundary or the workgroup
// barrier, as trsv reads x.  So the pointer to M's values is neither const nor __restrict__, and none of its loads may become a
// scalar or otherwise non-coherent load (DESIGN section 30 says how that was checked in the ISA).  a's values are only read.
//
// No atomic touches a value.  The one atomic is an integer minimum on the pivot word (the smallest row whose u_ii is +-0 or not
// finite): its result does not depend on the order of arrival and reaches no value.
//
// Positions are unsigned 32-bit (nnz < 2^31).  Every access is predicated on its array's own length: a handle that was never
// validated gives an unspecified result inside the arrays.
#include <climits>
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

struct Ilu0Row { uint32_t lo, hi; };      // positions [lo, hi) of a row, hi <= nnz, lo <= hi

__device__ __forceinline__ Ilu0Row ilu0_row(const int32_t *rp, int64_t row, uint32_t nnz)
{
    const uint32_t hi = min((uint32_t)rp[row + 1], nnz), lo = min((uint32_t)rp[row], hi);
    return Ilu0Row{lo, hi};
}

// ---- what spmv_csr_ilu0 asks of a: strictly ascending rows that store their diagonal ------------------------------------------
// bad[0]: the first row that is not strictly ascending, bad[1]: the first row without a diagonal entry (integer minima)
__global__ __launch_bounds__(kBlock) void k_ilu0_check(int64_t rows, uint32_t nnz, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       int32_t *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows) return;
    const Ilu0Row r = ilu0_row(rp, i, nnz);
    bool ascending = true, diagonal = false;
    int prev = 0;
    for (uint32_t s = r.lo; s < r.hi; ++s) {
        const int c = ci[s];
        if (s > r.lo && c <= prev) ascending = false;
        if (c == (int)i) diagonal = true;
        prev = c;
    }
    if (!ascending) atomicMin(&bad[0], (int32_t)i);
    if (!diagonal) atomicMin(&bad[1], (int32_t)i);
}

__global__ void k_ilu0_reset(int32_t *pivot)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *pivot = INT32_MAX;
}

// ---- the factorisation -----------------------------------------------------------------------------------------------------------
struct Ilu0Args {
    int64_t rows;
    uint32_t nnz;
    const int32_t *rp, *ci;
    const float *av;                      // a's values (read only)
    float *mv;                            // M's values: written here and read back, by this row's lanes and by later rows'
    const int32_t *order, *level_ptr, *diag;
    int32_t *pivot;
};

__device__ __forceinline__ void ilu0_pivot_check(const Ilu0Args &a, int row, float u)
{
    if (u == 0.0f || !(__builtin_fabsf(u) <= 3.402823466e+38f)) atomicMin(a.pivot, (int32_t)row);
}

// the rows at positions base + lane < end of the level's list
__device__ __forceinline__ void ilu0_wave(const Ilu0Args &a, int64_t base, int64_t end, int lane)
{
    const int64_t pos = base + lane;
    const uint32_t word = pos < end ? (uint32_t)a.order[pos] : 0xffffffffu;
    const int row = (int)(word & 0x7fffffffu);
    const bool have = pos < end && (int64_t)row < a.rows;
    Ilu0Row r{0u, 0u};
    if (have) r = ilu0_row(a.rp, row, a.nnz);
    const bool is_long = have && r.hi - r.lo > (uint32_t)SPMV_ILU0_SERIAL_MAX;
    if (have && !is_long) {
        for (uint32_t s = r.lo; s < r.hi; ++s) a.mv[s] = a.av[s];
        for (uint32_t p = r.lo; p < r.hi; ++p) {
            const int k = a.ci[p];
            if (k < 0 || k >= row) continue;
            const int32_t dk = a.diag[k];
            if (dk < 0 || (uint32_t)dk >= a.nnz) continue;
            const float l = a.mv[p] / a.mv[dk];
            a.mv[p] = l;
            const uint32_t q1 = ilu0_row(a.rp, k, a.nnz).hi;
            uint32_t t = p + 1;                               // (both rows ascend: the search for j goes on where the last one stopped)
            for (uint32_t q = (uint32_t)dk + 1; q < q1; ++q) {
                const int j = a.ci[q];
                if (j <= k) continue;
                while (t < r.hi && a.ci[t] < j) ++t;
                if (t >= r.hi) break;
                if (a.ci[t] == j) a.mv[t] = __builtin_fmaf(-l, a.mv[q], a.mv[t]);
            }
        }
        const int32_t dp = a.diag[row];
        if (dp >= 0 && (uint32_t)dp >= r.lo && (uint32_t)dp < r.hi) ilu0_pivot_check(a, row, a.mv[dp]);
    }
    for (uint64_t m = __ballot(is_long); m != 0; m &= m - 1) {
        const int src = __ffsll((unsigned long long)m) - 1;
        const int lrow = __shfl(row, src);
        const Ilu0Row w = ilu0_row(a.rp, lrow, a.nnz);
        for (uint64_t s = (uint64_t)w.lo + (uint32_t)lane; s < w.hi; s += kWave) a.mv[s] = a.av[s];
        for (uint32_t p = w.lo; p < w.hi; ++p) {
            const int k = a.ci[p];                            // (one address for the wavefront: every branch on k is uniform)
            if (k < 0 || k >= lrow) continue;
            const int32_t dk = a.diag[k];
            if (dk < 0 || (uint32_t)dk >= a.nnz) continue;
            const int owner = (int)((p - w.lo) & (uint32_t)(kWave - 1));
            float l = 0.0f;
            if (lane == owner) {
                l = a.mv[p] / a.mv[dk];
                a.mv[p] = l;
            }
            l = __shfl(l, owner);
            const uint32_t q0 = (uint32_t)dk + 1, q1 = ilu0_row(a.rp, k, a.nnz).hi;
            if (q0 >= q1) continue;
            // this lane's positions beyond p: r = lo + lane (mod 64)
            const uint32_t ahead = ((uint32_t)lane - (p + 1 - w.lo)) & (uint32_t)(kWave - 1);
            for (uint64_t t = (uint64_t)p + 1 + ahead; t < w.hi; t += kWave) {
                const int j = a.ci[t];
                uint32_t x0 = q0, x1 = q1;
                while (x0 < x1) {
                    const uint32_t mid = x0 + (x1 - x0) / 2;
                    if (a.ci[mid] < j) x0 = mid + 1; else x1 = mid;
                }
                if (x0 < q1 && a.ci[x0] == j) a.mv[t] = __builtin_fmaf(-l, a.mv[x0], a.mv[t]);
            }
        }
        const int32_t dp = a.diag[lrow];
        if (dp >= 0 && (uint32_t)dp >= w.lo && (uint32_t)dp < w.hi && lane == (int)(((uint32_t)dp - w.lo) & (uint32_t)(kWave - 1)))
            ilu0_pivot_check(a, lrow, a.mv[dp]);
    }
}

// one level, positions [p0, p1) of order: a wavefront per 64 rows
__global__ __launch_bounds__(kBlock) void k_ilu0_level(Ilu0Args a, int64_t p0, int64_t p1)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int64_t base = p0 + ((int64_t)blockIdx.x * kBlock + (threadIdx.x - (unsigned)lane));
    if (base >= p1) return;                                // (a whole wavefront)
    ilu0_wave(a, base, p1, lane);
}

// the levels [k0, k1), one workgroup: level after level, __syncthreads() between them
__global__ __launch_bounds__(kBlock) void k_ilu0_levels(Ilu0Args a, int32_t k0, int32_t k1)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int64_t first = (int64_t)(threadIdx.x - (unsigned)lane);
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t p1 = min((int64_t)(uint32_t)a.level_ptr[k + 1], a.rows), p0 = min((int64_t)(uint32_t)a.level_ptr[k], p1);
        for (int64_t base = p0 + first; base < p1; base += kBlock) ilu0_wave(a, base, p1, lane);
        __syncthreads();
    }
}

unsigned ilu0_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the launches of one factorisation: the pivot word's reset, then the steps of the lower plan
int ilu0_factor(spmv_csr &m, const float *a_vals, hipStream_t s)
{
    const TrsvPlan &p = m.plan_trsv[0];
    const Ilu0Args a{m.rows, (uint32_t)m.nnz, m.d_row_ptr, m.d_col_idx, a_vals, m.own_vals.get(), p.d_order.get(), p.d_level_ptr.get(),
                     p.d_diag.get(), m.plan_ilu0.d_pivot.get()};
    hipLaunchKernelGGL(k_ilu0_reset, dim3(1), dim3(kWave), 0, s, m.plan_ilu0.d_pivot.get());
    if (int rc = check_launch("k_ilu0_reset")) return rc;
    for (int64_t i = 0; i < p.nsteps; ++i) {
        const TrsvStep &step = p.steps[i];
        if (step.merged) {
            hipLaunchKernelGGL(k_ilu0_levels, dim3(1), dim3(kBlock), 0, s, a, step.first, step.last);
            if (int rc = check_launch("k_ilu0_levels")) return rc;
        } else {
            const int64_t p0 = p.level_ptr[step.first], p1 = p.level_ptr[step.first + 1];
            hipLaunchKernelGGL(k_ilu0_level, dim3(ilu0_blocks(p1 - p0)), dim3(kBlock), 0, s, a, p0, p1);
            if (int rc = check_launch("k_ilu0_level")) return rc;
        }
    }
    return SPMV_OK;
}

}  // namespace

int64_t ilu0_plan_bytes(const spmv_csr &m)
{
    return m.plan_ilu0.ready ? trsv_plan_bytes(m.plan_trsv[0], m.rows) + trsv_plan_bytes(m.plan_trsv[1], m.rows) + 4 : 0;
}

// Device memory while the call runs, beside M (4 (rows + 1) + 8 nnz bytes) and what it keeps (ilu0_plan_bytes): 8 bytes of the
// check's two minima, and the build peak of one trsv plan at a time (trsv_plan in kernels_trsv.hip), the lower one first.
int ilu0(const spmv_csr &a, int thin_rows, hipStream_t s, spmv_csr_t **out)
{
    const int64_t rows = a.rows, nnz = a.nnz;
    if (rows > 0) {
        DevPtr<int32_t> d_bad;
        int32_t bad[2] = {INT32_MAX, INT32_MAX};
        SPMV_HIP_TRY(d_bad.alloc(2));
        SPMV_HIP_TRY(hipMemcpyAsync(d_bad.get(), bad, sizeof bad, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_ilu0_check, dim3(ilu0_blocks(rows)), dim3(kBlock), 0, s, rows, (uint32_t)nnz, a.d_row_ptr, a.d_col_idx, d_bad.get());
        if (int rc = check_launch("k_ilu0_check")) return rc;
        SPMV_HIP_TRY(hipMemcpyAsync(bad, d_bad.get(), sizeof bad, hipMemcpyDeviceToHost, s));
        SPMV_HIP_TRY(hipStreamSynchronize(s));
        if (bad[0] != INT32_MAX || bad[1] != INT32_MAX) {
            const char *hint = "spmv_csr_add(A, empty, 1, 0, SPMV_ADD_UNION) sorts a matrix and spmv_csr_add(A, I, 1, 0, SPMV_ADD_UNION) gives it a "
                               "diagonal";
            if (bad[0] <= bad[1])
                set_error("spmv_csr_ilu0: row %d is not strictly ascending (unsorted, or a column repeats); %s", bad[0], hint);
            else
                set_error("spmv_csr_ilu0: row %d stores no diagonal entry; %s", bad[1], hint);
            return SPMV_ERR_INVALID;
        }
    }
    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("spmv_csr_ilu0: out of host memory"); return SPMV_ERR_INVALID; }
    struct Guard {                                          // a refusal below leaves nothing allocated
        spmv_csr *h;
        ~Guard() { if (h) (void)spmv_csr_destroy(h); }
    } guard{h};
    h->rows = rows; h->cols = a.cols; h->nnz = nnz;
    h->device = a.device;
    SPMV_HIP_TRY(h->own_row_ptr.alloc((size_t)rows + 1));
    SPMV_HIP_TRY(h->own_col_idx.alloc((size_t)nnz));
    SPMV_HIP_TRY(h->own_vals.alloc((size_t)nnz));
    SPMV_HIP_TRY(h->plan_ilu0.d_pivot.alloc(1));
    h->d_row_ptr = h->own_row_ptr; h->d_col_idx = h->own_col_idx; h->d_vals = h->own_vals;
    if (rows > 0)
        SPMV_HIP_TRY(hipMemcpyAsync(h->own_row_ptr.get(), a.d_row_ptr, sizeof(int32_t) * ((size_t)rows + 1), hipMemcpyDeviceToDevice, s));
    else
        SPMV_HIP_TRY(hipMemsetAsync(h->own_row_ptr.get(), 0, sizeof(int32_t), s));
    if (nnz > 0) SPMV_HIP_TRY(hipMemcpyAsync(h->own_col_idx.get(), a.d_col_idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    if (int rc = trsv_plan(*h, false, thin_rows, s)) return rc;
    if (int rc = trsv_plan(*h, true, thin_rows, s)) return rc;
    if (h->plan_trsv[0].bad_diag_row >= 0 || h->plan_trsv[1].bad_diag_row >= 0) {
        set_error("spmv_csr_ilu0: the plans found row %lld without exactly one diagonal entry (the arrays changed during the call)",
                  (long long)(h->plan_trsv[0].bad_diag_row >= 0 ? h->plan_trsv[0].bad_diag_row : h->plan_trsv[1].bad_diag_row));
        return SPMV_ERR_INVALID;
    }
    h->plan_ilu0.a_rows = rows;
    h->plan_ilu0.a_nnz = nnz;
    h->plan_ilu0.ready = true;
    if (int rc = ilu0_factor(*h, a.d_vals, s)) return rc;
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    guard.h = nullptr;
    *out = h;
    return SPMV_OK;
}

int ilu0_values(spmv_csr &m, const spmv_csr &a, hipStream_t s) { return ilu0_factor(m, a.d_vals, s); }

int ilu0_solve(const spmv_csr &m, const float *r, float *z, hipStream_t s)
{
    if (int rc = trsv_solve(m, false, true, r, z, s)) return rc;
    return trsv_solve(m, true, false, z, z, s);
}

int ilu0_pivot(const spmv_csr &m, hipStream_t s, int64_t *row)
{
    int32_t w = INT32_MAX;
    SPMV_HIP_TRY(hipMemcpyAsync(&w, m.plan_ilu0.d_pivot.get(), sizeof w, hipMemcpyDeviceToHost, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    *row = w == INT32_MAX ? -1 : (int64_t)w;
    return SPMV_OK;
}

}  // namespace spmv
