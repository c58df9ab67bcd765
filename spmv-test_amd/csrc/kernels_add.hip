// kernels_add.hip -- spmv_csr_add / spmv_csr_add_values / spmv_csr_add_gather (include/spmv_hip.h "the sparse sum"):
// C = alpha A + beta B on the union, the intersection or the difference of two patterns, as a new handle that owns its arrays.
// Every row of C is sorted and duplicate-free; the value of entry (i, j) is one chain over a's terms of column j in ascending
// storage position and then b's.  Nothing here depends on the order in which anything arrives: no read-modify-write atomic,
// no LDS and no row class -- a row of 5000 entries and a row of 2 go through the same lanes.
//
// Both operands are read through a VIEW with sorted rows: the operand's own arrays where k_add_sorted finds every row
// non-decreasing, else the handle of transpose(transpose(.)) (kernels_transpose.hip: a stable sort by column inside every row)
// and the composition of its two maps, which takes a sorted position back to the storage position it came from.
//
//   1. k_add_sorted   a lane per nonzero: does col_idx fall inside a row?  (an integer flag, stored, never read back on the device)
//   2. k_add_mark     a lane per nonzero of a side: is it the HEAD of its column's run in the row (the first of equal columns),
//                     and is its entry kept under op?  The other side's row is bisected for the column.  flags[p] = 0 / 1;
//                     exclusive_scan_i32 turns the flags into ranks.  Under UNION b's heads are marked too (kept: not in a).
//   3. k_add_count    a lane per row: kept heads = differences of the ranks at the row's ends; scan_offsets_i32 -> c.row_ptr.
//                     The total is the sum of the two scans' totals, a 64-bit number on the host (refused from 2^31 on).
//   4. k_add_place    a lane per nonzero again, kept heads only: the entry's place in its row is (kept heads of its own side
//                     before it) + (kept heads of the other side below its lower bound there) -- no sort.  Writes c.col_idx
//                     and the entry's number of terms; exclusive_scan_i32 makes them the plan's starts.
//   5. k_add_terms    a lane per entry of c: a's run of the column, then b's, as side << 31 | storage position.
//   6. k_add_values   a lane per entry of c walks its run (the first call and spmv_csr_add_values alike).
//      k_add_gather   a lane per entry of c: the words of the chosen side's terms.
//
// Positions are unsigned 32-bit (nnz < 2^31).  Every access is predicated on its array's own length: nothing here relies on
// slack behind an array, and a handle that was never validated gives an unspecified result inside the arrays.
#include <climits>
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

// one operand through its sorted view
struct AddSide {
    const int32_t *rp;        // [rows + 1]
    const int32_t *ci;        // [nnz] non-decreasing inside every row
    const uint32_t *perm;     // [nnz] the storage position of a sorted position; null: the same
    uint32_t nnz;
};

struct AddRow { uint32_t lo, hi; };      // positions [lo, hi) of a row, hi <= nnz, lo <= hi

__device__ __forceinline__ AddRow add_row(const AddSide &x, int64_t row)
{
    const uint32_t hi = min((uint32_t)x.rp[row + 1], x.nnz), lo = min((uint32_t)x.rp[row], hi);
    return AddRow{lo, hi};
}

// the row that holds position k of an array of n < 2^31 positions: the last r < rows with row_ptr[r] <= k (rows >= 1)
__device__ __forceinline__ int64_t add_row_of(const int32_t *__restrict__ row_ptr, int64_t rows, uint32_t k)
{
    int64_t lo = 0, hi = rows;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)row_ptr[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the first position of [lo, hi) whose column is not below j (hi where there is none)
__device__ __forceinline__ uint32_t add_lower(const int32_t *__restrict__ ci, uint32_t lo, uint32_t hi, int j)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ci[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// how many positions from p on (p < hi) hold column j
__device__ __forceinline__ uint32_t add_run(const int32_t *__restrict__ ci, uint32_t p, uint32_t hi, int j)
{
    uint32_t e = p;
    while (e < hi && ci[e] == j) ++e;
    return e - p;
}

// ---- 1. is every row non-decreasing? ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_add_sorted(int64_t rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       uint32_t nnz, int32_t *__restrict__ unsorted)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < 1 || k >= (int64_t)nnz) return;
    if (ci[k - 1] <= ci[k]) return;
    // a descent: inside a row, unless position k starts one
    const int64_t r = add_row_of(rp, rows, (uint32_t)k);
    if ((uint32_t)rp[r] != (uint32_t)k) __hip_atomic_store(unsorted, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (every writer stores the same word)
}

// ---- 2. the kept heads of one side ----------------------------------------------------------------------------------------
enum { kKeepAll = 0, kKeepIfOther = 1, kKeepIfNotOther = 2 };

__global__ __launch_bounds__(kBlock) void k_add_mark(AddSide x, AddSide y, int64_t rows, int keep, int32_t *__restrict__ flags)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)x.nnz) return;
    const uint32_t p = (uint32_t)k;
    const int64_t row = add_row_of(x.rp, rows, p);
    const AddRow rx = add_row(x, row);
    int kept = 0;
    if (p >= rx.lo && p < rx.hi) {
        const int j = x.ci[p];
        const bool head = p == rx.lo || x.ci[p - 1] != j;
        if (head) {
            kept = 1;
            if (keep != kKeepAll) {
                const AddRow ry = add_row(y, row);
                const uint32_t lb = add_lower(y.ci, ry.lo, ry.hi, j);
                const bool in_other = lb < ry.hi && y.ci[lb] == j;
                kept = in_other == (keep == kKeepIfOther) ? 1 : 0;
            }
        }
    }
    flags[p] = kept;
}

// ---- 3. the entries of every row ---------------------------------------------------------------------------------------------
// sx, sy: the scanned flags ([nnz + 1] each; sy null: that side owns no entry)
__global__ __launch_bounds__(kBlock) void k_add_count(AddSide x, AddSide y, int64_t rows, const int32_t *__restrict__ sx,
                                                      const int32_t *__restrict__ sy, int32_t *__restrict__ counts)
{
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    const AddRow rx = add_row(x, row);
    int32_t n = sx[rx.hi] - sx[rx.lo];
    if (sy) {
        const AddRow ry = add_row(y, row);
        n += sy[ry.hi] - sy[ry.lo];
    }
    counts[row] = n;
}

// ---- 4. the kept heads to their places -----------------------------------------------------------------------------------------
// x: the side whose nonzeros the lanes take; x_terms_only: the entries x owns have no term of y (b's entries under UNION: the
// column is not in a; MINUS: b has no terms).  len[e] = the entry's number of terms.
__global__ __launch_bounds__(kBlock) void k_add_place(AddSide x, AddSide y, int64_t rows, const int32_t *__restrict__ sx,
                                                      const int32_t *__restrict__ sy, bool x_terms_only,
                                                      const int32_t *__restrict__ c_rp, int32_t *__restrict__ c_ci,
                                                      int32_t *__restrict__ len, uint32_t c_nnz)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)x.nnz) return;
    const uint32_t p = (uint32_t)k;
    if (sx[p + 1] == sx[p]) return;                          // not a kept head
    const int64_t row = add_row_of(x.rp, rows, p);
    const AddRow rx = add_row(x, row), ry = add_row(y, row);
    if (p < rx.lo || p >= rx.hi) return;
    const int j = x.ci[p];
    const uint32_t lb = add_lower(y.ci, ry.lo, ry.hi, j);
    uint32_t at = (uint32_t)(sx[p] - sx[rx.lo]);
    if (sy) at += (uint32_t)(sy[lb] - sy[ry.lo]);
    uint32_t terms = add_run(x.ci, p, rx.hi, j);
    if (!x_terms_only) terms += add_run(y.ci, lb, ry.hi, j);
    const uint32_t e = (uint32_t)c_rp[row] + at;
    if (e < c_nnz && e >= (uint32_t)c_rp[row] && e < (uint32_t)c_rp[row + 1]) {
        c_ci[e] = j;
        len[e] = (int32_t)terms;
    }
}

// ---- 5. the terms of every entry -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_add_terms(AddSide a, AddSide b, int64_t rows, bool b_terms, const int32_t *__restrict__ c_rp,
                                                      const int32_t *__restrict__ c_ci, uint32_t c_nnz, const int32_t *__restrict__ start,
                                                      uint32_t *__restrict__ term, uint32_t n_terms)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)c_nnz) return;
    const uint32_t e = (uint32_t)k;
    const int64_t row = add_row_of(c_rp, rows, e);
    const int j = c_ci[e];
    uint32_t t = (uint32_t)start[e];
    const uint32_t t1 = min((uint32_t)start[e + 1], n_terms);
    const AddRow ra = add_row(a, row);
    for (uint32_t p = add_lower(a.ci, ra.lo, ra.hi, j); p < ra.hi && a.ci[p] == j && t < t1; ++p, ++t)
        term[t] = a.perm ? (a.perm[p] & 0x7fffffffu) : p;
    if (b_terms) {
        const AddRow rb = add_row(b, row);
        for (uint32_t q = add_lower(b.ci, rb.lo, rb.hi, j); q < rb.hi && b.ci[q] == j && t < t1; ++q, ++t)
            term[t] = 0x80000000u | (b.perm ? b.perm[q] : q);
    }
    for (; t < t1; ++t) term[t] = 0x7fffffffu;               // (only an operand that was never validated leaves a gap: no position)
}

// ---- 6. the values: a lane per entry walks its run ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_add_values(uint32_t c_nnz, const int32_t *__restrict__ start, const uint32_t *__restrict__ term,
                                                       uint32_t n_terms, const float *__restrict__ a_va, uint32_t a_nnz,
                                                       const float *__restrict__ b_va, uint32_t b_nnz, float alpha, float beta,
                                                       float *__restrict__ c_va)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)c_nnz) return;
    const uint32_t t0 = (uint32_t)start[k], t1 = min((uint32_t)start[k + 1], n_terms);
    const bool use_a = alpha != 0.0f, use_b = beta != 0.0f;  // (a coefficient of +0 or -0: no terms; a NaN one has them)
    float acc = 0.0f;
    bool first = true;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t w = term[t], pos = w & 0x7fffffffu;
        const bool side_b = (w >> 31) != 0u;
        if (side_b ? (!use_b || pos >= b_nnz) : (!use_a || pos >= a_nnz)) continue;
        const float coef = side_b ? beta : alpha, v = side_b ? b_va[pos] : a_va[pos];
        acc = first ? __fmul_rn(coef, v) : __builtin_fmaf(coef, v, acc);
        first = false;
    }
    c_va[k] = acc;
}

// dst[c][p] = src[c][e] for every term of `side` at storage position p of entry e
__global__ __launch_bounds__(kBlock) void k_add_gather(uint32_t c_nnz, const int32_t *__restrict__ start, const uint32_t *__restrict__ term,
                                                       uint32_t n_terms, uint32_t side, uint32_t side_nnz, int count,
                                                       const uint32_t *__restrict__ src, int64_t src_stride, uint32_t *__restrict__ dst,
                                                       int64_t dst_stride)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)c_nnz) return;
    const uint32_t t0 = (uint32_t)start[k], t1 = min((uint32_t)start[k + 1], n_terms);
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t w = term[t], pos = w & 0x7fffffffu;
        if ((w >> 31) != side || pos >= side_nnz) continue;
        for (int c = 0; c < count; ++c) dst[c * dst_stride + pos] = src[c * src_stride + k];
    }
}

unsigned add_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// an operand's sorted view and what keeps it alive
struct AddView {
    AddSide side{nullptr, nullptr, nullptr, 0u};
    spmv_csr_t *sorted = nullptr;        // transpose(transpose(operand)) where a row of the operand is not sorted
    DevPtr<uint32_t> perm;
    AddView() = default;
    AddView(const AddView &) = delete;
    AddView &operator=(const AddView &) = delete;
    ~AddView() { (void)spmv_csr_destroy(sorted); }
};

int add_view(const spmv_csr &x, hipStream_t s, int32_t *d_flag, AddView &v)
{
    v.side = AddSide{x.d_row_ptr, x.d_col_idx, nullptr, (uint32_t)x.nnz};
    if (x.nnz < 2 || x.rows < 1) return SPMV_OK;
    SPMV_HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_add_sorted, dim3(add_blocks(x.nnz)), dim3(kBlock), 0, s, x.rows, x.d_row_ptr, x.d_col_idx, (uint32_t)x.nnz, d_flag);
    if (int rc = check_launch("k_add_sorted")) return rc;
    int32_t unsorted = 0;
    SPMV_HIP_TRY(hipMemcpyAsync(&unsorted, d_flag, sizeof unsorted, hipMemcpyDeviceToHost, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    if (!unsorted) return SPMV_OK;
    // the rare route: two stable sorts by column (the transpose's peak memory), the maps composed
    spmv_csr_t *t1 = nullptr;
    if (int rc = transpose(x, true, s, &t1)) return rc;
    int rc = transpose(*t1, true, s, &v.sorted);
    if (rc == SPMV_OK && v.perm.alloc((size_t)x.nnz) != hipSuccess) {
        set_error("spmv_csr_add: out of device memory for the row-sorted view");
        rc = SPMV_ERR_HIP;
    }
    if (rc == SPMV_OK) rc = map_move(v.sorted->map, v.sorted->nnz, false, 1, t1->map.words.get(), 0, v.perm.get(), 0, s);
    if (rc == SPMV_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_error("spmv_csr_add: hipStreamSynchronize failed");
        rc = SPMV_ERR_HIP;
    }
    (void)spmv_csr_destroy(t1);
    if (rc) return rc;
    if (v.sorted->rows != x.rows || v.sorted->nnz != x.nnz) {
        set_error("spmv_csr_add: an operand's arrays are not a valid CSR (its row-sorted view has another shape)");
        return SPMV_ERR_INVALID;
    }
    v.side = AddSide{v.sorted->d_row_ptr, v.sorted->d_col_idx, v.perm.get(), (uint32_t)x.nnz};
    return SPMV_OK;
}

int add_launch_values(const AddPlan &p, const spmv_csr &a, const spmv_csr &b, float alpha, float beta, float *c_va, int64_t c_nnz,
                      hipStream_t s)
{
    if (c_nnz <= 0) return SPMV_OK;
    hipLaunchKernelGGL(k_add_values, dim3(add_blocks(c_nnz)), dim3(kBlock), 0, s, (uint32_t)c_nnz, (const int32_t *)p.d_start.get(),
                       (const uint32_t *)p.d_term.get(), (uint32_t)p.terms, a.d_vals, (uint32_t)a.nnz, b.d_vals, (uint32_t)b.nnz, alpha, beta,
                       c_va);
    return check_launch("k_add_values");
}

}  // namespace

int64_t add_plan_bytes(const spmv_csr &c) { return c.plan_add.ready ? 4 * c.plan_add.terms + 4 * (c.nnz + 1) : 0; }

// Device memory while the call runs, beside C's own arrays (4 (m + 1) + 8 nnz(C) bytes) and the plan (4 terms + 4 (nnz(C) + 1),
// freed on return without keep_plan): 4 (a.nnz + 1) + 4 (b.nnz + 1) (the ranks; b's under UNION only) + 8 + what the scans take
// (4 bytes per 4096 elements).  An unsorted operand adds its sorted view: 8 nnz + 4 (m + 1) (the second transpose) + 4 nnz (the
// composed map), and while it is built the first transpose (12 nnz + 4 (n + 1)) and the transpose's own temporaries.
int add(const spmv_csr &a, const spmv_csr &b, float alpha, float beta, int op, bool keep_plan, hipStream_t s, spmv_csr_t **out)
{
    const int64_t rows = a.rows;
    const bool b_owns = op == SPMV_ADD_UNION, b_terms = op != SPMV_ADD_MINUS;
    AddView va_, vb_;
    AddPlan plan;
    DevPtr<int32_t> rp, ci, total, sa, sb;
    DevPtr<float> va;
    SPMV_HIP_TRY(total.alloc(2));
    if (int rc = add_view(a, s, total.get(), va_)) return rc;
    if (&b == &a) vb_.side = va_.side;
    else if (int rc = add_view(b, s, total.get(), vb_)) return rc;
    const AddSide &xa = va_.side, &xb = vb_.side;

    SPMV_HIP_TRY(rp.alloc((size_t)rows + 1));
    SPMV_HIP_TRY(hipMemsetAsync(rp.get(), 0, sizeof(int32_t) * ((size_t)rows + 1), s));
    int32_t heads_a = 0, heads_b = 0, nnz_c = 0;
    if (rows > 0) {
        SPMV_HIP_TRY(sa.alloc((size_t)a.nnz + 1));
        SPMV_HIP_TRY(hipMemsetAsync(sa.get() + a.nnz, 0, sizeof(int32_t), s));
        if (a.nnz > 0) {
            hipLaunchKernelGGL(k_add_mark, dim3(add_blocks(a.nnz)), dim3(kBlock), 0, s, xa, xb, rows,
                               op == SPMV_ADD_UNION ? (int)kKeepAll : op == SPMV_ADD_INTERSECT ? (int)kKeepIfOther : (int)kKeepIfNotOther,
                               sa.get());
            if (int rc = check_launch("k_add_mark")) return rc;
        }
        if (int rc = scan_offsets_i32(sa.get(), a.nnz, total.get(), true, s, &heads_a)) return rc;
        if (b_owns) {
            SPMV_HIP_TRY(sb.alloc((size_t)b.nnz + 1));
            SPMV_HIP_TRY(hipMemsetAsync(sb.get() + b.nnz, 0, sizeof(int32_t), s));
            if (b.nnz > 0) {
                hipLaunchKernelGGL(k_add_mark, dim3(add_blocks(b.nnz)), dim3(kBlock), 0, s, xb, xa, rows, (int)kKeepIfNotOther, sb.get());
                if (int rc = check_launch("k_add_mark")) return rc;
            }
            if (int rc = scan_offsets_i32(sb.get(), b.nnz, total.get(), true, s, &heads_b)) return rc;
        }
        const int64_t entries = (int64_t)heads_a + (int64_t)heads_b;
        if (entries > (int64_t)INT32_MAX) {
            set_error("spmv_csr_add: the sum has %lld nonzeros (a handle holds fewer than 2^31)", (long long)entries);
            return SPMV_ERR_INVALID;
        }
        hipLaunchKernelGGL(k_add_count, dim3(add_blocks(rows)), dim3(kBlock), 0, s, xa, xb, rows, (const int32_t *)sa.get(),
                           (const int32_t *)sb.get(), rp.get());
        if (int rc = check_launch("k_add_count")) return rc;
        if (int rc = scan_offsets_i32(rp.get(), rows, total.get(), true, s, &nnz_c)) return rc;
        if (nnz_c < 0 || (int64_t)nnz_c != entries) {
            set_error("spmv_csr_add: an operand's row_ptr is not a valid CSR (the rows hold %d entries, the operands %lld)", nnz_c,
                      (long long)entries);
            return SPMV_ERR_INVALID;
        }
    }
    SPMV_HIP_TRY(ci.alloc((size_t)nnz_c));
    SPMV_HIP_TRY(va.alloc((size_t)nnz_c));
    SPMV_HIP_TRY(plan.d_start.alloc((size_t)nnz_c + 1));
    SPMV_HIP_TRY(hipMemsetAsync(plan.d_start.get(), 0, sizeof(int32_t) * ((size_t)nnz_c + 1), s));
    int32_t n_terms = 0;
    if (nnz_c > 0) {
        if (a.nnz > 0) {                           // (a grid of no workgroups is not a launch)
            hipLaunchKernelGGL(k_add_place, dim3(add_blocks(a.nnz)), dim3(kBlock), 0, s, xa, xb, rows, (const int32_t *)sa.get(),
                               (const int32_t *)sb.get(), !b_terms, (const int32_t *)rp.get(), ci.get(), plan.d_start.get(),
                               (uint32_t)nnz_c);
            if (int rc = check_launch("k_add_place")) return rc;
        }
        if (b_owns && b.nnz > 0) {
            hipLaunchKernelGGL(k_add_place, dim3(add_blocks(b.nnz)), dim3(kBlock), 0, s, xb, xa, rows, (const int32_t *)sb.get(),
                               (const int32_t *)sa.get(), true, (const int32_t *)rp.get(), ci.get(), plan.d_start.get(), (uint32_t)nnz_c);
            if (int rc = check_launch("k_add_place")) return rc;
        }
        if (int rc = scan_offsets_i32(plan.d_start.get(), nnz_c, total.get(), true, s, &n_terms)) return rc;
        if (n_terms < 0) {
            set_error("spmv_csr_add: an operand's arrays are not a valid CSR (%d terms)", n_terms);
            return SPMV_ERR_INVALID;
        }
    }
    SPMV_HIP_TRY(sa.reset());
    SPMV_HIP_TRY(sb.reset());
    SPMV_HIP_TRY(plan.d_term.alloc((size_t)n_terms));
    plan.terms = n_terms;
    if (nnz_c > 0) {
        hipLaunchKernelGGL(k_add_terms, dim3(add_blocks(nnz_c)), dim3(kBlock), 0, s, xa, xb, rows, b_terms, (const int32_t *)rp.get(),
                           (const int32_t *)ci.get(), (uint32_t)nnz_c, (const int32_t *)plan.d_start.get(), plan.d_term.get(),
                           (uint32_t)n_terms);
        if (int rc = check_launch("k_add_terms")) return rc;
        if (int rc = add_launch_values(plan, a, b, alpha, beta, va.get(), nnz_c, s)) return rc;
    }
    SPMV_HIP_TRY(hipStreamSynchronize(s));         // the views and the ranks are freed on return

    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("spmv_csr_add: out of host memory"); return SPMV_ERR_INVALID; }
    h->rows = a.rows; h->cols = a.cols; h->nnz = nnz_c;
    h->device = a.device;
    h->d_row_ptr = rp; h->d_col_idx = ci; h->d_vals = va;
    h->own_row_ptr = std::move(rp); h->own_col_idx = std::move(ci); h->own_vals = std::move(va);
    if (keep_plan) {
        plan.ready = true;
        plan.op = op;
        plan.a_nnz = a.nnz;
        plan.b_nnz = b.nnz;
        h->plan_add = std::move(plan);
    }
    *out = h;
    return SPMV_OK;
}

int add_values(spmv_csr &c, const spmv_csr &a, const spmv_csr &b, float alpha, float beta, hipStream_t s)
{
    return add_launch_values(c.plan_add, a, b, alpha, beta, c.own_vals.get(), c.nnz, s);
}

int add_gather(const spmv_csr &c, int side, int count, const void *src, int64_t src_stride, void *dst, int64_t dst_stride, hipStream_t s)
{
    if (c.nnz <= 0) return SPMV_OK;
    const AddPlan &p = c.plan_add;
    hipLaunchKernelGGL(k_add_gather, dim3(add_blocks(c.nnz)), dim3(kBlock), 0, s, (uint32_t)c.nnz, (const int32_t *)p.d_start.get(),
                       (const uint32_t *)p.d_term.get(), (uint32_t)p.terms, (uint32_t)side, (uint32_t)(side ? p.b_nnz : p.a_nnz), count,
                       (const uint32_t *)src, src_stride, (uint32_t *)dst, dst_stride);
    return check_launch("k_add_gather");
}

}  // namespace spmv
