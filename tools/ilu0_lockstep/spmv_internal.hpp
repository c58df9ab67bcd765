#pragma once
// tools/ilu0_lockstep: the few names of csrc/spmv_internal.hpp that csrc/kernels_ilu0.hip uses, without HIP; include/spmv_hip.h
// is the real one, copied beside this file.  The trsv plan (kernels_trsv.hip, with a lockstep tool of its own) is a serial
// statement of its header here: order, level_ptr, the diagonal's positions and the steps, built on the host, reading nothing
// outside the arrays whatever they hold.  The solve is not run here.
#include <hip/hip_runtime.h>
#include "spmv_hip.h"
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <utility>
#include <vector>
#define SPMV_HIP_TRY(call) do { if ((call) != hipSuccess) return SPMV_ERR_HIP; } while (0)
namespace spmv {
constexpr int kWave = 64; constexpr int kBlock = 256;
inline bool g_quiet = false;             // expected refusals are not printed
inline void set_error(const char *f, ...) { if (g_quiet) return; va_list a; va_start(a, f); vfprintf(stderr, f, a); va_end(a); fputc('\n', stderr); }
inline int check_launch(const char *) { return SPMV_OK; }
inline int hip_fail(hipError_t, const char *, const char *, int) { return SPMV_ERR_HIP; }
template <class T> struct DevPtr {       // an exactly sized heap block (an empty array: one element, as the library's)
    T *p = nullptr;
    DevPtr() = default;
    DevPtr(DevPtr &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevPtr &operator=(DevPtr &&o) noexcept { T *q = o.p; o.p = nullptr; free(p); p = q; return *this; }
    ~DevPtr() { free(p); }
    T *get() const { return p; }
    operator T *() const { return p; }
    hipError_t alloc(size_t n) { free(p); p = (T *)malloc(sizeof(T) * (n ? n : 1)); return p ? hipSuccess : 1; }
    hipError_t reset() { free(p); p = nullptr; return hipSuccess; }
};
struct TrsvStep { int32_t first = 0, last = 0; bool merged = false; };
struct TrsvPlan {
    bool ready = false;
    int64_t levels = 0, widest = 0, bad_diag_row = -1, nsteps = 0;
    int thin = 0, cap = 0;
    DevPtr<int32_t> d_order, d_level_ptr, d_diag;
    std::vector<int32_t> host_level_ptr;
    std::vector<TrsvStep> host_steps;
    int32_t *level_ptr = nullptr;
    TrsvStep *steps = nullptr;
};
struct Ilu0Plan { bool ready = false; int64_t a_rows = 0, a_nnz = 0; DevPtr<int32_t> d_pivot; };
}
struct spmv_csr { int64_t rows = 0, cols = 0, nnz = 0; const int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr; const float *d_vals = nullptr;
    spmv::DevPtr<int32_t> own_row_ptr, own_col_idx; spmv::DevPtr<float> own_vals; int device = 0;
    spmv::TrsvPlan plan_trsv[2]; spmv::Ilu0Plan plan_ilu0; };
inline int spmv_csr_destroy(spmv_csr_t *h) { delete h; return SPMV_OK; }
namespace spmv {
inline int64_t trsv_plan_bytes(const TrsvPlan &p, int64_t rows) { return p.ready ? 12 * rows + 4 * (p.levels + 1) + 4 : 0; }
inline int trsv_solve(const spmv_csr &, bool, bool, const float *, float *, hipStream_t) { return SPMV_OK; }
inline int trsv_plan(spmv_csr &h, bool upper, int thin_rows, hipStream_t)
{
    const int64_t n = h.rows, nnz = h.nnz;
    TrsvPlan &p = h.plan_trsv[upper ? 1 : 0];
    p = TrsvPlan();
    p.thin = thin_rows > 0 ? thin_rows : SPMV_TRSV_THIN_DEFAULT;
    p.cap = SPMV_TRSV_LEVEL_CAP;
    std::vector<int32_t> level((size_t)n, 0);
    if (p.d_diag.alloc((size_t)n) || p.d_order.alloc((size_t)n)) return SPMV_ERR_HIP;
    int64_t levels = 0;
    for (int64_t step = 0; step < n; ++step) {
        const int64_t i = upper ? n - 1 - step : step;
        const int64_t hi = std::min<int64_t>((uint32_t)h.d_row_ptr[i + 1], nnz), lo = std::min<int64_t>((uint32_t)h.d_row_ptr[i], hi);
        int32_t dpos = -1, ndiag = 0;
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t c = h.d_col_idx[s];
            if (c == i) { if (ndiag++ == 0) dpos = (int32_t)s; }
            else if (upper ? (c > i && c < n) : (c >= 0 && c < i)) level[i] = std::max(level[i], level[c] + 1);
        }
        p.d_diag.get()[i] = dpos;
        if (ndiag != 1 && (p.bad_diag_row < 0 || i < p.bad_diag_row)) p.bad_diag_row = i;
        levels = std::max<int64_t>(levels, level[i] + 1);
    }
    p.levels = levels;
    p.host_level_ptr.assign((size_t)levels + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++p.host_level_ptr[level[i] + 1];
    for (int64_t k = 0; k < levels; ++k) { p.widest = std::max<int64_t>(p.widest, p.host_level_ptr[k + 1]); p.host_level_ptr[k + 1] += p.host_level_ptr[k]; }
    std::vector<int32_t> at(p.host_level_ptr.begin(), p.host_level_ptr.end());
    for (int64_t i = 0; i < n; ++i) p.d_order.get()[at[level[i]]++] = (int32_t)i;
    if (p.d_level_ptr.alloc((size_t)levels + 1)) return SPMV_ERR_HIP;
    for (int64_t k = 0; k <= levels; ++k) p.d_level_ptr.get()[k] = p.host_level_ptr[k];
    for (int64_t k = 0; k < levels;) {
        TrsvStep st;
        st.first = (int32_t)k;
        if ((int64_t)p.host_level_ptr[k + 1] - p.host_level_ptr[k] > p.thin) { st.merged = false; ++k; }
        else {
            st.merged = true;
            const int64_t stop = std::min<int64_t>(k + p.cap, levels);
            while (k < stop && (int64_t)p.host_level_ptr[k + 1] - p.host_level_ptr[k] <= p.thin) ++k;
        }
        st.last = (int32_t)k;
        p.host_steps.push_back(st);
    }
    p.level_ptr = p.host_level_ptr.data();
    p.steps = p.host_steps.data();
    p.nsteps = (int64_t)p.host_steps.size();
    p.ready = true;
    return SPMV_OK;
}
}
