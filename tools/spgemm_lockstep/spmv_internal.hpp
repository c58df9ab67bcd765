#pragma once
// tools/spgemm_lockstep: the few names of csrc/spmv_internal.hpp that csrc/kernels_spgemm.hip uses, without HIP; include/spmv_hip.h
// is the real one, copied beside this file
#include <hip/hip_runtime.h>
#include "spmv_hip.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>
#define SPMV_HIP_TRY(call) do { if ((call) != hipSuccess) return SPMV_ERR_HIP; } while (0)
namespace spmv {
constexpr int kWave = 64; constexpr int kBlock = 256;
inline void set_error(const char *f, ...) { va_list a; va_start(a, f); vfprintf(stderr, f, a); va_end(a); fputc('\n', stderr); }
inline int check_launch(const char *) { return SPMV_OK; }
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
struct LdsOptIn { int ensure(const void *, int, int bytes) { return bytes <= 160 * 1024 ? SPMV_OK : SPMV_ERR_HIP; } };
struct SpgemmPlan { bool ready = false; int64_t inner = 0, a_nnz = 0, b_nnz = 0; int64_t cls[6] = {0, 0, 0, 0, 0, 0}; DevPtr<int32_t> d_order; };
}
struct spmv_csr { int64_t rows = 0, cols = 0, nnz = 0; const int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr; const float *d_vals = nullptr;
    spmv::DevPtr<int32_t> own_row_ptr, own_col_idx; spmv::DevPtr<float> own_vals; int device = 0; spmv::SpgemmPlan plan_spgemm; };
namespace spmv {
// the library's scan (kernels_dense.hip), serial here: d_data[i] = sum of d_data[0 .. i), the total appended and returned
inline int scan_offsets_i32(int32_t *d_data, int64_t n, int32_t *d_total, bool append_total, hipStream_t, int32_t *total_host)
{
    int32_t run = 0;
    for (int64_t i = 0; i < n; ++i) { const int32_t v = d_data[i]; d_data[i] = run; run += v; }
    *d_total = run;
    *total_host = run;
    if (append_total) d_data[n] = run;
    return SPMV_OK;
}
}
