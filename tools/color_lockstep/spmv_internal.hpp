#pragma once
// tools/color_lockstep: the few names of csrc/spmv_internal.hpp that csrc/kernels_color.hip, csrc/kernels_permute.hip and csrc/kernels_map.hip use,
// without HIP (hip/hip_runtime.h is the stub of tools/trsv_lockstep); include/spmv_hip.h is the real one, copied beside this
// file.  The scan, the column range and the transpose (other files of the library) are serial statements of their contracts.
#include <hip/hip_runtime.h>
#include "spmv_hip.h"
#include <cstdarg>
#include <cstdio>
#include <numeric>
#include <utility>
#define SPMV_HIP_TRY(call) do { if ((call) != hipSuccess) return SPMV_ERR_HIP; } while (0)
inline int32_t atomicMax(int32_t *p, int32_t v)
{
    int32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
namespace spmv {
constexpr int kWave = 64; constexpr int kBlock = 256;
inline bool g_quiet = false;             // the refusals of never-validated operands are expected: not printed
inline char g_last[512] = "";
inline void set_error(const char *f, ...)
{
    va_list a;
    va_start(a, f);
    vsnprintf(g_last, sizeof g_last, f, a);
    va_end(a);
    if (!g_quiet) { fputs(g_last, stderr); fputc('\n', stderr); }
}
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
// the handle's position map and its one move (csrc/spmv_internal.hpp; csrc/kernels_map.hip is the real one, copied beside this file)
enum class MapMaker { none = 0, transpose, select, permute };
struct PosMap { DevPtr<uint32_t> words; int64_t parent_len = 0; MapMaker maker = MapMaker::none; };
int map_move(const PosMap &map, int64_t n, bool scatter, int count, const void *src, int64_t src_stride, void *dst, int64_t dst_stride,
             hipStream_t s);
}
struct spmv_csr { int64_t rows = 0, cols = 0, nnz = 0; const int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr; const float *d_vals = nullptr;
    spmv::DevPtr<int32_t> own_row_ptr, own_col_idx; spmv::DevPtr<float> own_vals; spmv::PosMap map; int device = 0; };
inline int spmv_csr_destroy(spmv_csr_t *h) { delete h; return SPMV_OK; }
namespace spmv {
// the library's scan (kernels_dense.hip), serial here: d_data[i] = sum of d_data[0 .. i), the total appended and returned
inline int scan_offsets_i32(int32_t *d_data, int64_t n, int32_t *d_total, bool append_total, hipStream_t, int32_t *total_host)
{
    uint32_t run = 0;
    for (int64_t i = 0; i < n; ++i) { const uint32_t v = (uint32_t)d_data[i]; d_data[i] = (int32_t)run; run += v; }
    *d_total = (int32_t)run;
    *total_host = (int32_t)run;
    if (append_total) d_data[n] = (int32_t)run;
    return SPMV_OK;
}
// the library's column range (kernels_rows.hip): d_out2 = {smallest, largest} of col_idx, {INT_MAX, -1} without nonzeros
inline int launch_column_range(const spmv_csr &h, int32_t *d_out2, hipStream_t)
{
    d_out2[0] = 0x7fffffff; d_out2[1] = -1;
    for (int64_t k = 0; k < h.nnz; ++k) { d_out2[0] = std::min(d_out2[0], h.d_col_idx[k]); d_out2[1] = std::max(d_out2[1], h.d_col_idx[k]); }
    return SPMV_OK;
}
// the library's transpose (kernels_transpose.hip) as its header states it: a stable sort of the positions by column.  Like
// the library's it keeps every position whatever the arrays hold and reads nothing outside them: the row of a position is
// found by bisection, and a column out of range sorts as the unsigned number it is and counts in no row of the result.
inline int transpose(const spmv_csr &a, bool keep_map, hipStream_t, spmv_csr_t **out)
{
    std::vector<int32_t> row_of((size_t)a.nnz, 0);
    for (int64_t k = 0; k < a.nnz && a.rows > 0; ++k) {
        int64_t lo = 0, hi = a.rows;
        while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if ((int64_t)a.d_row_ptr[mid] <= k) lo = mid; else hi = mid; }
        row_of[k] = (int32_t)lo;
    }
    std::vector<uint32_t> perm((size_t)a.nnz);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return (uint32_t)a.d_col_idx[x] < (uint32_t)a.d_col_idx[y]; });
    spmv_csr *t = new spmv_csr();
    t->rows = a.cols; t->cols = a.rows; t->nnz = a.nnz;
    if (t->own_row_ptr.alloc((size_t)t->rows + 1) || t->own_col_idx.alloc(perm.size()) || t->own_vals.alloc(perm.size()) ||
        t->map.words.alloc(perm.size())) { delete t; return SPMV_ERR_HIP; }
    for (int64_t r = 0; r <= t->rows; ++r) t->own_row_ptr.get()[r] = 0;
    for (uint32_t k : perm)
        if (a.d_col_idx[k] >= 0 && a.d_col_idx[k] < a.cols) ++t->own_row_ptr.get()[a.d_col_idx[k] + 1];
    for (int64_t r = 0; r < t->rows; ++r) t->own_row_ptr.get()[r + 1] += t->own_row_ptr.get()[r];
    for (size_t i = 0; i < perm.size(); ++i) {
        t->own_col_idx.get()[i] = row_of[perm[i]];
        std::memcpy(&t->own_vals.get()[i], &a.d_vals[perm[i]], 4);
        t->map.words.get()[i] = perm[i];
    }
    t->d_row_ptr = t->own_row_ptr; t->d_col_idx = t->own_col_idx; t->d_vals = t->own_vals;
    t->map.parent_len = a.nnz; t->map.maker = spmv::MapMaker::transpose;
    if (!keep_map) t->map = spmv::PosMap();
    *out = t;
    return SPMV_OK;
}
}
