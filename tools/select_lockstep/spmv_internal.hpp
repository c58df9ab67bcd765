#pragma once
// tools/select_lockstep: the few names of csrc/spmv_internal.hpp that csrc/lane_group.hpp, csrc/kernels_select.hip and csrc/kernels_map.hip use,
// without HIP; csrc/attention_args.hpp is the real one, copied beside this file
#include <hip/hip_runtime.h>
#include "attention_args.hpp"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>
enum { SPMV_OK = 0, SPMV_ERR_INVALID = -2 };
#define SPMV_HIP_TRY(call) do { if ((call) != hipSuccess) return -3; } while (0)
#define SPMV_LAUNCHED(name) if (hipGetLastError() != hipSuccess) return -3
namespace spmv {
constexpr int kWave = 64; constexpr int kBlock = 256; constexpr int kXcds = 8; constexpr int kMaxHeads = 65535;
inline void set_error(const char *f, ...) { va_list a; va_start(a, f); vfprintf(stderr, f, a); va_end(a); }
inline int hip_fail(hipError_t, const char *, const char *, int) { return -3; }
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
};
struct SpmmPlan { bool ready = true; int n_long = 0, pieces = 0, row_cap = 512, piece_len = 512;
    DevPtr<int32_t> d_order, d_long_row, d_long_first, d_piece_k0, d_piece_len; DevPtr<float> d_partial; };
struct AttnPlan { bool ready = false; int heads = 0; DevPtr<float> d_scratch; int wide_heads = 0; DevPtr<float> d_scratch_wide; };
// the handle's position map and its one move (csrc/spmv_internal.hpp; csrc/kernels_map.hip is the real one, copied beside this file)
enum class MapMaker { none = 0, transpose, select, permute };
struct PosMap { DevPtr<uint32_t> words; int64_t parent_len = 0; MapMaker maker = MapMaker::none; };
int map_move(const PosMap &map, int64_t n, bool scatter, int count, const void *src, int64_t src_stride, void *dst, int64_t dst_stride,
             hipStream_t s);
}
struct spmv_csr { int64_t rows = 0, cols = 0, nnz = 0; const int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr; const float *d_vals = nullptr;
    spmv::DevPtr<int32_t> own_row_ptr, own_col_idx; spmv::DevPtr<float> own_vals; spmv::PosMap map;
    int device = 0; spmv::SpmmPlan plan_spmm; spmv::AttnPlan plan_attn; };
typedef spmv_csr spmv_csr_t;
namespace spmv {
inline int plan_spmm(spmv_csr &, hipStream_t) { return SPMV_OK; }
inline int64_t spmm_plan_bytes(const spmv_csr &) { return 0; }
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
