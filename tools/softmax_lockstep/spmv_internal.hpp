#pragma once
// tools/softmax_lockstep: the few names of csrc/spmv_internal.hpp that csrc/kernels_softmax.hip and csrc/lane_group.hpp use,
// without HIP
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdarg>
enum { SPMV_OK = 0, SPMV_ERR_INVALID = -2 };
#define SPMV_LAUNCHED(name) if (hipGetLastError() != hipSuccess) return -3
namespace spmv {
constexpr int kWave = 64; constexpr int kBlock = 256; constexpr int kXcds = 8; constexpr int kMaxHeads = 65535;
inline void set_error(const char *f, ...) { va_list a; va_start(a, f); vfprintf(stderr, f, a); va_end(a); }
inline int hip_fail(hipError_t, const char *, const char *, int) { return -3; }
template <class T> struct DevPtr { T *p = nullptr; T *get() const { return p; } };
struct SpmmPlan { bool ready = true; int n_long = 0, pieces = 0, row_cap = 512, piece_len = 512;
    DevPtr<int32_t> d_order, d_long_row, d_long_first, d_piece_k0, d_piece_len; DevPtr<float> d_partial; };
}
struct spmv_csr { int64_t rows = 0, cols = 0, nnz = 0; const int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr; spmv::SpmmPlan plan_spmm; };
