#pragma once
// tools/attention_lockstep: the few names of csrc/spmv_internal.hpp that csrc/lane_group.hpp, csrc/kernels_attention.hip and
// csrc/kernels_sddmm.hip use, without HIP; csrc/attention_args.hpp (AttnArgs, AttnPass) is the real one, copied beside this file
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
template <class T> struct DevPtr {       // (exactly sized heap blocks; freed by main through free_all)
    T *p = nullptr;
    T *get() const { return p; }
    operator T *() const { return p; }
    hipError_t alloc(size_t n) { free(p); p = (T *)malloc(sizeof(T) * (n ? n : 1)); return p ? hipSuccess : 1; }
};
struct SpmmPlan { bool ready = true; int n_long = 0, pieces = 0, row_cap = 512, piece_len = 512;
    DevPtr<int32_t> d_order, d_long_row, d_long_first, d_piece_k0, d_piece_len; DevPtr<float> d_partial; };
struct AttnPlan { bool ready = false; int heads = 0; DevPtr<float> d_scratch; int wide_heads = 0; DevPtr<float> d_scratch_wide; };
}
struct spmv_csr { int64_t rows = 0, cols = 0, nnz = 0; const int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr;
    spmv::SpmmPlan plan_spmm; spmv::AttnPlan plan_attn; };
namespace spmv {
inline int plan_spmm(spmv_csr &, hipStream_t) { return SPMV_OK; }       // (main builds it)
inline int64_t spmm_plan_bytes(const spmv_csr &) { return 0; }
}
