#pragma once
// tools/add_lockstep: just enough of the HIP kernel language to run csrc/kernels_add.hip on the host.  The work-items of a
// workgroup are dealt over kEmuThreads std::threads (work-item t, t + kEmuThreads, ...); the workgroups of a launch run one
// after the other inside each.  The kernels of the sparse sum have no ballot, shuffle, barrier or LDS, so the work-items
// need nothing from each other and any interleaving is a valid one; the one word several work-items may store
// (k_add_sorted's flag) is stored with the compiler's own __hip_atomic_store, on the host too.  Device memory is plain malloc
// memory, so AddressSanitizer sees every access.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
using std::max;
using std::min;
struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef int hipError_t;
typedef void *hipStream_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { std::memset(p, v, n); return 0; }
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return 0; }
struct Idx { unsigned x = 0, y = 0, z = 0; };
inline thread_local Idx threadIdx, blockIdx, gridDim;
#ifndef __HIP_MEMORY_SCOPE_AGENT
#define __HIP_MEMORY_SCOPE_AGENT 4
#endif
inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }     // one rounding, never contracted into a later add
constexpr unsigned kEmuThreads = 8;
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    if (grid.x == 0 || block.x == 0) { std::fprintf(stderr, "a launch of no workgroups: invalid configuration argument\n"); std::abort(); }
    std::vector<std::thread> ts;
    for (unsigned t0 = 0; t0 < kEmuThreads; ++t0)
        ts.emplace_back([&, t0] {
            gridDim.x = grid.x;
            for (unsigned b = 0; b < grid.x; ++b)
                for (unsigned t = t0; t < block.x; t += kEmuThreads) {
                    blockIdx.x = b;
                    threadIdx.x = t;
                    kernel(args...);
                }
        });
    for (auto &th : ts) th.join();
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)
