#pragma once
// tools/spgemm_lockstep: just enough of the HIP kernel language to run csrc/kernels_spgemm.hip on the host.  One std::thread
// per work-item of a workgroup (up to 1024).  Every ballot and shuffle of those kernels sits in wavefront-uniform control flow, so
// the 64 lanes of a wavefront exchange through a per-wavefront array between two barriers; __syncthreads is a barrier of the
// workgroup, and the workgroups of a launch run one after the other (the __shared__ arrays are statics).  Device memory is
// plain malloc memory, so AddressSanitizer sees every access; so is the dynamic LDS of a launch (SPG_DYNAMIC_LDS): an exactly
// sized heap block of the bytes the launch asks for.  A wave barrier is a barrier of the wavefront's 64 threads, a fence
// nothing (the barriers order everything), an atomic load or store of wavefront scope a relaxed one.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
using std::max;
using std::min;
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(8) float2 { float x, y; };
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline float2 make_float2(float x, float y) { return float2{x, y}; }
struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef int hipError_t;
typedef void *hipStream_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { std::memset(p, v, n); return 0; }
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return 0; }
struct WaveCtx { std::barrier<> bar{64}; uint64_t slot[64]; };
struct Idx { unsigned x = 0, y = 0, z = 0; };
inline thread_local Idx threadIdx, blockIdx, gridDim;
inline thread_local WaveCtx *g_wave = nullptr;
inline std::barrier<> *g_block_bar = nullptr;
inline int emu_lane() { return (int)(threadIdx.x & 63); }
template <class T> T __shfl(T v, int src, int = 64)
{
    uint64_t raw = 0; std::memcpy(&raw, &v, sizeof(T));
    g_wave->slot[emu_lane()] = raw;
    g_wave->bar.arrive_and_wait();
    uint64_t got = g_wave->slot[src & 63];
    g_wave->bar.arrive_and_wait();
    T out; std::memcpy(&out, &got, sizeof(T));
    return out;
}
template <class T> T __shfl_xor(T v, int m, int = 64) { return __shfl(v, emu_lane() ^ m); }
template <class T> T __shfl_up(T v, int o, int = 64) { return __shfl(v, emu_lane() >= o ? emu_lane() - o : emu_lane()); }
inline uint64_t __ballot(bool p)
{
    g_wave->slot[emu_lane()] = p ? 1u : 0u;
    g_wave->bar.arrive_and_wait();
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)(g_wave->slot[l] & 1u) << l;
    g_wave->bar.arrive_and_wait();
    return m;
}
inline int __popcll(uint64_t v) { return __builtin_popcountll(v); }
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
inline void emu_wave_barrier() { g_wave->bar.arrive_and_wait(); }
#define __builtin_amdgcn_wave_barrier emu_wave_barrier
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#ifndef __HIP_MEMORY_SCOPE_WAVEFRONT
#define __HIP_MEMORY_SCOPE_WAVEFRONT 2      // (__hip_atomic_load / __hip_atomic_store are the compiler's own builtins, on the host too)
#endif
inline int *g_dyn_lds = nullptr;
#define SPG_DYNAMIC_LDS(name) int *name = g_dyn_lds
inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline int emu_mbcnt_lo(unsigned, unsigned v) { return (int)v + std::min(emu_lane(), 32); }
inline int emu_mbcnt_hi(unsigned, unsigned v) { return (int)v + std::max(emu_lane() - 32, 0); }
#define __builtin_amdgcn_mbcnt_lo emu_mbcnt_lo
#define __builtin_amdgcn_mbcnt_hi emu_mbcnt_hi
#define __builtin_amdgcn_readfirstlane(v) __shfl((int)(v), 0)
// thread t runs work-item t of every block of the grid in turn; the blocks are separated by a barrier of the workgroup
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, size_t lds_bytes, A... args)
{
    std::unique_ptr<char, decltype(&free)> lds((char *)malloc(lds_bytes ? lds_bytes : 1), &free);
    g_dyn_lds = (int *)lds.get();
    std::vector<std::unique_ptr<WaveCtx>> waves;
    for (unsigned w = 0; w < block.x / 64; ++w) waves.emplace_back(new WaveCtx());
    std::barrier<> block_bar((std::ptrdiff_t)block.x);
    g_block_bar = &block_bar;
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < block.x; ++t)
        ts.emplace_back([&, t] {
            threadIdx.x = t;
            g_wave = waves[t / 64].get();
            gridDim.x = grid.x;
            gridDim.y = grid.y;
            for (unsigned by = 0; by < grid.y; ++by)
                for (unsigned b = 0; b < grid.x; ++b) {
                    blockIdx.x = b;
                    blockIdx.y = by;
                    kernel(args...);
                    block_bar.arrive_and_wait();
                }
        });
    for (auto &th : ts) th.join();
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, (size_t)(sh), __VA_ARGS__)
