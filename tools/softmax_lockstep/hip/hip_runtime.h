#pragma once
// tools/softmax_lockstep: just enough of the HIP kernel language to run csrc/kernels_softmax.hip on the host.  One
// std::thread per work-item, a workgroup at a time; __shfl / __shfl_xor exchange through a per-wavefront array between two
// barriers, so the 64 lanes of a wavefront run in lockstep wherever the kernel shuffles (every shuffle there sits in
// wavefront-uniform control flow).  Device memory is plain malloc memory, so AddressSanitizer sees every access.
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <memory>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct alignas(16) float4 { float x, y, z, w; };     // (for csrc/lane_group.hpp; the softmax kernels use none)
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1) : x(a) {} };
typedef int hipError_t;
typedef void *hipStream_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
struct WaveCtx { std::barrier<> bar{64}; uint64_t slot[64]; };
struct Idx { unsigned x = 0; };
inline thread_local Idx threadIdx, blockIdx;
inline thread_local WaveCtx *g_wave = nullptr;
template <class T> T __shfl(T v, int src)
{
    const int lane = threadIdx.x & 63;
    uint64_t raw = 0; std::memcpy(&raw, &v, sizeof(T));
    g_wave->slot[lane] = raw;
    g_wave->bar.arrive_and_wait();
    uint64_t got = g_wave->slot[src & 63];
    g_wave->bar.arrive_and_wait();
    T out; std::memcpy(&out, &got, sizeof(T));
    return out;
}
template <class T> T __shfl_xor(T v, int m) { return __shfl(v, (int)(threadIdx.x & 63) ^ m); }
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    for (unsigned b = 0; b < grid.x; ++b) {
        std::vector<std::unique_ptr<WaveCtx>> waves;
        for (unsigned w = 0; w < block.x / 64; ++w) waves.emplace_back(new WaveCtx);
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t)
            ts.emplace_back([&, t] { threadIdx.x = t; blockIdx.x = b; g_wave = waves[t / 64].get(); kernel(args...); g_wave->bar.arrive_and_drop(); });
        for (auto &th : ts) th.join();
    }
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)
