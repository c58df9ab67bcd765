#pragma once
// tools/attention_lockstep: just enough of the HIP kernel language to run csrc/kernels_attention.hip on the host.  One
// std::thread per work-item of a workgroup.  The kernels shuffle only inside a group of V lanes, and every shuffle
// sits in group-uniform control flow, so __shfl / __shfl_xor exchange through a per-group array between two barriers of
// g_group_lanes threads (main sets it to the V of the launch).  Device memory is plain malloc memory, so AddressSanitizer
// sees every access; float4 and float2 carry their device alignment, so UBSan sees a misaligned vector access.
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static      // (a lane touches only slots of its own, and thread t is lane t of every block it runs)
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
inline int g_group_lanes = 1;
struct GroupCtx { std::barrier<> bar; uint64_t slot[64]; explicit GroupCtx(int n) : bar(n) {} };
struct Idx { unsigned x = 0, y = 0, z = 0; };
inline thread_local Idx threadIdx, blockIdx, gridDim;
inline thread_local GroupCtx *g_group = nullptr;
template <class T> T __shfl(T v, int src)
{
    const int mask = g_group_lanes - 1;
    uint64_t raw = 0; std::memcpy(&raw, &v, sizeof(T));
    g_group->slot[threadIdx.x & mask] = raw;
    g_group->bar.arrive_and_wait();
    uint64_t got = g_group->slot[src & mask];
    g_group->bar.arrive_and_wait();
    T out; std::memcpy(&out, &got, sizeof(T));
    return out;
}
template <class T> T __shfl_xor(T v, int m) { return __shfl(v, (int)(threadIdx.x & 63) ^ m); }
// One thread per work-item of a workgroup, started once per launch: thread t runs work-item t of every block of the grid in
// turn (x fastest, then y, then z, as the device dispatches them).  Blocks do not talk to each other and a group's exits are group-uniform, so
// the groups may run ahead of one another; the lanes of one group meet at their shuffles.
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    std::vector<std::unique_ptr<GroupCtx>> groups;
    for (unsigned g = 0; g < block.x / g_group_lanes; ++g) groups.emplace_back(new GroupCtx(g_group_lanes));
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < block.x; ++t)
        ts.emplace_back([&, t] {
            threadIdx.x = t;
            g_group = groups[t / g_group_lanes].get();
            gridDim.x = grid.x, gridDim.y = grid.y, gridDim.z = grid.z;
            for (unsigned z = 0; z < grid.z; ++z)
                for (unsigned y = 0; y < grid.y; ++y)
                    for (unsigned b = 0; b < grid.x; ++b) {
                        blockIdx.x = b, blockIdx.y = y, blockIdx.z = z;
                        kernel(args...);
                    }
        });
    for (auto &th : ts) th.join();
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)
