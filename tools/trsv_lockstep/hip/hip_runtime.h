#pragma once
// tools/trsv_lockstep: just enough of the HIP kernel language to run csrc/kernels_trsv.hip on the host.  A workgroup is
// block.x std::threads, one per work-item, alive together: __syncthreads() is a std::barrier over them, and the wavefront
// collectives the kernels use (__ballot, __shfl, __shfl_down) exchange through a slot per lane between two barriers over
// the 64 threads of the wavefront.  A work-item that returns leaves both barriers, so the others never wait for it.  The
// workgroups of a launch run one after the other; __shared__ variables are function-local statics, which is one copy per
// workgroup because of that.  Atomics are the compiler's own.  Device memory is plain malloc memory, so AddressSanitizer
// sees every access.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef int hipError_t;
typedef void *hipStream_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { std::memset(p, v, n); return 0; }
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return 0; }
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { std::memcpy(d, s, n); return 0; }
struct Idx { unsigned x = 0, y = 0, z = 0; };
inline thread_local Idx threadIdx, blockIdx, gridDim;

constexpr int kEmuWave = 64;
struct EmuWave {
    std::barrier<> bar;
    uint32_t slot[kEmuWave] = {};
    explicit EmuWave(int lanes) : bar(lanes) {}
};
struct EmuBlock {
    std::barrier<> bar;
    explicit EmuBlock(int threads) : bar(threads) {}
};
inline thread_local EmuWave *emu_wave = nullptr;
inline thread_local EmuBlock *emu_block = nullptr;
inline thread_local int emu_lane = 0;

inline void __syncthreads() { emu_block->bar.arrive_and_wait(); }
inline unsigned long long __ballot(bool p)
{
    emu_wave->slot[emu_lane] = p ? 1u : 0u;
    emu_wave->bar.arrive_and_wait();
    unsigned long long m = 0;
    for (int i = 0; i < kEmuWave; ++i) m |= (unsigned long long)(emu_wave->slot[i] & 1u) << i;
    emu_wave->bar.arrive_and_wait();
    return m;
}
template <class T> inline T __shfl(T v, int src)
{
    static_assert(sizeof(T) == 4, "32-bit lanes");
    std::memcpy(&emu_wave->slot[emu_lane], &v, 4);
    emu_wave->bar.arrive_and_wait();
    T r;
    std::memcpy(&r, &emu_wave->slot[src & (kEmuWave - 1)], 4);
    emu_wave->bar.arrive_and_wait();
    return r;
}
template <class T> inline T __shfl_down(T v, int delta) { return __shfl(v, emu_lane + delta < kEmuWave ? emu_lane + delta : emu_lane); }
inline int __ffsll(unsigned long long m) { return __builtin_ffsll((long long)m); }
inline int32_t atomicAdd(int32_t *p, int32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline int32_t atomicSub(int32_t *p, int32_t v) { return __atomic_fetch_sub(p, v, __ATOMIC_RELAXED); }
inline int32_t atomicMin(int32_t *p, int32_t v)
{
    int32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}

inline long emu_launches = 0;
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    if (grid.x == 0 || block.x == 0 || block.x % kEmuWave != 0) {
        std::fprintf(stderr, "a launch of no workgroups (or of part of a wavefront): invalid configuration argument\n");
        std::abort();
    }
    ++emu_launches;
    for (unsigned b = 0; b < grid.x; ++b) {
        EmuBlock blk((int)block.x);
        std::vector<std::unique_ptr<EmuWave>> waves;
        for (unsigned w = 0; w < block.x / kEmuWave; ++w) waves.push_back(std::make_unique<EmuWave>(kEmuWave));
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t)
            ts.emplace_back([&, t] {
                gridDim.x = grid.x;
                blockIdx.x = b;
                threadIdx.x = t;
                emu_block = &blk;
                emu_wave = waves[t / kEmuWave].get();
                emu_lane = (int)(t % kEmuWave);
                kernel(args...);
                emu_wave->bar.arrive_and_drop();
                blk.bar.arrive_and_drop();
            });
        for (auto &th : ts) th.join();
    }
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)
