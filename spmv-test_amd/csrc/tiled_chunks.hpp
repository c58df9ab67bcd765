// tiled_chunks.hpp -- what the plan (plan_adaptive.hip) and the run kernels (kernels_adaptive.hip) of SPMV_ADAPTIVE / SPMV_TILED
// both need: the chunk geometry, the bits of a chunk's window word, the layout of the sorted words and of the block lists.
// The SPMV_T_* macros exist for A/B builds (tools/build_variant.sh); the shipped values are the defaults.  Both files read
// SPMV_T_BLKBITS (here) and SPMV_T_NPT (spmv_internal.hpp): such a build compiles both with them.
#pragma once
#include <type_traits>
#include "spmv_internal.hpp"

namespace spmv {

using i4 = int __attribute__((ext_vector_type(4)));
using f4 = float __attribute__((ext_vector_type(4)));
using u4 = unsigned __attribute__((ext_vector_type(4)));

#ifndef SPMV_T_GROUP
#define SPMV_T_GROUP 16
#endif
constexpr int kGroup = SPMV_T_GROUP;  // lanes that share one long segment

__host__ __device__ constexpr int chunk_of(int block) { return block * kNnzPerThread; }
__host__ __device__ constexpr int prod_words(int block) { return chunk_of(block) + (chunk_of(block) >> 5); }
// LDS region per workgroup: the padded product buffer (4224 floats per 256 threads) rounded up to
// what still lets 2048 threads share a CU's 160 KiB next to the segment queues (1.1 KiB per 256
// threads): 4832 / 9664 / 19328 floats.
__host__ __device__ constexpr int region_words(int block) { return (block / 256) * 4832; }
static_assert(region_words(256) >= prod_words(256), "region must hold the products");
__host__ __device__ constexpr int max_long(int block) { return chunk_of(block) / (kShortSeg + 1) + 2; }
#ifndef SPMV_T_HUGE
#define SPMV_T_HUGE 512
#endif
constexpr int kHugeSeg = SPMV_T_HUGE;  // segments longer than this are summed by one wavefront each
__host__ __device__ constexpr int max_huge(int block) { return chunk_of(block) / (kHugeSeg + 1) + 2; }

// f(std::integral_constant<int, B>{}) for the workgroup size B of a plan, 256 | 512 | 1024 threads (what build_plan admits)
template <typename F>
int dispatch_block(int block, F &&f)
{
    if (block == 256) return f(std::integral_constant<int, 256>{});
    if (block == 512) return f(std::integral_constant<int, 512>{});
    return f(std::integral_constant<int, 1024>{});
}

// The window word of chunk c, written by the plan and read by the run kernels (what k_plan_windows stages where is stated there):
//   win[2c]   = first staged column w0 (multiple of 4)
//   win[2c+1] = staged length wlen in floats (0 = nothing staged) | the bits below
constexpr int kOutsideBit = 1 << 30;   // some of the chunk's columns lie outside [w0, w0+wlen) and are gathered from global memory
constexpr int kCol16Bit = 1 << 29;   // the chunk's columns also exist as 16-bit offsets from w0 (plan.d_col16)
constexpr int kBlockBit = 1 << 28;   // ... as 16-bit indices into a LIST of staged 256-column blocks (plan.d_blk)
constexpr int kSortedBit = 1 << 27;  // nothing is staged: the chunk gathers x in COLUMN order (plan.d_perm), see sorted_body
constexpr int kLenMask = kSortedBit - 1;
#ifndef SPMV_T_SORTED_FROM
#define SPMV_T_SORTED_FROM (-1)   // -1: staged or sorted by modelled cost, per chunk
#endif
constexpr int kSortedFromDefault = SPMV_T_SORTED_FROM;
// Sorted chunks: one 32-bit word per nonzero = position in the chunk (log2(chunk) bits, high) | column - w0 (the rest,
// 18 bits: the plan's counting sort keeps one LDS counter per 128-byte line of the span).
__host__ __device__ constexpr int sorted_pos_bits(int block) { return block == 1024 ? 14 : (block == 512 ? 13 : 12); }
__host__ __device__ constexpr int sorted_col_bits(int) { return 18; }   // 8192 lines = 32 KiB of counters in the plan kernel
static_assert(sorted_pos_bits(1024) + sorted_col_bits(1024) <= 32, "one word per nonzero");
// The order of the mixed launch (k_tiled_mixed).  Lists: the 32-bit chunks first, then the sorted, then the 16-bit ones, each
// kind through its chunk list.  Identity: workgroup b takes chunk xcd_chunk(b) whatever its kind and reads no list -- the value
// loads leave before anything about the chunk is known -- but the slow chunks no longer start first.  The plan takes identity
// where at most one chunk in kIdentityShare is not a 16-bit one (0: never; SPMV_TILED_ORDER overrides at plan time).
#ifndef SPMV_T_IDENTITY_SHARE
#define SPMV_T_IDENTITY_SHARE 8
#endif
constexpr int kIdentityShare = SPMV_T_IDENTITY_SHARE;
#ifndef SPMV_T_IDENTITY_ORDER
#define SPMV_T_IDENTITY_ORDER 1   // 0: the identity order is not compiled in -- plan and kernel as they were without it (A/B)
#endif
constexpr bool kIdentityOrder = SPMV_T_IDENTITY_ORDER != 0;
// When the 16-bit body issues the x window of a one-pass chunk.  0: behind the row bounds, whose branch ends in an s_waitcnt
// vmcnt(0), so the window leaves when the stream has landed.  1: right behind the stream loads, the bounds last (A/B: slower on
// the headline).
#ifndef SPMV_T_WINDOW_FIRST
#define SPMV_T_WINDOW_FIRST 0
#endif
constexpr bool kWindowFirst = SPMV_T_WINDOW_FIRST != 0;
#ifndef SPMV_T_BLKBITS
#define SPMV_T_BLKBITS 8
#endif
constexpr int kBlkBits = SPMV_T_BLKBITS;
constexpr int kBlkCols = 1 << kBlkBits;      // columns per staged block (256: one 1-KiB LDS-DMA piece per wave)
constexpr int kBlkMax = 65536 / kBlkCols;    // blocks per chunk: 65 536 staged floats is what a 16-bit index reaches

// Modelled time of one full chunk, in 1/1024 of the time a chunk of that size takes to stream 8 bytes per nonzero with
// cache-resident gathers.  Fitted on one MI355X to c4 with bands of 8192 ... 200 000 columns and to c3, both workgroup
// sizes, every chunk forced staged and forced sorted (tools/exp/r02_calibrate.json -> profiles/r02_plan_calibration.jsonl;
// DESIGN.md section 4):
//   staged, 16-bit columns                 0.77 + 0.107 per pass            (1 ... 7 passes, 512 and 1024 threads)
//   staged, 32-bit columns (span >= 65536)  1.05 + 0.12  per pass
//   sorted                                  1.05 + 1.75 (512 threads) | 1.45 (1024) x 128-byte lines of the span per nonzero
//   sorted, <= 16 rows in the chunk         0.2 less: the inside of a long row whose columns ascend is an (almost)
//                                           identity permutation -- the LDS scatter is conflict-free
//   gathers from L2/fabric unsorted         3
struct PlanCost {
    int c16_base = 788, c16_pass = 110, c32_base = 1075, c32_pass = 123, sorted_base = 1075, sorted_line_512 = 1792,
        sorted_line_1024 = 1485, sorted_few_rows = 205, unstaged = 3072, long_piece = 512;
};

// The window pass of a TILED plan over the chunks of `p` (k_plan_windows; d_stats: six words, see build_plan).  The kernel is the
// one plan kernel that lives in kernels_adaptive.hip: its reductions go through the same __shfl_down as the run kernels' row
// sums, and compiled in a file without those it came out as other instructions ("Which file holds what").
int launch_plan_windows(const spmv_csr &h, const ChunkPlan &p, int32_t *d_stats, const PlanCost &cost, hipStream_t s);

}  // namespace spmv
