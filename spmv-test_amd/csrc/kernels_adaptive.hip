// kernels_adaptive.hip -- nnz-balanced CSR SpMV with LDS staging (SPMV_ADAPTIVE / SPMV_TILED): the run kernels and their launch.
// The plan they run from -- chunk boundaries, column windows, 16-bit columns, sorted words, chunk lists -- is built in
// plan_adaptive.hip; tiled_chunks.hpp holds what both files share.
//
// Role of the reference's adaptive family -- awsp_kernel_v0/1/2
// (/root/reference/src/kernels/awsp.cu:5-317), awsp_ref_kernel (awsp_ref.cu:6-185) -- and of its
// LDS-tiled kernels csr_tiling_kernel (csr_tiling.cu:24-114) / wsp_sm_kernel (wsp_sm.cu:6-211).
// Those walk 32x32 bitmap blocks with 32-lane warps; nothing of that survives here.  Re-derived
// for CSR on CDNA4:
//
//   * Work is split by NONZEROS, not rows: workgroup c streams nonzeros [c*T, (c+1)*T),
//     T = 16 per lane, with 16-byte-per-lane non-temporal loads of col_idx and vals (each wave
//     instruction covers 1 KiB contiguous).  Row lengths never unbalance the HBM stream.
//   * The T products vals[k]*x[col_idx[k]] are staged in LDS (padded one word per 32 so that
//     lane-per-row reads at power-of-two strides spread over the banks).
//   * Rows are then reduced adaptively inside the chunk: segments of <= kShortSeg products are
//     summed by one lane (sequential -> same order as the CPU oracle); longer ones are queued in
//     LDS with their bounds and summed by 16-lane groups with a __shfl_down tree.
//   * A row that crosses chunk boundaries is finished deterministically: every chunk stores the
//     partial sum of the row it inherits in carry[c]; a tiny second kernel adds the carries to
//     the owner's partial in chunk order.  No float atomics (MI355X_MICROARCH.md: atomics run
//     memory-side at ~1.3 TB/s and are order-nondeterministic).
//   * Blocks are dealt round-robin over the 8 XCDs, so blockIdx is remapped to give every XCD one
//     contiguous range of chunks: neighbouring chunks gather from neighbouring parts of x and
//     share that XCD's 4 MiB L2.
//   * TILED stages the chunk's column window of x in LDS and gathers from LDS instead of L1/L2
//     (a 4-byte gather that misses L1 costs a whole L2 request and a 128-byte line).  The window
//     lives in the SAME LDS region the products are written to afterwards, so it costs no
//     occupancy.  The region grows with the workgroup: 256/512/1024 threads hold 4832/9664/19328
//     floats at the same LDS bytes per wave; the plan picks the smallest workgroup whose region
//     covers the windows of >= 90 % of the chunks, and a chunk whose window does not fit
//     gathers from global memory.
//
// The values' element type E.  Every run kernel is a template on it: float (spmv_csr_run: the handle's vals) or bf16 / fp16
// (spmv_csr_run_vals16: a borrowed array of nnz 16-bit elements in the handle's storage order).  A lane keeps its element ->
// lane map -- nonzeros 4 (j BLOCK + tid) .. + 3 for j = 0..3 -- and a 16-bit stream vector is one 8-byte non-temporal load that
// waits packed, two registers, until stage_products widens each element exactly to fp32 (widen16 of lane_group.hpp) for its
// one fp32 multiplication.  The products, their LDS words and every sum are the float kernels': y is, bit for bit,
// spmv_csr_run on the widened values.  The persistent form is float only.
#include "spmv_internal.hpp"
#include "tiled_chunks.hpp"
#include "lane_group.hpp"

namespace spmv {

__device__ __forceinline__ int pad_idx(int i) { return i + (i >> 5); }
// The pad words themselves (slot 32 of every 33) hold 0.0f while the products are in LDS: the row sums then walk the PADDED
// positions [pad_idx(s), pad_idx(e)) of a segment with constant offsets -- no index arithmetic per product, the holes add
// +0.0 (round 3: two vector instructions per LDS read less; the kernel's vector units were busy two thirds of its time).
template <int BLOCK>
__device__ __forceinline__ void zero_pad_words(float *smem, int tid)
{
    for (int h = tid; h < (chunk_of(BLOCK) >> 5); h += BLOCK) smem[h * 33 + 32] = 0.0f;
}

// chunk handled by this block: XCD j = blockIdx % 8 gets a contiguous range
__device__ __forceinline__ int xcd_chunk(int bid, int n)
{
    const int q = n / kXcds, rem = n % kXcds;
    const int j = bid % kXcds, idx = bid / kXcds;
    return j * q + (j < rem ? j : rem) + idx;
}

// ---------------------------------------------------------------------------
// Segment t of chunk c: t = 0 is the head (the row inherited from chunk c-1, summed into
// carry[c]); t = 1..m are the rows that START in this chunk (summed into y).
struct Segment {
    int s, e;
    float *dst;
};

// Static LDS of a workgroup besides the dynamic region.
template <int BLOCK>
struct ChunkShared {
    int2 long_seg[max_long(BLOCK)];  // {segment id, first product | end product << 16}
    int2 huge_seg[max_huge(BLOCK)];
    int long_count, huge_count;
};

// The steps the three bodies share.  They take and return small values: handed a struct or a lane's array of vectors by
// reference, or the whole ChunkHead where a few of its fields do, the compiler chose other registers or addressing in some
// kernel (profiles/tiled_sources_asm.md), so reduce_chunk keeps scalar arguments and the 32-bit body its own bound prefetch.
// What every body reads first about its chunk c: its nonzeros are [base, lim), the m rows lb0 .. lb0 + m - 1 start in it.
struct ChunkHead {
    int c;
    int64_t base, lim;
    int lb0, m;
};

// ... read, and the two segment queues emptied by lane 0.  nnz: where the stream ends (left out by a body that only sees full chunks)
template <int BLOCK>
__device__ __forceinline__ ChunkHead chunk_head(ChunkShared<BLOCK> &sh, int tid, int c, const int32_t *chunk_lb,
                                                int64_t nnz = INT64_MAX)
{
    constexpr int kChunkT = chunk_of(BLOCK);
    ChunkHead h;
    h.c = c;
    h.base = (int64_t)c * kChunkT;
    h.lim = h.base + (int)((nnz - h.base) < kChunkT ? (nnz - h.base) : kChunkT);
    if (tid == 0) { sh.long_count = 0; sh.huge_count = 0; }
    h.lb0 = chunk_lb[c];
    h.m = chunk_lb[c + 1] - h.lb0;
    return h;
}

// the sum of segment t to where it goes
__device__ __forceinline__ void store_sum(int t, int c, int lb0, float *y, float *carry, float acc)
{
    if (t == 0) carry[c] = acc;
    else y[(int64_t)lb0 + t - 1] = acc;
}

// The row pointers that bound the first segment of lane `tid` (rb = row_ptr[lb0] for the head: lb0 <= rows and row_ptr[rows] =
// nnz), read while the stream is in flight: two registers; without them the row phase starts with an exposed L2/HBM round
// trip (+3.4 % at c4, A/B)
struct RowBounds {
    int32_t rb, re;
};

__device__ __forceinline__ RowBounds first_bounds(int tid, const ChunkHead h, const int32_t *row_ptr)
{
    RowBounds b = {0, 0};
    if (tid <= h.m) {
        b.rb = row_ptr[tid == 0 ? h.lb0 : h.lb0 + tid - 1];
        b.re = tid == 0 ? 0 : row_ptr[h.lb0 + tid];
    }
    return b;
}

__device__ __forceinline__ Segment make_segment(int t, int lb0, int64_t base, int64_t lim, int32_t rb, int32_t re,
                                                float *__restrict__ y, float *__restrict__ carry, int c)
{
    Segment g;
    if (t == 0) {  // rb = row_ptr[lb0]
        g.s = 0;
        g.e = (int)(((int64_t)rb < lim ? (int64_t)rb : lim) - base);
        g.dst = carry + c;
    } else {       // rb = row_ptr[r], re = row_ptr[r+1], r = lb0 + t - 1
        g.s = (int)((int64_t)rb - base);
        g.e = (int)(((int64_t)re < lim ? (int64_t)re : lim) - base);
        g.dst = y + ((int64_t)lb0 + t - 1);
    }
    return g;
}

// The j-th 16-byte vector lane tid takes of a stream (values, columns, 16-bit offsets, sorted words) of the chunk that begins
// at `chunk`: elements 4 (j BLOCK + tid) .. + 3 of 32-bit ones; non-temporal (read once), 1 KiB contiguous per wave instruction.
template <int BLOCK, typename V>
__device__ __forceinline__ V stream_load(const V *chunk, int tid, int j)
{
    return __builtin_nontemporal_load(&chunk[j * BLOCK + tid]);
}

// Four values of a lane as they wait in registers between their load and stage_products: f4, or the 8 bytes of four 16-bit
// elements as loaded (element q in half q & 1 of word q >> 1)
using u2 = unsigned __attribute__((ext_vector_type(2)));
template <typename E>
using vals4_t = std::conditional_t<kIs16<E>, u2, f4>;

// the values of the full chunk that begins at element `base`, as the vectors stream_load takes
template <typename E>
__device__ __forceinline__ const vals4_t<E> *value_vectors(const E *__restrict__ vals, int64_t base)
{
    return reinterpret_cast<const vals4_t<E> *>(vals + base);
}

// The products of a chunk into LDS, padded one word per 32 (lane-per-row reads then spread over the banks), the pad words
// zeroed.  x_of(j, q, w): the x that meets element q of value vector j, whose product goes to word w.
// 16-bit values are widened here and nowhere earlier: the packed words pass through an empty statement, so that no float of
// them is alive across the gathers (that would undo the packing: 16 registers instead of 8).
template <int BLOCK, typename E = float, typename X>
__device__ __forceinline__ void stage_products(float *smem, int tid, const vals4_t<E> (&vv)[kNnzPerThread / 4], X x_of)
{
    zero_pad_words<BLOCK>(smem, tid);
#pragma unroll
    for (int j = 0; j < kNnzPerThread / 4; ++j) {
        const int p0 = pad_idx((j * BLOCK + tid) * 4);  // a multiple of 4: the four words never straddle a pad slot
        if constexpr (kIs16<E>) {
            unsigned lo = vv[j][0], hi = vv[j][1];
            asm("" : "+v"(lo));
            asm("" : "+v"(hi));
            const float v[4] = {widen16<E>(lo & 0xffffu), widen16<E>(lo >> 16), widen16<E>(hi & 0xffffu), widen16<E>(hi >> 16)};
#pragma unroll
            for (int q = 0; q < 4; ++q) smem[p0 + q] = v[q] * x_of(j, q, p0 + q);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) smem[p0 + q] = vv[j][q] * x_of(j, q, p0 + q);
        }
    }
}

// acc + the acc of lane + O of the same 16-lane DPP row, in the lanes whose lane + O lies in the row (the others add 0): a row
// shift in the vector unit, v_add_f32_dpp row_shl:O.  __shfl_down is ds_bpermute_b32 -- an address, a trip through the LDS
// crossbar and a wait -- per step.
template <int O>
__device__ __forceinline__ float add_row_shl(float acc)
{
    return acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x100 + O, 0xf, 0xf, true));
}

// Lane 0 of every kGroup-lane group ends with the tree acc += acc[lane + 8], [lane + 4], [lane + 2], [lane + 1]; what the
// other lanes end with is not used.  Lane 0's tree reads lanes 0..15 of its own group only, and the groups of a wave are
// active or idle as a whole, so no source lane of it is ever disabled.  LEAN: the same tree with __shfl_down.
template <bool LEAN>
__device__ __forceinline__ float group_tree(float acc)
{
    if constexpr (!LEAN) {
        static_assert(kGroup == 16, "the DPP tree takes a lane group to be one DPP row (SPMV_T_GROUP is a build knob)");
        acc = add_row_shl<8>(acc);
        acc = add_row_shl<4>(acc);
        acc = add_row_shl<2>(acc);
        return add_row_shl<1>(acc);
    } else {
#pragma unroll
        for (int o = kGroup / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, kGroup);
        return acc;
    }
}

// Words a lane reads ahead of its adds in the row sums.  The reads behind a segment's last word are not clamped: they stay
// inside the workgroup's LDS region, which is kReadAhead words longer than the padded products at every workgroup size, and
// what they return is replaced by +0 before it is added (no partial sum here is ever -0 -- each starts from +0 -- so adding +0
// changes no bit).  The clamped and predicated form gave the same bits and cost a v_min and a v_add per word.
constexpr int kLongBatch = 4;    // words per lane and trip of a kGroup-lane group (A/B: 2 and 8 were no faster)
constexpr int kShortBatch = 16;  // words of a short segment in flight
constexpr int kReadAhead = (kLongBatch - 1) * kGroup > 4 ? (kLongBatch - 1) * kGroup : 4;
static_assert(region_words(256) >= prod_words(256) + kReadAhead && region_words(512) >= prod_words(512) + kReadAhead &&
                  region_words(1024) >= prod_words(1024) + kReadAhead,
              "the unclamped reads of the row sums stay inside the LDS region");

// The row reduction of one chunk, products already staged in `smem` (a barrier behind them):
//   short segments (<= kShortSeg): one lane each, sequential (the oracle's order);
//   longer ones up to kHugeSeg: queued in LDS with their bounds, summed by kGroup-lane groups: lane l adds the padded words
//     l, l + 16, .. of the segment from +0, then the tree of group_tree;
//   longer (a power-law row can fill the chunk): one wavefront each.
// The order of every sum is fixed (tests/_tiled_order.py states it in numpy); how the LDS reads are issued is not part of it:
// a lane reads a batch of words and then adds them, so that one LDS latency is waited for per batch and not per word.
// PREF: this lane's first row bounds were prefetched into rb0/re0.
// LEAN: 0 all of that; 1 the short segments keep their one-batch-at-a-time loop (the 16-bit body with block lists: it
// spills 20 bytes as it is and the read-ahead made that 28 to 36); 2 also the long loop one word at a time and the
// __shfl_down tree (the persistent forms, whose registers hold the next chunk's stream through the row sums: 20 -> 36 bytes
// of scratch otherwise).  profiles/tiled_rowsums_resources.md
// (Round 3, tried and dropped: summing the segments longer than kHugeSeg from the products every lane still holds in
// registers, by all wavefronts at once instead of one wavefront per segment reading LDS.  Slower on power-law rows -- c3 band
// 8192 0.2409 ms against 0.2309, a chunk holds up to 16 such segments and every lane then runs 16 compare-and-adds per
// segment -- and its 2 KiB of partials pushed the 1024-thread workgroup from two per CU to one (band 65 536: 0.49 -> 0.67 ms):
// the static LDS beside the region is budgeted to the last half KiB.  profiles/r03_huge_segments_from_registers_ab.jsonl)
// (Tried and dropped with the read-ahead, profiles/tiled_rowsums_ab.jsonl: the queue entry of the next round read under this
// round's sums and two pairs in flight in the wavefront loop -- both within 0.2 % at c4 and c3; the bounds of a lane's second
// segment prefetched with the stream -- even packed into one more register the 16-bit body then spills 20 bytes, and with
// that spill it ran 8 % slower.)
template <int BLOCK, bool PREF, int LEAN = 0>
__device__ __forceinline__ void reduce_chunk(const float *smem, ChunkShared<BLOCK> &sh, int tid, int c, int lb0, int m,
                                             int64_t base, int64_t lim, const int32_t *__restrict__ row_ptr,
                                             float *__restrict__ y, float *__restrict__ carry, int32_t rb0, int32_t re0)
{
    for (int t = tid; t <= m; t += BLOCK) {
        int32_t rb, re;
        if (PREF && t == tid) { rb = rb0; re = re0; }
        else { rb = row_ptr[t == 0 ? lb0 : lb0 + t - 1]; re = t == 0 ? 0 : row_ptr[lb0 + t]; }
        const Segment g = make_segment(t, lb0, base, lim, rb, re, y, carry, c);
        const int ps = pad_idx(g.s), pe = pad_idx(g.e);     // the segment's words in LDS, pad words (zeros) included
        if (g.e - g.s <= kShortSeg) {
            float acc = 0.0f;
            const float *w = smem + ps;
            const int n = pe - ps;
            if constexpr (LEAN == 0) {
                // left to right from +0: the whole fours, kShortBatch words read before the first of them is added, then
                // the one to three words behind them
                static_assert(kShortSeg <= 32 && kShortBatch % 4 == 0, "a short segment crosses one pad word at most");
                constexpr int kWords = (kShortSeg + 1) & ~3;   // n <= kShortSeg + 1: the whole fours end here
                const int nt = n & ~3;
#pragma unroll
                for (int i0 = 0; i0 < kWords; i0 += kShortBatch) {
                    if (i0 < nt) {
                        float b[kShortBatch];
#pragma unroll
                        for (int i = 0; i < kShortBatch; i += 4)
                            if (i == 0 || i0 + i < nt) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) b[i + q] = w[i0 + i + q];
                            }
#pragma unroll
                        for (int i = 0; i < kShortBatch; i += 4)
                            if (i == 0 || i0 + i < nt) acc = (((acc + b[i]) + b[i + 1]) + b[i + 2]) + b[i + 3];
                    }
                }
                const float *wt = w + nt;
                const float t0 = wt[0], t1 = wt[1], t2 = wt[2];
                acc += nt < n ? t0 : 0.0f;
                acc += nt + 1 < n ? t1 : 0.0f;
                acc += nt + 2 < n ? t2 : 0.0f;
            } else {
                int i = 0;
                for (; i + 3 < n; i += 4) {
                    const float a0 = w[i], a1 = w[i + 1], a2 = w[i + 2], a3 = w[i + 3];
                    acc = (((acc + a0) + a1) + a2) + a3;
                }
                for (; i < n; ++i) acc += w[i];
            }
            *g.dst = acc;
        } else if (g.e - g.s <= kHugeSeg) {
            const int slot = atomicAdd(&sh.long_count, 1);
            sh.long_seg[slot] = make_int2(t, ps | (pe << 16));  // both below 2^15
        } else {
            const int slot = atomicAdd(&sh.huge_count, 1);
            sh.huge_seg[slot] = make_int2(t, ps | (pe << 16));
        }
    }
    __syncthreads();

    const int nlong = sh.long_count;
    const int sub = tid & (kGroup - 1);
    for (int i = tid / kGroup; i < nlong; i += BLOCK / kGroup) {
        const int2 q = sh.long_seg[i];
        const int qe = (int)((unsigned)q.y >> 16);
        float acc = 0.0f;
        if constexpr (LEAN < 2) {
            for (int k = (q.y & 0xffff) + sub; k < qe; k += kLongBatch * kGroup) {
                float v[kLongBatch];
#pragma unroll
                for (int j = 0; j < kLongBatch; ++j) v[j] = smem[k + j * kGroup];
                acc += v[0];
#pragma unroll
                for (int j = 1; j < kLongBatch; ++j) acc += k + j * kGroup < qe ? v[j] : 0.0f;
            }
        } else {
            for (int k = (q.y & 0xffff) + sub; k < qe; k += kGroup) acc += smem[k];
        }
        acc = group_tree<LEAN == 2>(acc);
        if (sub == 0) store_sum(q.x, c, lb0, y, carry, acc);
    }

    // longer segments: one WAVE each, lanes striding the segment (no workgroup barrier: a chunk of a dense-ish
    // matrix is a handful of such rows and the waves take them side by side; a single segment that fills the chunk
    // costs one wave 256 LDS reads per lane)
    const int nhuge = sh.huge_count;
    const int lane = tid & (kWave - 1);
    for (int i = tid >> 6; i < nhuge; i += BLOCK / kWave) {
        const int2 q = sh.huge_seg[i];
        const int qe = (int)((unsigned)q.y >> 16);
        float a0 = 0.0f, a1 = 0.0f;
        int k = (q.y & 0xffff) + lane;
        for (; k + kWave < qe; k += 2 * kWave) {
            a0 += smem[k];
            a1 += smem[k + kWave];
        }
        if (k < qe) a0 += smem[k];
        float acc = a0 + a1;
        // the steps 32 and 16 cross DPP rows; after them lanes 0..15 hold what lane 0's steps 8..1 read
        acc += __shfl_down(acc, 32, kWave);
        acc += __shfl_down(acc, 16, kWave);
        if constexpr (LEAN < 2) {
            acc = group_tree<false>(acc);
        } else {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
        }
        if (lane == 0) store_sum(q.x, c, lb0, y, carry, acc);
    }
}

// The stream of one chunk: 16 B per lane per load (1 KiB contiguous per wave instruction),
// non-temporal (read once), all 8 loads issued back to back.
// (16-bit values: 8 B per lane per value load, 512 B contiguous per wave instruction; the ragged chunk reads them with guarded
// 2-byte loads and a padded lane takes the bits of +0)
template <int BLOCK, bool FULL_ONLY, typename E = float>
__device__ __forceinline__ void load_stream(int64_t base, int n, int pad_col, const int32_t *__restrict__ col_idx,
                                            const E *__restrict__ vals, int tid, i4 (&cc)[kNnzPerThread / 4],
                                            vals4_t<E> (&vv)[kNnzPerThread / 4])
{
    constexpr int kVec = kNnzPerThread / 4;
    if (FULL_ONLY || n == chunk_of(BLOCK)) {
        const i4 *c4 = reinterpret_cast<const i4 *>(col_idx + base);
        const vals4_t<E> *v4 = value_vectors(vals, base);
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            cc[j] = stream_load<BLOCK>(c4, tid, j);
            vv[j] = stream_load<BLOCK>(v4, tid, j);
        }
    } else {
        // last chunk: guarded scalar loads, same element->lane map; padded lanes use an in-window
        // column and value 0 (their products are never read)
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            const int i0 = (j * BLOCK + tid) * 4;
            if constexpr (kIs16<E>) vv[j] = u2{0u, 0u};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool ok = (i0 + q) < n;
                cc[j][q] = ok ? col_idx[base + i0 + q] : pad_col;
                if constexpr (kIs16<E>) vv[j][q >> 1] |= (ok ? (unsigned)bits16(vals)[base + i0 + q] : 0u) << (16 * (q & 1));
                else vv[j][q] = ok ? vals[base + i0 + q] : 0.0f;
            }
        }
    }
}

// Chunk schedule over chunks [chunk0, chunk0 + nrun).
// One-shot (PERSIST = false): workgroup b handles one chunk, xcd_chunk(b), and exits.
// Persistent (PERSIST = true): the grid is sized to what is resident; the workgroups of XCD j walk
// that XCD's contiguous chunk range with stride = workgroups on the XCD, and the stream loads of the
// NEXT chunk are issued as soon as the products of the current one are in LDS, so every wave keeps
// 8 KiB of HBM reads in flight while it reduces rows.  The host hands a persistent launch FULL
// chunks only (the guarded tail loads cost registers); a trailing partial chunk gets a one-shot
// launch of its own.
struct Walk {
    int c, end, stride;
};

__device__ __forceinline__ Walk first_chunk(bool persist, int bid, int grid, int nchunks)
{
    Walk w;
    if (!persist) {
        w.c = xcd_chunk(bid, nchunks);
        w.end = w.c + 1;
        w.stride = 1;
        return w;
    }
    const int j = bid % kXcds, i = bid / kXcds;
    const int q = nchunks / kXcds, rem = nchunks % kXcds;
    const int start = j * q + (j < rem ? j : rem);
    const int cnt = q + (j < rem ? 1 : 0);
    w.stride = grid / kXcds + (j < grid % kXcds ? 1 : 0);  // workgroups that landed on this XCD label
    w.c = start + i;
    w.end = start + cnt;
    return w;
}

// BLOCK/256 workgroups of BLOCK threads fill a CU to the same LDS bytes and waves.  One-shot: the
// second launch-bounds argument keeps the kernel at <= 64 VGPRs (8 waves/SIMD).  Persistent: the
// next chunk's 32 stream registers stay live through the reduction, so it is built for 80 VGPRs
// (6 waves/SIMD; 4 for the 1024-thread workgroup, of which only one fits a CU then).
__host__ __device__ constexpr int waves_per_simd(int block, bool persist) { return !persist ? 8 : (block == 1024 ? 4 : 6); }

// One slice of x, global -> LDS.  LDS-DMA (global_load_lds_dwordx4: no register in between), so all of a lane's
// 16-byte pieces are in flight at once; the register form is a load-store loop with one L2 round trip per trip
// (A/B: +1.8 % at c4 band 8192, +3 % at band 65 536, +8 % at band 200 000).  A slice that ends at the end of x is
// copied element by element.
template <int BLOCK, bool DMA>
__device__ __forceinline__ void stage_slice(const float *__restrict__ x, int64_t g0, int len, int64_t cols, float *smem,
                                            int tid)
{
    if (g0 + len + 3 < cols) {   // wave-uniform
        for (int i = tid * 4; i < len; i += BLOCK * 4) {
            if (DMA) __builtin_amdgcn_global_load_lds(x + g0 + i, smem + i, 16, 0, 0);
            else *reinterpret_cast<f4 *>(smem + i) = *reinterpret_cast<const f4 *>(x + g0 + i);
        }
    } else {
        for (int i = tid * 4; i < len; i += BLOCK * 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (g0 + i + q < cols) smem[i + q] = x[g0 + i + q];
        }
    }
}

// A slice of a chunk's BLOCK LIST, global -> LDS: block ids[b] (kBlkCols columns of x) lands at smem + kBlkCols b.  One wave
// per block and trip, one 1-KiB LDS-DMA piece each.  The last block of x is copied element by element.
template <int BLOCK>
__device__ __forceinline__ void stage_blocks(const float *__restrict__ x, const int32_t *__restrict__ ids, int nb,
                                             int64_t cols, float *smem, int tid)
{
    const int lane = tid & (kWave - 1);
    for (int b = __builtin_amdgcn_readfirstlane(tid >> 6); b < nb; b += BLOCK / kWave) {   // wave-uniform: scalar ids
        const int64_t g = (int64_t)ids[b] * kBlkCols;
        float *dst = smem + b * kBlkCols;
        if (g + kBlkCols + 3 < cols) {
            const float *src = x + g + lane * 4;
#pragma unroll 1
            for (int q = 0; q < kBlkCols / (kWave * 4); ++q)   // one trip at 256 columns per block
                __builtin_amdgcn_global_load_lds(src + q * kWave * 4, dst + (q * kWave + lane) * 4, 16, 0, 0);
        } else {
            for (int i = lane; i < kBlkCols; i += kWave)
                if (g + i < cols) dst[i] = x[g + i];
        }
    }
}

// The body of k_adaptive for workgroup `bid` of `grid` (a device function so that k_tiled_mixed can run it beside
// the 16-bit body in one launch).  smem: one dynamic LDS region, used twice: first as the x window (TILED), then
// -- after the gathers have landed in registers -- as the product staging buffer.
template <int BLOCK, bool TILED, bool PERSIST, typename E = float>
__device__ __forceinline__ void adaptive_body(float *smem, ChunkShared<BLOCK> &sh, int bid, int grid, int64_t rows,
                                              int64_t nnz, int64_t cols, int chunk0, int nrun,
                                              const int32_t *__restrict__ row_ptr,
                                              const int32_t *__restrict__ col_idx, const E *__restrict__ vals,
                                              const float *__restrict__ x, float *__restrict__ y,
                                              const int32_t *__restrict__ chunk_lb, float *__restrict__ carry,
                                              const int32_t *__restrict__ win, const int32_t *__restrict__ list,
                                              int kRegion)
{
    constexpr int kChunkT = chunk_of(BLOCK);
    constexpr int kVec = kNnzPerThread / 4;
    static_assert(!(PERSIST && kIs16<E>), "the persistent form is float only");

    const int tid0 = threadIdx.x;
    Walk wk = first_chunk(PERSIST, bid, grid, nrun);
    if (wk.c >= wk.end) return;
    if (!PERSIST && list) {  // one-shot launch over a chunk list (the chunks without 16-bit columns)
        wk.c = list[wk.c];
        wk.end = wk.c + 1;
    } else {
        wk.c += chunk0;
        wk.end += chunk0;
    }

    i4 cc[kVec];
    vals4_t<E> vv[kVec];
    {
        const int64_t b0 = (int64_t)wk.c * kChunkT;
        const int n0 = (int)((nnz - b0) < kChunkT ? (nnz - b0) : kChunkT);
        load_stream<BLOCK, PERSIST, E>(b0, n0, TILED ? win[2 * wk.c] : 0, col_idx, vals, tid0, cc, vv);
    }

    for (;;) {
        // (persistent form) keep lane-derived address math inside the iteration: hoisted out of the
        // loop it costs ~28 VGPRs and spills
        int tid = tid0;
        if (PERSIST) asm volatile("" : "+v"(tid));
        const ChunkHead h = chunk_head<BLOCK>(sh, tid, wk.c, chunk_lb, nnz);
        const int c = h.c, lb0 = h.lb0, m = h.m;
        const int64_t base = h.base, lim = h.lim;
        int w0 = 0, wlen = 0;
        bool outside = false;
        if (TILED) {
            w0 = win[2 * c];
            const int wl = win[2 * c + 1];
            wlen = wl & kLenMask;
            outside = (wl & kOutsideBit) != 0;
        }

        // ---- row pointers of this lane's first segment, in flight together with the stream
        //      (ADAPTIVE and k_tiled16 only: the 32-bit TILED form spills 20 bytes with them, wherever they
        //      are issued, and runs 5 % slower -- A/B).  first_bounds written out: through it k_adaptive<256, false, false>
        //      initialises the two registers in the other order.
        int32_t rb0 = 0, re0 = 0;
        if (!TILED && tid <= m) {
            rb0 = row_ptr[tid == 0 ? lb0 : lb0 + tid - 1];  // lb0 <= rows and row_ptr[rows] = nnz
            re0 = tid == 0 ? 0 : row_ptr[lb0 + tid];
        }

        // ---- gather x: from LDS where the plan staged a window, else through L1/L2
        f4 xv[kVec];
        if (TILED && wlen > 0) {
            // ceil(wlen / kRegion) passes (one for a chunk whose column span fits the region):
            // stage a slice of x, gather the nonzeros whose column lies in it.  Columns the plan
            // left outside the staged range come straight from global memory (issued first).
#pragma unroll
            for (int j = 0; j < kVec; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) xv[j][q] = 0.0f;
            if (outside) {
#pragma unroll
                for (int j = 0; j < kVec; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if ((unsigned)(cc[j][q] - w0) >= (unsigned)wlen) xv[j][q] = x[cc[j][q]];
            }
            for (int off = 0; off < wlen; off += kRegion) {
                const int len = (wlen - off) < kRegion ? (wlen - off) : kRegion;
                const int64_t g0 = (int64_t)w0 + off;
                stage_slice<BLOCK, true>(x, g0, len, cols, smem, tid);
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kVec; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned o = (unsigned)(cc[j][q] - w0 - off);
                        if (o < (unsigned)len) xv[j][q] = smem[o];
                    }
                __syncthreads();  // every gather has its value before the slice is overwritten
            }
        } else {
#pragma unroll
            for (int j = 0; j < kVec; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) xv[j][q] = x[cc[j][q]];
        }

        // ---- stage the products (padded one word per 32: lane-per-row reads spread over banks)
        stage_products<BLOCK, E>(smem, tid, vv, [&](int j, int q, int) { return xv[j][q]; });

        // ---- the next chunk's stream, into the registers the products just left
        const int cn = c + wk.stride;
        const bool more = PERSIST && cn < wk.end;
        if (more) {
            const int64_t bn = (int64_t)cn * kChunkT;
            const int nn = (int)((nnz - bn) < kChunkT ? (nnz - bn) : kChunkT);
            load_stream<BLOCK, PERSIST, E>(bn, nn, TILED ? win[2 * cn] : 0, col_idx, vals, tid, cc, vv);
        }
        __syncthreads();

        // ---- rows of this chunk
        // (the persistent form has no register for the read-ahead of the row sums: LEAN = 2)
        reduce_chunk<BLOCK, !TILED, PERSIST ? 2 : 0>(smem, sh, tid, c, lb0, m, base, lim, row_ptr, y, carry, rb0, re0);

        if (!more) break;
        __syncthreads();  // the region and the queues are reused by the next chunk
        wk.c = cn;
    }
}

template <int BLOCK, bool TILED, bool PERSIST, typename E = float>
__global__ __launch_bounds__(BLOCK, waves_per_simd(BLOCK, PERSIST))
void k_adaptive(int64_t rows, int64_t nnz, int64_t cols, int chunk0, int nrun, const int32_t *__restrict__ row_ptr,
                const int32_t *__restrict__ col_idx, const E *__restrict__ vals, const float *__restrict__ x,
                float *__restrict__ y, const int32_t *__restrict__ chunk_lb, float *__restrict__ carry,
                const int32_t *__restrict__ win, const int32_t *__restrict__ list, int kRegion)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ ChunkShared<BLOCK> sh;
    adaptive_body<BLOCK, TILED, PERSIST, E>(smem, sh, (int)blockIdx.x, (int)gridDim.x, rows, nnz, cols, chunk0, nrun, row_ptr,
                                            col_idx, vals, x, y, chunk_lb, carry, win, list, kRegion);
}

// ---------------------------------------------------------------------------
// 16-bit columns.  A chunk whose whole column span is staged in LDS never needs absolute columns:
// the plan stores col - w0 as uint16 (span < 65536), laid out so that each lane's 16 offsets are
// two 16-byte loads, and k_tiled16 streams 6 bytes per nonzero instead of 8 (HBM traffic of config 4:
// 1.8 GB against 2.35 GB algorithmic).  One-shot workgroups over the list of such chunks; the others
// (outliers gathered from global memory, the ragged last chunk) go through k_adaptive.

// 16-bit offset of element q of value vector j: a lane's sixteen offsets are two 16-byte loads of eight, element (j, q) is
// offset e = (j & 1) * 4 + q of load j >> 1
__device__ __forceinline__ unsigned col16_at(const u4 (&raw)[2], int j, int q)
{
    const int e = (j & 1) * 4 + q;
    const unsigned word = raw[j >> 1][e >> 1];
    return (e & 1) ? (word >> 16) : (word & 0xffffu);
}

// The chunk of workgroup `bid` of a launch over the `nrun` chunks of `list`.
// list == nullptr: every chunk is of the launch's kind (the list would be the identity) -- the stream addresses
// then depend on blockIdx only and the loads leave one dependent global load earlier
__device__ __forceinline__ int listed_chunk(int bid, int nrun, const int32_t *__restrict__ list)
{
    const int ci = xcd_chunk(bid, nrun);
    return list ? list[ci] : ci;
}

// The 16-bit body on chunk c0.  PRE: the caller has loaded the chunk's values into pre[] (the identity order of k_tiled_mixed,
// which issues them before it knows the kind of the chunk).
template <int BLOCK, bool BLOCKS, typename E = float, bool PRE = false>
__device__ __forceinline__ void tiled16_body(float *smem, ChunkShared<BLOCK> &sh, int c0, int64_t rows, int64_t cols,
                                             const int32_t *__restrict__ row_ptr,
                                             const uint16_t *__restrict__ col16, const E *__restrict__ vals,
                                             const float *__restrict__ x, float *__restrict__ y,
                                             const int32_t *__restrict__ chunk_lb, float *__restrict__ carry,
                                             const int32_t *__restrict__ win, int kRegionArg,
                                             const int32_t *__restrict__ blk, const vals4_t<E> *pre = nullptr)
{
    constexpr int kVec = kNnzPerThread / 4;
    static_assert(kNnzPerThread == 16, "the col16 lane layout is two 16-byte loads of eight offsets");

    const int tid = threadIdx.x;
    const ChunkHead h = chunk_head<BLOCK>(sh, tid, c0, chunk_lb);
    const int c = h.c;
    const int w0 = win[2 * c];
    const int wl = win[2 * c + 1];
    const int wlen = wl & kLenMask;
    // BLOCKS: this chunk's x is a LIST of 256-column blocks (its columns sit in a few clusters far apart); the
    // 16-bit offsets index the concatenation of the staged blocks, everything after the staging is the same
    const bool by_blocks = BLOCKS && (wl & kBlockBit);
    const int kRegion = by_blocks ? (kRegionArg / kBlkCols) * kBlkCols : kRegionArg;

    // ---- stream: 2 x 16 B of offsets + 4 x 16 B of values (16-bit values: 4 x 8 B) per lane, non-temporal
    u4 raw[2];
    vals4_t<E> vv[kVec];
    {
        const u4 *c8 = reinterpret_cast<const u4 *>(col16 + h.base);
        const vals4_t<E> *v4 = value_vectors(vals, h.base);
        raw[0] = __builtin_nontemporal_load(&c8[tid]);   // (not stream_load: the 1024-thread kernel then shares an offset register)
        raw[1] = __builtin_nontemporal_load(&c8[BLOCK + tid]);
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            if constexpr (PRE) vv[j] = pre[j];
            else vv[j] = stream_load<BLOCK>(v4, tid, j);
        }
    }
    // The bounds of this lane's first segment ride along with the stream (they only depend on chunk_lb).  The compiler widens
    // `re` inside the branch of first_bounds, behind an s_waitcnt vmcnt(0): every load issued before it has landed when the
    // wave goes on, so the window of a one-pass chunk (nearly every chunk) leaves for L2 when the stream is in.  kWindowFirst
    // (tiled_chunks.hpp, A/B) issues the window in front of the bounds, under the stream -- and measured 1.3 to 2.1 % slower
    // on the headline: the shipped order is this one.  The body with block lists has it in every build:
    // with the window first it spills 36 bytes instead of 20.
    const bool one_pass = wlen <= kRegion && wlen > 0;
    auto stage_window = [&] {
        if (by_blocks) stage_blocks<BLOCK>(x, blk + (int64_t)c * kBlkMax, wlen / kBlkCols, cols, smem, tid);
        else stage_slice<BLOCK, true>(x, (int64_t)w0, wlen, cols, smem, tid);
    };
    constexpr bool kFirst = kWindowFirst && !BLOCKS;
    if (kFirst && one_pass) stage_window();
    const RowBounds b0 = first_bounds(tid, h, row_ptr);

    // ---- gather x from the staged slices (every column of the chunk lies in [w0, w0+wlen))
    f4 xv[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) xv[j][q] = 0.0f;
    if (one_pass) {
        // every offset lies inside the staged window, no range check per element
        if (!kFirst) stage_window();
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kVec; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[j][q] = smem[col16_at(raw, j, q)];
        __syncthreads();  // every gather has its value before the products overwrite the window
    } else {
        for (int off = 0; off < wlen; off += kRegion) {
            const int len = (wlen - off) < kRegion ? (wlen - off) : kRegion;
            const int64_t g0 = (int64_t)w0 + off;
            if (by_blocks) stage_blocks<BLOCK>(x, blk + (int64_t)c * kBlkMax + off / kBlkCols, len / kBlkCols, cols, smem, tid);
            else stage_slice<BLOCK, true>(x, g0, len, cols, smem, tid);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kVec; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned o = col16_at(raw, j, q) - (unsigned)off;
                    if (o < (unsigned)len) xv[j][q] = smem[o];
                }
            __syncthreads();  // every gather has its value before the slice is overwritten
        }
    }

    // ---- products, then the rows of the chunk
    stage_products<BLOCK, E>(smem, tid, vv, [&](int j, int q, int) { return xv[j][q]; });
    __syncthreads();
    reduce_chunk<BLOCK, true, BLOCKS ? 1 : 0>(smem, sh, tid, h.c, h.lb0, h.m, h.base, h.lim, row_ptr, y, carry, b0.rb, b0.re);
}

template <int BLOCK, bool BLOCKS, typename E = float>
__global__ __launch_bounds__(BLOCK, 8)
void k_tiled16(int64_t rows, int64_t cols, int nrun, const int32_t *__restrict__ row_ptr, const uint16_t *__restrict__ col16,
               const E *__restrict__ vals, const float *__restrict__ x, float *__restrict__ y,
               const int32_t *__restrict__ chunk_lb, float *__restrict__ carry, const int32_t *__restrict__ win,
               const int32_t *__restrict__ list, int kRegion, const int32_t *__restrict__ blk)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ ChunkShared<BLOCK> sh;
    tiled16_body<BLOCK, BLOCKS, E>(smem, sh, listed_chunk((int)blockIdx.x, nrun, list), rows, cols, row_ptr, col16, vals, x, y,
                                   chunk_lb, carry, win, kRegion, blk);
}

// ---------------------------------------------------------------------------
// Sorted chunks.  A chunk whose column span is several LDS regions wide (a band of 65 536 columns; the inside of a
// power-law row) used to stage the span slice by slice: every slice is region floats of L2 -> LDS traffic, a barrier
// pair and 16 predicated LDS reads per lane.  Here the plan sorts the chunk's nonzeros by COLUMN once
// (perm[k] = position in the chunk << 18 | column - w0, 4 bytes per nonzero read INSTEAD of col_idx) and the kernel
// gathers x straight from L1/L2 in that order: the lanes of a gather instruction then touch a handful of
// neighbouring 128-byte lines instead of 64 scattered ones (every line of the span is requested about once per chunk,
// the same L2 traffic as staging it, without the passes).  The gathered x values are scattered through LDS to the
// positions their nonzeros have in the row-major stream, where the lane that holds the VALUES of those positions
// (read live from vals, original order: nothing is copied) picks them up, multiplies and leaves the products for
// the same row reduction as everywhere else.  Same products, same order of every sum as the other bodies.
// The sorted body on chunk c0, whose words are slot `ci` of perm[] (its position in the list of sorted chunks).  PRE: its values
// are in pre[] already (as in tiled16_body).
template <int BLOCK, typename E = float, bool PRE = false>
__device__ __forceinline__ void sorted_body(float *smem, ChunkShared<BLOCK> &sh, int c0, int ci, int64_t rows,
                                            const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ perm,
                                            const E *__restrict__ vals, const float *__restrict__ x,
                                            float *__restrict__ y, const int32_t *__restrict__ chunk_lb,
                                            float *__restrict__ carry, const int32_t *__restrict__ win,
                                            const vals4_t<E> *pre = nullptr)
{
    constexpr int kChunkT = chunk_of(BLOCK);
    constexpr int kVec = kNnzPerThread / 4;
    constexpr int kColBits = sorted_col_bits(BLOCK);
    constexpr unsigned kColMask = (1u << kColBits) - 1u;

    const int tid = threadIdx.x;
    const ChunkHead h = chunk_head<BLOCK>(sh, tid, c0, chunk_lb);
    const float *xw = x + win[2 * h.c];

    u4 pw[kVec];
    vals4_t<E> vv[kVec];
    {
        const u4 *p4 = reinterpret_cast<const u4 *>(perm + (int64_t)ci * kChunkT);
        const vals4_t<E> *v4 = value_vectors(vals, h.base);
#pragma unroll
        for (int j = 0; j < kVec; ++j) pw[j] = stream_load<BLOCK>(p4, tid, j);
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            if constexpr (PRE) vv[j] = pre[j];
            else vv[j] = stream_load<BLOCK>(v4, tid, j);
        }
    }
    const RowBounds b0 = first_bounds(tid, h, row_ptr);

    // gather in column order, scatter to the row-major position of each nonzero
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        float g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = xw[pw[j][q] & kColMask];
#pragma unroll
        for (int q = 0; q < 4; ++q) smem[pad_idx((int)(pw[j][q] >> kColBits))] = g[q];
    }
    __syncthreads();
    // this lane's values meet their x; the products take the same LDS words
    stage_products<BLOCK, E>(smem, tid, vv, [&](int, int, int w) { return smem[w]; });
    __syncthreads();
    reduce_chunk<BLOCK, true>(smem, sh, tid, h.c, h.lb0, h.m, h.base, h.lim, row_ptr, y, carry, b0.rb, b0.re);
}

template <int BLOCK, typename E = float>
__global__ __launch_bounds__(BLOCK, 8)
void k_sorted(int64_t rows, int nrun, const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ perm,
              const E *__restrict__ vals, const float *__restrict__ x, float *__restrict__ y,
              const int32_t *__restrict__ chunk_lb, float *__restrict__ carry, const int32_t *__restrict__ win,
              const int32_t *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ ChunkShared<BLOCK> sh;
    const int ci = xcd_chunk((int)blockIdx.x, nrun);   // position in the list of sorted chunks = slot of its words in perm[]
    sorted_body<BLOCK, E>(smem, sh, list[ci], ci, rows, row_ptr, perm, vals, x, y, chunk_lb, carry, win);
}

// All kinds of chunk in ONE launch, in one of two orders (the plan decides: ChunkPlan::identity_order, tiled_chunks.hpp).
// Two launches would each end with a partly idle chip (power-law rows: 1758 such chunks took 71 us after the 209 us of the rest).
// Lists: workgroups [0, n32) run the 32-bit body over list32 (the slow chunks -- outliers gathered from global memory, the
// ragged last chunk -- start first), the next nsorted the sorted body, the rest the 16-bit body over list16.
// Identity (list16 == nullptr; list_sorted then holds ChunkPlan::d_sorted_slot, one word per chunk): workgroup b takes chunk
// xcd_chunk(b) of all n32 + nsorted + n16 and reads no list.  The values of a full chunk lie at the same addresses whatever
// its kind, so their loads are issued first, from blockIdx alone; win[] then says which body goes on with them, and only a
// sorted chunk reads more: its slot in perm[], sorted_slot[c].  The ragged last chunk (always 32-bit, the slowest, guarded
// loads) changes places with the first chunk of its XCD's range, so that it starts with the launch and not at its end.
template <int BLOCK, bool BLOCKS, typename E = float>
__global__ __launch_bounds__(BLOCK, 8)
void k_tiled_mixed(int64_t rows, int64_t nnz, int64_t cols, int n32, int nsorted, int n16, const int32_t *__restrict__ row_ptr,
                   const int32_t *__restrict__ col_idx, const uint16_t *__restrict__ col16, const uint32_t *__restrict__ perm,
                   const E *__restrict__ vals, const float *__restrict__ x, float *__restrict__ y,
                   const int32_t *__restrict__ chunk_lb, float *__restrict__ carry, const int32_t *__restrict__ win,
                   const int32_t *__restrict__ list32, const int32_t *__restrict__ list_sorted,
                   const int32_t *__restrict__ list16, int kRegion, const int32_t *__restrict__ blk)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ ChunkShared<BLOCK> sh;
    const int b = (int)blockIdx.x;
    // (The order has no argument of its own: with two more scalar arguments the 16-bit path spilled scalars to a vector
    // register and, one VGPR short, a just-loaded value vector to scratch.  Not compiled in for plans with block lists,
    // BLOCKS: that kernel spills 20 bytes as it is, and 36 with this path in it.)
    if (kIdentityOrder && !BLOCKS && list16 == nullptr) {
        const int32_t *__restrict__ sorted_slot = list_sorted;
        constexpr int kChunkT = chunk_of(BLOCK);
        constexpr int kVec = kNnzPerThread / 4;
        const int nchunks = n32 + nsorted + n16;
        int c = xcd_chunk(b, nchunks);
        bool full = true;
        if ((int64_t)nchunks * kChunkT != nnz) {   // a ragged last chunk
            const int last = nchunks - 1, q = nchunks / kXcds;
            const int first = q > 0 ? nchunks - q : last;   // where the range of the last XCD that has chunks begins
            c = c == first ? last : (c == last ? first : c);
            full = c != last;
        }
        if (full) {
            vals4_t<E> vv[kVec];
            const vals4_t<E> *v4 = value_vectors(vals, (int64_t)c * kChunkT);
#pragma unroll
            for (int j = 0; j < kVec; ++j) vv[j] = stream_load<BLOCK>(v4, (int)threadIdx.x, j);
            const int wl = win[2 * c + 1];
            if (wl & kCol16Bit) {
                tiled16_body<BLOCK, BLOCKS, E, true>(smem, sh, c, rows, cols, row_ptr, col16, vals, x, y, chunk_lb, carry, win,
                                                     kRegion, blk, vv);
                return;
            }
            if (wl & kSortedBit) {
                sorted_body<BLOCK, E, true>(smem, sh, c, sorted_slot[c], rows, row_ptr, perm, vals, x, y, chunk_lb, carry, win, vv);
                return;
            }
        }
        // the few 32-bit chunks load their stream again, columns and values in the order that body keeps its registers by
        // (handed the values, it spilled 36 bytes instead of 20)
        adaptive_body<BLOCK, true, false, E>(smem, sh, 0, 1, rows, nnz, cols, c, 1, row_ptr, col_idx, vals, x, y, chunk_lb,
                                             carry, win, nullptr, kRegion);
        return;
    }
    if (b < n32)
        adaptive_body<BLOCK, true, false, E>(smem, sh, b, n32, rows, nnz, cols, 0, n32, row_ptr, col_idx, vals, x,
                                             y, chunk_lb, carry, win, list32, kRegion);
    else if (b < n32 + nsorted) {
        const int ci = xcd_chunk(b - n32, nsorted);
        sorted_body<BLOCK, E>(smem, sh, list_sorted[ci], ci, rows, row_ptr, perm, vals, x, y, chunk_lb, carry, win);
    } else
        tiled16_body<BLOCK, BLOCKS, E>(smem, sh, listed_chunk(b - n32 - nsorted, n16, list16), rows, cols, row_ptr, col16, vals,
                                       x, y, chunk_lb, carry, win, kRegion, blk);
}

// rows that continue past their owner chunk: y[r] += carry[c+1] + carry[c+2] + ... in chunk order
__global__ void k_carry_fixup(int nchunks, int chunk, const int32_t *__restrict__ row_ptr,
                              const int32_t *__restrict__ chunk_lb, const float *__restrict__ carry,
                              float *__restrict__ y)
{
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks - 1) return;
    const int lb0 = chunk_lb[c], lb1 = chunk_lb[c + 1];
    if (lb1 == lb0) return;  // no row starts in this chunk
    const int64_t r = (int64_t)lb1 - 1;
    const int64_t endp = row_ptr[r + 1];
    if (endp <= (int64_t)(c + 1) * chunk) return;
    float s = y[r];
    for (int64_t c2 = c + 1; c2 * chunk < endp; ++c2) s += carry[c2];
    y[r] = s;
}

// ---------------------------------------------------------------------------
// plan (TILED): what part of x chunk c stages in LDS.
// (win[2c] = first staged column, win[2c+1] = staged length | flag bits: tiled_chunks.hpp)
// A chunk whose whole column span [min, max] fits `maxpass` LDS regions is staged completely (in
// ceil(span/region) passes).  A wider one stages ONE region centred on the mean column (the dense
// part of a banded chunk that also holds a few very long rows) if that covers >= 1/4 of its
// nonzeros.  stats[0] = chunks staged in a single pass with nothing outside, stats[1] = chunks
// staged completely (any number of passes).
__global__ __launch_bounds__(256)
void k_plan_windows(int64_t nnz, int64_t cols, int nchunks, int chunk, const int32_t *__restrict__ col_idx,
                    int32_t *__restrict__ win, int32_t *__restrict__ stats, int region, int maxpass, int sorted_from,
                    int sorted_span, PlanCost cost, const int32_t *__restrict__ lb, const int32_t *__restrict__ row_ptr)
{
    __shared__ int s_min[4], s_max[4], s_cnt[4];
    __shared__ long long s_sum[4];
    __shared__ int s_w0;
    const int c = blockIdx.x;
    const int wv = threadIdx.x >> 6;
    const bool lane0 = (threadIdx.x & (kWave - 1)) == 0;
    const int64_t base = (int64_t)c * chunk;
    const int n = (int)((nnz - base) < chunk ? (nnz - base) : chunk);
    int mn = 0x7fffffff, mx = -1;
    long long sum = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        int v = col_idx[base + i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        sum += v;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        int a = __shfl_down(mn, o, kWave), b = __shfl_down(mx, o, kWave);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        sum += __shfl_down(sum, o, kWave);
    }
    if (lane0) { s_min[wv] = mn; s_max[wv] = mx; s_sum[wv] = sum; }
    __syncthreads();
    for (int w = 0; w < 4; ++w) {  // every thread folds the four partials
        mn = w == 0 ? s_min[0] : (s_min[w] < mn ? s_min[w] : mn);
        mx = w == 0 ? s_max[0] : (s_max[w] > mx ? s_max[w] : mx);
    }
    // Staged or sorted?  Every staging pass re-reads `region` floats of x from L2 and costs a barrier pair and 16
    // predicated LDS reads per lane; the sorted gather (sorted_body) touches every 128-byte line of the span about
    // once, with no barrier, but streams 8 bytes per nonzero where a staged chunk with 16-bit columns streams 6.  The
    // plan prices both for this chunk with the constants of PlanCost (fitted to measurements) and
    // takes the cheaper; the sum of the chunk prices is how the plan compares workgroup sizes.  sorted_from = 0:
    // never sort; > 0: sort from that many passes on, whatever the prices (tuning knob SPMV_SORTED_FROM).
    {
        const int w0_line = mn & ~31;
        const int64_t span_l = (int64_t)mx + 1 - w0_line;
        const int64_t span4 = (int64_t)mx + 1 - (mn & ~3);
        const int64_t passes = (span4 + region - 1) / region;
        const int lines = (int)((span_l + 31) >> 5);
        const int cost_staged = passes > maxpass ? cost.unstaged
                                : (span4 < 65536 ? cost.c16_base + cost.c16_pass * (int)passes
                                                 : cost.c32_base + cost.c32_pass * (int)passes);
        const int rows_here = lb[c + 1] - lb[c];
        // the longest piece of a row inside this chunk (the head segment included)
        int longest = 0;
        {
            const int64_t lim = base + n;
            for (int t = threadIdx.x; t <= rows_here; t += 256) {
                const int64_t a = t == 0 ? base : (int64_t)row_ptr[lb[c] + t - 1];
                int64_t b = t == 0 ? (int64_t)row_ptr[lb[c]] : (int64_t)row_ptr[lb[c] + t];
                b = b < lim ? b : lim;
                const int len = (int)(b - (a > base ? a : base));
                longest = len > longest ? len : longest;
            }
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) {
                const int v = __shfl_down(longest, o, kWave);
                longest = v > longest ? v : longest;
            }
            __syncthreads();                 // s_cnt is free here (its first use comes later, behind another barrier)
            if (lane0) s_cnt[wv] = longest;
            __syncthreads();
            longest = s_cnt[0];
            for (int w = 1; w < 4; ++w) longest = s_cnt[w] > longest ? s_cnt[w] : longest;
        }
        const int cost_sorted = cost.sorted_base + (int)((int64_t)(chunk >= 16384 ? cost.sorted_line_1024 : cost.sorted_line_512) * lines / chunk) -
                                (rows_here <= 16 ? cost.sorted_few_rows : 0);
        const bool eligible = sorted_from != 0 && n == chunk && span_l <= sorted_span;
        // ... and one rule the prices do not capture: a chunk that holds a piece of a long row (more than kHugeSeg
        // nonzeros: power-law rows, whose own column window is what makes the span wide) is sorted from three passes on
        // -- measured on c3 (4Mi rows, mean 32): 57.2 -> 60.2 % of peak over the priced choice
        const bool long_row_rule = longest > cost.long_piece && passes >= 3;
        const bool sort = eligible && (sorted_from > 0 ? span_l > (int64_t)region * (sorted_from - 1)
                                                       : (cost_sorted < cost_staged || long_row_rule));
        if (threadIdx.x == 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(stats + 4), (unsigned long long)(sort ? cost_sorted : cost_staged));
            if (long_row_rule) atomicAdd(&stats[3], 1);
        }
        if (sort) {
            if (threadIdx.x == 0) {
                win[2 * c] = w0_line;
                win[2 * c + 1] = kSortedBit;
                atomicAdd(&stats[2], 1);
            }
            return;
        }
    }
    const int w0_full = mn & ~3;
    const int64_t span = (int64_t)mx + 1 - w0_full;
    if (span <= (int64_t)region * maxpass) {
        if (threadIdx.x == 0) {
            win[2 * c] = w0_full;
            win[2 * c + 1] = (int32_t)span;
            if (span <= region) atomicAdd(&stats[0], 1);
            atomicAdd(&stats[1], 1);
        }
        return;
    }
    // too wide: one region around the mean column, if it is worth it
    if (threadIdx.x == 0) {
        const long long tot = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        long long w0 = tot / (n > 0 ? n : 1) - region / 2;
        if (w0 > cols - region) w0 = cols - region;
        if (w0 < 0) w0 = 0;
        s_w0 = (int)(w0 & ~3ll);
    }
    __syncthreads();
    const int w0 = s_w0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += 256) cnt += ((unsigned)(col_idx[base + i] - w0) < (unsigned)region) ? 1 : 0;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, kWave);
    if (lane0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const bool stage = 4 * (int64_t)cnt >= n;
        int64_t wl = region;
        if (w0 + wl > cols) wl = cols - w0;
        win[2 * c] = w0;
        win[2 * c + 1] = stage ? ((int32_t)wl | kOutsideBit) : 0;
    }
}

int launch_plan_windows(const spmv_csr &h, const ChunkPlan &p, int32_t *d_stats, const PlanCost &cost, hipStream_t s)
{
    hipLaunchKernelGGL(k_plan_windows, dim3(p.nchunks), dim3(256), 0, s, h.nnz, h.cols, p.nchunks, chunk_of(p.block), h.d_col_idx,
                       p.d_win, d_stats, p.region, p.maxpass, p.sorted_from, 1 << sorted_col_bits(p.block), cost, p.d_lb, h.d_row_ptr);
    return check_launch("k_plan_windows");
}

// ---------------------------------------------------------------------------
static int resident_workgroups(int device, int block, int waves_simd)
{
    int per_cu = (waves_simd * 4 * kWave) / block;  // workgroups per CU by waves
    if (per_cu < 1) per_cu = 1;
    return device_cus(device) * per_cu;
}

// One launch of a run kernel: `grid` workgroups of `block` threads with the plan's LDS region as dynamic LDS (the product buffer;
// a staged x slice is never wider: plan cap = region).  More than 64 KiB of it (1024 threads) needs an opt-in per (kernel,
// device), remembered in a static of this function: one per instantiation, that is, per kernel.
template <auto Kernel, typename... Args>
static int launch_region(const char *name, const spmv_csr &h, const ChunkPlan &p, int grid, int block, hipStream_t s,
                         const Args &...args)
{
    const size_t lds = sizeof(float) * (size_t)p.region;
    static LdsOptIn optin;
    if (int rc = optin.ensure(reinterpret_cast<const void *>(Kernel), h.device, (int)lds)) return rc;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds, s, args...);
    return check_launch(name);
}

// The launches below take the values as an argument: the handle's own fp32 array (launch_adaptive) or the caller's 16-bit
// one (launch_adaptive_vals16), element type E.
template <int BLOCK, bool TILED, bool PERSIST, typename E>
static int launch_range(const spmv_csr &h, const ChunkPlan &p, const E *vals, int chunk0, int nrun, const float *x, float *y,
                        hipStream_t s)
{
    if (nrun <= 0) return SPMV_OK;
    int grid = nrun;
    if (PERSIST) {
        const int res = resident_workgroups(h.device, BLOCK, waves_per_simd(BLOCK, true));
        if (grid > res) grid = res;
    }
    return launch_region<k_adaptive<BLOCK, TILED, PERSIST, E>>("k_adaptive", h, p, grid, BLOCK, s, h.rows, h.nnz, h.cols, chunk0, nrun,
                                                               h.d_row_ptr, h.d_col_idx, vals, x, y, p.d_lb, p.d_carry, p.d_win,
                                                               (const int32_t *)nullptr, p.region);
}

// BLOCKS: the block-list staging is compiled in only for plans that have such chunks
template <int BLOCK, bool BLOCKS, typename E>
static int launch_tiled16(const spmv_csr &h, const ChunkPlan &p, const E *vals, const float *x, float *y, hipStream_t s)
{
    if (p.n16 <= 0) return SPMV_OK;
    return launch_region<k_tiled16<BLOCK, BLOCKS, E>>("k_tiled16", h, p, p.n16, BLOCK, s, h.rows, h.cols, p.n16, h.d_row_ptr, p.d_col16,
                                                      vals, x, y, p.d_lb, p.d_carry, p.d_win,
                                                      p.n16 == p.nchunks ? (const int32_t *)nullptr : p.d_list16.get(), p.region, p.d_blk);
}

template <int BLOCK, bool BLOCKS, typename E>
static int launch_mixed(const spmv_csr &h, const ChunkPlan &p, const E *vals, const float *x, float *y, hipStream_t s)
{
    const int n32 = p.nchunks - p.n16 - p.nsorted;
    // identity order: no list16 (that is how the kernel knows), and the sorted chunks' slots where their list would be
    const int32_t *list_sorted = p.identity_order ? p.d_sorted_slot.get() : p.d_list_sorted.get();
    const int32_t *list16 = p.identity_order ? nullptr : p.d_list16.get();
    return launch_region<k_tiled_mixed<BLOCK, BLOCKS, E>>("k_tiled_mixed", h, p, p.nchunks, BLOCK, s, h.rows, h.nnz, h.cols, n32, p.nsorted,
                                                          p.n16, h.d_row_ptr, h.d_col_idx, p.d_col16, p.d_perm, vals, x, y, p.d_lb,
                                                          p.d_carry, p.d_win, p.d_list32, list_sorted, list16, p.region, p.d_blk);
}

template <int BLOCK, typename E>
static int launch_sorted(const spmv_csr &h, const ChunkPlan &p, const E *vals, const float *x, float *y, hipStream_t s)
{
    return launch_region<k_sorted<BLOCK, E>>("k_sorted", h, p, p.nsorted, BLOCK, s, h.rows, p.nsorted, h.d_row_ptr, p.d_perm, vals, x,
                                             y, p.d_lb, p.d_carry, p.d_win, p.d_list_sorted);
}

template <int BLOCK, bool TILED, typename E>
static int launch_either(bool persist, const spmv_csr &h, const ChunkPlan &p, const E *vals, const float *x, float *y, hipStream_t s)
{
    if constexpr (TILED) {
        if (!persist && (p.n16 > 0 || p.nsorted > 0)) {
            // every chunk has 16-bit columns: the lean kernel; otherwise all kinds in one launch
            const bool lists = p.nblk_chunks > 0;
            if (p.n16 == p.nchunks)
                return lists ? launch_tiled16<BLOCK, true>(h, p, vals, x, y, s) : launch_tiled16<BLOCK, false>(h, p, vals, x, y, s);
            if (p.nsorted == p.nchunks) return launch_sorted<BLOCK>(h, p, vals, x, y, s);
            return lists ? launch_mixed<BLOCK, true>(h, p, vals, x, y, s) : launch_mixed<BLOCK, false>(h, p, vals, x, y, s);
        }
    }
    if constexpr (kIs16<E>) {
        // no persistent form for 16-bit values: the one-shot kernel over the same chunks (persist is false here)
        return launch_range<BLOCK, TILED, false>(h, p, vals, 0, p.nchunks, x, y, s);
    } else {
        if (!persist) return launch_range<BLOCK, TILED, false>(h, p, vals, 0, p.nchunks, x, y, s);
        // persistent launch over the full chunks, one-shot launch for a trailing partial chunk
        const int nfull = (int)(h.nnz / chunk_of(BLOCK));
        int rc = launch_range<BLOCK, TILED, true>(h, p, vals, 0, nfull, x, y, s);
        if (rc == SPMV_OK && p.nchunks > nfull) rc = launch_range<BLOCK, TILED, false>(h, p, vals, nfull, p.nchunks - nfull, x, y, s);
        return rc;
    }
}

// y = A x with the values `vals` (element type E) in the place of the handle's: every launch of a run.  A plan with persist = 1
// runs 16-bit values through the one-shot kernels over the same chunks: the sums are the same by the documented order.
template <typename E>
static int launch_adaptive_with(const spmv_csr &h, const E *vals, const float *x, float *y, bool tiled, hipStream_t s)
{
    const ChunkPlan &p = tiled ? h.plan_tiled : h.plan_adaptive;
    if (!p.block) {
        set_error("%s used before spmv_csr_plan", tiled ? "SPMV_TILED" : "SPMV_ADAPTIVE");
        return SPMV_ERR_NOT_PLANNED;
    }
    if (h.rows == 0) return SPMV_OK;
    if (p.nchunks == 0) {  // no nonzeros: y = 0
        SPMV_HIP_TRY(hipMemsetAsync(y, 0, sizeof(float) * (size_t)h.rows, s));
        return SPMV_OK;
    }
    const bool persist = p.persist && !kIs16<E>;
    int rc;
    // a tiled plan that stages nothing runs the plain kernel (same chunks; it keeps the row-bound prefetch the
    // 32-bit tiled form has no registers for)
    const bool nothing_staged = tiled && p.block == 256 && p.staged_full == 0 && p.n16 == 0 && p.nsorted == 0;
    if (!tiled || nothing_staged) rc = launch_either<256, false>(persist, h, p, vals, x, y, s);
    else rc = dispatch_block(p.block, [&](auto B) { return launch_either<decltype(B)::value, true>(persist, h, p, vals, x, y, s); });
    if (rc) return rc;
    if (p.nchunks > 1 && p.spanning_rows > 0) {  // chunk boundaries that all fall on row boundaries need no fix-up
        hipLaunchKernelGGL(k_carry_fixup, dim3((p.nchunks - 1 + 255) / 256), dim3(256), 0, s, p.nchunks,
                           chunk_of(p.block), h.d_row_ptr, p.d_lb, p.d_carry, y);
        rc = check_launch("k_carry_fixup");
    }
    return rc;
}

int launch_adaptive(const spmv_csr &h, const float *x, float *y, bool tiled, hipStream_t s)
{
    return launch_adaptive_with(h, (const float *)h.d_vals, x, y, tiled, s);
}

int launch_adaptive_vals16(const spmv_csr &h, int dtype, const void *vals16, const float *x, float *y, bool tiled, hipStream_t s)
{
    return dtype == SPMV_ATTN_BF16 ? launch_adaptive_with(h, (const bf16 *)vals16, x, y, tiled, s)
                                   : launch_adaptive_with(h, (const fp16 *)vals16, x, y, tiled, s);
}

}  // namespace spmv
