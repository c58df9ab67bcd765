// kernels_select.hip -- spmv_csr_select_topk / spmv_csr_select_threshold and their companions (include/spmv_hip.h
// "selection"): a sub-pattern of a handle -- per row the k best-scored nonzeros, or those at or above a threshold -- as a
// new handle that owns its arrays.  Pure structure: keys are integers, nothing is summed, and no place comes from the value
// an atomic returns (the only atomics are LDS counter increments whose result is not used).
//
// Every nonzero has a 32-bit key (sel_key: the order-preserving map of its score, NaN = 0, -0 = +0) and ranks inside its row
// by (key descending, storage position ascending).  A row's selection is described by a CUT (tau, quota): kept is every
// nonzero with key > tau, and of those with key == tau the first `quota` in storage order.  A threshold is the cut
// (key(threshold), all) for every row; "take the whole row" is (0, all).
//
//   1. k_sel_cut      per row the cut (top-k only) and the kept count, which goes into out.row_ptr
//   2. scan_offsets_i32 (tile sums, two levels) makes the counts out.row_ptr; the total is read back and sizes out
//   3. k_sel_compact  every row re-reads its scores and writes col_idx, vals and the map of what its cut keeps, in
//                     storage order, to places that come from ballot prefixes
//
// Geometry of both kernels (that of kernels_softmax.hip).  A wavefront owns 64 consecutive rows, a workgroup 256, dealt per
// XCD (xcd_item64).  Lane l loads the bounds of row r0 + l; the longest of the 64 rows that has at most 512 nonzeros decides
// the walk: at most 64 -> groups of G = pow2 >= that length lanes, a row per group, an element per lane; more -> the whole
// wavefront per row, lane l holding elements l, l + 64, ... (1, 2, 4 or 8 slots, by the row's own length).  Either way a row
// is read once and held in registers: the cut is a bisection over the 32 key bits whose counts are ballots masked to the
// group.  Rows of more than 512 nonzeros are then taken by the whole workgroup one after the other: the cut by an 8-bit
// radix select in four passes over the row (a 256-counter LDS histogram per pass), the compaction tile by tile (1024
// nonzeros) with the two running counts carried.  G and the walk depend on the wavefront's own rows only and the result
// on neither.
//
// Positions are unsigned 32-bit (nnz < 2^31), byte offsets 64-bit.  Every access is predicated on its array's own length:
// nothing here relies on slack behind an array.
#include <climits>
#include <new>
#include "lane_group.hpp"

namespace spmv {

namespace {

constexpr int kSelBlockRows = kBlock;          // rows of a workgroup: 4 wavefronts x 64
constexpr int kSelWaves = kBlock / kWave;
constexpr int kSelCap = 512;                   // the longest row a wavefront holds in registers
constexpr int kSelSlots = kSelCap / kWave;     // 8 per lane
constexpr int kSelTileSlots = 4;               // long rows: a wavefront takes 4 x 64 consecutive nonzeros of a tile
constexpr int kSelTile = kSelWaves * kSelTileSlots * kWave;   // 1024
constexpr int kSelAll = INT_MAX;               // quota: every nonzero whose key equals tau

__device__ __forceinline__ int sel_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// the key of a score's bits (absmask = 0x7fffffff with SPMV_SELECT_ABS, else all ones): integer code, so neither a
// denormal mode nor a NaN payload has a say
__host__ __device__ __forceinline__ uint32_t sel_key(uint32_t u, uint32_t absmask)
{
    u &= absmask;
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;     // NaN
    if (u == 0x80000000u) u = 0u;                       // -0 is +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SelCut {
    uint32_t tau;
    int32_t quota;
};

// What a lane group (or the wavefront) knows of the row it walks.
struct SelRow {
    uint32_t start;      // first position of the row
    int len;             // its length; -1: not a row of this walk (past the matrix, or a long row)
    int j;               // my element of slot 0
    uint64_t gmask;      // the lanes of my group
    uint64_t below;      // ... of them, those before me
};

template <int S>
__device__ __forceinline__ void sel_load_keys(const SelRow &r, const uint32_t *__restrict__ score, uint32_t absmask, uint32_t nnz,
                                              uint32_t (&key)[S], bool (&valid)[S])
{
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const int e = r.j + i * kWave;
        const uint32_t p = r.start + (uint32_t)e;
        valid[i] = e < r.len && p < nnz;
        key[i] = valid[i] ? sel_key(score[p], absmask) : 0u;
    }
}

// ---- rows of at most 512 nonzeros: the cut and the count ----------------------------------------------------------------
template <int S, bool THRESH>
__device__ __forceinline__ void sel_cut_short(const SelRow &r, int64_t row, const uint32_t *__restrict__ score, uint32_t absmask,
                                              uint32_t nnz, int k, uint32_t thr_key, SelCut *__restrict__ cut,
                                              int32_t *__restrict__ counts)
{
    uint32_t key[S];
    bool valid[S];
    sel_load_keys<S>(r, score, absmask, nnz, key, valid);
    uint32_t tau = 0u;
    int quota = kSelAll, cnt = r.len;
    if (THRESH) {
        cnt = 0;
#pragma unroll
        for (int i = 0; i < S; ++i) cnt += (int)__popcll(__ballot(valid[i] && key[i] >= thr_key) & r.gmask);
    } else {
        const bool need = r.len > k;
        if (__ballot(need) != 0) {
            // the largest t with at least k keys >= t: the k-th key of the ranking
            uint32_t t = 0u;
            for (int b = 31; b >= 0; --b) {
                const uint32_t cand = t | (1u << b);
                int c = 0;
#pragma unroll
                for (int i = 0; i < S; ++i) c += (int)__popcll(__ballot(valid[i] && key[i] >= cand) & r.gmask);
                if (c >= k) t = cand;
            }
            int above = 0;
#pragma unroll
            for (int i = 0; i < S; ++i) above += (int)__popcll(__ballot(valid[i] && key[i] > t) & r.gmask);
            if (need) {
                tau = t;
                quota = k - above;
                cnt = k;
            }
        }
    }
    if (r.len >= 0 && r.j == 0) {
        counts[row] = cnt;
        if (!THRESH) cut[row] = SelCut{tau, quota};
    }
}

// ---- rows of at most 512 nonzeros: the stores ---------------------------------------------------------------------------
// Storage order in the register layout is slot-major, then lane: the tie rank and the place of a kept nonzero both run
// through the slots in order and inside a slot by lane number.
template <int S>
__device__ __forceinline__ void sel_compact_short(const SelRow &r, SelCut c, uint32_t obase, uint32_t out_nnz,
                                                  const uint32_t *__restrict__ score, uint32_t absmask, uint32_t nnz,
                                                  const int32_t *__restrict__ col_idx, const uint32_t *__restrict__ vals,
                                                  int32_t *__restrict__ out_col, uint32_t *__restrict__ out_vals,
                                                  uint32_t *__restrict__ out_map)
{
    uint32_t key[S];
    bool valid[S];
    sel_load_keys<S>(r, score, absmask, nnz, key, valid);
    int eq_run = 0, kept_run = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const bool eq = valid[i] && key[i] == c.tau;
        const uint64_t beq = __ballot(eq) & r.gmask;
        const int tie = eq_run + (int)__popcll(beq & r.below);
        const bool keep = valid[i] && (key[i] > c.tau || (eq && tie < c.quota));
        const uint64_t bk = __ballot(keep) & r.gmask;
        const uint32_t d = obase + (uint32_t)kept_run + (uint32_t)__popcll(bk & r.below);
        if (keep && d < out_nnz) {
            const uint32_t p = r.start + (uint32_t)(r.j + i * kWave);
            out_col[d] = col_idx[p];
            out_vals[d] = vals[p];
            if (out_map) out_map[d] = p;
        }
        eq_run += (int)__popcll(beq);
        kept_run += (int)__popcll(bk);
    }
}

template <int S>
struct SelSlots {
    static constexpr int value = S;
};

// The wavefront's 64 rows: lane l has loaded (start, len) of row r0 + l, len = -1 where the row is not this walk's.
// f(SelSlots<S>, SelRow, row, source lane) runs once per row: in groups with one slot, or with the whole wavefront and the
// 1, 2, 4 or 8 slots that hold the row (a bisection step costs a ballot per slot, and most rows of a mixed wavefront are short).
template <typename F>
__device__ __forceinline__ void sel_walk(int lane, int64_t r0, uint32_t my_start, int my_len, F f)
{
    int longest = my_len;
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    longest = __builtin_amdgcn_readfirstlane(longest);
    if (longest < 0) return;                       // no row of this walk at all
    if (longest <= kWave) {
        int lg = 0;
        while ((1 << lg) < longest) ++lg;
        const int G = 1 << lg, per = kWave >> lg;  // lanes of a group, rows of a pass
        const int g = lane >> lg;
        SelRow r;
        r.j = lane & (G - 1);
        r.gmask = (G == kWave ? ~0ull : ((1ull << G) - 1ull)) << (g * G);
        r.below = r.gmask & (lane == 0 ? 0ull : (~0ull >> (kWave - lane)));
        for (int t = 0; t < G; ++t) {
            const int src = t * per + g;
            r.start = (uint32_t)__shfl((int)my_start, src);
            r.len = __shfl(my_len, src);
            f(SelSlots<1>{}, r, r0 + src, src);
        }
    } else {
        SelRow r;
        r.j = lane;
        r.gmask = ~0ull;
        r.below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
        for (int t = 0; t < kWave; ++t) {
            r.len = __builtin_amdgcn_readfirstlane(__shfl(my_len, t));
            if (r.len < 0) continue;
            r.start = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)my_start, t));
            if (r.len <= kWave) f(SelSlots<1>{}, r, r0 + t, t);
            else if (r.len <= 2 * kWave) f(SelSlots<2>{}, r, r0 + t, t);
            else if (r.len <= 4 * kWave) f(SelSlots<4>{}, r, r0 + t, t);
            else f(SelSlots<kSelSlots>{}, r, r0 + t, t);
        }
    }
}

// the bounds of row r0 + lane as the walks take them, and which of the 64 rows are long
__device__ __forceinline__ void sel_bounds(int64_t rows, const int32_t *__restrict__ row_ptr, int64_t r0, int lane,
                                           uint32_t &start, int &len, uint64_t &long_rows)
{
    const int64_t row = r0 + lane;
    int b = 0, e = 0;
    if (row < rows) {
        b = row_ptr[row];
        e = row_ptr[row + 1];
    }
    const int n = e - b;
    const bool is_long = row < rows && n > kSelCap;
    long_rows = __ballot(is_long);
    start = (uint32_t)b;
    len = (row < rows && n >= 0 && !is_long) ? n : -1;
}

// the long rows of the workgroup's 256 rows, one after the other (s_long: one mask per wavefront, workgroup-uniform)
template <typename F>
__device__ __forceinline__ void sel_each_long(const uint64_t *s_long, int64_t block_r0, F f)
{
    for (int w = 0; w < kSelWaves; ++w) {
        const uint64_t m = s_long[w];
        uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
        uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32));
        while (lo | hi) {
            int b;
            if (lo) { b = __builtin_ctz(lo); lo &= lo - 1; }
            else { b = 32 + __builtin_ctz(hi); hi &= hi - 1; }
            f(block_r0 + w * kWave + b);
        }
    }
}

template <bool THRESH>
__global__ __launch_bounds__(kBlock) void k_sel_cut(int64_t rows, int64_t nblocks, uint32_t nnz, const int32_t *__restrict__ row_ptr,
                                                    const uint32_t *__restrict__ score, uint32_t absmask, int k, uint32_t thr_key,
                                                    SelCut *__restrict__ cut, int32_t *__restrict__ counts)
{
    __shared__ uint64_t s_long[kSelWaves];
    __shared__ int s_hist[256];
    __shared__ int s_wtot[kSelWaves];
    __shared__ int s_sel[2];
    const int tid = threadIdx.x, lane = sel_lane(), w = tid >> 6;
    const int64_t block_r0 = xcd_item64(blockIdx.x, nblocks) * kSelBlockRows;
    const int64_t r0 = block_r0 + w * kWave;
    uint32_t my_start;
    int my_len;
    uint64_t long_rows;
    sel_bounds(rows, row_ptr, r0, lane, my_start, my_len, long_rows);
    if (lane == 0) s_long[w] = long_rows;
    sel_walk(lane, r0, my_start, my_len, [&](auto slots, const SelRow &r, int64_t row, int) {
        sel_cut_short<decltype(slots)::value, THRESH>(r, row, score, absmask, nnz, k, thr_key, cut, counts);
    });
    __syncthreads();
    sel_each_long(s_long, block_r0, [&](int64_t row) {
        const uint32_t start = (uint32_t)row_ptr[row];
        const int len = row_ptr[row + 1] - row_ptr[row];
        if (THRESH) {
            int c = 0;
            for (int j0 = w * kWave; j0 < len; j0 += kBlock) {
                const int j = j0 + lane;
                const uint32_t p = start + (uint32_t)j;
                const bool ok = j < len && p < nnz;
                c += (int)__popcll(__ballot(ok && sel_key(score[ok ? p : 0u], absmask) >= thr_key));
            }
            if (lane == 0) s_wtot[w] = c;
            __syncthreads();
            if (tid == 0) counts[row] = s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
            __syncthreads();
            return;
        }
        if (len <= k) {
            if (tid == 0) {
                counts[row] = len;
                cut[row] = SelCut{0u, kSelAll};
            }
            return;
        }
        // radix select, most significant digit first: `prefix` are the digits found, `kk` the rank wanted among the keys
        // that share them
        uint32_t prefix = 0u;
        int kk = k;
        for (int pass = 3; pass >= 0; --pass) {
            const int shift = 8 * pass;
            const uint32_t himask = pass == 3 ? 0u : (~0u << (shift + 8));
            s_hist[tid] = 0;
            __syncthreads();
            for (int j0 = w * kWave; j0 < len; j0 += kBlock) {
                const int j = j0 + lane;
                const uint32_t p = start + (uint32_t)j;
                const bool ok = j < len && p < nnz;
                const uint32_t key = sel_key(score[ok ? p : 0u], absmask);
                const bool in = ok && (key & himask) == prefix;
                const int d = (int)((key >> shift) & 255u);
                const uint64_t ins = __ballot(in);
                if (ins == 0) continue;
                // (a wavefront whose keys all have one digit adds once; the result of the atomic is not used)
                const int first = __builtin_ctzll(ins);
                const int d0 = __shfl(d, first);
                if (__ballot(in && d != d0) == 0) {
                    if (lane == first) atomicAdd(&s_hist[d0], (int)__popcll(ins));
                } else if (in) {
                    atomicAdd(&s_hist[d], 1);
                }
            }
            __syncthreads();
            // thread t stands for digit 255 - t: an inclusive scan over t counts the keys of that digit or a larger one
            const int dig = 255 - tid;
            const int c = s_hist[dig];
            int incl = c;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const int v = __shfl_up(incl, o, kWave);
                if (lane >= o) incl += v;
            }
            if (lane == kWave - 1) s_wtot[w] = incl;
            __syncthreads();
            for (int q = 0; q < w; ++q) incl += s_wtot[q];
            if (incl >= kk && incl - c < kk) {      // exactly one digit: the one that holds rank kk
                s_sel[0] = dig;
                s_sel[1] = kk - (incl - c);
            }
            __syncthreads();
            prefix |= (uint32_t)s_sel[0] << shift;
            kk = s_sel[1];
        }
        if (tid == 0) {
            counts[row] = k;
            cut[row] = SelCut{prefix, kk};
        }
        __syncthreads();      // s_sel and s_wtot are the next long row's too
    });
}

// cut == nullptr: every row has the cut (thr_key, all)
__global__ __launch_bounds__(kBlock) void k_sel_compact(int64_t rows, int64_t nblocks, uint32_t nnz, const int32_t *__restrict__ row_ptr,
                                                        const uint32_t *__restrict__ score, uint32_t absmask, uint32_t thr_key,
                                                        const SelCut *__restrict__ cut, const int32_t *__restrict__ out_ptr,
                                                        uint32_t out_nnz, const int32_t *__restrict__ col_idx,
                                                        const uint32_t *__restrict__ vals, int32_t *__restrict__ out_col,
                                                        uint32_t *__restrict__ out_vals, uint32_t *__restrict__ out_map)
{
    __shared__ uint64_t s_long[kSelWaves];
    __shared__ int s_eq[2][kSelWaves], s_kept[2][kSelWaves];
    const int tid = threadIdx.x, lane = sel_lane(), w = tid >> 6;
    const int64_t block_r0 = xcd_item64(blockIdx.x, nblocks) * kSelBlockRows;
    const int64_t r0 = block_r0 + w * kWave;
    uint32_t my_start;
    int my_len;
    uint64_t long_rows;
    sel_bounds(rows, row_ptr, r0, lane, my_start, my_len, long_rows);
    if (lane == 0) s_long[w] = long_rows;
    SelCut my_cut{thr_key, kSelAll};
    uint32_t my_out = 0u;
    if (my_len >= 0) {
        if (cut) my_cut = cut[r0 + lane];
        my_out = (uint32_t)out_ptr[r0 + lane];
    }
    auto row_cut = [&](int src) {
        SelCut c;
        c.tau = (uint32_t)__shfl((int)my_cut.tau, src);
        c.quota = __shfl(my_cut.quota, src);
        return c;
    };
    sel_walk(lane, r0, my_start, my_len, [&](auto slots, const SelRow &r, int64_t, int src) {
        sel_compact_short<decltype(slots)::value>(r, row_cut(src), (uint32_t)__shfl((int)my_out, src), out_nnz, score, absmask, nnz,
                                                  col_idx, vals, out_col, out_vals, out_map);
    });
    __syncthreads();
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
    sel_each_long(s_long, block_r0, [&](int64_t row) {
        const uint32_t start = (uint32_t)row_ptr[row];
        const int len = row_ptr[row + 1] - row_ptr[row];
        const SelCut c = cut ? cut[row] : SelCut{thr_key, kSelAll};
        const uint32_t obase = (uint32_t)out_ptr[row];
        int eq_carry = 0, kept_carry = 0, par = 0;
        for (int tile0 = 0; tile0 < len; tile0 += kSelTile, par ^= 1) {
            uint32_t key[kSelTileSlots];
            bool valid[kSelTileSlots], eq[kSelTileSlots], keep[kSelTileSlots];
            uint64_t beq[kSelTileSlots], bk[kSelTileSlots];
            int weq = 0;
#pragma unroll
            for (int i = 0; i < kSelTileSlots; ++i) {
                const int j = tile0 + (w * kSelTileSlots + i) * kWave + lane;
                const uint32_t p = start + (uint32_t)j;
                valid[i] = j < len && p < nnz;
                key[i] = valid[i] ? sel_key(score[p], absmask) : 0u;
                eq[i] = valid[i] && key[i] == c.tau;
                beq[i] = __ballot(eq[i]);
                weq += (int)__popcll(beq[i]);
            }
            if (lane == 0) s_eq[par][w] = weq;
            __syncthreads();
            int eq_run = eq_carry, eq_all = 0;
#pragma unroll
            for (int q = 0; q < kSelWaves; ++q) {
                const int v = s_eq[par][q];
                if (q < w) eq_run += v;
                eq_all += v;
            }
            int wk = 0;
#pragma unroll
            for (int i = 0; i < kSelTileSlots; ++i) {
                const int tie = eq_run + (int)__popcll(beq[i] & below);
                keep[i] = valid[i] && (key[i] > c.tau || (eq[i] && tie < c.quota));
                bk[i] = __ballot(keep[i]);
                eq_run += (int)__popcll(beq[i]);
                wk += (int)__popcll(bk[i]);
            }
            if (lane == 0) s_kept[par][w] = wk;
            __syncthreads();
            int kept_run = kept_carry, kept_all = 0;
#pragma unroll
            for (int q = 0; q < kSelWaves; ++q) {
                const int v = s_kept[par][q];
                if (q < w) kept_run += v;
                kept_all += v;
            }
#pragma unroll
            for (int i = 0; i < kSelTileSlots; ++i) {
                const uint32_t d = obase + (uint32_t)kept_run + (uint32_t)__popcll(bk[i] & below);
                if (keep[i] && d < out_nnz) {
                    const uint32_t p = start + (uint32_t)(tile0 + (w * kSelTileSlots + i) * kWave + lane);
                    out_col[d] = col_idx[p];
                    out_vals[d] = vals[p];
                    if (out_map) out_map[d] = p;
                }
                kept_run += (int)__popcll(bk[i]);
            }
            eq_carry += eq_all;
            kept_carry += kept_all;
            // (the next tile writes the other half of s_eq / s_kept, and the one after it comes two barriers later)
        }
        __syncthreads();
    });
}

}  // namespace

uint32_t select_key(float score, bool abs)
{
    uint32_t u;
    static_assert(sizeof u == sizeof score, "a float is 32 bits");
    __builtin_memcpy(&u, &score, sizeof u);
    return sel_key(u, abs ? 0x7fffffffu : ~0u);
}

// Device memory while the call runs, beside out's own arrays (4 (rows + 1) + 8 kept bytes, + 4 kept for the map):
//   8 rows (the cuts; top-k only) + 4 (the total) + what exclusive_scan_i32 takes for rows counts (4 bytes per 4096 rows).
int select(const spmv_csr &a, const float *score, bool thresh, int k, uint32_t thr_key, bool abs, bool keep_map, hipStream_t s,
           spmv_csr_t **out)
{
    const int64_t rows = a.rows;
    const uint32_t absmask = abs ? 0x7fffffffu : ~0u;
    const uint32_t *sc = (const uint32_t *)(score ? score : a.d_vals);
    DevPtr<int32_t> rp, ci, total;
    DevPtr<float> va;
    DevPtr<uint32_t> map;
    DevPtr<SelCut> cut;
    SPMV_HIP_TRY(rp.alloc((size_t)rows + 1));
    SPMV_HIP_TRY(total.alloc(1));
    if (!thresh) SPMV_HIP_TRY(cut.alloc((size_t)rows));
    const int64_t nblocks = (rows + kSelBlockRows - 1) / kSelBlockRows;
    int32_t kept = 0;
    if (rows > 0) {
        if (thresh)
            hipLaunchKernelGGL(k_sel_cut<true>, dim3((unsigned)nblocks), dim3(kBlock), 0, s, rows, nblocks, (uint32_t)a.nnz, a.d_row_ptr,
                               sc, absmask, k, thr_key, cut.get(), rp.get());
        else
            hipLaunchKernelGGL(k_sel_cut<false>, dim3((unsigned)nblocks), dim3(kBlock), 0, s, rows, nblocks, (uint32_t)a.nnz, a.d_row_ptr,
                               sc, absmask, k, thr_key, cut.get(), rp.get());
        if (int rc = check_launch("k_sel_cut")) return rc;
        if (int rc = scan_offsets_i32(rp.get(), rows, total.get(), true, s, &kept)) return rc;
    } else {
        SPMV_HIP_TRY(hipMemsetAsync(rp.get(), 0, sizeof(int32_t), s));
    }
    SPMV_HIP_TRY(ci.alloc((size_t)kept));
    SPMV_HIP_TRY(va.alloc((size_t)kept));
    if (keep_map) SPMV_HIP_TRY(map.alloc((size_t)kept));
    if (kept > 0) {
        hipLaunchKernelGGL(k_sel_compact, dim3((unsigned)nblocks), dim3(kBlock), 0, s, rows, nblocks, (uint32_t)a.nnz, a.d_row_ptr, sc,
                           absmask, thr_key, (const SelCut *)cut.get(), (const int32_t *)rp.get(), (uint32_t)kept, a.d_col_idx,
                           (const uint32_t *)a.d_vals, ci.get(), (uint32_t *)va.get(), map.get());
        if (int rc = check_launch("k_sel_compact")) return rc;
    }
    SPMV_HIP_TRY(hipStreamSynchronize(s));   // the cuts are freed on return

    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("spmv_csr_select: out of host memory"); return SPMV_ERR_INVALID; }
    h->rows = a.rows; h->cols = a.cols; h->nnz = kept;
    h->device = a.device;
    h->d_row_ptr = rp; h->d_col_idx = ci; h->d_vals = va;
    h->own_row_ptr = std::move(rp); h->own_col_idx = std::move(ci); h->own_vals = std::move(va);
    h->map.parent_len = a.nnz;
    if (keep_map) {
        h->map.words = std::move(map);
        h->map.maker = MapMaker::select;
    }
    *out = h;
    return SPMV_OK;
}

}  // namespace spmv
