// kernels_transpose.hip -- spmv_csr_transpose / spmv_csr_transpose_values: T = A^T as a new CSR handle, built on the device.
//
// The job is a STABLE sort of the nonzero positions k of A by column, a histogram of the columns (T's row_ptr) and two
// gathers (T's col_idx = the row of every position, T's vals).  The order of equal columns is A's storage order and must not
// depend on scheduling, so no rank in this file comes from the value an atomic returns: the only atomics are integer
// counter increments whose result is not used (a count does not depend on the order of arrival).
//
//   1. k_tr_count      col_idx -> counters[cols + 1]; exclusive_scan_i32 makes them T's row_ptr.
//   2. per 8-bit digit of the column, least significant first (ceil(bits(col_max) / 8) passes):
//        k_tr_hist     tile (kTrTile consecutive elements: a function of nnz alone) -> table[digit][tile]
//        exclusive_scan_i32 over the table in that (digit-major) order
//        k_tr_scatter  rank inside the tile from lane order (ballots per digit bit, wavefront totals through LDS in
//                      wavefront order), the tile staged per digit in LDS and written as runs
//      pass 0 reads A's col_idx and takes the position from the index; the last pass writes no keys.
//   3. k_tr_rows       row of every position k (a search of A's row_ptr, coherent inside a wavefront: neighbours share
//                      the path), then k_tr_gather twice: T.col_idx[i] = row[map[i]], T.vals[i] = A.vals[map[i]].
//
// Positions are unsigned 32-bit (nnz < 2^31), byte offsets 64-bit; no launch has more than 2^21 workgroups.  Every access
// is predicated on its array's own length: nothing here relies on slack behind an array.
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

namespace {

constexpr int kTrTile = 4096;                         // elements of a tile: 4 wavefronts x 16 rounds x 64 lanes
constexpr int kTrRounds = kTrTile / kBlock;           // 16
constexpr int kTrWaves = kBlock / kWave;              // 4
constexpr int kTrWaveSpan = kTrRounds * kWave;        // 1024 consecutive elements per wavefront

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// counters[c] += 1 for every column (the result of the atomic is not used).  A wavefront whose 64 columns are all the
// same adds once.
__global__ __launch_bounds__(kBlock) void k_tr_count(int64_t nnz, int64_t cols, const int32_t *__restrict__ col_idx,
                                                     int32_t *__restrict__ counters)
{
    const int lane = lane_id();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); k0 < nnz; k0 += stride) {
        const int64_t k = k0 + lane;
        const bool valid = k < nnz;
        const int c = valid ? col_idx[k] : -1;
        const bool ok = valid && c >= 0 && (int64_t)c < cols;
        const int c0 = __builtin_amdgcn_readfirstlane(c);
        const uint64_t oks = __ballot(ok);
        if (__ballot(ok && c != c0) == 0) {
            if (lane == 0 && oks) atomicAdd(&counters[c0], (int)__popcll(oks));   // lane 0 is ok whenever anybody is
        } else if (ok) {
            atomicAdd(&counters[c], 1);
        }
    }
}

// table[digit * tiles + tile] = how many keys of the tile have that digit
__global__ __launch_bounds__(kBlock) void k_tr_hist(uint32_t n, const uint32_t *__restrict__ keys, int shift, uint32_t tiles,
                                                    int32_t *__restrict__ table)
{
    __shared__ int cnt[256];
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    cnt[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTrTile + w * kTrWaveSpan + lane;
#pragma unroll 4
    for (int i = 0; i < kTrRounds; ++i) {
        const int64_t idx = base + i * kWave;
        const bool valid = idx < (int64_t)n;
        const int d = valid ? (int)((keys[idx] >> shift) & 255u) : 256;
        const int d0 = __builtin_amdgcn_readfirstlane(d);
        const uint64_t vs = __ballot(valid);
        if (__ballot(valid && d != d0) == 0) {
            if (lane == 0 && vs) atomicAdd(&cnt[d0], (int)__popcll(vs));      // the valid lanes are a prefix of the wavefront
        } else if (valid) {
            atomicAdd(&cnt[d], 1);
        }
    }
    __syncthreads();
    table[(int64_t)tid * tiles + blockIdx.x] = cnt[tid];
}

// One tile: (key, position) pairs to their places of this pass.  `table` is the scanned table of k_tr_hist.
// pos_in == nullptr: the position is the index (pass 0); key_out == nullptr: the last pass, keys are not needed again.
__global__ __launch_bounds__(kBlock) void k_tr_scatter(uint32_t n, const uint32_t *__restrict__ key_in,
                                                       const uint32_t *__restrict__ pos_in, int shift, uint32_t tiles,
                                                       const int32_t *__restrict__ table, uint32_t *__restrict__ key_out,
                                                       uint32_t *__restrict__ pos_out)
{
    __shared__ int wcnt[kTrWaves][256];     // per wavefront: running count of every digit, then its offset inside the digit's run
    __shared__ int dstart[256];             // where the digit's run starts in the staged tile
    __shared__ int gbase[256];              // global place of the run's first element minus dstart
    __shared__ int wtot[kTrWaves];
    __shared__ uint32_t skey[kTrTile], spos[kTrTile];
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
#pragma unroll
    for (int j = 0; j < kTrWaves; ++j) wcnt[j][tid] = 0;
    __syncthreads();

    const int64_t tile0 = (int64_t)blockIdx.x * kTrTile;
    const int64_t base = tile0 + w * kTrWaveSpan + lane;
    const uint64_t below_me = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    volatile int *mine = wcnt[w];
    uint32_t key[kTrRounds], pos[kTrRounds];
    int rank[kTrRounds];
#pragma unroll
    for (int i = 0; i < kTrRounds; ++i) {
        const int64_t idx = base + i * kWave;
        const bool valid = idx < (int64_t)n;
        key[i] = valid ? key_in[idx] : 0u;
        pos[i] = (valid && pos_in) ? pos_in[idx] : (uint32_t)idx;
    }
    // rank inside the wavefront: round after round, inside a round by lane number
#pragma unroll
    for (int i = 0; i < kTrRounds; ++i) {
        const bool valid = base + i * kWave < (int64_t)n;
        const int d = (int)((key[i] >> shift) & 255u);
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const int before = (int)__popcll(same & below_me);
        const int seen = mine[d];
        __builtin_amdgcn_wave_barrier();
        if (valid && before == 0) mine[d] = seen + (int)__popcll(same);      // the lowest lane of every digit present
        __builtin_amdgcn_wave_barrier();
        rank[i] = seen + before;
    }
    __syncthreads();
    // thread = digit: wavefront totals -> offsets in wavefront order; the runs' starts = exclusive scan over the digits
    {
        int run = 0;
#pragma unroll
        for (int j = 0; j < kTrWaves; ++j) {
            const int c = wcnt[j][tid];
            wcnt[j][tid] = run;
            run += c;
        }
        int incl = run;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int v = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += v;
        }
        if (lane == kWave - 1) wtot[w] = incl;
        __syncthreads();
        int add = 0;
        for (int j = 0; j < w; ++j) add += wtot[j];
        const int start = add + incl - run;
        dstart[tid] = start;
        gbase[tid] = table[(int64_t)tid * tiles + blockIdx.x] - start;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTrRounds; ++i) {
        if (base + i * kWave < (int64_t)n) {
            const int d = (int)((key[i] >> shift) & 255u);
            const int loc = dstart[d] + wcnt[w][d] + rank[i];
            skey[loc] = key[i];
            spos[loc] = pos[i];
        }
    }
    __syncthreads();
    const int64_t left = (int64_t)n - tile0;
    const int count = left < kTrTile ? (int)left : kTrTile;
#pragma unroll 4
    for (int i = 0; i < kTrRounds; ++i) {
        const int loc = i * kBlock + tid;
        if (loc < count) {
            const uint32_t k = skey[loc];
            const int64_t dst = (int64_t)gbase[(k >> shift) & 255u] + loc;
            if (dst >= 0 && dst < (int64_t)n) {
                if (key_out) key_out[dst] = k;
                pos_out[dst] = spos[loc];
            }
        }
    }
}

// row_of[k] = the row that holds position k: the last r with row_ptr[r] <= k.  Four consecutive k per lane.
__device__ __forceinline__ int64_t tr_row_search(const int32_t *__restrict__ row_ptr, int64_t lo, int64_t hi, int64_t k)
{
    // invariant: row_ptr[lo] <= k < row_ptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)row_ptr[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void k_tr_rows(int64_t nnz, int64_t rows, const int32_t *__restrict__ row_ptr,
                                                    int32_t *__restrict__ row_of)
{
    const int64_t k0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (k0 >= nnz) return;
    int64_t r = tr_row_search(row_ptr, 0, rows, k0);
    int32_t out[4];
    out[0] = (int32_t)r;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const int64_t k = k0 + j;
        if (k < nnz && (int64_t)row_ptr[r + 1] <= k) r = tr_row_search(row_ptr, r + 1, rows, k);
        out[j] = (int32_t)r;
    }
    if (k0 + 4 <= nnz) {
        *reinterpret_cast<int4 *>(row_of + k0) = make_int4(out[0], out[1], out[2], out[3]);   // row_of is an allocation of its own: aligned
    } else {
        for (int j = 0; k0 + j < nnz; ++j) row_of[k0 + j] = out[j];
    }
}

// dst[i] = src[map[i]], 32-bit words copied as bits.  Four consecutive i per lane: map and dst are streams.
__global__ __launch_bounds__(kBlock) void k_tr_gather(int64_t n, const uint32_t *__restrict__ map, const uint32_t *__restrict__ src,
                                                      uint32_t *__restrict__ dst)
{
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i0 >= n) return;
    if (i0 + 4 <= n) {
        const uint4 m = *reinterpret_cast<const uint4 *>(map + i0);
        uint4 v;
        v.x = (int64_t)m.x < n ? src[m.x] : 0u;
        v.y = (int64_t)m.y < n ? src[m.y] : 0u;
        v.z = (int64_t)m.z < n ? src[m.z] : 0u;
        v.w = (int64_t)m.w < n ? src[m.w] : 0u;
        *reinterpret_cast<uint4 *>(dst + i0) = v;
    } else {
        for (int64_t i = i0; i < n; ++i) {
            const uint32_t m = map[i];
            dst[i] = (int64_t)m < n ? src[m] : 0u;
        }
    }
}

unsigned blocks_of4(int64_t n) { return (unsigned)((n + (int64_t)kBlock * 4 - 1) / ((int64_t)kBlock * 4)); }

int launch_gather(int64_t n, const uint32_t *map, const void *src, void *dst, hipStream_t s)
{
    if (n <= 0) return SPMV_OK;
    k_tr_gather<<<dim3(blocks_of4(n)), dim3(kBlock), 0, s>>>(n, map, (const uint32_t *)src, (uint32_t *)dst);
    return check_launch("k_tr_gather");
}

}  // namespace

int transpose_values(spmv_csr &t, const spmv_csr &a, hipStream_t s)
{
    return launch_gather(t.nnz, t.map.words.get(), a.d_vals, t.own_vals.get(), s);
}

// Device memory while the call runs, beside T's own arrays (8 nnz + 4 (cols + 1) bytes):
//   16 nnz (two position buffers, one of which becomes the map; two key buffers, the first also holds the rows)
//   + 1024 ceil(nnz / 4096) (the tile table) + what exclusive_scan_i32 takes for it (1 byte per 4096 table bytes).
int transpose(const spmv_csr &a, bool keep_map, hipStream_t s, spmv_csr_t **out)
{
    const int64_t nnz = a.nnz, trows = a.cols;
    DevPtr<int32_t> rp, ci, total, range;
    DevPtr<float> va;
    DevPtr<uint32_t> pos[2], key[2];
    DevPtr<int32_t> table;
    SPMV_HIP_TRY(rp.alloc((size_t)trows + 1));
    SPMV_HIP_TRY(ci.alloc((size_t)nnz));
    SPMV_HIP_TRY(va.alloc((size_t)nnz));
    SPMV_HIP_TRY(total.alloc(1));
    if (nnz == 0 && keep_map) SPMV_HIP_TRY(pos[0].alloc(0));   // an empty map is still a map
    SPMV_HIP_TRY(hipMemsetAsync(rp.get(), 0, sizeof(int32_t) * ((size_t)trows + 1), s));

    int passes = 0;
    if (nnz > 0) {
        SPMV_HIP_TRY(range.alloc(2));
        if (int rc = launch_column_range(a, range.get(), s)) return rc;
        int32_t r2[2] = {0, -1};
        SPMV_HIP_TRY(hipMemcpyAsync(r2, range.get(), sizeof r2, hipMemcpyDeviceToHost, s));
        SPMV_HIP_TRY(hipStreamSynchronize(s));
        passes = 1;
        while (passes < 4 && ((uint32_t)r2[1] >> (8 * passes)) != 0) ++passes;
    }
    const int64_t tiles = (nnz + kTrTile - 1) / kTrTile;
    if (nnz > 0) {
        SPMV_HIP_TRY(pos[0].alloc((size_t)nnz));
        if (passes >= 2) SPMV_HIP_TRY(pos[1].alloc((size_t)nnz));
        SPMV_HIP_TRY(key[0].alloc((size_t)nnz));
        if (passes >= 3) SPMV_HIP_TRY(key[1].alloc((size_t)nnz));
        SPMV_HIP_TRY(table.alloc((size_t)tiles * 256));

        int64_t blocks = (nnz + kBlock * 16 - 1) / (kBlock * 16);
        if (blocks > 256 * 32) blocks = 256 * 32;
        k_tr_count<<<dim3((unsigned)blocks), dim3(kBlock), 0, s>>>(nnz, trows, a.d_col_idx, rp.get());
        if (int rc = check_launch("k_tr_count")) return rc;
    }
    if (int rc = exclusive_scan_i32(rp.get(), trows + 1, total.get(), s)) return rc;

    int final_pos = 0;
    for (int p = 0; p < passes; ++p) {
        const uint32_t *kin = p == 0 ? (const uint32_t *)a.d_col_idx : key[(p - 1) & 1].get();
        const uint32_t *pin = p == 0 ? nullptr : pos[(p - 1) & 1].get();
        uint32_t *kout = p == passes - 1 ? nullptr : key[p & 1].get();
        uint32_t *pout = pos[p & 1].get();
        k_tr_hist<<<dim3((unsigned)tiles), dim3(kBlock), 0, s>>>((uint32_t)nnz, kin, 8 * p, (uint32_t)tiles, table.get());
        if (int rc = check_launch("k_tr_hist")) return rc;
        if (int rc = exclusive_scan_i32(table.get(), tiles * 256, total.get(), s)) return rc;
        k_tr_scatter<<<dim3((unsigned)tiles), dim3(kBlock), 0, s>>>((uint32_t)nnz, kin, pin, 8 * p, (uint32_t)tiles, table.get(),
                                                                      kout, pout);
        if (int rc = check_launch("k_tr_scatter")) return rc;
        final_pos = p & 1;
    }
    if (nnz > 0) {
        int32_t *row_of = (int32_t *)key[0].get();     // the keys are done with
        k_tr_rows<<<dim3(blocks_of4(nnz)), dim3(kBlock), 0, s>>>(nnz, a.rows, a.d_row_ptr, row_of);
        if (int rc = check_launch("k_tr_rows")) return rc;
        if (int rc = launch_gather(nnz, pos[final_pos].get(), row_of, ci.get(), s)) return rc;
        if (int rc = launch_gather(nnz, pos[final_pos].get(), a.d_vals, va.get(), s)) return rc;
    }
    SPMV_HIP_TRY(hipStreamSynchronize(s));   // the temporaries are freed on return

    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("spmv_csr_transpose: out of host memory"); return SPMV_ERR_INVALID; }
    h->rows = a.cols; h->cols = a.rows; h->nnz = nnz;
    h->device = a.device;
    h->d_row_ptr = rp; h->d_col_idx = ci; h->d_vals = va;
    h->own_row_ptr = std::move(rp); h->own_col_idx = std::move(ci); h->own_vals = std::move(va);
    if (keep_map) {
        h->map.words = std::move(pos[final_pos]);
        h->map.parent_len = nnz;
        h->map.maker = MapMaker::transpose;
    }
    *out = h;
    return SPMV_OK;
}

}  // namespace spmv
