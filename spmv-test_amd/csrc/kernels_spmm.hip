// kernels_spmm.hip -- Y = A X for k <= 64 right-hand sides at once (spmv_csr_spmm, include/spmv_hip.h "SpMM"), and for any
// k in column tiles of 64 (spmv_csr_spmm_cols: "Column tiles" below).
//
// The lane groups and their steps are lane_group.hpp's; the plan they share with SDDMM and attention is made here.  X is
// cols rows of ldx floats (row-major), Y rows rows of ldy floats.  Lane s of a row's group holds columns [4s, 4s+4) of
// Y's row in four accumulators; per step the group loads (col_idx, vals) coalesced, broadcasts them, issues all T slice
// gathers of X and only then multiplies and adds, one nonzero after the other.
//
// The order of the fp32 additions of column c is fixed by the row alone: acc = fma(v, x, acc) over the row's nonzeros in
// storage order, from +0 -- the same for every V, every ld and every position of c in the batch (batch invariance).  Rows
// longer than kSpmmRowCap nonzeros are cut by the plan into pieces of kSpmmPiece nonzeros (plan-fixed boundaries); a
// group sums each piece the same way into a partial of 64 floats, and k_spmm_combine adds a row's partials in piece
// order (from +0).  Nothing here depends on k but how many columns are computed and stored.
//
// X and Y may exceed 4 GiB (c4 at k = 64 is 4.3 GB each).  A lane whose slice starts at or past k does nothing.
//
// Element types.  Every kernel here takes the element type E of X and Y as its last template argument: float
// (spmv_csr_spmm) or 16-bit storage (bf16, fp16: spmv_csr_spmm_16).  The text above is E = float.  With 16-bit E nothing
// of the order changes: a step's gathered slices wait packed as loaded (slice_t<E>, 2 registers per slice), each is
// widened exactly to fp32 where it enters its fmaf, vals, the accumulators and the long rows' partials are fp32, and an
// element of Y is rounded to E once, to nearest even, at its store (store_slice; a long row's in k_spmm_combine, after
// the partials are added in piece order).  So Y of a 16-bit call is the fp32 call's Y on the widened X, rounded once.
//
// Column tiles (spmv_csr_spmm_cols, the TILED instantiations).  Tile t of a call at width k is the columns [64t, 64t + k_t),
// k_t = min(64, k - 64t), of m = ceil(k / 64) tiles.  The three kernels run once per tile in one launch each: the tile index
// rides in the grid (cols_tile), a tile's workgroups see X and Y advanced by 64t elements and k_t in the place of k, and do
// what the narrow call does on that column block at V = 16 (the idle lanes of a narrower last tile load nothing), so a
// column's bits are the narrow call's.  Each tile re-reads (col_idx, vals): 8 bytes per nonzero against up to 256 bytes of
// gathered X.  The long rows' partials go to a scratch of the plan's own (spmv_csr_spmm_plan_cols): piece p holds m * 64
// floats, column c of the call at offset c (64-bit offsets).
//
// One body per kernel, one launch function.  A kernel without TILED is the TILED one at m = 1, tile 0, the row block
// blockIdx.x: its `if constexpr (TILED)` is the only place that differs.  launch_spmm<E> is the one way in for the three
// entry points of an element type (`cols`: column tiles; `who`: the entry point's name for a refusal); launch_spmm_v
// issues the three launches of either kind: V from dispatch_lanes or kColsV, the grid plain or cols_grid, the scratch
// d_partial or d_partial_cols.
#include <algorithm>
#include <numeric>
#include <vector>
#include "lane_group.hpp"

namespace spmv {

namespace {

constexpr int kSpmmRowCap = 512;    // rows of more nonzeros go in pieces
constexpr int kSpmmPiece = 512;     // nonzeros of a piece
constexpr int kSpmmMaxK = 64;       // columns of a piece's partial (the scratch is sized for k = 64 at plan time)
constexpr int kSpmmSortRows = 4096; // the plan orders the rows of each block of this many by length (a wave's rows alike)

// Where the tile index of a TILED launch rides.  The default is blockIdx.y, as the heads of fused attention: workgroups are
// dispatched x-fastest, so all row blocks of tile 0 run before tile 1's.  SPMV_COLS_TILE_MINOR (an A/B build,
// tools/build_variant.sh) puts it in the low part of blockIdx.x instead: the m tiles of one row block run next to each
// other in time and re-read that block's (col_idx, vals) from cache.  DESIGN.md section 22 has both timings.
#ifdef SPMV_COLS_TILE_MINOR
constexpr bool kTileMinor = true;
#else
constexpr bool kTileMinor = false;
#endif

// (the tile of the workgroup, the index of its row block or block of pieces) of a TILED launch at width k
__device__ __forceinline__ int cols_tile(int k, int64_t &bid)
{
    if constexpr (kTileMinor) {
        const int m = cols_tiles(k);
        bid = blockIdx.x / m;
        return (int)(blockIdx.x % m);
    } else {
        bid = blockIdx.x;
        return (int)blockIdx.y;
    }
}

inline dim3 cols_grid(int64_t blocks, int m) { return kTileMinor ? dim3((unsigned)(blocks * m)) : dim3((unsigned)blocks, (unsigned)m); }

// sum over the nonzeros [b, e) of the group's row (or piece) of vals[n] * X[col_idx[n]][c0 .. c0+3], in storage order.
// All lanes of a group call it with the same b, e; lanes with c0 >= k load and add nothing (their shuffles still run).
template <int V, bool VEC, typename E>
__device__ __forceinline__ float4 row_dot(int lane, int64_t b, int64_t e, const int32_t *__restrict__ col_idx,
                                          const float *__restrict__ vals, const E *__restrict__ X, int64_t ldx, int c0,
                                          int k)
{
    constexpr int T = LaneGeom<V>::T, L = LaneGeom<V>::L;
    const int sub = lane & (V - 1), gbase = lane & ~(V - 1);
    const bool active = c0 < k;
    float4 acc = zero4();
    for (int64_t kb = b; kb < e; kb += T) {
        // group_columns and group_bcast for the pair (col_idx, vals), written pairwise: a nonzero's two loads under one
        // test and its two shuffles side by side (one after the other they cost the kernels up to a VGPR, V = 8 and 16)
        int32_t c[L], ct[T];
        float v[L], vt[T];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int64_t n = kb + (int64_t)i * V + sub;
            c[i] = n < e ? col_idx[n] : 0;
            v[i] = n < e ? vals[n] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            ct[t] = V == 1 ? c[t] : __shfl(c[t / V], gbase + t % V);
            vt[t] = V == 1 ? v[t] : __shfl(v[t / V], gbase + t % V);
        }
        slice_t<E> xt[T];
#pragma unroll
        for (int t = 0; t < T; ++t) xt[t] = (active && kb + t < e) ? load_slice<VEC>(X, ldx, ct[t], c0, k) : zero_slice<E>();
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (kb + t < e) {     // (a slot past the end adds nothing, not even +0: lane_group.hpp)
                // (16-bit E: the packed words pass through widen_again's empty statement, so that no slice is widened
                // before its turn and waits in 4 registers instead of 2)
                const float4 x = widen_again<E>(xt[t]);
                acc.x = fmaf(vt[t], x.x, acc.x);
                acc.y = fmaf(vt[t], x.y, acc.y);
                acc.z = fmaf(vt[t], x.z, acc.z);
                acc.w = fmaf(vt[t], x.w, acc.w);
            }
        }
    }
    return acc;
}

// the operands of a launch (by value); E: the element type of X and Y, whose ld count elements of E
template <typename E>
struct SpmmArgs {
    const float *vals;
    const E *X;
    int64_t ldx;
    E *Y;
    int64_t ldy;
    int k;
};

// the launch's operands as tile `tile` sees them: X and Y advanced to the tile's first column, k its width
template <typename E>
__device__ __forceinline__ void cols_advance(SpmmArgs<E> &a, int tile)
{
    a.X += (int64_t)kColsTile * tile;
    a.Y += (int64_t)kColsTile * tile;
    a.k = min(kColsTile, a.k - kColsTile * tile);
}

// a group of V lanes per row; rows of more than row_cap nonzeros are left to the pieces and the combine
// (TILED: per column tile of a _cols call, a.k the call's whole width)
template <int V, bool VEC, typename E, bool TILED = false>
__global__ __launch_bounds__(kBlock) void k_spmm_rows(GroupRows g, SpmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1), c0 = 4 * (lane & (V - 1));
    int64_t bid = blockIdx.x;
    if constexpr (TILED) cols_advance(a, cols_tile(a.k, bid));
    const int64_t r = group_row<V>(g, bid);
    if (r < 0) return;
    const int64_t b = g.row_ptr[r], e = g.row_ptr[r + 1];
    if (e - b > g.row_cap) return;
    const float4 acc = row_dot<V, VEC>(lane, b, e, g.col_idx, a.vals, a.X, a.ldx, c0, a.k);
    if (c0 < a.k) store_slice<VEC>(a.Y + r * a.ldy + c0, acc, c0, a.k);
}

// a group of V lanes per piece of a long row: scratch[p][0 .. 4V) (the plan's d_partial, kSpmmMaxK floats per piece)
// (TILED: scratch[p][64 tile + (0 .. 4V)) of the plan's d_partial_cols, cols_tiles(k) * 64 floats per piece)
template <int V, bool VEC, typename E, bool TILED = false>
__global__ __launch_bounds__(kBlock) void k_spmm_pieces(GroupPieces g, SpmmArgs<E> a)
{
    const int lane = threadIdx.x & (kWave - 1), c0 = 4 * (lane & (V - 1));
    int64_t bid = blockIdx.x;
    int m = 1, tile = 0;
    if constexpr (TILED) {
        m = cols_tiles(a.k), tile = cols_tile(a.k, bid);
        cols_advance(a, tile);
    }
    const int64_t p = group_piece<V>(g, bid);
    if (p < 0) return;
    const int64_t b = g.piece_k0[p], e = b + g.piece_len[p];
    const float4 acc = row_dot<V, VEC>(lane, b, e, g.col_idx, a.vals, a.X, a.ldx, c0, a.k);
    if (c0 < a.k) *reinterpret_cast<float4 *>(g.scratch + (p * m + tile) * kColsTile + c0) = acc;
}

// one thread per (long row, column < k): the row's partials added in piece order, the sum rounded to E at its store
// (TILED: per column tile, one thread per (long row, column of the tile); a piece's partials are cols_tiles(k) * 64 floats)
template <typename E, bool TILED = false>
__global__ __launch_bounds__(kBlock) void k_spmm_combine(int n_long, const int32_t *__restrict__ long_row,
                                                             const int32_t *__restrict__ long_first,
                                                             const float *__restrict__ partial, E *__restrict__ Y,
                                                             int64_t ldy, int k)
{
    int64_t bid = blockIdx.x;
    int m = 1, tile = 0, kt = k;
    if constexpr (TILED) {
        m = cols_tiles(k), tile = cols_tile(k, bid);
        kt = min(kColsTile, k - kColsTile * tile);
    }
    const int64_t t = bid * kBlock + threadIdx.x;
    const int64_t i = t / kt;
    const int c = kColsTile * tile + (int)(t % kt);
    if (i >= n_long) return;
    float acc = 0.0f;
    for (int p = long_first[i]; p < long_first[i + 1]; ++p) acc += partial[(int64_t)p * m * kColsTile + c];
    store_slice<false>(Y + (int64_t)long_row[i] * ldy + c, make_float4(acc, 0.0f, 0.0f, 0.0f), 0, 1);     // (one column)
}

}  // namespace

// The plan: the rows of more than kSpmmRowCap nonzeros and their pieces, in row order -- a function of row_ptr alone.
// Reads row_ptr back to the host once and waits for the stream (not graph-capturable; spmv_csr_spmm is).
int plan_spmm(spmv_csr &h, hipStream_t s)
{
    if (h.plan_spmm.ready) return SPMV_OK;
    h.plan_spmm = SpmmPlan{};
    std::vector<int32_t> rp((size_t)h.rows + 1);
    SPMV_HIP_TRY(hipMemcpyAsync(rp.data(), h.d_row_ptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> lr, lf, k0, ln;
    for (int64_t r = 0; r < h.rows; ++r) {
        const int32_t b = rp[(size_t)r], e = rp[(size_t)r + 1];
        if (e - b <= kSpmmRowCap) continue;
        lr.push_back((int32_t)r);
        lf.push_back((int32_t)k0.size());
        for (int64_t q = b; q < e; q += kSpmmPiece) {   // (64 bits: q + kSpmmPiece passes INT_MAX on a row that ends near it)
            k0.push_back((int32_t)q);
            ln.push_back((int32_t)(e - q < kSpmmPiece ? e - q : kSpmmPiece));
        }
    }
    lf.push_back((int32_t)k0.size());
    // the rows of every block of kSpmmSortRows, stably by length: the 64 / V rows a wavefront walks side by side end at
    // nearly the same step, and the block's rows still share their window of X.  V = 1 (k <= 4) keeps the row order:
    // there each lane streams its own row's col_idx / vals, and neighbouring rows keep those loads on neighbouring lines
    // (measured: 2x faster at k = 1 and 4 on configs 3 and 4; from V = 2 on the sorted order wins, up to 2.5x)
    std::vector<int32_t> order((size_t)h.rows);
    std::iota(order.begin(), order.end(), 0);
    for (int64_t r0 = 0; r0 < h.rows; r0 += kSpmmSortRows) {
        const int64_t r1 = std::min<int64_t>(h.rows, r0 + kSpmmSortRows);
        std::stable_sort(order.begin() + r0, order.begin() + r1, [&](int32_t a, int32_t b) {
            return rp[(size_t)a + 1] - rp[(size_t)a] < rp[(size_t)b + 1] - rp[(size_t)b];
        });
    }
    SpmmPlan p;
    p.n_long = (int)lr.size();
    p.pieces = (int)k0.size();
    DevPtr<int32_t> d_ord, d_lr, d_lf, d_k0, d_ln;
    SPMV_HIP_TRY(d_ord.alloc(order.size()));
    SPMV_HIP_TRY(hipMemcpyAsync(d_ord.get(), order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, s));
    DevPtr<float> d_part;
    SPMV_HIP_TRY(d_lr.alloc(lr.size()));
    SPMV_HIP_TRY(d_lf.alloc(lf.size()));
    SPMV_HIP_TRY(d_k0.alloc(k0.size()));
    SPMV_HIP_TRY(d_ln.alloc(ln.size()));
    SPMV_HIP_TRY(d_part.alloc((size_t)p.pieces * kSpmmMaxK));
    if (p.n_long) {
        SPMV_HIP_TRY(hipMemcpyAsync(d_lr.get(), lr.data(), sizeof(int32_t) * lr.size(), hipMemcpyHostToDevice, s));
        SPMV_HIP_TRY(hipMemcpyAsync(d_k0.get(), k0.data(), sizeof(int32_t) * k0.size(), hipMemcpyHostToDevice, s));
        SPMV_HIP_TRY(hipMemcpyAsync(d_ln.get(), ln.data(), sizeof(int32_t) * ln.size(), hipMemcpyHostToDevice, s));
    }
    SPMV_HIP_TRY(hipMemcpyAsync(d_lf.get(), lf.data(), sizeof(int32_t) * lf.size(), hipMemcpyHostToDevice, s));
    SPMV_HIP_TRY(hipStreamSynchronize(s));     // (the host vectors die with this call)
    p.d_order = std::move(d_ord);
    p.d_long_row = std::move(d_lr);
    p.d_long_first = std::move(d_lf);
    p.d_piece_k0 = std::move(d_k0);
    p.d_piece_len = std::move(d_ln);
    p.d_partial = std::move(d_part);
    p.row_cap = kSpmmRowCap;
    p.piece_len = kSpmmPiece;
    p.ready = true;
    h.plan_spmm = std::move(p);
    return SPMV_OK;
}

// The plan of the _cols calls: the plan above and, for the long rows' partials at widths up to k_max, a scratch of its own
// of pieces * cols_tiles(k_max) * 64 floats: a separate allocation, the narrow calls' d_partial keeps its size.  It only
// grows; the scratch it replaces may still be read by work on `s`, so that is waited for before the old block goes.
int plan_spmm_cols(spmv_csr &h, int k_max, hipStream_t s)
{
    if (int rc = plan_spmm(h, s)) return rc;
    SpmmPlan &p = h.plan_spmm;
    if (p.cols_k >= k_max) return SPMV_OK;
    if (cols_tiles(k_max) > cols_tiles(p.cols_k)) {
        DevPtr<float> scratch;
        SPMV_HIP_TRY(scratch.alloc((size_t)p.pieces * (size_t)cols_tiles(k_max) * kColsTile));
        if (p.cols_k) SPMV_HIP_TRY(hipStreamSynchronize(s));
        p.d_partial_cols = std::move(scratch);
    }
    p.cols_k = k_max;
    return SPMV_OK;
}

int64_t spmm_plan_bytes(const spmv_csr &h)
{
    const SpmmPlan &p = h.plan_spmm;
    if (!p.ready) return 0;
    return h.rows * 4 + (int64_t)p.n_long * 4 + ((int64_t)p.n_long + 1) * 4 + (int64_t)p.pieces * 8 + (int64_t)p.pieces * kSpmmMaxK * 4 +
           (int64_t)p.pieces * cols_tiles(p.cols_k) * kColsTile * 4;
}

// the three launches of a call (TILED: each over all m column tiles); who: the entry point, for a refusal
template <int V, bool VEC, typename E, bool TILED>
static int launch_spmm_v(const spmv_csr &h, const char *who, const SpmmArgs<E> &a, hipStream_t s)
{
    const SpmmPlan &p = h.plan_spmm;
    const int m = TILED ? cols_tiles(a.k) : 1;
    const int64_t nblocks = TILED ? group_tile_blocks(who, h, V, m) : group_row_blocks(who, h, V);
    if (nblocks < 0) return SPMV_ERR_INVALID;
    const auto grid = [&](int64_t blocks) { return TILED ? cols_grid(blocks, m) : dim3((unsigned)blocks); };
    float *partial = TILED ? p.d_partial_cols : p.d_partial;
    hipLaunchKernelGGL((k_spmm_rows<V, VEC, E, TILED>), grid(nblocks), dim3(kBlock), 0, s, group_rows(h, V, nblocks), a);
    SPMV_LAUNCHED("k_spmm_rows");
    if (!p.n_long) return SPMV_OK;
    hipLaunchKernelGGL((k_spmm_pieces<V, VEC, E, TILED>), grid(group_grid(p.pieces, V).x), dim3(kBlock), 0, s, group_pieces(h, partial), a);
    SPMV_LAUNCHED("k_spmm_pieces");
    // (TILED: the threads of a tile; a narrower last tile leaves some idle)
    const int64_t blocks = ((int64_t)p.n_long * (TILED ? kColsTile : a.k) + kBlock - 1) / kBlock;
    if (TILED && blocks * m * kBlock >= (1LL << 32)) {
        set_error("%s: %d long rows x %d column tiles reach the launch limit of 2^32 work-items", who, p.n_long, m);
        return SPMV_ERR_INVALID;
    }
    hipLaunchKernelGGL((k_spmm_combine<E, TILED>), grid(blocks), dim3(kBlock), 0, s, p.n_long, p.d_long_row, p.d_long_first, partial,
                       a.Y, a.ldy, a.k);
    SPMV_LAUNCHED("k_spmm_combine");
    return SPMV_OK;
}

// Arguments checked by capi.hip (product_args): ld >= k, X / Y aligned for E, and 1 <= k <= 64 with the plan made or, with
// `cols`, 1 <= k <= SPMV_COLS_MAX_K with the _cols plan covering k.  V = pow2 >= ceil(k / 4), or kColsV per column tile.
template <typename E>
int launch_spmm(const spmv_csr &h, const char *who, bool cols, int k, const E *X, int64_t ldx, E *Y, int64_t ldy, hipStream_t s)
{
    if (h.rows == 0) return SPMV_OK;
    const SpmmArgs<E> a{h.d_vals, X, ldx, Y, ldy, k};
    const bool vec = ldx % 4 == 0 && ldy % 4 == 0;
    if (cols) return vec ? launch_spmm_v<kColsV, true, E, true>(h, who, a, s) : launch_spmm_v<kColsV, false, E, true>(h, who, a, s);
    return dispatch_lanes((k + 3) / 4, [&](auto v) {
        constexpr int V = decltype(v)::value;
        return vec ? launch_spmm_v<V, true, E, false>(h, who, a, s) : launch_spmm_v<V, false, E, false>(h, who, a, s);
    });
}

template int launch_spmm(const spmv_csr &, const char *, bool, int, const float *, int64_t, float *, int64_t, hipStream_t);
template int launch_spmm(const spmv_csr &, const char *, bool, int, const bf16 *, int64_t, bf16 *, int64_t, hipStream_t);
template int launch_spmm(const spmv_csr &, const char *, bool, int, const fp16 *, int64_t, fp16 *, int64_t, hipStream_t);

}  // namespace spmv
