// lane_group.hpp -- the lane groups that SpMM, SDDMM and fused attention walk a CSR pattern with (kernels_spmm.hip,
// kernels_sddmm.hip, kernels_attention.hip): the one statement of the model, of its device code and of the part of the
// order-of-operations contract the three share.  Each kernel file states only what is its own.
//
// The model.  The operands are row-major matrices of k <= 64 columns (attention: k and kv, the wider decides).  A group
// of V = pow2 >= ceil(k / 4) lanes (1, 2, 4, 8 or 16: dispatch_lanes) owns one row of the pattern, or one plan piece of a
// row of more than row_cap = 512 nonzeros (SpmmPlan: the order of the rows, the long rows, their pieces of 512).  Lane s
// of the group holds the slice [4s, 4s+4) of the columns: of the row's own operands in registers, and of every operand
// row the CSR row refers to.  A workgroup is kBlock = 256 lanes, 256 / V groups; the row blocks are dealt so that each of
// the 8 XCDs takes one contiguous range of them (xcd_item64: neighbouring rows share lines of the gathered operand in
// that XCD's L2).  Fused attention's _wide entry points add a sixth group, V = 32, for operands of 65 to 128 columns: see
// "A step narrower than the group" below; SpMM and SDDMM go past 64 columns in tiles of 64 at V = 16 ("Column tiles" below).
// The groups take the rows in the plan's order (stably by length inside blocks of 4096 rows, so the rows a wavefront walks
// side by side end at nearly the same step), except at V = 1: see group_rows.
// Heads (fused attention only).  A launch may carry several heads of one pattern in blockIdx.y and blockIdx.z (the query head
// within its group of heads that share K and V, and the group; kernels_attention.hip); group_row and group_piece keep
// reading blockIdx.x alone (their default `bid`).  Workgroups are dispatched x-fastest, so the blocks of one head that an XCD sees
// are still one residue class of blockIdx.x mod 8, which xcd_item64 still maps to one contiguous range of row blocks: the
// L2 argument above holds head by head (where the grid's x extent is no multiple of 8 the class an XCD takes shifts from
// one head to the next, and stays one class).  This is reasoning from the dispatch order, not a measurement.
// A group walks its row in steps of T = max(V, 8) nonzeros (LaneGeom): lane s loads the step's column indices
// kb + i V + s, i < L = T / V, coalesced (0 past the end), the group broadcasts them with shuffles (group_columns), every
// lane issues all its gathers of the step, one slice per nonzero and operand (load_slice), and only then computes.
// All lanes of a group run every step and every shuffle together: the exits (group_row, group_piece) are group-uniform.
// A step narrower than the group (V = 32: T = kWideStep = 8 < V, L = 1).  T = V would hold 2 x 32 gathered slices of 4
// registers per lane.  Lanes s < T load the step's column indices kb + s and own those nonzeros (what a kernel loads or
// stores per nonzero is theirs); the lanes from T on own none and idle between the butterfly and the broadcast.  The order
// below holds word for word with V = 32: every lane still forms its partial of every dot product of the step, and
// reduce_scatter runs the butterfly's levels m = 16, 8, 4, 2, 1 for each result.
//
// The order of the fp32 operations, as far as it is shared.  No function here holds a product followed by a sum but
// where fmaf is written, so the floating-point contraction of the including file does not reach in.
//   * A sum over a row's nonzeros runs in storage order from +0, one fma per nonzero and column.  A slot of the last step
//     that lies past the end adds nothing: not even +0, which would turn an accumulator of -0 into +0.  Hence the
//     `kb + t < e` around every accumulation of the kernels; the slot's gathers are not issued either.
//   * A dot product over the columns (dot_partial, then the group): lane s forms p_s = +0, p_s = fma(a[c], b[c], p_s) for
//     c = 4s .. 4s+3 while c < k (a column at or past k is skipped, not multiplied by zero; a lane whose slice starts at or
//     past k keeps +0), then the V partials are added in the xor butterfly m = V/2, V/4, .., 1: p_s <- p_s + p_(s xor m).
//   * reduce_scatter runs that butterfly for the V results of a step at once: after the exchange at distance m a lane
//     keeps only the half of the results whose index has the lane's bit m, V - 1 shuffles per V results instead of
//     V log2 V.  Each result still goes through the very additions of the full butterfly, in the same order of levels, and
//     fp32 addition is commutative: the bits are the full butterfly's (group_sum's).
//   * A wider V than ceil(k / 4) asks for (attention with kv > k against SDDMM at k) changes no bit: fma(a, b, +0) is never
//     -0 and neither is a sum of two numbers that are not -0, so a partial is never -0; the extra lanes hold +0 and the
//     extra levels, which run first, add +0 to a number that is not -0.
// So a result is a function of the row's column list in storage order, the operands and k: not of V beyond that, of any
// ld, of the load path, of the row's place, its pieces' neighbours or the handle.
//
// Addresses are 64-bit throughout (an operand may exceed 4 GiB; 4 n passes 2^32 in col_idx from nnz = 2^30 on); no buffer
// descriptor and no range check is relied on.  The ld % 4 rule: where every ld of a call is a multiple of 4 (and the bases
// are 16-byte aligned: the C ABI checks) a slice is one 16-byte access (VEC); the last slice of a k that is no multiple
// of 4 is then read whole, inside its row's ld floats, and stored below k only.  Otherwise the kernels read and store
// 4-byte elements, columns below k only.
// All three also run on 16-bit dense matrices (element type E below; SpMM's vals and SDDMM's out stay float): a slice is then
// 8 bytes, bases are 8-byte aligned, the ld % 4 rule decides between one 8-byte access and 2-byte ones, and nothing of the
// order above changes: an element is widened exactly where it is used and a result is rounded once where it is stored.
#pragma once
#include <type_traits>
#include "spmv_internal.hpp"

namespace spmv {

// The step of a group of 32 lanes (fused attention at 64 < max(k, kv) <= 128, the _wide entry points only): T_wide of
// include/spmv_hip.h.  T = V = 32 would keep 2 x 32 gathered slices of 4 registers each per lane, the whole register file;
// 8 nonzeros per step keep 64, the register picture of V = 8.  Such a step is narrower than its group (T < V): lanes
// sub < T each own one nonzero of the step (its column index, its bias, its stats and delta, its expf, its dBias), the other
// lanes of the group own none.  The forward pass's bits depend on T (one rescale per step); nothing else does.
constexpr int kWideStep = 8;

template <int V>
struct LaneGeom {
    static constexpr int T = V > 16 ? kWideStep : V > 8 ? V : 8;   // nonzeros per step: T slice gathers in flight per lane and operand
    static constexpr int L = T >= V ? T / V : 1;   // of which a lane loads the column indices of L and ends with L results
                                                   // (T < V: one, and only in the lanes sub < T)
    // whether lane `sub` owns a nonzero in its slot i < L of a step at all (always, unless the step is narrower than the group)
    static constexpr bool owner(int sub) { return T >= V || sub < T; }
};
static_assert(LaneGeom<32>::T == 8 && LaneGeom<32>::L == 1 && LaneGeom<16>::T == 16 && LaneGeom<4>::L == 2, "the geometry of the header");

// block b of the grid takes item xcd_item64(b, n): blocks are dealt round-robin over the 8 XCDs, so each XCD gets one
// contiguous range of the n row blocks
__device__ __forceinline__ int64_t xcd_item64(int64_t bid, int64_t n)
{
    const int64_t q = n / kXcds, rem = n % kXcds;
    const int64_t j = bid % kXcds, idx = bid / kXcds;
    return j * q + (j < rem ? j : rem) + idx;
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// ---- the element type E of a dense matrix: float, or 16-bit storage (bf16, fp16 of attention_args.hpp) -------------------
// A 16-bit element is widened exactly to fp32 where it is used and an fp32 result is rounded to E once, to nearest even, where
// it is stored; nothing in between is 16-bit.  Neither direction flushes a subnormal; a NaN stays a NaN (payload unspecified).
// bf16 is plain integer code; fp16 is the compiler's _Float16 conversions (the host compiles both).
template <typename E>
constexpr bool kIs16 = !std::is_same<E, float>::value;

// four 16-bit elements as loaded, 8 bytes: columns c0 and c0 + 1 in lo (the first in the low half), c0 + 2 and c0 + 3 in hi
struct alignas(8) Packed4 {
    uint32_t lo, hi;
};

// a lane's slice as it waits in registers between its load and its use: float4, or the 8 bytes of 16-bit elements
template <typename E>
using slice_t = std::conditional_t<kIs16<E>, Packed4, float4>;

template <typename E>
__device__ __forceinline__ slice_t<E> zero_slice()
{
    if constexpr (kIs16<E>) return Packed4{0u, 0u};
    else return zero4();
}

template <typename E>
__device__ __forceinline__ float widen16(uint32_t h)      // h < 2^16: the bits of one element
{
    if constexpr (std::is_same<E, bf16>::value) {
        const uint32_t u = h << 16;
        float f;
        __builtin_memcpy(&f, &u, 4);
        return f;
    } else {
        const uint16_t b = (uint16_t)h;
        fp16 x;
        __builtin_memcpy(&x, &b, 2);
        return (float)x;
    }
}

// fp32 to the bits of E, round to nearest even (bf16: a NaN keeps its sign and gets the quiet bit; fp16 overflows to Inf)
template <typename E>
__device__ __forceinline__ uint32_t round16(float f)
{
    if constexpr (std::is_same<E, bf16>::value) {
        uint32_t u;
        __builtin_memcpy(&u, &f, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        // f is an fp32 number before it is converted: where it is a product (O = acc * r) the compiler would otherwise fold the
        // multiplication into a mixed-precision fma that rounds the exact product to fp16 once, another number in rare cases
        asm("" : "+v"(f));
#endif
        const fp16 x = (fp16)f;
        uint16_t b;
        __builtin_memcpy(&b, &x, 2);
        return b;
    }
}

// the slice as four floats (float: as it is)
template <typename E>
__device__ __forceinline__ float4 widen(slice_t<E> s)
{
    if constexpr (kIs16<E>)
        return make_float4(widen16<E>(s.lo & 0xffffu), widen16<E>(s.lo >> 16), widen16<E>(s.hi & 0xffffu), widen16<E>(s.hi >> 16));
    else return s;
}

template <typename E>
__device__ __forceinline__ const uint16_t *bits16(const E *p) { return reinterpret_cast<const uint16_t *>(p); }
template <typename E>
__device__ __forceinline__ uint16_t *bits16(E *p) { return reinterpret_cast<uint16_t *>(p); }

// the four columns [c0, c0+4) of row j of a row-major matrix (c0 < w); VEC: one 16-byte load (16-bit elements: one 8-byte
// load), else the columns below w only, element by element
template <bool VEC, typename E>
__device__ __forceinline__ slice_t<E> load_slice(const E *__restrict__ M, int64_t ld, int64_t j, int c0, int w)
{
    const E *p = M + j * ld + c0;
    if constexpr (kIs16<E>) {
        if (VEC) return *reinterpret_cast<const Packed4 *>(p);
        const uint16_t *h = bits16(p);
        Packed4 r{h[0], 0u};
        if (c0 + 1 < w) r.lo |= (uint32_t)h[1] << 16;
        if (c0 + 2 < w) r.hi = h[2];
        if (c0 + 3 < w) r.hi |= (uint32_t)h[3] << 16;
        return r;
    } else {
        if (VEC) return *reinterpret_cast<const float4 *>(p);
        float4 r = zero4();
        r.x = p[0];
        if (c0 + 1 < w) r.y = p[1];
        if (c0 + 2 < w) r.z = p[2];
        if (c0 + 3 < w) r.w = p[3];
        return r;
    }
}

// the same, widened: a row's own operand, which stays in registers as floats for the whole row
template <bool VEC, typename E>
__device__ __forceinline__ float4 load_wide(const E *__restrict__ M, int64_t ld, int64_t j, int c0, int w)
{
    return widen<E>(load_slice<VEC>(M, ld, j, c0, w));
}

// widen for a slice's second use in a step: the compiler must not keep the first use's four floats alive in between (they
// would undo the packing: 4 registers per slice instead of 2), so the packed words pass through an empty statement
template <typename E>
__device__ __forceinline__ float4 widen_again(slice_t<E> s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (kIs16<E>) {
        asm("" : "+v"(s.lo));
        asm("" : "+v"(s.hi));
    }
#endif
    return widen<E>(s);
}

// the columns [c0, c0+4) below w of one output row (c0 < w; vector stores only); 16-bit elements are rounded here
template <bool VEC, typename E>
__device__ __forceinline__ void store_slice(E *__restrict__ p, float4 a, int c0, int w)
{
    if constexpr (kIs16<E>) {
        const uint32_t x = round16<E>(a.x), y = round16<E>(a.y), z = round16<E>(a.z), v = round16<E>(a.w);
        if (VEC && c0 + 4 <= w) {
            *reinterpret_cast<Packed4 *>(p) = Packed4{x | (y << 16), z | (v << 16)};
            return;
        }
        uint16_t *h = bits16(p);
        h[0] = (uint16_t)x;
        if (c0 + 1 < w) h[1] = (uint16_t)y;
        if (c0 + 2 < w) h[2] = (uint16_t)z;
        if (c0 + 3 < w) h[3] = (uint16_t)v;
    } else {
        if (VEC && c0 + 4 <= w) {
            *reinterpret_cast<float4 *>(p) = a;
            return;
        }
        p[0] = a.x;
        if (c0 + 1 < w) p[1] = a.y;
        if (c0 + 2 < w) p[2] = a.z;
        if (c0 + 3 < w) p[3] = a.w;
    }
}

// the lane's partial of a dot product: fma over its n1 = w - c0 columns (at most 4) from +0; +0 for an idle lane
__device__ __forceinline__ float dot_partial(float4 u, float4 x, int n1)
{
    float a = 0.0f;
    if (n1 > 0) {
        a = fmaf(u.x, x.x, a);
        if (n1 > 1) a = fmaf(u.y, x.y, a);
        if (n1 > 2) a = fmaf(u.z, x.z, a);
        if (n1 > 3) a = fmaf(u.w, x.w, a);
    }
    return a;
}

// the xor butterfly over the group as a reduce-scatter: of results i*V + [0, V) lane `sub` ends with result i*V + sub in
// p[i*V].
// A step narrower than the group (T < V; gbase: the group's first lane in the wavefront, which only this case reads): the
// levels m = V/2 .. V/T each halve the results a lane still holds (the lane with bit m keeps the upper half), which leaves one;
// the levels below are the all-reduce of that one, p <- p + p_(sub xor m).  Every result has then gone through the additions of
// group_sum<V> in its order of levels, m = V/2, .., 1.  Result t sits in the V/T lanes t V/T + [0, V/T); one more shuffle
// hands it to its owner, lane t < T, in p[0].
template <int V, int T>
__device__ __forceinline__ void reduce_scatter(float (&p)[T], int sub, [[maybe_unused]] int gbase = 0)
{
    if constexpr (T < V) {
        constexpr int W = V / T;        // lanes that end up with the same result
#pragma unroll
        for (int m = V / 2, n = T / 2; n >= 1; m /= 2, n /= 2) {
            const bool up = (sub & m) != 0;
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const float lo = p[j], hi = p[j + n];
                const float keep = up ? hi : lo, send = up ? lo : hi;
                p[j] = keep + __shfl_xor(send, m);
            }
        }
#pragma unroll
        for (int m = W / 2; m >= 1; m /= 2) p[0] = p[0] + __shfl_xor(p[0], m);
        p[0] = __shfl(p[0], gbase + (sub & (T - 1)) * W);
        return;
    }
#pragma unroll
    for (int i = 0; i < T / V; ++i) {
#pragma unroll
        for (int m = V / 2; m >= 1; m /= 2) {
            const bool up = (sub & m) != 0;
#pragma unroll
            for (int j = 0; j < m; ++j) {
                const float lo = p[i * V + j], hi = p[i * V + j + m];
                const float keep = up ? hi : lo, send = up ? lo : hi;
                p[i * V + j] = keep + __shfl_xor(send, m);
            }
        }
    }
}

// what lane `sub` holds for nonzero i*V + sub of the step, in every lane of the group (T < V: lane t < T holds nonzero t's)
template <int V, int T, typename X>
__device__ __forceinline__ void group_bcast(const X (&w)[LaneGeom<V>::L], X (&wt)[T], int gbase)
{
    static_assert(T == LaneGeom<V>::T, "a step of the geometry");
#pragma unroll
    for (int t = 0; t < T; ++t) wt[t] = V == 1 ? w[t] : __shfl(w[t / V], gbase + t % V);
}

template <int V>
__device__ __forceinline__ float group_max(float x)
{
#pragma unroll
    for (int m = V / 2; m >= 1; m /= 2) x = fmaxf(x, __shfl_xor(x, m));
    return x;
}

template <int V>
__device__ __forceinline__ float group_sum(float x)
{
#pragma unroll
    for (int m = V / 2; m >= 1; m /= 2) x = x + __shfl_xor(x, m);
    return x;
}

// the step's column indices: lane `sub` loads nonzeros kb + i*V + sub (0 past the end e; T < V: the lanes sub < T one each,
// the others none), every lane gets all T
template <int V, int T>
__device__ __forceinline__ void group_columns(int64_t kb, int64_t e, int sub, int gbase, const int32_t *__restrict__ col_idx,
                                              int32_t (&c)[LaneGeom<V>::L], int32_t (&ct)[T])
{
#pragma unroll
    for (int i = 0; i < LaneGeom<V>::L; ++i) {
        const int64_t n = kb + (int64_t)i * V + sub;
        c[i] = LaneGeom<V>::owner(sub) && n < e ? col_idx[n] : 0;
    }
    group_bcast<V, T>(c, ct, gbase);
}

// the rows and the pieces of a launch (kernel arguments, by value)
struct GroupRows {
    int64_t rows, nblocks;
    int row_cap;
    const int32_t *order, *row_ptr, *col_idx;
};
struct GroupPieces {
    int npieces, n_long;
    const int32_t *long_row, *long_first, *piece_k0, *piece_len, *col_idx;
    float *scratch;     // the caller's floats per piece
};

// Column tiles (the _cols calls of SpMM and SDDMM only).  A call at any width k runs as m = cols_tiles(k) tiles of
// kColsTile = 64 columns, tile t the columns [64t, 64t + k_t) with k_t = min(64, k - 64t): each tile is the model above at
// V = 16 on operands advanced by 64t elements (which keeps the 16-byte / 8-byte path wherever the lds allow it).  SpMM
// carries the tile in the grid, so blockIdx.x alone no longer names the row block there: its TILED kernels hand `bid`, the
// index of the row block (of the block of pieces), to the two functions below.  SDDMM walks the tiles inside a step.
constexpr int kColsTile = 64;
constexpr int kColsV = 16;          // the lane group of every tile (kColsTile / 4 lanes)
__host__ __device__ constexpr int cols_tiles(int k) { return (k + kColsTile - 1) / kColsTile; }

// the row of slot `threadIdx.x / V` of row block `bid`, or -1 (group-uniform: a group never splits here)
template <int V>
__device__ __forceinline__ int64_t group_row(const GroupRows &g, int64_t bid = blockIdx.x)
{
    const int64_t slot = xcd_item64(bid, g.nblocks) * (kBlock / V) + threadIdx.x / V;
    if (slot >= g.rows) return -1;
    return g.order ? g.order[slot] : slot;
}

// the piece of the group in block `bid` of the pieces, or -1 (group-uniform)
template <int V>
__device__ __forceinline__ int64_t group_piece(const GroupPieces &g, int64_t bid = blockIdx.x)
{
    const int64_t p = bid * (kBlock / V) + threadIdx.x / V;
    return p < g.npieces ? p : -1;
}

// the same (of block blockIdx.x) and the index of its long row: long_first[lo] <= p < long_first[lo + 1]  (long_first[0] = 0,
// long_first[n_long] = npieces)
template <int V>
__device__ __forceinline__ int64_t group_piece(const GroupPieces &g, int &lo)
{
    const int64_t p = group_piece<V>(g);
    if (p < 0) return -1;
    int hi = g.n_long;
    lo = 0;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (g.long_first[mid] <= p) lo = mid;
        else hi = mid;
    }
    return p;
}

// ---- host side --------------------------------------------------------------------------------------------------------
// calls f(std::integral_constant<int, V>) for the V of `slices` = ceil(k / 4) slices, k <= 64
template <typename F>
int dispatch_lanes(int slices, F &&f)
{
    if (slices <= 1) return f(std::integral_constant<int, 1>{});
    if (slices <= 2) return f(std::integral_constant<int, 2>{});
    if (slices <= 4) return f(std::integral_constant<int, 4>{});
    if (slices <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

// a grid of kBlock lanes for `groups` groups of V lanes
inline dim3 group_grid(int64_t groups, int V)
{
    const int per = kBlock / V;
    return dim3((unsigned)((groups + per - 1) / per));
}

// the row blocks of a launch over the rows of h, or -1 and `who`'s error.  (A launch carries fewer than 2^32 work-items --
// the runtime passes grid x block on in 32 bits and a larger product wraps silently: rows x lanes per row < 2^32 -- any
// handle up to k = 8, rows < 2^30 / 2^29 / 2^28 up to k = 16 / 32 / 64.)
inline int64_t group_row_blocks(const char *who, const spmv_csr &h, int V)
{
    const int per = kBlock / V;
    const int64_t nblocks = (h.rows + per - 1) / per;
    if (nblocks * kBlock >= (1LL << 32)) {
        set_error("%s: %lld rows x %d lanes per row reach the launch limit of 2^32 work-items", who, (long long)h.rows, V);
        return -1;
    }
    return nblocks;
}

// the heads one launch over h's pattern may carry (blockIdx.y): no grid of the call -- row blocks, or the blocks of the long
// rows' pieces where those are more -- may reach 2^32 work-items over all heads, and a grid's y extent ends at kMaxHeads.
// 0: not even one head fits.
inline int64_t group_max_heads(const spmv_csr &h, int V)
{
    const int per = kBlock / V;
    const int64_t nblocks = (h.rows + per - 1) / per, pblocks = ((int64_t)h.plan_spmm.pieces + per - 1) / per;
    const int64_t blocks = nblocks > pblocks ? nblocks : pblocks;
    const int64_t fit = blocks ? ((1LL << 32) - 1) / (blocks * kBlock) : kMaxHeads;
    return fit < kMaxHeads ? fit : kMaxHeads;
}

// group_row_blocks for a launch of `heads` heads, or -1 and `who`'s error
inline int64_t group_head_blocks(const char *who, const spmv_csr &h, int V, int heads)
{
    const int64_t nblocks = group_row_blocks(who, h, V);
    if (nblocks < 0) return -1;
    if (heads > kMaxHeads) {
        set_error("%s: %d heads exceed the launch limit of %d heads (the grid's y extent)", who, heads, kMaxHeads);
        return -1;
    }
    if (heads > group_max_heads(h, V)) {
        set_error("%s: %lld rows (%d pieces of long rows) x %d lanes per row x %d heads reach the launch limit of 2^32 work-items",
                  who, (long long)h.rows, h.plan_spmm.pieces, V, heads);
        return -1;
    }
    return nblocks;
}

// group_row_blocks for a launch that carries `tiles` column tiles in its grid (SpMM's _cols call), or -1 and `who`'s error:
// like the heads, no grid of the call may reach 2^32 work-items over all tiles, nor its y extent pass kMaxHeads
inline int64_t group_tile_blocks(const char *who, const spmv_csr &h, int V, int tiles)
{
    const int64_t nblocks = group_row_blocks(who, h, V);
    if (nblocks < 0) return -1;
    if (tiles > group_max_heads(h, V)) {
        set_error("%s: %lld rows (%d pieces of long rows) x %d lanes per row x %d column tiles reach the launch limit of 2^32 work-items",
                  who, (long long)h.rows, h.plan_spmm.pieces, V, tiles);
        return -1;
    }
    return nblocks;
}

// V = 1 (k <= 4) keeps the row order: there each lane streams its own row's col_idx (and vals), and neighbouring rows keep
// those loads on neighbouring lines (measured on SpMM: 2x faster at k = 1 and 4 on configs 3 and 4; from V = 2 on the
// plan's sorted order wins, up to 2.5x)
inline GroupRows group_rows(const spmv_csr &h, int V, int64_t nblocks)
{
    const SpmmPlan &p = h.plan_spmm;
    return GroupRows{h.rows, nblocks, p.row_cap, V == 1 ? nullptr : p.d_order.get(), h.d_row_ptr, h.d_col_idx};
}

inline GroupPieces group_pieces(const spmv_csr &h, float *scratch)
{
    const SpmmPlan &p = h.plan_spmm;
    return GroupPieces{p.pieces, p.n_long, p.d_long_row.get(), p.d_long_first.get(), p.d_piece_k0.get(), p.d_piece_len.get(),
                       h.d_col_idx, scratch};
}

}  // namespace spmv
