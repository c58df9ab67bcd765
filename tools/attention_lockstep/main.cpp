// tools/attention_lockstep/main.cpp -- see run.sh.  One pattern whose rows (and whose transposed rows) cover empty rows, rows
// inside one step, several steps, exactly 512, pieces of long rows; a third of the rows unsorted and a fifth drawn with
// replacement, so keys repeat inside rows and queries inside transposed rows; the three passes at four (k, kv) on the 16-byte and the
// 4-byte load path, every array an exactly sized heap block, compared with a serial fp64 statement of attention.  SDDMM
// at the same four k on the pattern and on its transpose, every out[n] compared bit for bit with a serial statement of
// the documented order.  Then three heads in one launch (launch_attention at heads = 3, the head in blockIdx.z) at the same
// (k, kv) and load paths, as stacked operands with a padded head stride and as column blocks of one wide matrix, the scratch
// sized for exactly three heads: every head bit for bit the program's own single-head run on that head's data.  Then grouped-
// query heads (launch_attention at group = 2): four query heads on two K/V heads, the three passes on both load paths at a V below 16
// and at V = 16 (where k_attn_bwd_kv_rows_gqa parks its sums in LDS), the scratch sized for exactly four heads: O, stats,
// delta and dQ bit for bit the single-head runs on K, V of head y / 2, dK and dV bit for bit those runs' results added in
// head order from the first head's value.  Then the same four heads on two K/V heads on 16-bit matrices (bf16 and fp16; (6, 10)
// and (40, 64); both load paths): every array an exactly sized heap block of 2-byte elements, O, dQ, dK and dV bit for bit the
// program's own fp32 _gqa runs on the widened data, rounded to nearest even by a conversion written here, stats and delta those
// runs' bits.  Then the additive bias (the <..., AttnBias> kernels through launch_attention with an AttnBias): the same four heads on two
// K/V heads at (6, 10) and (40, 64) on both load paths, fp32 and bf16 matrices, a bias per query head and nonzero, bias, bias_t
// (the bias in the transposed pattern's order) and dBias exactly sized heap blocks of floats with head strides that are
// multiples of nothing, rows and transposed rows in pieces: O, dQ, dBias, dK and dV against a serial fp64 attention with bias
// written here (fp32: 2e-5 of the magnitude; bf16: 2^-7 more: half an ulp, 2^-8, for the rounded output and as much for the delta
// formed from the rounded O), and every position of dBias written.  Then V = 32 (the kernels of the _wide entry points): the
// same bias runs at (128, 128) and (65, 100) on the wide scratch (260 floats per piece, exactly sized), with a bias and
// without one (the unbiased kernels), and zero padding: (64, 20), (8, 40) and (16, 12) padded to (128, 128) give the narrow
// geometry's delta, dBias, dQ, dK and dV bit for bit on its stats and delta, and +0 in every padded column.
#include "kernels_attention.hip"
#include "kernels_sddmm.hip"
#include <algorithm>
#include <cstdlib>
#include <random>
using namespace spmv;

template <class T> static T *heap(const std::vector<T> &v)
{
    T *p = (T *)malloc(sizeof(T) * v.size() + 1);
    std::copy(v.begin(), v.end(), p);
    return p;
}

struct Pattern {
    int64_t rows, cols;
    std::vector<int32_t> rp, ci;
};

// the handle of a pattern with the plan of plan_spmm: rows of more than 512 in pieces of 512, the rows in row order
static spmv_csr make_handle(const Pattern &a, std::vector<void *> &owned)
{
    std::vector<int32_t> lr, lf, k0, ln, order((size_t)a.rows);
    for (int64_t r = 0; r < a.rows; ++r) {
        order[(size_t)r] = (int32_t)(a.rows - 1 - r);      // (any permutation serves)
        if (a.rp[r + 1] - a.rp[r] <= 512) continue;
        lr.push_back((int32_t)r);
        lf.push_back((int32_t)k0.size());
        for (int q = a.rp[r]; q < a.rp[r + 1]; q += 512) { k0.push_back(q); ln.push_back(std::min(512, a.rp[r + 1] - q)); }
    }
    lf.push_back((int32_t)k0.size());
    spmv_csr h;
    h.rows = a.rows, h.cols = a.cols, h.nnz = a.rp[a.rows];
    int32_t *rp = heap(a.rp), *ci = heap(a.ci);
    h.d_row_ptr = rp, h.d_col_idx = ci;
    SpmmPlan &pl = h.plan_spmm;
    pl.n_long = (int)lr.size(), pl.pieces = (int)k0.size();
    pl.d_order.p = heap(order), pl.d_long_row.p = heap(lr), pl.d_long_first.p = heap(lf), pl.d_piece_k0.p = heap(k0), pl.d_piece_len.p = heap(ln);
    if (plan_attention(h, nullptr) != SPMV_OK) abort();
    for (void *p : {(void *)rp, (void *)ci, (void *)pl.d_order.p, (void *)pl.d_long_row.p, (void *)pl.d_long_first.p, (void *)pl.d_piece_k0.p,
                    (void *)pl.d_piece_len.p})
        owned.push_back(p);       // (the scratch is the plan's: main frees it at the end)
    return h;
}

// the scratch of h for exactly `heads` heads (the stub's DevPtr frees the block it replaces)
static void plan_heads(spmv_csr &h, int heads)
{
    free(h.plan_attn.d_scratch.p);
    free(h.plan_attn.d_scratch_wide.p);
    h.plan_attn = AttnPlan{};
    if (plan_attention_heads(h, heads, nullptr) != SPMV_OK || h.plan_attn.heads != heads) abort();
}

// the same and the wide scratch (V = 32) for exactly `heads` heads: an exactly sized block of heads x pieces x 260 floats
static void plan_wide(spmv_csr &h, int heads)
{
    plan_heads(h, heads);
    if (plan_attention_wide(h, heads, nullptr) != SPMV_OK || h.plan_attn.wide_heads != heads) abort();
}

// `heads` heads of rows x w floats: head y at p + y * stride, its rows ld apart; one exactly sized block that ends where the
// last row of the last head does (at its width; on the 16-byte path at the end of its last slice)
struct HeadsMatrix {
    float *p;
    int64_t ld, stride;
};

static HeadsMatrix heads_matrix(int heads, int64_t rows, int w, int64_t ld, int64_t stride, bool vec)
{
    const size_t n = (size_t)((heads - 1) * stride + (rows - 1) * ld + (vec ? (w + 3) / 4 * 4 : w));
    float *p = (float *)malloc(4 * n);       // (16-byte aligned, and exact: the sanitizer sees the first byte past it)
    for (size_t i = 0; i < n; ++i) p[i] = NAN;
    return HeadsMatrix{p, ld, stride};
}

static void put_head(const HeadsMatrix &m, int y, const float *src, int64_t src_ld, int64_t rows, int w)
{
    for (int64_t r = 0; r < rows; ++r) std::memcpy(m.p + y * m.stride + r * m.ld, src + r * src_ld, 4 * (size_t)w);
}

// The three passes through launch_attention, AttnArgs filled by name.  Every operand is a HeadsMatrix: a call of one head
// passes {p, ld, 0}, a vector (stats, delta) {p, 0, its head stride}.
static AttnArgs attn_inputs(float scale, int k, int kv, const HeadsMatrix &Q, const HeadsMatrix &K, const HeadsMatrix &V)
{
    AttnArgs a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = Q.p, a.ldq = Q.ld, a.hq = Q.stride, a.K = K.p, a.ldk = K.ld, a.hk = K.stride, a.V = V.p, a.ldv = V.ld, a.hv = V.stride;
    return a;
}

static int forward(const spmv_csr &A, int heads, int group, float scale, int k, int kv, const HeadsMatrix &Q, const HeadsMatrix &K,
                   const HeadsMatrix &V, const HeadsMatrix &O, const HeadsMatrix &stats)
{
    AttnArgs a = attn_inputs(scale, k, kv, Q, K, V);
    a.out0 = O.p, a.ld0 = O.ld, a.h0 = O.stride, a.stats = stats.p, a.hstats = stats.stride;
    return launch_attention(kPassForward, A, a, nullptr, heads, group, false, "forward", nullptr);
}

static int backward_q(const spmv_csr &A, int heads, int group, float scale, int k, int kv, const HeadsMatrix &Q, const HeadsMatrix &K,
                      const HeadsMatrix &V, const HeadsMatrix &O, const HeadsMatrix &dO, const HeadsMatrix &stats,
                      const HeadsMatrix &delta, const HeadsMatrix &dQ)
{
    AttnArgs a = attn_inputs(scale, k, kv, Q, K, V);
    a.O = O.p, a.ldo = O.ld, a.ho = O.stride, a.dO = dO.p, a.lddo = dO.ld, a.hdo = dO.stride;
    a.stats_in = stats.p, a.hstats_in = stats.stride, a.delta = delta.p, a.hdelta = delta.stride;
    a.out0 = dQ.p, a.ld0 = dQ.ld, a.h0 = dQ.stride;
    return launch_attention(kPassBackwardQ, A, a, nullptr, heads, group, false, "backward_q", nullptr);
}

// sum_group: the _gqa call's kernels, which add the heads of a group
static int backward_kv(const spmv_csr &T, int heads, int group, bool sum_group, float scale, int k, int kv, const HeadsMatrix &Q,
                       const HeadsMatrix &K, const HeadsMatrix &V, const HeadsMatrix &dO, const HeadsMatrix &stats,
                       const HeadsMatrix &delta, const HeadsMatrix &dK, const HeadsMatrix &dV)
{
    AttnArgs a = attn_inputs(scale, k, kv, Q, K, V);
    a.dO = dO.p, a.lddo = dO.ld, a.hdo = dO.stride;
    a.stats_in = stats.p, a.hstats_in = stats.stride, a.delta_in = delta.p, a.hdelta_in = delta.stride;
    a.out0 = dK.p, a.ld0 = dK.ld, a.h0 = dK.stride, a.out1 = dV.p, a.ld1 = dV.ld, a.h1 = dV.stride;
    return launch_attention(kPassBackwardKV, T, a, nullptr, heads, group, sum_group, "backward_kv", nullptr);
}

// how many of head y's rows x w floats differ in a bit from the single-head result
static long head_differs(const HeadsMatrix &m, int y, const float *ref, int64_t ref_ld, int64_t rows, int w)
{
    long bad = 0;
    for (int64_t r = 0; r < rows; ++r) bad += std::memcmp(m.p + y * m.stride + r * m.ld, ref + r * ref_ld, 4 * (size_t)w) != 0;
    return bad;
}

static Pattern transpose(const Pattern &a)
{
    Pattern t{a.cols, a.rows, std::vector<int32_t>((size_t)a.cols + 1, 0), std::vector<int32_t>(a.ci.size())};
    for (int32_t c : a.ci) ++t.rp[(size_t)c + 1];
    for (int64_t j = 0; j < a.cols; ++j) t.rp[j + 1] += t.rp[j];
    std::vector<int32_t> at(t.rp.begin(), t.rp.end() - 1);
    for (int64_t r = 0; r < a.rows; ++r)
        for (int n = a.rp[r]; n < a.rp[r + 1]; ++n) t.ci[(size_t)at[a.ci[n]]++] = (int32_t)r;
    return t;
}

// rows x w floats of leading dimension ld in an exactly sized block (the last row ends at its width)
static float *matrix(int64_t rows, int w, int64_t ld, std::mt19937 &rng, bool fill)
{
    const size_t n = rows ? (size_t)((rows - 1) * ld + (ld % 4 == 0 ? (w + 3) / 4 * 4 : w)) : 0;
    float *p = (float *)aligned_alloc(16, (n * 4 + 15) / 16 * 16 + 16);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (size_t i = 0; i < n; ++i) p[i] = fill ? nd(rng) : NAN;
    return p;
}

// SDDMM's documented order, serially: the lane partials by fmaf from +0 over the columns below k, then the pairwise tree
// the xor butterfly spells
static float sddmm_serial(const float *u, const float *x, int k, int V)
{
    float p[16], q[16];
    for (int s = 0; s < V; ++s) {
        p[s] = 0.0f;
        for (int c = 4 * s; c < 4 * s + 4 && c < k; ++c) p[s] = fmaf(u[c], x[c], p[s]);
    }
    for (int m = V / 2; m >= 1; m /= 2) {
        for (int s = 0; s < V; ++s) q[s] = p[s] + p[s ^ m];
        std::copy(q, q + V, p);
    }
    return p[0];
}

// launch_sddmm on the handle h of pattern a into an exactly sized block: how many out[n] differ from the serial statement
// in any bit (-1: the launch failed)
static long sddmm_differing(const spmv_csr &h, const Pattern &a, int k, const float *U, int64_t ldu, const float *X, int64_t ldx)
{
    int V = 1;
    while (4 * V < k) V *= 2;
    g_group_lanes = V;
    std::vector<float> nan((size_t)h.nnz, NAN);
    float *out = heap(nan);
    long bad = launch_sddmm(h, k, U, ldu, X, ldx, out, nullptr) == SPMV_OK ? 0 : -1;
    for (int64_t r = 0; bad >= 0 && r < a.rows; ++r)
        for (int n = a.rp[r]; n < a.rp[r + 1]; ++n) {
            const float want = sddmm_serial(U + r * ldu, X + a.ci[n] * ldx, k, V);
            bad += std::memcmp(&want, out + n, 4) != 0;
        }
    free(out);
    return bad;
}

// Three heads in one launch against three single-head runs, at the four (k, kv) on both load paths, stacked and as column
// blocks.  The single-head runs come first, on a scratch of one head; then the plans grow to exactly three.
static int heads_runs(spmv_csr &A, spmv_csr &T, const Pattern &a, float scale, std::mt19937 &rng)
{
    constexpr int H = 3;
    const int shapes[][2] = {{24, 24}, {8, 40}, {64, 4}, {6, 10}};
    const int64_t R = a.rows, C = a.cols;
    int status = 0;
    for (auto &kk : shapes)
        for (int odd = 0; odd < 2; ++odd) {
            const int k = kk[0], kv = kk[1];
            int V = 1;
            while (4 * V < std::max(k, kv)) V *= 2;
            g_group_lanes = V;
            auto ld = [&](int w) { return (int64_t)(odd ? w + 1 + ((w + 1) % 4 == 0) : (w + 3) / 4 * 4 + 4); };
            const int64_t lk = ld(k), lv = ld(kv);
            // the single-head runs, every head on arrays of its own
            float *Q[H], *K[H], *Vm[H], *dO[H], *O[H], *dQ[H], *dK[H], *dV[H], *stats[H], *delta[H];
            plan_heads(A, 1);
            plan_heads(T, 1);
            for (int y = 0; y < H; ++y) {
                Q[y] = matrix(R, k, lk, rng, true), K[y] = matrix(C, k, lk, rng, true), Vm[y] = matrix(C, kv, lv, rng, true);
                dO[y] = matrix(R, kv, lv, rng, true), O[y] = matrix(R, kv, lv, rng, false), dQ[y] = matrix(R, k, lk, rng, false);
                dK[y] = matrix(C, k, lk, rng, false), dV[y] = matrix(C, kv, lv, rng, false);
                stats[y] = (float *)malloc(8 * R), delta[y] = (float *)malloc(4 * R);
                const HeadsMatrix q{Q[y], lk, 0}, kj{K[y], lk, 0}, vj{Vm[y], lv, 0}, o{O[y], lv, 0}, g{dO[y], lv, 0};
                const HeadsMatrix ms{stats[y], 0, 0}, md{delta[y], 0, 0};
                status |= forward(A, 1, 1, scale, k, kv, q, kj, vj, o, ms);
                status |= backward_q(A, 1, 1, scale, k, kv, q, kj, vj, o, g, ms, md, {dQ[y], lk, 0});
                status |= backward_kv(T, 1, 1, false, scale, k, kv, q, kj, vj, g, ms, md, {dK[y], lk, 0}, {dV[y], lv, 0});
            }
            plan_heads(A, H);
            plan_heads(T, H);
            for (int blocks = 0; blocks < 2; ++blocks) {
                // stacked: rows ld apart as above, heads a padded multiple of 4 floats apart; column blocks: head y at
                // columns [y s, y s + w) of rows that hold all heads, s = w rounded up to 4
                auto make = [&](int64_t rows, int w) {
                    const int64_t s4 = (w + 3) / 4 * 4;
                    if (blocks) return heads_matrix(H, rows, w, H * s4 + odd, s4, !odd);
                    return heads_matrix(H, rows, w, ld(w), (rows * ld(w) + 3) / 4 * 4 + 8, !odd);
                };
                HeadsMatrix hQ = make(R, k), hK = make(C, k), hV = make(C, kv), hdO = make(R, kv), hO = make(R, kv), hdQ = make(R, k),
                            hdK = make(C, k), hdV = make(C, kv);
                const int64_t sstats = 2 * R + 2 * blocks, sdelta = R + 3 * blocks;
                float *hstats = (float *)malloc(4 * (size_t)((H - 1) * sstats + 2 * R)), *hdelta = (float *)malloc(4 * (size_t)((H - 1) * sdelta + R));
                for (int y = 0; y < H; ++y) {
                    put_head(hQ, y, Q[y], lk, R, k), put_head(hK, y, K[y], lk, C, k), put_head(hV, y, Vm[y], lv, C, kv);
                    put_head(hdO, y, dO[y], lv, R, kv);
                }
                const HeadsMatrix ms{hstats, 0, sstats}, md{hdelta, 0, sdelta};
                status |= forward(A, H, 1, scale, k, kv, hQ, hK, hV, hO, ms);
                status |= backward_q(A, H, 1, scale, k, kv, hQ, hK, hV, hO, hdO, ms, md, hdQ);
                status |= backward_kv(T, H, 1, false, scale, k, kv, hQ, hK, hV, hdO, ms, md, hdK, hdV);
                long bad = 0;
                for (int y = 0; y < H; ++y) {
                    bad += head_differs(hO, y, O[y], lv, R, kv) + head_differs(hdQ, y, dQ[y], lk, R, k);
                    bad += head_differs(hdK, y, dK[y], lk, C, k) + head_differs(hdV, y, dV[y], lv, C, kv);
                    bad += std::memcmp(hstats + y * sstats, stats[y], 8 * (size_t)R) != 0;
                    bad += std::memcmp(hdelta + y * sdelta, delta[y], 4 * (size_t)R) != 0;
                }
                printf("heads %d k %d kv %d V %d %s, %s: status %d, %ld rows differ in a bit from the single-head runs\n", H, k, kv, V,
                       odd ? "4-byte path" : "16-byte path", blocks ? "column blocks" : "stacked", status, bad);
                if (bad) status |= 64;
                for (void *p : {(void *)hQ.p, (void *)hK.p, (void *)hV.p, (void *)hdO.p, (void *)hO.p, (void *)hdQ.p, (void *)hdK.p, (void *)hdV.p,
                                (void *)hstats, (void *)hdelta})
                    free(p);
            }
            for (int y = 0; y < H; ++y)
                for (void *p : {(void *)Q[y], (void *)K[y], (void *)Vm[y], (void *)dO[y], (void *)O[y], (void *)dQ[y], (void *)dK[y], (void *)dV[y],
                                (void *)stats[y], (void *)delta[y]})
                    free(p);
        }
    return status;
}

// Four query heads on two K/V heads in one _gqa call per pass against the program's own single-head runs: head y on K, V of
// head y / G; dK, dV of K/V head c = the runs' results of heads c G .. c G + G - 1 added in that order from the first one's.
static int gqa_runs(spmv_csr &A, spmv_csr &T, const Pattern &a, float scale, std::mt19937 &rng)
{
    constexpr int H = 4, G = 2, C2 = H / G;
    const int shapes[][2] = {{6, 10}, {40, 64}};
    const int64_t R = a.rows, C = a.cols;
    int status = 0;
    for (auto &kk : shapes)
        for (int odd = 0; odd < 2; ++odd) {
            const int k = kk[0], kv = kk[1];
            int V = 1;
            while (4 * V < std::max(k, kv)) V *= 2;
            g_group_lanes = V;
            auto ld = [&](int w) { return (int64_t)(odd ? w + 1 + ((w + 1) % 4 == 0) : (w + 3) / 4 * 4 + 4); };
            const int64_t lk = ld(k), lv = ld(kv);
            float *Q[H], *K[C2], *Vm[C2], *dO[H], *O[H], *dQ[H], *dK[H], *dV[H], *stats[H], *delta[H];
            plan_heads(A, 1);
            plan_heads(T, 1);
            for (int c = 0; c < C2; ++c) K[c] = matrix(C, k, lk, rng, true), Vm[c] = matrix(C, kv, lv, rng, true);
            for (int y = 0; y < H; ++y) {
                const int c = y / G;
                Q[y] = matrix(R, k, lk, rng, true), dO[y] = matrix(R, kv, lv, rng, true), O[y] = matrix(R, kv, lv, rng, false);
                dQ[y] = matrix(R, k, lk, rng, false), dK[y] = matrix(C, k, lk, rng, false), dV[y] = matrix(C, kv, lv, rng, false);
                stats[y] = (float *)malloc(8 * R), delta[y] = (float *)malloc(4 * R);
                const HeadsMatrix q{Q[y], lk, 0}, kj{K[c], lk, 0}, vj{Vm[c], lv, 0}, o{O[y], lv, 0}, g{dO[y], lv, 0};
                const HeadsMatrix ms{stats[y], 0, 0}, md{delta[y], 0, 0};
                status |= forward(A, 1, 1, scale, k, kv, q, kj, vj, o, ms);
                status |= backward_q(A, 1, 1, scale, k, kv, q, kj, vj, o, g, ms, md, {dQ[y], lk, 0});
                status |= backward_kv(T, 1, 1, false, scale, k, kv, q, kj, vj, g, ms, md, {dK[y], lk, 0}, {dV[y], lv, 0});
            }
            // the per-head dK, dV folded in head order into the first head's arrays of each group
            for (int c = 0; c < C2; ++c)
                for (int i = 1; i < G; ++i)
                    for (int64_t j = 0; j < C; ++j) {
                        for (int x = 0; x < k; ++x) dK[c * G][j * lk + x] = dK[c * G][j * lk + x] + dK[c * G + i][j * lk + x];
                        for (int x = 0; x < kv; ++x) dV[c * G][j * lv + x] = dV[c * G][j * lv + x] + dV[c * G + i][j * lv + x];
                    }
            plan_heads(A, H);
            plan_heads(T, H);
            auto make = [&](int heads, int64_t rows, int w) { return heads_matrix(heads, rows, w, ld(w), (rows * ld(w) + 3) / 4 * 4 + 8, !odd); };
            HeadsMatrix hQ = make(H, R, k), hK = make(C2, C, k), hV = make(C2, C, kv), hdO = make(H, R, kv), hO = make(H, R, kv),
                        hdQ = make(H, R, k), hdK = make(C2, C, k), hdV = make(C2, C, kv);
            const int64_t sstats = 2 * R + 2, sdelta = R + 3;
            float *hstats = (float *)malloc(4 * (size_t)((H - 1) * sstats + 2 * R)), *hdelta = (float *)malloc(4 * (size_t)((H - 1) * sdelta + R));
            for (int y = 0; y < H; ++y) put_head(hQ, y, Q[y], lk, R, k), put_head(hdO, y, dO[y], lv, R, kv);
            for (int c = 0; c < C2; ++c) put_head(hK, c, K[c], lk, C, k), put_head(hV, c, Vm[c], lv, C, kv);
            const HeadsMatrix ms{hstats, 0, sstats}, md{hdelta, 0, sdelta};
            status |= forward(A, H, G, scale, k, kv, hQ, hK, hV, hO, ms);
            status |= backward_q(A, H, G, scale, k, kv, hQ, hK, hV, hO, hdO, ms, md, hdQ);
            status |= backward_kv(T, H, G, true, scale, k, kv, hQ, hK, hV, hdO, ms, md, hdK, hdV);
            long bad = 0;
            for (int y = 0; y < H; ++y) {
                bad += head_differs(hO, y, O[y], lv, R, kv) + head_differs(hdQ, y, dQ[y], lk, R, k);
                bad += std::memcmp(hstats + y * sstats, stats[y], 8 * (size_t)R) != 0;
                bad += std::memcmp(hdelta + y * sdelta, delta[y], 4 * (size_t)R) != 0;
            }
            for (int c = 0; c < C2; ++c) bad += head_differs(hdK, c, dK[c * G], lk, C, k) + head_differs(hdV, c, dV[c * G], lv, C, kv);
            printf("gqa heads %d group %d k %d kv %d V %d %s: status %d, %ld rows differ in a bit from the single-head runs folded in head order\n",
                   H, G, k, kv, V, odd ? "4-byte path" : "16-byte path", status, bad);
            if (bad) status |= 128;
            for (void *p : {(void *)hQ.p, (void *)hK.p, (void *)hV.p, (void *)hdO.p, (void *)hO.p, (void *)hdQ.p, (void *)hdK.p, (void *)hdV.p,
                            (void *)hstats, (void *)hdelta})
                free(p);
            for (int c = 0; c < C2; ++c) free(K[c]), free(Vm[c]);
            for (int y = 0; y < H; ++y)
                for (void *p : {(void *)Q[y], (void *)dO[y], (void *)O[y], (void *)dQ[y], (void *)dK[y], (void *)dV[y], (void *)stats[y], (void *)delta[y]})
                    free(p);
        }
    return status;
}

// ---- 16-bit matrices ------------------------------------------------------------------------------------------------------
// fp32 to the bits of E, to nearest even, written apart from lane_group.hpp's round16: the two neighbours of f in E are found
// by dropping bits, the nearer wins, a tie goes to the even one (fp16: the compiler's conversion, as in the kernels)
template <typename E> static uint16_t to16(float f)
{
    if constexpr (std::is_same<E, fp16>::value) {
        const fp16 x = (fp16)f;
        uint16_t b;
        std::memcpy(&b, &x, 2);
        return b;
    } else {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        if (f != f) return (uint16_t)((u >> 16) | 0x40u);
        const uint32_t lo = u & 0xffff0000u, hi = lo + 0x10000u;        // (hi may be Inf: the magnitude bits just count up)
        float fl, fh;
        std::memcpy(&fl, &lo, 4);
        std::memcpy(&fh, &hi, 4);
        if (lo == u || std::isinf(f)) return (uint16_t)(u >> 16);
        const double dl = std::fabs((double)f - (double)fl), dh = std::isinf(fh) ? std::ldexp(1.0, 120) : std::fabs((double)fh - (double)f);
        const bool up = std::isinf(fh) ? (u & 0xffffu) >= 0x8000u : dh < dl || (dh == dl && ((lo >> 16) & 1u));
        return (uint16_t)((up ? hi : lo) >> 16);
    }
}

template <typename E> static float from16(uint16_t b)
{
    if constexpr (std::is_same<E, fp16>::value) {
        fp16 x;
        std::memcpy(&x, &b, 2);
        return (float)x;
    } else {
        const uint32_t u = (uint32_t)b << 16;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    }
}

// the 16-bit twin of a HeadsMatrix: the same ld and stride in elements, an exactly sized block of 2-byte elements (8-byte
// aligned; it ends where the last row of the last head does: at its width, on the 8-byte path at the end of its last slice);
// src: the fp32 block whose elements it holds rounded, or none (an output: NaN bits)
template <typename E> static E *twin16(const HeadsMatrix &m, int heads, int64_t rows, int w, bool vec, bool fill)
{
    const size_t n = (size_t)((heads - 1) * m.stride + (rows - 1) * m.ld + (vec ? (w + 3) / 4 * 4 : w));
    uint16_t *p = (uint16_t *)malloc(2 * n);
    for (size_t i = 0; i < n; ++i) p[i] = 0x7fffu;
    if (fill)
        for (int y = 0; y < heads; ++y)
            for (int64_t r = 0; r < rows; ++r)
                for (int c = 0; c < w; ++c) p[y * m.stride + r * m.ld + c] = to16<E>(m.p[y * m.stride + r * m.ld + c]);
    return (E *)p;
}

// how many of the heads x rows x w elements differ in a bit from the fp32 block's, rounded (a NaN against a NaN is no difference)
template <typename E> static long differs16(const E *got, const HeadsMatrix &m, int heads, int64_t rows, int w)
{
    long bad = 0;
    const uint16_t *g = (const uint16_t *)got;
    for (int y = 0; y < heads; ++y)
        for (int64_t r = 0; r < rows; ++r)
            for (int c = 0; c < w; ++c) {
                const float want = m.p[y * m.stride + r * m.ld + c];
                const uint16_t b = g[y * m.stride + r * m.ld + c];
                bad += want != want ? from16<E>(b) == from16<E>(b) : b != to16<E>(want);
            }
    return bad;
}

// Four query heads on two K/V heads on 16-bit matrices against the program's own fp32 _gqa runs on the same, widened data.
template <typename E> static int runs16(const char *name, spmv_csr &A, spmv_csr &T, const Pattern &a, float scale, std::mt19937 &rng)
{
    constexpr int H = 4, G = 2, C2 = H / G;
    const int shapes[][2] = {{6, 10}, {40, 64}};
    const int64_t R = a.rows, C = a.cols;
    int status = 0;
    plan_heads(A, H);
    plan_heads(T, H);
    for (auto &kk : shapes)
        for (int odd = 0; odd < 2; ++odd) {
            const int k = kk[0], kv = kk[1];
            int V = 1;
            while (4 * V < std::max(k, kv)) V *= 2;
            g_group_lanes = V;
            auto ld = [&](int w) { return (int64_t)(odd ? w + 1 + ((w + 1) % 4 == 0) : (w + 3) / 4 * 4 + 4); };
            auto make = [&](int heads, int64_t rows, int w) { return heads_matrix(heads, rows, w, ld(w), (rows * ld(w) + 3) / 4 * 4 + 8, !odd); };
            HeadsMatrix hQ = make(H, R, k), hK = make(C2, C, k), hV = make(C2, C, kv), hdO = make(H, R, kv), hO = make(H, R, kv),
                        hdQ = make(H, R, k), hdK = make(C2, C, k), hdV = make(C2, C, kv);
            // inputs: normal numbers with +0 and -0 among them, every one a number of E
            std::normal_distribution<float> nd(0.f, 1.f);
            auto fill = [&](const HeadsMatrix &m, int heads, int64_t rows, int w) {
                for (int y = 0; y < heads; ++y)
                    for (int64_t r = 0; r < rows; ++r)
                        for (int c = 0; c < w; ++c) {
                            const unsigned z = rng() % 64;
                            m.p[y * m.stride + r * m.ld + c] = z == 0 ? 0.0f : z == 1 ? -0.0f : from16<E>(to16<E>(nd(rng)));
                        }
            };
            fill(hQ, H, R, k), fill(hK, C2, C, k), fill(hV, C2, C, kv), fill(hdO, H, R, kv);
            const int64_t sstats = 2 * R + 2, sdelta = R + 3;
            const size_t nstats = (size_t)((H - 1) * sstats + 2 * R), ndelta = (size_t)((H - 1) * sdelta + R);
            float *stats = (float *)malloc(4 * nstats), *delta = (float *)malloc(4 * ndelta);
            float *stats16 = (float *)malloc(4 * nstats), *delta16 = (float *)malloc(4 * ndelta);
            const HeadsMatrix ms{stats, 0, sstats}, md{delta, 0, sdelta};
            // the fp32 runs; backward_q reads the rounded O, as the 16-bit call does
            status |= forward(A, H, G, scale, k, kv, hQ, hK, hV, hO, ms);
            HeadsMatrix hO16 = make(H, R, kv);
            for (int y = 0; y < H; ++y)
                for (int64_t r = 0; r < R; ++r)
                    for (int c = 0; c < kv; ++c) hO16.p[y * hO.stride + r * hO.ld + c] = from16<E>(to16<E>(hO.p[y * hO.stride + r * hO.ld + c]));
            status |= backward_q(A, H, G, scale, k, kv, hQ, hK, hV, hO16, hdO, ms, md, hdQ);
            status |= backward_kv(T, H, G, true, scale, k, kv, hQ, hK, hV, hdO, ms, md, hdK, hdV);
            // the 16-bit runs on exactly sized blocks of 2-byte elements
            const bool vec = !odd;
            E *Q = twin16<E>(hQ, H, R, k, vec, true), *K = twin16<E>(hK, C2, C, k, vec, true), *Vm = twin16<E>(hV, C2, C, kv, vec, true);
            E *dO = twin16<E>(hdO, H, R, kv, vec, true), *O = twin16<E>(hO, H, R, kv, vec, false), *dQ = twin16<E>(hdQ, H, R, k, vec, false);
            E *dK = twin16<E>(hdK, C2, C, k, vec, false), *dV = twin16<E>(hdV, C2, C, kv, vec, false);
            AttnArgsT<E> in{};
            in.scale = scale, in.k = k, in.kv = kv;
            in.Q = Q, in.ldq = hQ.ld, in.hq = hQ.stride, in.K = K, in.ldk = hK.ld, in.hk = hK.stride, in.V = Vm, in.ldv = hV.ld, in.hv = hV.stride;
            AttnArgsT<E> f = in, bq = in, bk = in;
            f.out0 = O, f.ld0 = hO.ld, f.h0 = hO.stride, f.stats = stats16, f.hstats = sstats;
            status |= launch_attention(kPassForward, A, f, nullptr, H, G, false, "forward_16", nullptr);
            bq.O = O, bq.ldo = hO.ld, bq.ho = hO.stride, bq.dO = dO, bq.lddo = hdO.ld, bq.hdo = hdO.stride;
            bq.stats_in = stats16, bq.hstats_in = sstats, bq.delta = delta16, bq.hdelta = sdelta, bq.out0 = dQ, bq.ld0 = hdQ.ld, bq.h0 = hdQ.stride;
            status |= launch_attention(kPassBackwardQ, A, bq, nullptr, H, G, false, "backward_q_16", nullptr);
            bk.dO = dO, bk.lddo = hdO.ld, bk.hdo = hdO.stride, bk.stats_in = stats16, bk.hstats_in = sstats, bk.delta_in = delta16, bk.hdelta_in = sdelta;
            bk.out0 = dK, bk.ld0 = hdK.ld, bk.h0 = hdK.stride, bk.out1 = dV, bk.ld1 = hdV.ld, bk.h1 = hdV.stride;
            status |= launch_attention(kPassBackwardKV, T, bk, nullptr, H, G, true, "backward_kv_16", nullptr);
            long bad = differs16<E>(O, hO, H, R, kv) + differs16<E>(dQ, hdQ, H, R, k) + differs16<E>(dK, hdK, C2, C, k) + differs16<E>(dV, hdV, C2, C, kv);
            for (int y = 0; y < H; ++y) {
                bad += std::memcmp(stats16 + y * sstats, stats + y * sstats, 8 * (size_t)R) != 0;
                bad += std::memcmp(delta16 + y * sdelta, delta + y * sdelta, 4 * (size_t)R) != 0;
            }
            printf("%s heads %d group %d k %d kv %d V %d %s: status %d, %ld elements differ in a bit from the fp32 runs on the widened data, rounded\n",
                   name, H, G, k, kv, V, odd ? "2-byte path" : "8-byte path", status, bad);
            if (bad) status |= 256;
            for (void *p : {(void *)hQ.p, (void *)hK.p, (void *)hV.p, (void *)hdO.p, (void *)hO.p, (void *)hO16.p, (void *)hdQ.p, (void *)hdK.p,
                            (void *)hdV.p, (void *)stats, (void *)delta, (void *)stats16, (void *)delta16, (void *)Q, (void *)K, (void *)Vm,
                            (void *)dO, (void *)O, (void *)dQ, (void *)dK, (void *)dV})
                free(p);
        }
    return status;
}

// ---- the additive bias --------------------------------------------------------------------------------------------------------
template <typename E> static float elem(const E *p, int64_t i)
{
    if constexpr (std::is_same<E, float>::value) {
        return p[i];
    } else {
        uint16_t b;
        std::memcpy(&b, (const uint16_t *)p + i, 2);
        return from16<E>(b);
    }
}

// an exactly sized block of E with the layout of m: the fp32 block itself, or its 16-bit twin
template <typename E> static E *as_elements(const HeadsMatrix &m, int heads, int64_t rows, int w, bool vec, bool fill)
{
    if constexpr (std::is_same<E, float>::value) return m.p;
    else return twin16<E>(m, heads, rows, w, vec, fill);
}

// v32: the V = 32 section instead: (128, 128) and (65, 100) on the wide scratch, with a bias and (with_bias = false) without one:
// the unbiased kernels, a bias of zeros in the serial statement, no dBias
template <typename E> static int bias_runs(const char *name, spmv_csr &A, spmv_csr &T, const Pattern &a, const Pattern &t, float scale, std::mt19937 &rng,
                                           bool v32 = false, bool with_bias = true)
{
    constexpr int H = 4, G = 2, C2 = H / G;
    constexpr bool wide = std::is_same<E, float>::value;
    const double tol = wide ? 2e-5 : 2e-5 + 1.0 / 128;
    const int narrow_shapes[][2] = {{6, 10}, {40, 64}}, wide_shapes[][2] = {{128, 128}, {65, 100}};
    const auto &shapes = v32 ? wide_shapes : narrow_shapes;
    const int64_t R = a.rows, C = a.cols, nnz = A.nnz;
    int status = 0;
    (v32 ? plan_wide : plan_heads)(A, H);
    (v32 ? plan_wide : plan_heads)(T, H);
    // map[i]: the position in a of nonzero i of t (the stable order of transpose() above)
    std::vector<int32_t> map((size_t)nnz), at(t.rp.begin(), t.rp.end() - 1);
    for (int64_t r = 0; r < R; ++r)
        for (int n = a.rp[r]; n < a.rp[r + 1]; ++n) map[(size_t)at[a.ci[n]]++] = n;
    for (auto &kk : shapes)
        for (int odd = 0; odd < 2; ++odd) {
            const int k = kk[0], kv = kk[1];
            int V = 1;
            while (4 * V < std::max(k, kv)) V *= 2;
            g_group_lanes = V;
            const bool vec = !odd;
            auto ld = [&](int w) { return (int64_t)(odd ? w + 1 + ((w + 1) % 4 == 0) : (w + 3) / 4 * 4 + 4); };
            auto make = [&](int heads, int64_t rows, int w) { return heads_matrix(heads, rows, w, ld(w), (rows * ld(w) + 3) / 4 * 4 + 8, vec); };
            HeadsMatrix hQ = make(H, R, k), hK = make(C2, C, k), hV = make(C2, C, kv), hdO = make(H, R, kv), hO = make(H, R, kv),
                        hdQ = make(H, R, k), hdK = make(C2, C, k), hdV = make(C2, C, kv);
            std::normal_distribution<float> nd(0.f, 1.f);
            auto fill = [&](const HeadsMatrix &m, int heads, int64_t rows, int w) {
                for (int y = 0; y < heads; ++y)
                    for (int64_t r = 0; r < rows; ++r)
                        for (int c = 0; c < w; ++c) {
                            const float x = nd(rng);
                            if constexpr (wide) m.p[y * m.stride + r * m.ld + c] = x;
                            else m.p[y * m.stride + r * m.ld + c] = from16<E>(to16<E>(x));
                        }
            };
            fill(hQ, H, R, k), fill(hK, C2, C, k), fill(hV, C2, C, kv), fill(hdO, H, R, kv);
            const int64_t sstats = 2 * R + 2, sdelta = R + 3, sb = nnz + 3, sdb = nnz + 1;
            float *stats = (float *)malloc(4 * (size_t)((H - 1) * sstats + 2 * R)), *delta = (float *)malloc(4 * (size_t)((H - 1) * sdelta + R));
            float *bias = (float *)malloc(4 * (size_t)((H - 1) * sb + nnz)), *bias_t = (float *)malloc(4 * (size_t)((H - 1) * sb + nnz));
            float *dbias = (float *)malloc(4 * (size_t)((H - 1) * sdb + nnz));
            for (int64_t i = 0; i < (H - 1) * sb + nnz; ++i) bias[i] = bias_t[i] = NAN;
            for (int64_t i = 0; i < (H - 1) * sdb + nnz; ++i) dbias[i] = NAN;
            for (int y = 0; y < H; ++y) {
                for (int64_t n = 0; n < nnz; ++n) bias[y * sb + n] = with_bias ? nd(rng) : 0.0f;
                for (int64_t i = 0; i < nnz; ++i) bias_t[y * sb + i] = bias[y * sb + map[(size_t)i]];
            }
            E *Q = as_elements<E>(hQ, H, R, k, vec, true), *K = as_elements<E>(hK, C2, C, k, vec, true), *Vm = as_elements<E>(hV, C2, C, kv, vec, true);
            E *dO = as_elements<E>(hdO, H, R, kv, vec, true), *O = as_elements<E>(hO, H, R, kv, vec, false), *dQ = as_elements<E>(hdQ, H, R, k, vec, false);
            E *dK = as_elements<E>(hdK, C2, C, k, vec, false), *dV = as_elements<E>(hdV, C2, C, kv, vec, false);
            AttnArgsT<E> in{};
            in.scale = scale, in.k = k, in.kv = kv;
            in.Q = Q, in.ldq = hQ.ld, in.hq = hQ.stride, in.K = K, in.ldk = hK.ld, in.hk = hK.stride, in.V = Vm, in.ldv = hV.ld, in.hv = hV.stride;
            AttnArgsT<E> f = in, bq = in, bk = in;
            const AttnBias bf{bias, sb, nullptr, 0}, bqb{bias, sb, dbias, sdb}, bkb{bias_t, sb, nullptr, 0};
            f.out0 = O, f.ld0 = hO.ld, f.h0 = hO.stride, f.stats = stats, f.hstats = sstats;
            status |= launch_attention(kPassForward, A, f, with_bias ? &bf : nullptr, H, G, false, "forward_bias", nullptr);
            bq.O = O, bq.ldo = hO.ld, bq.ho = hO.stride, bq.dO = dO, bq.lddo = hdO.ld, bq.hdo = hdO.stride;
            bq.stats_in = stats, bq.hstats_in = sstats, bq.delta = delta, bq.hdelta = sdelta, bq.out0 = dQ, bq.ld0 = hdQ.ld, bq.h0 = hdQ.stride;
            status |= launch_attention(kPassBackwardQ, A, bq, with_bias ? &bqb : nullptr, H, G, false, "backward_q_bias", nullptr);
            bk.dO = dO, bk.lddo = hdO.ld, bk.hdo = hdO.stride, bk.stats_in = stats, bk.hstats_in = sstats, bk.delta_in = delta, bk.hdelta_in = sdelta;
            bk.out0 = dK, bk.ld0 = hdK.ld, bk.h0 = hdK.stride, bk.out1 = dV, bk.ld1 = hdV.ld, bk.h1 = hdV.stride;
            status |= launch_attention(kPassBackwardKV, T, bk, with_bias ? &bkb : nullptr, H, G, true, "backward_kv_bias", nullptr);
            // serial fp64 attention with bias, per query head; dK and dV summed over the heads of a group
            double worst = 0.0;
            long unwritten = 0;
            auto err = [&](double got, double want, double mag) { worst = std::max(worst, std::fabs(got - want) / (mag + 1e-30)); };
            std::vector<double> rdK((size_t)(C2 * C * k), 0.0), rdV((size_t)(C2 * C * kv), 0.0), mK(rdK), mV(rdV);
            for (int y = 0; y < H; ++y) {
                const int c2 = y / G;
                const float *q = hQ.p + y * hQ.stride, *kj = hK.p + c2 * hK.stride, *vj = hV.p + c2 * hV.stride, *g = hdO.p + y * hdO.stride;
                for (int64_t i = 0; i < R; ++i) {
                    const int b = a.rp[i], e = a.rp[i + 1], L = e - b;
                    std::vector<double> p((size_t)L), dp((size_t)L), adp((size_t)L);
                    double M = -INFINITY, S = 0.0, dot = 0.0, adot = 0.0;
                    for (int n = b; n < e; ++n) {
                        double s = 0.0;
                        for (int c = 0; c < k; ++c) s += (double)q[i * hQ.ld + c] * kj[a.ci[n] * hK.ld + c];
                        p[n - b] = s * scale + bias[y * sb + n];
                        M = std::max(M, p[n - b]);
                    }
                    for (int n = 0; n < L; ++n) S += (p[n] = std::exp(p[n] - M));
                    for (int n = 0; n < L; ++n) {
                        p[n] /= S;
                        double s = 0.0, as = 0.0;
                        for (int c = 0; c < kv; ++c) {
                            const double x = (double)g[i * hdO.ld + c] * vj[a.ci[b + n] * hV.ld + c];
                            s += x, as += std::fabs(x);
                        }
                        dp[n] = s, adp[n] = as, dot += p[n] * s, adot += p[n] * as;
                    }
                    for (int c = 0; c < kv; ++c) {
                        double o = 0.0, ao = 0.0;
                        for (int n = 0; n < L; ++n) o += p[n] * vj[a.ci[b + n] * hV.ld + c], ao += p[n] * std::fabs(vj[a.ci[b + n] * hV.ld + c]);
                        err(elem<E>(O, y * hO.stride + i * hO.ld + c), o, ao + (L == 0));
                    }
                    for (int n = 0; n < L; ++n) {
                        const double gb = p[n] * (dp[n] - dot), agb = p[n] * (adp[n] + adot + 1e-3);
                        const float got = dbias[y * sdb + b + n];
                        if (with_bias) {
                            unwritten += got != got;
                            err(got, gb, agb);
                        }
                        for (int c = 0; c < k; ++c) {
                            rdK[(size_t)((c2 * C + a.ci[b + n]) * k + c)] += scale * gb * q[i * hQ.ld + c];
                            mK[(size_t)((c2 * C + a.ci[b + n]) * k + c)] += scale * agb * std::fabs(q[i * hQ.ld + c]);
                        }
                        for (int c = 0; c < kv; ++c) {
                            rdV[(size_t)((c2 * C + a.ci[b + n]) * kv + c)] += p[n] * g[i * hdO.ld + c];
                            mV[(size_t)((c2 * C + a.ci[b + n]) * kv + c)] += p[n] * std::fabs(g[i * hdO.ld + c]);
                        }
                    }
                    for (int c = 0; c < k; ++c) {
                        double d = 0.0, ad = 0.0;
                        for (int n = 0; n < L; ++n) {
                            d += scale * p[n] * (dp[n] - dot) * kj[a.ci[b + n] * hK.ld + c];
                            ad += scale * p[n] * (adp[n] + adot + 1e-3) * std::fabs(kj[a.ci[b + n] * hK.ld + c]);
                        }
                        err(elem<E>(dQ, y * hdQ.stride + i * hdQ.ld + c), d, ad + (L == 0));
                    }
                }
            }
            for (int c2 = 0; c2 < C2; ++c2)
                for (int64_t j = 0; j < C; ++j) {
                    const double none = t.rp[j + 1] == t.rp[j] ? 1.0 : 0.0;
                    for (int c = 0; c < k; ++c) err(elem<E>(dK, c2 * hdK.stride + j * hdK.ld + c), rdK[(size_t)((c2 * C + j) * k + c)], mK[(size_t)((c2 * C + j) * k + c)] + none);
                    for (int c = 0; c < kv; ++c) err(elem<E>(dV, c2 * hdV.stride + j * hdV.ld + c), rdV[(size_t)((c2 * C + j) * kv + c)], mV[(size_t)((c2 * C + j) * kv + c)] + none);
                }
            printf("%s %s heads %d group %d k %d kv %d V %d %s: status %d, worst normalised error %.3g (allowed %.3g), %ld positions of dBias unwritten\n",
                   with_bias ? "bias" : "no bias", name, H, G, k, kv, V, odd ? "scalar path" : "vector path", status, worst, tol, unwritten);
            if (!(worst <= tol) || unwritten) status |= 512;
            if constexpr (!wide)
                for (void *p : {(void *)Q, (void *)K, (void *)Vm, (void *)dO, (void *)O, (void *)dQ, (void *)dK, (void *)dV}) free(p);
            for (void *p : {(void *)hQ.p, (void *)hK.p, (void *)hV.p, (void *)hdO.p, (void *)hO.p, (void *)hdQ.p, (void *)hdK.p, (void *)hdV.p,
                            (void *)stats, (void *)delta, (void *)bias, (void *)bias_t, (void *)dbias})
                free(p);
        }
    return status;
}

// ---- V = 32 against the other geometries: zero padding ------------------------------------------------------------------------
// Four query heads on two K/V heads with a bias at (k, kv) <= 64, both load paths: the narrow run (forward, then both backward
// passes on its O, stats and delta), then the same operands padded with zero columns to (128, 128) through the V = 32 kernels on
// exactly sized blocks and the wide scratch, the backward passes on the narrow run's stats and delta (and its O, padded).  delta,
// dBias, dQ[:, :k], dK[:, :k], dV[:, :kv] bit for bit, the padded columns +0.  (The forward pass shares the bits only where every
// expf argument is exact: T differs, and the rescale is per step.)
static int padding_runs(spmv_csr &A, spmv_csr &T, const Pattern &a, const Pattern &t, float scale, std::mt19937 &rng)
{
    constexpr int H = 4, G = 2, C2 = H / G, W = 128;
    const int shapes[][2] = {{64, 20}, {8, 40}, {16, 12}};
    const int64_t R = a.rows, C = a.cols, nnz = A.nnz;
    int status = 0;
    plan_wide(A, H);
    plan_wide(T, H);
    std::vector<int32_t> map((size_t)nnz), at(t.rp.begin(), t.rp.end() - 1);
    for (int64_t r = 0; r < R; ++r)
        for (int n = a.rp[r]; n < a.rp[r + 1]; ++n) map[(size_t)at[a.ci[n]]++] = n;
    for (auto &kk : shapes)
        for (int odd = 0; odd < 2; ++odd) {
            const int k = kk[0], kv = kk[1];
            const bool vec = !odd;
            auto ld = [&](int w) { return (int64_t)(odd ? w + 1 + ((w + 1) % 4 == 0) : (w + 3) / 4 * 4 + 4); };
            auto make = [&](int heads, int64_t rows, int w) { return heads_matrix(heads, rows, w, ld(w), (rows * ld(w) + 3) / 4 * 4 + 8, vec); };
            std::normal_distribution<float> nd(0.f, 1.f);
            // n: the narrow operands; w: the same padded with zeros (inputs) or NaN-filled (outputs)
            HeadsMatrix nQ = make(H, R, k), nK = make(C2, C, k), nV = make(C2, C, kv), ndO = make(H, R, kv), nO = make(H, R, kv),
                        ndQ = make(H, R, k), ndK = make(C2, C, k), ndV = make(C2, C, kv);
            HeadsMatrix wQ = make(H, R, W), wK = make(C2, C, W), wV = make(C2, C, W), wdO = make(H, R, W), wO = make(H, R, W),
                        wdQ = make(H, R, W), wdK = make(C2, C, W), wdV = make(C2, C, W);
            auto fill = [&](const HeadsMatrix &m, const HeadsMatrix &p, int heads, int64_t rows, int w) {
                for (int y = 0; y < heads; ++y)
                    for (int64_t r = 0; r < rows; ++r)
                        for (int c = 0; c < W; ++c) {
                            const float x = c < w ? nd(rng) : 0.0f;
                            if (c < w) m.p[y * m.stride + r * m.ld + c] = x;
                            p.p[y * p.stride + r * p.ld + c] = x;
                        }
            };
            fill(nQ, wQ, H, R, k), fill(nK, wK, C2, C, k), fill(nV, wV, C2, C, kv), fill(ndO, wdO, H, R, kv);
            const int64_t sstats = 2 * R + 2, sdelta = R + 3, sb = nnz + 3, sdb = nnz + 1;
            float *stats = (float *)malloc(4 * (size_t)((H - 1) * sstats + 2 * R)), *delta = (float *)malloc(4 * (size_t)((H - 1) * sdelta + R));
            float *wdelta = (float *)malloc(4 * (size_t)((H - 1) * sdelta + R));
            float *bias = (float *)malloc(4 * (size_t)((H - 1) * sb + nnz)), *bias_t = (float *)malloc(4 * (size_t)((H - 1) * sb + nnz));
            float *dbias = (float *)malloc(4 * (size_t)((H - 1) * sdb + nnz)), *wdbias = (float *)malloc(4 * (size_t)((H - 1) * sdb + nnz));
            for (int64_t i = 0; i < (H - 1) * sb + nnz; ++i) bias[i] = bias_t[i] = NAN;
            for (int64_t i = 0; i < (H - 1) * sdb + nnz; ++i) dbias[i] = wdbias[i] = NAN;
            for (int y = 0; y < H; ++y) {
                for (int64_t n = 0; n < nnz; ++n) bias[y * sb + n] = nd(rng);
                for (int64_t i = 0; i < nnz; ++i) bias_t[y * sb + i] = bias[y * sb + map[(size_t)i]];
            }
            const AttnBias bf{bias, sb, nullptr, 0}, bkb{bias_t, sb, nullptr, 0};
            auto passes = [&](int w_k, int w_kv, const HeadsMatrix &Q, const HeadsMatrix &K, const HeadsMatrix &V, const HeadsMatrix &dO,
                              const HeadsMatrix &O, const HeadsMatrix &dQ, const HeadsMatrix &dK, const HeadsMatrix &dV, float *del, float *db,
                              bool fwd) {
                int lanes = 1;
                while (4 * lanes < std::max(w_k, w_kv)) lanes *= 2;
                g_group_lanes = lanes;
                AttnArgs in = attn_inputs(scale, w_k, w_kv, Q, K, V);
                AttnArgs f = in, bq = in, bk = in;
                f.out0 = O.p, f.ld0 = O.ld, f.h0 = O.stride, f.stats = stats, f.hstats = sstats;
                if (fwd) status |= launch_attention(kPassForward, A, f, &bf, H, G, false, "forward", nullptr);
                const AttnBias bqb{bias, sb, db, sdb};
                bq.O = O.p, bq.ldo = O.ld, bq.ho = O.stride, bq.dO = dO.p, bq.lddo = dO.ld, bq.hdo = dO.stride;
                bq.stats_in = stats, bq.hstats_in = sstats, bq.delta = del, bq.hdelta = sdelta, bq.out0 = dQ.p, bq.ld0 = dQ.ld, bq.h0 = dQ.stride;
                status |= launch_attention(kPassBackwardQ, A, bq, &bqb, H, G, false, "backward_q", nullptr);
                bk.dO = dO.p, bk.lddo = dO.ld, bk.hdo = dO.stride, bk.stats_in = stats, bk.hstats_in = sstats, bk.delta_in = delta, bk.hdelta_in = sdelta;
                bk.out0 = dK.p, bk.ld0 = dK.ld, bk.h0 = dK.stride, bk.out1 = dV.p, bk.ld1 = dV.ld, bk.h1 = dV.stride;
                status |= launch_attention(kPassBackwardKV, T, bk, &bkb, H, G, true, "backward_kv", nullptr);
            };
            passes(k, kv, nQ, nK, nV, ndO, nO, ndQ, ndK, ndV, delta, dbias, true);
            // the narrow O, padded, is the wide backward_q's O
            for (int y = 0; y < H; ++y)
                for (int64_t r = 0; r < R; ++r)
                    for (int c = 0; c < W; ++c) wO.p[y * wO.stride + r * wO.ld + c] = c < kv ? nO.p[y * nO.stride + r * nO.ld + c] : 0.0f;
            passes(W, W, wQ, wK, wV, wdO, wO, wdQ, wdK, wdV, wdelta, wdbias, false);
            // bit for bit in the original columns, +0 in the padded ones
            auto cmp = [&](const HeadsMatrix &n, const HeadsMatrix &w, int heads, int64_t rows, int width) {
                long bad = 0;
                const float zero = 0.0f;
                for (int y = 0; y < heads; ++y)
                    for (int64_t r = 0; r < rows; ++r) {
                        bad += std::memcmp(n.p + y * n.stride + r * n.ld, w.p + y * w.stride + r * w.ld, 4 * (size_t)width) != 0;
                        for (int c = width; c < W; ++c) bad += std::memcmp(w.p + y * w.stride + r * w.ld + c, &zero, 4) != 0;
                    }
                return bad;
            };
            long bad = cmp(ndQ, wdQ, H, R, k) + cmp(ndK, wdK, C2, C, k) + cmp(ndV, wdV, C2, C, kv);
            for (int y = 0; y < H; ++y) {
                bad += std::memcmp(delta + y * sdelta, wdelta + y * sdelta, 4 * (size_t)R) != 0;
                bad += std::memcmp(dbias + y * sdb, wdbias + y * sdb, 4 * (size_t)nnz) != 0;
            }
            printf("zero padding (%d, %d) -> (%d, %d), V 32 against the narrow run, %s: status %d, %ld rows differ in a bit\n", k, kv, W, W,
                   odd ? "4-byte path" : "16-byte path", status, bad);
            if (bad) status |= 1024;
            for (void *p : {(void *)nQ.p, (void *)nK.p, (void *)nV.p, (void *)ndO.p, (void *)nO.p, (void *)ndQ.p, (void *)ndK.p, (void *)ndV.p,
                            (void *)wQ.p, (void *)wK.p, (void *)wV.p, (void *)wdO.p, (void *)wO.p, (void *)wdQ.p, (void *)wdK.p, (void *)wdV.p,
                            (void *)stats, (void *)delta, (void *)wdelta, (void *)bias, (void *)bias_t, (void *)dbias, (void *)wdbias})
                free(p);
        }
    return status;
}

int main()
{
    std::mt19937 rng(11);
    Pattern a;
    a.cols = 300;
    std::vector<int> lens = {0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 64, 100, 299, 0, 3, 5};
    for (int i = 0; i < 1100; ++i) lens.push_back(i % 97 == 0 ? 0 : 1 + (int)(rng() % 4));     // (transposed rows of about 10)
    a.rows = (int64_t)lens.size();
    a.rp.assign(1, 0);
    std::vector<int32_t> all((size_t)a.cols);
    for (int i = 0; i < a.cols; ++i) all[i] = i;
    long unsorted = 0, repeats = 0;       // rows that are not sorted; entries whose key the row already lists
    for (int64_t r = 0; r < a.rows; ++r) {
        std::shuffle(all.begin(), all.end(), rng);
        std::vector<int32_t> row(all.begin(), all.begin() + lens[r]);
        // every fifth row draws its columns with replacement from a few keys (a key may repeat), every third stays unsorted;
        // the rest are sorted
        if (r % 5 == 2)
            for (int32_t &c : row) c = (int32_t)(rng() % std::min<int64_t>(a.cols, 2 * lens[r] + 4));
        if (r % 3 != 1) std::sort(row.begin(), row.end());
        // columns 0 and 1 sit in most rows, so that the transposed pattern has two rows in pieces
        if (r % 10 != 0 && lens[r] && row[0] != 0) row[0] = 0;
        if (r % 7 != 0 && lens[r] > 1 && row[1] != 1 && row[0] == 0) row[1] = 1;
        unsorted += !std::is_sorted(row.begin(), row.end());
        for (size_t i = 0; i < row.size(); ++i) repeats += std::count(row.begin(), row.begin() + (long)i, row[i]) > 0;
        a.ci.insert(a.ci.end(), row.begin(), row.end());
        a.rp.push_back((int32_t)a.ci.size());
    }
    // a long row of the pattern itself: 700 entries with repeats allowed
    for (int i = 0; i < 700; ++i) a.ci.push_back((int32_t)(rng() % a.cols));
    a.rp.push_back((int32_t)a.ci.size());
    ++a.rows;
    const Pattern t = transpose(a);
    std::vector<void *> owned;
    spmv_csr A = make_handle(a, owned), T = make_handle(t, owned);
    printf("pattern %lld x %lld, nnz %lld; long rows %d (pieces %d), transposed %d (pieces %d); %ld rows unsorted, %ld repeated keys before the long row\n",
           (long long)a.rows, (long long)a.cols, (long long)A.nnz, A.plan_spmm.n_long, A.plan_spmm.pieces, T.plan_spmm.n_long, T.plan_spmm.pieces,
           unsorted, repeats);
    if (!A.plan_spmm.n_long || T.plan_spmm.n_long < 2 || unsorted < 50 || repeats < 50) return 2;
    const float scale = 0.25f;
    int status = 0;
    double worst = 0.0;
    const int shapes[][2] = {{24, 24}, {8, 40}, {64, 4}, {6, 10}};
    for (auto &kk : shapes)
        for (int odd = 0; odd < 2; ++odd) {
            const int k = kk[0], kv = kk[1];
            int V = 1;
            while (4 * V < std::max(k, kv)) V *= 2;
            g_group_lanes = V;
            auto ld = [&](int w) { return (int64_t)(odd ? w + 1 + ((w + 1) % 4 == 0) : (w + 3) / 4 * 4 + 4); };
            const int64_t R = a.rows, C = a.cols;
            float *Q = matrix(R, k, ld(k), rng, true), *K = matrix(C, k, ld(k), rng, true), *Vm = matrix(C, kv, ld(kv), rng, true);
            float *dO = matrix(R, kv, ld(kv), rng, true), *O = matrix(R, kv, ld(kv), rng, false), *dQ = matrix(R, k, ld(k), rng, false);
            float *dK = matrix(C, k, ld(k), rng, false), *dV = matrix(C, kv, ld(kv), rng, false);
            float *stats = (float *)malloc(8 * R), *delta = (float *)malloc(4 * R);
            const HeadsMatrix q{Q, ld(k), 0}, kj{K, ld(k), 0}, vj{Vm, ld(kv), 0}, o{O, ld(kv), 0}, g{dO, ld(kv), 0};
            const HeadsMatrix ms{stats, 0, 0}, md{delta, 0, 0};
            status |= forward(A, 1, 1, scale, k, kv, q, kj, vj, o, ms);
            status |= backward_q(A, 1, 1, scale, k, kv, q, kj, vj, o, g, ms, md, {dQ, ld(k), 0});
            status |= backward_kv(T, 1, 1, false, scale, k, kv, q, kj, vj, g, ms, md, {dK, ld(k), 0}, {dV, ld(kv), 0});
            // serial fp64
            std::vector<double> rdK((size_t)(C * k), 0.0), rdV((size_t)(C * kv), 0.0), mK(rdK), mV(rdV);
            auto err = [&](double got, double want, double mag) { worst = std::max(worst, std::fabs(got - want) / (mag + 1e-30)); };
            for (int64_t i = 0; i < R; ++i) {
                const int b = a.rp[i], e = a.rp[i + 1], L = e - b;
                std::vector<double> p((size_t)L), dp((size_t)L);
                double M = -INFINITY, S = 0.0, dot = 0.0, adot = 0.0;
                for (int n = b; n < e; ++n) {
                    double s = 0.0;
                    for (int c = 0; c < k; ++c) s += (double)Q[i * ld(k) + c] * K[a.ci[n] * ld(k) + c];
                    p[n - b] = s * scale;
                    M = std::max(M, p[n - b]);
                }
                for (int n = 0; n < L; ++n) S += (p[n] = std::exp(p[n] - M));
                for (int n = 0; n < L; ++n) {
                    p[n] /= S;
                    double s = 0.0, as = 0.0;
                    for (int c = 0; c < kv; ++c) s += (double)dO[i * ld(kv) + c] * Vm[a.ci[b + n] * ld(kv) + c], as += std::fabs((double)dO[i * ld(kv) + c] * Vm[a.ci[b + n] * ld(kv) + c]);
                    dp[n] = s, dot += p[n] * s, adot += p[n] * as;
                }
                for (int c = 0; c < kv; ++c) {
                    double o = 0.0, ao = 0.0;
                    for (int n = 0; n < L; ++n) o += p[n] * Vm[a.ci[b + n] * ld(kv) + c], ao += p[n] * std::fabs(Vm[a.ci[b + n] * ld(kv) + c]);
                    if (L == 0 && O[i * ld(kv) + c] != 0.0f) status |= 4;
                    err(O[i * ld(kv) + c], o, ao);
                }
                if (L == 0 && !(stats[2 * i] == -INFINITY && stats[2 * i + 1] == 0.0f)) status |= 8;
                for (int c = 0; c < k; ++c) {
                    double g = 0.0, ag = 0.0;
                    for (int n = 0; n < L; ++n) {
                        const double ds = scale * p[n] * (dp[n] - dot), ads = scale * p[n] * (std::fabs(dp[n]) + adot + 1e-3);
                        g += ds * K[a.ci[b + n] * ld(k) + c], ag += ads * std::fabs(K[a.ci[b + n] * ld(k) + c]);
                        rdK[(size_t)(a.ci[b + n] * k + c)] += ds * Q[i * ld(k) + c];
                        mK[(size_t)(a.ci[b + n] * k + c)] += ads * std::fabs(Q[i * ld(k) + c]);
                    }
                    if (L == 0 && dQ[i * ld(k) + c] != 0.0f) status |= 16;
                    err(dQ[i * ld(k) + c], g, ag);
                }
                for (int n = 0; n < L; ++n)
                    for (int c = 0; c < kv; ++c) {
                        rdV[(size_t)(a.ci[b + n] * kv + c)] += p[n] * dO[i * ld(kv) + c];
                        mV[(size_t)(a.ci[b + n] * kv + c)] += p[n] * std::fabs(dO[i * ld(kv) + c]);
                    }
            }
            for (int64_t j = 0; j < C; ++j) {
                for (int c = 0; c < k; ++c) err(dK[j * ld(k) + c], rdK[(size_t)(j * k + c)], mK[(size_t)(j * k + c)] + (t.rp[j + 1] == t.rp[j] ? 1.0 : 0.0));
                for (int c = 0; c < kv; ++c) err(dV[j * ld(kv) + c], rdV[(size_t)(j * kv + c)], mV[(size_t)(j * kv + c)] + (t.rp[j + 1] == t.rp[j] ? 1.0 : 0.0));
            }
            printf("k %d kv %d V %d %s: status %d, worst normalised error so far %.3g\n", k, kv, V, odd ? "4-byte path" : "16-byte path", status, worst);
            // SDDMM at this k: U = Q, X = K on the pattern; the operands trade places on the transpose
            const long sa = sddmm_differing(A, a, k, Q, ld(k), K, ld(k)), st = sddmm_differing(T, t, k, K, ld(k), Q, ld(k));
            printf("sddmm k %d %s: %ld of %lld results differ in a bit on the pattern, %ld on its transpose\n", k,
                   odd ? "4-byte path" : "16-byte path", sa, (long long)A.nnz, st);
            if (sa != 0 || st != 0) status |= 32;
            for (void *p : {(void *)Q, (void *)K, (void *)Vm, (void *)dO, (void *)O, (void *)dQ, (void *)dK, (void *)dV, (void *)stats, (void *)delta}) free(p);
        }
    status |= heads_runs(A, T, a, scale, rng);
    status |= gqa_runs(A, T, a, scale, rng);
    status |= runs16<bf16>("bf16", A, T, a, scale, rng);
    status |= runs16<fp16>("fp16", A, T, a, scale, rng);
    status |= bias_runs<float>("fp32", A, T, a, t, scale, rng);
    status |= bias_runs<bf16>("bf16", A, T, a, t, scale, rng);
    // V = 32: widths above 64 on the wide scratch, with and without a bias, and against the narrow geometries by zero padding
    for (bool with_bias : {true, false}) {
        status |= bias_runs<float>("fp32", A, T, a, t, scale, rng, true, with_bias);
        status |= bias_runs<bf16>("bf16", A, T, a, t, scale, rng, true, with_bias);
    }
    status |= padding_runs(A, T, a, t, scale, rng);
    for (void *p : owned) free(p);
    free(A.plan_attn.d_scratch.p);
    free(T.plan_attn.d_scratch.p);
    free(A.plan_attn.d_scratch_wide.p);
    free(T.plan_attn.d_scratch_wide.p);
    return status != 0 || !(worst <= 2e-5);
}
