// tools/softmax_lockstep/main.cpp -- see run.sh.  Layouts: 0 rows of every length class (0 .. 5000) among short rows, rows
// of 33 .. 64 and rows up to 89, the row count no multiple of 64; 1 one row of 120 000; 2 a long row before empty rows;
// 3 thousands of empty rows; 4 rows of one entry.
#include "kernels_softmax.hip"
#include <algorithm>
#include <cstdlib>
#include <random>
using namespace spmv;

static float ordered_sum(const float *x, int n)
{
    float acc = 0.0f;
    const int pieces = (n + 511) / 512;
    for (int p = 0; p < pieces; ++p) {
        const float *px = x + p * 512;
        const int len = std::min(512, n - p * 512);
        float q[64], t[64];
        for (int l = 0; l < 64; ++l) {
            q[l] = 0.0f;
            for (int i = l; i < len; i += 64) q[l] = q[l] + px[i];
        }
        for (int m = 32; m >= 1; m /= 2) {
            for (int l = 0; l < 64; ++l) t[l] = q[l] + q[l ^ m];
            std::copy(t, t + 64, q);
        }
        if (pieces == 1) return q[0];
        acc = acc + q[0];
    }
    return acc;
}

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0 || (std::isnan(a) && std::isnan(b)); }

int main(int argc, char **argv)
{
    const int mode = argc > 1 ? atoi(argv[1]) : 0;
    std::mt19937 rng(7);
    std::vector<int> lens;
    const int special[] = {0, 1, 2, 3, 5, 17, 31, 32, 33, 63, 64, 65, 129, 300, 511, 512, 513, 1024, 1025, 2000, 5000};
    for (int rep = 0; rep < 3; ++rep)
        for (int s : special) {
            for (int i = 0; i < 37; ++i) lens.push_back(rep == 0 ? rng() % 5 : rep == 1 ? 33 + rng() % 32 : rng() % 90);
            lens.push_back(s);
        }
    for (int i = 0; i < 300; ++i) lens.push_back(rng() % 3);
    if (mode == 1) lens = {120000};
    if (mode == 2) lens = {4096, 0, 0, 0, 17};
    if (mode == 3) { lens.assign(5000, 0); lens[4999] = 7; lens[0] = 5; }
    if (mode == 4) lens.assign(700, 1);
    const int64_t rows = (int64_t)lens.size();
    std::vector<int32_t> rp(rows + 1, 0), lr, lf, k0, ln;
    for (int64_t r = 0; r < rows; ++r) rp[r + 1] = rp[r] + lens[r];
    const int64_t nnz = rp[rows];
    for (int64_t r = 0; r < rows; ++r) {          // the plan of plan_spmm: rows of more than 512 in pieces of 512
        if (lens[r] <= 512) continue;
        lr.push_back((int32_t)r);
        lf.push_back((int32_t)k0.size());
        for (int q = rp[r]; q < rp[r + 1]; q += 512) { k0.push_back(q); ln.push_back(std::min(512, rp[r + 1] - q)); }
    }
    lf.push_back((int32_t)k0.size());
    // exactly sized heap blocks, so that AddressSanitizer sees one float too far
    auto heap = [](auto &v) { auto *p = (typename std::remove_reference_t<decltype(v)>::value_type *)malloc(sizeof(v[0]) * v.size() + 1); std::copy(v.begin(), v.end(), p); return p; };
    spmv_csr h;
    h.rows = rows, h.cols = 10, h.nnz = nnz;
    int32_t *d_rp = heap(rp);
    h.d_row_ptr = d_rp;
    SpmmPlan &pl = h.plan_spmm;
    pl.n_long = (int)lr.size(), pl.pieces = (int)k0.size();
    pl.d_long_row.p = heap(lr), pl.d_long_first.p = heap(lf), pl.d_piece_k0.p = heap(k0), pl.d_piece_len.p = heap(ln);
    pl.d_partial.p = (float *)malloc(sizeof(float) * 64 * k0.size() + 1);
    auto floats = [&] { return (float *)malloc(4 * nnz + 1); };
    float *x = floats(), *out = floats(), *inpl = floats();
    std::normal_distribution<float> nd(0.f, 3.f);
    for (int64_t i = 0; i < nnz; ++i) {
        x[i] = rng() % 11 == 0 ? -INFINITY : nd(rng);
        out[i] = NAN, inpl[i] = x[i];
    }
    const float scale = 0.7f;
    int rc = launch_row_softmax(h, scale, x, out, nullptr) | launch_row_softmax(h, scale, inpl, inpl, nullptr);
    int64_t bad = 0;
    std::vector<float> e;
    for (int64_t r = 0; r < rows; ++r) {
        const int L = lens[r];
        if (!L) continue;
        e.assign(L, 0.f);
        float M = -INFINITY;
        for (int i = 0; i < L; ++i) M = fmaxf(M, scale * x[rp[r] + i]);
        for (int i = 0; i < L; ++i) e[i] = expf(scale * x[rp[r] + i] - M);
        const float rinv = 1.0f / ordered_sum(e.data(), L);
        for (int i = 0; i < L; ++i) bad += !same(e[i] * rinv, out[rp[r] + i]) + !same(out[rp[r] + i], inpl[rp[r] + i]);
    }
    printf("layout %d: rows %lld nnz %lld long rows %zu pieces %zu; forward status %d, %lld mismatches\n", mode, (long long)rows,
           (long long)nnz, lr.size(), k0.size(), rc, (long long)bad);
    float *P = floats(), *dP = floats(), *dS = floats(), *overP = floats(), *overdP = floats();
    for (int64_t i = 0; i < nnz; ++i) {
        P[i] = overP[i] = (float)((int)(rng() % 9) - 4);
        dP[i] = overdP[i] = (float)((int)(rng() % 9) - 4);
        dS[i] = NAN;
    }
    int rcb = launch_row_softmax_backward(h, -2.0f, P, dP, dS, nullptr) | launch_row_softmax_backward(h, -2.0f, overP, dP, overP, nullptr) |
              launch_row_softmax_backward(h, -2.0f, P, overdP, overdP, nullptr);
    int64_t badb = 0;
    for (int64_t r = 0; r < rows; ++r) {
        long long dot = 0;
        for (int i = rp[r]; i < rp[r + 1]; ++i) dot += (long long)P[i] * (long long)dP[i];
        for (int i = rp[r]; i < rp[r + 1]; ++i) {
            const float w = -2.0f * (float)((long long)P[i] * ((long long)dP[i] - dot));
            badb += !(w == dS[i] && w == overP[i] && w == overdP[i]);
        }
    }
    printf("layout %d: backward status %d, %lld mismatches\n", mode, rcb, (long long)badb);
    for (void *p : {(void *)x, (void *)out, (void *)inpl, (void *)P, (void *)dP, (void *)dS, (void *)overP, (void *)overdP, (void *)d_rp,
                    (void *)pl.d_long_row.p, (void *)pl.d_long_first.p, (void *)pl.d_piece_k0.p, (void *)pl.d_piece_len.p, (void *)pl.d_partial.p})
        free(p);
    return (rc | rcb) != 0 || bad != 0 || badb != 0;
}
