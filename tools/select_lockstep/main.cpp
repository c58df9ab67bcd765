// tools/select_lockstep/main.cpp -- csrc/kernels_select.hip executed on the host (hip/hip_runtime.h: a thread per work-item,
// the lanes of a wavefront in lockstep at every ballot and shuffle) against a serial statement of the contract of
// include/spmv_hip.h "selection": row_ptr, col_idx, the bits of vals and the map, bit for bit; then gather and scatter through
// the map.  Every array is an exactly sized heap block.
#include "kernels_select.hip"
#include "kernels_map.hip"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace {

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// the contract, stated apart from the kernels' key code: through float comparisons wherever they decide
bool ranks_before(float a, uint32_t pa, float b, uint32_t pb, bool abs)
{
    if (abs) { a = std::fabs(a); b = std::fabs(b); }
    const bool na = std::isnan(a), nb = std::isnan(b);
    if (na != nb) return nb;              // every number ranks above every NaN
    if (!na && a != b) return a > b;      // (-0 == +0)
    return pa < pb;
}

struct Csr {
    int64_t rows = 0, cols = 0;
    std::vector<int32_t> rp, ci;
    std::vector<float> va;
};

struct Result {
    std::vector<int32_t> rp, ci;
    std::vector<uint32_t> va, map;
};

Result reference(const Csr &a, const std::vector<float> &score, bool thresh, int k, float thr, bool abs)
{
    Result r;
    r.rp.push_back(0);
    for (int64_t row = 0; row < a.rows; ++row) {
        std::vector<uint32_t> pos;
        for (int32_t p = a.rp[row]; p < a.rp[row + 1]; ++p) pos.push_back((uint32_t)p);
        std::vector<uint32_t> kept;
        if (thresh) {
            for (uint32_t p : pos) {
                const float s = abs ? std::fabs(score[p]) : score[p];
                if (s >= thr) kept.push_back(p);
            }
        } else {
            std::vector<uint32_t> ranking = pos;
            std::sort(ranking.begin(), ranking.end(),
                      [&](uint32_t p, uint32_t q) { return ranks_before(score[p], p, score[q], q, abs); });
            if ((int64_t)ranking.size() > k) ranking.resize(k);
            kept = ranking;
            std::sort(kept.begin(), kept.end());
        }
        for (uint32_t p : kept) {
            r.ci.push_back(a.ci[p]);
            r.va.push_back(bits_of(a.va[p]));
            r.map.push_back(p);
        }
        r.rp.push_back((int32_t)r.ci.size());
    }
    return r;
}

template <class T> T *exact_copy(const std::vector<T> &v)
{
    T *p = (T *)malloc(sizeof(T) * (v.size() ? v.size() : 1));
    if (!v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

int g_checked = 0;

void check(const char *what, const Csr &a, const std::vector<float> *score, bool thresh, int k, float thr, bool abs)
{
    int32_t *rp = exact_copy(a.rp), *ci = exact_copy(a.ci);
    float *va = exact_copy(a.va), *sc = score ? exact_copy(*score) : nullptr;
    spmv_csr h;
    h.rows = a.rows; h.cols = a.cols; h.nnz = (int64_t)a.ci.size();
    h.d_row_ptr = rp; h.d_col_idx = ci; h.d_vals = va;
    const Result want = reference(a, score ? *score : a.va, thresh, k, thr, abs);
    for (int keep_map = 0; keep_map < 2; ++keep_map) {
        spmv_csr_t *out = nullptr;
        const int rc = spmv::select(h, sc, thresh, k, spmv::select_key(thr, false), abs, keep_map == 1, nullptr, &out);
        bool ok = rc == 0 && out && out->rows == a.rows && out->nnz == (int64_t)want.ci.size() && out->map.parent_len == h.nnz &&
                  (out->map.words.get() != nullptr) == (keep_map == 1) && (out->map.maker == spmv::MapMaker::select) == (keep_map == 1);
        auto same = [](const void *got, const auto &w) { return w.empty() || std::memcmp(got, w.data(), 4 * w.size()) == 0; };
        ok = ok && same(out->d_row_ptr, want.rp) && same(out->d_col_idx, want.ci) && same(out->d_vals, want.va);
        if (ok && keep_map) ok = same(out->map.words.get(), want.map);
        if (ok && keep_map && out->nnz > 0) {
            // gather three strided arrays, scatter them back into zeros: the identity on the kept positions
            const int64_t n = h.nnz, m = out->nnz, ss = n + 3, ds = m + 2;
            std::vector<uint32_t> src(3 * ss - 3), zero(3 * ss - 3, 0u);
            for (size_t i = 0; i < src.size(); ++i) src[i] = 0x9e3779b9u * (uint32_t)(i + 1);
            uint32_t *d_src = exact_copy(src), *d_back = exact_copy(zero);
            uint32_t *d_mid = (uint32_t *)malloc(4 * (3 * ds - 2));
            ok = spmv::map_move(out->map, out->nnz, false, 3, d_src, ss, d_mid, ds, nullptr) == 0 &&
                 spmv::map_move(out->map, out->nnz, true, 3, d_mid, ds, d_back, ss, nullptr) == 0;
            std::vector<char> is_kept(n, 0);
            for (uint32_t p : want.map) is_kept[p] = 1;
            for (int c = 0; ok && c < 3; ++c)
                for (int64_t p = 0; p < n; ++p) ok = ok && d_back[c * ss + p] == (is_kept[p] ? src[c * ss + p] : 0u);
            free(d_src); free(d_back); free(d_mid);
        }
        if (!ok) {
            std::fprintf(stderr, "MISMATCH %s: thresh %d k %d thr %g abs %d keep_map %d (rc %d, nnz %lld, want %zu)\n", what, (int)thresh, k,
                         (double)thr, (int)abs, keep_map, rc, out ? (long long)out->nnz : -1ll, want.ci.size());
            std::exit(1);
        }
        delete out;
        ++g_checked;
    }
    free(rp); free(ci); free(va); free(sc);
}

Csr make(std::mt19937 &rng, const std::vector<int> &lengths, int64_t cols, bool shuffled)
{
    Csr a;
    a.rows = (int64_t)lengths.size();
    a.cols = cols;
    a.rp.push_back(0);
    for (int n : lengths) {
        std::vector<int32_t> c(n);
        for (int i = 0; i < n; ++i) c[i] = (int32_t)(((int64_t)i * cols) / std::max(n, 1));
        if (shuffled) {
            for (int i = 0; i < n; ++i) if (rng() % 8 == 0) c[i] = c[rng() % n];
            std::shuffle(c.begin(), c.end(), rng);
        }
        a.ci.insert(a.ci.end(), c.begin(), c.end());
        a.rp.push_back((int32_t)a.ci.size());
    }
    std::normal_distribution<float> nd;
    a.va.resize(a.ci.size());
    for (float &v : a.va) v = nd(rng);
    return a;
}

const uint32_t kSpecial[] = {0x7FC00000u, 0x7F800001u, 0xFFC00000u, 0xFFFFFFFFu, 0x7F800000u, 0xFF800000u, 0x00000000u, 0x80000000u,
                             0x00000001u, 0x80000001u, 0x7F7FFFFFu, 0xFF7FFFFFu};

}  // namespace

int main()
{
    std::mt19937 rng(12345);
    const std::vector<int> edge = {0, 1, 2, 63, 64, 65, 127, 128, 511, 512, 513, 1024, 1025, 4097};
    // the lengths mixed, so that wavefronts hold unlike rows, padded with short rows past one workgroup (256 rows) ...
    std::vector<int> mixed;
    for (int rep = 0; rep < 2; ++rep)
        for (int n : edge) { mixed.push_back(n); for (int j = 0; j < 9; ++j) mixed.push_back((int)(rng() % 40)); }
    // ... and sorted, so that they do not: wavefronts of short rows only (groups of 1 .. 64 lanes)
    std::vector<int> sorted_l;
    for (int g = 0; g < 7; ++g) for (int j = 0; j < 64; ++j) sorted_l.push_back((int)(rng() % ((1 << g) + 1)));
    for (int n : edge) sorted_l.push_back(n);

    for (int shuffled = 0; shuffled < 2; ++shuffled) {
        const Csr a = make(rng, mixed, 5000, shuffled == 1);
        for (int k : {1, 2, 63, 64, 65, 512, 513, 4097, 2147483647}) check("mixed normal", a, nullptr, false, k, 0.0f, false);
        const Csr b = make(rng, sorted_l, 5000, shuffled == 1);
        for (int k : {1, 3, 64, 600}) check("sorted normal", b, nullptr, false, k, 0.0f, shuffled == 1);
        check("threshold", a, nullptr, true, 0, 0.3f, false);
        check("threshold abs", b, nullptr, true, 0, 0.3f, true);
    }
    std::printf("row lengths: %d selections\n", g_checked); std::fflush(stdout);
    // ties: all equal, two values, blocks of 64 and of 65
    {
        const Csr a = make(rng, {64, 65, 512, 513, 4097, 7, 0, 300}, 6000, false);
        const size_t nnz = a.ci.size();
        std::vector<std::vector<float>> scores(4, std::vector<float>(nnz));
        for (size_t i = 0; i < nnz; ++i) {
            scores[0][i] = 1.5f;
            scores[1][i] = (rng() & 1) ? 1.0f : -2.0f;
        }
        for (int64_t r = 0; r < a.rows; ++r)
            for (int32_t p = a.rp[r]; p < a.rp[r + 1]; ++p) {
                scores[2][p] = (float)(((p - a.rp[r]) / 64) % 3);
                scores[3][p] = (float)(((p - a.rp[r]) / 65) % 3);
            }
        for (const auto &s : scores)
            for (int k : {1, 32, 33, 63, 64, 256, 257, 511, 512, 2048, 2049, 4096}) check("ties", a, &s, false, k, 0.0f, false);
    }
    std::printf("ties: %d selections\n", g_checked); std::fflush(stdout);
    // keys: the special set, the lowest mantissa bit, the sign; rows of only NaNs; fewer numbers than k
    {
        const Csr a = make(rng, {12, 40, 64, 100, 513, 700, 5, 2000}, 4000, true);
        const size_t nnz = a.ci.size();
        std::vector<float> sp(nnz), lsb(nnz), sign(nnz), nans(nnz);
        for (size_t i = 0; i < nnz; ++i) {
            sp[i] = (rng() % 3) ? float_of(kSpecial[rng() % 12]) : (float)((int)(rng() % 7) - 3);
            lsb[i] = float_of(0x3F800000u + (rng() % 4));
            sign[i] = (rng() & 1) ? 0.75f : -0.75f;
            nans[i] = (rng() % 8) ? float_of(kSpecial[rng() % 4]) : (float)(rng() % 5);
        }
        for (int32_t p = a.rp[3]; p < a.rp[4]; ++p) nans[p] = float_of(kSpecial[p % 4]);      // a row of only NaNs
        for (int abs = 0; abs < 2; ++abs) {
            for (const auto *s : {&sp, &lsb, &sign, &nans})
                for (int k : {1, 4, 37, 64, 300, 600}) check("keys", a, s, false, k, 0.0f, abs == 1);
            for (uint32_t tb : {0xFF800000u, 0x80000000u, 0x00000000u, 0x3F400000u, 0x7F800000u, 0x7F7FFFFFu, 0x00000001u, 0xBF400000u}) {
                check("threshold specials", a, &sp, true, 0, float_of(tb), abs == 1);
                check("threshold sign", a, &sign, true, 0, float_of(tb), abs == 1);
                check("threshold nans", a, &nans, true, 0, float_of(tb), abs == 1);
            }
        }
        Csr own = a;
        own.va = sp;                                                       // d_score = NULL: the matrix's own values
        for (int k : {2, 70}) check("own values", own, nullptr, false, k, 0.0f, true);
    }
    std::printf("keys and thresholds: %d selections\n", g_checked); std::fflush(stdout);
    // edge sizes
    {
        Csr e;
        e.rows = 0; e.cols = 5; e.rp = {0};
        check("rows = 0", e, nullptr, false, 3, 0.0f, false);
        check("rows = 0", e, nullptr, true, 0, 0.0f, false);
        const Csr z = make(rng, std::vector<int>(300, 0), 9, false);
        check("nnz = 0", z, nullptr, false, 1, 0.0f, false);
        check("nnz = 0", z, nullptr, true, 0, 1.0f, false);
        const Csr one = make(rng, {1}, 1, false);
        check("one", one, nullptr, false, 1, 0.0f, false);
        check("nothing kept", one, nullptr, true, 0, float_of(0x7F800000u), true);
    }
    std::printf("select lockstep: %d selections bit for bit\n", g_checked);
    return 0;
}
