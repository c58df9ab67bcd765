// tools/spgemm_lockstep/main.cpp -- csrc/kernels_spgemm.hip executed on the host (hip/hip_runtime.h: a thread per work-item,
// the lanes of a wavefront in lockstep at every ballot, shuffle and wave barrier) against a serial statement of the contract of
// include/spmv_hip.h "the sparse product": row_ptr, col_idx and the bits of vals, bit for bit, from the first call and again
// from the numeric pass alone (spgemm_values on the kept plan, after the operands' values were rewritten).  Every array is an
// exactly sized heap block, the LDS of a launch included.
#include "kernels_spgemm.hip"

#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

namespace {

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Csr {
    int64_t rows = 0, cols = 0;
    std::vector<int32_t> rp{0}, ci;
    std::vector<float> va;
    void add_row(const std::vector<int32_t> &c, const std::vector<float> &v)
    {
        ci.insert(ci.end(), c.begin(), c.end());
        va.insert(va.end(), v.begin(), v.end());
        rp.push_back((int32_t)ci.size());
        ++rows;
    }
};

struct Result {
    std::vector<int32_t> rp, ci;
    std::vector<uint32_t> va;
    int64_t products = 0;
};

// the contract: per row an ordered map column -> chain, fed in ascending (s, q)
Result reference(const Csr &a, const Csr &b)
{
    Result r;
    r.rp.push_back(0);
    for (int64_t i = 0; i < a.rows; ++i) {
        std::map<int32_t, float> acc;
        for (int32_t s = a.rp[i]; s < a.rp[i + 1]; ++s) {
            const int32_t c = a.ci[s];
            for (int32_t q = b.rp[c]; q < b.rp[c + 1]; ++q) {
                auto it = acc.emplace(b.ci[q], 0.0f).first;
                it->second = std::fmaf(a.va[s], b.va[q], it->second);
                ++r.products;
            }
        }
        for (const auto &e : acc) {
            r.ci.push_back(e.first);
            r.va.push_back(bits_of(e.second));
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

struct Device {      // a handle on exactly sized copies of a Csr's arrays
    spmv_csr h;
    int32_t *rp, *ci;
    float *va;
    explicit Device(const Csr &m) : rp(exact_copy(m.rp)), ci(exact_copy(m.ci)), va(exact_copy(m.va))
    {
        h.rows = m.rows; h.cols = m.cols; h.nnz = (int64_t)m.ci.size();
        h.d_row_ptr = rp; h.d_col_idx = ci; h.d_vals = va;
    }
    ~Device() { free(rp); free(ci); free(va); }
};

int g_checked = 0;

bool same(const void *got, const void *want, size_t words) { return words == 0 || std::memcmp(got, want, 4 * words) == 0; }

void fail(const char *what, const char *stage, int rc, const spmv_csr *out, const Result &want)
{
    std::fprintf(stderr, "MISMATCH %s (%s): rc %d, nnz %lld, want %zu\n", what, stage, rc, out ? (long long)out->nnz : -1ll, want.ci.size());
    if (out && out->nnz == (int64_t)want.ci.size())
        for (size_t i = 0; i < want.ci.size(); ++i)
            if (out->d_col_idx[i] != want.ci[i] || bits_of(out->d_vals[i]) != want.va[i]) {
                std::fprintf(stderr, "  first at %zu: col %d want %d, bits %08x want %08x\n", i, out->d_col_idx[i], want.ci[i],
                             bits_of(out->d_vals[i]), want.va[i]);
                break;
            }
    std::exit(1);
}

void check(const char *what, Csr a, Csr b, bool same_handle = false)
{
    std::mt19937 rng(777);
    const Result want = reference(a, b);
    Device da(a), db_(b);
    const spmv_csr &ha = da.h, &hb = same_handle ? da.h : db_.h;
    float *vb = same_handle ? da.va : db_.va;
    for (int keep_plan = 0; keep_plan < 2; ++keep_plan) {
        spmv_csr_t *out = nullptr;
        int64_t products = -1;
        const int rc = spmv::spgemm(ha, hb, keep_plan == 1, nullptr, &out, &products);
        const bool ok = rc == 0 && out && out->rows == a.rows && out->cols == b.cols && out->nnz == (int64_t)want.ci.size() &&
                        products == want.products && out->plan_spgemm.ready == (keep_plan == 1) &&
                        same(out->d_row_ptr, want.rp.data(), want.rp.size()) && same(out->d_col_idx, want.ci.data(), want.ci.size()) &&
                        same(out->d_vals, want.va.data(), want.va.size());
        if (!ok) fail(what, keep_plan ? "keep_plan" : "first call", rc, out, want);
        if (keep_plan) {
            // new values in place, then the numeric pass alone
            for (size_t i = 0; i < a.va.size(); ++i) da.va[i] = a.va[i] = a.va[i] * 0.75f + (float)(int)(rng() % 5) - 2.0f;
            if (!same_handle)
                for (size_t i = 0; i < b.va.size(); ++i) vb[i] = b.va[i] = b.va[i] * 1.25f - (float)(int)(rng() % 3);
            const Result again = reference(a, same_handle ? a : b);
            for (int64_t i = 0; i < out->nnz; ++i) out->own_vals.get()[i] = float_of(0x7fc00123u);
            const int rc2 = spmv::spgemm_values(*out, ha, hb, nullptr);
            if (rc2 != 0 || !same(out->d_vals, again.va.data(), again.va.size()) || spmv::spgemm_plan_bytes(*out) != 4 * out->plan_spgemm.cls[5])
                fail(what, "spgemm_values", rc2, out, again);
        }
        delete out;
        ++g_checked;
    }
}

// values whose sums show their order: exponents spread over 2^20, both signs
float spread(std::mt19937 &rng)
{
    const float m = 1.0f + (float)(rng() % 4096) / 4096.0f;
    return std::ldexp((rng() & 1) ? m : -m, (int)(rng() % 21) - 10);
}

Csr random_csr(std::mt19937 &rng, int64_t rows, int64_t cols, int max_len, bool repeats)
{
    Csr m;
    m.cols = cols;
    for (int64_t r = 0; r < rows; ++r) {
        const int n = cols ? (int)(rng() % (max_len + 1)) : 0;
        std::vector<int32_t> c(n);
        std::vector<float> v(n);
        for (int i = 0; i < n; ++i) {
            c[i] = (int32_t)(rng() % cols);
            if (repeats && i > 0 && rng() % 6 == 0) c[i] = c[rng() % i];
            v[i] = spread(rng);
        }
        m.add_row(c, v);
    }
    return m;
}

// B for the class edges: WIDE rows of 64 columns each (row r: [64 r, 64 r + 64), shuffled), then UNIT rows of one column each
constexpr int kWide = 520, kUnit = 64;
Csr edge_b(std::mt19937 &rng)
{
    Csr b;
    b.cols = 64 * kWide + kUnit;
    for (int r = 0; r < kWide; ++r) {
        std::vector<int32_t> c(64);
        std::vector<float> v(64);
        for (int i = 0; i < 64; ++i) { c[i] = 64 * r + i; v[i] = spread(rng); }
        std::shuffle(c.begin(), c.end(), rng);
        b.add_row(c, v);
    }
    for (int u = 0; u < kUnit; ++u) b.add_row({64 * kWide + u}, {spread(rng)});
    return b;
}

// a row of A over edge_b with `distinct` distinct result columns (distinct / 64 wide rows and distinct % 64 unit rows) and
// `bound` terms: the bound - distinct others repeat wide row 0, 64 at a time, and unit row 0; its entries shuffled
void edge_row(std::mt19937 &rng, Csr &a, int bound, int distinct)
{
    std::vector<int32_t> c;
    for (int r = 0; r < distinct / 64; ++r) c.push_back(r);
    for (int u = 0; u < distinct % 64; ++u) c.push_back(kWide + u);
    int extra = bound - distinct;
    if (distinct >= 64)
        for (; extra >= 64; extra -= 64) c.push_back(0);
    if (extra > 0 && distinct % 64 == 0) { std::fprintf(stderr, "edge_row(%d, %d) cannot be built\n", bound, distinct); std::exit(2); }
    for (; extra > 0; --extra) c.push_back(kWide);
    std::shuffle(c.begin(), c.end(), rng);
    std::vector<float> v(c.size());
    for (float &x : v) x = spread(rng);
    a.add_row(c, v);
}

const uint32_t kSpecial[] = {0x7FC00000u, 0xFFC00001u, 0x7F800000u, 0xFF800000u, 0x00000000u, 0x80000000u, 0x00000001u,
                             0x80000001u, 0x007FFFFFu, 0x7F7FFFFFu, 0x3F800000u, 0xBF800000u};

}  // namespace

int main()
{
    std::mt19937 rng(4242);
    // generic: unsorted rows of 0 .. 40 entries with repeated columns on both sides
    {
        const Csr a = random_csr(rng, 257, 193, 40, true), b = random_csr(rng, 193, 300, 40, true);
        check("generic", a, b);
        Csr block;                       // rows 100 .. 163 of a: the same rows of the product (checked against the same contract)
        block.cols = a.cols;
        for (int r = 100; r < 164; ++r)
            block.add_row(std::vector<int32_t>(a.ci.begin() + a.rp[r], a.ci.begin() + a.rp[r + 1]),
                          std::vector<float>(a.va.begin() + a.rp[r], a.va.begin() + a.rp[r + 1]));
        check("row block", block, b);
        const Csr sq = random_csr(rng, 150, 150, 12, true);
        check("a == b", sq, sq, true);
    }
    std::printf("generic: %d products\n", g_checked); std::fflush(stdout);
    // class edges: terms T - 1, T, T + 1 and distinct columns T - 1, T, T + 1 around every class, a full table, short and empty
    // neighbours
    {
        const Csr b = edge_b(rng);
        const int slots[] = {SPMV_SPGEMM_CLASS_SLOTS};
        for (int T : slots) {
            Csr a;
            a.cols = b.rows;
            a.add_row({}, {});
            edge_row(rng, a, 3, 3);
            for (int d = -1; d <= 1; ++d) {
                edge_row(rng, a, T + d, T + d);                              // terms = distinct = T - 1, T (a full table), T + 1
                a.add_row({}, {});
                edge_row(rng, a, T + d, T > 64 ? T + d - 64 : T + d - 3);     // terms at the edge, fewer distinct
                edge_row(rng, a, T + d + 64, T + d);                          // distinct at the edge, terms beyond it
                edge_row(rng, a, 2, 2);
            }
            a.add_row({}, {});
            check("class edges", a, b);
        }
    }
    std::printf("class edges: %d products\n", g_checked); std::fflush(stdout);
    // one column: every term of a row of 600 entries lands on one entry; then B's rows repeat column 0 three times
    for (int rep : {1, 3}) {
        Csr b, a;
        b.cols = 1;
        for (int r = 0; r < 50; ++r) {
            std::vector<float> v(rep);
            for (float &x : v) x = spread(rng);
            b.add_row(std::vector<int32_t>(rep, 0), v);
        }
        a.cols = b.rows;
        for (int n : {2, 600, 0, 65}) {
            std::vector<int32_t> c(n);
            std::vector<float> v(n);
            for (int i = 0; i < n; ++i) { c[i] = (int32_t)(rng() % 50); v[i] = spread(rng); }
            a.add_row(c, v);
        }
        check("one column", a, b);
    }
    // oversized: 700 entries over rows of 64 distinct columns (44 800 distinct); then oversized terms, few distinct columns
    {
        Csr b;
        b.cols = 64 * 700 + 5;
        for (int r = 0; r < 700; ++r) {
            std::vector<int32_t> c(64);
            std::vector<float> v(64);
            for (int i = 0; i < 64; ++i) { c[i] = 64 * r + i; v[i] = spread(rng); }
            std::shuffle(c.begin(), c.end(), rng);
            b.add_row(c, v);
        }
        Csr a;
        a.cols = b.rows;
        a.add_row({3, 1}, {1.5f, -2.0f});
        std::vector<int32_t> c(700);
        std::vector<float> v(700);
        for (int i = 0; i < 700; ++i) { c[i] = i; v[i] = spread(rng); }
        std::shuffle(c.begin(), c.end(), rng);
        a.add_row(c, v);
        a.add_row({}, {});
        for (int i = 0; i < 700; ++i) c[i] = (int32_t)(rng() % 3);           // 44 800 terms on 192 columns
        a.add_row(c, v);
        a.add_row({699}, {0.5f});
        check("oversized", a, b);
    }
    std::printf("one column and oversized: %d products\n", g_checked); std::fflush(stdout);
    // the edges of the types and the degenerate sizes
    {
        Csr a, b;
        b.cols = 2147483647;
        b.add_row({2147483646, 0, 2147483646, 5}, {1.0f, 2.0f, 3.0f, 4.0f});
        b.add_row({2147483645}, {-1.0f});
        a.cols = 2;
        a.add_row({1, 0, 0}, {2.0f, 3.0f, 5.0f});
        check("2^31 - 1 columns", a, b);
        Csr e0;                                                          // m = 0
        e0.cols = 2;
        check("m = 0", e0, b);
        Csr an, bn;                                                      // n = 0
        an.cols = 0; an.add_row({}, {}); an.add_row({}, {});
        bn.cols = 7;
        check("n = 0", an, bn);
        Csr bp;                                                          // p = 0
        bp.cols = 0; bp.add_row({}, {}); bp.add_row({}, {});
        check("p = 0", a, bp);
        Csr az;                                                          // nnz = 0 on either side
        az.cols = 2;
        for (int i = 0; i < 300; ++i) az.add_row({}, {});
        check("a without nonzeros", az, b);
        Csr bz;
        bz.cols = 9; bz.add_row({}, {}); bz.add_row({}, {});
        check("b without nonzeros", a, bz);
    }
    // values: the special set on both sides, and a pair of terms that cancels
    {
        Csr b = random_csr(rng, 40, 30, 12, true), a = random_csr(rng, 70, 40, 20, true);
        for (float &x : a.va) if (rng() % 3 == 0) x = float_of(kSpecial[rng() % 12]);
        for (float &x : b.va) if (rng() % 3 == 0) x = float_of(kSpecial[rng() % 12]);
        a.add_row({0, 0}, {1.0f, -1.0f});
        check("special values", a, b);
    }
    std::printf("spgemm lockstep: %d products bit for bit\n", g_checked);
    return 0;
}
