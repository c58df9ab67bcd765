// tools/color_lockstep/main.cpp -- csrc/kernels_color.hip and csrc/kernels_permute.hip executed on the host
// (hip/hip_runtime.h of tools/trsv_lockstep: a thread per work-item, real barriers) against a serial statement of the contract
// of include/spmv_hip.h "the multicolour ordering": color, perm, color_ptr and the counts of spmv_csr_color under two seeds;
// row_ptr, col_idx, the bits of vals and the map of spmv_csr_permute through both routes, the companions and
// spmv_permute_vector.  Every array is an exactly sized heap block.
#include "kernels_color.hip"
#include "kernels_permute.hip"
#include "kernels_map.hip"

#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

namespace {

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Csr {
    int64_t n = 0, cols = 0;
    std::vector<int32_t> rp{0}, ci;
    std::vector<float> va;
    void add_row(const std::vector<int32_t> &c)
    {
        for (int32_t j : c) { ci.push_back(j); va.push_back(float_of(0x3f800000u + (uint32_t)ci.size() * 7u)); }
        rp.push_back((int32_t)ci.size());
        ++n;
    }
};

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
        h.rows = m.n; h.cols = m.cols ? m.cols : m.n; h.nnz = (int64_t)m.ci.size();
        h.d_row_ptr = rp; h.d_col_idx = ci; h.d_vals = va;
    }
    ~Device() { free(rp); free(ci); free(va); }
};

[[noreturn]] void fail(const char *what, const char *stage, long extra = 0)
{
    std::fprintf(stderr, "MISMATCH %s (%s) %ld\n", what, stage, extra);
    std::exit(1);
}

uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// ---- the colouring, serially: the rows in descending key order ---------------------------------------------------------------
struct Coloring { std::vector<int32_t> color, perm, color_ptr; int64_t colors = 0, rounds = 0, largest = 0, smallest = 0; };

Coloring color_reference(const Csr &a, uint32_t seed)
{
    const int64_t n = a.n;
    std::vector<std::set<int32_t>> nb((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t s = a.rp[i]; s < a.rp[i + 1]; ++s) {
            const int32_t j = a.ci[s];
            if (j != i) { nb[i].insert(j); nb[j].insert((int32_t)i); }
        }
    std::vector<int32_t> by_key((size_t)n);
    std::iota(by_key.begin(), by_key.end(), 0);
    std::sort(by_key.begin(), by_key.end(), [&](int32_t x, int32_t y) { return fmix32((uint32_t)x ^ seed) > fmix32((uint32_t)y ^ seed); });
    Coloring c;
    c.color.assign((size_t)n, -1);
    std::vector<int64_t> round((size_t)n, 0);
    for (int32_t i : by_key) {
        std::set<int32_t> used;
        int64_t r = 0;
        for (int32_t j : nb[i])
            if (c.color[j] >= 0) { used.insert(c.color[j]); r = std::max(r, round[j]); }
        int32_t k = 0;
        while (used.count(k)) ++k;
        c.color[i] = k;
        round[i] = r + 1;
        c.rounds = std::max(c.rounds, round[i]);
        c.colors = std::max<int64_t>(c.colors, k + 1);
    }
    c.color_ptr.assign((size_t)c.colors + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++c.color_ptr[c.color[i] + 1];
    for (int64_t k = 0; k < c.colors; ++k) c.color_ptr[k + 1] += c.color_ptr[k];
    c.perm.resize((size_t)n);
    std::vector<int32_t> at(c.color_ptr.begin(), c.color_ptr.end());
    for (int64_t i = 0; i < n; ++i) c.perm[at[c.color[i]]++] = (int32_t)i;
    c.smallest = n > 0 ? n : 0;
    for (int64_t k = 0; k < c.colors; ++k) {
        const int64_t m = c.color_ptr[k + 1] - c.color_ptr[k];
        c.largest = std::max(c.largest, m);
        c.smallest = std::min(c.smallest, m);
    }
    return c;
}

int g_colorings = 0, g_permutes = 0;

Coloring check_color(const char *what, const Csr &a)
{
    Coloring last;
    for (uint32_t seed : {0u, 0x9e3779b9u}) {
        const Coloring want = color_reference(a, seed);
        Device d(a);
        std::vector<int32_t> poison((size_t)a.n, -77);
        int32_t *color = exact_copy(poison), *perm = exact_copy(poison);
        std::vector<int32_t> cp((size_t)want.colors + 1, -5);
        int64_t info[8];
        if (spmv::color(d.h, seed, nullptr, color, perm, cp.data(), (int)cp.size(), info) != SPMV_OK) fail(what, "refused", seed);
        if (a.n && std::memcmp(color, want.color.data(), 4 * (size_t)a.n) != 0) fail(what, "color", seed);
        if (a.n && std::memcmp(perm, want.perm.data(), 4 * (size_t)a.n) != 0) fail(what, "perm", seed);
        if (cp != want.color_ptr) fail(what, "color_ptr", seed);
        if (info[0] != want.colors) fail(what, "colours", info[0]);
        if (info[1] != want.rounds) fail(what, "rounds", info[1]);
        if (info[3] != want.largest || info[4] != want.smallest) fail(what, "classes", info[3]);
        free(color); free(perm);
        ++g_colorings;
        last = want;
    }
    return last;
}

// ---- the permutation, serially -----------------------------------------------------------------------------------------------
struct Permuted { std::vector<int32_t> rp{0}, ci; std::vector<uint32_t> va, map; };

Permuted permute_reference(const Csr &a, const std::vector<int32_t> *rowp, const std::vector<int32_t> *colp)
{
    const int64_t cols = a.cols ? a.cols : a.n;
    std::vector<int32_t> inv((size_t)cols);
    for (int64_t c = 0; c < cols; ++c) inv[colp ? (*colp)[c] : c] = (int32_t)c;
    Permuted b;
    for (int64_t r = 0; r < a.n; ++r) {
        const int64_t old = rowp ? (*rowp)[r] : r;
        std::vector<std::pair<int32_t, int32_t>> e;
        for (int32_t s = a.rp[old]; s < a.rp[old + 1]; ++s) e.push_back({inv[a.ci[s]], s});
        std::sort(e.begin(), e.end());
        for (auto &x : e) { b.ci.push_back(x.first); b.va.push_back(bits_of(a.va[x.second])); b.map.push_back((uint32_t)x.second); }
        b.rp.push_back((int32_t)b.ci.size());
    }
    return b;
}

void compare_permuted(const char *what, const char *stage, const spmv_csr &b, const Permuted &want, bool keep_map)
{
    if (std::memcmp(b.d_row_ptr, want.rp.data(), 4 * want.rp.size()) != 0) fail(what, stage, 1);
    if (!want.ci.empty() && std::memcmp(b.d_col_idx, want.ci.data(), 4 * want.ci.size()) != 0) fail(what, stage, 2);
    if (!want.ci.empty() && std::memcmp(b.d_vals, want.va.data(), 4 * want.va.size()) != 0) fail(what, stage, 3);
    if (keep_map != (bool)b.map.words || b.map.maker != (keep_map ? spmv::MapMaker::permute : spmv::MapMaker::none)) fail(what, stage, 4);
    if (keep_map && !want.ci.empty() && std::memcmp(b.map.words.get(), want.map.data(), 4 * want.map.size()) != 0) fail(what, stage, 5);
}

std::vector<int32_t> shuffled(int64_t n, uint32_t seed)
{
    std::vector<int32_t> p((size_t)n);
    std::iota(p.begin(), p.end(), 0);
    std::mt19937 rng(seed);
    std::shuffle(p.begin(), p.end(), rng);
    return p;
}

void check_permute(const char *what, const Csr &a)
{
    const int64_t cols = a.cols ? a.cols : a.n;
    const std::vector<int32_t> rowp = shuffled(a.n, 11), colp = shuffled(cols, 12);
    bool longer_than_4096 = false;
    for (int64_t i = 0; i < a.n; ++i) longer_than_4096 = longer_than_4096 || a.rp[i + 1] - a.rp[i] > 4096;
    for (int mode = 0; mode < 4; ++mode) {
        const std::vector<int32_t> *rp = (mode & 1) ? &rowp : nullptr, *cp = (mode & 2) ? &colp : nullptr;
        const Permuted want = permute_reference(a, rp, cp);
        int32_t *d_rp = rp ? exact_copy(*rp) : nullptr, *d_cp = cp ? exact_copy(*cp) : nullptr;
        long count[2][2] = {};
        for (int via = 0; via < 2; ++via)
            for (int keep = 0; keep < 2; ++keep) {
                Device d(a);
                spmv_csr_t *b = nullptr;
                const long before = emu_launches;
                if (spmv::permute(d.h, d_rp, d_cp, keep, via, nullptr, &b) != SPMV_OK || !b) fail(what, "refused", mode);
                count[via][keep] = emu_launches - before;
                compare_permuted(what, via ? "via transpose" : "direct", *b, want, keep);
                if (keep) {
                    // the companions: the values again after a rewrite, and two arrays at once
                    for (int64_t k = 0; k < d.h.nnz; ++k) d.va[k] = float_of(0x7fc00001u + (uint32_t)k);
                    if (spmv::map_move(b->map, b->nnz, false, 1, d.va, 0, b->own_vals.get(), 0, nullptr) != SPMV_OK) fail(what, "values", mode);
                    for (int64_t k = 0; k < d.h.nnz; ++k)
                        if (bits_of(b->d_vals[k]) != 0x7fc00001u + want.map[k]) fail(what, "values", k);
                    std::vector<uint32_t> src(2 * (size_t)d.h.nnz + 1), dst(2 * (size_t)d.h.nnz + 1, 0xdeadbeefu);
                    for (size_t k = 0; k < src.size(); ++k) src[k] = (uint32_t)(k * 3 + 1);
                    uint32_t *ds = exact_copy(src), *dd = exact_copy(dst);
                    if (spmv::map_move(b->map, b->nnz, false, 2, ds, d.h.nnz, dd, d.h.nnz, nullptr) != SPMV_OK) fail(what, "gather", mode);
                    for (int c = 0; c < 2; ++c)
                        for (int64_t k = 0; k < d.h.nnz; ++k)
                            if (dd[c * d.h.nnz + k] != src[c * d.h.nnz + want.map[k]]) fail(what, "gather", k);
                    if (dd[2 * d.h.nnz] != 0xdeadbeefu) fail(what, "gather wrote past its arrays");
                    free(ds); free(dd);
                }
                spmv_csr_destroy(b);
                ++g_permutes;
            }
        // a call with a row above 4096 entries took the route via the transpose: its launches are the forced call's and the one
        // that gathered the row lengths
        for (int keep = 0; keep < 2; ++keep)
            if (longer_than_4096 && count[0][keep] != count[1][keep] + 1) fail(what, "a long row did not switch the route", count[0][keep]);
        free(d_rp); free(d_cp);
    }
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------
Csr generic(uint32_t seed, bool sorted)
{
    std::mt19937 rng(seed);
    const int n = 257;
    Csr a;
    for (int i = 0; i < n; ++i) {
        const int k = i % 16 == 8 ? 70 + (int)(rng() % 51) : (int)(rng() % 25);
        std::vector<int32_t> c;
        for (int t = 0; t < k; ++t) c.push_back((int32_t)(rng() % n));
        if (sorted) {
            c.push_back(i);
            std::sort(c.begin(), c.end());
            c.erase(std::unique(c.begin(), c.end()), c.end());
        }
        a.add_row(c);
    }
    return a;
}

Csr tridiagonal(int n)
{
    Csr a;
    for (int i = 0; i < n; ++i) {
        std::vector<int32_t> c;
        if (i > 0) c.push_back(i - 1);
        c.push_back(i);
        if (i + 1 < n) c.push_back(i + 1);
        a.add_row(c);
    }
    return a;
}

Csr stencil7(int m)
{
    Csr a;
    for (int z = 0; z < m; ++z)
        for (int y = 0; y < m; ++y)
            for (int x = 0; x < m; ++x) {
                std::vector<int32_t> c;
                const int i = (z * m + y) * m + x;
                if (z > 0) c.push_back(i - m * m);
                if (y > 0) c.push_back(i - m);
                if (x > 0) c.push_back(i - 1);
                c.push_back(i);
                if (x + 1 < m) c.push_back(i + 1);
                if (y + 1 < m) c.push_back(i + m);
                if (z + 1 < m) c.push_back(i + m * m);
                a.add_row(c);
            }
    return a;
}

Csr clique(int n)
{
    Csr a;
    for (int i = 0; i < n; ++i) {
        std::vector<int32_t> c;
        for (int j = 0; j < n; ++j) c.push_back(j);
        a.add_row(c);
    }
    return a;
}

Csr star(int leaves, bool both)
{
    Csr a;
    std::vector<int32_t> c{0};
    for (int j = 1; j <= leaves; ++j) c.push_back(j);
    a.add_row(c);
    for (int j = 1; j <= leaves; ++j) a.add_row(both ? std::vector<int32_t>{0, j} : std::vector<int32_t>{j});
    return a;
}

Csr fan(int heads, int fans)
{
    std::mt19937 rng(13);
    Csr a;
    const int n = heads + fans;
    for (int i = 0; i < n; ++i) {
        std::set<int32_t> c{i};
        if (i < heads) for (int t = 0; t < 3; ++t) c.insert(heads + (int)(rng() % fans));
        else for (int t = 0, k = 1 + (int)(rng() % heads); t < k; ++t) c.insert((int)(rng() % heads));
        a.add_row(std::vector<int32_t>(c.begin(), c.end()));
    }
    return a;
}

Csr arrow(int n)
{
    Csr a;
    for (int i = 0; i + 1 < n; ++i) a.add_row({i, n - 1});
    std::vector<int32_t> c;
    for (int j = 0; j < n; ++j) c.push_back(j);
    a.add_row(c);
    return a;
}

// row 0 .. 2 hold exactly 31, 32 and 33 neighbour entries, a's and its transpose's counted together: half of them stored in the
// row, the others in the rows they point to (strictly upper-triangular beyond: found through the transpose only)
Csr boundary()
{
    const int n = 200;
    std::vector<std::vector<int32_t>> rows((size_t)n);
    int next = 3;
    for (int i = 0; i < 3; ++i) {
        const int want = 31 + i, own = want / 2;
        for (int t = 0; t < own; ++t) rows[i].push_back(next++);
        for (int t = own; t < want; ++t) rows[next++].push_back(i);
    }
    Csr a;
    for (auto &r : rows) a.add_row(r);
    return a;
}

Csr upper(int n)
{
    std::mt19937 rng(21);
    Csr a;
    for (int i = 0; i < n; ++i) {
        std::vector<int32_t> c;
        for (int t = 0; t < 4 && i + 1 < n; ++t) c.push_back(i + 1 + (int)(rng() % (n - i - 1)));
        a.add_row(c);
    }
    return a;
}

Csr lengths(const std::vector<int> &lens, int cols, int pad_rows)
{
    std::mt19937 rng(31);
    Csr a;
    a.cols = cols;
    for (int len : lens) {
        std::vector<int32_t> c;
        for (int t = 0; t < len; ++t) c.push_back((int32_t)(rng() % cols));      // unsorted, with repeats
        a.add_row(c);
    }
    for (int i = 0; i < pad_rows; ++i) a.add_row({(int32_t)(rng() % cols)});
    return a;
}

// operands that were never validated, handed to the calls and straight to the direct route's kernels: any result or refusal,
// no access outside the arrays, every loop ends
void unvalidated()
{
    spmv::g_quiet = true;
    Csr base = generic(5, false);
    for (int kind = 0; kind < 3; ++kind) {
        Csr a = base;
        if (kind == 0) std::reverse(a.rp.begin(), a.rp.end());                       // a descending row_ptr
        if (kind == 1) for (size_t k = 0; k < a.ci.size(); k += 3) a.ci[k] = (k % 2) ? -7 : 100000;      // columns out of range
        if (kind == 2) for (auto &v : a.rp) v += 1000;                               // a row_ptr beyond nnz
        Device d(a);
        std::vector<int32_t> out((size_t)a.n, -1);
        int32_t *color = exact_copy(out), *perm = exact_copy(out);
        int64_t info[8];
        (void)spmv::color(d.h, 3u, nullptr, color, perm, nullptr, 0, info);
        free(color); free(perm);
        const std::vector<int32_t> rowp = shuffled(a.n, 3), colp = shuffled(a.n, 4);
        int32_t *d_rp = exact_copy(rowp), *d_cp = exact_copy(colp);
        for (int via = 0; via < 2; ++via) {
            spmv_csr_t *b = nullptr;
            if (spmv::permute(d.h, d_rp, d_cp, true, via, nullptr, &b) == SPMV_OK && b) spmv_csr_destroy(b);
        }
        free(d_rp); free(d_cp);
    }
    // a perm with repeats and an inverse with entries out of range, straight to the kernels (equal row lengths keep nnz)
    {
        Csr a = tridiagonal(300);
        Device d(a);
        std::vector<int32_t> rowp = shuffled(a.n, 5), icol = shuffled(a.n, 6);
        for (auto &v : rowp) if (v == 0 || v == 299) v = 7;
        rowp[5] = rowp[6] = 100; rowp[17] = 101;
        icol[3] = -1; icol[4] = 300; icol[9] = icol[10];
        int32_t *d_rp = exact_copy(rowp), *d_ic = exact_copy(icol);
        spmv_csr_t *b = nullptr;
        int64_t longest = 0;
        if (spmv::permute_direct(d.h, d_rp, d_ic, true, nullptr, &b, &longest) == SPMV_OK && b) spmv_csr_destroy(b);
        // and one with an entry out of range: the lengths no longer add up, a refusal
        rowp[0] = -3;
        free(d_rp);
        d_rp = exact_copy(rowp);
        b = nullptr;
        if (spmv::permute_direct(d.h, d_rp, d_ic, true, nullptr, &b, &longest) == SPMV_OK && b) spmv_csr_destroy(b);
        // the same long row twice through the bitonic kernel
        Csr l = lengths({4096, 4096, 100}, 5000, 0);
        Device dl(l);
        std::vector<int32_t> twice{0, 0, 2};
        int32_t *d_tw = exact_copy(twice);
        b = nullptr;
        if (spmv::permute_direct(dl.h, d_tw, nullptr, true, nullptr, &b, &longest) == SPMV_OK && b) spmv_csr_destroy(b);
        std::vector<float> src((size_t)a.n, 1.0f), dst((size_t)a.n, 0.0f);
        float *ds = exact_copy(src), *dd = exact_copy(dst);
        (void)spmv::permute_vector(d_rp, a.n, false, ds, dd, nullptr);
        (void)spmv::permute_vector(d_rp, a.n, true, ds, dd, nullptr);
        free(ds); free(dd); free(d_rp); free(d_ic); free(d_tw);
    }
    spmv::g_quiet = false;
}

void refusals()
{
    spmv::g_quiet = true;
    Csr a = tridiagonal(40);
    Device d(a);
    for (int kind = 0; kind < 3; ++kind) {
        std::vector<int32_t> p = shuffled(a.n, 9);
        int want = 0;
        if (kind == 0) { p[5] = p[2]; want = 5; }
        if (kind == 1) { p[0] = -1; want = 0; }
        if (kind == 2) { p[0] = (int32_t)a.n; want = 0; }
        int32_t *dp = exact_copy(p);
        for (int side = 0; side < 2; ++side) {
            spmv_csr_t *b = (spmv_csr_t *)0x1;
            if (spmv::permute(d.h, side ? nullptr : dp, side ? dp : nullptr, false, false, nullptr, &b) != SPMV_ERR_INVALID || b != (spmv_csr_t *)0x1)
                fail("refusals", "a bad permutation passed", kind);
            char expect[64];
            std::snprintf(expect, sizeof expect, "index %d ", want);
            if (!std::strstr(spmv::g_last, expect) || !std::strstr(spmv::g_last, side ? "d_col_perm" : "d_row_perm")) fail("refusals", spmv::g_last, kind);
        }
        free(dp);
    }
    spmv::g_quiet = false;
}

void vectors()
{
    const int64_t n = 1000;
    const std::vector<int32_t> p = shuffled(n, 77);
    std::vector<float> src((size_t)n);
    for (int64_t i = 0; i < n; ++i) src[i] = float_of(0x7fc00000u + (uint32_t)i);
    int32_t *dp = exact_copy(p);
    float *ds = exact_copy(src), *dm = exact_copy(src), *dd = exact_copy(src);
    if (spmv::permute_vector(dp, n, false, ds, dm, nullptr) != SPMV_OK) fail("vectors", "forward");
    for (int64_t r = 0; r < n; ++r) if (bits_of(dm[r]) != bits_of(src[p[r]])) fail("vectors", "forward", r);
    std::memset(dd, 0, 4 * (size_t)n);
    if (spmv::permute_vector(dp, n, true, dm, dd, nullptr) != SPMV_OK) fail("vectors", "backward");
    for (int64_t r = 0; r < n; ++r) if (bits_of(dd[r]) != bits_of(src[r])) fail("vectors", "round trip", r);
    free(dp); free(ds); free(dm); free(dd);
}

}  // namespace

int main()
{
    check_color("generic, unsorted with repeats", generic(1, false));
    const Csr g = generic(2, true);
    const Coloring cg = check_color("generic, sorted", g);
    check_color("tridiagonal", tridiagonal(3000));
    check_color("stencil7(8)", stencil7(8));
    check_color("fan", fan(10, 5000));
    check_color("arrow", arrow(300));
    const Coloring cq = check_color("70-clique", clique(70));
    if (cq.colors != 70 || cq.rounds != 70) fail("70-clique", "70 colours in 70 rounds", cq.colors);
    check_color("130-clique", clique(130));
    const Coloring cs = check_color("star of 5000 leaves", star(5000, true));
    if (cs.colors != 2) fail("star", "two colours", cs.colors);
    check_color("star stored in its centre only", star(5000, false));
    check_color("31, 32 and 33 neighbour entries", boundary());
    check_color("strictly upper-triangular", upper(300));
    {
        Csr dg;
        for (int i = 0; i < 500; ++i) dg.add_row({i});
        const Coloring c = check_color("diagonal", dg);
        if (c.colors != 1 || c.rounds != 1) fail("diagonal", "one colour, one round");
        Csr empty;
        for (int i = 0; i < 300; ++i) empty.add_row({});
        const Coloring e = check_color("nnz = 0", empty);
        if (e.colors != 1 || e.rounds != 1) fail("nnz = 0", "one colour, one round");
        check_color("rows = 0", Csr());
        Csr one;
        one.add_row({0});
        check_color("rows = 1", one);
    }
    // P A P^T of the sorted generic case by its colouring: no stored entry joins two rows of a colour
    {
        Device d(g);
        int32_t *perm = exact_copy(cg.perm);
        spmv_csr_t *b = nullptr;
        if (spmv::permute(d.h, perm, perm, false, false, nullptr, &b) != SPMV_OK) fail("P A P^T", "refused");
        for (int64_t c = 0; c < cg.colors; ++c)
            for (int32_t r = cg.color_ptr[c]; r < cg.color_ptr[c + 1]; ++r)
                for (int32_t s = b->d_row_ptr[r]; s < b->d_row_ptr[r + 1]; ++s)
                    if (b->d_col_idx[s] != r && b->d_col_idx[s] >= cg.color_ptr[c] && b->d_col_idx[s] < cg.color_ptr[c + 1]) fail("P A P^T", "an entry inside a colour", r);
        spmv_csr_destroy(b);
        free(perm);
    }

    check_permute("generic, unsorted with repeats", generic(1, false));
    check_permute("generic, sorted", g);
    check_permute("rows of 0, 1, 63, 64, 65, 4095 and 4096 entries", lengths({0, 1, 63, 64, 65, 4095, 4096, 7, 8, 9}, 5000, 300));
    check_permute("a row of 4097 entries", lengths({0, 1, 64, 65, 4097}, 6000, 40));
    check_permute("rectangular 256 x 384", lengths(std::vector<int>(256, 5), 384, 0));
    check_permute("stencil7(6)", stencil7(6));
    {
        Csr empty;
        for (int i = 0; i < 70; ++i) empty.add_row({});
        check_permute("nnz = 0", empty);
        check_permute("rows = 0", Csr());
    }
    refusals();
    vectors();
    unvalidated();
    std::printf("%d colourings, %d permutations\n", g_colorings, g_permutes);
    return 0;
}
