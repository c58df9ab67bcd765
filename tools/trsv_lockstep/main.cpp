// tools/trsv_lockstep/main.cpp -- csrc/kernels_trsv.hip executed on the host (hip/hip_runtime.h: a thread per work-item, real
// barriers) against a serial statement of the contract of include/spmv_hip.h "the triangular solve": level_ptr, order, the
// counts the plan reports, the launches of a solve and the bits of x, for both triangles, unit and non-unit, and the thin
// thresholds 1, the default and 1 << 30.  Every array, b and x included, is an exactly sized heap block.
#include "kernels_trsv.hip"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace {

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> rp{0}, ci;
    std::vector<float> va;
    void add_row(const std::vector<int32_t> &c, const std::vector<float> &v)
    {
        ci.insert(ci.end(), c.begin(), c.end());
        va.insert(va.end(), v.begin(), v.end());
        rp.push_back((int32_t)ci.size());
        ++n;
    }
};

struct Want {
    std::vector<int32_t> level_ptr, order;
    std::vector<uint32_t> x;
    int64_t long_rows = 0, bad_row = -1, widest = 0;
};

// the contract, one row after the other
Want reference(const Csr &a, const std::vector<float> &b, bool upper, bool unit)
{
    const int64_t n = a.n;
    Want w;
    std::vector<int32_t> level((size_t)n, 0);
    std::vector<float> x((size_t)n, 0.0f);
    int32_t levels = 0;
    for (int64_t step = 0; step < n; ++step) {
        const int64_t i = upper ? n - 1 - step : step;
        std::vector<int32_t> terms;
        int ndiag = 0;
        float d = 1.0f;
        for (int32_t s = a.rp[i]; s < a.rp[i + 1]; ++s) {
            const int32_t c = a.ci[s];
            if (c == i) { if (ndiag++ == 0 && !unit) d = a.va[s]; }
            else if (upper ? c > i : c < i) terms.push_back(s);
        }
        if (ndiag != 1 && (w.bad_row < 0 || i < w.bad_row)) w.bad_row = i;
        for (int32_t s : terms) level[i] = std::max(level[i], level[a.ci[s]] + 1);
        levels = std::max(levels, level[i] + 1);
        float sum = 0.0f;
        if ((int64_t)terms.size() <= SPMV_TRSV_SERIAL_MAX) {
            for (int32_t s : terms) sum = std::fmaf(a.va[s], x[a.ci[s]], sum);
        } else {
            ++w.long_rows;
            float p[64] = {};
            for (size_t t = 0; t < terms.size(); ++t) p[t % 64] = std::fmaf(a.va[terms[t]], x[a.ci[terms[t]]], p[t % 64]);
            for (int wd = 32; wd >= 1; wd >>= 1)
                for (int l = 0; l < wd; ++l) { volatile float q = p[l] + p[l + wd]; p[l] = q; }
            sum = p[0];
        }
        volatile float num = b[i] - sum;
        volatile float q = unit ? num : num / d;
        x[i] = q;
    }
    w.level_ptr.assign((size_t)levels + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++w.level_ptr[level[i] + 1];
    for (int32_t k = 0; k < levels; ++k) { w.widest = std::max<int64_t>(w.widest, w.level_ptr[k + 1]); w.level_ptr[k + 1] += w.level_ptr[k]; }
    w.order.resize((size_t)n);
    std::vector<int32_t> at(w.level_ptr.begin(), w.level_ptr.end());
    for (int64_t i = 0; i < n; ++i) w.order[at[level[i]]++] = (int32_t)i;
    for (float v : x) w.x.push_back(bits_of(v));
    return w;
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
        h.rows = h.cols = m.n; h.nnz = (int64_t)m.ci.size();
        h.d_row_ptr = rp; h.d_col_idx = ci; h.d_vals = va;
    }
    ~Device() { free(rp); free(ci); free(va); }
};

int g_checked = 0;

[[noreturn]] void fail(const char *what, const char *stage, bool upper, bool unit, int thin)
{
    std::fprintf(stderr, "MISMATCH %s (%s): %s %s thin_rows %d\n", what, stage, upper ? "upper" : "lower", unit ? "unit" : "non-unit", thin);
    std::exit(1);
}

void check(const char *what, const Csr &a, const std::vector<float> &b, bool both_diags = true, std::vector<int> thins = {1, 0, 1 << 30})
{
    for (int upper = 0; upper < 2; ++upper) {
        Device d(a);
        for (int thin : thins) {
            if (spmv::trsv_plan(d.h, upper == 1, thin, nullptr) != SPMV_OK) fail(what, "plan refused", upper, false, thin);
            const spmv::TrsvPlan &p = d.h.plan_trsv[upper];
            for (int unit = both_diags ? 0 : 1; unit < 2; ++unit) {
                const Want w = reference(a, b, upper == 1, unit == 1);
                const int64_t levels = (int64_t)w.level_ptr.size() - 1;
                if (!p.ready || p.levels != levels || p.widest != w.widest || p.long_rows != w.long_rows || p.bad_diag_row != w.bad_row ||
                    std::memcmp(p.level_ptr, w.level_ptr.data(), 4 * w.level_ptr.size()) != 0 ||
                    std::memcmp(p.d_level_ptr.get(), w.level_ptr.data(), 4 * w.level_ptr.size()) != 0)
                    fail(what, "levels", upper, unit, thin);
                for (int64_t i = 0; i < a.n; ++i)
                    if ((p.d_order.get()[i] & INT32_MAX) != w.order[i]) fail(what, "order", upper, unit, thin);
                // the launches of a solve, as the header states them
                int64_t launches = 0;
                for (int64_t k = 0; k < levels; ++launches) {
                    if (w.level_ptr[k + 1] - w.level_ptr[k] > p.thin) { ++k; continue; }
                    const int64_t k0 = k;
                    while (k < levels && k - k0 < p.cap && w.level_ptr[k + 1] - w.level_ptr[k] <= p.thin) ++k;
                }
                if (p.nsteps != launches) fail(what, "launches", upper, unit, thin);
                if (!unit && w.bad_row >= 0) continue;                       // (the entry point refuses this solve)
                float *db = exact_copy(b), *dx = (float *)malloc(sizeof(float) * (a.n ? a.n : 1));
                for (int64_t i = 0; i < a.n; ++i) dx[i] = NAN;
                const long before = emu_launches;
                if (spmv::trsv_solve(d.h, upper == 1, unit == 1, db, dx, nullptr) != SPMV_OK || emu_launches - before != launches)
                    fail(what, "solve", upper, unit, thin);
                for (int64_t i = 0; i < a.n; ++i)
                    if (bits_of(dx[i]) != w.x[i]) {
                        float wf;
                        std::memcpy(&wf, &w.x[i], 4);
                        if (std::isnan(dx[i]) && std::isnan(wf)) continue;     // a NaN matches any NaN
                        std::fprintf(stderr, "  row %lld: %.9g (%08x), want %.9g (%08x)\n", (long long)i, dx[i], bits_of(dx[i]), wf, w.x[i]);
                        fail(what, "x", upper, unit, thin);
                    }
                // in place
                if (spmv::trsv_solve(d.h, upper == 1, unit == 1, db, db, nullptr) != SPMV_OK) fail(what, "in place", upper, unit, thin);
                for (int64_t i = 0; i < a.n; ++i)
                    if (bits_of(db[i]) != bits_of(dx[i]) && !(std::isnan(db[i]) && std::isnan(dx[i]))) fail(what, "in place x", upper, unit, thin);
                free(db);
                free(dx);
                ++g_checked;
            }
        }
    }
}

// a row-dominant matrix from per-row term columns (in the given order), the diagonal at a random place
Csr dominant(const std::vector<std::vector<int32_t>> &cols, std::mt19937 &rng, int skip_diag_of = -1, int twice_diag_of = -1)
{
    Csr m;
    std::uniform_real_distribution<float> u(0.05f, 1.0f);
    for (size_t i = 0; i < cols.size(); ++i) {
        std::vector<int32_t> c = cols[i];
        std::vector<float> v;
        float lo = 0.0f, up = 0.0f;
        for (int32_t cc : c) {
            const float x = (rng() & 1) ? u(rng) : -u(rng);
            v.push_back(x);
            (cc < (int32_t)i ? lo : up) += std::fabs(x);
        }
        const float d = std::max(std::max(lo, up), 0.45f) / 0.9f * (1.0f + 0.5f * u(rng)) * ((rng() & 1) ? 1.0f : -1.0f);
        const int copies = (int)i == skip_diag_of ? 0 : (int)i == twice_diag_of ? 2 : 1;
        for (int k = 0; k < copies; ++k) {
            const size_t at = rng() % (c.size() + 1);
            c.insert(c.begin() + (long)at, (int32_t)i);
            v.insert(v.begin() + (long)at, d);
        }
        m.add_row(c, v);
    }
    return m;
}

std::vector<float> rhs(int64_t n, std::mt19937 &rng)
{
    std::uniform_real_distribution<float> u(0.5f, 1.5f);
    std::vector<float> b((size_t)n);
    for (float &x : b) x = (rng() & 1) ? u(rng) : -u(rng);
    return b;
}

// operands that were never validated: any result or refusal, no access outside the arrays and no unbounded loop
void unvalidated(const char *what, const Csr &bad)
{
    spmv::g_quiet = true;
    for (int upper = 0; upper < 2; ++upper)
        for (int thin : {1, 0}) {
            Device d(bad);
            if (spmv::trsv_plan(d.h, upper == 1, thin, nullptr) != SPMV_OK) continue;
            for (int unit = 0; unit < 2; ++unit) {
                std::vector<float> b((size_t)bad.n, 1.0f);
                float *db = exact_copy(b), *dx = (float *)malloc(sizeof(float) * (bad.n ? bad.n : 1));
                (void)spmv::trsv_solve(d.h, upper == 1, unit == 1, db, dx, nullptr);
                free(db);
                free(dx);
            }
        }
    spmv::g_quiet = false;
    std::printf("  %s: inside the arrays\n", what);
    ++g_checked;
}

}  // namespace

int main()
{
    std::mt19937 rng(20261);
    {   // generic: 257 x 257 full, unsorted rows with repeats, long rows in both triangles
        std::vector<std::vector<int32_t>> cols(257);
        for (int i = 0; i < 257; ++i) {
            const int k = i % 16 == 8 ? 70 + (int)(rng() % 51) : (int)(rng() % 25);
            for (int j = 0; j < k; ++j) { const int32_t c = (int32_t)(rng() % 257); if (c != i) cols[i].push_back(c); }
        }
        const Csr m = dominant(cols, rng);
        check("generic", m, rhs(257, rng), true, {1, 0, 7, 1 << 30});
        std::vector<float> b = rhs(257, rng);
        b[100] = NAN; b[130] = INFINITY;
        check("generic with NaN and Inf in b", m, b, true, {0});
        check("a missing diagonal", dominant(cols, rng, 41), rhs(257, rng), true, {0});
        check("a repeated diagonal", dominant(cols, rng, -1, 77), rhs(257, rng), true, {0});
    }
    {   // the shapes of the level graph
        std::vector<std::vector<int32_t>> none(3000), lower(3000), upper(3000);
        for (int i = 0; i < 3000; ++i) { if (i > 0) lower[i].push_back(i - 1); if (i < 2999) upper[i].push_back(i + 1); }
        check("diagonal", dominant(none, rng), rhs(3000, rng), true, {0});
        check("bidiagonal chain, lower", dominant(lower, rng), rhs(3000, rng), false, {0});
        check("bidiagonal chain, upper", dominant(upper, rng), rhs(3000, rng), false, {0});
        std::vector<std::vector<int32_t>> fan(5010);
        for (int i = 10; i < 5010; ++i)
            for (int j = 0, k = 1 + (int)(rng() % 10); j < k; ++j) fan[i].push_back((int32_t)(rng() % 10));
        check("fan", dominant(fan, rng), rhs(5010, rng), false, {0});
        const int sizes[] = {69, 70, 71, 70, 69, 1, 71};
        std::vector<std::vector<int32_t>> st;
        int first = 0, prev = 0;
        for (int s : sizes) {
            for (int r = 0; r < s; ++r) {
                st.emplace_back();
                if (first > 0) for (int j = 0, k = 1 + (int)(rng() % 3); j < k; ++j) st.back().push_back(prev + (int32_t)(rng() % (first - prev)));
            }
            prev = first;
            first += s;
        }
        check("levels around thin_rows = 70", dominant(st, rng), rhs((int64_t)st.size(), rng), true, {70, 1});
        std::vector<std::vector<int32_t>> grid(512);
        for (int r = 0; r < 512; ++r)
            for (int o : {-64, -8, -1, 1, 8, 64}) {
                const int i = r / 64, j = (r / 8) % 8, k = r % 8;
                const bool ok = o == -64 ? i > 0 : o == -8 ? j > 0 : o == -1 ? k > 0 : o == 1 ? k < 7 : o == 8 ? j < 7 : i < 7;
                if (ok) grid[r].push_back(r + o);
            }
        check("7-point stencil on 8^3", dominant(grid, rng), rhs(512, rng));
    }
    {   // row lengths: 5000 rows without terms, then one row of each length
        std::vector<std::vector<int32_t>> cols(5000);
        for (int len : {1, SPMV_TRSV_SERIAL_MAX - 1, SPMV_TRSV_SERIAL_MAX, SPMV_TRSV_SERIAL_MAX + 1, 63, 64, 65, 129, 5000}) {
            cols.emplace_back();
            for (int j = 0; j < len; ++j) cols.back().push_back((int32_t)(rng() % 5000));
        }
        check("row lengths", dominant(cols, rng), rhs((int64_t)cols.size(), rng), false, {1, 0, 1 << 30});
    }
    {   // special values and the edges
        Csr s;
        const float tiny = 1e-41f;
        s.add_row({0}, {0.0f}); s.add_row({1}, {-0.0f}); s.add_row({2}, {2.0f}); s.add_row({3}, {4.0f});
        s.add_row({3, 4}, {tiny, 3.0f}); s.add_row({5}, {0.0f}); s.add_row({6, 2, 3}, {1.0f, 5.0f, 1.0f});
        check("special values", s, {1.0f, 1.0f, -0.0f, tiny * 3, 1.0f, 0.0f, 0.0f});
        check("no rows", Csr{}, {});
        Csr one;
        one.add_row({0}, {3.0f});
        check("one row", one, {1.0f});
        Csr hollow;
        for (int i = 0; i < 5; ++i) hollow.add_row({}, {});
        check("no nonzeros", hollow, {1.5f, -2.0f, 0.0f, INFINITY, 1e-40f});
    }
    std::printf("%d solves agree with the contract\n", g_checked);
    {
        std::vector<std::vector<int32_t>> cols(64);
        for (int i = 0; i < 64; ++i)
            for (int j = 0; j < (int)(rng() % 40); ++j) cols[i].push_back((int32_t)(rng() % 64));
        const Csr good = dominant(cols, rng);
        Csr a = good, b = good, c = good, d = good;
        std::reverse(a.rp.begin() + 1, a.rp.end() - 1);                         // a descending row_ptr
        unvalidated("a descending row_ptr", a);
        for (size_t k = 0; k < b.ci.size(); k += 7) b.ci[k] = k % 3 == 0 ? -5 : k % 3 == 1 ? 64 : INT32_MAX;
        unvalidated("columns out of range", b);
        for (int32_t &r : c.rp) r = r * 2 + 3;                                 // row_ptr beyond nnz (and not from 0)
        unvalidated("a row_ptr beyond nnz", c);
        for (int32_t &r : d.rp) r = -r;
        unvalidated("a negative row_ptr", d);
    }
    return 0;
}
