// tools/ilu0_lockstep/main.cpp -- csrc/kernels_ilu0.hip executed on the host (hip/hip_runtime.h of tools/trsv_lockstep: a thread
// per work-item, real barriers) against a serial statement of the contract of include/spmv_hip.h "the incomplete
// factorisation": the bits of M, the pivot word and the launches of a factorisation, under the thin thresholds 1, the default
// and 1 << 30, through spmv_csr_ilu0's own path (the check, the copies, the plans, the factor) and again through ilu0_values.
// order, level_ptr and the diagonal's positions come from the serial plan of spmv_internal.hpp beside this file, so nothing of
// kernels_trsv.hip is needed.  Every array is an exactly sized heap block.
#include "kernels_ilu0.hip"

#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
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

// the contract, one row after the other; rows sorted with their diagonal.  Returns M and the pivot row (-1: none)
std::vector<float> reference(const Csr &a, int64_t *pivot)
{
    std::vector<float> M = a.va;
    std::vector<int32_t> diag((size_t)a.n, -1);
    for (int64_t i = 0; i < a.n; ++i)
        for (int32_t s = a.rp[i]; s < a.rp[i + 1]; ++s)
            if (a.ci[s] == i) diag[i] = s;
    *pivot = -1;
    for (int64_t i = 0; i < a.n; ++i) {
        for (int32_t p = a.rp[i]; p < a.rp[i + 1]; ++p) {
            const int32_t k = a.ci[p];
            if (k >= i) continue;
            volatile float l = M[p] / M[diag[k]];
            M[p] = l;
            for (int32_t q = diag[k] + 1; q < a.rp[k + 1]; ++q)
                for (int32_t r = a.rp[i]; r < a.rp[i + 1]; ++r)
                    if (a.ci[r] == a.ci[q]) M[r] = std::fmaf(-l, M[q], M[r]);
        }
        const float u = M[diag[i]];
        if ((u == 0.0f || !std::isfinite(u)) && *pivot < 0) *pivot = i;
    }
    return M;
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

[[noreturn]] void fail(const char *what, const char *stage, int thin)
{
    std::fprintf(stderr, "MISMATCH %s (%s): thin_rows %d\n", what, stage, thin);
    std::exit(1);
}

void compare(const char *what, const char *stage, int thin, const spmv_csr &m, const std::vector<float> &want, int64_t want_pivot)
{
    for (size_t s = 0; s < want.size(); ++s)
        if (bits_of(m.d_vals[s]) != bits_of(want[s]) && !(std::isnan(m.d_vals[s]) && std::isnan(want[s]))) {
            std::fprintf(stderr, "  position %zu: %.9g (%08x), want %.9g (%08x)\n", s, m.d_vals[s], bits_of(m.d_vals[s]), want[s], bits_of(want[s]));
            fail(what, stage, thin);
        }
    int64_t got = -2;
    if (spmv::ilu0_pivot(m, nullptr, &got) != SPMV_OK || got != want_pivot) {
        std::fprintf(stderr, "  pivot row %lld, want %lld\n", (long long)got, (long long)want_pivot);
        fail(what, "pivot", thin);
    }
}

void check(const char *what, const Csr &a, std::vector<int> thins = {1, 0, 1 << 30})
{
    int64_t want_pivot = -1;
    const std::vector<float> want = reference(a, &want_pivot);
    for (int thin : thins) {
        Device d(a);
        spmv_csr_t *m = nullptr;
        const long before = emu_launches;
        if (spmv::ilu0(d.h, thin, nullptr, &m) != SPMV_OK || !m) fail(what, "refused", thin);
        const long launches = emu_launches - before;
        // the check (rows > 0), the reset and the steps of the lower plan
        if (launches != (a.n > 0 ? 1 : 0) + 1 + m->plan_trsv[0].nsteps) fail(what, "launches", thin);
        if (std::memcmp(m->d_row_ptr, a.rp.data(), 4 * a.rp.size()) != 0 || (a.ci.size() && std::memcmp(m->d_col_idx, a.ci.data(), 4 * a.ci.size()) != 0))
            fail(what, "pattern", thin);
        compare(what, "ilu0", thin, *m, want, want_pivot);
        // again from other values, then from these: _values alone
        Csr other = a;
        for (float &v : other.va) v *= 0.5f;
        Device d2(other);
        for (size_t s = 0; s < a.ci.size(); ++s) m->own_vals.get()[s] = NAN;
        if (spmv::ilu0_values(*m, d2.h, nullptr) != SPMV_OK) fail(what, "values", thin);
        const long again = emu_launches;
        if (spmv::ilu0_values(*m, d.h, nullptr) != SPMV_OK || emu_launches - again != 1 + m->plan_trsv[0].nsteps) fail(what, "values", thin);
        compare(what, "ilu0_values", thin, *m, want, want_pivot);
        (void)spmv_csr_destroy(m);
        ++g_checked;
    }
}

// sorted unique columns, the diagonal with |d| >= sum |row| / 0.9
Csr dominant(const std::vector<std::vector<int32_t>> &cols, std::mt19937 &rng)
{
    Csr m;
    std::uniform_real_distribution<float> u(0.05f, 1.0f);
    for (size_t i = 0; i < cols.size(); ++i) {
        std::set<int32_t> cs(cols[i].begin(), cols[i].end());
        cs.erase((int32_t)i);
        std::vector<int32_t> c;
        std::vector<float> v;
        float sum = 0.0f;
        for (int32_t cc : cs) {
            const float x = (rng() & 1) ? u(rng) : -u(rng);
            c.push_back(cc);
            v.push_back(x);
            sum += std::fabs(x);
        }
        const float d = std::max(sum, 0.45f) / 0.9f * (1.0f + 0.5f * u(rng)) * ((rng() & 1) ? 1.0f : -1.0f);
        const size_t at = (size_t)(std::lower_bound(c.begin(), c.end(), (int32_t)i) - c.begin());
        c.insert(c.begin() + (long)at, (int32_t)i);
        v.insert(v.begin() + (long)at, d);
        m.add_row(c, v);
    }
    return m;
}

// operands that were never validated, handed straight to the kernels: any result, no access outside the arrays, no unbounded loop
void unvalidated(const char *what, const Csr &bad)
{
    spmv::g_quiet = true;
    for (int thin : {1, 0}) {
        Device d(bad);
        spmv_csr m;
        m.rows = m.cols = bad.n; m.nnz = (int64_t)bad.ci.size();
        if (m.own_row_ptr.alloc(bad.rp.size()) || m.own_col_idx.alloc(bad.ci.size()) || m.own_vals.alloc(bad.ci.size()) ||
            m.plan_ilu0.d_pivot.alloc(1)) std::exit(2);
        std::memcpy(m.own_row_ptr.get(), bad.rp.data(), 4 * bad.rp.size());
        if (!bad.ci.empty()) std::memcpy(m.own_col_idx.get(), bad.ci.data(), 4 * bad.ci.size());
        m.d_row_ptr = m.own_row_ptr; m.d_col_idx = m.own_col_idx; m.d_vals = m.own_vals;
        if (spmv::trsv_plan(m, false, thin, nullptr) != SPMV_OK) continue;
        (void)spmv::ilu0_factor(m, d.va, nullptr);
    }
    spmv::g_quiet = false;
    std::printf("  %s: inside the arrays\n", what);
    ++g_checked;
}

void refused(const char *what, const Csr &bad)
{
    spmv::g_quiet = true;
    Device d(bad);
    spmv_csr_t *m = (spmv_csr_t *)16;
    const long before = emu_launches;
    if (spmv::ilu0(d.h, 0, nullptr, &m) != SPMV_ERR_INVALID || m != (spmv_csr_t *)16 || emu_launches - before != 1) fail(what, "not refused", 0);
    spmv::g_quiet = false;
    ++g_checked;
}

}  // namespace

int main()
{
    std::mt19937 rng(20262);
    std::vector<std::vector<int32_t>> generic(257);
    for (int i = 0; i < 257; ++i) {
        const int k = i % 16 == 8 ? 70 + (int)(rng() % 51) : (int)(rng() % 25);
        for (int j = 0; j < k; ++j) generic[i].push_back((int32_t)(rng() % 257));
    }
    {   // generic: 257 x 257, long rows whose terms come from short and from long rows; special values in it
        const Csr m = dominant(generic, rng);
        check("generic", m, {1, 0, 7, 1 << 30});
        Csr s = m;
        s.va[(size_t)s.rp[40] + 1] = NAN;
        s.va[(size_t)s.rp[100]] = INFINITY;
        check("generic with a NaN and an Inf", s, {0});
        Csr z = m;
        z.va[(size_t)z.rp[8] + 3] = -0.0f;
        z.va[(size_t)z.rp[24] + 5] = 1e-41f;
        check("generic with -0 and a subnormal", z, {0});
    }
    {   // the shapes of the level graph
        std::vector<std::vector<int32_t>> none(3000), tri(3000);
        for (int i = 0; i < 3000; ++i) { if (i > 0) tri[i].push_back(i - 1); if (i < 2999) tri[i].push_back(i + 1); }
        check("diagonal", dominant(none, rng), {0});
        check("tridiagonal chain", dominant(tri, rng), {0});
        std::vector<std::vector<int32_t>> fan(5010);
        for (int i = 0; i < 10; ++i) for (int j = 0; j < 3; ++j) fan[i].push_back(10 + (int32_t)(rng() % 5000));
        for (int i = 10; i < 5010; ++i)
            for (int j = 0, k = 1 + (int)(rng() % 10); j < k; ++j) fan[i].push_back((int32_t)(rng() % 10));
        check("5000 rows behind 10", dominant(fan, rng), {0, 1 << 30});
        const int sizes[] = {69, 70, 71, 70, 69, 1, 71};
        const int total = 421;
        std::vector<std::vector<int32_t>> st;
        int first = 0, prev = 0;
        for (int s : sizes) {
            for (int r = 0; r < s; ++r) {
                st.emplace_back();
                if (first > 0) for (int j = 0, k = 1 + (int)(rng() % 3); j < k; ++j) st.back().push_back(prev + (int32_t)(rng() % (first - prev)));
                if ((rng() & 1) && first + s < total) st.back().push_back(first + s + (int32_t)(rng() % (total - first - s)));   // (upper: a later level)
            }
            prev = first;
            first += s;
        }
        check("levels around thin_rows = 70", dominant(st, rng), {70, 1});
        std::vector<std::vector<int32_t>> grid(512);
        for (int r = 0; r < 512; ++r)
            for (int o : {-64, -8, -1, 1, 8, 64}) {
                const int i = r / 64, j = (r / 8) % 8, k = r % 8;
                const bool ok = o == -64 ? i > 0 : o == -8 ? j > 0 : o == -1 ? k > 0 : o == 1 ? k < 7 : o == 8 ? j < 7 : i < 7;
                if (ok) grid[r].push_back(r + o);
            }
        check("7-point stencil on 8^3", dominant(grid, rng));
        std::vector<std::vector<int32_t>> arrow(300);
        for (int i = 0; i < 299; ++i) { arrow[i].push_back(299); arrow[299].push_back(i); }
        check("arrow", dominant(arrow, rng));
    }
    {   // stored row lengths over 5000 diagonal rows
        std::vector<std::vector<int32_t>> cols(5000);
        for (int len : {1, 31, 32, 33, 63, 64, 65, 129, 5000}) {
            std::vector<int32_t> all(5000);
            for (int j = 0; j < 5000; ++j) all[j] = j;
            std::shuffle(all.begin(), all.end(), rng);
            cols.emplace_back(all.begin(), all.begin() + (len - 1));
        }
        check("row lengths", dominant(cols, rng), {1, 0, 1 << 30});
    }
    {   // a zero pivot, and the edges
        Csr z;
        for (int i = 0; i < 12; ++i) {
            if (i == 5) z.add_row({5, 6}, {1.0f, 1.0f});
            else if (i == 6) z.add_row({5, 6, 9}, {1.0f, 1.0f, 2.0f});
            else if (i == 9) z.add_row({6, 9}, {3.0f, 1.0f});
            else z.add_row({i}, {2.0f + (float)i});
        }
        check("a zero pivot", z);
        check("no rows", Csr{});
        Csr one;
        one.add_row({0}, {3.0f});
        check("one row", one);
    }
    std::printf("%d factorisations agree with the contract\n", g_checked);
    {
        const Csr good = dominant(generic, rng);
        Csr unsorted = good, repeated = good;
        std::swap(unsorted.ci[(size_t)unsorted.rp[8]], unsorted.ci[(size_t)unsorted.rp[8] + 1]);
        repeated.ci[(size_t)repeated.rp[24] + 1] = repeated.ci[(size_t)repeated.rp[24]];
        refused("an unsorted row", unsorted);
        refused("a repeated column", repeated);
        Csr nodiag;
        nodiag.add_row({0}, {1.0f}); nodiag.add_row({0}, {1.0f}); nodiag.add_row({2}, {1.0f});
        refused("a missing diagonal", nodiag);

        Csr a = good, b = good, c = good, d = good;
        std::reverse(a.rp.begin() + 1, a.rp.end() - 1);                         // a descending row_ptr
        unvalidated("a descending row_ptr", a);
        for (size_t k = 0; k < b.ci.size(); k += 7) b.ci[k] = k % 3 == 0 ? -5 : k % 3 == 1 ? 257 : INT32_MAX;
        unvalidated("columns out of range", b);
        for (int32_t &r : c.rp) r = r * 2 + 3;                                 // row_ptr beyond nnz (and not from 0)
        unvalidated("a row_ptr beyond nnz", c);
        for (int i = 8; i < 257; i += 16) std::reverse(d.ci.begin() + d.rp[i], d.ci.begin() + d.rp[i + 1]);
        unvalidated("unsorted rows handed straight to the kernels", d);
        unvalidated("an unsorted short row", unsorted);
    }
    return 0;
}
