// tools/add_lockstep/main.cpp -- csrc/kernels_add.hip executed on the host (hip/hip_runtime.h: a thread per work-item) against a
// serial statement of the contract of include/spmv_hip.h "the sparse sum": row_ptr, col_idx, the bits of vals and the plan's two
// arrays from the first call, the bits of vals again from add_values on the kept plan (after the operands' values were
// rewritten, with other coefficients), and add_gather into a poisoned target.  Every array is an exactly sized heap block.
#include "kernels_add.hip"

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
    std::vector<int32_t> rp, ci, start;
    std::vector<uint32_t> va, term;
};

// the contract: per row an ordered map column -> (a's positions, b's positions), each ascending
Result reference(const Csr &a, const Csr &b, float alpha, float beta, int op)
{
    Result r;
    r.rp.push_back(0);
    for (int64_t i = 0; i < a.rows; ++i) {
        std::map<int32_t, std::pair<std::vector<int32_t>, std::vector<int32_t>>> cols;
        for (int32_t s = a.rp[i]; s < a.rp[i + 1]; ++s) cols[a.ci[s]].first.push_back(s);
        for (int32_t q = b.rp[i]; q < b.rp[i + 1]; ++q) cols[b.ci[q]].second.push_back(q);
        for (const auto &e : cols) {
            const bool in_a = !e.second.first.empty(), in_b = !e.second.second.empty();
            const bool kept = op == SPMV_ADD_UNION ? true : op == SPMV_ADD_INTERSECT ? (in_a && in_b) : (in_a && !in_b);
            if (!kept) continue;
            float acc = 0.0f;
            bool first = true;
            r.start.push_back((int32_t)r.term.size());
            for (int32_t s : e.second.first) {
                r.term.push_back((uint32_t)s);
                if (alpha == 0.0f) continue;
                volatile float prod = alpha * a.va[s];
                acc = first ? prod : std::fmaf(alpha, a.va[s], acc);
                first = false;
            }
            if (op != SPMV_ADD_MINUS)
                for (int32_t q : e.second.second) {
                    r.term.push_back(0x80000000u | (uint32_t)q);
                    if (beta == 0.0f) continue;
                    volatile float prod = beta * b.va[q];
                    acc = first ? prod : std::fmaf(beta, b.va[q], acc);
                    first = false;
                }
            r.ci.push_back(e.first);
            r.va.push_back(bits_of(acc));
        }
        r.rp.push_back((int32_t)r.ci.size());
    }
    r.start.push_back((int32_t)r.term.size());
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

// words equal, except that a NaN matches any NaN where `floats`
bool same(const void *got, const void *want, size_t words, bool floats = false)
{
    const uint32_t *g = (const uint32_t *)got, *w = (const uint32_t *)want;
    for (size_t i = 0; i < words; ++i)
        if (g[i] != w[i] && !(floats && std::isnan(float_of(g[i])) && std::isnan(float_of(w[i])))) return false;
    return true;
}

void fail(const char *what, const char *stage, int op, int rc, const spmv_csr *out, const Result &want)
{
    std::fprintf(stderr, "MISMATCH %s op %d (%s): rc %d, nnz %lld, want %zu\n", what, op, stage, rc, out ? (long long)out->nnz : -1ll,
                 want.ci.size());
    if (out && out->nnz == (int64_t)want.ci.size())
        for (size_t i = 0; i < want.ci.size(); ++i)
            if (out->d_col_idx[i] != want.ci[i] || bits_of(out->d_vals[i]) != want.va[i]) {
                std::fprintf(stderr, "  first at %zu: col %d want %d, bits %08x want %08x\n", i, out->d_col_idx[i], want.ci[i],
                             bits_of(out->d_vals[i]), want.va[i]);
                break;
            }
    std::exit(1);
}

const float kCoef[][2] = {{1.0f / 3.0f, 3.0f}, {1.0f, 0.0f}, {-0.0f, 1.0f}, {1.0f, 1.0f}};

void check(const char *what, Csr a, Csr b, bool same_handle = false)
{
    std::mt19937 rng(777);
    for (int op = 0; op < 3; ++op)
        for (int keep_plan = 0; keep_plan < 2; ++keep_plan) {
            const float alpha = kCoef[(op + keep_plan) % 4][0], beta = kCoef[(op + keep_plan) % 4][1];
            const Result want = reference(a, same_handle ? a : b, alpha, beta, op);
            Device da(a), db_(b);
            const spmv_csr &ha = da.h, &hb = same_handle ? da.h : db_.h;
            float *vb = same_handle ? da.va : db_.va;
            spmv_csr_t *out = nullptr;
            const int rc = spmv::add(ha, hb, alpha, beta, op, keep_plan == 1, nullptr, &out);
            const bool ok = rc == 0 && out && out->rows == a.rows && out->cols == a.cols && out->nnz == (int64_t)want.ci.size() &&
                            out->plan_add.ready == (keep_plan == 1) && same(out->d_row_ptr, want.rp.data(), want.rp.size()) &&
                            same(out->d_col_idx, want.ci.data(), want.ci.size()) && same(out->d_vals, want.va.data(), want.va.size(), true);
            if (!ok) fail(what, keep_plan ? "keep_plan" : "first call", op, rc, out, want);
            if (keep_plan) {
                const spmv::AddPlan &p = out->plan_add;
                if (p.terms != (int64_t)want.term.size() || !same(p.d_term.get(), want.term.data(), want.term.size()) ||
                    !same(p.d_start.get(), want.start.data(), want.start.size()) ||
                    spmv::add_plan_bytes(*out) != 4 * (int64_t)want.term.size() + 4 * (out->nnz + 1))
                    fail(what, "plan", op, 0, out, want);
                // new values in place and other coefficients, then the value pass alone
                for (size_t i = 0; i < a.va.size(); ++i) da.va[i] = a.va[i] = a.va[i] * 0.75f + (float)(int)(rng() % 5) - 2.0f;
                if (!same_handle)
                    for (size_t i = 0; i < b.va.size(); ++i) vb[i] = b.va[i] = b.va[i] * 1.25f - (float)(int)(rng() % 3);
                const float al2 = kCoef[(op + 2) % 4][0], be2 = kCoef[(op + 2) % 4][1];
                const Result again = reference(a, same_handle ? a : b, al2, be2, op);
                for (int64_t i = 0; i < out->nnz; ++i) out->own_vals.get()[i] = float_of(0x7fc00123u);
                const int rc2 = spmv::add_values(*out, ha, hb, al2, be2, nullptr);
                if (rc2 != 0 || !same(out->d_vals, again.va.data(), again.va.size(), true)) fail(what, "add_values", op, rc2, out, again);
                // the gather: two arrays in c's order to each side's order, the words without a term keep the poison
                for (int side = 0; side < 2; ++side) {
                    const int64_t n = side ? hb.nnz : ha.nnz, stride = n + 3;
                    std::vector<uint32_t> src(2 * (size_t)out->nnz + 1), expect(2 * (size_t)stride, 0xdeadbeefu);
                    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint32_t)rng();
                    for (int64_t e = 0; e < out->nnz; ++e)
                        for (int32_t t = want.start[e]; t < want.start[e + 1]; ++t)
                            if ((int)(want.term[t] >> 31) == side)
                                for (int k = 0; k < 2; ++k) expect[k * stride + (want.term[t] & 0x7fffffffu)] = src[k * out->nnz + e];
                    uint32_t *s_ = exact_copy(src), *d_ = exact_copy(std::vector<uint32_t>(2 * (size_t)stride - 3, 0xdeadbeefu));
                    const int rc3 = spmv::add_gather(*out, side, 2, s_, out->nnz, d_, stride, nullptr);
                    const bool good = rc3 == 0 && same(d_, expect.data(), 2 * (size_t)stride - 3);
                    free(s_); free(d_);
                    if (!good) fail(what, "add_gather", op, rc3, out, want);
                }
            }
            delete out;
            ++g_checked;
        }
}

// operands that were never validated: whatever comes out, no access outside the arrays (the sanitizer is the check)
void survive(const char *what, const Csr &a, const Csr &b)
{
    for (int op = 0; op < 3; ++op) {
        Device da(a), db_(b);
        spmv_csr_t *out = nullptr;
        const int rc = spmv::add(da.h, db_.h, 0.5f, 2.0f, op, true, nullptr, &out);
        if (rc == 0 && out) {
            std::vector<uint32_t> src((size_t)out->nnz + 1, 7u);
            uint32_t *d_ = exact_copy(std::vector<uint32_t>((size_t)da.h.nnz, 0u));
            (void)spmv::add_values(*out, da.h, db_.h, 1.0f, 1.0f, nullptr);
            (void)spmv::add_gather(*out, 0, 1, src.data(), 0, d_, 0, nullptr);
            free(d_);
        }
        std::printf("  %s op %d: rc %d, nnz %lld\n", what, op, rc, out ? (long long)out->nnz : -1ll);
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

Csr random_csr(std::mt19937 &rng, int64_t rows, int64_t cols, int max_len, bool repeats, bool sorted = false)
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
        if (sorted) {
            std::sort(c.begin(), c.end());
            if (!repeats) c.erase(std::unique(c.begin(), c.end()), c.end());
            v.resize(c.size());
        }
        m.add_row(c, v);
    }
    return m;
}

std::vector<int32_t> pick(std::mt19937 &rng, int n, int cols)
{
    std::vector<int32_t> all(cols);
    for (int i = 0; i < cols; ++i) all[i] = i;
    std::shuffle(all.begin(), all.end(), rng);
    all.resize(n);
    std::sort(all.begin(), all.end());
    return all;
}

void push(std::mt19937 &rng, Csr &m, const std::vector<int32_t> &c)
{
    std::vector<float> v(c.size());
    for (float &x : v) x = spread(rng);
    m.add_row(c, v);
}

std::vector<int32_t> range(int lo, int hi, int step)
{
    std::vector<int32_t> c;
    for (int i = lo; i < hi; i += step) c.push_back(i);
    return c;
}

const uint32_t kSpecial[] = {0x7FC00000u, 0xFFC00001u, 0x7F800000u, 0xFF800000u, 0x00000000u, 0x80000000u, 0x00000001u,
                             0x80000001u, 0x007FFFFFu, 0x7F7FFFFFu, 0x3F800000u, 0xBF800000u};

}  // namespace

int main()
{
    std::mt19937 rng(4343);
    // 1. generic: unsorted rows of 0 .. 40 entries with repeated columns on both sides (the row-sorted view)
    {
        const Csr a = random_csr(rng, 257, 193, 40, true), b = random_csr(rng, 257, 193, 40, true);
        check("generic", a, b);
        Csr ba, bb;                       // rows 100 .. 163 of both: the same rows of the sum (checked against the same contract)
        ba.cols = bb.cols = a.cols;
        for (int r = 100; r < 164; ++r) {
            ba.add_row(std::vector<int32_t>(a.ci.begin() + a.rp[r], a.ci.begin() + a.rp[r + 1]),
                       std::vector<float>(a.va.begin() + a.rp[r], a.va.begin() + a.rp[r + 1]));
            bb.add_row(std::vector<int32_t>(b.ci.begin() + b.rp[r], b.ci.begin() + b.rp[r + 1]),
                       std::vector<float>(b.va.begin() + b.rp[r], b.va.begin() + b.rp[r + 1]));
        }
        check("row block", ba, bb);
        check("a == b", a, a, true);
        check("one side sorted", random_csr(rng, 257, 193, 40, false, true), b);
    }
    std::printf("generic: %d sums\n", g_checked); std::fflush(stdout);
    // 2. sorted operands (the merge on the operands' own arrays), duplicate-free and with repeated columns
    check("sorted", random_csr(rng, 300, 211, 30, false, true), random_csr(rng, 300, 211, 30, false, true));
    check("sorted with repeats", random_csr(rng, 300, 211, 30, true, true), random_csr(rng, 300, 211, 30, true, true));
    {
        const Csr s = random_csr(rng, 120, 90, 30, true, true);
        check("sorted a == b", s, s, true);
    }
    std::printf("sorted: %d sums\n", g_checked); std::fflush(stdout);
    // 3. row lengths on either side against 0, 1, 64 and a row of 5000; identical, disjoint, interleaved rows; b below / above a
    {
        Csr a, b;
        a.cols = b.cols = 20000;
        for (int la : {0, 1, 2, 63, 64, 65, 129})
            for (int lb : {0, 1, 64}) {
                push(rng, a, pick(rng, la, 20000)); push(rng, b, pick(rng, lb, 20000));
                push(rng, a, pick(rng, lb, 20000)); push(rng, b, pick(rng, la, 20000));
            }
        for (int la : {0, 1, 2, 63, 64, 65, 129}) {
            push(rng, a, pick(rng, la, 20000)); push(rng, b, pick(rng, 5000, 20000));
            push(rng, a, pick(rng, 5000, 20000)); push(rng, b, pick(rng, la, 20000));
        }
        const std::vector<int32_t> same_row = pick(rng, 70, 20000);
        push(rng, a, same_row); push(rng, b, same_row);
        push(rng, a, range(0, 200, 2)); push(rng, b, range(1, 200, 2));
        push(rng, a, range(0, 300, 3)); push(rng, b, range(0, 300, 2));
        push(rng, a, range(1000, 1100, 1)); push(rng, b, range(0, 90, 1));
        push(rng, a, range(0, 90, 1)); push(rng, b, range(1000, 1100, 1));
        push(rng, a, std::vector<int32_t>(300, 17)); push(rng, b, std::vector<int32_t>(5, 17));     // one column, long runs
        check("row lengths", a, b);
    }
    std::printf("row lengths: %d sums\n", g_checked); std::fflush(stdout);
    // 4. the edges of the types and the degenerate sizes
    {
        Csr a, b;
        a.cols = b.cols = 2147483647;
        a.add_row({2147483646, 0, 2147483646, 5}, {1.0f, 2.0f, 3.0f, 4.0f});
        a.add_row({2147483645}, {-1.0f});
        b.add_row({5, 2147483646}, {2.0f, 3.0f});
        b.add_row({2147483646, 2147483645, 2147483645}, {5.0f, 0.5f, 0.25f});
        check("2^31 - 1 columns", a, b);
        Csr e0, f0;                                                      // m = 0
        e0.cols = f0.cols = 9;
        check("m = 0", e0, f0);
        Csr an, bn;                                                      // n = 0
        an.cols = bn.cols = 0;
        an.add_row({}, {}); an.add_row({}, {}); bn.add_row({}, {}); bn.add_row({}, {});
        check("n = 0", an, bn);
        Csr z;                                                           // nnz = 0 on either side, on both
        z.cols = a.cols;
        z.add_row({}, {}); z.add_row({}, {});
        check("a without nonzeros", z, b);
        check("b without nonzeros", a, z);
        check("no nonzeros", z, z);
        Csr p, q;                                                        // an empty intersection
        p.cols = q.cols = 10;
        p.add_row({1, 3, 5}, {1.0f, 2.0f, 3.0f}); q.add_row({0, 2, 4}, {1.0f, 2.0f, 3.0f});
        check("disjoint", p, q);
    }
    // 5. values: the special set on both sides, a cancelling pair, stored zeros
    {
        Csr a = random_csr(rng, 70, 40, 20, true), b = random_csr(rng, 70, 40, 20, true);
        for (float &x : a.va) if (rng() % 3 == 0) x = float_of(kSpecial[rng() % 12]);
        for (float &x : b.va) if (rng() % 3 == 0) x = float_of(kSpecial[rng() % 12]);
        a.add_row({5, 7}, {1.5f, 0.0f});
        b.add_row({5, 7}, {-0.5f, 0.0f});
        check("special values", a, b);
        Csr nanb = b;
        for (float &x : nanb.va) x = float_of(0x7FC00000u);
        check("a mask of NaNs", a, nanb);                                // (kCoef holds beta = 0 and alpha = -0 among its pairs)
    }
    std::printf("edges and values: %d sums\n", g_checked); std::fflush(stdout);
    // 6. operands that were never validated
    {
        const Csr good = random_csr(rng, 40, 30, 12, true, true);
        Csr desc = good;
        std::reverse(desc.rp.begin(), desc.rp.end());                    // a descending row_ptr
        survive("descending row_ptr", desc, good);
        survive("descending row_ptr (b)", good, desc);
        Csr wild = good;
        for (size_t i = 0; i < wild.ci.size(); i += 7) wild.ci[i] = (i % 2) ? -5 : 1000000;      // columns out of range (and unsorted rows)
        survive("columns out of range", wild, good);
        survive("columns out of range (b)", good, wild);
        Csr far = good;
        for (size_t i = 1; i < far.rp.size(); ++i) far.rp[i] += 1000;    // a row_ptr beyond nnz
        survive("row_ptr beyond nnz", far, good);
        Csr un = random_csr(rng, 40, 30, 12, true);
        std::reverse(un.rp.begin(), un.rp.end());
        survive("unsorted and descending", un, good);
    }
    std::printf("add lockstep: %d sums bit for bit or survived\n", g_checked);
    return 0;
}
