// main.cpp -- the tester executable (reference: test/main.cpp:3-7 hard-codes 4096 x 4096).
//   sparse_sgemv [M N]                          the reference flow on a random dense M x N matrix
//   sparse_sgemv --mtx FILE [--variant NAME] [--transpose] [--out Y.txt] [--save FILE.csrbin] [--parse-only]
//   sparse_sgemv --csrbin FILE [--variant NAME] [--transpose] [--out Y.txt]
//        y = A * ones through the C ABI on a matrix from disk (row f-4), checked against a host walk;
//        --transpose: y = A^T * ones (x of `rows` ones, y of `cols` entries) through spmv_csr_transpose
//   sparse_sgemv --mtx A.mtx --spgemm B.mtx [--out C.mtx]
//        C = A * B through spmv_csr_spgemm, checked against a host walk of the same fma chains (pattern and bits), written
//        as a Matrix Market coordinate file
//   sparse_sgemv --mtx A.mtx --add B.mtx [--alpha x --beta y --op union|intersect|minus] [--out C.mtx]
//        C = alpha A + beta B through spmv_csr_add, checked against a host walk of the same chains (pattern and bits), written
//        as a Matrix Market coordinate file
//   sparse_sgemv --mtx A.mtx --trsv lower|upper [--unit] [--out x.txt]
//        x = T^-1 ones for the chosen triangle of a square A through spmv_csr_trsv (the other triangle is never read), checked
//        bit for bit against a host walk of the contract of include/spmv_hip.h "the triangular solve"
//   sparse_sgemv --mtx A.mtx --ilu0 [--out m.txt]
//        M = ILU(0) of a square A through spmv_csr_ilu0 (the reader sorts every row; every row must store its diagonal), M's
//        values in storage order checked bit for bit against a host walk of the contract of include/spmv_hip.h "the incomplete
//        factorisation"
//   sparse_sgemv --mtx A.mtx --color [--seed S] [--ilu0] --out B.mtx
//        colours a square A through spmv_csr_color (seed S, default 0), builds P A P^T through spmv_csr_permute and writes it as a
//        Matrix Market coordinate file; prints colours, rounds and the levels of both triangles of P A P^T; color and P A P^T's
//        bytes are checked against a host walk of the contract of include/spmv_hip.h "the multicolour ordering"; with --ilu0 it
//        also factors P A P^T and checks the factor as --ilu0 does
// $SPMV_SEED makes the random inputs reproducible.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <numeric>
#include <set>
#include <string>
#include <vector>
#include <hip/hip_runtime_api.h>
#include "kernel.hpp"
#include "mtx_io.hpp"
#include "tester.hpp"

static int variant_by_name(const std::string &n)
{
    for (int v = 0; v < SPMV_VARIANT_COUNT; ++v)
        if (n == spmv_variant_name(v)) return v;
    return -1;
}

// C = A B through the C ABI against the contract of include/spmv_hip.h "the sparse product", walked on the host
static int run_spgemm(const HostCsr &a, const std::string &b_path, const std::string &out)
{
    HostCsr b;
    std::string err = read_matrix_market(b_path, b);
    if (!err.empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    std::printf("times matrix %lld x %lld, nnz %lld\n", (long long)b.rows, (long long)b.cols, (long long)b.nnz());
    spmv_csr_t *A = nullptr, *B = nullptr, *Cm = nullptr;
    SPMV_CHECK(spmv_csr_create_host(a.rows, a.cols, a.nnz(), a.row_ptr.data(), a.col_idx.data(), a.vals.data(), &A));
    SPMV_CHECK(spmv_csr_create_host(b.rows, b.cols, b.nnz(), b.row_ptr.data(), b.col_idx.data(), b.vals.data(), &B));
    int64_t products = 0, rows = 0, cols = 0, nnz = 0;
    SPMV_CHECK(spmv_csr_spgemm(A, B, 0, nullptr, &Cm, &products));
    SPMV_CHECK(spmv_csr_dims(Cm, &rows, &cols, &nnz));
    HostCsr c;
    c.rows = rows; c.cols = cols;
    c.row_ptr.resize((size_t)rows + 1); c.col_idx.resize((size_t)nnz); c.vals.resize((size_t)nnz);
    SPMV_CHECK(spmv_csr_download(Cm, c.row_ptr.data(), c.col_idx.data(), c.vals.data()));
    SPMV_CHECK(spmv_csr_destroy(Cm));
    SPMV_CHECK(spmv_csr_destroy(B));
    SPMV_CHECK(spmv_csr_destroy(A));
    std::printf("spmv_csr_spgemm: %lld x %lld, nnz %lld from %lld products\n", (long long)rows, (long long)cols, (long long)nnz, (long long)products);
    int64_t bad = 0, at = 0;
    for (int64_t i = 0; i < a.rows; ++i) {
        std::map<int32_t, float> acc;
        for (int32_t s = a.row_ptr[i]; s < a.row_ptr[i + 1]; ++s)
            for (int32_t q = b.row_ptr[a.col_idx[s]]; q < b.row_ptr[a.col_idx[s] + 1]; ++q) {
                float &v = acc.emplace(b.col_idx[q], 0.0f).first->second;
                v = std::fmaf(a.vals[s], b.vals[q], v);
            }
        if (c.row_ptr[i] != at || c.row_ptr[i + 1] - c.row_ptr[i] != (int64_t)acc.size()) { ++bad; at = c.row_ptr[i + 1]; continue; }
        for (const auto &e : acc) {
            const bool same = c.col_idx[at] == e.first && (std::memcmp(&c.vals[at], &e.second, 4) == 0 || (std::isnan(c.vals[at]) && std::isnan(e.second)));
            if (!same) {
                if (bad < 16) std::fprintf(stderr, "[row %lld] cpu: (%d, %g), gpu: (%d, %g)\n", (long long)i, e.first, e.second, c.col_idx[at], c.vals[at]);
                ++bad;
            }
            ++at;
        }
    }
    if (!out.empty()) {
        FILE *f = std::fopen(out.c_str(), "w");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 2; }
        std::fprintf(f, "%%%%MatrixMarket matrix coordinate real general\n%lld %lld %lld\n", (long long)rows, (long long)cols, (long long)nnz);
        for (int64_t i = 0; i < rows; ++i)
            for (int32_t k = c.row_ptr[i]; k < c.row_ptr[i + 1]; ++k) std::fprintf(f, "%lld %d %.9g\n", (long long)i + 1, c.col_idx[k] + 1, c.vals[k]);
        if (std::fclose(f) != 0) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 2; }
    }
    std::printf(bad ? "====== %lld MISMATCHES ======\n" : "========== OK ===========\n", (long long)bad);
    return bad ? 1 : 0;
}

// C = alpha A + beta B through the C ABI against the contract of include/spmv_hip.h "the sparse sum", walked on the host
static int run_add(const HostCsr &a, const std::string &b_path, float alpha, float beta, int op, const std::string &out)
{
    HostCsr b;
    std::string err = read_matrix_market(b_path, b);
    if (!err.empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    std::printf("plus matrix %lld x %lld, nnz %lld\n", (long long)b.rows, (long long)b.cols, (long long)b.nnz());
    spmv_csr_t *A = nullptr, *B = nullptr, *Cm = nullptr;
    SPMV_CHECK(spmv_csr_create_host(a.rows, a.cols, a.nnz(), a.row_ptr.data(), a.col_idx.data(), a.vals.data(), &A));
    SPMV_CHECK(spmv_csr_create_host(b.rows, b.cols, b.nnz(), b.row_ptr.data(), b.col_idx.data(), b.vals.data(), &B));
    int64_t rows = 0, cols = 0, nnz = 0;
    SPMV_CHECK(spmv_csr_add(A, B, alpha, beta, op, 0, nullptr, &Cm));
    SPMV_CHECK(spmv_csr_dims(Cm, &rows, &cols, &nnz));
    HostCsr c;
    c.rows = rows; c.cols = cols;
    c.row_ptr.resize((size_t)rows + 1); c.col_idx.resize((size_t)nnz); c.vals.resize((size_t)nnz);
    SPMV_CHECK(spmv_csr_download(Cm, c.row_ptr.data(), c.col_idx.data(), c.vals.data()));
    SPMV_CHECK(spmv_csr_destroy(Cm));
    SPMV_CHECK(spmv_csr_destroy(B));
    SPMV_CHECK(spmv_csr_destroy(A));
    std::printf("spmv_csr_add: %lld x %lld, nnz %lld\n", (long long)rows, (long long)cols, (long long)nnz);
    struct Entry { bool in_a = false, in_b = false, any = false; float acc = 0.0f; };
    int64_t bad = 0, at = 0;
    for (int64_t i = 0; i < a.rows; ++i) {
        std::map<int32_t, Entry> acc;
        auto term = [](Entry &e, float coef, float v) {
            if (coef == 0.0f) return;                                   // +0 or -0: the pattern, no terms
            volatile float first = coef * v;                            // one rounding of its own
            e.acc = e.any ? std::fmaf(coef, v, e.acc) : first;
            e.any = true;
        };
        for (int32_t s = a.row_ptr[i]; s < a.row_ptr[i + 1]; ++s) { Entry &e = acc[a.col_idx[s]]; e.in_a = true; term(e, alpha, a.vals[s]); }
        for (int32_t q = b.row_ptr[i]; q < b.row_ptr[i + 1]; ++q) { Entry &e = acc[b.col_idx[q]]; e.in_b = true; if (op != SPMV_ADD_MINUS) term(e, beta, b.vals[q]); }
        for (auto it = acc.begin(); it != acc.end();) {
            const bool kept = op == SPMV_ADD_UNION ? true : op == SPMV_ADD_INTERSECT ? (it->second.in_a && it->second.in_b) : (it->second.in_a && !it->second.in_b);
            it = kept ? std::next(it) : acc.erase(it);
        }
        if (c.row_ptr[i] != at || c.row_ptr[i + 1] - c.row_ptr[i] != (int64_t)acc.size()) { ++bad; at = c.row_ptr[i + 1]; continue; }
        for (const auto &e : acc) {
            const float want = e.second.acc;
            const bool same = c.col_idx[at] == e.first && (std::memcmp(&c.vals[at], &want, 4) == 0 || (std::isnan(c.vals[at]) && std::isnan(want)));
            if (!same) {
                if (bad < 16) std::fprintf(stderr, "[row %lld] cpu: (%d, %g), gpu: (%d, %g)\n", (long long)i, e.first, want, c.col_idx[at], c.vals[at]);
                ++bad;
            }
            ++at;
        }
    }
    if (!out.empty()) {
        FILE *f = std::fopen(out.c_str(), "w");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 2; }
        std::fprintf(f, "%%%%MatrixMarket matrix coordinate real general\n%lld %lld %lld\n", (long long)rows, (long long)cols, (long long)nnz);
        for (int64_t i = 0; i < rows; ++i)
            for (int32_t k = c.row_ptr[i]; k < c.row_ptr[i + 1]; ++k) std::fprintf(f, "%lld %d %.9g\n", (long long)i + 1, c.col_idx[k] + 1, c.vals[k]);
        if (std::fclose(f) != 0) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 2; }
    }
    std::printf(bad ? "====== %lld MISMATCHES ======\n" : "========== OK ===========\n", (long long)bad);
    return bad ? 1 : 0;
}

// x = T^-1 ones through the C ABI against the contract of include/spmv_hip.h "the triangular solve", walked on the host
static int run_trsv(const HostCsr &a, bool upper, bool unit, const std::string &out)
{
    const int64_t n = a.rows;
    const int uplo = upper ? SPMV_TRSV_UPPER : SPMV_TRSV_LOWER;
    std::vector<float> b((size_t)n, 1.0f), x((size_t)n, NAN), ref((size_t)n, 0.0f);
    spmv_csr_t *A = nullptr;
    SPMV_CHECK(spmv_csr_create_host(a.rows, a.cols, a.nnz(), a.row_ptr.data(), a.col_idx.data(), a.vals.data(), &A));
    SPMV_CHECK(spmv_csr_trsv_plan(A, uplo, 0, nullptr));
    char line[256];
    SPMV_CHECK(spmv_csr_trsv_describe(A, uplo, line, (int)sizeof line));
    std::printf("spmv_csr_trsv: %s\n", line);
    float *d_b = nullptr, *d_x = nullptr;
    const size_t bytes = sizeof(float) * (size_t)(n ? n : 1);
    if (hipMalloc((void **)&d_b, bytes) != hipSuccess || hipMalloc((void **)&d_x, bytes) != hipSuccess ||
        hipMemcpy(d_b, b.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_x, x.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
        std::fprintf(stderr, "error: no device memory for b and x\n");
        return 2;
    }
    SPMV_CHECK(spmv_csr_trsv(A, uplo, unit ? SPMV_TRSV_UNIT : SPMV_TRSV_NON_UNIT, d_b, d_x, nullptr));
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(x.data(), d_x, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "error: the solve failed on the device\n");
        return 2;
    }
    (void)hipFree(d_b);
    (void)hipFree(d_x);
    SPMV_CHECK(spmv_csr_destroy(A));
    // the contract, row after row in dependency order (lower: ascending; upper: descending)
    for (int64_t step = 0; step < n; ++step) {
        const int64_t i = upper ? n - 1 - step : step;
        std::vector<int32_t> terms;
        float d = 1.0f;
        for (int32_t s = a.row_ptr[i]; s < a.row_ptr[i + 1]; ++s) {
            const int32_t c = a.col_idx[s];
            if (c == i) { if (!unit) d = a.vals[s]; }
            else if (upper ? c > i : c < i) terms.push_back(s);
        }
        float sum = 0.0f;
        if ((int64_t)terms.size() <= SPMV_TRSV_SERIAL_MAX) {
            for (int32_t s : terms) sum = std::fmaf(a.vals[s], ref[a.col_idx[s]], sum);
        } else {
            float p[64] = {};
            for (size_t t = 0; t < terms.size(); ++t) p[t % 64] = std::fmaf(a.vals[terms[t]], ref[a.col_idx[terms[t]]], p[t % 64]);
            for (int w = 32; w >= 1; w >>= 1)
                for (int l = 0; l < w; ++l) p[l] += p[l + w];
            sum = p[0];
        }
        const float num = b[i] - sum;
        ref[i] = unit ? num : num / d;
    }
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
        if (std::memcmp(&ref[i], &x[i], 4) != 0 && !(std::isnan(ref[i]) && std::isnan(x[i]))) {
            if (bad < 16) std::fprintf(stderr, "[row %lld] cpu: %.9g, gpu: %.9g\n", (long long)i, ref[i], x[i]);
            ++bad;
        }
    std::string err;
    if (!out.empty() && !(err = write_vector_text(out, x)).empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    std::printf(bad ? "====== %lld MISMATCHES ======\n" : "========== OK ===========\n", (long long)bad);
    return bad ? 1 : 0;
}

// M = ILU(0) of a through the C ABI against the contract of include/spmv_hip.h "the incomplete factorisation", walked on the host
static int run_ilu0(const HostCsr &a, const std::string &out)
{
    const int64_t n = a.rows, nnz = a.nnz();
    spmv_csr_t *A = nullptr, *M = nullptr;
    SPMV_CHECK(spmv_csr_create_host(a.rows, a.cols, nnz, a.row_ptr.data(), a.col_idx.data(), a.vals.data(), &A));
    SPMV_CHECK(spmv_csr_ilu0(A, 0, nullptr, &M));
    int64_t pivot = -1, info[8] = {};
    SPMV_CHECK(spmv_csr_ilu0_pivot(M, nullptr, &pivot));
    SPMV_CHECK(spmv_csr_trsv_plan_info(M, SPMV_TRSV_LOWER, info));
    std::printf("spmv_csr_ilu0: rows=%lld nnz=%lld levels=%lld launches=%lld pivot=%lld bytes=%lld\n", (long long)n, (long long)nnz,
                (long long)info[0], (long long)(info[1] + 1), (long long)pivot, (long long)spmv_csr_ilu0_plan_bytes(M));
    std::vector<float> m((size_t)nnz, NAN), ref(a.vals);
    float *d_m = nullptr;
    if (hipMalloc((void **)&d_m, sizeof(float) * (size_t)(nnz ? nnz : 1)) != hipSuccess) {
        std::fprintf(stderr, "error: no device memory for M's values\n");
        return 2;
    }
    SPMV_CHECK(spmv_csr_copy_arrays(M, nullptr, nullptr, d_m, nullptr));
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(m.data(), d_m, sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "error: the factorisation failed on the device\n");
        return 2;
    }
    (void)hipFree(d_m);
    SPMV_CHECK(spmv_csr_destroy(M));
    SPMV_CHECK(spmv_csr_destroy(A));
    // the contract, row after row
    std::vector<int32_t> diag((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t s = a.row_ptr[i]; s < a.row_ptr[i + 1]; ++s)
            if (a.col_idx[s] == i) diag[i] = s;
    int64_t ref_pivot = -1;
    for (int64_t i = 0; i < n; ++i) {
        for (int32_t p = a.row_ptr[i]; p < a.row_ptr[i + 1]; ++p) {
            const int32_t k = a.col_idx[p];
            if (k >= i) break;
            const float l = ref[p] / ref[diag[k]];
            ref[p] = l;
            int32_t r = p + 1;
            for (int32_t q = diag[k] + 1; q < a.row_ptr[k + 1]; ++q) {
                while (r < a.row_ptr[i + 1] && a.col_idx[r] < a.col_idx[q]) ++r;
                if (r < a.row_ptr[i + 1] && a.col_idx[r] == a.col_idx[q]) ref[r] = std::fmaf(-l, ref[q], ref[r]);
            }
        }
        const float u = ref[diag[i]];
        if (ref_pivot < 0 && (u == 0.0f || !std::isfinite(u))) ref_pivot = i;
    }
    int64_t bad = pivot == ref_pivot ? 0 : 1;
    if (bad) std::fprintf(stderr, "[pivot] cpu: %lld, gpu: %lld\n", (long long)ref_pivot, (long long)pivot);
    for (int64_t s = 0; s < nnz; ++s)
        if (std::memcmp(&ref[s], &m[s], 4) != 0 && !(std::isnan(ref[s]) && std::isnan(m[s]))) {
            if (bad < 16) std::fprintf(stderr, "[position %lld] cpu: %.9g, gpu: %.9g\n", (long long)s, ref[s], m[s]);
            ++bad;
        }
    std::string err;
    if (!out.empty() && !(err = write_vector_text(out, m)).empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    std::printf(bad ? "====== %lld MISMATCHES ======\n" : "========== OK ===========\n", (long long)bad);
    return bad ? 1 : 0;
}

// P A P^T by the colouring of a through the C ABI against the contract of include/spmv_hip.h "the multicolour ordering", walked on the host
static int run_color(const HostCsr &a, uint32_t seed, bool ilu0, const std::string &out)
{
    const int64_t n = a.rows, nnz = a.nnz();
    spmv_csr_t *A = nullptr, *B = nullptr;
    SPMV_CHECK(spmv_csr_create_host(a.rows, a.cols, nnz, a.row_ptr.data(), a.col_idx.data(), a.vals.data(), &A));
    int32_t *d_color = nullptr, *d_perm = nullptr;
    const size_t bytes = sizeof(int32_t) * (size_t)(n ? n : 1);
    if (hipMalloc((void **)&d_color, bytes) != hipSuccess || hipMalloc((void **)&d_perm, bytes) != hipSuccess) {
        std::fprintf(stderr, "error: no device memory for color and perm\n");
        return 2;
    }
    std::vector<int32_t> color((size_t)n, -1), perm((size_t)n, -1), color_ptr((size_t)n + 1, -1);
    int64_t info[8] = {}, lower[8] = {}, upper[8] = {};
    SPMV_CHECK(spmv_csr_color(A, seed, nullptr, d_color, d_perm, color_ptr.data(), (int)color_ptr.size(), info));
    SPMV_CHECK(spmv_csr_permute(A, d_perm, d_perm, 0, nullptr, &B));
    if (hipMemcpy(color.data(), d_color, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(perm.data(), d_perm, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "error: the colouring failed on the device\n");
        return 2;
    }
    (void)hipFree(d_color);
    (void)hipFree(d_perm);
    HostCsr b;
    b.rows = n; b.cols = n;
    b.row_ptr.resize((size_t)n + 1); b.col_idx.resize((size_t)nnz); b.vals.resize((size_t)nnz);
    SPMV_CHECK(spmv_csr_download(B, b.row_ptr.data(), b.col_idx.data(), b.vals.data()));
    SPMV_CHECK(spmv_csr_trsv_plan(B, SPMV_TRSV_LOWER, 0, nullptr));
    SPMV_CHECK(spmv_csr_trsv_plan(B, SPMV_TRSV_UPPER, 0, nullptr));
    SPMV_CHECK(spmv_csr_trsv_plan_info(B, SPMV_TRSV_LOWER, lower));
    SPMV_CHECK(spmv_csr_trsv_plan_info(B, SPMV_TRSV_UPPER, upper));
    SPMV_CHECK(spmv_csr_destroy(B));
    SPMV_CHECK(spmv_csr_destroy(A));
    std::printf("spmv_csr_color: rows=%lld colors=%lld rounds=%lld launches=%lld largest=%lld smallest=%lld\n", (long long)n, (long long)info[0],
                (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4]);
    std::printf("P A P^T: levels lower=%lld upper=%lld\n", (long long)lower[0], (long long)upper[0]);
    // the contract: the rows in descending key order take the smallest colour no coloured neighbour has
    auto key = [seed](uint32_t i) {
        uint32_t h = i ^ seed;
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        return h;
    };
    std::vector<std::vector<int32_t>> nb((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t s = a.row_ptr[i]; s < a.row_ptr[i + 1]; ++s)
            if (a.col_idx[s] != i) { nb[i].push_back(a.col_idx[s]); nb[a.col_idx[s]].push_back((int32_t)i); }
    std::vector<int32_t> by_key((size_t)n), ref((size_t)n, -1), round((size_t)n, 0);
    std::iota(by_key.begin(), by_key.end(), 0);
    std::sort(by_key.begin(), by_key.end(), [&](int32_t x, int32_t y) { return key((uint32_t)x) > key((uint32_t)y); });
    int64_t bad = 0, colors = 0, rounds = 0;
    for (int32_t i : by_key) {
        std::set<int32_t> used;
        int32_t r = 0;
        for (int32_t j : nb[i])
            if (ref[j] >= 0) { used.insert(ref[j]); r = std::max(r, round[j]); }
        int32_t c = 0;
        while (used.count(c)) ++c;
        ref[i] = c;
        round[i] = r + 1;
        colors = std::max<int64_t>(colors, c + 1);
        rounds = std::max<int64_t>(rounds, r + 1);
    }
    if (colors != info[0] || rounds != info[1]) {
        std::fprintf(stderr, "[counts] cpu: %lld colours in %lld rounds, gpu: %lld in %lld\n", (long long)colors, (long long)rounds, (long long)info[0], (long long)info[1]);
        ++bad;
    }
    for (int64_t i = 0; i < n; ++i)
        if (ref[i] != color[i]) {
            if (bad < 16) std::fprintf(stderr, "[row %lld] cpu: colour %d, gpu: %d\n", (long long)i, ref[i], color[i]);
            ++bad;
        }
    // perm: the rows by (colour, row); P A P^T: every row by (new column, position)
    std::vector<int32_t> want_perm((size_t)n), inv((size_t)n, 0);
    std::iota(want_perm.begin(), want_perm.end(), 0);
    std::stable_sort(want_perm.begin(), want_perm.end(), [&](int32_t x, int32_t y) { return ref[x] < ref[y]; });
    for (int64_t r = 0; r < n; ++r) {
        if (want_perm[r] != perm[r]) { if (bad < 16) std::fprintf(stderr, "[perm %lld] cpu: %d, gpu: %d\n", (long long)r, want_perm[r], perm[r]); ++bad; }
        inv[want_perm[r]] = (int32_t)r;
    }
    for (int64_t c = 0; c <= colors; ++c) {
        const int64_t start = std::lower_bound(want_perm.begin(), want_perm.end(), (int32_t)c, [&](int32_t x, int32_t v) { return ref[x] < v; }) - want_perm.begin();
        if (color_ptr[c] != start) { if (bad < 16) std::fprintf(stderr, "[color_ptr %lld] cpu: %lld, gpu: %d\n", (long long)c, (long long)start, color_ptr[c]); ++bad; }
    }
    int64_t at = 0;
    for (int64_t r = 0; r < n && bad == 0; ++r) {
        const int32_t old = want_perm[r];
        std::vector<std::pair<int32_t, int32_t>> e;
        for (int32_t s = a.row_ptr[old]; s < a.row_ptr[old + 1]; ++s) e.push_back({inv[a.col_idx[s]], s});
        std::sort(e.begin(), e.end());
        if (b.row_ptr[r] != at) ++bad;
        for (const auto &x : e) {
            if (b.col_idx[at] != x.first || std::memcmp(&b.vals[at], &a.vals[x.second], 4) != 0) {
                if (bad < 16) std::fprintf(stderr, "[P A P^T row %lld] cpu: (%d, %g), gpu: (%d, %g)\n", (long long)r, x.first, a.vals[x.second], b.col_idx[at], b.vals[at]);
                ++bad;
            }
            ++at;
        }
    }
    if (bad == 0 && b.row_ptr[n] != nnz) ++bad;
    if (!out.empty()) {
        FILE *f = std::fopen(out.c_str(), "w");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 2; }
        std::fprintf(f, "%%%%MatrixMarket matrix coordinate real general\n%lld %lld %lld\n", (long long)n, (long long)n, (long long)nnz);
        for (int64_t i = 0; i < n; ++i)
            for (int32_t k = b.row_ptr[i]; k < b.row_ptr[i + 1]; ++k) std::fprintf(f, "%lld %d %.9g\n", (long long)i + 1, b.col_idx[k] + 1, b.vals[k]);
        if (std::fclose(f) != 0) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 2; }
    }
    if (bad) {
        std::printf("====== %lld MISMATCHES ======\n", (long long)bad);
        return 1;
    }
    std::printf("color check ok\n");
    if (ilu0) return run_ilu0(b, "");
    std::printf("========== OK ===========\n");
    return 0;
}

static int run_file(int argc, char **argv)
{
    std::string mtx, bin, out, save, spgemm_b, add_b, add_op = "union", trsv, vname = "tiled";
    float alpha = 1.0f, beta = 1.0f;
    bool parse_only = false, transpose = false, unit = false, ilu0 = false, color = false;
    uint32_t seed = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--mtx") mtx = next();
        else if (a == "--csrbin") bin = next();
        else if (a == "--out") out = next();
        else if (a == "--save") save = next();
        else if (a == "--variant") vname = next();
        else if (a == "--parse-only") parse_only = true;
        else if (a == "--transpose") transpose = true;
        else if (a == "--spgemm") spgemm_b = next();
        else if (a == "--add") add_b = next();
        else if (a == "--alpha") alpha = std::strtof(next().c_str(), nullptr);
        else if (a == "--beta") beta = std::strtof(next().c_str(), nullptr);
        else if (a == "--op") add_op = next();
        else if (a == "--trsv") trsv = next();
        else if (a == "--unit") unit = true;
        else if (a == "--ilu0") ilu0 = true;
        else if (a == "--color") color = true;
        else if (a == "--seed") seed = (uint32_t)std::strtoul(next().c_str(), nullptr, 0);
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    HostCsr m;
    std::string err = !mtx.empty() ? read_matrix_market(mtx, m) : read_csr_binary(bin, m);
    if (!err.empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    std::printf("matrix %lld x %lld, nnz %lld\n", (long long)m.rows, (long long)m.cols, (long long)m.nnz());
    if (!save.empty() && !(err = write_csr_binary(save, m)).empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (parse_only) return 0;
    if (!spgemm_b.empty()) return run_spgemm(m, spgemm_b, out);
    if (!add_b.empty()) {
        const int op = add_op == "union" ? SPMV_ADD_UNION : add_op == "intersect" ? SPMV_ADD_INTERSECT : add_op == "minus" ? SPMV_ADD_MINUS : -1;
        if (op < 0) { std::fprintf(stderr, "unknown op %s (union, intersect or minus)\n", add_op.c_str()); return 2; }
        return run_add(m, add_b, alpha, beta, op, out);
    }
    if (!trsv.empty()) {
        if (trsv != "lower" && trsv != "upper") { std::fprintf(stderr, "unknown triangle %s (lower or upper)\n", trsv.c_str()); return 2; }
        if (m.rows != m.cols) { std::fprintf(stderr, "error: --trsv needs a square matrix\n"); return 2; }
        return run_trsv(m, trsv == "upper", unit, out);
    }
    if (color && m.rows != m.cols) { std::fprintf(stderr, "error: --color needs a square matrix\n"); return 2; }
    if (ilu0) {
        if (m.rows != m.cols) { std::fprintf(stderr, "error: --ilu0 needs a square matrix\n"); return 2; }
        for (int64_t i = 0; i < m.rows; ++i) {
            bool have = false;
            for (int32_t s = m.row_ptr[i]; s < m.row_ptr[i + 1]; ++s) have = have || m.col_idx[s] == i;
            if (!have) { std::fprintf(stderr, "error: --ilu0 needs a diagonal entry in every row (row %lld has none)\n", (long long)(i + 1)); return 2; }
        }
        if (!color) return run_ilu0(m, out);
    }
    if (color) return run_color(m, seed, ilu0, out);
    const int variant = variant_by_name(vname);
    if (variant < 0) { std::fprintf(stderr, "unknown variant %s\n", vname.c_str()); return 2; }

    const int64_t nx = transpose ? m.rows : m.cols, ny = transpose ? m.cols : m.rows;
    std::vector<float> x((size_t)nx, 1.0f), y((size_t)ny, NAN), ref((size_t)ny, 0.0f), mag((size_t)ny, 0.0f);
    for (int64_t r = 0; r < m.rows; ++r) {  // the harness's own CPU check, like SgemvCPU (tester.cpp:36-45)
        float acc = 0.0f, sum = 0.0f;
        for (int32_t k = m.row_ptr[r]; k < m.row_ptr[r + 1]; ++k) {
            if (transpose) {   // column sums in storage order: the order of T's rows
                ref[m.col_idx[k]] += x[r] * m.vals[k];
                mag[m.col_idx[k]] += std::fabs(m.vals[k]);
            } else {
                acc += x[m.col_idx[k]] * m.vals[k];
                sum += std::fabs(m.vals[k]);
            }
        }
        if (!transpose) { ref[r] = acc; mag[r] = sum; }
    }
    spmv_csr_t *A = nullptr, *T = nullptr;
    SPMV_CHECK(spmv_csr_create_host(m.rows, m.cols, m.nnz(), m.row_ptr.data(), m.col_idx.data(), m.vals.data(), &A));
    if (transpose) SPMV_CHECK(spmv_csr_transpose(A, 0, nullptr, &T));
    float ms = 0.0f;
    SPMV_CHECK(spmv_csr_run_host(transpose ? T : A, variant, x.data(), y.data(), &ms));
    std::printf("spmv_csr_run<%s>%s took %g ms\n", spmv_variant_name(variant), transpose ? " on the transpose" : "", ms);
    SPMV_CHECK(spmv_csr_destroy(T));
    SPMV_CHECK(spmv_csr_destroy(A));
    int bad = 0;
    for (int64_t r = 0; r < ny; ++r) {
        if (!(std::fabs(ref[r] - y[r]) <= 1e-5f * mag[r] + 1e-30f)) {
            if (bad < 16) std::fprintf(stderr, "[row %lld] cpu: %g, gpu: %g\n", (long long)r, ref[r], y[r]);
            ++bad;
        }
    }
    if (!out.empty() && !(err = write_vector_text(out, y)).empty()) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    std::printf(bad ? "====== %d MISMATCHES ======\n" : "========== OK ===========\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::strncmp(argv[1], "--", 2) == 0) return run_file(argc, argv);
    int m = 4096, n = 4096;
    if (argc >= 3) { m = std::atoi(argv[1]); n = std::atoi(argv[2]); }
    SparseSgemvTester tester(m, n);
    tester.RunTest();
    return tester.Mismatches() == 0 ? 0 : 1;
}
