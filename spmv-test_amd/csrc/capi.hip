// capi.hip -- the extern "C" entry points of include/spmv_hip.h.
#include <cctype>
#include <cstdarg>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include "spmv_internal.hpp"

namespace spmv {

static thread_local char g_err[512] = "";
static thread_local float g_first_launch_ms = 0.0f;   // the FIRST (cold) launch of the last *_run_host call on this thread

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    set_error("HIP error %s:%d: %s (%s)", file, line, hipGetErrorString(e), what);
    return SPMV_ERR_HIP;
}

static int require_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device visible (hipGetDeviceCount: %s); libspmv_hip has no CPU path",
                  e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return SPMV_ERR_NO_DEVICE;
    }
    return SPMV_OK;
}

int LdsOptIn::ensure(const void *fn, int device, int bytes)
{
    const uint64_t bit = (device >= 0 && device < 64) ? (1ull << device) : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return SPMV_OK;
    SPMV_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (bit) done.fetch_or(bit, std::memory_order_release);
    return SPMV_OK;
}

int device_cus(int device)
{
    static std::atomic<int> cache[64];
    const bool cached = device >= 0 && device < 64;
    if (cached) {
        const int c = cache[device].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    if (cached) cache[device].store(cus, std::memory_order_relaxed);
    return cus;
}

int require_current(int device, const char *what)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipGetDevice failed", what);
        return SPMV_ERR_HIP;
    }
    if (cur != device) {
        set_error("%s: the handle lives on device %d but the current device is %d (hipSetDevice first)", what, device, cur);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// Is `dtype` one a call takes -- SPMV_ATTN_BF16, SPMV_ATTN_FP16 and, with fp32_too, SPMV_ATTN_FP32?  Else `what`'s refusal.
static int dtype_ok(int dtype, bool fp32_too, const char *what)
{
    if (dtype == SPMV_ATTN_BF16 || dtype == SPMV_ATTN_FP16 || (fp32_too && dtype == SPMV_ATTN_FP32)) return SPMV_OK;
    if (fp32_too)
        set_error("%s: dtype = %d (need SPMV_ATTN_FP32 = %d, SPMV_ATTN_BF16 = %d or SPMV_ATTN_FP16 = %d)", what, dtype, (int)SPMV_ATTN_FP32,
                  (int)SPMV_ATTN_BF16, (int)SPMV_ATTN_FP16);
    else set_error("%s: dtype = %d (need SPMV_ATTN_BF16 = %d or SPMV_ATTN_FP16 = %d)", what, dtype, (int)SPMV_ATTN_BF16, (int)SPMV_ATTN_FP16);
    return SPMV_ERR_INVALID;
}

// f(E{}) for the element type E that a dtype accepted by dtype_ok names: float, bf16 or fp16
template <typename F>
static int with_element(int dtype, F &&f)
{
    return dtype == SPMV_ATTN_FP32 ? f(float{}) : dtype == SPMV_ATTN_BF16 ? f(bf16{}) : f(fp16{});
}

// The host-buffer conveniences time two launches: the reference's TIME_KERNEL (kernel.hpp:31-48) times a single COLD
// launch, code object load included -- that figure is kept (spmv_last_first_launch_ms); *kernel_ms is the second launch:
// the kernel.  Each launch runs on the null stream and is followed by a device synchronisation.
template <typename Launch>
static int time_cold_then_warm(const Launch &launch, float *kernel_ms)
{
    hipEvent_t ev[2] = {nullptr, nullptr};
    const int rc = [&]() -> int {
        SPMV_HIP_TRY(hipEventCreate(&ev[0]));
        SPMV_HIP_TRY(hipEventCreate(&ev[1]));
        float ms = 0.0f;
        for (int i = 0; i < 2; ++i) {
            SPMV_HIP_TRY(hipEventRecord(ev[0], nullptr));
            const int r = launch();
            SPMV_HIP_TRY(hipEventRecord(ev[1], nullptr));
            SPMV_HIP_TRY(hipEventSynchronize(ev[1]));
            if (r) return r;
            SPMV_HIP_TRY(hipEventElapsedTime(i == 0 ? &g_first_launch_ms : &ms, ev[0], ev[1]));
            SPMV_HIP_TRY(hipDeviceSynchronize());
        }
        if (kernel_ms) *kernel_ms = ms;
        return SPMV_OK;
    }();
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

int spmv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *spmv_last_error(void) { return g_err; }

float spmv_last_first_launch_ms(void) { return g_first_launch_ms; }

int spmv_debug_bounds(int64_t *records, int n)
{
#if defined(SPMV_CHECK_BOUNDS)
    if (n < 0 || (n > 0 && !records)) {
        spmv::set_error("spmv_debug_bounds: n = %d records at %p", n, (void *)records);
        return SPMV_ERR_INVALID;
    }
    unsigned long long t[spmv::kBoundsSites][2] = {};
    if (int rc = spmv::bounds_collect_binned(t)) return rc;
    if (int rc = spmv::bounds_collect_panel(t)) return rc;
    int hit = 0;
    for (int i = 0; i < spmv::kBoundsSites; ++i) {
        if (t[i][0] == 0) continue;
        if (hit < n) {
            records[3 * hit] = i;
            records[3 * hit + 1] = (int64_t)t[i][0];
            records[3 * hit + 2] = (int64_t)t[i][1];
        }
        ++hit;
    }
    return hit;
#else
    (void)records;
    (void)n;
    spmv::set_error("spmv_debug_bounds: not instrumented (this is the normal build; lib/libspmv_hip_checked.so is the checked one)");
    return SPMV_ERR_INVALID;
#endif
}

const char *spmv_variant_name(int variant)
{
    switch (variant) {
        case SPMV_SCALAR: return "scalar";
        case SPMV_WAVE: return "wave";
        case SPMV_WAVE_PIPE: return "wave_pipe";
        case SPMV_VECTOR: return "vector";
        case SPMV_ADAPTIVE: return "adaptive";
        case SPMV_TILED: return "tiled";
        case SPMV_PANEL: return "panel";
        case SPMV_AUTO: return "auto";
        case SPMV_XSKIP: return "xskip";
        default: return "unknown";
    }
}

static int check_dims(int64_t rows, int64_t cols, int64_t nnz)
{
    if (rows < 0 || cols < 0 || nnz < 0 || rows >= (1LL << 31) || cols >= (1LL << 31) || nnz >= (1LL << 31)) {
        set_error("bad dimensions rows=%lld cols=%lld nnz=%lld (each must be in [0, 2^31))", (long long)rows,
                  (long long)cols, (long long)nnz);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

int spmv_csr_validate(const spmv_csr_t *h, void *stream)
{
    if (!h) { set_error("spmv_csr_validate: null handle"); return SPMV_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    const int32_t init[4] = {INT32_MAX, INT32_MAX, 0, (int32_t)h->nnz};
    int32_t bad[4];
    DevPtr<int32_t> d_bad;
    SPMV_HIP_TRY(d_bad.alloc(4));
    SPMV_HIP_TRY(hipMemcpyAsync(d_bad.get(), init, sizeof init, hipMemcpyHostToDevice, st));
    int rc = launch_validate(h, d_bad.get(), st);
    if (rc) return rc;
    SPMV_HIP_TRY(hipMemcpyAsync(bad, d_bad.get(), sizeof bad, hipMemcpyDeviceToHost, st));
    SPMV_HIP_TRY(hipStreamSynchronize(st));
    if (bad[2] != 0 || (int64_t)bad[3] != h->nnz) {
        set_error("malformed CSR: row_ptr[0]=%d row_ptr[rows]=%d, expected 0 and nnz=%lld", bad[2], bad[3],
                  (long long)h->nnz);
        return SPMV_ERR_INVALID;
    }
    if (bad[0] != INT32_MAX) {
        set_error("malformed CSR: row_ptr decreases or leaves [0, nnz] at row %d", bad[0]);
        return SPMV_ERR_INVALID;
    }
    if (bad[1] != INT32_MAX) {
        set_error("malformed CSR: column index of element %d is outside [0, %lld)", bad[1], (long long)h->cols);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

int spmv_csr_create_host(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr,
                         const int32_t *col_idx, const float *vals, spmv_csr_t **out)
{
    if (!out || !row_ptr || (nnz > 0 && (!col_idx || !vals))) {
        set_error("spmv_csr_create_host: null argument");
        return SPMV_ERR_INVALID;
    }
    int rc = check_dims(rows, cols, nnz);
    if (rc) return rc;
    if ((rc = require_device())) return rc;
    if (row_ptr[0] != 0 || row_ptr[rows] != nnz) {
        set_error("spmv_csr_create_host: row_ptr[0]=%d row_ptr[rows]=%d, expected 0 and nnz=%lld", row_ptr[0],
                  row_ptr[rows], (long long)nnz);
        return SPMV_ERR_INVALID;
    }
    DevPtr<int32_t> rp, ci;
    DevPtr<float> va;
    SPMV_HIP_TRY(rp.alloc((size_t)rows + 1));
    SPMV_HIP_TRY(ci.alloc((size_t)nnz));
    SPMV_HIP_TRY(va.alloc((size_t)nnz));
    SPMV_HIP_TRY(hipMemcpy(rp.get(), row_ptr, sizeof(int32_t) * ((size_t)rows + 1), hipMemcpyHostToDevice));
    if (nnz > 0) {
        SPMV_HIP_TRY(hipMemcpy(ci.get(), col_idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
        SPMV_HIP_TRY(hipMemcpy(va.get(), vals, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice));
    }
    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("out of host memory"); return SPMV_ERR_INVALID; }
    h->rows = rows; h->cols = cols; h->nnz = nnz;
    if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
    h->d_row_ptr = rp; h->d_col_idx = ci; h->d_vals = va;
    h->own_row_ptr = std::move(rp); h->own_col_idx = std::move(ci); h->own_vals = std::move(va);
    if ((rc = spmv_csr_validate(h, nullptr))) {
        spmv_csr_destroy(h);
        return rc;
    }
    *out = h;
    return SPMV_OK;
}

int spmv_csr_create_device(int64_t rows, int64_t cols, int64_t nnz, const int32_t *d_row_ptr,
                           const int32_t *d_col_idx, const float *d_vals, spmv_csr_t **out)
{
    if (!out || !d_row_ptr || (nnz > 0 && (!d_col_idx || !d_vals))) {
        set_error("spmv_csr_create_device: null argument");
        return SPMV_ERR_INVALID;
    }
    int rc = check_dims(rows, cols, nnz);
    if (rc) return rc;
    if ((rc = require_device())) return rc;
    if (!aligned16(d_col_idx) || !aligned16(d_vals)) {
        set_error("spmv_csr_create_device: col_idx and vals must be 16-byte aligned");
        return SPMV_ERR_INVALID;
    }
    spmv_csr *h = new (std::nothrow) spmv_csr();
    if (!h) { set_error("out of host memory"); return SPMV_ERR_INVALID; }
    h->rows = rows; h->cols = cols; h->nnz = nnz;
    h->d_row_ptr = d_row_ptr; h->d_col_idx = d_col_idx; h->d_vals = d_vals;
    if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
    if ((rc = spmv_csr_validate(h, nullptr))) {
        delete h;
        return rc;
    }
    *out = h;
    return SPMV_OK;
}

int spmv_csr_from_dense_device(int M, int N, const float *d_A, void *stream, spmv_csr_t **out)
{
    if (!out || M < 0 || N < 0 || (!d_A && (int64_t)M * N > 0)) {
        set_error("spmv_csr_from_dense_device: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    return dense_to_csr(M, N, d_A, (hipStream_t)stream, out);
}

int spmv_csr_from_dense_host(int M, int N, const float *A_host, void *stream, spmv_csr_t **out)
{
    if (!out || M < 0 || N < 0 || (!A_host && (int64_t)M * N > 0)) {
        set_error("spmv_csr_from_dense_host: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    const size_t bytes = sizeof(float) * (size_t)M * (size_t)N;
    DevPtr<float> dA;
    SPMV_HIP_TRY(dA.alloc((size_t)M * (size_t)N));
    SPMV_HIP_TRY(hipMemcpyAsync(dA.get(), A_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = dense_to_csr(M, N, dA.get(), (hipStream_t)stream, out);
    (void)hipStreamSynchronize((hipStream_t)stream);
    return rc;
}

int spmv_csr_download(const spmv_csr_t *h, int32_t *row_ptr, int32_t *col_idx, float *vals)
{
    if (!h) { set_error("spmv_csr_download: null handle"); return SPMV_ERR_INVALID; }
    if (row_ptr)
        SPMV_HIP_TRY(hipMemcpy(row_ptr, h->d_row_ptr, sizeof(int32_t) * ((size_t)h->rows + 1), hipMemcpyDeviceToHost));
    if (col_idx && h->nnz)
        SPMV_HIP_TRY(hipMemcpy(col_idx, h->d_col_idx, sizeof(int32_t) * (size_t)h->nnz, hipMemcpyDeviceToHost));
    if (vals && h->nnz)
        SPMV_HIP_TRY(hipMemcpy(vals, h->d_vals, sizeof(float) * (size_t)h->nnz, hipMemcpyDeviceToHost));
    return SPMV_OK;
}

int spmv_csr_dims(const spmv_csr_t *h, int64_t *rows, int64_t *cols, int64_t *nnz)
{
    if (!h) { set_error("spmv_csr_dims: null handle"); return SPMV_ERR_INVALID; }
    if (rows) *rows = h->rows;
    if (cols) *cols = h->cols;
    if (nnz) *nnz = h->nnz;
    return SPMV_OK;
}

int spmv_csr_column_range(const spmv_csr_t *h, int64_t *col_min, int64_t *col_max, void *stream)
{
    if (!h || !col_min || !col_max) { set_error("spmv_csr_column_range: null argument"); return SPMV_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    DevPtr<int32_t> d;
    SPMV_HIP_TRY(d.alloc(2));
    int rc = launch_column_range(*h, d.get(), st);
    if (rc) return rc;
    int32_t out[2] = {0, 0};
    SPMV_HIP_TRY(hipMemcpyAsync(out, d.get(), sizeof out, hipMemcpyDeviceToHost, st));
    SPMV_HIP_TRY(hipStreamSynchronize(st));
    *col_min = out[1] < 0 ? h->cols : (int64_t)out[0];
    *col_max = (int64_t)out[1];
    return SPMV_OK;
}

int spmv_csr_destroy(spmv_csr_t *h)
{
    if (!h) return SPMV_OK;
    int rc = SPMV_OK;
    for (hipError_t e : {h->own_row_ptr.reset(), h->own_col_idx.reset(), h->own_vals.reset()})
        if (e != hipSuccess) rc = SPMV_ERR_HIP;
    delete h;
    if (rc) set_error("hipFree failed in spmv_csr_destroy");
    return rc;
}

int spmv_csr_transpose(const spmv_csr_t *a, int keep_map, void *stream, spmv_csr_t **out)
{
    if (!a || !out) { set_error("spmv_csr_transpose: null argument"); return SPMV_ERR_INVALID; }
    if (keep_map != 0 && keep_map != 1) {
        set_error("spmv_csr_transpose: keep_map = %d (0 or 1)", keep_map);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_device()) return rc;
    if (int rc = require_current(a->device, "spmv_csr_transpose")) return rc;
    return transpose(*a, keep_map == 1, (hipStream_t)stream, out);
}

// ---- the companions of a derived handle: _values, _gather / _scatter, _map_bytes ------------------------------------------
// One description per maker of what its companions' checks say differently; the checks themselves are written once below, and
// fire in one order for every maker.
struct Companions {
    MapMaker maker;             // whose map the calls take (none: spmv_csr_add, whose plan stands in the map's place)
    char letter;                // the handle's name in a message
    const char *missing;        // the refusal of a handle without that map or plan
    const char *parent;         // _values: how a message introduces the parent's shape
    bool stride_names_nnz;      // the dst_stride refusal says "is below nnz = ...", not "is below the ... words of an array"
};
static const Companions kOfTranspose = {MapMaker::transpose, 't', "the handle has no map (it was not made by spmv_csr_transpose with keep_map = 1)",
                                        "the transpose of t would be", true};
static const Companions kOfSelect = {MapMaker::select, 's', "the handle has no map (it was not made by a spmv_csr_select call with keep_map = 1)",
                                     "s was selected from", false};
static const Companions kOfPermute = {MapMaker::permute, 'b', "the handle has no map (it was not made by spmv_csr_permute with SPMV_PERMUTE_KEEP_MAP)",
                                      "b was permuted from", true};
static const Companions kOfAdd = {MapMaker::none, 'c', "the handle has no plan (it was not made by spmv_csr_add with keep_plan = 1)", nullptr, false};

static bool made_by(const Companions &m, const spmv_csr_t *h)
{
    return m.maker == MapMaker::none ? h->plan_add.ready : h->map.maker == m.maker;
}

// What every strided move refuses; nothing is launched before it has passed.  side: spmv_csr_add_gather's, null for the maps;
// scatter: dst is in the parent's order.
static int move_check(const char *what, const Companions &m, const spmv_csr_t *h, const int *side, bool scatter, int count,
                      const void *d_src, int64_t src_stride, const void *d_dst, int64_t dst_stride)
{
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (!made_by(m, h)) { set_error("%s: %s", what, m.missing); return SPMV_ERR_INVALID; }
    if (side && *side != 0 && *side != 1) { set_error("%s: side = %d (0: a, 1: b)", what, *side); return SPMV_ERR_INVALID; }
    if (count < 1) { set_error("%s: count = %d (need count >= 1)", what, count); return SPMV_ERR_INVALID; }
    if ((!d_src || !d_dst) && h->nnz > 0) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(d_src) % 4 != 0 || reinterpret_cast<uintptr_t>(d_dst) % 4 != 0) {
        set_error("%s: src and dst must be 4-byte aligned", what);
        return SPMV_ERR_INVALID;
    }
    if (src_stride < 0 || dst_stride < 0) {
        set_error("%s: src_stride = %lld, dst_stride = %lld (a stride is not negative)", what, (long long)src_stride, (long long)dst_stride);
        return SPMV_ERR_INVALID;
    }
    if (src_stride > INT64_MAX / 4 / count || dst_stride > INT64_MAX / 4 / count) {
        set_error("%s: a stride overflows 64-bit byte offsets", what);
        return SPMV_ERR_INVALID;
    }
    // words of one array of dst
    const int64_t dst_len = side ? (*side ? h->plan_add.b_nnz : h->plan_add.a_nnz) : scatter ? h->map.parent_len : h->nnz;
    if (count > 1 && dst_stride < dst_len) {
        if (m.stride_names_nnz)
            set_error("%s: dst_stride = %lld is below nnz = %lld with count = %d", what, (long long)dst_stride, (long long)dst_len, count);
        else
            set_error("%s: dst_stride = %lld is below the %lld words of an array with count = %d", what, (long long)dst_stride,
                      (long long)dst_len, count);
        return SPMV_ERR_INVALID;
    }
    return require_current(h->device, what);
}

// a gather or a scatter through h's own map
static int map_move_checked(const char *what, const Companions &m, const spmv_csr_t *h, bool scatter, int count, const void *d_src,
                            int64_t src_stride, void *d_dst, int64_t dst_stride, void *stream)
{
    if (int rc = move_check(what, m, h, nullptr, scatter, count, d_src, src_stride, d_dst, dst_stride)) return rc;
    return map_move(h->map, h->nnz, scatter, count, d_src, src_stride, d_dst, dst_stride, (hipStream_t)stream);
}

// h's values again from its parent's (one parent, through h's map), and what spmv_csr_values_changed does
static int map_values(const char *what, const Companions &m, spmv_csr_t *h, const spmv_csr_t *a, void *stream)
{
    if (!h || !a) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (!made_by(m, h)) { set_error("%s: %s", what, m.missing); return SPMV_ERR_INVALID; }
    if (a == h) {
        set_error("%s: a is %c itself (%c's values would be read while they are written)", what, m.letter, m.letter);
        return SPMV_ERR_INVALID;
    }
    const bool transposed = m.maker == MapMaker::transpose;
    const int64_t rows = transposed ? h->cols : h->rows, cols = transposed ? h->rows : h->cols;
    if (a->rows != rows || a->cols != cols || a->nnz != h->map.parent_len) {
        set_error("%s: a is %lld x %lld with %lld nonzeros, %s %lld x %lld with %lld", what, (long long)a->rows, (long long)a->cols,
                  (long long)a->nnz, m.parent, (long long)rows, (long long)cols, (long long)h->map.parent_len);
        return SPMV_ERR_INVALID;
    }
    if (m.maker == MapMaker::permute && a->nnz > 0 && !a->d_vals) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, what)) return rc;
    if (a->device != h->device) {
        set_error("%s: a lives on device %d, %c on device %d", what, a->device, m.letter, h->device);
        return SPMV_ERR_INVALID;
    }
    const hipStream_t s = (hipStream_t)stream;
    // (the transpose's values land in the library's own allocation: four words per lane, kernels_transpose.hip)
    if (int rc = transposed ? transpose_values(*h, *a, s) : map_move(h->map, h->nnz, false, 1, a->d_vals, 0, h->own_vals.get(), 0, s))
        return rc;
    ++h->values_gen;
    return SPMV_OK;
}

static int64_t map_bytes(const char *what, const Companions &m, const spmv_csr_t *h)
{
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    return h->map.maker == m.maker ? 4 * h->nnz : 0;
}

int spmv_csr_transpose_values(spmv_csr_t *t, const spmv_csr_t *a, void *stream)
{
    return map_values("spmv_csr_transpose_values", kOfTranspose, t, a, stream);
}

int spmv_csr_transpose_gather(const spmv_csr_t *t, int count, const void *d_src, int64_t src_stride, void *d_dst, int64_t dst_stride,
                              void *stream)
{
    return map_move_checked("spmv_csr_transpose_gather", kOfTranspose, t, false, count, d_src, src_stride, d_dst, dst_stride, stream);
}

int64_t spmv_csr_transpose_map_bytes(const spmv_csr_t *t) { return map_bytes("spmv_csr_transpose_map_bytes", kOfTranspose, t); }

// ---- selection (kernels_select.hip) ------------------------------------------------------------------------------------
// what spmv_csr_select_topk and _threshold refuse alike; nothing is launched before it has passed
static int select_check(const char *what, const spmv_csr_t *a, const float *d_score, int flags, int keep_map, spmv_csr_t **out)
{
    if (!a || !out) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (flags & ~SPMV_SELECT_ABS) { set_error("%s: flags = 0x%x (SPMV_SELECT_ABS or 0)", what, (unsigned)flags); return SPMV_ERR_INVALID; }
    if (keep_map != 0 && keep_map != 1) { set_error("%s: keep_map = %d (0 or 1)", what, keep_map); return SPMV_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(d_score) % 4 != 0) { set_error("%s: d_score must be 4-byte aligned", what); return SPMV_ERR_INVALID; }
    if (int rc = require_device()) return rc;
    return require_current(a->device, what);
}

int spmv_csr_select_topk(const spmv_csr_t *a, const float *d_score, int k, int flags, int keep_map, void *stream, spmv_csr_t **out)
{
    const char *what = "spmv_csr_select_topk";
    if (a && out && k < 1) { set_error("%s: k = %d (need k >= 1)", what, k); return SPMV_ERR_INVALID; }
    if (int rc = select_check(what, a, d_score, flags, keep_map, out)) return rc;
    return select(*a, d_score, false, k, 0u, (flags & SPMV_SELECT_ABS) != 0, keep_map == 1, (hipStream_t)stream, out);
}

int spmv_csr_select_threshold(const spmv_csr_t *a, const float *d_score, float threshold, int flags, int keep_map, void *stream,
                              spmv_csr_t **out)
{
    const char *what = "spmv_csr_select_threshold";
    if (a && out && threshold != threshold) { set_error("%s: the threshold is a NaN", what); return SPMV_ERR_INVALID; }
    if (int rc = select_check(what, a, d_score, flags, keep_map, out)) return rc;
    // (|s| >= t and s >= t are comparisons of keys: the key of the threshold itself is never taken from |t|)
    return select(*a, d_score, true, 0, select_key(threshold, false), (flags & SPMV_SELECT_ABS) != 0, keep_map == 1,
                  (hipStream_t)stream, out);
}

int spmv_csr_select_values(spmv_csr_t *s, const spmv_csr_t *a, void *stream)
{
    return map_values("spmv_csr_select_values", kOfSelect, s, a, stream);
}

int spmv_csr_select_gather(const spmv_csr_t *s, int count, const void *d_src, int64_t src_stride, void *d_dst, int64_t dst_stride,
                           void *stream)
{
    return map_move_checked("spmv_csr_select_gather", kOfSelect, s, false, count, d_src, src_stride, d_dst, dst_stride, stream);
}

int spmv_csr_select_scatter(const spmv_csr_t *s, int count, const void *d_src, int64_t src_stride, void *d_dst, int64_t dst_stride,
                            void *stream)
{
    return map_move_checked("spmv_csr_select_scatter", kOfSelect, s, true, count, d_src, src_stride, d_dst, dst_stride, stream);
}

int64_t spmv_csr_select_map_bytes(const spmv_csr_t *s) { return map_bytes("spmv_csr_select_map_bytes", kOfSelect, s); }

int spmv_csr_copy_arrays(const spmv_csr_t *h, int32_t *d_row_ptr, int32_t *d_col_idx, float *d_vals, void *stream)
{
    const char *what = "spmv_csr_copy_arrays";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, what)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (d_row_ptr)
        SPMV_HIP_TRY(hipMemcpyAsync(d_row_ptr, h->d_row_ptr, sizeof(int32_t) * ((size_t)h->rows + 1), hipMemcpyDeviceToDevice, st));
    if (d_col_idx && h->nnz)
        SPMV_HIP_TRY(hipMemcpyAsync(d_col_idx, h->d_col_idx, sizeof(int32_t) * (size_t)h->nnz, hipMemcpyDeviceToDevice, st));
    if (d_vals && h->nnz)
        SPMV_HIP_TRY(hipMemcpyAsync(d_vals, h->d_vals, sizeof(float) * (size_t)h->nnz, hipMemcpyDeviceToDevice, st));
    return SPMV_OK;
}

// ---- the sparse product (kernels_spgemm.hip) ------------------------------------------------------------------------------
int spmv_csr_spgemm(const spmv_csr_t *a, const spmv_csr_t *b, int keep_plan, void *stream, spmv_csr_t **out, int64_t *products)
{
    const char *what = "spmv_csr_spgemm";
    if (!a || !b || !out) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (a->cols != b->rows) {
        set_error("%s: a is %lld x %lld, b is %lld x %lld (a.cols must be b.rows)", what, (long long)a->rows, (long long)a->cols,
                  (long long)b->rows, (long long)b->cols);
        return SPMV_ERR_INVALID;
    }
    if (keep_plan != 0 && keep_plan != 1) { set_error("%s: keep_plan = %d (0 or 1)", what, keep_plan); return SPMV_ERR_INVALID; }
    if (int rc = require_device()) return rc;
    if (a->device != b->device) {
        set_error("%s: a lives on device %d, b on device %d", what, a->device, b->device);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(a->device, what)) return rc;
    return spgemm(*a, *b, keep_plan == 1, (hipStream_t)stream, out, products);
}

int spmv_csr_spgemm_values(spmv_csr_t *c, const spmv_csr_t *a, const spmv_csr_t *b, void *stream)
{
    const char *what = "spmv_csr_spgemm_values";
    if (!c || !a || !b) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    const SpgemmPlan &p = c->plan_spgemm;
    if (!p.ready || !c->own_vals) {
        set_error("%s: the handle has no plan (it was not made by spmv_csr_spgemm with keep_plan = 1)", what);
        return SPMV_ERR_INVALID;
    }
    if (a == c || b == c) {
        set_error("%s: %s is c itself (c's values would be read while they are written)", what, a == c ? "a" : "b");
        return SPMV_ERR_INVALID;
    }
    if (a->rows != c->rows || a->cols != p.inner || b->rows != p.inner || b->cols != c->cols || a->nnz != p.a_nnz || b->nnz != p.b_nnz) {
        set_error("%s: a is %lld x %lld with %lld nonzeros and b %lld x %lld with %lld, c was made from %lld x %lld with %lld and "
                  "%lld x %lld with %lld", what, (long long)a->rows, (long long)a->cols, (long long)a->nnz, (long long)b->rows,
                  (long long)b->cols, (long long)b->nnz, (long long)c->rows, (long long)p.inner, (long long)p.a_nnz, (long long)p.inner,
                  (long long)c->cols, (long long)p.b_nnz);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(c->device, what)) return rc;
    if (a->device != c->device || b->device != c->device) {
        set_error("%s: a lives on device %d, b on device %d, c on device %d", what, a->device, b->device, c->device);
        return SPMV_ERR_INVALID;
    }
    if (int rc = spgemm_values(*c, *a, *b, (hipStream_t)stream)) return rc;
    ++c->values_gen;
    return SPMV_OK;
}

int64_t spmv_csr_spgemm_plan_bytes(const spmv_csr_t *c)
{
    if (!c) { set_error("spmv_csr_spgemm_plan_bytes: null handle"); return SPMV_ERR_INVALID; }
    return spgemm_plan_bytes(*c);
}

// ---- the sparse sum (kernels_add.hip) ----------------------------------------------------------------------------------------
int spmv_csr_add(const spmv_csr_t *a, const spmv_csr_t *b, float alpha, float beta, int op, int keep_plan, void *stream, spmv_csr_t **out)
{
    const char *what = "spmv_csr_add";
    if (!a || !b || !out) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (a->rows != b->rows || a->cols != b->cols) {
        set_error("%s: a is %lld x %lld, b is %lld x %lld (the shapes must be equal)", what, (long long)a->rows, (long long)a->cols,
                  (long long)b->rows, (long long)b->cols);
        return SPMV_ERR_INVALID;
    }
    if (op != SPMV_ADD_UNION && op != SPMV_ADD_INTERSECT && op != SPMV_ADD_MINUS) {
        set_error("%s: op = %d (SPMV_ADD_UNION, SPMV_ADD_INTERSECT or SPMV_ADD_MINUS)", what, op);
        return SPMV_ERR_INVALID;
    }
    if (keep_plan != 0 && keep_plan != 1) { set_error("%s: keep_plan = %d (0 or 1)", what, keep_plan); return SPMV_ERR_INVALID; }
    if (int rc = require_device()) return rc;
    if (a->device != b->device) {
        set_error("%s: a lives on device %d, b on device %d", what, a->device, b->device);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(a->device, what)) return rc;
    return add(*a, *b, alpha, beta, op, keep_plan == 1, (hipStream_t)stream, out);
}

int spmv_csr_add_values(spmv_csr_t *c, const spmv_csr_t *a, const spmv_csr_t *b, float alpha, float beta, void *stream)
{
    const char *what = "spmv_csr_add_values";
    if (!c || !a || !b) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    const AddPlan &p = c->plan_add;
    if (!p.ready || !c->own_vals) {
        set_error("%s: the handle has no plan (it was not made by spmv_csr_add with keep_plan = 1)", what);
        return SPMV_ERR_INVALID;
    }
    if (a == c || b == c) {
        set_error("%s: %s is c itself (c's values would be read while they are written)", what, a == c ? "a" : "b");
        return SPMV_ERR_INVALID;
    }
    if (a->rows != c->rows || a->cols != c->cols || b->rows != c->rows || b->cols != c->cols || a->nnz != p.a_nnz || b->nnz != p.b_nnz) {
        set_error("%s: a is %lld x %lld with %lld nonzeros and b %lld x %lld with %lld, c was made from two %lld x %lld operands with "
                  "%lld and %lld", what, (long long)a->rows, (long long)a->cols, (long long)a->nnz, (long long)b->rows, (long long)b->cols,
                  (long long)b->nnz, (long long)c->rows, (long long)c->cols, (long long)p.a_nnz, (long long)p.b_nnz);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(c->device, what)) return rc;
    if (a->device != c->device || b->device != c->device) {
        set_error("%s: a lives on device %d, b on device %d, c on device %d", what, a->device, b->device, c->device);
        return SPMV_ERR_INVALID;
    }
    if (int rc = add_values(*c, *a, *b, alpha, beta, (hipStream_t)stream)) return rc;
    ++c->values_gen;
    return SPMV_OK;
}

int spmv_csr_add_gather(const spmv_csr_t *c, int side, int count, const void *d_src, int64_t src_stride, void *d_dst, int64_t dst_stride,
                        void *stream)
{
    if (int rc = move_check("spmv_csr_add_gather", kOfAdd, c, &side, false, count, d_src, src_stride, d_dst, dst_stride)) return rc;
    return add_gather(*c, side, count, d_src, src_stride, d_dst, dst_stride, (hipStream_t)stream);
}

int64_t spmv_csr_add_plan_bytes(const spmv_csr_t *c)
{
    if (!c) { set_error("spmv_csr_add_plan_bytes: null handle"); return SPMV_ERR_INVALID; }
    return add_plan_bytes(*c);
}

// ---- the triangular solve (kernels_trsv.hip) -------------------------------------------------------------------------------
// what every trsv entry point checks of its handle and uplo
static int trsv_check(const spmv_csr_t *h, int uplo, const char *what)
{
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (uplo != SPMV_TRSV_LOWER && uplo != SPMV_TRSV_UPPER) {
        set_error("%s: uplo = %d (SPMV_TRSV_LOWER or SPMV_TRSV_UPPER)", what, uplo);
        return SPMV_ERR_INVALID;
    }
    if (h->rows != h->cols) {
        set_error("%s: the handle is %lld x %lld (a triangular solve needs a square one)", what, (long long)h->rows, (long long)h->cols);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

static int trsv_planned(const spmv_csr_t *h, int uplo, const char *what)
{
    if (int rc = trsv_check(h, uplo, what)) return rc;
    if (!h->plan_trsv[uplo].ready) {
        set_error("%s: the handle has no plan for the %s triangle (spmv_csr_trsv_plan)", what, uplo == SPMV_TRSV_UPPER ? "upper" : "lower");
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

int spmv_csr_trsv_plan(spmv_csr_t *h, int uplo, int thin_rows, void *stream)
{
    const char *what = "spmv_csr_trsv_plan";
    if (int rc = trsv_check(h, uplo, what)) return rc;
    if (thin_rows < 0) { set_error("%s: thin_rows = %d (0: the default, or a positive number of rows)", what, thin_rows); return SPMV_ERR_INVALID; }
    if (h->rows > 0 && (!h->d_row_ptr || (h->nnz > 0 && (!h->d_col_idx || !h->d_vals)))) {
        set_error("%s: null array", what);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_device()) return rc;
    if (int rc = require_current(h->device, what)) return rc;
    return trsv_plan(*h, uplo == SPMV_TRSV_UPPER, thin_rows, (hipStream_t)stream);
}

int spmv_csr_trsv(spmv_csr_t *h, int uplo, int diag, const float *d_b, float *d_x, void *stream)
{
    const char *what = "spmv_csr_trsv";
    if (int rc = trsv_check(h, uplo, what)) return rc;
    if (diag != SPMV_TRSV_NON_UNIT && diag != SPMV_TRSV_UNIT) {
        set_error("%s: diag = %d (SPMV_TRSV_NON_UNIT or SPMV_TRSV_UNIT)", what, diag);
        return SPMV_ERR_INVALID;
    }
    if (h->rows > 0 && (!d_b || !d_x)) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = trsv_planned(h, uplo, what)) return rc;
    const TrsvPlan &p = h->plan_trsv[uplo];
    if (diag == SPMV_TRSV_NON_UNIT && p.bad_diag_row >= 0) {
        set_error("%s: row %lld has no diagonal entry or more than one (SPMV_TRSV_NON_UNIT needs exactly one in every row)", what,
                  (long long)p.bad_diag_row);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(h->device, what)) return rc;
    return trsv_solve(*h, uplo == SPMV_TRSV_UPPER, diag == SPMV_TRSV_UNIT, d_b, d_x, (hipStream_t)stream);
}

int64_t spmv_csr_trsv_plan_bytes(const spmv_csr_t *h, int uplo)
{
    if (int rc = trsv_check(h, uplo, "spmv_csr_trsv_plan_bytes")) return rc;
    return trsv_plan_bytes(h->plan_trsv[uplo], h->rows);
}

int spmv_csr_trsv_plan_info(const spmv_csr_t *h, int uplo, int64_t info[8])
{
    const char *what = "spmv_csr_trsv_plan_info";
    if (int rc = trsv_planned(h, uplo, what)) return rc;
    if (!info) { set_error("%s: null info", what); return SPMV_ERR_INVALID; }
    const TrsvPlan &p = h->plan_trsv[uplo];
    const int64_t v[8] = {p.levels, p.nsteps, p.widest, p.long_rows, p.bad_diag_row, p.thin, p.cap, 0};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return SPMV_OK;
}

int spmv_csr_trsv_plan_rows(const spmv_csr_t *h, int uplo, int32_t *level_ptr, int32_t *order)
{
    const char *what = "spmv_csr_trsv_plan_rows";
    if (int rc = trsv_planned(h, uplo, what)) return rc;
    if (!level_ptr || (h->rows > 0 && !order)) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, what)) return rc;
    const TrsvPlan &p = h->plan_trsv[uplo];
    for (int64_t k = 0; k <= p.levels; ++k) level_ptr[k] = p.level_ptr[k];
    if (h->rows > 0) {
        SPMV_HIP_TRY(hipMemcpy(order, p.d_order.get(), sizeof(int32_t) * (size_t)h->rows, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < h->rows; ++i) order[i] &= INT32_MAX;      // (bit 31: the kernels' mark of a long row)
    }
    return SPMV_OK;
}

int spmv_csr_trsv_describe(const spmv_csr_t *h, int uplo, char *buf, int n)
{
    const char *what = "spmv_csr_trsv_describe";
    if (int rc = trsv_planned(h, uplo, what)) return rc;
    if (!buf || n < 1) { set_error("%s: a buffer of n = %d bytes at %p", what, n, (void *)buf); return SPMV_ERR_INVALID; }
    const TrsvPlan &p = h->plan_trsv[uplo];
    snprintf(buf, (size_t)n, "trsv %s levels=%lld launches=%lld widest=%lld long_rows=%lld bad_diag_row=%lld thin=%d cap=%d bytes=%lld",
             uplo == SPMV_TRSV_UPPER ? "upper" : "lower", (long long)p.levels, (long long)p.nsteps, (long long)p.widest, (long long)p.long_rows,
             (long long)p.bad_diag_row, p.thin, p.cap, (long long)trsv_plan_bytes(p, h->rows));
    return SPMV_OK;
}

// ---- the incomplete factorisation (kernels_ilu0.hip) -------------------------------------------------------------------------
// what _values, _solve and _pivot check of their handle
static int ilu0_factor_handle(const spmv_csr_t *m, const char *what)
{
    if (!m) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (!m->plan_ilu0.ready || !m->own_vals || !m->plan_trsv[0].ready || !m->plan_trsv[1].ready) {
        set_error("%s: the handle is no factor handle (it was not made by spmv_csr_ilu0)", what);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

int spmv_csr_ilu0(const spmv_csr_t *a, int thin_rows, void *stream, spmv_csr_t **out)
{
    const char *what = "spmv_csr_ilu0";
    if (!a || !out) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (a->rows != a->cols) {
        set_error("%s: the handle is %lld x %lld (a factorisation needs a square one)", what, (long long)a->rows, (long long)a->cols);
        return SPMV_ERR_INVALID;
    }
    if (thin_rows < 0) { set_error("%s: thin_rows = %d (0: the default, or a positive number of rows)", what, thin_rows); return SPMV_ERR_INVALID; }
    if (a->rows > 0 && (!a->d_row_ptr || (a->nnz > 0 && (!a->d_col_idx || !a->d_vals)))) {
        set_error("%s: null array", what);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_device()) return rc;
    if (int rc = require_current(a->device, what)) return rc;
    return ilu0(*a, thin_rows, (hipStream_t)stream, out);
}

int spmv_csr_ilu0_values(spmv_csr_t *m, const spmv_csr_t *a, void *stream)
{
    const char *what = "spmv_csr_ilu0_values";
    if (!a) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (int rc = ilu0_factor_handle(m, what)) return rc;
    if (a == m) { set_error("%s: a is m itself (m's values would be read while they are written)", what); return SPMV_ERR_INVALID; }
    if (a->rows != m->plan_ilu0.a_rows || a->cols != a->rows || a->nnz != m->plan_ilu0.a_nnz) {
        set_error("%s: a is %lld x %lld with %lld nonzeros, m was factored from %lld x %lld with %lld", what, (long long)a->rows,
                  (long long)a->cols, (long long)a->nnz, (long long)m->plan_ilu0.a_rows, (long long)m->plan_ilu0.a_rows,
                  (long long)m->plan_ilu0.a_nnz);
        return SPMV_ERR_INVALID;
    }
    if (a->nnz > 0 && !a->d_vals) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = require_current(m->device, what)) return rc;
    if (a->device != m->device) {
        set_error("%s: a lives on device %d, m on device %d", what, a->device, m->device);
        return SPMV_ERR_INVALID;
    }
    if (int rc = ilu0_values(*m, *a, (hipStream_t)stream)) return rc;
    ++m->values_gen;
    return SPMV_OK;
}

int spmv_csr_ilu0_solve(spmv_csr_t *m, const float *d_r, float *d_z, void *stream)
{
    const char *what = "spmv_csr_ilu0_solve";
    if (int rc = ilu0_factor_handle(m, what)) return rc;
    if (m->rows > 0 && (!d_r || !d_z)) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = require_current(m->device, what)) return rc;
    return ilu0_solve(*m, d_r, d_z, (hipStream_t)stream);
}

int spmv_csr_ilu0_pivot(const spmv_csr_t *m, void *stream, int64_t *row)
{
    const char *what = "spmv_csr_ilu0_pivot";
    if (int rc = ilu0_factor_handle(m, what)) return rc;
    if (!row) { set_error("%s: null row", what); return SPMV_ERR_INVALID; }
    if (int rc = require_current(m->device, what)) return rc;
    return ilu0_pivot(*m, (hipStream_t)stream, row);
}

int64_t spmv_csr_ilu0_plan_bytes(const spmv_csr_t *m)
{
    if (!m) { set_error("spmv_csr_ilu0_plan_bytes: null handle"); return SPMV_ERR_INVALID; }
    return ilu0_plan_bytes(*m);
}

// ---- the multicolour ordering (kernels_color.hip, kernels_permute.hip) ----------------------------------------------------
int spmv_csr_color(const spmv_csr_t *a, uint32_t seed, void *stream, int32_t *d_color, int32_t *d_perm, int32_t *color_ptr, int cap,
                   int64_t info[8])
{
    const char *what = "spmv_csr_color";
    if (!a) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (!d_color) { set_error("%s: null d_color", what); return SPMV_ERR_INVALID; }
    if (a->rows != a->cols) {
        set_error("%s: the handle is %lld x %lld (a colouring needs a square one)", what, (long long)a->rows, (long long)a->cols);
        return SPMV_ERR_INVALID;
    }
    if (cap < 0) { set_error("%s: cap = %d (the entries of color_ptr are not negative)", what, cap); return SPMV_ERR_INVALID; }
    if (color_ptr && cap == 0) { set_error("%s: color_ptr with cap = 0", what); return SPMV_ERR_INVALID; }
    if (a->rows > 0 && (!a->d_row_ptr || (a->nnz > 0 && !a->d_col_idx))) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = require_device()) return rc;
    if (int rc = require_current(a->device, what)) return rc;
    return color(*a, seed, (hipStream_t)stream, d_color, d_perm, color_ptr, cap, info);
}

int spmv_csr_permute(const spmv_csr_t *a, const int32_t *d_row_perm, const int32_t *d_col_perm, int flags, void *stream, spmv_csr_t **out)
{
    const char *what = "spmv_csr_permute";
    if (!a || !out) { set_error("%s: null argument", what); return SPMV_ERR_INVALID; }
    if (flags & ~(SPMV_PERMUTE_KEEP_MAP | SPMV_PERMUTE_VIA_TRANSPOSE)) {
        set_error("%s: flags = 0x%x (SPMV_PERMUTE_KEEP_MAP | SPMV_PERMUTE_VIA_TRANSPOSE or 0)", what, (unsigned)flags);
        return SPMV_ERR_INVALID;
    }
    if (a->rows >= 0x7f7f7f7f || a->cols >= 0x7f7f7f7f || a->nnz > INT32_MAX) {
        set_error("%s: the handle is %lld x %lld with %lld nonzeros (too large for 32-bit marks)", what, (long long)a->rows, (long long)a->cols,
                  (long long)a->nnz);
        return SPMV_ERR_INVALID;
    }
    if (a->rows > 0 && (!a->d_row_ptr || (a->nnz > 0 && (!a->d_col_idx || !a->d_vals)))) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    if (int rc = require_device()) return rc;
    if (int rc = require_current(a->device, what)) return rc;
    return permute(*a, d_row_perm, d_col_perm, (flags & SPMV_PERMUTE_KEEP_MAP) != 0, (flags & SPMV_PERMUTE_VIA_TRANSPOSE) != 0,
                   (hipStream_t)stream, out);
}

int spmv_csr_permute_values(spmv_csr_t *b, const spmv_csr_t *a, void *stream)
{
    return map_values("spmv_csr_permute_values", kOfPermute, b, a, stream);
}

int spmv_csr_permute_gather(const spmv_csr_t *b, int count, const void *d_src, int64_t src_stride, void *d_dst, int64_t dst_stride,
                            void *stream)
{
    return map_move_checked("spmv_csr_permute_gather", kOfPermute, b, false, count, d_src, src_stride, d_dst, dst_stride, stream);
}

int64_t spmv_csr_permute_map_bytes(const spmv_csr_t *b) { return map_bytes("spmv_csr_permute_map_bytes", kOfPermute, b); }

int spmv_permute_vector(const int32_t *d_perm, int64_t n, int inverse, const float *d_src, float *d_dst, void *stream)
{
    const char *what = "spmv_permute_vector";
    if (n < 0) { set_error("%s: n = %lld", what, (long long)n); return SPMV_ERR_INVALID; }
    if (inverse != 0 && inverse != 1) { set_error("%s: inverse = %d (0 or 1)", what, inverse); return SPMV_ERR_INVALID; }
    if (n > 0 && (!d_perm || !d_src || !d_dst)) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst), bytes = (uintptr_t)n * 4;
    if (n > 0 && s0 < d0 + bytes && d0 < s0 + bytes) { set_error("%s: src and dst overlap", what); return SPMV_ERR_INVALID; }
    if (int rc = require_device()) return rc;
    return permute_vector(d_perm, n, inverse == 1, d_src, d_dst, (hipStream_t)stream);
}

// SPMV_AUTO.  TILED's plan is made first (cheap: a few passes over col_idx, no trial launches) and priced (model_cost,
// in units of "a chunk that streams 8 bytes per nonzero with cache-resident gathers").
//   1. It stages (nearly) everything in one or two passes (model_cost <= 1.20: bands up to ~60 000 columns at config 4): TILED.
//   2. Otherwise the sorted-blocks layout of SPMV_PANEL (kernels_colsort.hip) is tried where a look at the matrix says it can
//      work -- short rows (at most a tenth of the nonzeros in rows of more than 256), blocks of 4096 rows whose window of
//      x fits an L2 -- and taken when its own model prices it below TILED (wide bands: 65 536 columns and beyond; uniform
//      columns over a few MiB of x: config 2).
//   3. Otherwise, when TILED could stage or sort less than half of the chunks -- it gathers most of x through L2/fabric,
//      one request per nonzero -- and x fills one XCD's 4 MiB L2 or more, the panel sweep (1.2x at config 2's 4 MiB, 3-4x at
//      64 MiB: DESIGN.md section 4); below that size x sits in every L2 anyway and the row-major kernel keeps its lead.
static int plan_auto(spmv_csr &h, hipStream_t s)
{
    if (h.auto_variant == SPMV_PANEL) return refresh_panel(h, h.plan_auto_panel, s);   // idempotent, except that a stale copy of vals is rebuilt
    if (h.auto_variant >= 0) return SPMV_OK;
    h.auto_made_tiled = h.plan_tiled.block == 0;
    int rc = plan_adaptive(h, true, s);
    if (rc) return rc;
    // a TILED plan the caller made stays; one made here for a look is released when another variant is chosen (up to
    // 6 bytes per nonzero of column copies nobody would read)
    auto release_tiled = [&]() { if (h.auto_made_tiled) h.plan_tiled = ChunkPlan{}; h.auto_made_tiled = false; };
    const ChunkPlan &p = h.plan_tiled;
    const double cost_tiled = p.model_cost;
    const bool little_staged = p.nchunks > 0 && 2 * ((int64_t)p.staged_full + p.nsorted) < p.nchunks &&
                               2 * (int64_t)p.nblk_chunks < p.nchunks;
    const bool x_beyond_l2 = h.cols * (int64_t)sizeof(float) >= (4ll << 20);   // an L2 also holds the stream passing through
    // (a workgroup per 4096 rows, one or two per CU: fewer blocks than three quarters of the CUs leave the chip idle)
    bool try_sorted = p.nchunks > 0 && cost_tiled > 1.20 && 2 * (int64_t)p.nblk_chunks < p.nchunks &&
                      h.rows >= 4096ll * (3 * device_cus(h.device) / 4);
    if (const char *e = getenv("SPMV_AUTO_SORTED_BLOCKS")) try_sorted = try_sorted && atoi(e) != 0;   // 0: never (A/B runs)
    if (try_sorted) {
        double long_frac = 0.0, wide_frac = 0.0, lines_est = 0.0;
        if ((rc = colsort_probe(h, s, &long_frac, &wide_frac, &lines_est))) return rc;
        // (the estimate of the lines per nonzero prices the layout before it is built: 5 % slack for what it cannot see)
        if (long_frac <= 0.10 && wide_frac <= 0.10 && 0.95 * colsort_cost(4096, lines_est, long_frac) < cost_tiled) {
            // (the layout takes 8192-row blocks where the 4096-row ones touch more than 0.27 lines of x per nonzero: where the
            // probe's estimate is clearly beyond that, the 4096-row build -- 23 ms at config 4 -- is skipped)
            const bool big = lines_est > 0.30 && h.rows >= 4096ll * 16 * device_cus(h.device);
            rc = build_panel(h, h.plan_auto_panel, big ? 8192 : 0, big ? 4 : 0, 3, s);
            if (rc == SPMV_OK) {
                const SortedBlocksPlan &pp = h.plan_auto_panel.sorted;
                const bool fits = (double)pp.tail <= 0.10 * (double)h.nnz && 10 * pp.wide_blocks <= pp.nblocks;
                if (fits && colsort_model_cost(pp, h.nnz) < 0.98 * cost_tiled) {   // (a tie goes to TILED: it reads vals live)
                    h.auto_variant = SPMV_PANEL;
                    release_tiled();
                    return SPMV_OK;
                }
                h.plan_auto_panel = PanelPlan{};
            } else if (rc != SPMV_ERR_INVALID) {
                return rc;   // INVALID: outside the layout's limits -> on with the other candidates
            }
        }
    }
    if (little_staged && x_beyond_l2) {
        // x beyond every L2 (each gather would be a 128-byte line from the fabric) and tiles that still hold a line or
        // two of products: the binned layout -- two streaming launches, nothing gathered from memory
        // (measured, profiles/r04_binned_*.jsonl: config 4 uniform 1.33 -> 1.06 ms at 83 nonzeros per tile, config 3 uniform
        // 0.86 -> 0.52 ms at 663; config 5's shard 3.0 -> 4.1 ms at 10: the sum launch works on nearly empty pieces)
        // Thinner tiles (config 5's shard: 14 at 4096 rows per bin, 28 at 8192): the flavour whose product launch stores in bin
        // order -- the sum launch then streams whatever the tiles hold (3.0 -> 1.12 ms there, the sweep with its shorter step 2.4).
        // Constant rows of 8 / 10 / 12 / 16 / 24 on 16Mi x 16Mi (64 ... 192 nonzeros per 4096 rows x 32768 columns): 0.55 / 0.67 /
        // 0.78 / 1.01 / 1.50 ms against the fetching flavour's 0.69 / 0.78 / 0.87 / 1.06 / 1.53 (profiles/
        // r04_binned_flavours_by_tile.jsonl), config 4 itself (128) 0.97 against 1.01, config 3 (1024, a third of the nonzeros in
        // long rows) 0.52 against 0.54 once it has a bin per resident wavefront: the fetching flavour (mode 4) is never the
        // rule's answer any more; it stays selectable
        const bool big_x = h.cols * (int64_t)sizeof(float) >= (8ll << 20);
        const double tile = binned_tile_nonzeros(h, 4096);
        int try_binned = big_x && tile >= 4.0 ? 5 : 0;
        if (const char *e = getenv("SPMV_AUTO_BINNED")) try_binned = atoi(e) != 0 ? try_binned : 0;   // 0: never (A/B runs)
        if (try_binned) {
            rc = build_panel(h, h.plan_auto_panel, 0, 0, try_binned, s);
            // (bins that ran out of spare accumulators add with LDS atomics, four times slower: rows with dozens of nonzeros in
            // one tile -- long rows over a band of a few million columns -- are the fetching flavour's case)
            if (rc == SPMV_OK && try_binned == 5 && 32 * (int64_t)h.plan_auto_panel.scattered.flagged_bins > h.plan_auto_panel.scattered.nblocks)
                rc = build_panel(h, h.plan_auto_panel, 0, 0, 4, s);
            if (rc == SPMV_OK) {
                h.auto_variant = SPMV_PANEL;
                release_tiled();
                return SPMV_OK;
            }
            if (rc != SPMV_ERR_INVALID) return rc;   // INVALID: outside the layout's limits -> the sweep
        }
        rc = build_panel(h, h.plan_auto_panel, 0, 0, 1, s);
        if (rc == SPMV_OK) {
            h.auto_variant = SPMV_PANEL;
            release_tiled();
            return SPMV_OK;
        }
        if (rc != SPMV_ERR_INVALID) return rc;   // INVALID: outside the panel layout's limits -> stay with TILED
    }
    h.auto_variant = SPMV_TILED;
    return SPMV_OK;
}

int spmv_csr_plan(spmv_csr_t *h, int variant, void *stream)
{
    if (!h) { set_error("spmv_csr_plan: null handle"); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, "spmv_csr_plan")) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (variant) {
        case SPMV_AUTO: return plan_auto(*h, s);
        case SPMV_WAVE: return h->nnz <= 32 * h->rows ? plan_wave(*h, s) : SPMV_OK;   // short rows: bundles (the long rows' pieces)
        case SPMV_SCALAR:        // (the x windows of the bundle kernel, which SPMV_SCALAR runs with ordered sums)
        case SPMV_WAVE_PIPE: return plan_wave(*h, s);
        case SPMV_VECTOR: return plan_vector(*h, s);
        case SPMV_ADAPTIVE: return plan_adaptive(*h, false, s);
        case SPMV_TILED: return plan_adaptive(*h, true, s);
        case SPMV_PANEL: return refresh_panel(*h, h->plan_panel, s);
        case SPMV_XSKIP: return plan_xskip(*h, s);
        default:
            set_error("spmv_csr_plan: unknown variant %d", variant);
            return SPMV_ERR_VARIANT;
    }
}

int spmv_csr_run(spmv_csr_t *h, int variant, const float *d_x, float *d_y, void *stream)
{
    if (!h || (!d_x && h->cols > 0) || (!d_y && h->rows > 0)) {
        set_error("spmv_csr_run: null argument");
        return SPMV_ERR_INVALID;
    }
    if (!aligned16(d_x)) {
        set_error("spmv_csr_run: x must be 16-byte aligned");
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(h->device, "spmv_csr_run")) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (variant == SPMV_AUTO) {
        if (h->auto_variant < 0) { set_error("SPMV_AUTO used before spmv_csr_plan"); return SPMV_ERR_NOT_PLANNED; }
        if (h->auto_variant == SPMV_PANEL) return launch_panel_plan(*h, h->plan_auto_panel, d_x, d_y, s);
        variant = h->auto_variant;
    }
    switch (variant) {
        case SPMV_SCALAR: return launch_scalar(*h, d_x, d_y, s);
        case SPMV_WAVE: return launch_wave(*h, d_x, d_y, false, s);
        case SPMV_WAVE_PIPE: return launch_wave(*h, d_x, d_y, true, s);
        case SPMV_VECTOR: return launch_vector(*h, d_x, d_y, s);
        case SPMV_ADAPTIVE: return launch_adaptive(*h, d_x, d_y, false, s);
        case SPMV_TILED: return launch_adaptive(*h, d_x, d_y, true, s);
        case SPMV_PANEL: return launch_panel_plan(*h, h->plan_panel, d_x, d_y, s);
        case SPMV_XSKIP: return launch_xskip(*h, d_x, d_y, s);
        default:
            set_error("spmv_csr_run: unknown variant %d", variant);
            return SPMV_ERR_VARIANT;
    }
}

// y = A x with the values of A read from nnz bf16 / fp16 elements of the caller's (include/spmv_hip.h, "SpMV on 16-bit values")
int spmv_csr_run_vals16(spmv_csr_t *h, int variant, int dtype, const void *d_vals16, const float *d_x, float *d_y, void *stream)
{
    const char *what = "spmv_csr_run_vals16";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (int rc = dtype_ok(dtype, false, what)) return rc;
    if ((!d_vals16 && h->nnz > 0) || (!d_x && h->cols > 0) || (!d_y && h->rows > 0)) {
        set_error("%s: null vals16, x or y", what);
        return SPMV_ERR_INVALID;
    }
    if (!aligned16(d_vals16) || !aligned16(d_x)) {
        set_error("%s: vals16 and x must be 16-byte aligned", what);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(h->device, what)) return rc;
    int resolved = variant;
    if (variant == SPMV_AUTO) {
        if (h->auto_variant < 0) { set_error("%s: SPMV_AUTO used before spmv_csr_plan", what); return SPMV_ERR_NOT_PLANNED; }
        resolved = h->auto_variant;
    }
    if (resolved != SPMV_TILED && resolved != SPMV_ADAPTIVE) {
        if (variant == SPMV_AUTO)
            set_error("%s: SPMV_AUTO resolved to %s, whose layout holds a copy of the fp32 values (need SPMV_TILED or SPMV_ADAPTIVE)",
                      what, spmv_variant_name(resolved));
        else set_error("%s: variant %d (%s) does not read 16-bit values (need SPMV_TILED, SPMV_ADAPTIVE, or SPMV_AUTO resolved to SPMV_TILED)",
                       what, variant, spmv_variant_name(variant));
        return SPMV_ERR_VARIANT;
    }
    return launch_adaptive_vals16(*h, dtype, d_vals16, d_x, d_y, resolved == SPMV_TILED, (hipStream_t)stream);
}

int spmv_csr_spmm_plan(spmv_csr_t *h, void *stream)
{
    if (!h) { set_error("spmv_csr_spmm_plan: null handle"); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, "spmv_csr_spmm_plan")) return rc;
    return plan_spmm(*h, (hipStream_t)stream);
}

// ---- SpMM and SDDMM: one description of a run call, checked in one place ------------------------------
// A dense matrix of a call: its name in the messages ("X"; its ld is "ldx"), pointer and ld, and whether the handle's cols
// (else its rows) count its rows.
struct DenseArg {
    const char *name;
    const void *p;
    int64_t ld;
    bool by_cols;
};

// One of the six run calls: its name, its two matrices in argument order, SDDMM's out (has_out), whether dtype may be
// SPMV_ATTN_FP32 (the fp32 calls pass that constant), and whether it runs in column tiles: then k goes up to SPMV_COLS_MAX_K
// and the plan is spmv_csr_spmm_plan_cols' and has to cover k, else k <= 64 on the plan of spmv_csr_spmm_plan.
struct ProductCall {
    const char *what;
    bool fp32_too, cols;
    DenseArg a, b;
    bool has_out;
    const float *out;
};

// What every one of them checks, in this order: the handle, the dtype, 1 <= k <= the widest and both ld >= k, the pointers
// present and aligned for the dtype (16 bytes of floats, 8 of 16-bit elements; out 4), the byte offsets, the device, the plan.
static int product_args(const ProductCall &c, const spmv_csr_t *h, int dtype, int k)
{
    const char *what = c.what, *na = c.a.name, *nb = c.b.name;
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (int rc = dtype_ok(dtype, c.fp32_too, what)) return rc;
    const int max_k = c.cols ? (int)SPMV_COLS_MAX_K : 64;
    const char la = (char)tolower(na[0]), lb = (char)tolower(nb[0]);
    if (k < 1 || k > max_k || c.a.ld < k || c.b.ld < k) {
        set_error("%s: k = %d, ld%c = %lld, ld%c = %lld (need 1 <= k <= %d, ld%c >= k, ld%c >= k)", what, k, la, (long long)c.a.ld, lb,
                  (long long)c.b.ld, max_k, la, lb);
        return SPMV_ERR_INVALID;
    }
    const int64_t ra = c.a.by_cols ? h->cols : h->rows, rb = c.b.by_cols ? h->cols : h->rows;
    if ((!c.a.p && ra > 0) || (!c.b.p && rb > 0) || (c.has_out && !c.out && h->nnz > 0)) {
        if (c.has_out) set_error("%s: null %s, %s or out", what, na, nb);
        else set_error("%s: null %s or %s", what, na, nb);
        return SPMV_ERR_INVALID;
    }
    const bool f32 = dtype == SPMV_ATTN_FP32;
    if (f32 ? !aligned16(c.a.p) || !aligned16(c.b.p) : !aligned8(c.a.p) || !aligned8(c.b.p)) {
        set_error("%s: %s and %s must be %d-byte aligned", what, na, nb, f32 ? 16 : 8);
        return SPMV_ERR_INVALID;
    }
    if (c.has_out && reinterpret_cast<uintptr_t>(c.out) % 4 != 0) { set_error("%s: out must be 4-byte aligned", what); return SPMV_ERR_INVALID; }
    const int64_t es = f32 ? 4 : 2;
    if (c.a.ld > INT64_MAX / es / (ra > 0 ? ra : 1) || c.b.ld > INT64_MAX / es / (rb > 0 ? rb : 1)) {
        set_error("%s: ld%c = %lld or ld%c = %lld overflows 64-bit byte offsets", what, la, (long long)c.a.ld, lb, (long long)c.b.ld);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(h->device, what)) return rc;
    if (!h->plan_spmm.ready || (c.cols && !h->plan_spmm.cols_k)) {
        set_error("%s used before %s", what, c.cols ? "spmv_csr_spmm_plan_cols" : "spmv_csr_spmm_plan");
        return SPMV_ERR_NOT_PLANNED;
    }
    if (c.cols && k > h->plan_spmm.cols_k) {
        set_error("%s: k = %d, the plan covers %d (spmv_csr_spmm_plan_cols)", what, k, h->plan_spmm.cols_k);
        return SPMV_ERR_NOT_PLANNED;
    }
    return SPMV_OK;
}

// Y = A X (kernels_spmm.hip) and out = (U X^T)[pattern] (kernels_sddmm.hip) for any of their three entry points each
static int run_spmm(const char *what, bool fp32_too, bool cols, spmv_csr_t *h, int dtype, int k, const void *d_X, int64_t ldx, void *d_Y,
                    int64_t ldy, void *stream)
{
    if (int rc = product_args({what, fp32_too, cols, {"X", d_X, ldx, true}, {"Y", d_Y, ldy, false}, false, nullptr}, h, dtype, k)) return rc;
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return launch_spmm<E>(*h, what, cols, k, (const E *)d_X, ldx, (E *)d_Y, ldy, (hipStream_t)stream);
    });
}

static int run_sddmm(const char *what, bool fp32_too, bool cols, spmv_csr_t *h, int dtype, int k, const void *d_U, int64_t ldu,
                     const void *d_X, int64_t ldx, float *d_out, void *stream)
{
    if (int rc = product_args({what, fp32_too, cols, {"U", d_U, ldu, false}, {"X", d_X, ldx, true}, true, d_out}, h, dtype, k)) return rc;
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return launch_sddmm<E>(*h, what, cols, k, (const E *)d_U, ldu, (const E *)d_X, ldx, d_out, (hipStream_t)stream);
    });
}

int spmv_csr_spmm(spmv_csr_t *h, int k, const float *d_X, int64_t ldx, float *d_Y, int64_t ldy, void *stream)
{
    return run_spmm("spmv_csr_spmm", true, false, h, SPMV_ATTN_FP32, k, d_X, ldx, d_Y, ldy, stream);
}

int64_t spmv_csr_spmm_plan_bytes(const spmv_csr_t *h)
{
    if (!h) { set_error("spmv_csr_spmm_plan_bytes: null handle"); return SPMV_ERR_INVALID; }
    return spmm_plan_bytes(*h);
}

int spmv_csr_spmm_describe(const spmv_csr_t *h, char *buf, int n)
{
    if (!h || !buf || n <= 0) { set_error("spmv_csr_spmm_describe: bad argument"); return SPMV_ERR_INVALID; }
    const SpmmPlan &p = h->plan_spmm;
    if (!p.ready) snprintf(buf, (size_t)n, "not planned");
    else snprintf(buf, (size_t)n, "row_cap=%d piece_len=%d long_rows=%d pieces=%d", p.row_cap, p.piece_len, p.n_long, p.pieces);
    return SPMV_OK;
}

int spmv_csr_sddmm(spmv_csr_t *h, int k, const float *d_U, int64_t ldu, const float *d_X, int64_t ldx, float *d_out, void *stream)
{
    return run_sddmm("spmv_csr_sddmm", true, false, h, SPMV_ATTN_FP32, k, d_U, ldu, d_X, ldx, d_out, stream);
}

// ---- the same two products on 16-bit matrices (bf16 or fp16 storage; vals, out and every sum fp32) ------------------------
int spmv_csr_spmm_16(spmv_csr_t *h, int dtype, int k, const void *d_X, int64_t ldx, void *d_Y, int64_t ldy, void *stream)
{
    return run_spmm("spmv_csr_spmm_16", false, false, h, dtype, k, d_X, ldx, d_Y, ldy, stream);
}

int spmv_csr_sddmm_16(spmv_csr_t *h, int dtype, int k, const void *d_U, int64_t ldu, const void *d_X, int64_t ldx, float *d_out,
                      void *stream)
{
    return run_sddmm("spmv_csr_sddmm_16", false, false, h, dtype, k, d_U, ldu, d_X, ldx, d_out, stream);
}

// ---- the same two products at any k, in column tiles of 64 (fp32, bf16 or fp16 matrices; kernels_spmm.hip, kernels_sddmm.hip) ----
int spmv_csr_spmm_plan_cols(spmv_csr_t *h, int k_max, void *stream)
{
    const char *what = "spmv_csr_spmm_plan_cols";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (k_max < 1 || k_max > SPMV_COLS_MAX_K) {
        set_error("%s: k_max = %d (need 1 <= k_max <= %d)", what, k_max, (int)SPMV_COLS_MAX_K);
        return SPMV_ERR_INVALID;
    }
    if (int rc = require_current(h->device, what)) return rc;
    return plan_spmm_cols(*h, k_max, (hipStream_t)stream);
}

int spmv_csr_spmm_cols(spmv_csr_t *h, int dtype, int k, const void *d_X, int64_t ldx, void *d_Y, int64_t ldy, void *stream)
{
    return run_spmm("spmv_csr_spmm_cols", true, true, h, dtype, k, d_X, ldx, d_Y, ldy, stream);
}

int spmv_csr_sddmm_cols(spmv_csr_t *h, int dtype, int k, const void *d_U, int64_t ldu, const void *d_X, int64_t ldx, float *d_out,
                        void *stream)
{
    return run_sddmm("spmv_csr_sddmm_cols", true, true, h, dtype, k, d_U, ldu, d_X, ldx, d_out, stream);
}

// what spmv_csr_row_softmax and its backward check alike: a finite scale; with nnz > 0 every array present and 4-byte
// aligned; the handle's device current; the SpMM plan made
static int softmax_args(const spmv_csr_t *h, float scale, const void *const *arrays, int n_arrays, const char *what)
{
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (!(scale - scale == 0.0f)) { set_error("%s: scale must be finite", what); return SPMV_ERR_INVALID; }
    for (int i = 0; i < n_arrays && h->nnz > 0; ++i) {
        if (!arrays[i]) { set_error("%s: null array", what); return SPMV_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(arrays[i]) % 4 != 0) { set_error("%s: every array must be 4-byte aligned", what); return SPMV_ERR_INVALID; }
    }
    if (int rc = require_current(h->device, what)) return rc;
    if (!h->plan_spmm.ready) { set_error("%s used before spmv_csr_spmm_plan", what); return SPMV_ERR_NOT_PLANNED; }
    return SPMV_OK;
}

int spmv_csr_row_softmax(spmv_csr_t *h, float scale, const float *d_scores, float *d_out, void *stream)
{
    const void *arrays[] = {d_scores, d_out};
    if (int rc = softmax_args(h, scale, arrays, 2, "spmv_csr_row_softmax")) return rc;
    return launch_row_softmax(*h, scale, d_scores, d_out, (hipStream_t)stream);
}

int spmv_csr_row_softmax_backward(spmv_csr_t *h, float scale, const float *d_P, const float *d_dP, float *d_dS, void *stream)
{
    const void *arrays[] = {d_P, d_dP, d_dS};
    if (int rc = softmax_args(h, scale, arrays, 3, "spmv_csr_row_softmax_backward")) return rc;
    return launch_row_softmax_backward(*h, scale, d_P, d_dP, d_dS, (hipStream_t)stream);
}

// ---- fused attention (kernels_attention.hip) ---------------------------------------------------------------------------
int spmv_csr_attention_plan(spmv_csr_t *h, void *stream)
{
    if (!h) { set_error("spmv_csr_attention_plan: null handle"); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, "spmv_csr_attention_plan")) return rc;
    return plan_attention(*h, (hipStream_t)stream);
}

int64_t spmv_csr_attention_plan_bytes(const spmv_csr_t *h)
{
    if (!h) { set_error("spmv_csr_attention_plan_bytes: null handle"); return SPMV_ERR_INVALID; }
    return attention_plan_bytes(*h);
}

int spmv_csr_attention_plan_heads(spmv_csr_t *h, int heads, void *stream)
{
    const char *what = "spmv_csr_attention_plan_heads";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (heads < 1 || heads > kMaxHeads) { set_error("%s: heads = %d (need 1 <= heads <= %d)", what, heads, kMaxHeads); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, what)) return rc;
    return plan_attention_heads(*h, heads, (hipStream_t)stream);
}

// widest: 64, or 128 in the _wide calls
static int attention_widths(int k, int kv, const char *what, int widest = 64)
{
    if (k < 1 || k > widest || kv < 1 || kv > widest) {
        set_error("%s: k = %d, kv = %d (need 1 <= k <= %d and 1 <= kv <= %d)", what, k, kv, widest, widest);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

int spmv_csr_attention_plan_wide(spmv_csr_t *h, int heads, void *stream)
{
    const char *what = "spmv_csr_attention_plan_wide";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (heads < 1 || heads > kMaxHeads) { set_error("%s: heads = %d (need 1 <= heads <= %d)", what, heads, kMaxHeads); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, what)) return rc;
    return plan_attention_wide(*h, heads, (hipStream_t)stream);
}

int spmv_csr_attention_max_heads_wide(const spmv_csr_t *h, int k, int kv)
{
    const char *what = "spmv_csr_attention_max_heads_wide";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (int rc = attention_widths(k, kv, what, 128)) return rc;
    if (!h->plan_spmm.ready) { set_error("%s used before spmv_csr_attention_plan", what); return SPMV_ERR_NOT_PLANNED; }
    return attention_max_heads(*h, k > kv ? k : kv);
}

int spmv_csr_attention_max_heads(const spmv_csr_t *h, int k, int kv)
{
    const char *what = "spmv_csr_attention_max_heads";
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (int rc = attention_widths(k, kv, what)) return rc;
    if (!h->plan_spmm.ready) { set_error("%s used before spmv_csr_attention_plan", what); return SPMV_ERR_NOT_PLANNED; }
    return attention_max_heads(*h, k > kv ? k : kv);
}

namespace {
// One operand of an attention call, as its checks see it: a matrix of n rows (the queries or the keys) of ld elements, of which
// `width` (k or kv) are used, or a vector of `width` floats per query (stats: 2, delta: 1; ld unused).  An element is a float,
// or 2 bytes in the _16 calls (`elem` of attention_operands).
struct AttnOperand {
    const char *name;
    const void *p;
    int64_t ld, n;
    int width;
    int64_t stride;    // elements (a vector: floats) from one head to the next
    int unit;          // the stride is a multiple of it: 4 for a matrix (heads aligned like head 0), 2 for stats, 1 for delta
    bool out;          // an output: with more than one head its stride is at least its width
    bool kv_heads;     // it holds the K/V heads (heads / group of them), not the query heads
    bool vector() const { return unit != 4; }
};
constexpr bool kIn = false, kOut = true, kQHeads = false, kKVHeads = true;

// a call of one head is the _heads call on this: one head, every stride 0
const spmv_attn_heads_t kOneHead = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
}  // namespace

// what the attention calls check before an operand is looked at: the handle, the header of hs and the group (1 for a
// call that has none)
static int attention_header(const spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, const char *what)
{
    if (!h) { set_error("%s: null handle", what); return SPMV_ERR_INVALID; }
    if (!hs) { set_error("%s: null hs", what); return SPMV_ERR_INVALID; }
    if (hs->heads < 1 || hs->heads > kMaxHeads) {
        set_error("%s: heads = %d (need 1 <= heads <= %d, the launch limit)", what, hs->heads, kMaxHeads);
        return SPMV_ERR_INVALID;
    }
    if (hs->reserved != 0) { set_error("%s: reserved = %d (must be 0)", what, hs->reserved); return SPMV_ERR_INVALID; }
    if (group < 1) { set_error("%s: group = %d (need group >= 1)", what, group); return SPMV_ERR_INVALID; }
    if (hs->heads % group != 0) {
        set_error("%s: heads = %d is no multiple of group = %d", what, hs->heads, group);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

// and after it, in this order: every head stride (they read k and kv as given); k and kv; the scale; every matrix (ld,
// presence, alignment to four elements of `elem` bytes: 16 bytes of floats, 8 of 16-bit elements; 64-bit byte offsets); the
// vectors (presence, then stats 8-byte and delta 4-byte aligned); the device; the plan and the heads it covers.
// wide: a _wide call, whose widths end at 128 and whose plan is spmv_csr_attention_plan_wide's, at every width.
static int attention_operands(const spmv_csr_t *h, int heads, int group, float scale, int k, int kv, const AttnOperand *ops, size_t n_ops,
                              int elem, const char *what, bool wide = false)
{
    for (size_t i = 0; i < n_ops; ++i) {
        const AttnOperand &o = ops[i];
        if (o.stride < 0) { set_error("%s: head stride of %s = %lld is negative", what, o.name, (long long)o.stride); return SPMV_ERR_INVALID; }
        if (o.stride % o.unit != 0) {
            set_error("%s: head stride of %s = %lld is no multiple of %d", what, o.name, (long long)o.stride, o.unit);
            return SPMV_ERR_INVALID;
        }
        if (o.out && (o.kv_heads ? heads / group : heads) > 1 && o.stride < o.width) {
            set_error("%s: head stride of the output %s = %lld is below its width %d", what, o.name, (long long)o.stride, o.width);
            return SPMV_ERR_INVALID;
        }
        if (o.stride > INT64_MAX / 4 / heads) {
            set_error("%s: head stride of %s = %lld overflows 64-bit byte offsets", what, o.name, (long long)o.stride);
            return SPMV_ERR_INVALID;
        }
    }
    if (int rc = attention_widths(k, kv, what, wide ? 128 : 64)) return rc;
    if (!(scale - scale == 0.0f)) { set_error("%s: scale must be finite", what); return SPMV_ERR_INVALID; }
    for (size_t i = 0; i < n_ops; ++i) {
        const AttnOperand &o = ops[i];
        if (o.vector()) continue;
        if (o.ld < o.width) { set_error("%s: ld of %s = %lld is below its width %d", what, o.name, (long long)o.ld, o.width); return SPMV_ERR_INVALID; }
        if (!o.p && o.n > 0) { set_error("%s: null %s", what, o.name); return SPMV_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(o.p) % (4 * elem) != 0) { set_error("%s: %s must be %d-byte aligned", what, o.name, 4 * elem); return SPMV_ERR_INVALID; }
        if (o.ld > INT64_MAX / 4 / (o.n > 0 ? o.n : 1)) {
            set_error("%s: ld of %s = %lld overflows 64-bit byte offsets", what, o.name, (long long)o.ld);
            return SPMV_ERR_INVALID;
        }
    }
    for (size_t i = 0; i < n_ops; ++i)
        if (ops[i].vector() && !ops[i].p && ops[i].n > 0) { set_error("%s: null stats or delta", what); return SPMV_ERR_INVALID; }
    for (size_t i = 0; i < n_ops; ++i)
        if (ops[i].vector() && reinterpret_cast<uintptr_t>(ops[i].p) % (4 * ops[i].unit) != 0) {
            set_error("%s: stats must be 8-byte aligned and delta 4-byte aligned", what);
            return SPMV_ERR_INVALID;
        }
    if (int rc = require_current(h->device, what)) return rc;
    if (wide) {
        if (!h->plan_attn.ready || !h->plan_spmm.ready || !h->plan_attn.wide_heads) {
            set_error("%s used before spmv_csr_attention_plan_wide", what);
            return SPMV_ERR_NOT_PLANNED;
        }
        if (heads > h->plan_attn.wide_heads) {
            set_error("%s: %d heads, the wide plan covers %d (spmv_csr_attention_plan_wide)", what, heads, h->plan_attn.wide_heads);
            return SPMV_ERR_NOT_PLANNED;
        }
        return SPMV_OK;      // (plan_wide covers at least as many heads in the narrow plan)
    }
    if (!h->plan_attn.ready || !h->plan_spmm.ready) { set_error("%s used before spmv_csr_attention_plan", what); return SPMV_ERR_NOT_PLANNED; }
    if (heads > h->plan_attn.heads) {
        set_error("%s: %d heads, the plan covers %d (spmv_csr_attention_plan_heads)", what, heads, h->plan_attn.heads);
        return SPMV_ERR_NOT_PLANNED;
    }
    return SPMV_OK;
}

extern "C++" {      // (templates: this file is otherwise C linkage)
// The three passes.  Each is every entry point of its pass: hs->heads query heads, `group` of them per K/V head;
// sum_group: backward_kv adds the heads of a group in the kernel (the _gqa call).  E: float for the nine fp32 entry points,
// bf16 or fp16 for the _16 one.  wide: a _wide entry point (attention_operands).
template <typename E>
static int attention_forward(const char *what, spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, bool sum_group, float scale,
                             int k, const E *d_Q, int64_t ldq, const E *d_K, int64_t ldk, int kv, const E *d_V,
                             int64_t ldv, E *d_O, int64_t ldo, float *d_stats, void *stream, const AttnBias *bb = nullptr, bool wide = false)
{
    if (int rc = attention_header(h, hs, group, what)) return rc;
    const int64_t rows = h->rows, cols = h->cols;
    const AttnOperand ops[] = {{"Q", d_Q, ldq, rows, k, hs->q, 4, kIn, kQHeads}, {"K", d_K, ldk, cols, k, hs->k, 4, kIn, kKVHeads},
                               {"V", d_V, ldv, cols, kv, hs->v, 4, kIn, kKVHeads}, {"O", d_O, ldo, rows, kv, hs->o, 4, kOut, kQHeads},
                               {"stats", d_stats, 0, rows, 2, hs->stats, 2, kOut, kQHeads}};
    if (int rc = attention_operands(h, hs->heads, group, scale, k, kv, ops, sizeof ops / sizeof *ops, (int)sizeof(E), what, wide)) return rc;
    AttnArgsT<E> a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = d_Q, a.ldq = ldq, a.hq = hs->q, a.K = d_K, a.ldk = ldk, a.hk = hs->k, a.V = d_V, a.ldv = ldv, a.hv = hs->v;
    a.out0 = d_O, a.ld0 = ldo, a.h0 = hs->o, a.stats = d_stats, a.hstats = hs->stats;
    return launch_attention(kPassForward, *h, a, bb, hs->heads, group, sum_group, what, (hipStream_t)stream);
}

template <typename E>
static int attention_backward_q(const char *what, spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, bool sum_group, float scale,
                                int k, const E *d_Q, int64_t ldq, const E *d_K, int64_t ldk, int kv, const E *d_V,
                                int64_t ldv, const E *d_O, int64_t ldo, const E *d_dO, int64_t lddo, const float *d_stats,
                                float *d_delta, E *d_dQ, int64_t lddq, void *stream, const AttnBias *bb = nullptr, bool wide = false)
{
    if (int rc = attention_header(h, hs, group, what)) return rc;
    const int64_t rows = h->rows, cols = h->cols;
    const AttnOperand ops[] = {{"Q", d_Q, ldq, rows, k, hs->q, 4, kIn, kQHeads}, {"K", d_K, ldk, cols, k, hs->k, 4, kIn, kKVHeads},
                               {"V", d_V, ldv, cols, kv, hs->v, 4, kIn, kKVHeads}, {"O", d_O, ldo, rows, kv, hs->o, 4, kIn, kQHeads},
                               {"dO", d_dO, lddo, rows, kv, hs->d_o, 4, kIn, kQHeads}, {"stats", d_stats, 0, rows, 2, hs->stats, 2, kIn, kQHeads},
                               {"delta", d_delta, 0, rows, 1, hs->delta, 1, kOut, kQHeads}, {"dQ", d_dQ, lddq, rows, k, hs->dq, 4, kOut, kQHeads}};
    if (int rc = attention_operands(h, hs->heads, group, scale, k, kv, ops, sizeof ops / sizeof *ops, (int)sizeof(E), what, wide)) return rc;
    AttnArgsT<E> a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = d_Q, a.ldq = ldq, a.hq = hs->q, a.K = d_K, a.ldk = ldk, a.hk = hs->k, a.V = d_V, a.ldv = ldv, a.hv = hs->v;
    a.O = d_O, a.ldo = ldo, a.ho = hs->o, a.dO = d_dO, a.lddo = lddo, a.hdo = hs->d_o;
    a.stats_in = d_stats, a.hstats_in = hs->stats, a.delta = d_delta, a.hdelta = hs->delta, a.out0 = d_dQ, a.ld0 = lddq, a.h0 = hs->dq;
    return launch_attention(kPassBackwardQ, *h, a, bb, hs->heads, group, sum_group, what, (hipStream_t)stream);
}

// t is the handle of the TRANSPOSED pattern: t->rows keys, t->cols queries.  dK and dV hold the K/V heads (the output-stride
// rule counts those).
template <typename E>
static int attention_backward_kv(const char *what, spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, bool sum_group, float scale,
                                 int k, const E *d_Q, int64_t ldq, const E *d_K, int64_t ldk, int kv, const E *d_V,
                                 int64_t ldv, const E *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                 E *d_dK, int64_t lddk, E *d_dV, int64_t lddv, void *stream, const AttnBias *bb = nullptr, bool wide = false)
{
    if (int rc = attention_header(t, hs, group, what)) return rc;
    const int64_t keys = t->rows, queries = t->cols;
    const AttnOperand ops[] = {{"Q", d_Q, ldq, queries, k, hs->q, 4, kIn, kQHeads}, {"K", d_K, ldk, keys, k, hs->k, 4, kIn, kKVHeads},
                               {"V", d_V, ldv, keys, kv, hs->v, 4, kIn, kKVHeads}, {"dO", d_dO, lddo, queries, kv, hs->d_o, 4, kIn, kQHeads},
                               {"stats", d_stats, 0, queries, 2, hs->stats, 2, kIn, kQHeads},
                               {"delta", d_delta, 0, queries, 1, hs->delta, 1, kIn, kQHeads}, {"dK", d_dK, lddk, keys, k, hs->dk, 4, kOut, kKVHeads},
                               {"dV", d_dV, lddv, keys, kv, hs->dv, 4, kOut, kKVHeads}};
    if (int rc = attention_operands(t, hs->heads, group, scale, k, kv, ops, sizeof ops / sizeof *ops, (int)sizeof(E), what, wide)) return rc;
    AttnArgsT<E> a{};
    a.scale = scale, a.k = k, a.kv = kv;
    a.Q = d_Q, a.ldq = ldq, a.hq = hs->q, a.K = d_K, a.ldk = ldk, a.hk = hs->k, a.V = d_V, a.ldv = ldv, a.hv = hs->v;
    a.dO = d_dO, a.lddo = lddo, a.hdo = hs->d_o;
    a.stats_in = d_stats, a.hstats_in = hs->stats, a.delta_in = d_delta, a.hdelta_in = hs->delta;
    a.out0 = d_dK, a.ld0 = lddk, a.h0 = hs->dk, a.out1 = d_dV, a.ld1 = lddv, a.h1 = hs->dv;
    return launch_attention(kPassBackwardKV, *t, a, bb, hs->heads, group, sum_group, what, (hipStream_t)stream);
}

}  // extern "C++"

// ---- the nine entry points: one head (kOneHead), the heads of one pattern in one launch, grouped-query heads ----------------
int spmv_csr_attention_forward(spmv_csr_t *h, float scale, int k, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                               int kv, const float *d_V, int64_t ldv, float *d_O, int64_t ldo, float *d_stats, void *stream)
{
    return attention_forward("spmv_csr_attention_forward", h, &kOneHead, 1, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv, d_O, ldo,
                             d_stats, stream);
}

int spmv_csr_attention_backward_q(spmv_csr_t *h, float scale, int k, const float *d_Q, int64_t ldq, const float *d_K,
                                  int64_t ldk, int kv, const float *d_V, int64_t ldv, const float *d_O, int64_t ldo,
                                  const float *d_dO, int64_t lddo, const float *d_stats, float *d_delta, float *d_dQ,
                                  int64_t lddq, void *stream)
{
    return attention_backward_q("spmv_csr_attention_backward_q", h, &kOneHead, 1, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv, d_O,
                                ldo, d_dO, lddo, d_stats, d_delta, d_dQ, lddq, stream);
}

int spmv_csr_attention_backward_kv(spmv_csr_t *t, float scale, int k, const float *d_Q, int64_t ldq, const float *d_K,
                                   int64_t ldk, int kv, const float *d_V, int64_t ldv, const float *d_dO, int64_t lddo,
                                   const float *d_stats, const float *d_delta, float *d_dK, int64_t lddk, float *d_dV,
                                   int64_t lddv, void *stream)
{
    return attention_backward_kv("spmv_csr_attention_backward_kv", t, &kOneHead, 1, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv,
                                 d_dO, lddo, d_stats, d_delta, d_dK, lddk, d_dV, lddv, stream);
}

int spmv_csr_attention_forward_heads(spmv_csr_t *h, const spmv_attn_heads_t *hs, float scale, int k, const float *d_Q,
                                     int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V, int64_t ldv,
                                     float *d_O, int64_t ldo, float *d_stats, void *stream)
{
    return attention_forward("spmv_csr_attention_forward_heads", h, hs, 1, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv, d_O, ldo,
                             d_stats, stream);
}

int spmv_csr_attention_backward_q_heads(spmv_csr_t *h, const spmv_attn_heads_t *hs, float scale, int k, const float *d_Q,
                                        int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V, int64_t ldv,
                                        const float *d_O, int64_t ldo, const float *d_dO, int64_t lddo, const float *d_stats,
                                        float *d_delta, float *d_dQ, int64_t lddq, void *stream)
{
    return attention_backward_q("spmv_csr_attention_backward_q_heads", h, hs, 1, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv, d_O,
                                ldo, d_dO, lddo, d_stats, d_delta, d_dQ, lddq, stream);
}

int spmv_csr_attention_backward_kv_heads(spmv_csr_t *t, const spmv_attn_heads_t *hs, float scale, int k, const float *d_Q,
                                         int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V, int64_t ldv,
                                         const float *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                         float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, void *stream)
{
    return attention_backward_kv("spmv_csr_attention_backward_kv_heads", t, hs, 1, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv,
                                 d_dO, lddo, d_stats, d_delta, d_dK, lddk, d_dV, lddv, stream);
}

int spmv_csr_attention_forward_gqa(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, float scale, int k, const float *d_Q,
                                   int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V, int64_t ldv,
                                   float *d_O, int64_t ldo, float *d_stats, void *stream)
{
    return attention_forward("spmv_csr_attention_forward_gqa", h, hs, group, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv, d_O, ldo,
                             d_stats, stream);
}

int spmv_csr_attention_backward_q_gqa(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, float scale, int k,
                                      const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V,
                                      int64_t ldv, const float *d_O, int64_t ldo, const float *d_dO, int64_t lddo,
                                      const float *d_stats, float *d_delta, float *d_dQ, int64_t lddq, void *stream)
{
    return attention_backward_q("spmv_csr_attention_backward_q_gqa", h, hs, group, false, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv, d_O,
                                ldo, d_dO, lddo, d_stats, d_delta, d_dQ, lddq, stream);
}

int spmv_csr_attention_backward_kv_gqa(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, float scale, int k,
                                       const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V,
                                       int64_t ldv, const float *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                       float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, void *stream)
{
    return attention_backward_kv("spmv_csr_attention_backward_kv_gqa", t, hs, group, true, scale, k, d_Q, ldq, d_K, ldk, kv, d_V, ldv,
                                 d_dO, lddo, d_stats, d_delta, d_dK, lddk, d_dV, lddv, stream);
}

// ---- the same three passes on 16-bit matrices (bf16 or fp16 storage, fp32 sums): the most general form only ---------------
int spmv_csr_attention_forward_16(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, float scale, int k,
                                  const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv,
                                  void *d_O, int64_t ldo, float *d_stats, void *stream)
{
    const char *what = "spmv_csr_attention_forward_16";
    if (int rc = attention_header(h, hs, group, what)) return rc;
    if (int rc = dtype_ok(dtype, false, what)) return rc;
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_forward<E>(what, h, hs, group, false, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V, ldv,
                                    (E *)d_O, ldo, d_stats, stream);
    });
}

int spmv_csr_attention_backward_q_16(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, float scale, int k,
                                     const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V,
                                     int64_t ldv, const void *d_O, int64_t ldo, const void *d_dO, int64_t lddo,
                                     const float *d_stats, float *d_delta, void *d_dQ, int64_t lddq, void *stream)
{
    const char *what = "spmv_csr_attention_backward_q_16";
    if (int rc = attention_header(h, hs, group, what)) return rc;
    if (int rc = dtype_ok(dtype, false, what)) return rc;
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_backward_q<E>(what, h, hs, group, false, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V,
                                       ldv, (const E *)d_O, ldo, (const E *)d_dO, lddo, d_stats, d_delta, (E *)d_dQ, lddq, stream);
    });
}

int spmv_csr_attention_backward_kv_16(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, int dtype, float scale, int k,
                                      const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V,
                                      int64_t ldv, const void *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                      void *d_dK, int64_t lddk, void *d_dV, int64_t lddv, void *stream)
{
    const char *what = "spmv_csr_attention_backward_kv_16";
    if (int rc = attention_header(t, hs, group, what)) return rc;
    if (int rc = dtype_ok(dtype, false, what)) return rc;
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_backward_kv<E>(what, t, hs, group, true, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V,
                                        ldv, (const E *)d_dO, lddo, d_stats, d_delta, (E *)d_dK, lddk, (E *)d_dV, lddv, stream);
    });
}

// ---- the same three passes with an additive fp32 bias per nonzero (fp32, bf16 or fp16 matrices): the most general form only ------
// What the _bias calls check of their bias arguments, after the header and the dtype and before everything the unbiased call
// of that dtype checks.  d_dbias: backward_q's output (may be null: not written); has_dbias: the call has one at all.
// optional: a _wide call, where a null bias means no bias (and then a dBias is refused).
static int attention_bias(const spmv_csr_t *h, int heads, int dtype, const float *d_bias, int64_t bias_stride, bool has_dbias,
                          const float *d_dbias, int64_t dbias_stride, const char *what, bool optional = false)
{
    if (int rc = dtype_ok(dtype, true, what)) return rc;
    if (optional) {
        if (!d_bias && d_dbias) { set_error("%s: dBias without a bias", what); return SPMV_ERR_INVALID; }
    } else if (!d_bias && h->nnz > 0) { set_error("%s: null bias", what); return SPMV_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(d_bias) % 4 != 0 || reinterpret_cast<uintptr_t>(d_dbias) % 4 != 0) {
        set_error("%s: bias and dBias must be 4-byte aligned", what);
        return SPMV_ERR_INVALID;
    }
    if (bias_stride < 0 || (has_dbias && dbias_stride < 0)) {
        set_error("%s: head stride of the bias = %lld or of dBias = %lld is negative", what, (long long)bias_stride,
                  (long long)(has_dbias ? dbias_stride : 0));
        return SPMV_ERR_INVALID;
    }
    if (bias_stride > INT64_MAX / 4 / heads || (has_dbias && dbias_stride > INT64_MAX / 4 / heads)) {
        set_error("%s: head stride of the bias or of dBias overflows 64-bit byte offsets", what);
        return SPMV_ERR_INVALID;
    }
    if (d_dbias && heads > 1 && dbias_stride < h->nnz) {
        set_error("%s: head stride of the output dBias = %lld is below nnz = %lld", what, (long long)dbias_stride, (long long)h->nnz);
        return SPMV_ERR_INVALID;
    }
    return SPMV_OK;
}

int spmv_csr_attention_forward_bias(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias,
                                    int64_t bias_stride, float scale, int k, const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk,
                                    int kv, const void *d_V, int64_t ldv, void *d_O, int64_t ldo, float *d_stats, void *stream)
{
    const char *what = "spmv_csr_attention_forward_bias";
    if (int rc = attention_header(h, hs, group, what)) return rc;
    if (int rc = attention_bias(h, hs->heads, dtype, d_bias, bias_stride, false, nullptr, 0, what)) return rc;
    const AttnBias bb{d_bias, bias_stride, nullptr, 0};
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_forward<E>(what, h, hs, group, false, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V, ldv,
                                    (E *)d_O, ldo, d_stats, stream, &bb);
    });
}

int spmv_csr_attention_backward_q_bias(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias,
                                       int64_t bias_stride, float *d_dbias, int64_t dbias_stride, float scale, int k, const void *d_Q,
                                       int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv, const void *d_O,
                                       int64_t ldo, const void *d_dO, int64_t lddo, const float *d_stats, float *d_delta, void *d_dQ,
                                       int64_t lddq, void *stream)
{
    const char *what = "spmv_csr_attention_backward_q_bias";
    if (int rc = attention_header(h, hs, group, what)) return rc;
    if (int rc = attention_bias(h, hs->heads, dtype, d_bias, bias_stride, true, d_dbias, dbias_stride, what)) return rc;
    const AttnBias bb{d_bias, bias_stride, d_dbias, dbias_stride};
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_backward_q<E>(what, h, hs, group, false, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V,
                                       ldv, (const E *)d_O, ldo, (const E *)d_dO, lddo, d_stats, d_delta, (E *)d_dQ, lddq, stream, &bb);
    });
}

int spmv_csr_attention_backward_kv_bias(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias_t,
                                        int64_t bias_stride, float scale, int k, const void *d_Q, int64_t ldq, const void *d_K,
                                        int64_t ldk, int kv, const void *d_V, int64_t ldv, const void *d_dO, int64_t lddo,
                                        const float *d_stats, const float *d_delta, void *d_dK, int64_t lddk, void *d_dV, int64_t lddv,
                                        void *stream)
{
    const char *what = "spmv_csr_attention_backward_kv_bias";
    if (int rc = attention_header(t, hs, group, what)) return rc;
    if (int rc = attention_bias(t, hs->heads, dtype, d_bias_t, bias_stride, false, nullptr, 0, what)) return rc;
    const AttnBias bb{d_bias_t, bias_stride, nullptr, 0};
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_backward_kv<E>(what, t, hs, group, true, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V,
                                        ldv, (const E *)d_dO, lddo, d_stats, d_delta, (E *)d_dK, lddk, (E *)d_dV, lddv, stream, &bb);
    });
}

// ---- the same three passes at widths up to 128: the _bias calls' arguments, an optional bias, the plan of _plan_wide -----------
// Up to width 64 they launch what the _bias call (or, without a bias, the _gqa or _16 call) launches; above, the kernels at
// V = 32 (kernels_attention.hip).  A null bias means none: the unbiased kernels run.
int spmv_csr_attention_forward_wide(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias,
                                    int64_t bias_stride, float scale, int k, const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk,
                                    int kv, const void *d_V, int64_t ldv, void *d_O, int64_t ldo, float *d_stats, void *stream)
{
    const char *what = "spmv_csr_attention_forward_wide";
    if (int rc = attention_header(h, hs, group, what)) return rc;
    if (int rc = attention_bias(h, hs->heads, dtype, d_bias, bias_stride, false, nullptr, 0, what, true)) return rc;
    const AttnBias bb{d_bias, bias_stride, nullptr, 0};
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_forward<E>(what, h, hs, group, false, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V, ldv,
                                    (E *)d_O, ldo, d_stats, stream, d_bias ? &bb : nullptr, true);
    });
}

int spmv_csr_attention_backward_q_wide(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias,
                                       int64_t bias_stride, float *d_dbias, int64_t dbias_stride, float scale, int k, const void *d_Q,
                                       int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv, const void *d_O,
                                       int64_t ldo, const void *d_dO, int64_t lddo, const float *d_stats, float *d_delta, void *d_dQ,
                                       int64_t lddq, void *stream)
{
    const char *what = "spmv_csr_attention_backward_q_wide";
    if (int rc = attention_header(h, hs, group, what)) return rc;
    if (int rc = attention_bias(h, hs->heads, dtype, d_bias, bias_stride, true, d_dbias, dbias_stride, what, true)) return rc;
    const AttnBias bb{d_bias, bias_stride, d_dbias, dbias_stride};
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_backward_q<E>(what, h, hs, group, false, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V,
                                       ldv, (const E *)d_O, ldo, (const E *)d_dO, lddo, d_stats, d_delta, (E *)d_dQ, lddq, stream,
                                       d_bias ? &bb : nullptr, true);
    });
}

int spmv_csr_attention_backward_kv_wide(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias_t,
                                        int64_t bias_stride, float scale, int k, const void *d_Q, int64_t ldq, const void *d_K,
                                        int64_t ldk, int kv, const void *d_V, int64_t ldv, const void *d_dO, int64_t lddo,
                                        const float *d_stats, const float *d_delta, void *d_dK, int64_t lddk, void *d_dV, int64_t lddv,
                                        void *stream)
{
    const char *what = "spmv_csr_attention_backward_kv_wide";
    if (int rc = attention_header(t, hs, group, what)) return rc;
    if (int rc = attention_bias(t, hs->heads, dtype, d_bias_t, bias_stride, false, nullptr, 0, what, true)) return rc;
    const AttnBias bb{d_bias_t, bias_stride, nullptr, 0};
    return with_element(dtype, [&](auto e) {
        using E = decltype(e);
        return attention_backward_kv<E>(what, t, hs, group, true, scale, k, (const E *)d_Q, ldq, (const E *)d_K, ldk, kv, (const E *)d_V,
                                        ldv, (const E *)d_dO, lddo, d_stats, d_delta, (E *)d_dK, lddk, (E *)d_dV, lddv, stream,
                                        d_bias_t ? &bb : nullptr, true);
    });
}

int spmv_csr_values_changed(spmv_csr_t *h)
{
    if (!h) { set_error("spmv_csr_values_changed: null handle"); return SPMV_ERR_INVALID; }
    ++h->values_gen;
    return SPMV_OK;
}

int spmv_csr_plan_get(const spmv_csr_t *h, int variant, int32_t params[8])
{
    if (!h || !params) { set_error("spmv_csr_plan_get: null argument"); return SPMV_ERR_INVALID; }
    for (int i = 0; i < 8; ++i) params[i] = 0;
    const bool is_auto = variant == SPMV_AUTO;
    if (variant == SPMV_AUTO) {
        if (h->auto_variant < 0) { set_error("spmv_csr_plan_get: SPMV_AUTO is not planned"); return SPMV_ERR_NOT_PLANNED; }
        variant = h->auto_variant;
    }
    const PanelPlan &panel = is_auto ? h->plan_auto_panel : h->plan_panel;
    params[0] = variant;
    switch (variant) {
        case SPMV_SCALAR: case SPMV_WAVE: case SPMV_WAVE_PIPE: return SPMV_OK;
        case SPMV_VECTOR: params[1] = h->vector_width; return SPMV_OK;
        case SPMV_ADAPTIVE:
        case SPMV_TILED: {
            const ChunkPlan &p = variant == SPMV_TILED ? h->plan_tiled : h->plan_adaptive;
            if (!p.block) { set_error("spmv_csr_plan_get: variant %d is not planned", variant); return SPMV_ERR_NOT_PLANNED; }
            params[1] = p.block; params[2] = p.maxpass; params[3] = p.col16_wanted ? 1 : 0;
            return SPMV_OK;
        }
        case SPMV_XSKIP:
            if (!h->plan_xskip.ready) { set_error("spmv_csr_plan_get: xskip is not planned"); return SPMV_ERR_NOT_PLANNED; }
            params[1] = h->plan_xskip.slabs;
            return SPMV_OK;
        case SPMV_PANEL:
            if (panel.layout == PanelLayout::none) { set_error("spmv_csr_plan_get: panel is not planned"); return SPMV_ERR_NOT_PLANNED; }
            panel_params(panel, params);
            return SPMV_OK;
        default: set_error("spmv_csr_plan_get: unknown variant %d", variant); return SPMV_ERR_VARIANT;
    }
}

int spmv_csr_plan_set(spmv_csr_t *h, int variant, const int32_t params[8], void *stream)
{
    if (!h || !params) { set_error("spmv_csr_plan_set: null argument"); return SPMV_ERR_INVALID; }
    if (int rc = require_current(h->device, "spmv_csr_plan_set")) return rc;
    hipStream_t s = (hipStream_t)stream;
    int target = variant;
    if (variant == SPMV_AUTO) {
        target = params[0];
        if (target != SPMV_TILED && target != SPMV_PANEL) {
            set_error("spmv_csr_plan_set: SPMV_AUTO resolves to tiled or panel, not %d", target);
            return SPMV_ERR_INVALID;
        }
    } else if (params[0] != variant) {
        set_error("spmv_csr_plan_set: params describe variant %d, not %d", params[0], variant);
        return SPMV_ERR_INVALID;
    }
    int rc;
    switch (target) {
        case SPMV_SCALAR: case SPMV_WAVE: case SPMV_WAVE_PIPE: rc = SPMV_OK; break;
        case SPMV_VECTOR: {
            const int w = params[1];
            if (w != 2 && w != 4 && w != 8 && w != 16 && w != 32) { set_error("spmv_csr_plan_set: lanes per row %d", w); return SPMV_ERR_INVALID; }
            h->vector_width = w;
            rc = SPMV_OK;
            break;
        }
        case SPMV_ADAPTIVE: rc = plan_adaptive_with(*h, params[1], s); break;
        case SPMV_TILED: rc = plan_tiled_with(*h, params[1], params[2], params[3] != 0, s); break;
        case SPMV_PANEL: rc = build_panel(*h, variant == SPMV_AUTO ? h->plan_auto_panel : h->plan_panel, params[4], params[5], params[6], s); break;
        case SPMV_XSKIP: h->plan_xskip = XskipPlan{}; rc = plan_xskip(*h, s); break;   // always rebuilt: the values are a copy
        default: set_error("spmv_csr_plan_set: unknown variant %d", target); return SPMV_ERR_VARIANT;
    }
    if (rc == SPMV_OK && variant == SPMV_AUTO) h->auto_variant = target;
    return rc;
}

int spmv_csr_plan_like(spmv_csr_t *dst, const spmv_csr_t *src, int variant, void *stream)
{
    int32_t params[8];
    int rc = spmv_csr_plan_get(src, variant, params);
    return rc ? rc : spmv_csr_plan_set(dst, variant, params, stream);
}

int64_t spmv_csr_plan_bytes(const spmv_csr_t *h, int variant)
{
    if (!h) return 0;
    const PanelPlan &panel = variant == SPMV_AUTO ? h->plan_auto_panel : h->plan_panel;
    if (variant == SPMV_AUTO) variant = h->auto_variant;
    switch (variant) {
        case SPMV_ADAPTIVE:  // chunk_lb read + carry written and re-read
            return (int64_t)(h->plan_adaptive.nchunks + 1) * 4 + (int64_t)h->plan_adaptive.nchunks * 8;
        case SPMV_TILED:     // + the two window words per chunk, the chunk lists, the 16-bit offsets and the sorted words
                             // (identity order: no lists, one slot word per chunk where some chunks are sorted)
            return (int64_t)(h->plan_tiled.nchunks + 1) * 4 + (int64_t)h->plan_tiled.nchunks * 16 +
                   ((h->plan_tiled.identity_order ? h->plan_tiled.nsorted : (h->plan_tiled.n16 || h->plan_tiled.nsorted))
                        ? (int64_t)h->plan_tiled.nchunks * 4 : 0) +
                   (int64_t)h->plan_tiled.n16 * 2 * h->plan_tiled.block * kNnzPerThread +
                   (int64_t)h->plan_tiled.nsorted * 4 * h->plan_tiled.block * kNnzPerThread +
                   (int64_t)h->plan_tiled.nblk_chunks * 256 * 4;   // block lists: up to 256 ids per chunk that has one
        case SPMV_XSKIP:     // segment list + slab partials; erow16/evals (6 B per nonzero) REPLACE col_idx/vals (8 B)
            return (int64_t)h->plan_xskip.nseg * 8 + ((int64_t)h->plan_xskip.nblocks + 1) * 4 +
                   (h->plan_xskip.slabs > 1 ? (int64_t)h->plan_xskip.nblocks * h->plan_xskip.slabs * 1024 * 8 : 0);
        case SPMV_PANEL: return panel_plan_bytes(panel, h->nnz);   // (its arrays REPLACE col_idx/vals: what comes on top of them)
        case SPMV_WAVE:      // (short rows: the same plan without the windows and the offsets; long rows: none)
            if (h->nnz > 32 * h->rows) return 0;
            return (int64_t)h->plan_wave.n_long * 8 + (int64_t)h->plan_wave.pieces * 16;
        case SPMV_SCALAR:    // (the same plan; the ordered kernel does not use the pieces)
        case SPMV_WAVE_PIPE: // the long rows' list, piece table read, partial sums written and re-read (col16 REPLACES 4 of col_idx's bytes with 2)
            return (int64_t)h->plan_wave.n_long * 8 + (int64_t)h->plan_wave.pieces * 16 + h->plan_wave.blocks * 8;
        default: return 0;
    }
}

int spmv_csr_plan_chunk_order(const spmv_csr_t *h, int variant)
{
    if (!h) { set_error("spmv_csr_plan_chunk_order: null handle"); return SPMV_ERR_INVALID; }
    if (variant == SPMV_AUTO) variant = h->auto_variant;
    if (variant != SPMV_TILED) { set_error("spmv_csr_plan_chunk_order: SPMV_TILED, or SPMV_AUTO resolved to it"); return SPMV_ERR_VARIANT; }
    const ChunkPlan &p = h->plan_tiled;
    if (!p.block) { set_error("SPMV_TILED used before spmv_csr_plan"); return SPMV_ERR_NOT_PLANNED; }
    const bool mixed = !p.persist && (p.n16 > 0 || p.nsorted > 0) && p.n16 != p.nchunks && p.nsorted != p.nchunks;
    return !mixed ? 0 : (p.identity_order ? 2 : 1);
}

int spmv_csr_plan_describe(const spmv_csr_t *h, int variant, char *buf, int n)
{
    if (!h || !buf || n <= 0) { set_error("spmv_csr_plan_describe: bad argument"); return SPMV_ERR_INVALID; }
    const PanelPlan *panel = &h->plan_panel;
    if (variant == SPMV_AUTO) {   // "auto -> <variant>: <that variant's plan>"
        if (h->auto_variant < 0) { snprintf(buf, (size_t)n, "not planned"); return SPMV_OK; }
        const int w = snprintf(buf, (size_t)n, "auto -> %s: ", spmv_variant_name(h->auto_variant));
        if (w < 0 || w >= n) return SPMV_OK;
        if (h->auto_variant != SPMV_PANEL) return spmv_csr_plan_describe(h, h->auto_variant, buf + w, n - w);
        panel = &h->plan_auto_panel;
        variant = SPMV_PANEL;
        buf += w;
        n -= w;
    }
    const ChunkPlan *p = variant == SPMV_ADAPTIVE ? &h->plan_adaptive : (variant == SPMV_TILED ? &h->plan_tiled : nullptr);
    if (variant == SPMV_VECTOR) snprintf(buf, (size_t)n, "lanes_per_row=%d", h->vector_width);
    else if (variant == SPMV_WAVE && h->nnz > 32 * h->rows) snprintf(buf, (size_t)n, "no plan (a wavefront per row)");
    else if (variant == SPMV_WAVE_PIPE || variant == SPMV_SCALAR || variant == SPMV_WAVE) {
        if (!h->plan_wave.ready) snprintf(buf, (size_t)n, "not planned (the first run plans)");
        else snprintf(buf, (size_t)n, "long_rows=%d pieces=%d block_rows=%d blocks=%lld blocks_with_x_window=%lld col16=%d", h->plan_wave.n_long,
                      h->plan_wave.pieces, h->plan_wave.block_rows, (long long)h->plan_wave.blocks, (long long)h->plan_wave.win_blocks,
                      h->plan_wave.d_col16 ? 1 : 0);
    }
    else if (variant == SPMV_PANEL) panel_describe(*panel, *h, buf, n);
    else if (variant == SPMV_XSKIP && h->plan_xskip.ready)
        snprintf(buf, (size_t)n, "output_blocks=%d segments=%d slabs_per_block=%d", h->plan_xskip.nblocks, h->plan_xskip.nseg,
                 h->plan_xskip.slabs);
    else if (!p) snprintf(buf, (size_t)n, "no plan");
    else if (!p->block) snprintf(buf, (size_t)n, "not planned");
    else
        snprintf(buf, (size_t)n, "block=%d region=%d maxpass=%d chunks=%d staged_single=%d staged_full=%d col16_chunks=%d sorted_chunks=%d block_list_chunks=%d spanning_rows=%d persist=%d model_cost=%.3f",
                 p->block, p->region, p->maxpass, p->nchunks, p->staged_single, p->staged_full, p->n16, p->nsorted,
                 p->nblk_chunks, p->spanning_rows, p->persist ? 1 : 0, p->model_cost);
    return SPMV_OK;
}

int spmv_csr_time(spmv_csr_t *h, int variant, const float *d_x, float *d_y, int iters, void *stream,
                  float *ms_per_launch)
{
    if (iters <= 0 || !ms_per_launch) { set_error("spmv_csr_time: bad argument"); return SPMV_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t t0, t1;
    SPMV_HIP_TRY(hipEventCreate(&t0));
    SPMV_HIP_TRY(hipEventCreate(&t1));
    int rc = SPMV_OK;
    SPMV_HIP_TRY(hipEventRecord(t0, s));
    for (int i = 0; i < iters && rc == SPMV_OK; ++i) rc = spmv_csr_run(h, variant, d_x, d_y, s);
    SPMV_HIP_TRY(hipEventRecord(t1, s));
    SPMV_HIP_TRY(hipEventSynchronize(t1));
    float ms = 0.0f;
    SPMV_HIP_TRY(hipEventElapsedTime(&ms, t0, t1));
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    *ms_per_launch = ms / (float)iters;
    return rc;
}

int spmv_csr_run_host(spmv_csr_t *h, int variant, const float *x_host, float *y_host, float *kernel_ms)
{
    if (!h || (!x_host && h->cols > 0) || (!y_host && h->rows > 0)) {
        set_error("spmv_csr_run_host: null argument");
        return SPMV_ERR_INVALID;
    }
    int rc = spmv_csr_plan(h, variant, nullptr);
    if (rc) return rc;
    DevPtr<float> dx, dy;
    SPMV_HIP_TRY(dx.alloc((size_t)h->cols));
    SPMV_HIP_TRY(dy.alloc((size_t)h->rows));
    SPMV_HIP_TRY(hipMemcpy(dx.get(), x_host, sizeof(float) * (size_t)h->cols, hipMemcpyHostToDevice));
    if ((rc = time_cold_then_warm([&] { return spmv_csr_run(h, variant, dx.get(), dy.get(), nullptr); }, kernel_ms)))
        return rc;
    SPMV_HIP_TRY(hipMemcpy(y_host, dy.get(), sizeof(float) * (size_t)h->rows, hipMemcpyDeviceToHost));
    return SPMV_OK;
}

int spmv_dense_gemv_host(int M, int N, const float *A_host, const float *x_host, float *y_host, int mode,
                         float *kernel_ms)
{
    if (M < 0 || N < 0 || ((int64_t)M * N > 0 && (!A_host || !x_host)) || (N > 0 && !y_host)) {
        set_error("spmv_dense_gemv_host: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    DevPtr<float> dA, dx, dy;
    SPMV_HIP_TRY(dA.alloc((size_t)M * (size_t)N));
    SPMV_HIP_TRY(dx.alloc((size_t)M));
    SPMV_HIP_TRY(dy.alloc((size_t)N));
    SPMV_HIP_TRY(hipMemcpy(dA.get(), A_host, sizeof(float) * (size_t)M * (size_t)N, hipMemcpyHostToDevice));
    SPMV_HIP_TRY(hipMemcpy(dx.get(), x_host, sizeof(float) * (size_t)M, hipMemcpyHostToDevice));
    if ((rc = time_cold_then_warm([&] { return dense_gemv(M, N, dA.get(), dx.get(), dy.get(), mode, nullptr); }, kernel_ms)))
        return rc;
    SPMV_HIP_TRY(hipMemcpy(y_host, dy.get(), sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
    return SPMV_OK;
}

static int tcsr_check_dims(int M, int N, const void *A, const void *out)
{
    if (!out || M < 0 || N < 0 || (M % 32) || (N % 32) || (!A && (int64_t)M * N > 0) || (int64_t)M * N >= (1LL << 36)) {
        set_error("spmv_tcsr_from_dense: M and N must be non-negative multiples of 32 (got %d x %d)", M, N);
        return SPMV_ERR_INVALID;
    }
    return require_device();
}

int spmv_tcsr_from_dense_device(int M, int N, const float *d_A, void *stream, spmv_tcsr_t **out)
{
    int rc = tcsr_check_dims(M, N, d_A, out);
    if (rc) return rc;
    return tcsr_from_dense(M, N, d_A, (hipStream_t)stream, out);
}

int spmv_tcsr_from_dense_host(int M, int N, const float *A_host, void *stream, spmv_tcsr_t **out)
{
    int rc = tcsr_check_dims(M, N, A_host, out);
    if (rc) return rc;
    DevPtr<float> dA;
    const size_t bytes = sizeof(float) * (size_t)M * (size_t)N;
    SPMV_HIP_TRY(dA.alloc((size_t)M * (size_t)N));
    SPMV_HIP_TRY(hipMemcpyAsync(dA.get(), A_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = tcsr_from_dense(M, N, dA.get(), (hipStream_t)stream, out);
    (void)hipStreamSynchronize((hipStream_t)stream);
    return rc;
}

int spmv_tcsr_sizes(const spmv_tcsr_t *h, int64_t *n_blk_idx, int64_t *n_bitmaps, int64_t *n_vals)
{
    if (!h) { set_error("spmv_tcsr_sizes: null handle"); return SPMV_ERR_INVALID; }
    return tcsr_sizes(*h, n_blk_idx, n_bitmaps, n_vals);
}

int spmv_tcsr_download(const spmv_tcsr_t *h, int32_t *blk_idx, uint32_t *bitmaps, float *vals)
{
    if (!h) { set_error("spmv_tcsr_download: null handle"); return SPMV_ERR_INVALID; }
    return tcsr_download(*h, blk_idx, bitmaps, vals);
}

int spmv_tcsr_run(const spmv_tcsr_t *h, const float *d_x, float *d_y, void *stream)
{
    if (!h || !d_x || !d_y) { set_error("spmv_tcsr_run: null argument"); return SPMV_ERR_INVALID; }
    return tcsr_run(*h, d_x, d_y, (hipStream_t)stream);
}

int spmv_tcsr_run_host(const spmv_tcsr_t *h, const float *x_host, float *y_host, float *kernel_ms)
{
    if (!h || !x_host || !y_host) { set_error("spmv_tcsr_run_host: null argument"); return SPMV_ERR_INVALID; }
    int64_t nb = 0, nw = 0, nv = 0;
    tcsr_sizes(*h, &nb, &nw, &nv);
    int M = 0, N = 0;
    tcsr_dims(*h, &M, &N);
    DevPtr<float> dx, dy;
    SPMV_HIP_TRY(dx.alloc((size_t)M));
    SPMV_HIP_TRY(dy.alloc((size_t)N));
    SPMV_HIP_TRY(hipMemcpy(dx.get(), x_host, sizeof(float) * (size_t)M, hipMemcpyHostToDevice));
    if (int rc = time_cold_then_warm([&] { return tcsr_run(*h, dx.get(), dy.get(), nullptr); }, kernel_ms)) return rc;
    SPMV_HIP_TRY(hipMemcpy(y_host, dy.get(), sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
    return SPMV_OK;
}

int spmv_tcsr_destroy(spmv_tcsr_t *h)
{
    delete h;
    return SPMV_OK;
}

static int bitmap_check_dims(int format, int M, int N, const void *A, const void *out)
{
    if (format < 0 || format >= SPMV_FMT_COUNT) { set_error("spmv_bitmap_from_dense: unknown format %d", format); return SPMV_ERR_VARIANT; }
    if (!out || M < 0 || N < 0 || (M % 32) || (N % 32) || (!A && (int64_t)M * N > 0) || (int64_t)M * N >= (1LL << 36)) {
        set_error("spmv_bitmap_from_dense: M and N must be non-negative multiples of 32 (got %d x %d)", M, N);
        return SPMV_ERR_INVALID;
    }
    return require_device();
}

int spmv_bitmap_from_dense_device(int format, int M, int N, const float *d_A, void *stream, spmv_bitmap_t **out)
{
    int rc = bitmap_check_dims(format, M, N, d_A, out);
    if (rc) return rc;
    return bitmap_from_dense(format, M, N, d_A, (hipStream_t)stream, out);
}

int spmv_bitmap_from_dense_host(int format, int M, int N, const float *A_host, void *stream, spmv_bitmap_t **out)
{
    int rc = bitmap_check_dims(format, M, N, A_host, out);
    if (rc) return rc;
    DevPtr<float> dA;
    const size_t bytes = sizeof(float) * (size_t)M * (size_t)N;
    SPMV_HIP_TRY(dA.alloc((size_t)M * (size_t)N));
    SPMV_HIP_TRY(hipMemcpyAsync(dA.get(), A_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = bitmap_from_dense(format, M, N, dA.get(), (hipStream_t)stream, out);
    (void)hipStreamSynchronize((hipStream_t)stream);
    return rc;
}

int spmv_bitmap_sizes(const spmv_bitmap_t *h, int64_t *n_bitmaps, int64_t *n_vals, int32_t stats[4])
{
    if (!h) { set_error("spmv_bitmap_sizes: null handle"); return SPMV_ERR_INVALID; }
    bitmap_info(*h, nullptr, nullptr, nullptr, n_bitmaps, n_vals, stats);
    return SPMV_OK;
}

int spmv_bitmap_download(const spmv_bitmap_t *h, uint32_t *bitmaps, float *vals)
{
    if (!h) { set_error("spmv_bitmap_download: null handle"); return SPMV_ERR_INVALID; }
    return bitmap_download(*h, bitmaps, vals);
}

int spmv_bitmap_run(const spmv_bitmap_t *h, const float *d_x, float *d_y, void *stream)
{
    if (!h || !d_x || !d_y) { set_error("spmv_bitmap_run: null argument"); return SPMV_ERR_INVALID; }
    if (int rc = require_current(bitmap_device(*h), "spmv_bitmap_run")) return rc;
    return bitmap_run(*h, d_x, d_y, (hipStream_t)stream);
}

int spmv_bitmap_run_host(const spmv_bitmap_t *h, const float *x_host, float *y_host, float *kernel_ms)
{
    if (!h || !x_host || !y_host) { set_error("spmv_bitmap_run_host: null argument"); return SPMV_ERR_INVALID; }
    int M = 0, N = 0;
    bitmap_info(*h, nullptr, &M, &N, nullptr, nullptr, nullptr);
    DevPtr<float> dx, dy;
    SPMV_HIP_TRY(dx.alloc((size_t)M));
    SPMV_HIP_TRY(dy.alloc((size_t)N));
    SPMV_HIP_TRY(hipMemcpy(dx.get(), x_host, sizeof(float) * (size_t)M, hipMemcpyHostToDevice));
    if (int rc = time_cold_then_warm([&] { return bitmap_run(*h, dx.get(), dy.get(), nullptr); }, kernel_ms)) return rc;
    SPMV_HIP_TRY(hipMemcpy(y_host, dy.get(), sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
    return SPMV_OK;
}

int spmv_bitmap_destroy(spmv_bitmap_t *h)
{
    delete h;
    return SPMV_OK;
}

int spmv_dense_gemv(int M, int N, const float *d_A, const float *d_x, float *d_y, int mode, void *stream)
{
    if (M < 0 || N < 0 || ((int64_t)M * N > 0 && (!d_A || !d_x)) || (N > 0 && !d_y)) {
        set_error("spmv_dense_gemv: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    return dense_gemv(M, N, d_A, d_x, d_y, mode, (hipStream_t)stream);
}

int64_t spmv_dense_gemv_workspace_bytes(int N, int mode) { return (int64_t)dense_gemv_workspace_bytes(N, mode); }

int spmv_dense_gemv_ws(int M, int N, const float *d_A, const float *d_x, float *d_y, int mode, void *d_workspace,
                       int64_t workspace_bytes, void *stream)
{
    if (M < 0 || N < 0 || ((int64_t)M * N > 0 && (!d_A || !d_x)) || (N > 0 && !d_y) || workspace_bytes < 0) {
        set_error("spmv_dense_gemv_ws: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    return dense_gemv_ws(M, N, d_A, d_x, d_y, mode, d_workspace, (size_t)workspace_bytes, (hipStream_t)stream);
}

int spmv_asp_retile(int M, int N, const float *d_A, float *d_asp, void *stream)
{
    if (M < 0 || N < 0 || (M % 32) || (N % 32) || ((int64_t)M * N > 0 && (!d_A || !d_asp))) {
        set_error("spmv_asp_retile: bad argument (M and N are multiples of 32, like the reference's tester asserts)");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    return asp_retile(M, N, d_A, d_asp, (hipStream_t)stream);
}

int spmv_asp_gemv_ws(int M, int N, const float *d_asp, const float *d_x, float *d_y, void *d_workspace, int64_t workspace_bytes,
                     void *stream)
{
    if (M < 0 || N < 0 || (M % 32) || (N % 32) || ((int64_t)M * N > 0 && (!d_asp || !d_x)) || (N > 0 && !d_y) ||
        workspace_bytes < 0) {
        set_error("spmv_asp_gemv_ws: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    return asp_gemv_ws(M, N, d_asp, d_x, d_y, d_workspace, (size_t)workspace_bytes, (hipStream_t)stream);
}

int spmv_synth_fill(uint64_t seed, int64_t row0, int64_t n_local, int64_t rows, int64_t cols, int64_t band,
                    const int32_t *d_row_ptr, int32_t *d_col_idx, float *d_vals, void *stream)
{
    if (n_local < 0 || row0 < 0 || row0 + n_local > rows || cols <= 0 || cols >= (1LL << 31) ||
        rows >= (1LL << 31) || !d_row_ptr) {
        set_error("spmv_synth_fill: bad argument");
        return SPMV_ERR_INVALID;
    }
    int rc = require_device();
    if (rc) return rc;
    return synth_fill(seed, row0, n_local, rows, cols, band, d_row_ptr, d_col_idx, d_vals, (hipStream_t)stream);
}

int spmv_synth_x(uint64_t seed, int64_t j0, int64_t n, float *d_x, void *stream)
{
    if (n < 0 || j0 < 0 || (n > 0 && !d_x)) { set_error("spmv_synth_x: bad argument"); return SPMV_ERR_INVALID; }
    int rc = require_device();
    if (rc) return rc;
    return synth_x(seed, j0, n, d_x, (hipStream_t)stream);
}

}  // extern "C"
