/*
 * spmv_hip.h -- C ABI of libspmv_hip.so: the MI355X (gfx950) fp32 CSR SpMV hot path.
 *
 * This is the drop-in boundary underneath the reference's launcher surface
 * (/root/reference/src/include/kernel.hpp:8-17).  The reference launchers are
 * C++ free functions that take a dense host matrix; include/kernel.hpp in this
 * repo re-declares them unchanged and spmv-test_amd/host/launchers.cpp
 * implements them on top of the entry points below.  Every entry point is
 * extern "C", takes plain pointers and sizes, and returns 0 on success or a
 * negative spmv_status code; spmv_last_error() then holds a message.  Nothing
 * here falls back to the CPU: without a HIP device every compute entry point
 * fails with SPMV_ERR_NO_DEVICE.
 *
 * Conventions (from matrix_csr.cpp:8-22):
 *   CSR row i   = output index i in [0, rows)   (column i of the dense A)
 *   column idx  = input index j in [0, cols)    (row j of the dense A)
 *   y[i] = sum_k vals[k] * x[col_idx[k]],  k in [row_ptr[i], row_ptr[i+1])
 *   Every term of row i counts and nothing else does: a column may repeat
 *   (each occurrence adds its term), rows need not be sorted, IEEE rules hold
 *   (Inf * 0 = NaN, +Inf + -Inf = NaN, subnormals kept), an x entry no row
 *   refers to is never read into a sum, and an empty row is 0.  Only the
 *   order of the fp32 additions is the variant's own.  SPMV_XSKIP differs
 *   (see the enum): it leaves out the terms whose x is +-0.
 *   row_ptr has rows+1 int32 entries (row_ptr[rows] == nnz); the reference's
 *   CSRMatrix omits the last one and csr_naive.cu:15 substitutes nnz for it.
 *   nnz < 2^31 per handle; larger problems are row-block shards, one handle each.
 */
#ifndef SPMV_HIP_H
#define SPMV_HIP_H

#include <stdint.h>

#if defined(__GNUC__)
#define SPMV_API __attribute__((visibility("default")))
#else
#define SPMV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmv_csr spmv_csr_t;

enum spmv_status {
    SPMV_OK = 0,
    SPMV_ERR_NO_DEVICE = -1, /* no HIP device visible: there is no CPU path      */
    SPMV_ERR_INVALID = -2,   /* bad argument (null, negative size, misaligned)   */
    SPMV_ERR_HIP = -3,       /* a HIP runtime call failed (message has details)  */
    SPMV_ERR_VARIANT = -4,   /* unknown variant id (reference: silently no-op,   */
                             /* wsp.cu:187 -- here it is reported)               */
    SPMV_ERR_NOT_PLANNED = -5,
    SPMV_ERR_STALE_PLAN = -6 /* the variant's plan holds a COPY of vals taken before   */
                             /* spmv_csr_values_changed (or, under SPMV_CHECK_VALUES=1,*/
                             /* before the array changed): re-plan                     */
};

/* Kernel variants.  The right-hand column is the reference slot each one
 * replaces (file:line in /root/reference) -- same role, re-derived for CSR on
 * 64-lane wavefronts, not a translation of the bitmap kernels. */
enum spmv_variant {
    SPMV_SCALAR = 0,    /* thread per row, k ascending, mul+add unfused:           */
                        /*   csr_naive_kernel      src/kernels/csr_naive.cu:6-23   */
                        /*   (bit-identical to SgemvCPU, src/tester.cpp:36-45).    */
                        /* Shares SPMV_WAVE_PIPE's plan (operands only; see there). */
    SPMV_WAVE = 1,      /* 64-lane wavefronts + __shfl_down reduction:             */
                        /*   wsp_kernel_v0         src/kernels/wsp.cu:4-56         */
                        /* Rows of mean > 32 nonzeros: a wavefront per row.  Shorter */
                        /* rows (round 4): a wavefront per 64 rows as in            */
                        /* SPMV_WAVE_PIPE -- coalesced streams, a lane per short row, */
                        /* the wave + __shfl_down per longer one, the longest in     */
                        /* pieces -- but x gathered from memory: no window in LDS,   */
                        /* no 16-bit offsets (the plain kernel of the pair).  Shares */
                        /* SPMV_WAVE_PIPE's plan there (the long rows' pieces).      */
    SPMV_WAVE_PIPE = 2, /* a wavefront per 64 rows: their nonzeros streamed        */
                        /* coalesced with all loads of a run in flight, products    */
                        /* parked in LDS, a lane per short row, the wave +          */
                        /* __shfl_down per longer one; rows of more than 512        */
                        /* nonzeros in pieces, a wavefront per piece; x from a      */
                        /* window in LDS per block of rows where the columns fit:   */
                        /*   wsp_kernel_v1         src/kernels/wsp.cu:59-138       */
                        /* Plan: the long rows and the windows, a function of       */
                        /* row_ptr and col_idx (NOT of the values).  A handle that  */
                        /* was not planned plans on its first run (allocates and    */
                        /* waits for the stream once: call spmv_csr_plan before     */
                        /* capturing a graph).                                      */
    SPMV_VECTOR = 3,    /* 2..32-lane groups per row, width from mean row length:  */
                        /*   asp_kernel_v0/1/2     src/kernels/asp.cu:6-211        */
    SPMV_ADAPTIVE = 4,  /* nnz-balanced chunks, products staged in LDS, per-chunk  */
                        /* adaptive row reduction, deterministic carry fix-up:     */
                        /*   awsp_kernel_v0/1/2    src/kernels/awsp.cu:5-317,      */
                        /*   awsp_ref_kernel       src/kernels/awsp_ref.cu:6-185   */
    SPMV_TILED = 5,     /* ADAPTIVE + the chunk's window of x staged in LDS:       */
                        /*   csr_tiling_kernel     src/kernels/csr_tiling.cu:24-114,*/
                        /*   wsp_sm_kernel         src/kernels/wsp_sm.cu:6-211     */
    SPMV_PANEL = 6,     /* (row block x column panel) sweep for columns without       */
                        /* locality: a wavefront keeps its block's sums in LDS and all */
                        /* resident waves walk the panels of x in step, so the panel   */
                        /* stays in L2.  The sparse-scale counterpart of the reference's*/
                        /* tiled format: TCSRMatrix src/tcsr.cpp:5-38 + csr_tiling_kernel*/
                        /* src/kernels/csr_tiling.cu:24-114.  Its plan COPIES the values */
                        /* (re-plan after changing them).                               */
    SPMV_AUTO = 7,      /* the library chooses at plan time: SPMV_TILED where its plan can stage the    */
                        /* chunks' x windows in LDS, SPMV_PANEL where it cannot (columns without        */
                        /* locality) and x is larger than one XCD's L2.  spmv_csr_plan_describe names   */
                        /* the choice.  Role: the reference's adaptive slot awsp_gemv_gpu               */
                        /* (src/kernels/awsp.cu:319-388), which the launcher of that name now runs.     */
    SPMV_XSKIP = 8,     /* activation sparsity on the CSR side: the plan re-orders the matrix into input-major */
                        /* segments per block of 1024 outputs; a run skips, whole, the segments of the inputs    */
                        /* whose x is zero (6 contiguous bytes per nonzero never read) and sums the rest in LDS. */
                        /*   the `x_i != 0` skip of asp_kernel_v* (src/kernels/asp.cu:20-26), awsp_kernel_v1     */
                        /*   (awsp.cu:127-134), awsp_ref_kernel (awsp_ref.cu:52).  For dense-ish matrices (the    */
                        /*   reference's regime): the plan refuses when ceil(rows/1024) x cols exceeds 2^27, and  */
                        /*   rows must be sorted and duplicate-free.  Its plan COPIES the values, like PANEL.  */
                        /* Its sum leaves out every term whose x is +-0, like the reference's asp skip: a    */
                        /* value of Inf or NaN against x == 0 adds nothing here (NaN everywhere else).       */
    SPMV_VARIANT_COUNT = 9
};

/* ---- runtime ---------------------------------------------------------- */
SPMV_API int spmv_device_count(void);            /* >= 0; 0 when no HIP device is usable */
SPMV_API const char *spmv_last_error(void);      /* thread-local, never NULL             */
SPMV_API const char *spmv_variant_name(int variant);
/* The event time of the FIRST launch of the last spmv_*_run_host call on this thread: cold, code-object load and first-touch
 * included -- the figure the reference's TIME_KERNEL prints (kernel.hpp:31-48 times one cold launch).  *kernel_ms of those
 * calls is the second, warm launch.  The launchers of include/kernel.hpp print both. */
SPMV_API float spmv_last_first_launch_ms(void);

/* ---- matrix handles ---------------------------------------------------
 * replaces: CSRMatrix (src/matrix_csr.cpp:5-23, src/include/matrix_csr.hpp:4-25)
 * and the cudaMalloc/cudaMemcpy block of every launcher (e.g. csr_naive.cu:36-52). */

/* Copy host CSR arrays to the current device (owned by the handle). */
SPMV_API int spmv_csr_create_host(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr,
                         const int32_t *col_idx, const float *vals, spmv_csr_t **out);

/* Borrow device arrays (caller keeps them alive; col_idx/vals 16-byte aligned). */
SPMV_API int spmv_csr_create_device(int64_t rows, int64_t cols, int64_t nnz, const int32_t *d_row_ptr,
                           const int32_t *d_col_idx, const float *d_vals, spmv_csr_t **out);

/* Dense row-major host A[M][N] -> CSR of A^T, built ON THE DEVICE with the
 * reference's semantics (keep iff value != 0.0f, columns ascending):
 * replaces the O(MN) host scan of matrix_csr.cpp:5-23.  rows = N, cols = M. */
SPMV_API int spmv_csr_from_dense_host(int M, int N, const float *A_host, void *stream, spmv_csr_t **out);

/* Same with A already resident on the device. */
SPMV_API int spmv_csr_from_dense_device(int M, int N, const float *d_A, void *stream, spmv_csr_t **out);

/* Copy the handle's CSR arrays back (row_ptr: rows+1 entries).  Any pointer may be NULL. */
SPMV_API int spmv_csr_download(const spmv_csr_t *h, int32_t *row_ptr, int32_t *col_idx, float *vals);

/* Check the arrays on the device: row_ptr[0] == 0, row_ptr non-decreasing, row_ptr[rows] == nnz, every column
 * index in [0, cols).  SPMV_ERR_INVALID + spmv_last_error() names the first offending row / element.  Both
 * spmv_csr_create_* call it (one pass over row_ptr and col_idx, synchronous): the kernels index x and their LDS
 * windows with these numbers unchecked, so a malformed matrix must never reach them.  The reference has no
 * counterpart (its CSR only ever comes from its own dense scan, matrix_csr.cpp:5-23). */
SPMV_API int spmv_csr_validate(const spmv_csr_t *h, void *stream);

SPMV_API int spmv_csr_dims(const spmv_csr_t *h, int64_t *rows, int64_t *cols, int64_t *nnz);

/* The smallest and the largest column index the matrix references (one device pass over col_idx, synchronous):
 * *col_min = cols, *col_max = -1 for a matrix without nonzeros.  A row block's x footprint -- what a sharded multiply has
 * to make available to the rank that holds it (include/spmv_dist.h: spmv_dist_pipe_set_footprint). */
SPMV_API int spmv_csr_column_range(const spmv_csr_t *h, int64_t *col_min, int64_t *col_max, void *stream);
SPMV_API int spmv_csr_destroy(spmv_csr_t *h);

/* ---- the transpose -------------------------------------------------------
 * The library multiplies by a handle's own orientation only; z = A^T u (the backward pass of a sparse layer, BiCG / LSQR,
 * pull versus push) goes through an explicit transpose: T = A^T is an ordinary spmv_csr_t, so every variant, SPMV_AUTO,
 * SpMM and the row-block exchange work on it as on any other handle, and the order of every sum stays a pure function of
 * the matrix (a scatter-add kernel with float atomics would give that up).  The reference has no counterpart: it only
 * multiplies one way.
 *
 * spmv_csr_transpose: T = A^T as a new handle on A's device, built on the device (no host pass over the nonzeros).
 * T has rows = a.cols, cols = a.rows, nnz = a.nnz and owns its three arrays (spmv_csr_destroy frees them); every
 * spmv_csr_* call accepts it; it has no plans yet.  `a` is only read and keeps its plans; it may own or borrow its arrays,
 * be a whole matrix or a row block.
 *   The order is part of the interface.  Row j of T lists the nonzeros of A whose column is j in ascending STORAGE POSITION
 * k of A.  With perm = argsort(a.col_idx, stable):
 *     t.row_ptr    = [0, cumsum(bincount(a.col_idx, minlength = a.cols))]
 *     t.col_idx[i] = the row of A that holds position perm[i]
 *     t.vals[i]    = a.vals[perm[i]]      (the bits are copied: NaN payloads, -0.0, subnormals)
 *     map[i]       = perm[i]              (kept with keep_map = 1: 4 bytes per nonzero)
 * So: the rows of T are always sorted (column indices non-decreasing), whatever the order inside A's rows; a column that
 * A repeats inside a row gives a repeated column inside a row of T, in A's storage order; an empty column of A is an empty
 * row of T; T is a pure function of A's arrays -- two calls, two handles of one matrix, any stream give the same bytes (no
 * place is taken from the value an atomic returns).  transpose(transpose(A)) is A with every row stably sorted by column:
 * A itself, bit for bit, when A's rows are sorted.
 *   Like spmv_csr_plan it allocates, enqueues on `stream` and waits for it before it returns.  SPMV_ERR_INVALID (the
 * message names the function, *out untouched) for a null `a` or `out`, keep_map other than 0 / 1, or another current device
 * than a's; SPMV_ERR_HIP when an allocation fails (what was allocated is released, `a` stays usable); SPMV_ERR_NO_DEVICE as
 * everywhere.  Every handle is admitted (rows, cols, nnz < 2^31): positions are unsigned 32-bit numbers, byte offsets 64-bit,
 * t.row_ptr may pass 4 GiB, t.col_idx holds row numbers up to 2^31 - 2; nnz = 0, rows = 0 and cols = 0 work.
 *   Device memory: T itself takes 8 nnz + 4 (a.cols + 1) bytes (+ 4 nnz for the map).  While the call runs it holds at
 * most 16 nnz + 1024 ceil(nnz / 4096) + 4 ceil(nnz / 65536) + 4 ceil((a.cols + 1) / 4096) + 64 bytes more (two position
 * and two key buffers of 4 nnz each -- one position buffer is the map, the others are freed on return --, the table of
 * 256 counters per tile of 4096 nonzeros, the tile sums of the two scans): 24.25 bytes per nonzero + 4 per column at the
 * peak, T included.
 *
 * spmv_csr_transpose_values: t.vals[i] = a.vals[map[i]] for a handle made with keep_map = 1 -- the values of A as they are
 * now, in one gather launch.  Asynchronous, allocates nothing, never waits: graph-capturable.  `a` must have t's shape
 * swapped and the same nnz and live on t's device (else SPMV_ERR_INVALID); that it still has the PATTERN t was made from
 * is the caller's promise, as for plans.  It reads a's values live (borrowed arrays the caller has rewritten are the point)
 * and then does for t what spmv_csr_values_changed(t) does: the plans of t that read vals live (SPMV_SCALAR ... SPMV_TILED,
 * SpMM) use the new values on their next run, the plans that hold a copy (SPMV_PANEL, SPMV_XSKIP, SPMV_AUTO where it
 * resolved to one of them) answer SPMV_ERR_STALE_PLAN until re-planned.  On a handle without a map (keep_map = 0, or not
 * made by spmv_csr_transpose): SPMV_ERR_INVALID, nothing launched.  `a` must not be t itself (t's values would be read while
 * they are written): SPMV_ERR_INVALID, nothing launched.
 *
 * spmv_csr_transpose_gather: dst[c * dst_stride + i] = src[c * src_stride + map[i]] for c < count, i < nnz, through the map of
 * a handle made with keep_map = 1: `count` arrays of nnz 32-bit words in the parent's storage order brought into t's, copied
 * as bits (a NaN keeps its payload, -0.0 its sign).  It is how the bias of the _bias attention calls below reaches
 * backward_kv.  One launch that reads the map once; src and dst need 4-byte alignment only and must not overlap; strides
 * count words.  Asynchronous, allocates nothing, never waits: graph-capturable.  It touches neither t's vals nor its plans.
 * SPMV_ERR_INVALID, nothing launched: a handle without a map; count < 1; a null array while nnz > 0; an array that is not
 * 4-byte aligned; a negative stride; dst_stride < nnz with count > 1.
 *
 * spmv_csr_transpose_map_bytes: device bytes of the kept map (4 * nnz; 0 without one or for a handle not made by
 * spmv_csr_transpose; < 0: null handle). */
SPMV_API int spmv_csr_transpose(const spmv_csr_t *a, int keep_map, void *stream, spmv_csr_t **out);
SPMV_API int spmv_csr_transpose_values(spmv_csr_t *t, const spmv_csr_t *a, void *stream);
SPMV_API int spmv_csr_transpose_gather(const spmv_csr_t *t, int count, const void *d_src, int64_t src_stride, void *d_dst,
                                       int64_t dst_stride, void *stream);
SPMV_API int64_t spmv_csr_transpose_map_bytes(const spmv_csr_t *t);

/* ---- selection -------------------------------------------------------------
 * A new pattern from an old one: per row the k best-scored nonzeros (spmv_csr_select_topk) or the nonzeros whose score is
 * at or above a threshold (spmv_csr_select_threshold), as a new handle on a's device.  It is the middle step of a dynamic
 * sparse attention (score a candidate pattern with spmv_csr_sddmm, keep the k best keys per query, attend on what is
 * left) and of magnitude pruning (keep the k largest |vals| per row).  Selection is pure structure -- integer keys, no
 * floating-point sum -- so the contract below holds bit for bit (tests/_select.py states it in numpy).
 *
 *   Scores.  d_score holds a.nnz floats in a's storage order; NULL means a's own vals, read live.
 *   Key.  The nonzero at storage position p gets a 32-bit unsigned key from s = score[p] (with SPMV_SELECT_ABS in flags:
 * from |s|, the sign bit cleared).  A NaN of either sign and any payload gets key 0.  Otherwise u = bits(s + 0.0f), so that
 * -0 and +0 are one key, and the key is ~u if the sign bit of u is set, else u | 0x80000000: the usual order-preserving map.
 * Every number, -Inf included, ranks above every NaN.
 *   Order.  Nonzero p ranks before nonzero q of the same row iff key(p) > key(q), or the keys are equal and p < q.
 *   spmv_csr_select_topk keeps, in every row, the first min(k, len) nonzeros of that ranking.
 *   spmv_csr_select_threshold keeps nonzero p iff s >= threshold (|s| >= threshold with SPMV_SELECT_ABS) as an IEEE
 * comparison: a NaN score is never kept, -0 >= +0 holds.
 *   The output handle.  *out has a's rows and cols, owns its three arrays (spmv_csr_destroy frees them), is accepted by
 * every spmv_csr_* call and has no plans yet.  A row lists its kept nonzeros in ASCENDING STORAGE POSITION of a: sorted rows
 * stay sorted, unsorted rows and repeated columns keep their relative order.  With map[m] the position in a of out's
 * nonzero m:
 *     out.col_idx[m] = a.col_idx[map[m]]
 *     out.vals[m]    = a.vals[map[m]]        (the bits are copied: NaN payloads, -0.0, subnormals)
 *     map            kept with keep_map = 1: 4 bytes per kept nonzero
 *   Purity.  The result is a pure function of a's arrays, the scores and k or the threshold: two calls, two handles of one
 * matrix, any stream and any neighbouring rows give the same bytes.  No place is taken from the value an atomic returns
 * (the only atomics are integer LDS counters whose result is not used: a count does not depend on the order of arrival).
 *   Copy case.  k >= the longest row, or threshold = -Inf on NaN-free scores, reproduces a's arrays bit for bit.
 *   Like spmv_csr_transpose each call allocates, enqueues on `stream` and waits for it before it returns (out.nnz is a
 * result).  `a` is only read and keeps its plans; it may own or borrow its arrays, be a whole matrix or a row block.
 *   SPMV_ERR_INVALID (the message names the function, *out untouched, nothing launched): a null `a` or `out`; k < 1; a NaN
 * threshold; a flag bit other than SPMV_SELECT_ABS; keep_map other than 0 / 1; a d_score that is not 4-byte aligned;
 * another current device than a's.  SPMV_ERR_HIP when an allocation fails (what was allocated is released, `a` stays
 * usable); SPMV_ERR_NO_DEVICE as everywhere.  Every handle is admitted (rows, cols, nnz < 2^31): positions are unsigned
 * 32-bit numbers, byte offsets 64-bit; nnz = 0, rows = 0 and a result without nonzeros work.
 *   Device memory: out itself takes 4 (rows + 1) + 8 kept bytes (+ 4 kept for the map), kept = out.nnz.  While the call
 * runs it holds at most 8 rows + 4 ceil(rows / 4096) + 64 bytes more (top-k: a cut of 8 bytes per row; the tile sums of the
 * scan of the row counts), freed on return: 12 rows + 12 kept bytes at the peak.  Nothing of a.nnz elements is allocated.
 *   The route (spmv-test_amd/csrc/kernels_select.hip): per row a cut (the k-th key tau and how many nonzeros with key ==
 * tau are admitted, by storage position) -- rows of at most 512 nonzeros in registers by bisection over the key bits, longer
 * rows by an 8-bit radix select of four passes --, a scan of the row counts, and a compaction that re-reads the scores.
 *
 * spmv_csr_select_values: s.vals[m] = a.vals[map[m]] for a handle made with keep_map = 1, then what
 * spmv_csr_values_changed(s) does (see spmv_csr_transpose_values).  `a` must have s's shape, the nnz of s's parent (the
 * handle records it) and live on s's device; that it still has the parent's PATTERN is the caller's promise.  `a` must not
 * be s itself (s's values would be read while they are written): SPMV_ERR_INVALID, nothing launched.
 *
 * spmv_csr_select_gather:  dst[c * dst_stride + m] = src[c * src_stride + map[m]]
 * spmv_csr_select_scatter: dst[c * dst_stride + map[m]] = src[c * src_stride + m]; every other word of dst is left
 * untouched (zero-fill first for a dense gradient; map entries are distinct, so nothing races)
 * for c < count, m < s.nnz, on 32-bit words copied as bits; strides count words; src and dst need 4-byte alignment only and
 * must not overlap.  The arrays in the parent's order hold the parent's nnz words, those in s's order s.nnz.
 * SPMV_ERR_INVALID, nothing launched: a handle without a select map; count < 1; a null array while s.nnz > 0; an array that
 * is not 4-byte aligned; a negative stride; dst_stride below the words of one array of dst with count > 1.
 *
 * _values, _gather, _scatter and spmv_csr_copy_arrays are asynchronous, allocate nothing, never wait: graph-capturable.
 *
 * One map per handle: a handle made by spmv_csr_transpose is refused by the _select_* companions, a handle made by a select
 * call by the _transpose_* companions, and spmv_csr_transpose_map_bytes is 0 for a selected handle.
 * spmv_csr_select_map_bytes: device bytes of the kept map (4 * nnz; 0 without one; < 0: null handle).
 *
 * spmv_csr_copy_arrays: device-to-device copies of a handle's arrays (rows + 1, nnz, nnz elements) into the caller's
 * buffers on the handle's device, enqueued on `stream`; any pointer may be NULL.  This is how an owned pattern reaches
 * arrays that another handle borrows (spmv_csr_download goes to the host only).  SPMV_ERR_INVALID: a null handle, another
 * current device than the handle's. */
enum { SPMV_SELECT_ABS = 1 };   /* rank by |score| (sign bit cleared) */
SPMV_API int spmv_csr_select_topk(const spmv_csr_t *a, const float *d_score, int k, int flags, int keep_map, void *stream,
                                  spmv_csr_t **out);
SPMV_API int spmv_csr_select_threshold(const spmv_csr_t *a, const float *d_score, float threshold, int flags, int keep_map,
                                       void *stream, spmv_csr_t **out);
SPMV_API int spmv_csr_select_values(spmv_csr_t *s, const spmv_csr_t *a, void *stream);
SPMV_API int spmv_csr_select_gather(const spmv_csr_t *s, int count, const void *d_src, int64_t src_stride, void *d_dst,
                                    int64_t dst_stride, void *stream);
SPMV_API int spmv_csr_select_scatter(const spmv_csr_t *s, int count, const void *d_src, int64_t src_stride, void *d_dst,
                                     int64_t dst_stride, void *stream);
SPMV_API int64_t spmv_csr_select_map_bytes(const spmv_csr_t *s);
SPMV_API int spmv_csr_copy_arrays(const spmv_csr_t *h, int32_t *d_row_ptr, int32_t *d_col_idx, float *d_vals, void *stream);

/* ---- the sparse product ------------------------------------------------------
 * A pattern from two patterns: C = A B for two CSR handles (SpGEMM), as a new handle on their device.  It is how A A^T
 * becomes a candidate pattern for a top-k selection, how two hops of a graph or R A P are formed, and how two sparse layers
 * without an activation between them fold into one.  The contract below holds bit for bit (tests/_spgemm.py states it in
 * numpy).
 *
 *   Shapes.  a is m x n, b is n x p, both on one device; *out is m x p, owns its three arrays (spmv_csr_destroy frees
 * them), is accepted by every spmv_csr_* call and has no plans of a variant yet.  a and b are only read and keep their
 * plans; either may own or borrow its arrays and be a whole matrix or a row block; a == b is allowed.
 *   Pattern.  Row i of C lists every column j that occurs in a row b[col] for some col among the entries of a's row i, each
 * once, in ascending order: the rows of C are sorted and duplicate-free whatever the rows of a and b are.  The pattern is
 * structural: an entry stays when its value is 0, -0 or a NaN and when its terms cancel; stored zeros of a and b count as
 * nonzeros.
 *   Values.  Every term counts, and a repeated column adds each of its terms.  For the entry (i, j): walk a's row i in
 * ascending storage position s, inside each s walk b's row a.col_idx[s] in ascending storage position q, and for every q
 * with b.col_idx[q] == j do acc = fma(a.vals[s], b.vals[q], acc), starting from +0 -- the chain of spmv_csr_spmm restricted
 * to the terms that exist.  IEEE rules, subnormals kept; a NaN result is a NaN of the hardware's sign and payload.  The
 * order holds for every row, however long it is and however the kernels divide the work.
 *   Purity.  C is a pure function of the six input arrays: two calls, two handles, any stream and any neighbouring rows
 * give the same bytes, and the rows of spgemm(row block of a, b) are the corresponding rows of spgemm(a, b).  No place and
 * no sum depends on the order in which anything arrives: a row's columns come out of a sort, the only atomic is an integer
 * LDS add whose result is not used, and there is no float atomic.
 *   *products (may be NULL) = the sum over all entries s of a of the length of b's row a.col_idx[s]: the number of terms,
 * a 64-bit number.  It is set once the bounds are known, also when the call is refused afterwards for its result's size.
 *   Like spmv_csr_transpose the call allocates, enqueues on `stream` and waits for it before it returns (out.nnz is a
 * result); it also reads one 64-bit bound per row of a back to the host, where the rows are sorted into classes.
 *   SPMV_ERR_INVALID (the message names the function, *out untouched, nothing left allocated): a null a, b or out;
 * a.cols != b.rows; a and b on different devices, or another current device than theirs; keep_plan other than 0 / 1; a
 * result of 2^31 or more nonzeros (refused after the count; the message carries the count); a single row of a with more
 * than 2^30 terms.  SPMV_ERR_HIP when an allocation fails (what was allocated is released, a and b stay usable);
 * SPMV_ERR_NO_DEVICE as everywhere.  m = 0, n = 0, p = 0, nnz = 0 on either side and a result without nonzeros work.
 *   Classes.  A row of a with t terms is taken by the smallest class of SPMV_SPGEMM_CLASS_SLOTS that holds t words (a
 * wavefront sorts the t columns in that much LDS); a row beyond the last class is OVERSIZED: a workgroup sorts its columns
 * in a scratch of global memory (slow: DESIGN.md section 26).  The result does not depend on the class.
 *   Device memory.  C itself takes 4 (m + 1) + 8 nnz(C) bytes.  With L = the rows of a that have at least one term,
 * V = the oversized rows among them and S = the sum over the oversized rows of (their terms rounded up to a power of two),
 * the call holds at most max(8 m, 8 nnz(C)) + 4 L + 8 (V + 1) + 4 S + 4 ceil(m / 4096) + 80 bytes beside 4 (m + 1) of C at the
 * peak (the bounds, freed before col_idx and vals are allocated; the row lists; the scratch offsets and the scratch; the
 * totals and the tile sums of the scan).  Kept with keep_plan = 1: the row lists, 4 L bytes -- what
 * spmv_csr_spgemm_plan_bytes returns (0 without a plan; < 0: null handle).
 *
 * spmv_csr_spgemm_values: for a c made with keep_plan = 1, c.vals recomputed from the values a and b hold now, under the
 * same contract (the numeric pass of the first call: at most four launches).  Asynchronous, allocates nothing, never waits:
 * graph-capturable.  Afterwards it does for c what spmv_csr_values_changed(c) does (see spmv_csr_transpose_values).  a must
 * be c.rows x n and b n x c.cols with the nnz of c's parents (the handle records n and both) on c's device, else
 * SPMV_ERR_INVALID; that their PATTERNS are unchanged is the caller's promise.  On a handle without a plan (keep_plan = 0,
 * or not made by spmv_csr_spgemm): SPMV_ERR_INVALID, nothing launched.  Neither a nor b may be c itself (c's values would be
 * read while they are written): SPMV_ERR_INVALID, nothing launched; a == b stays allowed.  A product handle carries no
 * transpose or select map: those companions refuse it. */
#define SPMV_SPGEMM_CLASS_SLOTS 64, 512, 4096, 32768   /* words of LDS per row of each class, ascending */
SPMV_API int spmv_csr_spgemm(const spmv_csr_t *a, const spmv_csr_t *b, int keep_plan, void *stream, spmv_csr_t **out,
                             int64_t *products /* may be NULL */);
SPMV_API int spmv_csr_spgemm_values(spmv_csr_t *c, const spmv_csr_t *a, const spmv_csr_t *b, void *stream);
SPMV_API int64_t spmv_csr_spgemm_plan_bytes(const spmv_csr_t *c);

/* ---- the sparse sum ----------------------------------------------------------
 * A pattern from two patterns of one shape: C = alpha A + beta B on the union, the intersection or the difference of the two
 * patterns, as a new handle on their device.  It is how an attention pattern is put together (a band UNION a top-k selection
 * UNION a few global columns), how a candidate pattern is masked (INTERSECT) or already-attended keys are removed (MINUS), how a
 * pruned layer grows again (the old pattern UNION new positions, which start at +0), and how A + A^T or A - sigma I are formed.
 * The contract below holds bit for bit (tests/_add.py states it in numpy).
 *
 *   Shapes.  a and b are both m x n on one device; *out is m x n, owns its three arrays (spmv_csr_destroy frees them), is
 * accepted by every spmv_csr_* call and has no plans of a variant yet.  a and b are only read and keep their plans; either may
 * own or borrow its arrays and be a whole matrix or a row block; a == b is allowed.
 *   Pattern.  Row i of C lists each of these columns once, in ascending order -- SPMV_ADD_UNION: a column that occurs in row
 * i of a or of b; SPMV_ADD_INTERSECT: a column that occurs in both; SPMV_ADD_MINUS: a column that occurs in a and not in b.
 * The rows of C are sorted and duplicate-free whatever the rows of a and b are (unsorted, repeated columns).  The pattern is
 * structural: stored zeros of a and b count, and an entry stays when its value is 0, -0 or a NaN and when its terms cancel.
 *   Values.  The terms of entry (i, j) come in this order: the storage positions s of a's row i with a.col_idx[s] == j,
 * ascending, then the positions q of b's row i with b.col_idx[q] == j, ascending.  A term has the coefficient of its side
 * (alpha for a, beta for b).  The first term gives acc = fl(coef * v), every later one acc = fma(coef, v, acc).  A side whose
 * coefficient is +0 or -0 contributes to the pattern and has NO terms (its values, NaN and Inf included, are not read into
 * the sum); an entry without terms is +0.  Under SPMV_ADD_MINUS only a has terms and beta is ignored.  A NaN or infinite
 * coefficient follows IEEE rules; subnormals are kept; a NaN result is a NaN of the hardware's sign and payload.
 *   So: add(A, empty, 1, x, UNION) is A with every row stably sorted by column (A itself bit for bit when its rows are sorted
 * and duplicate-free); add(A, M, 1, 0, INTERSECT) restricts A to M's pattern whatever M's values are; add(A, G, 1, 0, UNION) is
 * A widened by G's positions at +0.
 *   Purity.  C is a pure function of the six input arrays, the coefficients and op: two calls, two handles, any stream and any
 * neighbouring rows give the same bytes, and the rows of add(row block of a, the same block of b) are the corresponding rows
 * of add(a, b).  There is no atomic in the route, so no place and no sum depends on the order in which anything arrives.
 *   Like spmv_csr_transpose the call allocates, enqueues on `stream` and waits for it before it returns (out.nnz is a
 * result).  There are no row classes: every row, however long, takes the same launches.
 *   SPMV_ERR_INVALID (the message names the function, *out untouched, nothing left allocated): a null a, b or out; shapes
 * that differ (the message gives both); a and b on different devices, or another current device than theirs; op outside the
 * enum; keep_plan other than 0 / 1; a result of 2^31 or more entries (refused after the count and before anything of that
 * size is allocated; the message carries the count).  SPMV_ERR_HIP when an allocation fails (what was allocated is released,
 * a and b stay usable); SPMV_ERR_NO_DEVICE as everywhere.  m = 0, n = 0, nnz = 0 on either side and an empty result work.
 *   Plan.  The call builds the kept terms in C's order: per kept term a 32-bit word (the side in the top bit, the storage
 * position in that side below it) and per entry of C where its terms start.  The kept terms T are the nonzeros of a whose
 * column is an entry of C and, under UNION and INTERSECT, those of b -- whatever the coefficients are.  With keep_plan = 1
 * the handle keeps both arrays: 4 T + 4 (nnz(C) + 1) bytes, what spmv_csr_add_plan_bytes returns (0 without a plan; < 0: null
 * handle).
 *   Device memory.  C itself takes 4 (m + 1) + 8 nnz(C) bytes.  Sorted operands (every row non-decreasing): the call holds at
 * most 4 (nnz(a) + 1) + 4 (nnz(b) + 1) [b's under UNION only] + 4 (nnz(C) + 1) + 4 T + 4 ceil(max(nnz(a), nnz(b), nnz(C), m) /
 * 4096) + 16 bytes more (the ranks of the kept heads, freed before the terms are allocated; the plan's two arrays, freed on
 * return without keep_plan; the tile sums of a scan).  An operand x with an unsorted row is replaced by its stably
 * row-sorted view, transpose(transpose(x)) with both maps composed: 12 nnz(x) + 4 (m + 1) bytes more for the whole call, and
 * while the view is built the transpose's peak above (24.25 nnz(x) + 4 n, beside 12 nnz(x) + 4 (n + 1) of the first
 * transpose).
 *
 * spmv_csr_add_values: for a c made with keep_plan = 1, c.vals recomputed under the contract above from the values a and b
 * hold now, with the coefficients given now (one that is +0 or -0 now drops that side's terms, as in the first call): the value
 * kernel of the first call, a lane per entry of C that walks its run.  One launch; asynchronous, allocates nothing, never
 * waits: graph-capturable.  Afterwards it does for c what spmv_csr_values_changed(c) does (see spmv_csr_transpose_values).  a
 * and b must have c's shape and the nnz of c's parents (the handle records both) on c's device, else SPMV_ERR_INVALID; that
 * their PATTERNS are unchanged is the caller's promise.  On a handle without a plan: SPMV_ERR_INVALID, nothing launched.
 * Neither a nor b may be c itself (c's values would be read while they are written): SPMV_ERR_INVALID, nothing launched; a == b
 * stays allowed.
 *
 * spmv_csr_add_gather: dst[k * dst_stride + p] = src[k * src_stride + e] for every kept term at storage position p of the
 * chosen side (0: a, 1: b) whose entry of C is e, for k < count: 32-bit words copied as bits; every other word of dst is left
 * untouched (the targets are distinct, so nothing races).  It is how a gradient on C's pattern reaches the operands (dA =
 * alpha * gathered) and how state kept in C's order is read back.  The arrays in C's order hold c.nnz words, those in the
 * side's order that side's nnz; strides count words; src and dst need 4-byte alignment only and must not overlap.
 * Asynchronous, allocates nothing, never waits: graph-capturable.  SPMV_ERR_INVALID, nothing launched: a handle without a
 * plan; side other than 0 / 1; count < 1; a null array while c.nnz > 0; an array that is not 4-byte aligned; a negative
 * stride; dst_stride below the words of one array of dst with count > 1.
 *
 * One map per handle: a sum handle carries no transpose map, select map or product plan, so those companions refuse it, and
 * the companions here refuse a handle made by another call. */
enum { SPMV_ADD_UNION = 0, SPMV_ADD_INTERSECT = 1, SPMV_ADD_MINUS = 2 };
SPMV_API int spmv_csr_add(const spmv_csr_t *a, const spmv_csr_t *b, float alpha, float beta, int op, int keep_plan, void *stream,
                          spmv_csr_t **out);
SPMV_API int spmv_csr_add_values(spmv_csr_t *c, const spmv_csr_t *a, const spmv_csr_t *b, float alpha, float beta, void *stream);
SPMV_API int spmv_csr_add_gather(const spmv_csr_t *c, int side /* 0: a, 1: b */, int count, const void *d_src, int64_t src_stride,
                                 void *d_dst, int64_t dst_stride, void *stream);
SPMV_API int64_t spmv_csr_add_plan_bytes(const spmv_csr_t *c);

/* ---- the triangular solve -----------------------------------------------------
 * x = T^-1 b for the lower or the upper triangle T of a square handle, level by level: what a Gauss-Seidel or SSOR sweep and
 * the application of an ILU / IC factor repeat.  spmv_csr_trsv_plan analyses the pattern once (on the device); spmv_csr_trsv
 * enqueues one solve.  The contract below holds bit for bit (tests/_trsv.py states it in numpy).
 *
 *   Shapes.  h is square (rows == cols) and may own or borrow its arrays; rows may be unsorted and may repeat columns.  h may
 * be a full matrix: SPMV_TRSV_LOWER reads only the entries with col <= row, SPMV_TRSV_UPPER only those with col >= row; the
 * values of the other triangle, whatever they are, are never read into a result (the fill-mode convention of the vendor
 * libraries).  So Gauss-Seidel runs on A's own handle.
 *   Terms.  The terms of row i are its storage positions s, ascending, with col_idx[s] < i (UPPER: > i).  A column that
 * repeats gives several terms.
 *   Diagonal.  SPMV_TRSV_NON_UNIT needs exactly one storage position with col_idx[s] == i in every row; the plan records the
 * first row with none or several, and a NON_UNIT solve on such a plan is refused (the message names the row; nothing is
 * launched).  Under SPMV_TRSV_UNIT diagonal entries are ignored: a stored NaN there changes nothing.  A diagonal whose VALUE
 * is 0 is no error: the result follows IEEE rules.
 *   Values.  For the n terms t_0 .. t_(n-1) of a row (value v_t, column c_t): n <= SPMV_TRSV_SERIAL_MAX: s = +0, then
 * s = fma(v_t, x[c_t], s) in term order.  Larger n: 64 chains, chain l over the terms l, l + 64, ... by the same fma from
 * +0; then p[l] += p[l + w] for l < w, for w = 32, 16, 8, 4, 2, 1, and s = p[0].  Then x_i = fl(fl(b_i - s) / d_i), under
 * UNIT x_i = fl(b_i - s); the division is the correctly rounded one.  NaN, Inf, -0 and subnormals follow IEEE rules.
 *   Purity.  x is a pure function of the three arrays, b, uplo and diag: it does not depend on thin_rows, on how levels were
 * merged into launches, on the stream or on a second handle of the same arrays.  Values are read live at every solve and the
 * plan is a function of the pattern alone: a borrowed vals rewritten between two solves needs no new plan.  No atomic, no
 * flag, no grid barrier and no cooperative launch is on the solve path: the only waits are kernel boundaries and the
 * workgroup barrier, and every loop bound comes from the plan.
 *   Aliasing.  d_x == d_b is allowed (in place); any other overlap is the caller's error.
 *   The plan.  level[i] = 0 for a row without terms, else 1 + the largest level among its terms' columns.  `order` lists the
 * rows by (level, row) ascending and `level_ptr` where each level starts (spmv_csr_trsv_plan_rows returns exactly these,
 * level_ptr[levels + 1] and order[rows], to host arrays).  A level of more than thin_rows rows is one grid launch; a maximal
 * run of consecutive levels of at most thin_rows rows each is one launch of ONE workgroup, which walks the run with a
 * workgroup barrier between levels; a run is cut every SPMV_TRSV_LEVEL_CAP levels.  thin_rows = 0 takes
 * SPMV_TRSV_THIN_DEFAULT.  A handle keeps one plan per uplo; planning again replaces it.  The call allocates, enqueues on
 * `stream` and waits for it.
 *   Device memory.  The plan keeps 4 rows (order) + 4 rows (the diagonal's position) + 4 (levels + 1) (level_ptr) + 4 (rows
 * + 1) + 4 L bytes (where the L terms of the rows of more than SPMV_TRSV_SERIAL_MAX terms are, listed by storage position):
 * what spmv_csr_trsv_plan_bytes returns (0 without a plan; < 0: null handle).  While the plan is built the call also holds
 * the transpose of the pattern (12 nnz + 4 (rows + 1) bytes, and while that is made the transpose's own peak) beside 16 rows
 * + 32 bytes of term counters, levels and two frontiers; then, that transpose, the counters and the frontiers freed, the rows
 * x levels pattern of one entry per row and its transpose (the levels kept, 8 rows + 4 more for the pattern, 4 rows for the
 * transpose's values beside order and level_ptr, and the transpose's peak at nnz = rows).
 *   The solve enqueues its launches (info[1] of them, one after the other on `stream`), allocates nothing and never waits:
 * graph-capturable, and the captured graph has no parallel branches.
 *   spmv_csr_trsv_plan_info: info[0] levels, [1] launches of one solve, [2] rows of the widest level, [3] rows of more than
 * SPMV_TRSV_SERIAL_MAX terms, [4] the first row whose diagonal is missing or repeated (-1: none), [5] the thin threshold in
 * force, [6] the cap of levels per merged launch, [7] 0.  spmv_csr_trsv_describe: the same as a line of text.
 *   SPMV_ERR_INVALID (the message names the function; nothing launched or left allocated): a null handle, or a null array
 * while rows > 0; a handle that is not square; uplo or diag outside the enums; a negative thin_rows; a solve, plan_info,
 * plan_rows or describe without a plan for that uplo; another current device than the handle's; a pattern whose levels do
 * not close (arrays that are no valid CSR).  rows = 0 and nnz = 0 work: with nnz = 0 and rows > 0, UNIT gives x = b and
 * NON_UNIT is the diagonal refusal. */
enum { SPMV_TRSV_LOWER = 0, SPMV_TRSV_UPPER = 1 };
enum { SPMV_TRSV_NON_UNIT = 0, SPMV_TRSV_UNIT = 1 };
#define SPMV_TRSV_SERIAL_MAX 32     /* terms of a row summed as one chain; see Values */
#define SPMV_TRSV_THIN_DEFAULT 256  /* thin_rows = 0: levels of at most this many rows are merged into one-workgroup launches */
#define SPMV_TRSV_LEVEL_CAP 1024    /* levels of one merged launch at the most */
SPMV_API int spmv_csr_trsv_plan(spmv_csr_t *h, int uplo, int thin_rows /* 0: default */, void *stream);
SPMV_API int spmv_csr_trsv(spmv_csr_t *h, int uplo, int diag, const float *d_b, float *d_x, void *stream);
SPMV_API int64_t spmv_csr_trsv_plan_bytes(const spmv_csr_t *h, int uplo);
SPMV_API int spmv_csr_trsv_plan_info(const spmv_csr_t *h, int uplo, int64_t info[8]);
SPMV_API int spmv_csr_trsv_plan_rows(const spmv_csr_t *h, int uplo, int32_t *level_ptr /* levels + 1, host */,
                                     int32_t *order /* rows, host */);
SPMV_API int spmv_csr_trsv_describe(const spmv_csr_t *h, int uplo, char *buf, int n);

/* ---- the incomplete factorisation ---------------------------------------------
 * M = ILU(0) of a square handle: the factor the triangular solve applies, made on the device.  M has a's pattern; L (unit
 * lower, its ones not stored) and U (upper, the diagonal included) live in ONE handle, so spmv_csr_trsv LOWER / UNIT followed
 * by UPPER / NON_UNIT on it applies (L U)^-1: that is spmv_csr_ilu0_solve.  The contract below holds bit for bit
 * (tests/_ilu0.py states it in numpy).
 *
 *   Shapes.  a is square and owns or borrows its arrays.  Every row of a is strictly ascending (sorted, no repeated column)
 * and stores its diagonal entry; otherwise SPMV_ERR_INVALID, and the message names the first offending row and which of the
 * two rules it breaks (spmv_csr_add(A, empty, 1, 0, SPMV_ADD_UNION) sorts a matrix, spmv_csr_add(A, I, 1, 0, SPMV_ADD_UNION)
 * gives it a diagonal).  *out owns copies of row_ptr and col_idx and its own vals; every spmv_csr_* call accepts it.  It
 * carries both trsv plans, lower and upper, made with thin_rows (0: SPMV_TRSV_THIN_DEFAULT), and records a's rows and nnz.
 * The call allocates, enqueues on `stream` and waits for it.  rows = 0 works.
 *   Values.  Rows are taken in ascending i.  w starts as a copy of a's row i.  For each storage position p of row i with
 * column k < i, ascending: (1) w[p] = fl(w[p] / M[diag_k]), the correctly rounded division, l = w[p]; (2) for each position q
 * of row k of M with column j > k, ascending: if j is stored in row i at position r, w[r] = fma(-l, M[q], w[r]).  Row i of M
 * is then w.  Equivalently entry (i, j) is a_ij with the terms k < min(i, j) that have (i, k) and (k, j) both stored, applied
 * in ascending k, then divided by u_jj if j < i: which lane did the work cannot matter.  A pivot of value 0 is no error; NaN,
 * Inf, -0 and subnormals follow IEEE rules.
 *   Purity.  M's vals are a pure function of a's three arrays: they do not depend on thin_rows, on how levels were merged
 * into launches, on whether a lane or a wavefront took a row (rows that store more than SPMV_ILU0_SERIAL_MAX entries take a
 * wavefront), on the stream or on a second handle.  No atomic touches a value; no flag, no spin, no grid barrier and no
 * cooperative launch is on the path: the only waits are kernel boundaries and the workgroup barrier, and every loop bound
 * comes from row_ptr or the plan.
 *   spmv_csr_ilu0_values(m, a) factors again from the values a holds now: asynchronous, allocates nothing, never waits,
 * graph-capturable (no parallel branches).  a must have the recorded rows and nnz; an unchanged pattern is the caller's
 * promise; a == m is refused.  A row's own lanes copy a's row into m first, so there is no copy launch: the launches are the
 * steps of the lower plan (spmv_csr_trsv_plan_info info[1]) plus one that resets the pivot word.  Afterwards it does what
 * spmv_csr_values_changed(m) does.
 *   spmv_csr_ilu0_solve(m, r, z): z = U^-1 (L^-1 r), the two solves above on `stream`, the second in place; no kernel of its
 * own, allocates nothing, graph-capturable; d_z == d_r is allowed.
 *   spmv_csr_ilu0_pivot: the smallest row whose pivot u_ii is +-0 or not finite after the last factorisation, -1: none.  The
 * factor kernel takes an integer minimum on one device word (independent of arrival order; it reaches no value); this call
 * copies the word on `stream` and waits.
 *   One map per handle, as elsewhere: a factor handle has no transpose or select map and no spgemm or add plan, so those
 * companions (_values, _gather, _scatter) refuse it, and _ilu0_values, _solve and _pivot refuse every handle that
 * spmv_csr_ilu0 did not make.
 *   Device memory.  M itself: 4 (rows + 1) + 8 nnz bytes.  Beyond its three arrays the handle keeps the two trsv plans
 * (spmv_csr_trsv_plan_bytes of each uplo) and the 4 bytes of the pivot word: what spmv_csr_ilu0_plan_bytes returns (0 for a
 * handle that is no factor handle; < 0: null handle).  While spmv_csr_ilu0 runs it also holds 8 bytes of the check's two
 * minima and the build peak of one trsv plan at a time (see the triangular solve), the lower one first.  _values, _solve and
 * _pivot allocate nothing.
 *   SPMV_ERR_INVALID (the message names the function; *out untouched, nothing left allocated): a null argument, or a null
 * array while rows > 0; a handle that is not square; a negative thin_rows; a row that is not strictly ascending or stores no
 * diagonal; another current device than the handle's; for _values also a == m, or an a of other rows or nnz than recorded. */
#define SPMV_ILU0_SERIAL_MAX 32   /* stored entries of a row factored by one lane; longer rows take a wavefront */
SPMV_API int spmv_csr_ilu0(const spmv_csr_t *a, int thin_rows /* 0: default */, void *stream, spmv_csr_t **out);
SPMV_API int spmv_csr_ilu0_values(spmv_csr_t *m, const spmv_csr_t *a, void *stream);
SPMV_API int spmv_csr_ilu0_solve(spmv_csr_t *m, const float *d_r, float *d_z, void *stream);      /* z = U^-1 (L^-1 r) */
SPMV_API int spmv_csr_ilu0_pivot(const spmv_csr_t *m, void *stream, int64_t *row);                /* waits; -1: none */
SPMV_API int64_t spmv_csr_ilu0_plan_bytes(const spmv_csr_t *m);

/* ---- the multicolour ordering -----------------------------------------------
 * A colouring of a square handle's graph, the relabelled handle B = P A Q^T, and what moves values and vectors between the
 * two orders.  With the rows of one colour contiguous and no stored entry between two rows of a colour, the lower and the
 * upper dependency graph of P A P^T are at most as deep as there are colours: spmv_csr_trsv_plan finds those few levels by
 * itself and spmv_csr_ilu0 reuses them.  Everything here is structure -- integer keys, no floating-point sum -- so the
 * contract holds bit for bit (tests/_color.py states it in numpy).
 *
 * spmv_csr_color.  a is square and owns or borrows its arrays; rows may be unsorted and may repeat columns; vals are never
 * read.  The graph is the symmetrised pattern, N(i) = { j != i : (i, j) stored or (j, i) stored }, so a pattern that is not
 * structurally symmetric is coloured correctly (the other direction comes from the library's transpose, freed before the call
 * returns).  key(i) = fmix32((uint32_t)i ^ seed), compared unsigned, with fmix32(h): h ^= h >> 16; h *= 0x85ebca6b;
 * h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16 in 32-bit arithmetic -- a bijection, so keys never tie.  color[i] is the
 * smallest c >= 0 that is not in { color[j] : j in N(i), key(j) > key(i) }: the sequential greedy colouring in descending key
 * order (Jones-Plassmann), at most the maximum degree + 1 colours.  d_perm lists the rows by (colour, row) ascending and
 * color_ptr[c] is where colour c starts in it (the transpose of the rows x colours pattern with one entry per row: the
 * library's stable sort, no atomic).  color_ptr is a HOST array of `cap` entries: min(colours + 1, cap) of them are filled.
 *   info[0] colours; [1] rounds = max_i round(i), round(i) = 1 + max(round(j) : j in N(i), key(j) > key(i)) and 1 where there
 * is no such j; [2] launches of the colouring loop; [3] / [4] the rows of the largest / smallest colour; [5] neighbour
 * entries a full sweep visits (the stored entries of a and of its transpose); [6] device bytes the call held at its peak;
 * [7] 0.  [0], [1], [3] and [4] belong to the contract.  rows = 0: no colour, no round.  nnz = 0: one colour, one round, the
 * identity.
 *   Purity.  color, perm, color_ptr and info[0], [1], [3], [4] are a pure function of row_ptr, col_idx and seed: they do not
 * depend on timing, on the stream, on whether a lane or a wavefront took a row (rows of more than SPMV_COLOR_SERIAL_MAX
 * neighbour entries, a's and its transpose's counted together, take a wavefront) or on how rounds were merged into launches.
 * A row reads a neighbour's colour only when an EARLIER round wrote it (every colour carries the number of its round; a
 * merged launch of one workgroup separates its rounds by the workgroup barrier).  The only atomic decides a row's place in
 * the list of the rows still uncoloured, whose order reaches no output.  No flag, no spin, no grid barrier and no cooperative
 * launch: the only waits are kernel boundaries and the workgroup barrier; every loop bound is an argument or comes from a
 * row_ptr; the host loop makes at most `rows` trips with one read each and fails if a trip colours nothing.
 *   Device memory.  Nothing is kept.  At the peak (info[6]): the transpose of a (4 (rows + 1) + 8 nnz) with its temporaries
 * while it is made (see the transpose), then beside it 4 bytes per row of round numbers, two lists of 4 bytes per row and 32
 * bytes of state; then, the transpose freed, the rows x colours pattern and its transpose (24 bytes per row and their
 * temporaries).
 *   SPMV_ERR_INVALID, nothing launched, outputs untouched: a null handle or a null d_color; a handle that is not square;
 * cap < 0; color_ptr non-NULL with cap == 0; another current device than the handle's.
 *
 * spmv_csr_permute.  B = P A Q^T as a new handle that owns its arrays.  Both permutations use one convention: new index r
 * holds old index perm[r] (NULL: the identity).  Row r of B is row d_row_perm[r] of a; an entry in column j of a lands in the
 * column c with d_col_perm[c] = j.  Inside a row of B the entries ascend by (new column, storage position in a): rows are
 * always sorted, repeated columns stay repeated in a's order, values are copied as bits.  With SPMV_PERMUTE_KEEP_MAP the
 * handle keeps map[i], a's storage position of B's entry i (4 bytes per nonzero).  d_row_perm = d_col_perm = perm of
 * spmv_csr_color gives P A P^T; where a's rows are strictly ascending with a stored diagonal spmv_csr_ilu0 accepts it.  a may
 * be rectangular, owning or borrowing, and keeps its plans.  The call allocates, enqueues on `stream` and waits for it.
 *   Both arrays are checked on the device to be permutations (a mark per index); the first index whose entry is out of range
 * or was taken by an earlier index is an integer minimum: SPMV_ERR_INVALID, the message names the array and the index, *out
 * untouched, nothing left allocated.
 *   Two routes, the same bytes.  Direct: the row lengths gathered and scanned into row_ptr; a row of at most 64 entries is
 * ranked inside a wavefront (a lane per entry, the others' columns through the cross-lane shuffle), a row of at most 4096
 * entries is a bitonic sort of the 64-bit keys (column << 32 | position) of one workgroup in LDS.  Via the transpose
 * (SPMV_PERMUTE_VIA_TRANSPOSE, and every call with a longer row): the columns relabelled, the library's transpose, its columns
 * (a's rows) relabelled by the inverse row permutation, the transpose again, the two maps composed: linear in nnz for any
 * row length.
 *   spmv_csr_permute_values(b, a): b.vals[i] = a.vals[map[i]], then what spmv_csr_values_changed(b) does.
 * spmv_csr_permute_gather: dst[c * dst_stride + i] = src[c * src_stride + map[i]] for c < count, arrays of nnz 32-bit words
 * from a's order into b's.  Each is one launch, asynchronous, allocates nothing, never waits: graph-capturable.  They refuse
 * what spmv_csr_transpose_values / _gather refuse: a handle without a map; a == b; an a of another shape or nnz or device;
 * count < 1; a null array while nnz > 0; an array that is not 4-byte aligned; a negative or overflowing stride; dst_stride <
 * nnz with count > 1.  One map per handle, as elsewhere: B has no transpose or select map, so those companions refuse it, and
 * these two refuse every handle spmv_csr_permute did not make.  spmv_csr_permute_map_bytes: 4 nnz with a map, else 0 (< 0:
 * null handle).
 *   Device memory.  B: 4 (rows + 1) + 8 nnz bytes, and 4 nnz of the map when kept.  While the call runs also 4 bytes per row
 * and per column for the inverse permutations and 16 bytes of state; the direct route adds 4 bytes per row (the list of the
 * rows of more than 64 entries), the route via the transpose the relabelled columns (4 nnz), one intermediate transpose with
 * its map (4 (cols + 1) + 12 nnz) and the temporaries of one transpose at a time.
 *   SPMV_ERR_INVALID: a null handle or a null out; flags outside the two; an array that is no permutation; nnz of 2^31 or more
 * or a dimension of 0x7f7f7f7f or more (the marks are 32-bit); another current device.
 *
 * spmv_permute_vector: dst[r] = src[perm[r]] for r < n, or with inverse = 1 dst[perm[r]] = src[r]; bits copied, one launch,
 * asynchronous, graph-capturable.  An entry of perm outside [0, n) moves nothing.  SPMV_ERR_INVALID: a null array while
 * n > 0, n < 0, inverse outside {0, 1}, src and dst that overlap (a pointer equal to the other included). */
#define SPMV_COLOR_SERIAL_MAX 32        /* neighbour entries (a's row plus its transpose's) of a row coloured by one lane */
#define SPMV_PERMUTE_KEEP_MAP 1
#define SPMV_PERMUTE_VIA_TRANSPOSE 2
SPMV_API int spmv_csr_color(const spmv_csr_t *a, uint32_t seed, void *stream, int32_t *d_color /* rows */,
                            int32_t *d_perm /* rows, or NULL */, int32_t *color_ptr /* host, or NULL */, int cap /* entries of color_ptr */,
                            int64_t info[8]);
SPMV_API int spmv_csr_permute(const spmv_csr_t *a, const int32_t *d_row_perm /* NULL: identity */,
                              const int32_t *d_col_perm /* NULL: identity */, int flags, void *stream, spmv_csr_t **out);
SPMV_API int spmv_csr_permute_values(spmv_csr_t *b, const spmv_csr_t *a, void *stream);
SPMV_API int spmv_csr_permute_gather(const spmv_csr_t *b, int count, const void *d_src, int64_t src_stride, void *d_dst,
                                     int64_t dst_stride, void *stream);
SPMV_API int64_t spmv_csr_permute_map_bytes(const spmv_csr_t *b);
SPMV_API int spmv_permute_vector(const int32_t *d_perm, int64_t n, int inverse, const float *d_src, float *d_dst, void *stream);

/* ---- the hot path ------------------------------------------------------
 * spmv_csr_plan: one-off device-side preprocessing a variant needs (chunk
 * boundaries, column windows, for SPMV_TILED also a 16-bit copy of the column
 * indices; workgroup size and pass budget follow from the chunk statistics,
 * with SPMV_AUTOTUNE=1 from timed trial launches instead); SPMV_SCALAR, SPMV_WAVE
 * and SPMV_WAVE_PIPE share one (see the enum; a no-op for SPMV_WAVE on rows of mean > 32).  A handle belongs to the device that was current when it was
 * created: plan and run fail with SPMV_ERR_INVALID under another current device.  Excluded from the timed SpMV like the reference
 * excludes its host format build from TIME_KERNEL (e.g. wsp.cu:146 vs :167).
 * A plan snapshots the sparsity PATTERN (row_ptr, col_idx): with borrowed
 * arrays (spmv_csr_create_device) the pattern must not change afterwards;
 * vals are read live on every run and may be updated freely -- except by
 * SPMV_PANEL and SPMV_XSKIP, whose plans re-order the nonzeros and keep their own copy
 * of the values (after changing them re-plan with spmv_csr_plan_set, which always
 * rebuilds; spmv_csr_plan is idempotent; the panel layout also replaces col_idx and
 * vals byte for byte in what a run reads, and is limited to 2^29 columns).
 * spmv_csr_run: enqueue y = A x on `stream` (a hipStream_t, NULL = default).
 * Asynchronous; d_x has cols floats, d_y has rows floats and is fully
 * overwritten.  No allocation, no synchronisation: graph-capturable -- with
 * one exception: SPMV_SCALAR / SPMV_WAVE_PIPE on a handle that spmv_csr_plan
 * has not seen make their plan on the first run (an allocation and a wait).
 * Alignment: d_x must be 16-byte aligned (SPMV_ERR_INVALID otherwise, nothing launched: the kernels stage x with
 * 16-byte loads); d_y needs only its natural 4 bytes -- a row block of a larger y (y_full + first_row) is fine, and
 * nothing outside y[0, rows) is written.
 *
 * Limits of the layouts.  A handle admits rows, cols, nnz < 2^31, and SPMV_SCALAR, SPMV_WAVE, SPMV_WAVE_PIPE,
 * SPMV_VECTOR, SPMV_ADAPTIVE and SPMV_TILED run every such handle (nnz up to 2^31 - 1, y and row_ptr beyond 4 GiB, x
 * beyond 4 GiB).  The layouts that re-order the nonzeros hold less; a plan outside a limit fails with SPMV_ERR_INVALID
 * and a message that names it, launches nothing and leaves the handle usable, and SPMV_AUTO passes on to the next
 * layout that can hold the matrix (in the end SPMV_TILED):
 *   SPMV_PANEL, panel sweep (params[6] = 1)   nnz <= INT_MAX - 8192 (the stream reads four steps of 2048 ahead);
 *                                             cols <= 2^29 (4096 panels of 2^17 columns)
 *   ... x panels in LDS (params[6] = 2)       the same nnz; cols <= 2^26 (4096 panels of 2^14 columns)
 *   ... sorted blocks (params[6] = 3)         nnz <= INT_MAX / 17 * 16 - 4096 (2 021 156 976: a unit of 16 slots may
 *                                             hold one pad slot, and the padded count stays a 32-bit number)
 *   ... binned, both flavours (4, 5)          cols <= 2^27 (4096 panels of 2^15 columns); nnz <= 2^30 - 8 * panels - 512
 *                                             (the products lie behind one buffer descriptor: 4 GiB); bins x (panels + 1)
 *                                             <= 2^30 table entries; params[6] = 5 also: the entries padded per bin
 *                                             stay below 2^30, bins x panel groups <= 2^30 fill items
 *   SPMV_XSKIP                                ceil(rows / 1024) x cols <= 2^27 table entries; rows sorted, duplicate-free
 *   spmv_csr_spmm                             rows x lanes per row < 2^32 (one launch): any handle up to k = 8,
 *                                             rows < 2^30 up to k = 16, < 2^29 up to k = 32, < 2^28 up to k = 64
 *   spmv_csr_sddmm                            the same as spmv_csr_spmm (rows x lanes per row < 2^32); any nnz < 2^31
 *   spmv_csr_spmm_16, spmv_csr_sddmm_16       the same as spmv_csr_spmm and spmv_csr_sddmm (the lanes per row are those of k)
 *   spmv_csr_spmm_cols                        rows x 16 lanes x ceil(k / 64) column tiles < 2^32 (one launch carries all tiles)
 *   spmv_csr_sddmm_cols                       rows x 16 lanes < 2^32 (rows < 2^28) at every k
 *   spmv_csr_row_softmax                      any handle (rows, nnz < 2^31; a wavefront per 64 rows, byte offsets 64-bit)
 *   spmv_csr_row_softmax_backward             the same as spmv_csr_row_softmax
 *   spmv_csr_attention_forward, _backward_q,  the same as spmv_csr_spmm with max(k, kv) in the place of k (rows x lanes per
 *   _backward_kv                              row < 2^32; on the transposed handle its rows); any nnz < 2^31
 *   spmv_csr_attention_forward_heads,         the single-head limits with rows x lanes per row x heads < 2^32 (every head of a
 *   _backward_q_heads, _backward_kv_heads     call is one launch) and heads <= 65535; where the long rows have more pieces
 *                                             than the handle has rows, the pieces stand in the place of the rows
 *   spmv_csr_transpose                        any handle
 *   spmv_csr_select_topk, _select_threshold   any handle (rows, nnz < 2^31; a wavefront per 64 rows, byte offsets 64-bit)
 *   spmv_csr_spgemm                           any two handles whose product has fewer than 2^31 nonzeros and whose rows of a
 *                                             have at most 2^30 terms each
 * (tests/test_gpu_limits.py runs every path on either side of these; the _heads calls' limits are refused and queried on
 * either side in tests/test_gpu_attention_heads.py, where a launch at the limit itself would write 64 GiB.) */
SPMV_API int spmv_csr_plan(spmv_csr_t *h, int variant, void *stream);
SPMV_API int spmv_csr_run(spmv_csr_t *h, int variant, const float *d_x, float *d_y, void *stream);

/* Tell the handle that the caller has rewritten vals (borrowed arrays, spmv_csr_create_device).  The variants that
 * read vals live need nothing; the plans of SPMV_PANEL and SPMV_XSKIP hold a re-ordered COPY of the values, and from
 * this call on spmv_csr_run of those variants (and of SPMV_AUTO where it resolved to one of them) fails with
 * SPMV_ERR_STALE_PLAN instead of multiplying with the old values, until spmv_csr_plan (which rebuilds a stale plan
 * with the parameters it had) or spmv_csr_plan_set has run again.  The library cannot see a write it is not told
 * about; for hunting one down set SPMV_CHECK_VALUES=1 in the environment: plans then also keep a checksum of vals and
 * every run of those variants recomputes it first (one pass over vals and a host wait per run -- a debug aid, not
 * graph-capturable).  Runs of one handle must be stream-ordered: plans own scratch buffers (slab partials, carries)
 * that two concurrent runs of the same handle on different streams would share. */
SPMV_API int spmv_csr_values_changed(spmv_csr_t *h);

/* What decides a plan's chunk cuts and with them the order of every fp32 sum, as numbers a caller can carry from
 * one handle to another (rank 0 to the other ranks of a job, one run to the next):
 *   params[0] variant actually planned (SPMV_AUTO resolves to SPMV_TILED or SPMV_PANEL)
 *   params[1] threads per workgroup (ADAPTIVE/TILED: 256 | 512 | 1024; a chunk is 16x that many nonzeros)
 *   params[2] staging-pass budget (TILED)        params[3] 1 = keep the 16-bit column copy where it pays (TILED)
 *   params[4] log2(columns per panel) (PANEL)    params[5] wavefronts per launch (PANEL)
 *   params[6] PANEL layout: 1 = panel sweep, x gathered through L2; 2 = the sweep with x staged in LDS; 3 = sorted blocks
 *             (params[4] = rows per block 4096 | 8192, params[5] = wavefronts per workgroup); 4 = binned, the sum launch fetches
 *             the tiles (params[4] = rows per bin 1024 ... 8192); 5 = binned, the product launch stores in bin order
 *             (params[4] = rows per bin 4096 | 8192 | 16384); 0 on input: the library's rule                 params[7] 0
 * spmv_csr_plan (the default) derives them from the matrix alone -- no timing -- so two handles of one matrix
 * already agree; handles of DIFFERENT row blocks of one matrix may not, and with SPMV_AUTOTUNE=1 nothing is
 * guaranteed.  spmv_csr_plan_set plans with exactly these numbers (replacing any existing plan of that variant),
 * spmv_csr_plan_like copies them from `src`.  Row blocks whose first nonzero offsets are multiples of the chunk
 * size, planned alike, give y bit-identical to the whole matrix planned alike (ADAPTIVE/TILED). */
SPMV_API int spmv_csr_plan_get(const spmv_csr_t *h, int variant, int32_t params[8]);
SPMV_API int spmv_csr_plan_set(spmv_csr_t *h, int variant, const int32_t params[8], void *stream);
SPMV_API int spmv_csr_plan_like(spmv_csr_t *dst, const spmv_csr_t *src, int variant, void *stream);

/* Bytes of plan data the variant reads per run.  Chunk boundaries, carries and windows come on top
 * of the CSR arrays; the 16-bit column offsets of SPMV_TILED REPLACE the 4-byte col_idx reads of the
 * chunks that have them (2 bytes per nonzero instead of 4), so a tiled run can move fewer HBM
 * bytes than the CSR-algorithmic count. */
SPMV_API int64_t spmv_csr_plan_bytes(const spmv_csr_t *h, int variant);

/* One-line description of the plan ("block=512 maxpass=4 chunks=32768 single=31080 col16=31080 ...")
 * written to buf (NUL-terminated, truncated to n). */
SPMV_API int spmv_csr_plan_describe(const spmv_csr_t *h, int variant, char *buf, int n);

/* The order in which the one launch of a SPMV_TILED plan with chunks of several kinds takes them (SPMV_AUTO: where it
 * resolved to SPMV_TILED): 0 = no such launch (every chunk is of one kind, or the plan is persistent), 1 = lists (the
 * 32-bit chunks first, then the sorted, then the 16-bit ones), 2 = identity (workgroup b takes chunk b of its XCD's range,
 * no chunk list is read).  The plan picks it from the share of chunks without 16-bit columns; SPMV_TILED_ORDER=identity|lists
 * in the environment forces one when the plan is made.  y does not depend on it.  Negative: an error code. */
SPMV_API int spmv_csr_plan_chunk_order(const spmv_csr_t *h, int variant);

/* Run `iters` back-to-back launches on `stream` between two HIP events
 * recorded on that same stream; returns the mean milliseconds per launch.
 * replaces: TIME_KERNEL (src/include/kernel.hpp:31-48). */
SPMV_API int spmv_csr_time(spmv_csr_t *h, int variant, const float *d_x, float *d_y, int iters,
                  void *stream, float *ms_per_launch);

/* Host-buffer convenience used by the C++ launchers: upload x (cols floats),
 * plan if needed, one untimed launch (code-object load, caches), one launch
 * between HIP events, download y (rows floats).  Synchronous.  *kernel_ms (may
 * be NULL) receives the event time of the second launch (the reference times a
 * single cold launch, kernel.hpp:31-48).  The dense and tcsr *_host calls do
 * the same.
 * replaces: the malloc/memcpy/TIME_KERNEL/memcpy/free body of a reference
 * launcher (e.g. csr_naive.cu:36-73). */
SPMV_API int spmv_csr_run_host(spmv_csr_t *h, int variant, const float *x_host, float *y_host,
                               float *kernel_ms);

/* ---- SpMM: one handle times k right-hand sides at once -------------------------------------------------------
 * Y = A X, where X holds k vectors side by side: X is cols rows of ldx floats, row-major (column c of X is
 * X[j*ldx + c], j < cols), Y is rows rows of ldy floats.  Column c < k of Y is A times column c of X under the CSR
 * semantics above: every term counts and a repeated column adds each of its terms, rows need not be sorted, IEEE rules
 * hold and subnormals are kept, an empty row gives 0, and an X row no nonzero refers to is never read into a sum.
 * Limits: 1 <= k <= 64, ldx >= k, ldy >= k, rows x lanes per row < 2^32 ("Limits of the layouts" above); d_X and d_Y 16-byte aligned (d_X may be NULL when cols == 0, d_Y when
 * rows == 0).  Any ld >= k works; ldx % 4 == 0 and ldy % 4 == 0 together are the fast path (16-byte loads and stores;
 * a run then reads the whole 16-byte block that holds X[j*ldx + k-1]).  Anything else, a null handle or another current
 * device than the handle's is SPMV_ERR_INVALID, and nothing is launched.  Y[i*ldy + c] for c >= k is never written, and
 * X[j*ldx + c] for c >= k is never read into a sum.
 * spmv_csr_spmm_plan: a function of the pattern (row_ptr) alone -- not of the values, of k or of timing.  It reads row_ptr
 * back and waits for the stream; it is idempotent, and spmv_csr_destroy frees it.  Its scratch for the partial sums of
 * long rows is sized for k = 64.  vals are read live on every run: after an in-place update the next run uses them.
 * spmv_csr_spmm: enqueue Y = A X on `stream`; asynchronous, allocates nothing, never waits: graph-capturable once the
 * plan exists; SPMV_ERR_NOT_PLANNED without it.  Runs of one handle must be stream-ordered (the plan owns the scratch).
 * Batch invariance: for one plan, Y[:, c] is bit-identical whatever k, ldx and ldy are, whichever position the column
 * has in the batch and whatever the other columns of X hold (NaN and Inf included); two runs, and two handles of the same
 * matrix, agree bit for bit.  The order of the fp32 additions of a row is the plan's own and part of the interface: per
 * output column acc = fma(vals[n], X[col_idx[n]][c], acc) over the row's nonzeros in storage order, from +0; a row of more
 * than 512 nonzeros is summed per piece of 512 in the same way, each from +0, and the pieces' sums are added in piece order,
 * from +0 (no variant's order).  tests/test_gpu_order.py holds the kernels to this bit for bit.
 * spmv_csr_spmm_plan_bytes: device bytes of the plan (0 when not planned; negative for a null handle).
 * spmv_csr_spmm_describe: the plan in one line ("row_cap=512 piece_len=512 long_rows=... pieces=..."). */
SPMV_API int spmv_csr_spmm_plan(spmv_csr_t *h, void *stream);
SPMV_API int spmv_csr_spmm(spmv_csr_t *h, int k, const float *d_X, int64_t ldx, float *d_Y, int64_t ldy, void *stream);
SPMV_API int64_t spmv_csr_spmm_plan_bytes(const spmv_csr_t *h);
SPMV_API int spmv_csr_spmm_describe(const spmv_csr_t *h, char *buf, int n);

/* ---- SDDMM: a dense-dense product sampled at the handle's pattern ----------------------------------------------
 * out[n] = sum over c < k of U[i*ldu + c] * X[j*ldx + c] for every storage position n in [row_ptr[i], row_ptr[i+1]) with
 * j = col_idx[n]: the entries of U X^T at the stored nonzeros, in the storage order of h.  U is rows rows of ldu floats,
 * row-major, X is cols rows of ldx floats, out holds nnz floats.  With Y = A X (spmv_csr_spmm) and a gradient dY this is
 * the gradient for the VALUES of A, dvals = sddmm(dY, X); the gradient for X is spmv_csr_spmm on the transposed handle.
 * Every stored nonzero gets its own result: a column repeated inside a row gives the same number at each occurrence, rows
 * need not be sorted, IEEE rules hold and subnormals are kept.  An X row no nonzero refers to and the U row of an empty
 * row never reach a result.  vals is never read, so d_out may be the caller's own borrowed vals array (followed by
 * spmv_csr_values_changed).  Nothing outside out[0, nnz) is written.
 * Limits: 1 <= k <= 64, ldu >= k, ldx >= k, rows x lanes per row < 2^32 ("Limits of the layouts" above; any nnz < 2^31:
 * byte offsets into col_idx and out are 64-bit); d_U and d_X 16-byte aligned (d_U may be NULL when rows == 0, d_X when
 * cols == 0, d_out when nnz == 0); d_out needs only its natural 4 bytes -- a row block may write into out_full +
 * first_nnz.  Any ld >= k works; ldu % 4 == 0 and ldx % 4 == 0 together are the fast path (16-byte loads; a run then
 * reads the whole 16-byte block that holds column k-1 of a row).  U[i*ldu + c] and X[j*ldx + c] for c >= k are never
 * read into a sum (they are skipped, not multiplied by zero).
 * The plan is spmv_csr_spmm_plan's (a function of row_ptr alone; one plan serves both calls); SPMV_ERR_NOT_PLANNED
 * without it.  A row of more than 512 nonzeros is processed per plan piece; results are independent, so there is no
 * scratch and runs of one handle need no stream order among themselves.  Asynchronous, allocates nothing, never waits:
 * graph-capturable once the plan exists.  A null handle, k or an ld out of range, a misaligned or missing pointer or
 * another current device than the handle's is SPMV_ERR_INVALID with a message that names the function; nothing is
 * launched and out is untouched.
 * The order of the sums is part of the interface.  With V = the power of two >= ceil(k / 4) (1, 2, 4, 8, 16):
 *     p_s = +0;  p_s = fma(U[i][c], X[j][c], p_s) for c = 4s, 4s+1, 4s+2, 4s+3 while c < k        (s = 0 .. V-1)
 *     for m = V/2, V/4, ..., 1:  p_s = p_s + p_(s xor m) for every s;      out[n] = p_0
 * So out[n] is a pure function of the k floats of its U row, the k floats of its X row and k: not of ldu or ldx, of the
 * fast or slow load path, of the nonzero's position in its row or the row's length, of whether the row went in pieces,
 * of what other rows hold, of the stream or of the handle.  It is symmetric in its operands (fma(u, x, p) == fma(x, u,
 * p)): with T = transpose(A) and perm = argsort(a.col_idx, stable), sddmm(T, X, U)[i] == sddmm(A, U, X)[perm[i]] bit for
 * bit (for results that are not NaN; a NaN is a NaN on both sides). */
SPMV_API int spmv_csr_sddmm(spmv_csr_t *h, int k, const float *d_U, int64_t ldu, const float *d_X, int64_t ldx,
                            float *d_out, void *stream);

/* ---- Row softmax over the handle's pattern, forward and backward -------------------------------------------------
 * The step between the SDDMM that makes the scores of a sparse attention and the SpMM that applies them:
 *     forward    S = sddmm(Q, K);  P = row_softmax(scale, S);  O = spmm(P, V)
 *     backward   dV = spmm(P^T, dO);  dP = sddmm(dO, V);  dS = row_softmax_backward(scale, P, dP);  dQ = spmm(dS, K);
 *                dK = spmm(dS^T, Q)
 * all on one pattern, one SpMM plan and one transposed handle (spmv-test_amd/sparse_attention.py composes them).  Every
 * array holds nnz floats in the storage order of h.  col_idx and vals are never read: only row_ptr and the SpMM plan.
 * spmv_csr_row_softmax, for every row i with L = row_ptr[i+1] - row_ptr[i] > 0 and n in [row_ptr[i], row_ptr[i+1]):
 *     t[n] = scale * scores[n]         (one fp32 rounding; never fused into the subtraction)
 *     M    = max t                      (fmaxf: a NaN is ignored here)
 *     e[n] = expf(t[n] - M)             (the device library's expf, 1 ulp)
 *     S    = sum e                      (the order below)
 *     r    = 1.0f / S                   (IEEE division)
 *     out[n] = e[n] * r
 * An empty row writes nothing.  IEEE rules decide every special case and agree with torch.softmax: t = -Inf beside a
 * finite maximum gives exactly +0; a row that holds a NaN or a +Inf (or whose scale * s overflows to +Inf) is NaN
 * throughout; a row whose every entry is -Inf is NaN throughout; subnormal results are kept.
 * spmv_csr_row_softmax_backward, with P and dP whatever the caller passes (P need not come from the forward call):
 *     dot = sum over the row of fp32(P[n] * dP[n])             (the products rounded, then summed in the order below)
 *     dS[n] = scale * (P[n] * (dP[n] - dot))                   (three roundings)
 * The order of the sums is part of the interface.  A piece is a whole row of at most 512 entries, or, in a row of more
 * (the SpMM plan's row_cap), entries [512 j, 512 j + 512) of the row; x_0 .. x_(len-1) are a piece's terms:
 *     q_l = +0;  q_l = q_l + x_(l + 64 i) for i = 0, 1, ... while l + 64 i < len            (l = 0 .. 63)
 *     for m = 32, 16, ..., 1:  q_l = q_l + q_(l xor m) for every l;      the piece's sum is q_0
 * and a row of several pieces adds its pieces' sums in piece order, starting from +0.  The maximum is exact in any order.
 * So a row's results are a pure function of its L inputs in storage order, of L and of scale: not of other rows, of the
 * row's position in the matrix, of the stream, of the handle, of running in place, or of whether the handle is a row
 * block (row_ptr rebased, arrays at array_full + first_nnz) or the whole matrix.  (A short row runs in a group of
 * G = pow2 >= L lanes; the lanes it leaves out would hold +0, and adding +0 changes no q, so the bits are the ones above.)
 * Long rows take the three-read form: the pieces' maxima, the row's maximum, the pieces' sums of expf(t - M), the row's
 * sum, then the store (backward: the pieces' dots, the row's dot, the store); rows of at most 512 entries are read once,
 * held in registers and written once.  The scratch of the long rows is the SpMM plan's (64 floats per piece), so runs
 * of one handle -- these two calls and spmv_csr_spmm alike -- must be stream-ordered; a handle without a long row uses none.
 * Aliasing: d_out == d_scores, d_dS == d_P and d_dS == d_dP are allowed (the identical pointer only; a partial overlap
 * is the caller's error and is not checked), and each array may be the handle's own borrowed vals (then follow with
 * spmv_csr_values_changed).  Every pointer needs only its natural 4 bytes; nothing outside [0, nnz) is written.
 * Asynchronous, allocates nothing, never waits: graph-capturable once spmv_csr_spmm_plan has run; SPMV_ERR_NOT_PLANNED
 * without it.  Any handle is accepted (rows, nnz < 2^31; byte offsets are 64-bit).  A null handle, a null array while
 * nnz > 0, a pointer that is not 4-byte aligned, a scale that is not finite or another current device than the handle's
 * is SPMV_ERR_INVALID with a message that names the function; nothing is launched and the output is untouched.  With
 * nnz == 0 the call returns SPMV_OK whatever the pointers are. */
SPMV_API int spmv_csr_row_softmax(spmv_csr_t *h, float scale, const float *d_scores, float *d_out, void *stream);
SPMV_API int spmv_csr_row_softmax_backward(spmv_csr_t *h, float scale, const float *d_P, const float *d_dP,
                                           float *d_dS, void *stream);

/* ---- Fused attention: forward and backward on the pattern without an array of nnz floats ---------------------------
 * O = softmax_rows(scale * Q K^T at the pattern of h) V and its gradients in three row-parallel passes.  What the
 * composition above (SDDMM, row softmax, SpMM, transpose_values) does in nnz-sized arrays happens here in registers:
 * no score, probability or gradient of one is stored, of nnz size only col_idx is read (4 bytes per nonzero and pass), no
 * atomics, no transpose map.  h is queries x keys: Q is rows rows of k floats (leading dimension ldq), K cols rows of k,
 * V cols rows of kv, O and dO rows rows of kv, dQ like Q, dK like K, dV like V; stats holds 2 rows floats, delta rows
 * floats.  vals is never read (handle creation still wants the array).
 *   spmv_csr_attention_forward(h)       writes O and stats: stats[2i] = M_i, the maximum of t = fp32(scale * s) over row i,
 *                                       stats[2i+1] = r_i = 1.0f / l_i with l_i the row's sum of exponentials below -- not a
 *                                       log-sum-exp.  An empty row gets a zero row of O and stats = (-Inf, +0).
 *   spmv_csr_attention_backward_q(h)    reads O, dO and stats; writes delta_i = dO_i . O_i and dQ (0 for an empty row).
 *   spmv_csr_attention_backward_kv(t)   t = the handle of the TRANSPOSED pattern (spmv_csr_transpose(h, keep_map = 0)): its
 *                                       rows are keys, its columns queries.  Reads stats and delta; writes dK and dV (0 for a
 *                                       key no query refers to).  Needs only t's pattern: no map, no values.
 * The probability of a nonzero is p = expf(t - M_i) * r_i in both backward passes, and s is spmv_csr_sddmm's number bit
 * for bit in all three passes and on both handles, so the passes agree on every p.
 * Special cases agree with torch.softmax and with the row softmax above: t = -Inf beside a finite maximum contributes
 * exactly nothing (also when a whole leading stretch of the row is -Inf); a row that holds a NaN or a +Inf score, or whose
 * every score is -Inf, has a NaN row of O (and NaN gradients wherever it contributes).
 * The plan: spmv_csr_attention_plan makes the SpMM plan if it is missing (spmv_csr_spmm_plan, unchanged) and allocates the
 * scratch of the long rows: per piece of a row of more than 512 nonzeros 132 floats (m, l, and up to 128 partial sums at a
 * 16-byte boundary); nothing for a handle without such a row.  Idempotent; h and t each need theirs.  After it the three
 * calls allocate nothing and never wait: graph-capturable.  Calls on one handle must be stream-ordered (they share the
 * scratch).  spmv_csr_attention_plan_bytes: device bytes of both plans together (0 when not planned).
 * Limits and refusals as spmv_csr_sddmm: 1 <= k, kv <= 64, every ld >= its width, every matrix 16-byte aligned (stats
 * 8-byte, delta 4-byte), a finite scale, the plan made (SPMV_ERR_NOT_PLANNED), rows x lanes per row < 2^32; anything else
 * is SPMV_ERR_INVALID with a message that names the function, nothing is launched and every output is untouched.  With
 * every ld % 4 == 0 the passes use 16-byte loads and stores, otherwise 4-byte ones; columns at or past the width are never
 * read into a sum nor written.  Outputs must not overlap inputs (not checked).
 * The order of the sums is part of the interface.  V = the power of two >= ceil(max(k, kv) / 4), T = max(V, 8):
 *   s, dp    p_s = +0; p_s = fma(a[c], b[c], p_s) for c = 4s .. 4s+3 while c < width; then for m = V/2 .. 1: p_s = p_s +
 *            p_(s xor m); the number is p_0 (a group wider than SDDMM's adds lanes that hold +0: the same bits).
 *            s = Q_i . K_j over k, dp = dO_i . V_j over kv; t = scale * s, rounded.
 *   forward  a span is a row of at most 512 nonzeros or one of the SpMM plan's pieces; m = -Inf, l = +0, acc = +0, then per
 *            step of T consecutive nonzeros: m' = max(m, the step's t) (a NaN is ignored here); z = m' unless m' = -Inf,
 *            then 0; a = expf(m - z); e_t = expf(t_t - z); l = l * a; acc[c] = acc[c] * a; then for the step's nonzeros in
 *            storage order l = l + e_t, acc[c] = fma(e_t, V[j_t][c], acc[c]); m = m'.
 *            A row of one span: r = 1.0f / l, O[i][c] = acc[c] * r, stats = (m, r).  A row in pieces: M = max m_p, z as
 *            above, w_p = expf(m_p - z), and from +0 in piece order l = fma(l_p, w_p, l), acc[c] = fma(acc_p[c], w_p, acc[c]);
 *            then r, O and stats = (M, r) alike.
 *   delta_i  d_s = +0; d_s = fma(dO[i][c], O[i][c], d_s) over the lane's columns below kv; the same butterfly.
 *   ds       = scale * (p * (dp - delta_i)), three roundings (as spmv_csr_row_softmax_backward)
 *   dQ_i[c]  = fma(ds, K[j][c], dQ_i[c]) over a span in storage order from +0; the spans of a row added in piece order from +0
 *   dV_j[c]  = fma(p, dO[i][c], dV_j[c]) and dK_j[c] = fma(ds, Q[i][c], dK_j[c]) over a span of t likewise
 * So a row's outputs are a pure function of its column list in storage order, its operands, k, kv and scale: not of any
 * ld or of the load path, of the row's position or neighbours, of the stream, of the handle, or of whether the handle is a
 * row block (row_ptr rebased) or the whole matrix. */
SPMV_API int spmv_csr_attention_plan(spmv_csr_t *h, void *stream);
SPMV_API int64_t spmv_csr_attention_plan_bytes(const spmv_csr_t *h);
SPMV_API int spmv_csr_attention_forward(spmv_csr_t *h, float scale, int k, const float *d_Q, int64_t ldq, const float *d_K,
                                        int64_t ldk, int kv, const float *d_V, int64_t ldv, float *d_O, int64_t ldo,
                                        float *d_stats, void *stream);
SPMV_API int spmv_csr_attention_backward_q(spmv_csr_t *h, float scale, int k, const float *d_Q, int64_t ldq, const float *d_K,
                                           int64_t ldk, int kv, const float *d_V, int64_t ldv, const float *d_O, int64_t ldo,
                                           const float *d_dO, int64_t lddo, const float *d_stats, float *d_delta,
                                           float *d_dQ, int64_t lddq, void *stream);
SPMV_API int spmv_csr_attention_backward_kv(spmv_csr_t *t, float scale, int k, const float *d_Q, int64_t ldq,
                                            const float *d_K, int64_t ldk, int kv, const float *d_V, int64_t ldv,
                                            const float *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                            float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, void *stream);

/* ---- Fused attention, all heads of one pattern in one launch ----------------------------------------------------------
 * The three passes above for `heads` heads at once: one grid per kernel with the head in its y dimension, instead of one
 * call (one to four launches) per head.  Every pointer argument is head 0's; spmv_attn_heads_t says how many floats lie
 * between head y and head y + 1 of each operand.
 * Semantics: head y of a _heads call is, bit for bit, the single-head call with every pointer advanced by y times its
 * stride.  Nothing of the order of the sums above changes; the kernels are the same ones (a single-head call is heads = 1
 * with every stride 0).  Each call reads only the strides of the operands it takes: forward q, k, v, o, stats;
 * backward_q q, k, v, o, d_o, stats, delta, dq; backward_kv q, k, v, d_o, stats, delta, dk, dv.
 * The plan: spmv_csr_attention_plan_heads makes the attention plan if it is missing and sizes the scratch of the long rows
 * for `heads` heads: heads x pieces x 132 floats, head y using the slice at y x pieces x 132.  It only grows, and is
 * idempotent when the plan already covers `heads`; like the other plan calls it allocates and waits for the stream.
 * spmv_csr_attention_plan remains and means heads = 1.  spmv_csr_attention_plan_bytes reports the grown scratch
 * ((heads - 1) x pieces x 132 x 4 bytes more; nothing more for a handle without a long row).  A _heads call with more heads
 * than planned is SPMV_ERR_NOT_PLANNED, also on a handle without a long row (one rule).  After the plan the three calls
 * allocate nothing and never wait: graph-capturable.  h and t each need theirs.
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, every output untouched): a null hs,
 * heads < 1, reserved != 0, heads > 65535 or rows x lanes per row x heads >= 2^32 ("Limits of the layouts";
 * spmv_csr_attention_max_heads says how many heads fit); a negative
 * stride; a stride of a matrix operand that is no multiple of 4 (every head stays 16-byte aligned), a stats stride that is
 * odd (delta: any); with heads > 1 an output stride below the output's width (o: kv, dq and dk: k, dv: kv, stats: 2,
 * delta: 1); and everything the single-head call refuses.
 * Shared inputs: an input stride may be 0, so one K and V serve all heads (multi-query attention) without a copy; dK and
 * dV then still come out per head, and the caller sums them.  (The _gqa calls below share K and V in groups and sum dK
 * and dV themselves.)
 * Not checked: overlap between the outputs of different heads beyond the width rule (a stride below rows x ld of a stacked
 * output, say) is the caller's error, as "outputs must not overlap inputs" is.  Column blocks of one wide matrix
 * (stride = k, ld = heads x k) are a legal layout: the heads' rows interleave without overlapping. */
typedef struct spmv_attn_heads {
    int32_t heads, reserved;                            /* reserved = 0 */
    int64_t q, k, v, o, d_o, stats, delta, dq, dk, dv;  /* floats from head h to head h+1 */
} spmv_attn_heads_t;

SPMV_API int spmv_csr_attention_plan_heads(spmv_csr_t *h, int heads, void *stream);
/* The most heads one _heads call on h takes at these widths (the launch limits above, from h's rows and the pieces of its
 * long rows; 0: not even one; needs the plan, else SPMV_ERR_NOT_PLANNED; a negative status otherwise).  A caller with more
 * heads splits them into several calls; h and t may differ. */
SPMV_API int spmv_csr_attention_max_heads(const spmv_csr_t *h, int k, int kv);
SPMV_API int spmv_csr_attention_forward_heads(spmv_csr_t *h, const spmv_attn_heads_t *hs, float scale, int k, const float *d_Q,
                                              int64_t ldq, const float *d_K, int64_t ldk, int kv, const float *d_V,
                                              int64_t ldv, float *d_O, int64_t ldo, float *d_stats, void *stream);
SPMV_API int spmv_csr_attention_backward_q_heads(spmv_csr_t *h, const spmv_attn_heads_t *hs, float scale, int k,
                                                 const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv,
                                                 const float *d_V, int64_t ldv, const float *d_O, int64_t ldo,
                                                 const float *d_dO, int64_t lddo, const float *d_stats, float *d_delta,
                                                 float *d_dQ, int64_t lddq, void *stream);
SPMV_API int spmv_csr_attention_backward_kv_heads(spmv_csr_t *t, const spmv_attn_heads_t *hs, float scale, int k,
                                                  const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv,
                                                  const float *d_V, int64_t ldv, const float *d_dO, int64_t lddo,
                                                  const float *d_stats, const float *d_delta, float *d_dK, int64_t lddk,
                                                  float *d_dV, int64_t lddv, void *stream);

/* ---- Fused attention, grouped-query heads (GQA): H query heads on H / g K/V heads, dK and dV summed in the kernel ---------
 * The three _heads passes for query heads that share K and V in groups: hs->heads = H query heads, group = g query heads
 * per K/V head, query head y uses K/V head y / g.  hs->k, hs->v, hs->dk and hs->dv are the floats from one K/V head to the
 * next (K, V, dK and dV hold H / g heads); every other stride is per query head as above.  spmv_attn_heads_t is unchanged
 * (88 bytes, reserved = 0).  K and V are neither expanded nor copied, dK and dV come out once per K/V head: g times fewer
 * rows written than by a _heads call on expanded K/V, and no reduction pass afterwards.
 * The plan: the call needs the plan to cover hs->heads query heads (spmv_csr_attention_plan_heads), else
 * SPMV_ERR_NOT_PLANNED; the scratch layout (a slice per query head), spmv_csr_attention_plan_bytes and
 * spmv_csr_attention_max_heads are unchanged, and the limit of one launch is the _heads limit on hs->heads.  After the plan
 * the calls allocate nothing and never wait: graph-capturable.
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, every output untouched): group < 1,
 * hs->heads % group != 0, and everything the _heads call refuses; the output-stride rule for dk and dv applies when there is
 * more than one K/V head (hs->heads / group > 1).
 * The order of the sums (part of the interface, beside the text of "Fused attention" above):
 *   forward, backward_q   head y of a _gqa call is, bit for bit, the single-head call with Q, O, dO, stats, delta and dQ
 *            advanced by y times their strides and K, V advanced by (y / g) times theirs.  group = 1 is the _heads call bit
 *            for bit.
 *   backward_kv   for K/V head c let dK^(i), dV^(i) be what the single-head spmv_csr_attention_backward_kv gives for query
 *            head c g + i with K, V of head c (the order above: a span in storage order from +0, a long row's pieces added
 *            in piece order from +0).  Then dK_c = (..((dK^(0) + dK^(1)) + dK^(2)) .. + dK^(g-1)): fp32 additions in head
 *            order, starting from head 0's value and not from +0; dV_c alike.  It is not a sum over the heads inside a
 *            piece.  group = 1 is therefore the _heads call bit for bit.  A key no query lists gets +0. */
SPMV_API int spmv_csr_attention_forward_gqa(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, float scale, int k,
                                            const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv,
                                            const float *d_V, int64_t ldv, float *d_O, int64_t ldo, float *d_stats,
                                            void *stream);
SPMV_API int spmv_csr_attention_backward_q_gqa(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, float scale, int k,
                                               const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv,
                                               const float *d_V, int64_t ldv, const float *d_O, int64_t ldo,
                                               const float *d_dO, int64_t lddo, const float *d_stats, float *d_delta,
                                               float *d_dQ, int64_t lddq, void *stream);
SPMV_API int spmv_csr_attention_backward_kv_gqa(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, float scale, int k,
                                                const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, int kv,
                                                const float *d_V, int64_t ldv, const float *d_dO, int64_t lddo,
                                                const float *d_stats, const float *d_delta, float *d_dK, int64_t lddk,
                                                float *d_dV, int64_t lddv, void *stream);

/* ---- Fused attention on 16-bit matrices: bf16 or fp16 operands, fp32 sums, all three passes ---------------------------------
 * The three _gqa passes with Q, K, V, O, dO, dQ, dK and dV stored as bf16 (dtype = SPMV_ATTN_BF16) or IEEE half
 * (SPMV_ATTN_FP16), all of one dtype; stats, delta and the scratch of the long rows stay fp32 (the same plan, the same
 * bytes).  Only the most general form exists: a _heads call is group = 1, one head is hs->heads = 1 with every stride 0.
 * Units: every ld and every matrix stride of hs counts ELEMENTS of the dtype (2 bytes); the stats and delta strides count
 * floats as before.
 * The rounding contract (part of the interface, beside the order of the sums above).  An operand element is widened
 * exactly to fp32 where it is used; every sum, expf, maximum and butterfly is the fp32 order stated under "Fused attention"
 * and "grouped-query heads", unchanged; an output element is rounded to the dtype once, to nearest even, at its store.
 * Nothing is accumulated in 16 bits.  So every element of O, dQ, dK and dV is, bit for bit, the round-to-nearest-even
 * conversion to dtype of what the matching _gqa fp32 call writes on the same operands widened to fp32, and stats and delta
 * are that call's bits.  backward_q forms delta from the 16-bit O it is given (the rounded one, if it is the forward call's).
 * No conversion flushes a subnormal; a NaN is stored as a NaN of the dtype (payload unspecified); fp16 overflows to +-Inf
 * as round-to-nearest-even says.
 * The plan: spmv_csr_attention_plan_heads, _plan_bytes, _max_heads and SPMV_ERR_NOT_PLANNED as for the _gqa calls; after the
 * plan the calls allocate nothing and never wait: graph-capturable.
 * Loads and stores: a lane's slice is 4 elements, 8 bytes.  With every ld of the pass a multiple of 4 it is one 8-byte access
 * (the last slice of a width that is no multiple of 4 is read whole inside its row's ld elements and stored below the width
 * only); otherwise the passes use 2-byte accesses of the columns below the width only.
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, every output untouched): a dtype other
 * than the two; a matrix that is not 8-byte aligned; a matrix stride that is no multiple of 4 elements; and everything the
 * _gqa call refuses. */
enum { SPMV_ATTN_BF16 = 1, SPMV_ATTN_FP16 = 2 };
SPMV_API int spmv_csr_attention_forward_16(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, float scale, int k,
                                           const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk, int kv,
                                           const void *d_V, int64_t ldv, void *d_O, int64_t ldo, float *d_stats,
                                           void *stream);
SPMV_API int spmv_csr_attention_backward_q_16(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, float scale,
                                              int k, const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk, int kv,
                                              const void *d_V, int64_t ldv, const void *d_O, int64_t ldo,
                                              const void *d_dO, int64_t lddo, const float *d_stats, float *d_delta,
                                              void *d_dQ, int64_t lddq, void *stream);
SPMV_API int spmv_csr_attention_backward_kv_16(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, int dtype, float scale,
                                               int k, const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk, int kv,
                                               const void *d_V, int64_t ldv, const void *d_dO, int64_t lddo,
                                               const float *d_stats, const float *d_delta, void *d_dK, int64_t lddk,
                                               void *d_dV, int64_t lddv, void *stream);

/* ---- SpMM and SDDMM on 16-bit matrices: bf16 or fp16 dense operands, fp32 values and sums ------------------------------------
 * spmv_csr_spmm and spmv_csr_sddmm with the dense matrices stored as bf16 (dtype = SPMV_ATTN_BF16) or IEEE half
 * (SPMV_ATTN_FP16), the enum of the _16 attention calls: X and Y of spmv_csr_spmm_16, U and X of spmv_csr_sddmm_16, all of one
 * dtype.  The handle's vals (the master weights of a layer), d_out (the gradient of those values) and the scratch of the long
 * rows stay fp32.  SPMV_ATTN_FP32 is refused here: the fp32 calls are spmv_csr_spmm and spmv_csr_sddmm.
 * Units: every ld counts ELEMENTS of the dtype (2 bytes).
 * The rounding contract (part of the interface, beside the order of the sums under "SpMM" and "SDDMM").  An operand element
 * is widened exactly to fp32 where it enters an fma; every accumulator, every partial of a long row and every butterfly is
 * the fp32 order stated there, unchanged; an element of Y is rounded to the dtype once, to nearest even, at its store (a long
 * row's after its pieces' fp32 partials are added in piece order).  Nothing is accumulated in 16 bits and vals is never
 * rounded.
 *   SpMM.   Every element of Y is, bit for bit, the round-to-nearest-even conversion to the dtype of what spmv_csr_spmm
 *           writes for the same handle on X widened to fp32.  Batch invariance carries over: a column's bits do not depend
 *           on k, ldx, ldy, its position in the batch or the other columns.  Y at columns >= k is never written; X at
 *           columns >= k is never read into a sum.
 *   SDDMM.  d_out holds the bits of spmv_csr_sddmm on U and X widened to fp32.  The symmetry with the transposed handle
 *           carries over: T.sddmm_16(X, U) is A.sddmm_16(U, X) through the transpose's permutation, bit for bit.
 *   Conversions.  No conversion flushes a subnormal; a NaN is stored as a NaN of the dtype (payload unspecified); fp16
 *           overflows to +-Inf as round-to-nearest-even says.
 * The plan is spmv_csr_spmm_plan's, unchanged, with the same bytes (spmv_csr_spmm_plan_bytes); SPMV_ERR_NOT_PLANNED without it.
 * After the plan the calls allocate nothing and never wait: graph-capturable.
 * Loads and stores: a lane's slice is 4 elements, 8 bytes.  With every ld of the call a multiple of 4 it is one 8-byte access
 * (the last slice of a k that is no multiple of 4 is read whole inside its row's ld elements and stored below k only);
 * otherwise the kernels use 2-byte accesses of the columns below k only.
 * Limits: 1 <= k <= 64, every ld >= k, rows x lanes per row < 2^32 ("Limits of the layouts" above).
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, every output untouched): a dtype other
 * than the two; a matrix that is not 8-byte aligned; and everything the fp32 call refuses: a null handle, k or an ld out of
 * range, a missing pointer (with the fp32 call's exceptions for empty dimensions), another current device, d_out not 4-byte
 * aligned. */
SPMV_API int spmv_csr_spmm_16(spmv_csr_t *h, int dtype, int k, const void *d_X, int64_t ldx, void *d_Y, int64_t ldy, void *stream);
SPMV_API int spmv_csr_sddmm_16(spmv_csr_t *h, int dtype, int k, const void *d_U, int64_t ldu, const void *d_X, int64_t ldx,
                               float *d_out, void *stream);

/* ---- SpMV on 16-bit values: bf16 or fp16 matrix values, fp32 x, y and sums ----------------------------------------------------
 * spmv_csr_run with the values of A taken from d_vals16 instead of the handle's fp32 vals: nnz elements of bf16 (dtype =
 * SPMV_ATTN_BF16) or IEEE half (SPMV_ATTN_FP16), the enum of the _16 calls, in the handle's storage order -- element n belongs
 * to col_idx[n].  The array is borrowed and read live on every call (overwrite it between calls freely; nothing is copied and
 * spmv_csr_values_changed is not needed).  The handle's own vals is never read by this call (creation still wants the array, as
 * for the attention calls); x and y stay fp32.  SPMV_ATTN_FP32 is refused here: the fp32 call is spmv_csr_run.
 * The contract (part of the interface).  Every value is widened exactly to fp32 where it is used, its product with x is one
 * fp32 multiplication, and every sum is the fp32 kernel's: y is, bit for bit, what spmv_csr_run(h', variant, x, y) writes on
 * a handle h' that has the same pattern, the same plan and vals[n] = widen(vals16[n]).  The order of every sum is therefore
 * the one tests/_tiled_order.py states for SPMV_TILED and SPMV_ADAPTIVE, and row blocks planned alike reproduce the whole
 * matrix as they do in fp32.  No conversion flushes a subnormal: an fp16 or bf16 subnormal widens to its exact fp32 value; an
 * Inf or a NaN widens to an Inf or a NaN.  Nothing is accumulated or multiplied in 16 bits.
 * Variants.  SPMV_TILED and SPMV_ADAPTIVE run, and SPMV_AUTO where its plan resolved to SPMV_TILED.  Every other variant is
 * SPMV_ERR_VARIANT with a message that names the function and what the variant resolved to -- SPMV_AUTO resolved to SPMV_PANEL
 * among them: the panel layouts hold a re-ordered copy of the fp32 values.  A variant that spmv_csr_plan has not seen is
 * SPMV_ERR_NOT_PLANNED.
 * The plan is spmv_csr_plan's own and is not changed: it is a function of the pattern, so one plan serves both calls, with the
 * same bytes (spmv_csr_plan_bytes) and the same line (spmv_csr_plan_describe).  A plan made with SPMV_PERSIST=1 runs this call
 * through the one-shot kernels (the persistent form exists for fp32 values only); the sums are the same, by the documented order.
 * After the plan the call allocates nothing and never waits: graph-capturable.  Runs of one handle must be stream-ordered, with
 * each other and with spmv_csr_run: the plan's carries are shared.
 * Loads: a lane reads four values in one 8-byte load; the ragged last chunk reads 2-byte elements below nnz only.  Nothing
 * outside y[0, rows) is written; d_y needs only its natural 4 bytes (a row block of a larger y is fine).  nnz == 0 gives
 * y = 0; rows == 0 returns SPMV_OK.
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, y untouched): a null handle; a dtype other
 * than the two; a null d_vals16 while nnz > 0; a d_vals16 or d_x that is not 16-byte aligned; a null x or y as in
 * spmv_csr_run; another current device than the handle's. */
SPMV_API int spmv_csr_run_vals16(spmv_csr_t *h, int variant, int dtype, const void *d_vals16, const float *d_x, float *d_y,
                                 void *stream);

/* ---- SpMM and SDDMM at any k: column tiles of 64 in one call -------------------------------------------------------------------
 * spmv_csr_spmm and spmv_csr_sddmm (and their _16 forms) for 1 <= k <= SPMV_COLS_MAX_K columns in one call.  dtype is
 * SPMV_ATTN_FP32 (fp32 matrices, 16-byte aligned, every ld in floats), SPMV_ATTN_BF16 or SPMV_ATTN_FP16 (8-byte aligned, every
 * ld in 16-bit elements), the codes of the _wide attention calls; vals, d_out and every sum are fp32 as in the narrow calls.
 * Column tile t of a call at width k is the columns [64t, 64t + k_t), k_t = min(64, k - 64t), of m = ceil(k / 64) tiles.
 *   SpMM.   Y[:, c] is bit for bit what spmv_csr_spmm (spmv_csr_spmm_16) writes for that column in any narrow call that
 *           contains it: the order per column is unchanged -- fma in storage order from +0; a row of more than 512 nonzeros per
 *           piece of 512, the pieces' sums added in piece order from +0; a 16-bit Y rounded once at its store -- and batch
 *           invariance now holds at every k.  Y at columns [k, ldy) is never written; X at columns >= k is never read into a sum.
 *   SDDMM.  out[n] = (..((r_0 + r_1) + r_2) .. + r_(m-1)): fp32 additions in tile order, starting from r_0's value and not from
 *           +0 (a result of -0 in a single tile stays -0).  r_t is exactly the number spmv_csr_sddmm defines for U[:, tile t] and
 *           X[:, tile t] at width k_t: lane partials by fma from +0, then the xor butterfly ("SDDMM" above).  No lane partial is
 *           carried from one tile into the next tile's butterfly.  At k <= 64 the bits are the narrow call's.  16-bit operands
 *           are widened exactly; out is fp32.  out is written once per nonzero and never read; vals is never read; nothing
 *           depends on any ld, on the row's length or pieces, on other rows or on the handle.
 * The plan: spmv_csr_spmm_plan_cols(h, k_max) does what spmv_csr_spmm_plan does and also allocates a scratch of its own for the
 * long rows' SpMM partials, pieces x ceil(k_max / 64) x 64 floats: a separate allocation, so the narrow calls' scratch and
 * spmv_csr_spmm_describe's line keep their size and text; spmv_csr_spmm_plan_bytes counts it once it exists.  It only grows,
 * waits for the stream before it replaces an allocation, and a repeated call changes nothing.  Both _cols calls need it to
 * cover k, else SPMV_ERR_NOT_PLANNED: one rule at every width, also on a handle without a long row.  After the plan the two
 * calls allocate nothing and never wait: graph-capturable.  Runs of spmv_csr_spmm_cols on one handle must be stream-ordered.
 * Limits: 1 <= k, k_max <= SPMV_COLS_MAX_K; every ld >= k; rows x 16 lanes x m tiles < 2^32 work-items for SpMM (one launch
 * carries all tiles), rows x 16 lanes < 2^32 for SDDMM (the tiles are walked inside the kernel).
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, Y / out untouched): a dtype other than the
 * three, k or k_max out of range, an ld below k, a matrix not aligned for its dtype, d_out not 4-byte aligned, a missing
 * pointer (with the narrow calls' exceptions for empty dimensions), a null handle, another current device. */
#define SPMV_COLS_MAX_K 65536
SPMV_API int spmv_csr_spmm_plan_cols(spmv_csr_t *h, int k_max, void *stream);
SPMV_API int spmv_csr_spmm_cols(spmv_csr_t *h, int dtype, int k, const void *d_X, int64_t ldx, void *d_Y, int64_t ldy, void *stream);
SPMV_API int spmv_csr_sddmm_cols(spmv_csr_t *h, int dtype, int k, const void *d_U, int64_t ldu, const void *d_X, int64_t ldx,
                                 float *d_out, void *stream);

/* ---- Fused attention with an additive bias per nonzero, and the bias's gradient: all three passes ---------------------------
 * O = softmax_rows(scale * Q K^T + B at the pattern) V with one fp32 number per (query, key) pair of the pattern: a
 * relative-position table, ALiBi slopes, edge features, a soft mask, or -Inf to switch a listed key off without rebuilding
 * the handle.  Only the most general form exists, as for _16: the arguments are the _16 call's with the bias arguments after
 * dtype, and dtype also takes SPMV_ATTN_FP32 = 0 (fp32 matrices, the _gqa call's units and alignment; the _16 calls go on
 * refusing 0).
 * The bias.  d_bias holds nnz floats per query head in the storage order of the handle it is passed with: position n
 * belongs to col_idx[n]; on a row block with a rebased row_ptr, n is the position in that handle's col_idx.  It is fp32
 * whatever dtype is, and an array of its own: the handle's vals is still never read.  bias_stride counts floats from query
 * head y to y + 1; 0 means one bias for all heads.  The bias belongs to the QUERY head: within a group each query head uses
 * its own in backward_kv too.  backward_kv runs on the transposed handle and takes d_bias_t, the bias in t's storage order
 * (bias_t[i] = bias[map[i]]): spmv_csr_transpose_gather makes it, for all heads in one call.
 * The score (part of the interface).  The score of nonzero n is  t = fl(fl(scale * s) + bias[n]):  s is spmv_csr_sddmm's
 * number, unchanged; the product is rounded first, then one fp32 addition is made (not an fma).  Everything after t is the
 * documented order of "Fused attention", word for word, in all three passes: the online softmax, stats = (M, 1/l),
 * p = expf(t - M_i) * r_i, delta, the chains and the pieces.  Both backward passes recompute t with the bias, so the three
 * passes agree on every p.  Consequences:
 *   - a bias of -0.0f everywhere gives, bit for bit, what the matching _gqa call (dtype 0) or _16 call gives: x + (-0) = x
 *     for every x, -0 included;
 *   - a bias of -Inf beside a finite maximum removes the nonzero exactly (e = +0, p = +0);
 *   - a NaN or +Inf bias, or a row whose every t is -Inf, behaves as the same t does without a bias: a NaN row.
 * The gradient.  dBias[n] = fl(p * fl(dp - delta_i)): the two inner roundings of ds, and ds = fl(scale * dBias[n]) keeps its
 * bits.  backward_q writes it on the pattern handle, in storage order, per query head at y * dbias_stride (always per head:
 * a caller who shares one bias sums dBias over the heads, as _heads callers do for a shared K and V).  Every position of
 * [0, nnz) is written exactly once, positions of rows in pieces and positions whose p is 0 (they hold +-0) included; no
 * atomics.  d_dbias may be NULL: nothing is written, dQ and delta are the same bits.  dbias_stride must be >= nnz when
 * heads > 1 and needs to be a multiple of nothing.
 * The plan, the scratch, _plan_heads, _max_heads and SPMV_ERR_NOT_PLANNED are the unbiased calls'; after the plan the calls
 * allocate nothing and never wait: graph-capturable.  Of nnz size a pass reads col_idx and the bias (8 bytes per nonzero
 * and head; backward_q with dBias 12).
 * Refusals (SPMV_ERR_INVALID, a message that names the function, nothing launched, every output untouched), after the
 * header of hs and the group and before the rest: a dtype outside {0, 1, 2}; a null d_bias while nnz > 0; a bias or dBias
 * pointer that is not 4-byte aligned; a negative stride; dbias_stride < nnz with heads > 1 and a non-null d_dbias; then
 * everything the _gqa call (dtype 0) or the _16 call of that dtype refuses. */
enum { SPMV_ATTN_FP32 = 0 };
SPMV_API int spmv_csr_attention_forward_bias(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias,
                                             int64_t bias_stride, float scale, int k, const void *d_Q, int64_t ldq,
                                             const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv, void *d_O,
                                             int64_t ldo, float *d_stats, void *stream);
SPMV_API int spmv_csr_attention_backward_q_bias(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype,
                                                const float *d_bias, int64_t bias_stride, float *d_dbias, int64_t dbias_stride,
                                                float scale, int k, const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk,
                                                int kv, const void *d_V, int64_t ldv, const void *d_O, int64_t ldo,
                                                const void *d_dO, int64_t lddo, const float *d_stats, float *d_delta,
                                                void *d_dQ, int64_t lddq, void *stream);
SPMV_API int spmv_csr_attention_backward_kv_bias(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, int dtype,
                                                 const float *d_bias_t, int64_t bias_stride, float scale, int k, const void *d_Q,
                                                 int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv,
                                                 const void *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                                 void *d_dK, int64_t lddk, void *d_dV, int64_t lddv, void *stream);

/* ---- Fused attention at head widths up to 128: the most general calls once more, on lane groups of 32 -----------------------
 * The three passes take exactly the argument lists of the _bias calls.  What differs from _bias, and nothing else:
 *   - 1 <= k <= 128 and 1 <= kv <= 128;
 *   - d_bias (d_bias_t) may be NULL: no bias, and the unbiased kernels run.  A non-null d_dbias with a null d_bias is refused;
 *   - dtype is SPMV_ATTN_FP32, SPMV_ATTN_BF16 or SPMV_ATTN_FP16 as for _bias;
 *   - the calls need spmv_csr_attention_plan_wide(h, heads) to cover hs->heads, else SPMV_ERR_NOT_PLANNED: one rule at every
 *     width, which also holds on a handle without a long row.
 * spmv_csr_attention_plan_wide does what spmv_csr_attention_plan_heads(h, heads) does and allocates a scratch of its own for
 * the long rows' pieces at widths above 64: per head and piece 4 + 2 * 128 = 260 floats (m_p, l_p and, from a 16-byte
 * boundary, two sets of 128 partial sums: backward_kv's dK_p and dV_p).  It is a separate allocation: the scratch of the other
 * calls keeps its size and layout, and spmv_csr_attention_plan_bytes counts the wide scratch only once _plan_wide has been
 * called.  It only grows, waits for the stream before it replaces a scratch, and a repeated call changes nothing.
 * spmv_csr_attention_max_heads_wide applies the launch limit of spmv_csr_attention_max_heads (rows x lanes per row x heads <
 * 2^32 on the row blocks and on the blocks of the pieces, heads <= 65535) with 32 lanes per row where max(k, kv) > 64; up to
 * 64 it returns what spmv_csr_attention_max_heads returns.
 * Refusals come in the _bias call's order with the width range replaced; the message names the _wide function; nothing is
 * launched and every output stays untouched.  After the plan the calls allocate nothing and never wait: graph-capturable.
 *
 * The contract (part of the interface).
 * max(k, kv) <= 64: the call launches the very kernels the _bias call launches (bias non-null), or the _gqa (dtype 0) or _16
 *   call's (bias null): it is that call bit for bit.
 * max(k, kv) > 64: a group of V = 32 lanes owns a row or a piece, and lane s owns columns [4s, 4s + 4) as everywhere else.
 *   The documented order of "Fused attention" (and of csrc/lane_group.hpp) holds word for word with V = 32: lane partials by
 *   fma from +0 over the lane's columns below the width, then the xor butterfly over the levels m = 16, 8, 4, 2, 1;
 *   t = fl(fl(scale * s) + bias) when there is a bias; the online softmax rescaled once per step; stats = (M, 1/l); p, ds and
 *   dBias with their three roundings; the chains in storage order from +0, the pieces in piece order, the GQA fold from head
 *   0's value.
 *   The step is T_wide = SPMV_ATTN_WIDE_STEP = 8 nonzeros (stated because the forward bits depend on it: one rescale per
 *   step): 64 registers of gathered fp32 slices per lane, the register picture of the V = 8 kernels; a step of 32 would need
 *   256.  A step is thus narrower than its group: lanes 0 .. 7 of the group each own one nonzero of the step (its column
 *   index, its bias, its stats and delta, its expf, its dBias).
 *   16-bit: the contract of the _16 calls carries over unchanged.  A 16-bit wide call is the fp32 wide call on the widened
 *   operands, each output rounded once, to nearest even, at the store; a lane still holds 4 elements per slice.
 *   SDDMM: above width 64 there is no spmv_csr_sddmm for a score to be equal to (its k ends at 64); the score is the dot
 *   product in the order just stated.
 * Zero padding (what ties the geometry of 32 lanes to the others).  Pad every operand with zero columns from (k, kv) <= 64 up
 *   to (128, 128).  On caller-made stats (and, in backward_kv, delta) the wide call's scores, dp, delta, ds, dBias,
 *   dQ[:, :k], dK[:, :k] and dV[:, :kv] are then bit for bit the narrow call's on the unpadded operands, and the padded
 *   output columns are +0: the extra lanes hold +0, a partial is never -0, and the extra levels run first.  The forward pass
 *   shares this only on data whose every expf argument is +-0, at most -128 or -Inf: T differs between the two geometries and
 *   the rescale is per step, so on general data O and stats agree to rounding, not bit for bit. */
#define SPMV_ATTN_WIDE_STEP 8
SPMV_API int spmv_csr_attention_plan_wide(spmv_csr_t *h, int heads, void *stream);
SPMV_API int spmv_csr_attention_max_heads_wide(const spmv_csr_t *h, int k, int kv);
SPMV_API int spmv_csr_attention_forward_wide(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype, const float *d_bias,
                                             int64_t bias_stride, float scale, int k, const void *d_Q, int64_t ldq,
                                             const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv, void *d_O,
                                             int64_t ldo, float *d_stats, void *stream);
SPMV_API int spmv_csr_attention_backward_q_wide(spmv_csr_t *h, const spmv_attn_heads_t *hs, int group, int dtype,
                                                const float *d_bias, int64_t bias_stride, float *d_dbias, int64_t dbias_stride,
                                                float scale, int k, const void *d_Q, int64_t ldq, const void *d_K, int64_t ldk,
                                                int kv, const void *d_V, int64_t ldv, const void *d_O, int64_t ldo,
                                                const void *d_dO, int64_t lddo, const float *d_stats, float *d_delta,
                                                void *d_dQ, int64_t lddq, void *stream);
SPMV_API int spmv_csr_attention_backward_kv_wide(spmv_csr_t *t, const spmv_attn_heads_t *hs, int group, int dtype,
                                                 const float *d_bias_t, int64_t bias_stride, float scale, int k, const void *d_Q,
                                                 int64_t ldq, const void *d_K, int64_t ldk, int kv, const void *d_V, int64_t ldv,
                                                 const void *d_dO, int64_t lddo, const float *d_stats, const float *d_delta,
                                                 void *d_dK, int64_t lddk, void *d_dV, int64_t lddv, void *stream);

/* ---- dense baselines (reference slots cublas / naive / tiling) ---------
 * y[i] = sum_j x[j] * A[j*N+i] on the dense device matrix.
 * replaces: cublas_gemv_gpu (cublas.cu:4-44), naive_kernel (naive.cu:4-11),
 * tiling_kernel (tiling_smem.cu:4-32).  mode 0 = thread per output (naive),
 * 1 = LDS-staged x tile (tiling), 2 = split-M wave-coalesced (vendor slot),
 * 3 = mode 2 + activation sparsity: rows of A whose x[j] is 0 are not read
 *     (asp_kernel_v0/1/2, src/kernels/asp.cu:20-26). */
SPMV_API int spmv_dense_gemv(int M, int N, const float *d_A, const float *d_x, float *d_y, int mode,
                    void *stream);

/* Modes 2 and 3 split M over 64 row slabs and need 64*N floats for the per-slab partial sums.
 * spmv_dense_gemv_ws takes that workspace from the caller (spmv_dense_gemv_workspace_bytes says how much; 0 for
 * modes 0/1): no allocation, no host wait, graph-capturable.  spmv_dense_gemv without the argument uses a
 * buffer the library keeps per device and hands from call to call in stream order (asynchronous too; it waits on
 * the host only when the buffer has to grow). */
SPMV_API int64_t spmv_dense_gemv_workspace_bytes(int N, int mode);
SPMV_API int spmv_dense_gemv_ws(int M, int N, const float *d_A, const float *d_x, float *d_y, int mode,
                                void *d_workspace, int64_t workspace_bytes, void *stream);

/* Host-buffer form of the same (upload A and x, run, download y). */
SPMV_API int spmv_dense_gemv_host(int M, int N, const float *A_host, const float *x_host, float *y_host,
                                  int mode, float *kernel_ms);

/* ---- the reference's ASP layout (the uncompressed one of its activation-sparsity launcher) -----
 * replaces: ASPMatrix (src/asp.cpp:3-14, src/include/asp.hpp) and the read pattern of asp_kernel_v0/1/2
 * (src/kernels/asp.cu:6-211).  spmv_asp_retile: d_A[M][N] row-major -> d_asp (M*N floats), the same array bit for
 * bit: 32 x 32 blocks, column panel by column panel (asp[(bn/32 * M + j) * 32 + c] = A[j*N + bn + c]); M and N
 * multiples of 32 (tester.cpp:10-11).  spmv_asp_gemv_ws: y = A^T x from that layout, a row of a panel skipped
 * when its x is zero (asp.cu:20-26); workspace as for spmv_dense_gemv_ws mode 3; asynchronous, no allocation.
 * (asp_gemv_gpu of include/kernel.hpp runs dense mode 3 on the row-major matrix -- the same skip without the copy.) */
SPMV_API int spmv_asp_retile(int M, int N, const float *d_A, float *d_asp, void *stream);
SPMV_API int spmv_asp_gemv_ws(int M, int N, const float *d_asp, const float *d_x, float *d_y, void *d_workspace,
                              int64_t workspace_bytes, void *stream);

/* ---- the reference's tiled bitmap-CSR format (dense-ish matrices, density > 1/32) -----
 * replaces: TCSRMatrix (src/tcsr.cpp:5-38, src/include/tcsr.hpp:4-23) and csr_tiling_kernel
 * with its launcher (src/kernels/csr_tiling.cu:24-166).  Same arrays, bit for bit: blk_idx
 * (exclusive nonzero prefix per 32x32 block + sentinel), bitmaps (word = output column inside
 * the block, bit = input row), vals (unpadded, bitmap order).  M and N must be multiples of 32
 * (the reference asserts it, src/tester.cpp:9-10); anything else is SPMV_ERR_INVALID.
 * Built on the device from the dense matrix; y[i] = sum_j x[j]*A[j*N+i] as everywhere. */
typedef struct spmv_tcsr spmv_tcsr_t;
SPMV_API int spmv_tcsr_from_dense_host(int M, int N, const float *A_host, void *stream, spmv_tcsr_t **out);
SPMV_API int spmv_tcsr_from_dense_device(int M, int N, const float *d_A, void *stream, spmv_tcsr_t **out);
SPMV_API int spmv_tcsr_sizes(const spmv_tcsr_t *h, int64_t *n_blk_idx, int64_t *n_bitmaps, int64_t *n_vals);
SPMV_API int spmv_tcsr_download(const spmv_tcsr_t *h, int32_t *blk_idx, uint32_t *bitmaps, float *vals);
SPMV_API int spmv_tcsr_run(const spmv_tcsr_t *h, const float *d_x, float *d_y, void *stream);
SPMV_API int spmv_tcsr_run_host(const spmv_tcsr_t *h, const float *x_host, float *y_host, float *kernel_ms);
SPMV_API int spmv_tcsr_destroy(spmv_tcsr_t *h);

/* ---- the reference's bitmap formats of its wsp / awsp / awsp_ref launchers (density > 1/32) -------------------
 * replaces: WSPMatrix (src/wsp.cpp:3-40) + wsp_kernel_v0/v1 (src/kernels/wsp.cu:4-138),
 *           AWSPMatrix (src/awsp.cpp:3-49) + awsp_kernel_v0/1/2 (src/kernels/awsp.cu:5-317),
 *           AWSPRefMatrix (src/awsp_ref.cpp:4-58) + awsp_ref_kernel / wsp_sm_kernel (awsp_ref.cu:6-185, wsp_sm.cu:6-211).
 * The arrays are the reference's, bit for bit (built on the device from the dense matrix); the multiply is re-derived
 * for 64-lane wavefronts (64-bit word pairs, __popcll ranks, running value offsets, the reference's x == 0 skip).
 * M and N must be multiples of 32.  stats[4] = what the reference classes expose: WSP {nz_max_m, nz_max_n, 0, 0},
 * AWSP {nz_bk_max_, 0, 0, 0}, AWSPRef warp_nz_offset_[0..3]. */
enum spmv_bitmap_format { SPMV_FMT_WSP = 0, SPMV_FMT_AWSP = 1, SPMV_FMT_AWSP_REF = 2, SPMV_FMT_COUNT = 3 };
typedef struct spmv_bitmap spmv_bitmap_t;
SPMV_API int spmv_bitmap_from_dense_host(int format, int M, int N, const float *A_host, void *stream, spmv_bitmap_t **out);
SPMV_API int spmv_bitmap_from_dense_device(int format, int M, int N, const float *d_A, void *stream, spmv_bitmap_t **out);
SPMV_API int spmv_bitmap_sizes(const spmv_bitmap_t *h, int64_t *n_bitmaps, int64_t *n_vals, int32_t stats[4]);
SPMV_API int spmv_bitmap_download(const spmv_bitmap_t *h, uint32_t *bitmaps, float *vals);
SPMV_API int spmv_bitmap_run(const spmv_bitmap_t *h, const float *d_x, float *d_y, void *stream);
SPMV_API int spmv_bitmap_run_host(const spmv_bitmap_t *h, const float *x_host, float *y_host, float *kernel_ms);
SPMV_API int spmv_bitmap_destroy(spmv_bitmap_t *h);

/* ---- synthetic CSR of stated (rows, cols, nnz) ---------------------------
 * Counter-based generator (DESIGN.md "Synthetic workloads"): element k of
 * global row r is a pure function of (seed, r, k, row length, band), so the
 * host can regenerate any row.  d_row_ptr (n_local+1 entries, rebased to 0)
 * gives the lengths of global rows [row0, row0+n_local).  band = 0: columns
 * uniform over [0, cols); band > 0: inside a diagonal band of that width. */
SPMV_API int spmv_synth_fill(uint64_t seed, int64_t row0, int64_t n_local, int64_t rows, int64_t cols,
                    int64_t band, const int32_t *d_row_ptr, int32_t *d_col_idx, float *d_vals,
                    void *stream);
SPMV_API int spmv_synth_x(uint64_t seed, int64_t j0, int64_t n, float *d_x, void *stream);

/* ---- measurement aids: kernels of KNOWN traffic + a marker dispatch ------------------------------------------
 * The metric of this path is rocprofv3's FETCH_SIZE / WRITE_SIZE over the kernel time (role of the reference's
 * profile.sh:18-20, a profiler around the executable).  The counters are uncalibrated outside 16-byte streams on
 * gfx950, so a profiled process launches these beside the SpMV kernels and corrects per access class
 * (bench.py --traffic-child; tools/summarize_profile.py).  spmv_calib_stream reads exactly `bytes` (a multiple of 16,
 * buffer 16-byte aligned) with 16-byte loads.  spmv_calib_gather reads n_lines DISTINCT 128-byte lines of a table of
 * table_lines lines (a power of two; 128 bytes each), one lane per line, neighbouring lanes far apart; touch = 1: one
 * word per line, 2: one word in each 64-byte half, 4: one word in each 32-byte sector.  spmv_calib_marker launches an
 * empty kernel (spmv::k_marker) of `id` workgroups of 64 threads: a cut mark in a per-dispatch counter file.
 * d_sink: one float the kernels never write in practice. */
SPMV_API int spmv_calib_stream(const void *d_src, int64_t bytes, float *d_sink, void *stream);
SPMV_API int spmv_calib_gather(const float *d_table, int64_t table_lines, int64_t n_lines, int touch, float *d_sink,
                               void *stream);
SPMV_API int spmv_calib_store(float *d_dst, int64_t bytes, int width, void *stream);
SPMV_API int spmv_calib_marker(int id, void *stream);

/* ---- TEST ONLY: the bounds-checked build ---------------------------------------------------------------------
 * lib/libspmv_hip_checked.so is this library compiled with SPMV_CHECK_BOUNDS: the streams of the panel family that
 * read or write past a tile's or a bin's end check every access against the array's allocation, record a violation
 * instead of issuing the access, and go on.  spmv_debug_bounds waits for the current device, writes up to n records
 * {site, violations, largest overrun in bytes} (three int64 each) of the sites that recorded any since the last call,
 * clears the tables and returns how many sites did (>= 0; may exceed n).  Site numbers: csrc/spmv_internal.hpp
 * BoundsSite.  The normal library returns SPMV_ERR_INVALID ("not instrumented"). */
SPMV_API int spmv_debug_bounds(int64_t *records, int n);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_HIP_H */
