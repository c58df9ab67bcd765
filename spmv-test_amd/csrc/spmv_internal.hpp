// spmv_internal.hpp -- shared declarations of libspmv_hip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <utility>
#include "spmv_hip.h"
#include "attention_args.hpp"

namespace spmv {

// ---- error plumbing -------------------------------------------------------
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define SPMV_HIP_TRY(call)                                                   \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return ::spmv::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

static inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what, __FILE__, __LINE__);
    return SPMV_OK;
}

// after a kernel launch in a function that returns an SPMV_* code: leaves with the launch's error, if any
#define SPMV_LAUNCHED(name)                                                                                     \
    if (hipError_t e__ = hipGetLastError(); e__ != hipSuccess) return ::spmv::hip_fail(e__, name, __FILE__, __LINE__)

// The one owner of a device array: move-only, freed when it is destroyed, reset() or assigned over.  Reads convert it to
// T * (kernel arguments, offsets, null tests); it is written only by alloc(), a move or reset(), never from a raw pointer.
// Not for anything of static storage duration: its destructor would call hipFree after the HIP runtime may be gone.
template <typename T>
class DevPtr {
    T *p_ = nullptr;
public:
    DevPtr() = default;
    DevPtr(DevPtr &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevPtr &operator=(DevPtr &&o) noexcept
    {
        T *q = o.p_;
        o.p_ = nullptr;
        (void)reset();
        p_ = q;
        return *this;
    }
    ~DevPtr() { (void)reset(); }
    DevPtr *operator&() = delete;   // no hipMalloc((void **)&d, ...) into it
    hipError_t alloc(size_t count)   // at least one element, so that an empty array is not null
    {
        (void)reset();
        return hipMalloc((void **)&p_, sizeof(T) * (count ? count : 1));
    }
    hipError_t reset()
    {
        T *q = p_;
        p_ = nullptr;
        return q ? hipFree(q) : hipSuccess;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): a function-local static of this type
// remembers the devices a kernel has been opted in on (one bit per device id; ids >= 64 set it on every launch).
struct LdsOptIn {
    std::atomic<uint64_t> done{0};
    int ensure(const void *fn, int device, int bytes);
};
int device_cus(int device);   // compute units of a device (cached per device id; 256 if the query fails)
// SPMV_OK when `device` (where a handle's arrays live) is the calling thread's current device
int require_current(int device, const char *what);

// ---- geometry constants ----------------------------------------------------
constexpr int kWave = 64;          // gfx950 wavefront
constexpr int kBlock = 256;        // 4 waves: one per SIMD of a CU
constexpr int kXcds = 8;           // MI355X: 8 XCDs, blocks dealt round-robin over them
constexpr int kMaxHeads = 65535;   // heads of one spmv_csr_attention_*_heads launch: a grid's y extent

// ADAPTIVE / TILED chunking: every lane streams kNnzPerThread consecutive-by-4 nonzeros
// (col_idx + vals = 8 B each) with 16-byte loads; a workgroup of B threads owns B*16 nonzeros.
// (the SPMV_T_* macros exist for A/B builds, tools/explore.py; the shipped values are the defaults)
#ifndef SPMV_T_NPT
#define SPMV_T_NPT 16
#endif
#ifndef SPMV_T_SHORT
#define SPMV_T_SHORT 32
#endif
constexpr int kNnzPerThread = SPMV_T_NPT;
constexpr int kShortSeg = SPMV_T_SHORT;            // row segments up to this long: one lane sums them

// Chunk boundaries (and, for TILED, column windows) for workgroups of `block` threads.
struct ChunkPlan {
    int block = 0;             // 0 = not planned; 256 | 512 | 1024 threads per workgroup
    int nchunks = 0;           // ceil(nnz / (block*16))
    DevPtr<int32_t> d_lb;      // [nchunks+1] first row whose row_ptr >= c*chunk
    DevPtr<float> d_carry;     // [nchunks]   partial sum of the row continued from chunk c-1
    DevPtr<int32_t> d_win;     // [2*nchunks+2] TILED: first column, window length (0 = not staged); stats
    // 16-bit columns (TILED): chunks whose span is fully staged also carry col - w0 as uint16
    DevPtr<uint16_t> d_col16;      // [nchunks * chunk], lane layout of k_tiled16
    DevPtr<int32_t> d_list16;      // [n16] chunks run by k_tiled16
    DevPtr<int32_t> d_list32;      // [nchunks - n16 - nsorted] the others, run by the 32-bit body
    int n16 = 0;
    // sorted chunks (TILED): spans of several LDS regions gather x in column order instead of staging it
    DevPtr<uint32_t> d_perm;           // [nsorted * chunk] position << 18 | column - w0 of the sorted chunks (list order), read INSTEAD of col_idx
    DevPtr<int32_t> d_list_sorted;     // [nsorted]
    DevPtr<int32_t> d_sorted_slot;     // [nchunks] identity order: sorted chunks before chunk c = the slot of a sorted c in d_perm
    bool identity_order = false;       // the mixed launch takes its chunks in identity order and has no lists (tiled_chunks.hpp)
    int nsorted = 0;                   // chunks run by the sorted body
    int nsorted_marked = 0;            // chunks the window pass marked (a few may still switch to a block list)
    int sorted_from = 0;               // -1: sorted where the modelled cost is lower; 0: never; n: from n passes on
    int long_piece_chunks = 0;         // chunks of three passes or more that hold a piece of a long row (> 512 nonzeros)
    double model_cost = 0.0;           // modelled time per nonzero of this plan (PlanCost units; compares block sizes)
    DevPtr<int32_t> d_blk;         // [64 * nchunks] ids of the staged 1024-column blocks of the chunks that use a list
    int nblk_chunks = 0;           // how many chunks do
    int maxpass = 0;
    bool col16_wanted = false;     // the plan asked for the 16-bit copy (it is kept only where enough chunks qualify)
    int spanning_rows = 0;         // rows that continue past their owner chunk (0: no fix-up launch)
    int region = 0;                // floats of the dynamic LDS region (x slice, then products)
    bool persist = false;      // persistent software-pipelined launch (measured slower: DESIGN.md section 4)
    int staged_single = 0;     // TILED: chunks whose whole column span is staged in one pass
    int staged_full = 0;       // TILED: chunks staged completely (any number of passes)
};

// Plans that COPY the values (PANEL, XSKIP) remember which state of vals they copied: the handle's generation counter
// (spmv_csr_values_changed bumps it) and, under SPMV_CHECK_VALUES=1, a checksum of the array itself.
struct ValuesStamp {
    uint64_t gen = 0;
    uint64_t sum = 0;
    bool have_sum = false;
};

// SPMV_PANEL is five layouts behind one variant number (params[6] of include/spmv_hip.h); each has a plan struct of its own.
enum class PanelLayout { none = 0, sweep_l2 = 1, sweep_lds = 2, sorted_blocks = 3, binned = 4, binned_scattered = 5 };
// the sweep (modes 1 and 2, kernels_panel.hip): row blocks of at most 8192 rows and equal nonzero counts, each block's nonzeros stably sorted by column panel.
struct SweepPlan {
    bool lds = false;              // panels of 2^14 columns staged in LDS by 16-wavefront workgroups (small x) instead of gathered through L2
    int pw_bits = 0, npanels = 0;  // log2(columns per panel), panels
    int nblocks = 0;               // row blocks (<= 8192 rows, equal nonzero counts) = wavefronts of work
    int waves_per_launch = 0;      // what is resident at once: one launch = one sweep in step
    int step_vecs = 8;             // 16-byte vectors per lane and step of the sweep (8 | 4: thin tiles, kernels_panel.hip kVecMax)
    DevPtr<uint32_t> d_packed;     // [nnz + slack] row_in_block << 18 | join << 17 | column_in_panel (kernels_panel.hip)
    DevPtr<float> d_pvals;         // [nnz + slack] values in the same order (a COPY: re-plan after changing vals)
    DevPtr<int32_t> d_tile_ptr;    // [nblocks * (npanels + 1)]
    DevPtr<int32_t> d_brow;        // [nblocks + 1] first row of every block
};
// sorted blocks (mode 3, kernels_colsort.hip): blocks of <= 4096 rows streamed in column order, d_packed / d_pvals (a COPY of vals) in
// units of 256 slots (four groups of 64 nonzeros with distinct rows)
struct SortedBlocksPlan {
    int nblocks = 0, sb_rows = 0, sb_waves = 0;   // blocks, rows per block (4096 | 8192), wavefronts per workgroup (8 | 4)
    DevPtr<uint32_t> d_packed;     // [units * 256] row_in_block << colbits | column - ubase[unit]
    DevPtr<float> d_pvals;         // [units * 256]
    DevPtr<int32_t> d_brow;        // [nblocks + 1] first row of every block
    DevPtr<int32_t> d_ubeg;        // [nblocks + 1] first unit of every block
    DevPtr<int32_t> d_usimple;     // [nblocks] leading units of the block that hold groups (64 distinct rows per instruction)
    DevPtr<int32_t> d_uend;        // [nblocks] one past the last unit the block uses (groups, then its row-sorted tail)
    DevPtr<int32_t> d_ubase;       // [units] first column of every unit (packed holds offsets from it)
    DevPtr<int32_t> d_tbeg;        // [nblocks] first tail unit of the block in d_trow
    DevPtr<uint16_t> d_trow;       // [tail_units * 256] rows of the tail units (their packed words are whole columns)
    int64_t units = 0, tail_units = 0;
    int64_t wide_blocks = 0;       // blocks whose short rows span more than 32768 lines of x (4 MiB)
    int64_t lines = 0;             // occupied 128-byte lines of x, summed over the blocks (plan statistic)
    int64_t tail = 0;              // nonzeros in the tails (long rows, what could not be grouped)
};
// binned (mode 4, kernels_binned.hip): the nonzeros twice over -- in PANEL-major order (d_c16 + d_pvals: what the
// product launch streams, its panel of x in LDS) and in BIN-major order (d_r16: what the sum launch streams beside the
// products); tile (bin b, panel p) is contiguous in both, rows ascending inside it
struct BinnedPlan {
    int bin_rows = 0;              // most rows of a bin (4096 | 8192): a wavefront's private sums in LDS
    int npanels = 0, nblocks = 0;  // panels of 2^15 columns, bins
    int splits = 1;                // workgroups per panel of the product launch
    bool wide_pieces = false;      // the sum launch takes four products per lane (fat tiles) instead of two
    int64_t padded = 0;            // entries of the panel-major arrays
    DevPtr<uint16_t> d_c16;        // [padded] column - panel * 2^15, panel-major (every panel padded to a multiple of 8)
    DevPtr<float> d_pvals;         // [padded] values in the same order (a COPY: re-plan after changing vals)
    DevPtr<float> d_prod;          // [padded] scratch of a run: the products, panel-major
    DevPtr<uint16_t> d_r16;        // [nnz] row - brow[bin], bin-major (d_tile_ptr positions)
    DevPtr<int32_t> d_pm;          // [nblocks * npanels] panel-major position of tile (b, p)
    DevPtr<int32_t> d_pbase;       // [npanels + 1] panel-major position of every panel's first entry
    DevPtr<int32_t> d_tile_ptr;    // [nblocks * (npanels + 1)]
    DevPtr<int32_t> d_brow;        // [nblocks + 1] first row of every bin
    int flagged_tiles = 0;         // tiles that go through the fold (bins whose long rows need more spare sums than there are)
    int long_rows = 0;             // rows with spare sums (more products in some tile than a lane takes)
    DevPtr<int32_t> d_lptr;        // [nblocks + 1] first long row of every bin in d_lrow / d_lcnt
    DevPtr<uint32_t> d_lrow;       // [long_rows] row in bin << 16 | first spare slot
    DevPtr<int32_t> d_lcnt;        // [long_rows] spare slots of the row
};
// ... its scattered flavour (mode 5): the product launch stores in bin order (d_offset, d_first_run; bit 15 of d_c16), the sum launch
// streams d_prod + d_acc16 bin by bin.  bin_rows (4096 | 8192 | 16384) ... d_brow: as in BinnedPlan, the panels padded to multiples of 512
struct ScatteredPlan {
    int bin_rows = 0, npanels = 0, nblocks = 0, splits = 1;
    int64_t padded = 0;
    DevPtr<uint16_t> d_c16;
    DevPtr<float> d_pvals;
    DevPtr<int32_t> d_pbase, d_brow;
    DevPtr<float> d_prod;          // [bm_alloc] scratch of a run: the products, bin-major
    DevPtr<int32_t> d_offset;      // [runs] bin-major minus panel-major position of a run (a nonempty tile, or a panel's pad slots)
    DevPtr<int32_t> d_first_run;   // [padded / 512] run of every 512-entry block's first entry (minus one where it starts a run)
    int64_t runs = 0;
    DevPtr<int32_t> d_bbase;       // [nblocks + 1] first entry of every bin in d_prod / d_acc16 (multiples of 256)
    DevPtr<int32_t> d_bcnt;        // [nblocks] entries of the bin
    DevPtr<int32_t> d_nlong;       // [nblocks] rows with spare accumulators (-1: the bin adds with LDS atomics)
    int64_t bm_entries = 0;        // entries of the bin-major arrays
    int64_t bm_alloc = 0;          // ... as allocated: bm_entries + the slack of the sum launch's read-ahead (kernels_binned.hip kBsSlack)
    DevPtr<uint16_t> d_acc16;      // [bm_alloc] accumulator number of every product, bin-major
    DevPtr<uint32_t> d_pool_rows;  // [nblocks * 1024] row << 17 | first spare accumulator << 7 | how many
    int flagged_bins = 0;          // bins that ran out of spare accumulators (they add with LDS atomics)
    int long_rows = 0;             // rows with spare accumulators
};
// One of the handle's two SPMV_PANEL slots: `layout` says which ONE of the four members is populated (none: not planned).
struct PanelPlan {
    PanelLayout layout = PanelLayout::none;
    ValuesStamp stamp;             // which state of vals the layout's d_pvals is a copy of
    SweepPlan sweep; SortedBlocksPlan sorted; BinnedPlan binned; ScatteredPlan scattered;
};

// SPMV_XSKIP (kernels_xskip.hip): the matrix in input-major segments per block of 1024 outputs
struct XskipPlan {
    bool ready = false;
    int nblocks = 0, nseg = 0, slabs = 0;
    DevPtr<int32_t> d_block_seg;      // [nblocks+1] first segment of every output block
    DevPtr<int32_t> d_seg_input;      // [nseg+1] input (column) of a segment
    DevPtr<int32_t> d_seg_ptr;        // [nseg+1] first entry of a segment
    DevPtr<uint16_t> d_erow;          // [nnz] output - 1024 * block
    DevPtr<float> d_evals;            // [nnz] values in segment order (a COPY: re-plan after changing vals)
    DevPtr<float> d_part;             // [nblocks * slabs * 1024] slab partials (slabs > 1)
    ValuesStamp stamp;                // which state of vals d_evals is a copy of
};

// SPMV_WAVE_PIPE (kernels_rows.hip): the rows too long for a wavefront's bundle, cut into pieces for the whole chip
struct WavePlan {
    bool ready = false;
    int n_long = 0, pieces = 0;
    DevPtr<int32_t> d_long_row;       // [n_long] the rows, ascending
    DevPtr<int32_t> d_long_first;     // [n_long + 1] first piece of every row
    DevPtr<int32_t> d_piece_k0;       // [pieces] first nonzero of a piece
    DevPtr<int32_t> d_piece_len;      // [pieces] its length (<= 1024)
    DevPtr<float> d_partial;          // [pieces] scratch of a run: the pieces' sums
    int block_rows = 512;             // rows of a bundle workgroup (512 | 1024)
    DevPtr<int32_t> d_blk_lo;         // [blocks] first entry of the x window of every block of block_rows rows, -1: none
    DevPtr<uint16_t> d_col16;         // [nnz] 16-bit column offsets: from blk_lo for windowed blocks' short rows, from piece_base for pieces (null: not built)
    DevPtr<int32_t> d_piece_base;     // [pieces] smallest column of a piece whose offsets are in d_col16, -1: 32-bit columns
    bool windows = false;             // the bundle kernel stages windows (at least half of the blocks have one)
    int64_t blocks = 0, win_blocks = 0;   // blocks of block_rows rows, and how many have a window
};

// spmv_csr_spmm (kernels_spmm.hip), spmv_csr_sddmm (kernels_sddmm.hip) and spmv_csr_row_softmax (kernels_softmax.hip): the
// rows too long for one lane group, cut into pieces at plan-fixed boundaries
struct SpmmPlan {
    bool ready = false;
    int n_long = 0, pieces = 0;
    int row_cap = 0, piece_len = 0;   // rows of more than row_cap nonzeros go in pieces of piece_len
    DevPtr<int32_t> d_order;          // [rows] the rows in the order the row kernel takes them (by length per 4096 rows)
    DevPtr<int32_t> d_long_row;       // [n_long] the rows, ascending
    DevPtr<int32_t> d_long_first;     // [n_long + 1] first piece of every row
    DevPtr<int32_t> d_piece_k0;       // [pieces] first nonzero of a piece
    DevPtr<int32_t> d_piece_len;      // [pieces] its length
    DevPtr<float> d_partial;          // [pieces * 64] scratch of a run: a piece's sums of up to 64 columns (SpMM), a piece's
                                      // maximum / sum / dot and its row's in slots 0 .. 3 (row softmax)
    int cols_k = 0;                   // the widest k the _cols calls may take (spmv_csr_spmm_plan_cols; 0: never called)
    DevPtr<float> d_partial_cols;     // [pieces * ceil(cols_k / 64) * 64] scratch of spmv_csr_spmm_cols: a piece's sums per column tile
};

// spmv_csr_attention_* (kernels_attention.hip): on the SpMM plan, plus the scratch of the long rows' pieces
struct AttnPlan {
    bool ready = false;
    int heads = 0;                    // heads one launch may carry (spmv_csr_attention_plan: 1; _plan_heads grows it)
    DevPtr<float> d_scratch;          // [heads * pieces * 132] per head and piece (m, l) and up to 128 partial sums (empty: no long row)
    int wide_heads = 0;               // heads the _wide calls may carry (spmv_csr_attention_plan_wide; 0: never called)
    DevPtr<float> d_scratch_wide;     // [wide_heads * pieces * 260] the same for widths above 64: (m, l) and up to 2 x 128 partial sums
};

// spmv_csr_spgemm(keep_plan = 1) (kernels_spgemm.hip): what the numeric pass needs to start without a host decision
struct SpgemmPlan {
    bool ready = false;
    int64_t inner = 0, a_nnz = 0, b_nnz = 0;   // a.cols = b.rows and the parents' nonzeros when the product was made
    int64_t cls[6] = {0, 0, 0, 0, 0, 0};       // cls[c] .. cls[c + 1]: the rows of class c in d_order (class 4: oversized)
    DevPtr<int32_t> d_order;                   // [cls[5]] the rows of a with at least one term, class by class, ascending inside
};

// spmv_csr_add(keep_plan = 1) (kernels_add.hip): the kept terms in c's order, what spmv_csr_add_values and _gather walk
struct AddPlan {
    bool ready = false;
    int op = 0;                                // SPMV_ADD_*
    int64_t a_nnz = 0, b_nnz = 0, terms = 0;   // the parents' nonzeros when the sum was made; the kept terms
    DevPtr<uint32_t> d_term;                   // [terms] side << 31 | storage position in that side, entry by entry, a's before b's
    DevPtr<int32_t> d_start;                   // [nnz + 1] the first term of every entry of c
};

// spmv_csr_trsv (kernels_trsv.hip): the rows of one triangle by level, and the launches of one solve
struct TrsvStep {
    int32_t first = 0, last = 0;               // the levels [first, last) of the launch
    bool merged = false;                       // one workgroup walks them (each of at most thin_rows rows); else first + 1 == last
};
struct TrsvPlan {
    bool ready = false;
    int64_t levels = 0, widest = 0, long_rows = 0, long_terms = 0;
    int64_t bad_diag_row = -1;                 // the first row whose diagonal is missing or repeated
    int thin = 0, cap = 0;                     // the thin threshold and the cap of levels per merged launch in force
    DevPtr<int32_t> d_order;                   // [rows] the rows by (level, row) ascending
    DevPtr<int32_t> d_level_ptr;               // [levels + 1] where every level starts in d_order
    DevPtr<int32_t> d_diag;                    // [rows] the storage position of the diagonal, -1: none
    DevPtr<int32_t> d_lstart;                  // [rows + 1] where a long row's terms start in d_lterm (a short row: none)
    DevPtr<uint32_t> d_lterm;                  // [long_terms] the storage positions of the long rows' terms, ascending per row
    int32_t *level_ptr = nullptr;              // [levels + 1] the host's copy (new[]; what the steps were formed from)
    TrsvStep *steps = nullptr;                 // [nsteps] (new[])
    int64_t nsteps = 0;
    TrsvPlan() = default;
    TrsvPlan(const TrsvPlan &) = delete;
    TrsvPlan &operator=(const TrsvPlan &) = delete;
    TrsvPlan &operator=(TrsvPlan &&o) noexcept
    {
        if (this == &o) return *this;
        delete[] level_ptr;
        delete[] steps;
        ready = o.ready; levels = o.levels; widest = o.widest; long_rows = o.long_rows; long_terms = o.long_terms;
        bad_diag_row = o.bad_diag_row; thin = o.thin; cap = o.cap;
        d_order = std::move(o.d_order); d_level_ptr = std::move(o.d_level_ptr); d_diag = std::move(o.d_diag);
        d_lstart = std::move(o.d_lstart); d_lterm = std::move(o.d_lterm);
        level_ptr = o.level_ptr; steps = o.steps; nsteps = o.nsteps;
        o.level_ptr = nullptr; o.steps = nullptr; o.nsteps = 0; o.ready = false;
        return *this;
    }
    ~TrsvPlan() { delete[] level_ptr; delete[] steps; }
};

// spmv_csr_ilu0 (kernels_ilu0.hip): what makes a handle a factor handle (its schedule is plan_trsv[SPMV_TRSV_LOWER])
struct Ilu0Plan {
    bool ready = false;
    int64_t a_rows = 0, a_nnz = 0;             // a's rows and nonzeros when the factor was made
    DevPtr<int32_t> d_pivot;                   // [1] the smallest row whose pivot is +-0 or not finite, INT32_MAX: none
};

// A derived handle's map of storage positions back into its parent: vals[i] = the parent's vals[words[i]].  spmv_csr_transpose
// (keep_map = 1), spmv_csr_select_* (keep_map = 1; positions ascending inside a row) and spmv_csr_permute
// (SPMV_PERMUTE_KEEP_MAP) keep one; `maker` says which, and each family of companions takes its own maker's map alone.
enum class MapMaker { none = 0, transpose, select, permute };
struct PosMap {
    DevPtr<uint32_t> words;            // [the handle's nnz]
    int64_t parent_len = 0;            // the length of the parent's arrays: every entry lies below it (a select call notes it without a map too)
    MapMaker maker = MapMaker::none;   // none: the handle has no map
};

}  // namespace spmv


// The opaque handle of include/spmv_hip.h.
struct spmv_csr {
    int64_t rows = 0, cols = 0, nnz = 0;
    const int32_t *d_row_ptr = nullptr;
    const int32_t *d_col_idx = nullptr;
    const float *d_vals = nullptr;
    spmv::DevPtr<int32_t> own_row_ptr, own_col_idx;   // the handle's own copies behind the views (empty: the caller's arrays)
    spmv::DevPtr<float> own_vals;
    spmv::PosMap map;              // where every entry sits in the parent's arrays (a handle of spmv_csr_transpose, _select_*, _permute)
    int device = 0;

    // plan state
    int vector_width = 0;          // SPMV_VECTOR: lanes per row (2..32), 0 = not planned
    spmv::ChunkPlan plan_adaptive; // SPMV_ADAPTIVE: 256-thread workgroups
    spmv::ChunkPlan plan_tiled;    // SPMV_TILED: workgroup size chosen from the column windows
    spmv::PanelPlan plan_panel;    // SPMV_PANEL
    spmv::PanelPlan plan_auto_panel;   // SPMV_AUTO where it resolved to the panel family (its own: see refresh_panel)
    bool auto_made_tiled = false;  // SPMV_AUTO made the TILED plan it looked at (and may release it)
    spmv::XskipPlan plan_xskip;    // SPMV_XSKIP
    spmv::WavePlan plan_wave;      // SPMV_WAVE_PIPE
    spmv::SpmmPlan plan_spmm;      // spmv_csr_spmm
    spmv::AttnPlan plan_attn;      // spmv_csr_attention_*
    spmv::SpgemmPlan plan_spgemm;  // spmv_csr_spgemm_values (a handle made by spmv_csr_spgemm with keep_plan = 1)
    spmv::AddPlan plan_add;        // spmv_csr_add_values / _gather (a handle made by spmv_csr_add with keep_plan = 1)
    spmv::TrsvPlan plan_trsv[2];   // spmv_csr_trsv: one slot per uplo (SPMV_TRSV_LOWER, SPMV_TRSV_UPPER)
    spmv::Ilu0Plan plan_ilu0;      // spmv_csr_ilu0_values / _solve / _pivot (a handle made by spmv_csr_ilu0)
    int auto_variant = -1;         // SPMV_AUTO: the variant its plan chose (-1 = not planned)
    uint64_t values_gen = 0;       // bumped by spmv_csr_values_changed: plans that copied vals before that are stale
};

// The tiled bitmap-CSR handle (kernels_tcsr.hip).
struct spmv_tcsr {
    int M = 0, N = 0;
    int64_t nnz = 0, nblocks = 0;
    spmv::DevPtr<int32_t> d_blk_idx;   // [nblocks+1]
    spmv::DevPtr<uint32_t> d_bitmaps;  // [M*N/32]
    spmv::DevPtr<float> d_vals;        // [nnz]
    int nseg = 0;                      // input-dimension segments per strip pair
    spmv::DevPtr<float> d_partial;     // [nseg][N] partial sums, combined in segment order
};

// The WSP / AWSP / AWSPRef handle (kernels_bitmap.hip).
struct spmv_bitmap {
    int format = 0;                 // enum spmv_bitmap_format
    int M = 0, N = 0;
    int device = 0;
    int64_t n_bitmaps = 0, n_vals = 0;
    int32_t stats[4] = {0, 0, 0, 0};   // WSP {nz_max_m, nz_max_n}, AWSP {nz_bk_max_}, AWSPRef warp_nz_offset_[4]
    spmv::DevPtr<uint32_t> d_bitmaps;
    spmv::DevPtr<float> d_vals;
    spmv::DevPtr<float> d_partial;  // AWSP/AWSPRef: [4][N] quarter partials
};

namespace spmv {

// ---- kernel launchers (each enqueues on `s`, returns a status) -------------
int launch_scalar(spmv_csr &h, const float *x, float *y, hipStream_t s);
int launch_wave(spmv_csr &h, const float *x, float *y, bool pipelined, hipStream_t s);
int plan_wave(spmv_csr &h, hipStream_t s);
int launch_vector(const spmv_csr &h, const float *x, float *y, hipStream_t s);
int launch_adaptive(const spmv_csr &h, const float *x, float *y, bool tiled, hipStream_t s);
// the same run on nnz 16-bit values of the caller's (dtype SPMV_ATTN_BF16 | SPMV_ATTN_FP16) in the place of h.d_vals
int launch_adaptive_vals16(const spmv_csr &h, int dtype, const void *vals16, const float *x, float *y, bool tiled, hipStream_t s);

int plan_xskip(spmv_csr &h, hipStream_t s);
int launch_xskip(const spmv_csr &h, const float *x, float *y, hipStream_t s);
int plan_vector(spmv_csr &h, hipStream_t s);
int plan_adaptive(spmv_csr &h, bool tiled, hipStream_t s);
// TILED with exactly these parameters (spmv_csr_plan_set); block 256|512|1024, maxpass >= 1
int plan_tiled_with(spmv_csr &h, int block, int maxpass, bool col16, hipStream_t s);
int plan_adaptive_with(spmv_csr &h, int block, hipStream_t s);
int build_panel(spmv_csr &h, PanelPlan &dst, int want_bits, int want_waves, int want_mode, hipStream_t s);   // params[4..6]; 0 = library default
int refresh_panel(spmv_csr &h, PanelPlan &dst, hipStream_t s);
int launch_panel_plan(const spmv_csr &h, const PanelPlan &p, const float *x, float *y, hipStream_t s);
void panel_params(const PanelPlan &p, int32_t params[8]);   // fills params[4..6]
int64_t panel_plan_bytes(const PanelPlan &p, int64_t nnz);
void panel_describe(const PanelPlan &p, const spmv_csr &h, char *buf, int n);
// kernels_panel.hip helpers shared with kernels_colsort.hip
int panel_row_blocks(const spmv_csr &h, int64_t nb0, int cap, hipStream_t s, DevPtr<int32_t> &brow, int32_t *nblocks);
int panel_rowloc(const spmv_csr &h, const int32_t *d_brow, int nblocks, uint16_t *d_rowloc, hipStream_t s);
// kernels_colsort.hip: SPMV_PANEL mode 3
int plan_colsort(spmv_csr &h, SortedBlocksPlan &p, int want_rows, int want_waves, hipStream_t s);
void colsort_params(const SortedBlocksPlan &p, int32_t params[8]);
int64_t colsort_plan_bytes(const SortedBlocksPlan &p, int64_t nnz);
void colsort_describe(const SortedBlocksPlan &p, const spmv_csr &h, char *buf, int n);
double colsort_model_cost(const SortedBlocksPlan &p, int64_t nnz);
double colsort_cost(int rows_per_block, double lines_per_nnz, double tail_frac);
int colsort_probe(const spmv_csr &h, hipStream_t s, double *long_frac, double *wide_frac, double *lines_per_nnz);
int launch_colsort(const spmv_csr &h, const SortedBlocksPlan &p, const float *x, float *y, hipStream_t s);
// kernels_binned.hip: SPMV_PANEL modes 4 and 5
int panel_tile_ptr(const spmv_csr &h, const int32_t *d_brow, int nblocks, int pw_bits, int np, int32_t *d_tile_ptr, hipStream_t s);
int plan_binned(spmv_csr &h, BinnedPlan &p, int want_rows, hipStream_t s);
int launch_binned(const spmv_csr &h, const BinnedPlan &p, const float *x, float *y, hipStream_t s);
void binned_params(const BinnedPlan &p, int32_t params[8]);
int64_t binned_plan_bytes(const BinnedPlan &p, int64_t nnz);
void binned_describe(const BinnedPlan &p, const spmv_csr &h, char *buf, int n);
int plan_scatter(spmv_csr &h, ScatteredPlan &p, int want_rows, hipStream_t s);
int launch_scatter(const spmv_csr &h, const ScatteredPlan &p, const float *x, float *y, hipStream_t s);
void scatter_params(const ScatteredPlan &p, int32_t params[8]);
int64_t scatter_plan_bytes(const ScatteredPlan &p, int64_t nnz);
void scatter_describe(const ScatteredPlan &p, const spmv_csr &h, char *buf, int n);
double binned_tile_nonzeros(const spmv_csr &h, int bin_rows);
// kernels_spmm.hip: spmv_csr_spmm
int plan_spmm(spmv_csr &h, hipStream_t s);
int plan_spmm_cols(spmv_csr &h, int k_max, hipStream_t s);      // and the scratch of the _cols calls at up to k_max columns
int64_t spmm_plan_bytes(const spmv_csr &h);
// One launch function per product, instantiated for E = float, bf16 and fp16 (every ld in elements of E).  who: the entry
// point's name, for a refusal.  cols = false: k <= 64, a lane group sized by k (spmv_csr_spmm, _16; spmv_csr_sddmm, _16);
// cols = true: any k in column tiles of 64 on the plan of plan_spmm_cols (spmv_csr_spmm_cols, spmv_csr_sddmm_cols).
template <typename E>
int launch_spmm(const spmv_csr &h, const char *who, bool cols, int k, const E *X, int64_t ldx, E *Y, int64_t ldy, hipStream_t s);
// kernels_sddmm.hip: spmv_csr_sddmm (on the plan of plan_spmm)
template <typename E>
int launch_sddmm(const spmv_csr &h, const char *who, bool cols, int k, const E *U, int64_t ldu, const E *X, int64_t ldx, float *out,
                 hipStream_t s);
// kernels_softmax.hip: spmv_csr_row_softmax / spmv_csr_row_softmax_backward (on the plan of plan_spmm and its scratch)
int launch_row_softmax(const spmv_csr &h, float scale, const float *scores, float *out, hipStream_t s);
int launch_row_softmax_backward(const spmv_csr &h, float scale, const float *P, const float *dP, float *dS, hipStream_t s);
// kernels_attention.hip: spmv_csr_attention_* (on the plan of plan_spmm and a scratch of its own)
int plan_attention(spmv_csr &h, hipStream_t s);
int plan_attention_heads(spmv_csr &h, int heads, hipStream_t s);
int plan_attention_wide(spmv_csr &h, int heads, hipStream_t s);     // the same and the scratch of widths above 64
int64_t attention_plan_bytes(const spmv_csr &h);
int attention_max_heads(const spmv_csr &h, int width);   // heads one launch takes at operands of `width` <= 128 columns (>= 0)
// (one call of any of the nine entry points: `a` filled and checked by capi.hip; `heads` query heads, `group` of them per K/V head;
// sum_group: backward_kv adds the heads of a group in the kernel, as the _gqa call does; `what` names the caller in a refusal;
// bb: the bias of a _bias entry point, null for every other call)
int launch_attention(AttnPass pass, const spmv_csr &h, const AttnArgs &a, const AttnBias *bb, int heads, int group, bool sum_group,
                     const char *what, hipStream_t s);
int launch_attention(AttnPass pass, const spmv_csr &h, const AttnArgsT<bf16> &a, const AttnBias *bb, int heads, int group, bool sum_group,
                     const char *what, hipStream_t s);       // 16-bit matrices: every ld and stride in elements
int launch_attention(AttnPass pass, const spmv_csr &h, const AttnArgsT<fp16> &a, const AttnBias *bb, int heads, int group, bool sum_group,
                     const char *what, hipStream_t s);
// kernels_transpose.hip: spmv_csr_transpose / spmv_csr_transpose_values
int transpose(const spmv_csr &a, bool keep_map, hipStream_t s, spmv_csr_t **out);
int transpose_values(spmv_csr &t, const spmv_csr &a, hipStream_t s);
// kernels_map.hip: the one strided move through a map over n entries (the handle's nnz), 32-bit words copied as bits, for
// c < count, i < n: dst[c * dst_stride + i] = src[c * src_stride + words[i]], or (scatter) dst[c * dst_stride + words[i]] =
// src[c * src_stride + i].  An entry at or beyond parent_len (the library builds none): a transpose or permute map's gather
// stores 0, a select map's and every scatter leave the word as it is.
int map_move(const PosMap &map, int64_t n, bool scatter, int count, const void *src, int64_t src_stride, void *dst, int64_t dst_stride,
             hipStream_t s);
// kernels_select.hip: spmv_csr_select_topk (thresh = false: k) / spmv_csr_select_threshold (thresh = true: thr_key = select_key of
// the threshold); score null: a's vals
int select(const spmv_csr &a, const float *score, bool thresh, int k, uint32_t thr_key, bool abs, bool keep_map, hipStream_t s,
           spmv_csr_t **out);
uint32_t select_key(float score, bool abs);

// kernels_spgemm.hip: spmv_csr_spgemm / spmv_csr_spgemm_values (the numeric pass alone, on c's plan)
int spgemm(const spmv_csr &a, const spmv_csr &b, bool keep_plan, hipStream_t s, spmv_csr_t **out, int64_t *products);
int spgemm_values(spmv_csr &c, const spmv_csr &a, const spmv_csr &b, hipStream_t s);
int64_t spgemm_plan_bytes(const spmv_csr &c);

// kernels_add.hip: spmv_csr_add / spmv_csr_add_values (the value pass alone, on c's plan) / spmv_csr_add_gather
int add(const spmv_csr &a, const spmv_csr &b, float alpha, float beta, int op, bool keep_plan, hipStream_t s, spmv_csr_t **out);
int add_values(spmv_csr &c, const spmv_csr &a, const spmv_csr &b, float alpha, float beta, hipStream_t s);
int add_gather(const spmv_csr &c, int side, int count, const void *src, int64_t src_stride, void *dst, int64_t dst_stride, hipStream_t s);
int64_t add_plan_bytes(const spmv_csr &c);

// kernels_trsv.hip: spmv_csr_trsv_plan / spmv_csr_trsv (upper: SPMV_TRSV_UPPER; unit: SPMV_TRSV_UNIT)
int trsv_plan(spmv_csr &h, bool upper, int thin_rows, hipStream_t s);
int trsv_solve(const spmv_csr &h, bool upper, bool unit, const float *b, float *x, hipStream_t s);
int64_t trsv_plan_bytes(const TrsvPlan &p, int64_t rows);

// kernels_ilu0.hip: spmv_csr_ilu0 / _values (the factorisation alone, on m's lower trsv plan) / _solve / _pivot
int ilu0(const spmv_csr &a, int thin_rows, hipStream_t s, spmv_csr_t **out);
int ilu0_values(spmv_csr &m, const spmv_csr &a, hipStream_t s);
int ilu0_solve(const spmv_csr &m, const float *r, float *z, hipStream_t s);
int ilu0_pivot(const spmv_csr &m, hipStream_t s, int64_t *row);
int64_t ilu0_plan_bytes(const spmv_csr &m);

// kernels_color.hip: spmv_csr_color (perm may be null; color_ptr: the host's, cap entries, may be null; info may be null)
int color(const spmv_csr &a, uint32_t seed, hipStream_t s, int32_t *d_color, int32_t *d_perm, int32_t *color_ptr, int cap, int64_t info[8]);
// kernels_permute.hip: spmv_csr_permute / spmv_permute_vector (_permute_values and _gather: map_move)
int permute(const spmv_csr &a, const int32_t *row_perm, const int32_t *col_perm, bool keep_map, bool via_transpose, hipStream_t s,
            spmv_csr_t **out);
int permute_vector(const int32_t *perm, int64_t n, bool inverse, const float *src, float *dst, hipStream_t s);

int dense_to_csr(int M, int N, const float *d_A, hipStream_t s, spmv_csr_t **out);
int dense_gemv(int M, int N, const float *d_A, const float *d_x, float *d_y, int mode, hipStream_t s);
// the reference's ASP layout (kernels_dense.hip): re-tile, and the multiply from it with the x == 0 skip
int asp_retile(int M, int N, const float *d_A, float *d_asp, hipStream_t s);
int asp_gemv_ws(int M, int N, const float *d_asp, const float *d_x, float *d_y, void *d_ws, size_t ws_bytes, hipStream_t s);
size_t dense_gemv_workspace_bytes(int N, int mode);
int dense_gemv_ws(int M, int N, const float *d_A, const float *d_x, float *d_y, int mode, void *d_ws, size_t ws_bytes,
                  hipStream_t s);

// kernels_rows.hip: structural check of a CSR (bad[0] first row with row_ptr[r] > row_ptr[r+1] or outside [0,nnz],
// bad[1] first element with a column outside [0,cols), bad[2]/bad[3] row_ptr[0] / row_ptr[rows] when wrong)
int launch_validate(const spmv_csr *h, int32_t *d_bad4, hipStream_t stream);
// order-sensitive 64-bit checksum of vals (a device pass + a host wait: debug aid behind SPMV_CHECK_VALUES=1)
int values_checksum(const spmv_csr &h, hipStream_t s, uint64_t *out);
bool check_values_env();   // SPMV_CHECK_VALUES=1 (read once)
// stamp a plan that has just copied vals / refuse to run one whose copy is out of date (SPMV_ERR_STALE_PLAN)
int stamp_values(const spmv_csr &h, hipStream_t s, ValuesStamp &st);
int require_fresh_values(const spmv_csr &h, const ValuesStamp &st, hipStream_t s, const char *variant);
// min / max of col_idx (kernels_rows.hip): d_out[0] = min (INT_MAX when nnz = 0), d_out[1] = max (-1)
int launch_column_range(const spmv_csr &h, int32_t *d_out2, hipStream_t s);
// in-place exclusive scan of n int32 (one 1024-thread workgroup); the total goes to *d_total
int exclusive_scan_i32(int32_t *d_data, int64_t n, int32_t *d_total, hipStream_t s);
// ... for offset tables the host sizes arrays from: the total also comes to *total_host and, where append_total, into d_data[n]; waits for s
int scan_offsets_i32(int32_t *d_data, int64_t n, int32_t *d_total, bool append_total, hipStream_t s, int32_t *total_host);

int tcsr_from_dense(int M, int N, const float *d_A, hipStream_t s, spmv_tcsr_t **out);
int tcsr_run(const spmv_tcsr &h, const float *d_x, float *d_y, hipStream_t s);
int tcsr_sizes(const spmv_tcsr &h, int64_t *n_blk_idx, int64_t *n_bitmaps, int64_t *n_vals);
int tcsr_download(const spmv_tcsr &h, int32_t *blk_idx, uint32_t *bitmaps, float *vals);
void tcsr_dims(const spmv_tcsr &h, int *M, int *N);

// kernels_bitmap.hip: the reference's WSP / AWSP / AWSPRef formats
int bitmap_from_dense(int format, int M, int N, const float *d_A, hipStream_t s, spmv_bitmap_t **out);
int bitmap_run(const spmv_bitmap &h, const float *d_x, float *d_y, hipStream_t s);
void bitmap_info(const spmv_bitmap &h, int *format, int *M, int *N, int64_t *n_bitmaps, int64_t *n_vals, int32_t stats[4]);
int bitmap_download(const spmv_bitmap &h, uint32_t *bitmaps, float *vals);
int bitmap_device(const spmv_bitmap &h);

int synth_fill(uint64_t seed, int64_t row0, int64_t n_local, int64_t rows, int64_t cols, int64_t band,
               const int32_t *d_row_ptr, int32_t *d_col_idx, float *d_vals, hipStream_t s);
int synth_x(uint64_t seed, int64_t j0, int64_t n, float *d_x, hipStream_t s);


// ---- bounds-checked build (SPMV_CHECK_BOUNDS: lib/libspmv_hip_checked.so, a test aid) --------------------------------
// The streams that read or write past a tile's or a bin's end on purpose (and rely on slack allocated behind the arrays)
// check every access's byte range [lo, lo + len) against the array's allocated bytes.  A violation is recorded in a
// table of the translation unit (no -fgpu-rdc: every .hip file has its own; site -> count, largest overrun in bytes) and
// the access is NOT issued: a load is redirected to offset 0 and its value replaced by zero, a store is skipped.  Without
// the define every macro below expands to nothing (or to its plain operand): the library's device code is unchanged.
//   SPMV_BOUNDS_LOAD(ok, site, var, lo, len, limit)   declares bool ok; out of range: var (the offset the load uses) = 0
//   SPMV_BOUNDS_VALUE(ok, v)                           v, or zero where !ok
//   SPMV_BOUNDS_BUF(ok, site, voff, soff, len, limit)  a buffer load at voff + soff: out of range, both become 0 (else
//                                                      the sum moves to voff: the scalar offset may not diverge)
//   SPMV_BOUNDS_STORE(site, lo, len, limit) stmt;      the store runs only when in range
enum BoundsSite {
    kSiteBsSumsProd = 0, kSiteBsSumsAcc, kSiteBinSumsProd, kSiteBinSumsR16, kSiteBsProductsC16, kSiteBsProductsVals,
    kSiteBsProductsStore, kSiteBsGroupStore, kSiteBsPlaceLoad, kSiteBsPlaceAcc, kSiteBsPlaceC16, kSiteBsFillAcc,
    kSiteBsFillC16, kSitePanelPacked, kSitePanelVals,
    kBoundsSites
};
#if defined(SPMV_CHECK_BOUNDS)
namespace {
// [site][0] = violations, [site][1] = largest overrun in bytes (this translation unit's kernels only)
__device__ __attribute__((unused)) unsigned long long g_bounds[kBoundsSites][2];
}
#if defined(__HIPCC__)
__device__ __forceinline__ bool bounds_in(int site, int64_t lo, int64_t len, int64_t limit)
{
    if (lo >= 0 && lo + len <= limit) return true;
    atomicAdd(&g_bounds[site][0], 1ull);
    atomicMax(&g_bounds[site][1], (unsigned long long)(lo < 0 ? -lo : lo + len - limit));
    return false;
}
#endif
// host: add this translation unit's table into out[site][2] and clear it (the device is synchronised first)
static inline int bounds_collect_local(unsigned long long out[kBoundsSites][2])
{
    unsigned long long t[kBoundsSites][2] = {};
    SPMV_HIP_TRY(hipDeviceSynchronize());
    SPMV_HIP_TRY(hipMemcpyFromSymbol(t, HIP_SYMBOL(g_bounds), sizeof t));
    const unsigned long long zero[kBoundsSites][2] = {};
    SPMV_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bounds), zero, sizeof zero));
    for (int i = 0; i < kBoundsSites; ++i) {
        out[i][0] += t[i][0];
        if (t[i][1] > out[i][1]) out[i][1] = t[i][1];
    }
    return SPMV_OK;
}
#define SPMV_BOUNDS_LOAD(ok, site, var, lo, len, limit) \
    const bool ok = ::spmv::bounds_in((site), (int64_t)(lo), (int64_t)(len), (int64_t)(limit)); \
    if (!ok) var = 0
#define SPMV_BOUNDS_VALUE(ok, v) ((ok) ? (v) : decltype(v){})
#define SPMV_BOUNDS_BUF(ok, site, voff, soff, len, limit) \
    const bool ok = ::spmv::bounds_in((site), (int64_t)(uint32_t)(voff) + (int64_t)(uint32_t)(soff), (int64_t)(len), (int64_t)(limit)); \
    voff = ok ? voff + soff : 0; \
    soff = 0
#define SPMV_BOUNDS_STORE(site, lo, len, limit) if (::spmv::bounds_in((site), (int64_t)(lo), (int64_t)(len), (int64_t)(limit)))
#else
#define SPMV_BOUNDS_LOAD(ok, site, var, lo, len, limit)
#define SPMV_BOUNDS_VALUE(ok, v) (v)
#define SPMV_BOUNDS_BUF(ok, site, voff, soff, len, limit)
#define SPMV_BOUNDS_STORE(site, lo, len, limit)
#endif
// kernels_binned.hip / kernels_panel.hip: their tables, added into out (SPMV_ERR_INVALID in the normal build)
int bounds_collect_binned(unsigned long long out[kBoundsSites][2]);
int bounds_collect_panel(unsigned long long out[kBoundsSites][2]);

#if defined(__HIPCC__)
// Stable scatter by key, 64 entries per step (k_panel_fill, k_bin_fill, k_bs_fill): which lanes hold a key that NO other lane of
// the step holds?  They take their cursor and bump it themselves; only the keys held twice go through the ballot loop -- on
// uniform columns over thousands of panels that is one or two trips instead of 64.  `tags` = 256 words of the wavefront's
// own LDS, hashed by the key's low bits: two keys in one slot both go to the loop (conservative, never wrong).
__device__ __forceinline__ bool lone_in_step(volatile int *tags, bool valid, int key, int lane)
{
    const int slot = key & 255;
    if (valid) tags[slot] = lane;
    __builtin_amdgcn_wave_barrier();
    const int first = valid ? tags[slot] : lane;
    __builtin_amdgcn_wave_barrier();
    if (valid && first != lane) tags[slot] = kWave;                 // somebody else's slot too: nobody in it is alone
    __builtin_amdgcn_wave_barrier();
    const int second = valid ? tags[slot] : kWave;
    __builtin_amdgcn_wave_barrier();
    return valid && second == lane;
}
#endif

}  // namespace spmv
