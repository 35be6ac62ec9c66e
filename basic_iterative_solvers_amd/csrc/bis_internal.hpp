// bis_internal.hpp -- shared internals of libbis_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bis_hip.h"

struct bis_trsv_plan;
struct bis_trsv_tiled;
struct bis_trsv_chain;
struct bis_trsm_plan;
// What the triangular sweeps of one direction have built on a matrix, all lazily (trsv_resolve, bis_sptrsv.hip).  A value
// change (bis_mat_values_changed) drops the tiled plan with its `tried` flag (it holds a copy of the values) and the level
// plan (its row views carry dictionaries); the chained plan and its flag stay (chains depend on the pattern only).
// Destroying the matrix drops everything.
struct bis_trsv_side {
    bis_trsv_plan *level = nullptr;  // level analysis, row views, the level-scheduled kernels' scratch
    bis_trsv_tiled *tiled = nullptr; // bis_trsv_tiled.hip, tried first: where it exists no level analysis is made
    bis_trsv_chain *chain = nullptr; // bis_trsv_chain.hip, for matrices without a grid: built from the level analysis
    bis_trsm_plan *multi = nullptr;  // bis_sptrsm.hip: the multi-vector sweeps' own level plan (structure only), whatever form the single-vector sweep takes
    bool tiled_tried = false, chain_tried = false; // the build ran (whether or not a plan came of it)
    const char *kernel = "";         // the kernel the last sweep of this direction ran (bis_mat_sweep_kernel)
    const char *kernel_m = "";       // ... and the last multi-vector sweep, with its instance (bis_mat_sweepm_kernel)
};

struct bis_named_kernel {
    int type = 0;
    const bis_mat *A = nullptr;
    double *B = nullptr, *C = nullptr;
    int64_t size_B = 0, size_C = 0;
    const double *D = nullptr;
    bool upper = false;
};

struct bis_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cus = 0;
    std::string arch;
    int64_t hbm_bytes = 0;
    std::string err;

    // reduction scratch: per-block partials + result slots (device), and a
    // pinned host mirror for blocking scalar returns
    double *partials = nullptr;   // [partials_cap], grown on demand
    size_t partials_cap = 0;
    double *scalars_dev = nullptr; // [64]
    double *scalars_host = nullptr; // pinned [64]
    unsigned *counters = nullptr; // [64] tickets / arrival counters (zeroed)
    // device-side waits that gave up (a lost hand-off in a triangular sweep) set this word (pinned host
    // memory mapped into the device); every blocking entry point checks it after its synchronisation
    unsigned *fault_host = nullptr, *fault_dev = nullptr;

    std::map<std::string, bis_named_kernel> kernels; // named-kernel registry (SMAX protocol)

    // set by every solver handle's *_iterate around its launches (bis_stop_guard, bis_solver.hpp): the SpMV, the SpMM, the
    // sweeps and the diagonal applies return at once when spmv_stop[1] (the solve's stop flag) is set, like the other
    // passes of a stopped iteration
    const int *spmv_stop = nullptr;

    // profiling
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t prof_used = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_sweep_events; // one pair per bis_sptrsv / bis_bsptrsv call
    size_t prof_sweep_used = 0;
};

// Tuning knobs (bis_set_option / BIS_* environment variables at first use).
struct bis_options;
bis_options &bis_opts();
struct bis_options {
    int spmv_variant = -1; // -1: default (40 = 256 threads, 4 staged vectors)
    int spmv_window = -1;  // -1: default (0: CRS gather kernel)
    int spmv_chunk = -1;   // -1: default (1024 non-zeros + rows per row block)
    int spmv_chunk_fused = -1; // -1: default (2048) for the SpMV with the fused dot epilogue
    int spmv_xcd_remap = -1; // 1: each XCD sweeps its own slab of row blocks (default: blockIdx order)
    int trsv_grid = -1;    // -1: automatic
    int ilu0_wave = -1;    // 0: lane-per-row ILU(0) level kernel (default: wave per row)
    int ilu0_wgs = -1;     // persistent ILU(0): workgroups per CU (default 6; never all 8 the runtime reports: the grid must be resident as a whole)
    int ilu0_persistent = -1; // 0: a launch per level (default: one persistent launch, a flag per finished row)
    int trsv_host_analysis = -1; // 1: level analysis on the host (default: on the device)
    int trsv_wave = -1;    // 1: one wave per row in the sync-free sweeps (default for rows > 16)
    int trsv_wave_wgs = -1; // wave-per-row level sweep: workgroups per CU (default 4; up to the 8 the runtime reports resident)
    int trsv_trial = -1;   // 0: the level-scheduled sweeps never time their two kernels against each other (default: the first sweep of a large triangle does)
    int trsv_batch = -1;   // dependencies polled per round trip (4, 8, 16; -1: by row length)
    int trsv_by_pos = -1;  // 1 (default): sentinel scratch in level order; 0: in row order
    int trsv_one_xcd = -1; // k > 0: sync-free sweeps run on one elected XCD with k workgroups per CU
    int tune_placement = -1; // k > 0: bis_dist_create runs bis_mat_tune_placement(A, k) before it makes the row views
    int spmv_packed32 = -1; // 1: also try the 32-window packed format (opt-in)
    int spmv_lds_pad = -1; // diagnostic: extra dynamic LDS bytes per workgroup (lowers occupancy)
    int spmv_packed = -1;  // 16-bit packed column stream: 0 off, 1 select tree, 2 lane permute (-1: default = 1)
    int spmv_valdict = -1; // value dictionary (a matrix with <= 256 distinct values streams 1-byte value codes): 0 off, 1 consecutive form only, 2 lane-per-row form where it applies (-1: default)
    int dist_host_plan = -1; // 1: bis_dist_create plans the halo on the host from the downloaded structure (default: on the device)
    int grid_autodetect = -1; // bis_mat_create: recognise a stencil on a structured grid from the offsets of a few rows (0: off)
    int trsv_chain = -1;    // natural-order sweeps of matrices without a grid: -1 = the chained sweep (bis_trsv_chain.hip) where its plan applies (chains of >= 3 rows on
                            // average, fewer chains straddling a level than resident waves), 1 = also with shorter chains, 0 = level-scheduled kernels only
    int trsv_chain_idle = -1;  // chained sweep: poll rounds without a delivery after which a feeder polls one word only (default: never -- measured slower with the pairs kept near the bound)
    int trsv_chain_pause = -1; // ... and pauses up to this many x 256 cycles between its looks (default 8)
    int trsv_chain_prefix = -1; // 1: the feeder sums the part of a row's fma chain before its first chain-internal operand (default off: measured slower -- the feeder then paces the pair: fem:80,80,81 forward 2.55 -> 3.0 ms)
    int trsv_chain_pairs = -1; // wave pairs per ticket queue (default: the plan's straddle bound + 1/8 + 8)
    int trsv_tiled = -1;    // natural-order sweeps: -1 = tiled sweep (bis_trsv_tiled.hip) where its device plan applies (grid hint), 1 = also with the host plan, 2 = host plan only, 0 = level-scheduled kernels
    int trsv_tile_rows = -1; // rows per tile at most (default 8192 for rows of <= 8 entries, else 2048)
    int trsv_tile_wgs = -1;  // resident workgroups per CU of the tiled sweep (default: what fits, 3)
    int trsv_tile_backoff = -1; // tiled sweep: a poller's pause grows by 64 cycles per round that delivers nothing, up to this many (default 16: HPCG-256 2.35 -> 2.30 ms per sweep, HPCG-128 0.77 -> 0.74, the 7-point grid unchanged; 0: never)
    int spmv_sellwin_nt = -1; // sliced-ELL SpMV: 0 = the code stream through the caches (default: non-temporal loads)
    int cg_nt_x = -1;        // fused CG: 0 = x read and written through the caches in the p-update pass (default: non-temporal)
    int trsv_tile_exp = -1;  // tiled sweep, timing experiments (bis_trsv_tiled.hip, TiledArgs::exp_flags); results are wrong with any bit set
    int trsv_tile_edge = -1; // grid-hinted matrices: tile extents in nodes, e (cubic) or ex | ey << 8 | ez << 16 (default by row length; 0 = interval tiles of the natural order)
    int force_rp64 = -1;   // 1: matrices created afterwards get 64-bit row pointers whatever their size (tests of the HPCG-512 code path)
    int spmv_sellwin = -1; // dictionary SpMV with the block's x window in LDS and sliced-ELL codes (bis_spmv_sellwin.hip): 0 off (-1: on where the matrix qualifies)
    int spmv_sellwin_rows = -1; // rows per lane of the sliced-ELL form: 1 or 2 (blocks of 256 or 512 rows; -1: default 2)
    int spmv_sellwin_pairs = -1; // 0: never the one-byte (column - row, value) pair codes
    int spmv_sellwin_joint = -1; // 0: never the 16-bit joint (slot, value) codes
    int spmv_colslab = -1;     // column slabs for matrices without locality (bis_spmv_slab.hip): 0 never, -1 where a build-time trial measures them faster, k >= 2: k slabs wherever the plan applies (tests)
    int spmv_win8 = -1;        // window + sliced-ELL SpMV with the 8-byte values streamed (matrices without a dictionary form, or with spmv_valdict = 0): 0 off, 1 on where its plan applies (-1: default = on)
    int spmv_win8_rows = -1;   // ... rows per lane: 1, 2 or 4 (blocks of 256, 512, 1024 rows; default 2)
    int spmv_win8_depth = -1;  // ... chunks requested ahead per lane: 1, 2, 3, 4 or 6 (default 3; 2 for 256-row blocks)
    int spmv_win8_sets = -1;   // ... register sets of the chunk ring: 1 = one set, drained once per round, 2 = two sets, never drained (depths 1-4; default by measurement, bis_spmv_win8_launch)
    int spmv_win8_implicit = -1; // ... implied window slots in the slices of a stencil (0: every chunk keeps its slots; default on where >= half the chunks qualify)
    int spmv_win8_tune = -1;   // ... placement tuning of the stream at build time: up to k re-allocations, the fastest kept (default 12 for streams of >= 1 GiB; 0 off)
    int spmv_win4 = -1;        // ... the same form with 4-byte values for a matrix that bis_mat_round_f32 flagged ("win4"): 0 off (such a matrix then streams win8), -1: default = on
    int spmv_sellwin_masks = -1; // 0: never the per-row pair masks (fmt 4: 4 bytes per ROW where the matrix has at most 32 (column - row, value) pairs)
    int device_share = -1;  // k > 1: this device is shared by k processes that all run persistent grids (several ranks on one GPU in a test
                            // or rehearsal): kernels that need their whole grid resident keep to 1/k of the device
    int trsm_form = -1;     // multi-vector sweeps (bis_sptrsm.hip): -1 / 0 by level count, 1 = a launch per level at any level count, 2 = the persistent wave-per-row kernel at any level count
    int spgemm_row_cap = -1;   // bis_spgemm: products per row up to which the row path (candidate columns sorted in LDS) is used; 0: every row takes the sort fallback (default and most: 4096)
    int spgemm_batch = -1;     // bis_spgemm: products per batch of the sort fallback (default 2^26)
    int trsv_inject_oom = -1;  // test hook: 1 makes the tiled sweep's device plan run out of memory
    int trsv_inject_loss = -1; // test hook: k > 0 makes row k-1 of the next natural-order sweep wait for a result nobody publishes
};
// row_ptr width of a new matrix: int64 when the non-zeros (plus the stream padding) do not fit int32
inline bool bis_want_rp64(int64_t nnz) { return nnz >= (int64_t)INT32_MAX - 8 || bis_opts().force_rp64 > 0; }

constexpr int kMaxReduceBlocks = 2048;
// workgroups (= partial sums) of the stand-alone reductions -- dot, sum of squares, the fused axpy + dot, the Jacobi step's
// residual norm: 16 N bytes of two non-temporal read streams move 5.9 TB/s from a grid of 2048, 6.3 from 4096, 6.4 from 8192
// (tools/blas1_bench.hip).  One constant for all of them: kernels that promise the bits of "ew3 then dot" share the index map.
constexpr int kMaxDotBlocks = 8192;
constexpr int kMaxEwBlocks = 16384; // elementwise kernels (no partial sums: the grid is free)
constexpr int kMaxIters = 1 << 20;  // iterations one solver handle may enqueue between two *_init calls
constexpr int kWinMaxTiles = 128; // x window: at most 128 tiles of 16 columns (16 KiB of LDS)
constexpr int kWinTile = 16;
constexpr int kWinTileLog = 4;
constexpr int kSwRows = 256; // window + sliced-ELL forms (bis_winplan.hpp): a block is kSwRows R rows, R rows per lane, R = 1, 2 or 4
constexpr int kSwMaxR = 4;

struct bis_mat {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    bool rp64 = false;        // row_ptr width on the device
    bool view = false;        // row-range view: row_ptr/col/val belong to another bis_mat
    void *row_ptr = nullptr;  // int32_t[n_rows+1] or int64_t[n_rows+1]
    int32_t *col = nullptr;   // [nnz + pad]
    double *val = nullptr;    // [nnz + pad]
    // SpMV row-block metadata: block k covers rows [blk_row[k], blk_row[k+1])
    int32_t *blk_row = nullptr;
    int64_t *blk_nnz = nullptr; // row_ptr[blk_row[k]] (saves a dependent load)
    int n_blocks = 0;
    int64_t view_row0 = 0;     // row views: first row of the view in the matrix it was cut from
    // The forms of the SpMV (table in bis_spmv.hip), each built lazily by spmv_resolve and owned by its unit: a pointer to the
    // unit's struct and a state, 0 = not tried, 1 = usable, -1 = does not apply.  bis_mat_free_meta and bis_mat_values_changed
    // say which of them a finalize and a value change drop.
    struct bis_xwin *xw = nullptr; // x window (bis_spmv_xwin.hip), built by bis_mat_finalize where spmv_window asks: null = none
    // packed-column streams (bis_spmv_colpack.hip), one per row-block table (0 plain, 1 fused): 10 instead of 12 streamed
    // bytes per non-zero; -1 = some block needs more column windows than the format has
    struct { struct bis_colpack *p = nullptr; int state = 0; } pk[2];
    // value dictionary and its lane-per-row blocks (bis_spmv_valdict.hip); -1 = too many distinct values
    struct { struct bis_valdict *p = nullptr; int state = 0; } vd;
    // x-window + sliced-ELL form of the dictionary kernel (bis_spmv_sellwin.hip)
    struct bis_sellwin *sw = nullptr;
    int sw_state = 0;
    // the same plan with the values streamed (no dictionary needed), bis_spmv_win8.hip.  [0]: 8-byte values, "win8";
    // [1]: 4-byte values, "win4", built only while f32_exact holds
    struct { struct bis_win8 *p = nullptr; int state = 0; } w8[2];
    // column slabs of a matrix without locality (bis_spmv_slab.hip, colslab_try in bis_spmv.hip); -1 = refused
    struct { std::vector<bis_mat *> *slabs = nullptr; int state = 0; double trial_ms[2] = {0.0, 0.0}; } cs; // trial_ms: the build-time trial, one pass / the K passes
    // every value of val is exactly representable in binary32: set by bis_mat_round_f32, cleared by bis_mat_scale_sym and
    // bis_mat_retune, inherited by row views (bis_mat_row_view) and by nothing else
    bool f32_exact = false;
    // second table for the SpMV with the fused (y,w) epilogue (CG): larger blocks win there
    int32_t *blkf_row = nullptr;
    int64_t *blkf_nnz = nullptr;
    int n_blocks_f = 0;
    int chunk_f = 0;
    int chunk_nnz = 0;        // nnz budget per block used to build blk_row
    int max_row_nnz = 0;
    int64_t max_block_nnz = 0;
    // structured-grid hint (generators, bis_mat_set_grid_hint): row = ((z*ny + y)*nx + x)*dof + d; 0 = none.
    // Inherited by the strict triangles and the ILU(0) factors; the tiled sweep cuts its tiles in all grid directions with it.
    int64_t grid[4] = {0, 0, 0, 0};
    bis_trsv_side trsv[2]; // what the sweeps built for this triangle, forward / backward (bis_trsv_side_of)
    const char *spmv_kernel[2] = {"", ""};  // the kernel the last plain / fused-dot SpMV of this matrix launched (bis_mat_spmv_kernel)
    const char *ilu0_kernel = "";           // the elimination kernel that made this ILU(0) L factor (bis_mat_ilu0_kernel)
    const char *itrsv_kernel = "";          // the path the last step of bis_itrsv took on this triangle (bis_itrsv_kernel)
    const char *spmm_kernel = "";           // the path and template instance the last bis_spmm on this matrix launched (bis_mat_spmm_kernel)
    const char *iluk_kernel = "";           // the symbolic search that made this ILU(k) pattern or L factor, k >= 1 (bis_mat_iluk_kernel)
    const char *spgemm_kernel = "";         // the path(s) of bis_spgemm that made this product (bis_spgemm_kernel)
    const char *fsai_kernel = "";           // the instance of fsai_rows_kernel that computed this FSAI factor G (bis_mat_fsai_kernel)
    struct bis_mg *mg = nullptr;            // the hierarchy this matrix is the preconditioner operand of (bis_mg_operand): an n x n matrix without
                                            // entries that the hierarchy owns; bis_mat_destroy leaves it alone
    struct bis_bj *bj = nullptr;            // ... or the block-Jacobi handle (bis_bj_operand), in the same way
};

#define BIS_HIP_CHECK(ctx, call)                                               \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);    \
            return BIS_ERR_HIP;                                                \
        }                                                                      \
    } while (0)

// after a stream synchronisation: did a kernel raise the fault word?
bis_status bis_fault_check(bis_ctx *ctx);
#define BIS_SYNC_CHECK(ctx)                                                    \
    do {                                                                       \
        BIS_HIP_CHECK(ctx, hipStreamSynchronize((ctx)->stream));               \
        if (bis_status fs_ = bis_fault_check(ctx)) return fs_;                 \
    } while (0)

#define BIS_REQUIRE(ctx, cond, msg)                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (ctx) (ctx)->err = (msg);                                       \
            return BIS_ERR_INVALID;                                            \
        }                                                                      \
    } while (0)

#define BIS_CTX_OK(ctx)                                                        \
    do {                                                                       \
        if (!(ctx)) return BIS_ERR_NO_DEVICE;                                  \
    } while (0)

// Status words of the build and check kernels: the words of ctx->counters in use, each with the number of words from its index.
// A site zeroes its words on the stream, launches, reads them back.  Words 0-31 are free, and every later word that no entry covers.
enum bis_slot {
    kSlotMaxRow = 32,   // 1: the longest row (bis_mat_finalize)
    kSlotValidate = 36, // 1: bis_mat_create's check of row_ptr and col
    kSlotDups = 38,     // 1: a row holds a column twice (bis_mat_sorted_copy)
    kSlotXwin = 40,     // 2: some block touches too many tiles, most tiles of a block (bis_spmv_xwin.hip)
    kSlotColpack = 44,  // 1: some block needs a window too many (bis_spmv_colpack.hip)
    kSlotValdict = 46,  // 1: too many distinct values (bis_spmv_valdict.hip)
    kSlotWinplan = 52,  // 6: the plans of bis_spmv_sellwin.hip and bis_spmv_win8.hip ([0] not representable, [1] largest window,
                        //    [2] win8: the windows' sum, sellwin: a fill gave up, [3] sellwin: too many pairs, [5] most chunks of a slice)
};
inline int *bis_slot_ptr(bis_ctx *ctx, int slot) { return (int *)ctx->counters + slot; }
// host == nullptr: zeroes n words from `slot` on the stream; otherwise copies them to host and synchronises the stream
inline hipError_t bis_slot_io(bis_ctx *ctx, int slot, int n, int *host = nullptr) {
    if (!host) return hipMemsetAsync(bis_slot_ptr(ctx, slot), 0, sizeof(int) * (size_t)n, ctx->stream);
    const hipError_t e = hipMemcpyAsync(host, bis_slot_ptr(ctx, slot), sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    return e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
}

// operands that a kernel loads 16 bytes per lane
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the header's hash32: two multiply-xorshift rounds.  The MIS key and the power iteration's start (bis_mg.hip), IDR's shadow
// space (bis_idr.hip), the start vector of the Lanczos handles (bis_lanczos.hpp)
__host__ __device__ __forceinline__ uint32_t bis_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// `count` device words, zeroed on the stream: a handle's flags and arrival counters
template <class T>
inline bis_status bis_alloc_zeroed(bis_ctx *ctx, T **out, size_t count) {
    const size_t bytes = sizeof(T) * count;
    return hipMalloc(out, bytes) == hipSuccess && hipMemsetAsync(*out, 0, bytes, ctx->stream) == hipSuccess ? BIS_OK : BIS_ERR_HIP;
}

// ---- device helpers ---------------------------------------------------------
// wave64 sum via DPP-free shuffles (ds_bpermute under the hood for doubles).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// a b rounded on its own.  __dmul_rn is a plain `*` in this toolchain's headers and the default contraction mode fuses it
// into a following addition (pragmas notwithstanding); a value that went through an opaque register cannot be fused.  For
// results that are promised bit for bit against "product rounded, then sum rounded".
__device__ __forceinline__ double bis_mul_sep(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// Block sum for blockDim.x == T (multiple of 64). Result valid in thread 0.
template <int T>
__device__ __forceinline__ double block_sum(double v, double *lds /*[T/64]*/) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) lds[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < T / 64; ++i) r += lds[i];
    }
    return r;
}

// ---- last-arriver reductions ---------------------------------------------------------
// A streaming pass ends with a global reduction of per-workgroup partial sums.  Instead of a
// second launch, every workgroup publishes its partials (write-through `sc1` stores, drained with
// vmcnt(0) before the arrival is counted -- the "drained sc1 payload, then the flag" hand-off of
// MI355X_MICROARCH.md, no release fence that would write back the pass' own dirty lines) and
// takes a ticket; the workgroup that takes the LAST ticket re-reads all partials with L2-bypassing
// loads and sums them in index order, so the result does not depend on which workgroup finishes
// last: bit-reproducible like the two-launch form.
__device__ __forceinline__ void publish(double *slot, double v) {
    __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double fetch(const double *slot) {
    return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0 only; returns true in the workgroup that arrives last (and re-arms the counter)
__device__ __forceinline__ bool arrive_last(unsigned *counter, unsigned n_groups) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the published partials have left this CU
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != n_groups - 1) return false;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // next use: after a kernel boundary
    return true;
}

// The same with a counter per 16 workgroups under one top counter.  Tickets on ONE address serialise at ~11.4 ns each (measured:
// the sweeps' ticket counter): 2048 workgroups of pass B cost 23 us in tickets alone -- nothing next to 70 us of streaming
// on 16.8 M rows, but most of the pass on one rank's 1/8 share of a strong-scaled problem (34 us measured for 2 M rows against
// 10 us of bandwidth time: profiles/r04_b_dist_gap_slab32.txt).  Two levels: 16 + n/16 tickets on the critical path.
constexpr unsigned kArriveGroup = 16;
constexpr unsigned kArriveSubs = 2048 / kArriveGroup; // kMaxReduceBlocks workgroups at most
__device__ __forceinline__ bool arrive_last2(unsigned *top, unsigned *sub, unsigned block, unsigned n_blocks) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the published partials have left this CU
    const unsigned g = block / kArriveGroup;
    const unsigned n_in = min(kArriveGroup, n_blocks - g * kArriveGroup), n_groups = (n_blocks + kArriveGroup - 1) / kArriveGroup;
    if (__hip_atomic_fetch_add(&sub[g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != n_in - 1) return false;
    __hip_atomic_store(&sub[g], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != n_groups - 1) return false;
    __hip_atomic_store(top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // next use: after a kernel boundary
    return true;
}

// XCD-aware remap (cdna_hip_programming.md T1 / MI355X_MICROARCH.md "Workgroup
// dispatch"): hardware deals workgroups round-robin over the 8 XCDs, so
// blockIdx b lands on XCD b%8.  Map it to a logical block id such that each
// XCD sweeps one contiguous range of logical blocks (its private L2 then sees
// neighbouring rows / x-planes).  Valid for any n; ids >= n are skipped by the
// caller.  Placement is a speed matter only.
__device__ __forceinline__ int xcd_remap(int b, int n_padded8) {
    const int per = n_padded8 >> 3;
    return (b & 7) * per + (b >> 3);
}
// Grouped form: within every window of 8*G consecutive logical blocks, XCD j
// takes the G consecutive blocks [j*G, (j+1)*G).  G = 1 is blockIdx order.
__device__ __forceinline__ int xcd_group_remap(int b, int G) {
    const int j = b & 7, q = b >> 3;
    return (q / G) * (8 * G) + j * G + (q % G);
}

// HIP-event bracket around one launch (bis_profile_enable)
inline void bis_prof_begin(bis_ctx *ctx) {
    if (!ctx->profile) return;
    if (ctx->prof_used == ctx->prof_events.size()) {
        hipEvent_t a, b;
        hipEventCreate(&a);
        hipEventCreate(&b);
        ctx->prof_events.emplace_back(a, b);
    }
    hipEventRecord(ctx->prof_events[ctx->prof_used].first, ctx->stream);
}
inline void bis_prof_end(bis_ctx *ctx) {
    if (!ctx->profile) return;
    hipEventRecord(ctx->prof_events[ctx->prof_used].second, ctx->stream);
    ++ctx->prof_used;
}

// result_dev[v] = sum_i partials[v*stride + i], i < n_partials (fixed order)
bis_status bis_reduce_finish(bis_ctx *ctx, int n_partials, int n_values,
                             size_t stride, double *result_dev);
// make sure ctx->partials holds at least n doubles (stream-synchronising
// only when it has to grow)
bis_status bis_ensure_partials(bis_ctx *ctx, size_t n);
// y = A x; if w != nullptr also partials[partials_off + b] = sum_{r in block b}
// y[r]*w[r] (n_partials = number written).  The caller sizes ctx->partials
// (bis_spmv_partials_bound).
bis_status bis_spmv_launch(bis_ctx *ctx, const bis_mat *A, const double *x,
                           double *y, const double *w, int *n_partials,
                           size_t partials_off = 0);
// Y = A X for n_rhs interleaved vectors (bis_spmm.hip); a launch made while ctx->spmv_stop is set returns at once when
// spmv_stop[1] is, like bis_spmv_launch (n_rhs == 1 IS bis_spmv_launch)
bis_status bis_spmm_launch(bis_ctx *ctx, const bis_mat *A, const double *X, double *Y, int n_rhs);
// upper bound on the partials one fused bis_spmv_launch of A writes, whichever form A gets (nothing is built)
size_t bis_spmv_partials_bound(const bis_mat *A);
bis_status bis_spmv_trsv_level(bis_ctx *ctx, const bis_mat *T, const double *x, double *y,
                               const double *b, const double *D);
// one step of bis_itrsv: x_new = (b - T x_old) * D_inv.  *form = -1: done, fused into the row-block kernel; otherwise
// x_new = T x_old in the SpMV form of that public number, and the caller finishes the step in place
bis_status bis_spmv_itrsv_step(bis_ctx *ctx, const bis_mat *T, const double *x_old, double *x_new, const double *b,
                               const double *D_inv, int *form);
// rows [ra,rb) of A as a matrix sharing A's arrays (y must be offset by ra)
bis_status bis_mat_row_view(bis_ctx *ctx, const bis_mat *A, int64_t ra,
                            int64_t rb, bis_mat **out);

// internal launchers shared between translation units
bis_status bis_mat_alloc(bis_ctx *ctx, int64_t n_rows, int64_t n_cols,
                         int64_t nnz, bool rp64, bis_mat **out);
bis_status bis_mat_finalize(bis_ctx *ctx, bis_mat *A);
// (the row-block, packed-column, dictionary and x-window forms: bis_spmv_forms.hpp)
// x-window + sliced-ELL dictionary form (bis_spmv_sellwin.hip)
bis_status bis_spmv_sellwin_try(bis_ctx *ctx, bis_mat *A);
int bis_spmv_sellwin_blocks(const bis_mat *A);
int64_t bis_spmv_sellwin_bytes(const bis_mat *A);
int64_t bis_spmv_sellwin_slices(const bis_mat *A);
int bis_spmv_sellwin_format(const bis_mat *A);
bis_status bis_spmv_sellwin_launch(bis_ctx *ctx, const bis_mat *A, const double *x, double *y, int mode, const double *w,
                                   double *partials, const int *stop, int remap_arg, int grid);
void bis_spmv_sellwin_drop(bis_mat *A);
// window + sliced-ELL form with the 8-byte values streamed (bis_spmv_win8.hip, "win8")
// vb: bytes per streamed value -- 8, or 4 for the stream of a matrix flagged f32_exact ("win4", A->w8[1]); one code path
bis_status bis_spmv_win8_try(bis_ctx *ctx, bis_mat *A, int vb = 8);
int bis_spmv_win8_blocks(const bis_mat *A, int vb = 8);
int bis_spmv_win8_rows(const bis_mat *A, int vb = 8);
int64_t bis_spmv_win8_bytes(const bis_mat *A, int vb = 8);
bis_status bis_spmv_win8_launch(bis_ctx *ctx, const bis_mat *A, const double *x, double *y, int mode, const double *w,
                                double *partials, const int *stop, int remap_arg, int grid, int vb = 8);
void bis_spmv_win8_drop(bis_mat *A); // both streams
int bis_spmv_win8_active(const bis_mat *A); // 4 where the 4-byte stream is built and the flag and options still select it, else 8
bis_status bis_spmv_colslab_build(bis_ctx *ctx, const bis_mat *A, int K, std::vector<bis_mat *> &slabs, bool *ok);
void bis_spmv_colslab_free(bis_ctx *ctx, std::vector<bis_mat *> &slabs);
void bis_spmv_colslab_drop(bis_mat *A);
int bis_spmv_remap_arg(int nb);
int bis_spmv_grid(int nb);
size_t bis_spmv_win8_stream_bytes(const bis_mat *A, int vb = 8);
bool bis_spmv_win8_implied(const bis_mat *A, int vb = 8);         // the implied-slot layout was built
double bis_spmv_win8_moved_bytes(const bis_mat *A, int vb = 8);  // bytes a launch moves: the form's arrays, the windows' x granules, y
bool bis_spmv_win8_fast(const bis_mat *A, double ms, int vb = 8); // a launch of ms runs at the stream placement's fast level
void *bis_spmv_win8_swap_stream(bis_mat *A, void *stream, int vb = 8); // returns the buffer that was in use
// free the row-block tables and every SpMV form (not the CRS arrays)
void bis_mat_free_meta(bis_mat *A);
// after the values of A changed in place: drops every structure derived from them (dictionary, code streams, slabs, sweep
// plans); the packed column streams and the x window depend on the pattern only and stay
void bis_mat_values_changed(bis_mat *A);
void bis_trsv_plan_destroy(bis_trsv_plan *p);
void bis_trsm_plan_destroy(bis_trsm_plan *p); // bis_sptrsm.hip
inline bis_trsv_side &bis_trsv_side_of(bis_mat *A, bool backward) { return A->trsv[backward ? 1 : 0]; }
// drops the tiled plans, their `tried` flags and the level plans of both directions; with chains = true the chained plans
// and their flags as well (see bis_trsv_side)
void bis_trsv_drop(bis_mat *A, bool chains);
bool bis_trsv_holds_plans(const bis_mat *A); // some direction holds a level, tiled or chained plan
// `to` has the sparsity pattern of `from` (ILU(0): the factor L and the strict lower triangle of A the elimination was scheduled
// by): it takes over from's level plan (levels, level-sorted rows) instead of analysing the same pattern again.  No-op when
// from has none, to has one, or the plan refers to from's storage (row views).
void bis_trsv_plan_adopt(bis_mat *to, bis_mat *from, bool backward);
bis_status bis_mat_split_strict_impl(bis_ctx *ctx, const bis_mat *A, bis_mat **L_strict,
                                     bis_mat **U_strict, double *D, double *D_inv, bool check_diag);
// bis_mat_ilu0 behind its argument checks; fill = true (bis_iluk.hip): an update applies to every position of a row's
// pattern, whether its current value is zero or not
bis_status bis_mat_ilu0_impl(bis_ctx *ctx, const bis_mat *A, double pivot_tol, double pivot_repl, bis_mat **L_strict,
                             bis_mat **U_strict, double *L_D, double *U_D, bool fill);
// W = A with ascending columns inside each row (bis_ilu0.hip's sort, stable for repeated columns; W is not finalized), and
// per row the position of its first diagonal entry (-1: none) and of its first entry right of the diagonal.  The caller
// destroys W and frees the two device arrays.
bis_status bis_mat_sorted_copy(bis_ctx *ctx, const bis_mat *A, bis_mat **W, int64_t **dpos, int64_t **ustart);
// every off-diagonal entry has its mirror and no row holds a column twice (bis_order.hip: the check of bis_mat_bfs_order).  Blocking.
bis_status bis_mat_pattern_symmetric(bis_ctx *ctx, const bis_mat *A, bool *symmetric);
// tiled natural-order sweep (bis_trsv_tiled.hip); *out stays null when the matrix does not qualify
bis_status bis_trsv_tiled_build(bis_ctx *ctx, const bis_mat *T, bool backward, bis_trsv_tiled **out);
bis_status bis_trsv_tiled_solve(bis_ctx *ctx, bis_trsv_tiled *p, double *x, const double *D, const double *b);
void bis_trsv_tiled_destroy(bis_trsv_tiled *p);
// device-side level analysis of a strictly triangular matrix (bis_analysis.hip); level_out (optional): the level of
// every row, a device array the caller frees
bis_status bis_trsv_analyse_device(bis_ctx *ctx, const bis_mat *T, bool backward, int32_t *perm_dev,
                                   std::vector<int64_t> &level_ptr, int &n_levels, int64_t &max_width,
                                   bool &triangular, int **level_out = nullptr);
// chained sweep (bis_trsv_chain.hip); *out stays null where it does not apply
bis_status bis_trsv_chain_build(bis_ctx *ctx, const bis_mat *T, bool backward, const int *level_dev, int n_levels,
                                bis_trsv_chain **out);
bis_status bis_trsv_chain_solve(bis_ctx *ctx, const bis_mat *T, bis_trsv_chain *p, double *x, const double *D, const double *b);
void bis_trsv_chain_destroy(bis_trsv_chain *p);
int bis_trsv_chain_resident_pairs(const bis_ctx *ctx, bool rp64, bool backward); // wave pairs (= chains in flight) of a full grid
// contiguous independent row blocks of a strictly triangular matrix, in processing order (bis_analysis.hip)
bis_status bis_trsv_blocks_device(bis_ctx *ctx, const bis_mat *T, bool backward, int max_blocks,
                                  std::vector<int64_t> &bounds, int32_t *perm_dev, bool &triangular);
// dependency levels of a strict-lower matrix: host level boundaries + device row list
bis_status bis_trsv_level_sets(bis_ctx *ctx, const bis_mat *T_lower, const std::vector<int64_t> **level_ptr,
                               const int32_t **perm_dev);
