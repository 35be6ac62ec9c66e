// bis_spmv.hip -- the SpMV plan: which form y = A x takes on a matrix (spmv_resolve), its launch (spmv_launch_plan) and what the
// library reports of it (spmv_report).  The forms live in units of their own (bis_spmv_forms.hpp; bis_spmv_sellwin.hip,
// bis_spmv_win8.hip, bis_spmv_slab.hip); this unit keeps the column-slab driver, which runs on the plan itself.
//
// The forms of y = A x, in the order of precedence in which spmv_resolve chooses (the only place that does); "dictionary":
// the matrix has a value dictionary (spmv_valdict >= 1) -- "lane per row" needs spmv_valdict 2 (the default) --; "default
// variant": spmv_variant -1 or 20.  Modes: plain, fused dot, sweep level.  Public form number: bis_mat_spmv_stream_info.
//
//   form (name reported)             chosen when                                            streams per non-zero      fused-dot partials
//   long rows (spmv_wave_per_row_    a block's products and the longest row exceed 64 KiB   12 B                      -- (plain only: fused dot
//     kernel), public 0              of LDS                                                                           and sweep level refuse)
//   x-window (spmv_window_kernel),   spmv_window 1 and every block touches <= 128 tiles;    10 B (2-byte position     4 per block (plain table)
//     public 0                       plain, fused                                           in the window)
//   sellwin ("sellwin fmt=F"),       dictionary, lane per row, default variant,             fmt 0, 1: 3 B; 2: 2 B;    1 per 64-row slice
//     public 4 / 5                   spmv_sellwin != 0, the plan applies; plain, fused      3: 1 B; 4: 4 B per ROW
//   rowmajor (spmv_rowmajor_vd_      dictionary, lane per row, default variant, rows <= 40  3 B                       4 per 256 rows
//     kernel), public 2 / 3          entries, <= 8 (32) column windows per 256 rows; all
//   win4 ("win4 rows=R"), public 8   no dictionary, the matrix is flagged fp32-exact        6 B (4 B + a descriptor   4 per block of 256 R rows
//                                    (bis_mat_round_f32), spmv_win4 != 0, spmv_win8 != 0,   per chunk: implied slots)
//                                    default variant, the plan applies; plain, fused
//   win8 ("win8 rows=R"), public 6   no dictionary, spmv_win8 != 0, default variant, the    10 B (8 B + a descriptor  4 per block of 256 R rows
//                                    plan applies (<= 12 % padding); plain, fused           per chunk: implied slots)
//   colslab ("colslab K=k"),         no dictionary, < 2^29 columns, spmv_colslab != 0,      12 B (10 B where every    4 per block of the last
//     public 7                       variant -1 / 20 / 41, colslab_try's conditions and     slab packs) + 16 B per    slab (fused table)
//                                    trial; plain, fused                                    row and later pass
//   rowblock_vd (spmv_rowblock_vd_   dictionary with consecutive codes, variant 20 on the   3 B                       4 per block (fused table)
//     kernel), public 1              8-window packed stream; all
//   rowblock (spmv_rowblock_kernel   everything else; all                                   10 B packed, 12 B         4 per block (fused table)
//     U= PK= BR=), public 0
//   (+ 8 B per row where the dictionary keeps the diagonal's values per row: public 3 and 5)
#include "bis_spmv_forms.hpp"

#include <algorithm>
#include <vector>

namespace {

constexpr int kFusedThreads = 256; // threads per workgroup of every row-block variant (the fused dot writes one partial per wave)

// "sellwin fmt=F", "win8 rows=R", "colslab K=k", "win4 rows=R" (F 0..4, R 1..4, k up to 32)
const char *form_name(int kind, int v) {
    static const std::vector<std::string> names[4] = {
        [] { std::vector<std::string> n; for (int i = 0; i <= 4; ++i) n.push_back("sellwin fmt=" + std::to_string(i)); return n; }(),
        [] { std::vector<std::string> n; for (int i = 0; i <= 4; ++i) n.push_back("win8 rows=" + std::to_string(i)); return n; }(),
        [] { std::vector<std::string> n; for (int i = 0; i <= 32; ++i) n.push_back("colslab K=" + std::to_string(i)); return n; }(),
        [] { std::vector<std::string> n; for (int i = 0; i <= 4; ++i) n.push_back("win4 rows=" + std::to_string(i)); return n; }()};
    const std::vector<std::string> &t = names[kind];
    return t[(size_t)std::max(0, std::min(v, (int)t.size() - 1))].c_str();
}

} // namespace

// default: select tree (see the tuning record in DESIGN.md section 4)
static int spmv_packed_mode() { return bis_opts().spmv_packed < 0 ? 1 : bis_opts().spmv_packed; }

// The packed stream of table t, built at the first use unless bis_mat_finalize
// already did (a cache on the matrix: the const handle of the SpMV entry points
// is cast away here only).  Identical tables (packed default) share stream 1.
static bis_status ensure_packed(bis_ctx *ctx, const bis_mat *A_c, int t, SpmvArgs *a) {
    bis_mat *A = const_cast<bis_mat *>(A_c);
    a->pk_mode = 0;
    a->wide = A->n_cols >= ((int64_t)1 << 29);
    if (a->wide || !spmv_packed_mode() || A->nnz == 0) return BIS_OK;
    if (A->chunk_nnz == A->chunk_f) t = 1;
    if (bis_status st = bis_spmv_try_pack(ctx, A, t)) return st;
    if (A->pk[t].state == 1) {
        const bis_colpack *pk = A->pk[t].p;
        a->pk = pk->codes; a->pk_base = pk->base; a->seg_base = pk->seg;
        a->col_max = (int)std::max<int64_t>(A->n_cols - 1, 0);
        a->pk_mode = pk->kind == 3 ? 3 : (spmv_packed_mode() == 2 ? 2 : 1);
    }
    if (spmv_valdict_mode()) { // value dictionary: the consecutive kernel rides on the packed stream of the row-block table,
                               // the lane-per-row kernel brings its own
        if (bis_status st = bis_spmv_try_valdict(ctx, A, a->pk_mode == 1)) return st;
        if (A->vd.state == 1) { a->vcode = A->vd.p->codes; a->vd_base = A->vd.p->base; a->vdict = A->vd.p->table; a->vd_rm_only = A->vd.p->rm_only; }
    }
    return BIS_OK;
}

// ---- the form of a matrix' SpMV: resolved in ONE place (the table in the file header); launches and reports read the plan ----

enum SpmvForm { kFormLongRows, kFormWindow, kFormSellwin, kFormRowmajor, kFormWin4, kFormWin8, kFormColslab, kFormRowblockVd, kFormRowblock };

struct SpmvPlan {
    SpmvForm form = kFormRowblock;
    SpmvArgs a{};          // tables, block map (nb, remap_arg, grid), column stream, dictionary; the caller adds x, y, w, partials, stop
    int n_partials = 0;    // partials the fused dot writes (mode 1)
    const char *name = ""; // what bis_mat_spmv_kernel reports: a static string
};

static bis_status spmv_resolve(bis_ctx *ctx, const bis_mat *A_c, int mode, SpmvPlan *p, bool pass = false);
static bis_status spmv_launch_plan(bis_ctx *ctx, const bis_mat *A, const SpmvPlan &p);

// ---- column slabs (bis_spmv_slab.hip): K passes of the row-block kernel, each gathering from an x slice that fits the L2 ----

void bis_spmv_colslab_drop(bis_mat *A) {
    if (A->cs.slabs) {
        for (bis_mat *B : *A->cs.slabs) { // (no context at hand: what bis_mat_destroy does for a matrix that owns its arrays)
            bis_mat_free_meta(B);
            hipFree(B->row_ptr); hipFree(B->col); hipFree(B->val);
            delete B;
        }
        delete A->cs.slabs;
        A->cs.slabs = nullptr;
    }
    A->cs.state = 0;
    A->cs.trial_ms[0] = A->cs.trial_ms[1] = 0.0;
}

// one pass of the row-block kernel over matrix B (A itself, or one of its slabs); a fused dot's partials go to `partials`
static bis_status rowblock_pass(bis_ctx *ctx, const bis_mat *B, const double *x, double *y, const double *w, double *partials,
                                int acc_y, const int *stop) {
    SpmvPlan p;
    if (bis_status st = spmv_resolve(ctx, B, w ? 1 : 0, &p, true)) return st;
    p.a.x = x; p.a.y = y; p.a.w = w; p.a.partials = partials; p.a.stop = stop;
    p.a.acc_y = acc_y;
    return spmv_launch_plan(ctx, B, p);
}

static bis_status colslab_passes(bis_ctx *ctx, const bis_mat *A, const double *x, double *y, const double *w, double *partials,
                                 const int *stop) {
    const std::vector<bis_mat *> &S = *A->cs.slabs;
    for (size_t k = 0; k < S.size(); ++k) // (the fused dot rides on the last pass: y is complete there)
        if (bis_status st = rowblock_pass(ctx, S[k], x, y, k + 1 == S.size() ? w : nullptr, partials, k > 0 ? 1 : 0, stop)) return st;
    return BIS_OK;
}

// Builds the slabs where the plan applies: 32-bit row pointers, not a row view, rows of at most the LDS budget, a column stream
// that did NOT pack (a matrix whose row blocks each touch at most 8 windows of 8192 columns has the locality the slabs would
// make), an x of more than 6 MiB, ascending rows.  Default: K = x's bytes / 2 MiB (2..32) and a trial -- three timed launches of
// the one pass and of the K passes on a scratch x -- keeps the slabs only where they are at least 15 % faster.
static bis_status colslab_try(bis_ctx *ctx, bis_mat *A, bool packed) {
    if (A->cs.state != 0) return BIS_OK;
    A->cs.state = -1;
    const int opt = bis_opts().spmv_colslab;
    const bool forced = opt >= 2;
    if (opt == 0 || A->rp64 || A->view || A->n_rows == 0 || A->nnz == 0) return BIS_OK;
    if (!forced && (packed || 8 * A->n_cols <= (int64_t)6 << 20 || A->nnz < ((int64_t)1 << 22))) return BIS_OK;
    if (sizeof(double) * (size_t)((int64_t)A->chunk_f + A->max_row_nnz + 8) > 64 * 1024) return BIS_OK;
    int K = forced ? std::min(opt, 32) : (int)std::min<int64_t>(32, std::max<int64_t>(2, (8 * A->n_cols + ((int64_t)2 << 20) - 1) / ((int64_t)2 << 20)));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (int64_t)free_b < 16 * A->nnz + ((int64_t)8 << 30)) { (void)hipGetLastError(); return BIS_OK; }
    auto *slabs = new std::vector<bis_mat *>();
    bool ok = false;
    bis_status st = bis_spmv_colslab_build(ctx, A, K, *slabs, &ok);
    if (st != BIS_OK || !ok) { delete slabs; return st; }
    A->cs.slabs = slabs;
    if (!forced) { // the trial
        double *xs = nullptr, *ys = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool good = hipMalloc(&xs, sizeof(double) * (size_t)A->n_cols) == hipSuccess && hipMalloc(&ys, sizeof(double) * (size_t)A->n_rows) == hipSuccess &&
                    hipMemsetAsync(xs, 0, sizeof(double) * (size_t)A->n_cols, ctx->stream) == hipSuccess &&
                    hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
        float ms[2] = {0.f, 0.f};
        for (int which = 0; which < 2 && good && st == BIS_OK; ++which) {
            for (int rep = 0; rep < 5 && st == BIS_OK; ++rep) {
                if (rep == 2) good = good && hipEventRecord(ev[0], ctx->stream) == hipSuccess;
                st = which ? colslab_passes(ctx, A, xs, ys, nullptr, nullptr, nullptr) : rowblock_pass(ctx, A, xs, ys, nullptr, nullptr, 0, nullptr);
            }
            good = good && hipEventRecord(ev[1], ctx->stream) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
                   hipEventElapsedTime(&ms[which], ev[0], ev[1]) == hipSuccess;
        }
        if (ev[0]) hipEventDestroy(ev[0]);
        if (ev[1]) hipEventDestroy(ev[1]);
        hipFree(xs); hipFree(ys);
        (void)hipGetLastError();
        A->cs.trial_ms[0] = ms[0] / 3.0;
        A->cs.trial_ms[1] = ms[1] / 3.0;
        if (st != BIS_OK || !good || !(ms[1] < 0.85f * ms[0])) {
            const double keep[2] = {A->cs.trial_ms[0], A->cs.trial_ms[1]};
            bis_spmv_colslab_drop(A);
            A->cs.state = -1;
            A->cs.trial_ms[0] = keep[0]; A->cs.trial_ms[1] = keep[1];
            return st;
        }
    }
    A->cs.state = 1;
    return BIS_OK;
}

// The one place that reads the form-selecting options together with the matrix' build states and runs the lazy builds.
// mode 0: y = A x; 1: with the fused dot (its own block table); 2: one triangular-sweep level (lane-per-row dictionary form or
// row-block kernel only).  pass: one plain row-block pass over a slab (or over A: the slabs' trial).  Precedence as in the table
// of the file header; the builds run in that order too, so the first SpMV's device allocations land where they always did.
static bis_status spmv_resolve(bis_ctx *ctx, const bis_mat *A_c, int mode, SpmvPlan *p, bool pass) {
    bis_mat *A = const_cast<bis_mat *>(A_c); // (the forms are a cache on the matrix: the entry points' const handle is cast away here only)
    *p = SpmvPlan{};
    SpmvArgs &a = p->a;
    const bool window = !pass && mode != 2 && A->xw && spmv_window_mode();
    const bool use_f = mode == 1 && !window; // fused epilogue: its own table
    a.lds_bytes = sizeof(double) * (size_t)((int64_t)(use_f ? A->chunk_f : A->chunk_nnz) + A->max_row_nnz + 8);
    if (!pass && a.lds_bytes > 64 * 1024) {
        if (mode == 1) { ctx->err = "bis_spmv: fused dot unsupported for very long rows"; return BIS_ERR_UNSUPPORTED; }
        if (mode == 2) { ctx->err = "sptrsv level: row too long for the streaming kernel"; return BIS_ERR_UNSUPPORTED; }
        p->form = kFormLongRows;
        p->name = "spmv_wave_per_row_kernel";
        return BIS_OK;
    }
    auto block_map = [&a](int nb) {
        a.nb = nb;
        a.nb8 = (nb + 7) & ~7;
        a.remap_arg = bis_spmv_remap_arg(nb);
        a.grid = bis_spmv_grid(nb);
    };
    a.row_ptr = A->row_ptr; a.col = A->col; a.val = A->val;
    a.blk_row = use_f ? A->blkf_row : A->blk_row;
    a.blk_nnz = use_f ? A->blkf_nnz : A->blk_nnz;
    a.stream = ctx->stream;
    a.mode = mode;
    block_map(use_f ? A->n_blocks_f : A->n_blocks);
    if (window) {
        p->form = kFormWindow;
        p->n_partials = mode == 1 ? a.nb * 4 : 0; // 256-thread workgroups: 4 waves
        p->name = "spmv_window_kernel";
        return BIS_OK;
    }
    if (bis_status st = ensure_packed(ctx, A, use_f ? 1 : 0, &a)) return st;
    if (pass) {
        a.vcode = nullptr; // (the plain row-block kernel: the value-dictionary kernel has no accumulating form)
    } else {
        const int v = bis_opts().spmv_variant;
        const bool lane_per_row = a.vcode && spmv_valdict_mode() >= 2 && (v < 0 || v == 20);
        if (mode != 2 && lane_per_row && bis_opts().spmv_sellwin != 0) {
            if (bis_status st = bis_spmv_sellwin_try(ctx, A)) return st;
            if (const int nb = bis_spmv_sellwin_blocks(A)) {
                block_map(nb);
                p->form = kFormSellwin;
                p->n_partials = mode == 1 ? (int)bis_spmv_sellwin_slices(A) : 0; // one per 64-row slice
                p->name = form_name(0, bis_spmv_sellwin_format(A));
                return BIS_OK;
            }
        }
        if (lane_per_row) {
            if (bis_status st = bis_spmv_valdict_try_rowmajor(ctx, A)) return st;
            if (A->vd.p->rm_state == 1) {
                block_map(A->vd.p->rm_blocks);
                p->form = kFormRowmajor;
                p->n_partials = mode == 1 ? A->vd.p->rm_blocks * 4 : 0;
                p->name = "spmv_rowmajor_vd_kernel";
                return BIS_OK;
            }
        }
        // (a matrix with a value dictionary keeps its dictionary kernels: 3 bytes per non-zero)
        // (win4: only a matrix that bis_mat_round_f32 flagged; where the plan does not apply -- it is win8's -- the successors follow)
        if (mode != 2 && !a.vcode && A->f32_exact && bis_opts().spmv_win4 != 0 && bis_opts().spmv_win8 != 0 && (v < 0 || v == 20)) {
            if (bis_status st = bis_spmv_win8_try(ctx, A, 4)) return st;
            if (const int nb = bis_spmv_win8_blocks(A, 4)) {
                block_map(nb);
                p->form = kFormWin4;
                p->n_partials = mode == 1 ? nb * 4 : 0; // one per wave
                p->name = form_name(3, bis_spmv_win8_rows(A, 4));
                return BIS_OK;
            }
        }
        if (mode != 2 && !a.vcode && bis_opts().spmv_win8 != 0 && (v < 0 || v == 20)) {
            if (bis_status st = bis_spmv_win8_try(ctx, A)) return st;
            if (const int nb = bis_spmv_win8_blocks(A)) {
                block_map(nb);
                p->form = kFormWin8;
                p->n_partials = mode == 1 ? nb * 4 : 0; // one per wave
                p->name = form_name(1, bis_spmv_win8_rows(A));
                return BIS_OK;
            }
        }
        if (mode != 2 && !a.vcode && !a.wide && bis_opts().spmv_colslab != 0 && (v < 0 || v == 20 || v == 41)) {
            if (bis_status st = colslab_try(ctx, A, a.pk_mode != 0)) return st;
            if (A->cs.state == 1) {
                p->form = kFormColslab;
                p->n_partials = mode == 1 ? A->cs.slabs->back()->n_blocks_f * (kFusedThreads / 64) : 0; // the last pass writes them
                p->name = form_name(2, (int)A->cs.slabs->size());
                return BIS_OK;
            }
        }
        if (mode != 2 && bis_opts().spmv_lds_pad > 0) a.lds_bytes += (size_t)bis_opts().spmv_lds_pad;
    }
    const int id = spmv_variant(a);
    const bool vd = rowblock_is_vd(id, a);
    p->name = vd ? "spmv_rowblock_vd_kernel" : rowblock_name(id, a);
    if (!p->name) { ctx->err = "bis_spmv: unknown BIS_SPMV_VARIANT"; return BIS_ERR_INVALID; }
    p->form = vd ? kFormRowblockVd : kFormRowblock;
    p->n_partials = mode == 1 ? a.nb * (kFusedThreads / 64) : 0;
    return BIS_OK;
}

// launches what the plan names; x, y, w, partials (a sweep level: b and D in their place) and stop are in p.a
static bis_status spmv_launch_plan(bis_ctx *ctx, const bis_mat *A, const SpmvPlan &p) {
    const SpmvArgs &a = p.a;
    switch (p.form) {
    case kFormLongRows:
        bis_spmv_longrows_launch(ctx, A, a.x, a.y);
        return BIS_OK;
    case kFormWindow:
        bis_spmv_xwin_launch(A, a);
        return BIS_OK;
    case kFormSellwin:
        return bis_spmv_sellwin_launch(ctx, A, a.x, a.y, a.mode, a.w, a.partials, a.stop, a.remap_arg, a.grid);
    case kFormWin4:
        return bis_spmv_win8_launch(ctx, A, a.x, a.y, a.mode, a.w, a.partials, a.stop, a.remap_arg, a.grid, 4);
    case kFormWin8:
        return bis_spmv_win8_launch(ctx, A, a.x, a.y, a.mode, a.w, a.partials, a.stop, a.remap_arg, a.grid);
    case kFormRowmajor:
        bis_spmv_valdict_launch_rowmajor(A, a);
        return BIS_OK;
    case kFormColslab:
        return colslab_passes(ctx, A, a.x, a.y, a.w, a.partials, a.stop);
    case kFormRowblockVd:
        bis_spmv_valdict_launch_rowblock(A, a);
        return BIS_OK;
    case kFormRowblock:
        bis_spmv_rowblock_launch(A->rp64, spmv_variant(a), a);
        return BIS_OK;
    }
    return BIS_ERR_INVALID;
}

// Upper bound on the partials one fused SpMV of A writes, over every form spmv_resolve can choose -- from the matrix' shape
// and block tables alone, so that it holds before any form is built.  Row-block kernel: one per wave of a block of the fused
// table (4; the 16 dates from workgroups of up to 1024 threads and is kept); x-window kernel: 4 per block of the plain table.
// The forms on blocks of kSwRows R rows, R = 1, 2, 4 (lane-per-row dictionary: R = 1, 4 per block; win8 / win4: 4 per block; sellwin:
// one per slice of kSwRows / 4 rows) write at most ceil(n / (kSwRows R)) 4 R <= n / (kSwRows / 4) + 4 kSwMaxR.  The slabs'
// last pass runs on a table of no more blocks than A's own.
size_t bis_spmv_partials_bound(const bis_mat *A) {
    const size_t rows = (size_t)std::max<int64_t>(A->n_rows, 0);
    return std::max({(size_t)A->n_blocks_f * 16, (size_t)A->n_blocks * 4, rows / (kSwRows / 4) + 4 * (size_t)kSwMaxR});
}

// internal: y = A x, optionally partials[b] = sum_{r in block b} y[r]*w[r]
// (n_partials returns the number of partials written; 0 if not fused).
bis_status bis_spmv_launch(bis_ctx *ctx, const bis_mat *A, const double *x, double *y,
                           const double *w, int *n_partials, size_t partials_off) {
    if (n_partials) *n_partials = 0;
    if (A->n_rows == 0) return BIS_OK;
    SpmvPlan p;
    if (bis_status st = spmv_resolve(ctx, A, w ? 1 : 0, &p)) return st;
    if (w && partials_off + (size_t)p.n_partials > ctx->partials_cap) {
        ctx->err = "bis_spmv: partials buffer too small (internal)";
        return BIS_ERR_INVALID;
    }
    p.a.x = x; p.a.y = y; p.a.w = w; p.a.partials = ctx->partials + partials_off;
    p.a.stop = ctx->spmv_stop; // a device schedule (bis_cg_iterate, bis_stat_iterate) is enqueuing: no-op once its stop flag is set
    bis_prof_begin(ctx);
    const bis_status st = spmv_launch_plan(ctx, A, p);
    bis_prof_end(ctx);
    if (st != BIS_OK) return st;
    BIS_HIP_CHECK(ctx, hipGetLastError());
    if (n_partials) *n_partials = p.n_partials;
    const_cast<bis_mat *>(A)->spmv_kernel[w ? 1 : 0] = p.name; // (bis_mat_spmv_kernel)
    return BIS_OK;
}

// internal: one triangular-sweep level on the row range a view T covers:
// y[r] = (b[r] - (T x)[r]) / D[r]  (y, b, D already offset to the view's first row)
bis_status bis_spmv_trsv_level(bis_ctx *ctx, const bis_mat *T, const double *x, double *y,
                               const double *b, const double *D) {
    if (T->n_rows == 0) return BIS_OK;
    SpmvPlan p;
    if (bis_status st = spmv_resolve(ctx, T, 2, &p)) return st;
    p.a.x = x; p.a.y = y; p.a.w = b; p.a.partials = const_cast<double *>(D);
    p.a.stop = ctx->spmv_stop;
    if (bis_status st = spmv_launch_plan(ctx, T, p)) return st;
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

extern "C" {

const char *bis_mat_spmv_kernel(const bis_mat *A, int fused) { return A ? A->spmv_kernel[fused ? 1 : 0] : ""; }

bis_status bis_spmv(bis_ctx *ctx, const bis_mat *A, const double *x, double *y) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && (A->n_rows == 0 || (x && y)), "bis_spmv: bad arguments");
    BIS_REQUIRE(ctx, x != y, "bis_spmv: x and y must not alias");
    return bis_spmv_launch(ctx, A, x, y, nullptr, nullptr);
}

} // extern "C"

// What the plain SpMV of A streams: the plan's form (and sellwin format) -> col_bytes, val_bytes, n_dict and the public form
// number (include/bis_hip.h).  sellwin's formats: 0, 1 a 2-byte window slot and a 1-byte value code per non-zero; 2 one 16-bit
// code (slot : 13 | value index : 3); 3 one byte, the index of the non-zero's (column - row, value) pair; 4 a 32-bit mask of
// pairs per ROW.  win8 and win4 keep col_bytes 2 also with implied slots (bis_mat_win8_layout tells the layouts apart).
struct SpmvReport { int col_bytes, val_bytes, n_dict, form; };

static bis_status spmv_report(bis_ctx *ctx, const bis_mat *A, SpmvPlan *p, SpmvReport *r) {
    if (bis_status st = spmv_resolve(ctx, A, 0, p)) return st;
    switch (p->form) {
    case kFormLongRows: *r = {4, 8, 0, 0}; break;
    case kFormWindow: *r = {2, 8, 0, 0}; break; // (16-bit positions in the block's x window)
    case kFormRowblock: *r = {p->a.pk_mode ? 2 : 4, 8, 0, 0}; break;
    case kFormRowblockVd: *r = {2, 1, A->vd.p->n, 1}; break;
    case kFormRowmajor: *r = {2, 1, A->vd.p->n, A->vd.p->diag ? 3 : 2}; break;
    case kFormSellwin: {
        static const int col_val[5][2] = {{2, 1}, {2, 1}, {2, 0}, {1, 0}, {0, 0}}; // val_bytes 0: the value index shares the column code
        const int fmt = bis_spmv_sellwin_format(A);
        *r = {col_val[fmt][0], col_val[fmt][1], A->vd.p->n, A->vd.p->diag ? 5 : 4};
        break;
    }
    case kFormWin4: *r = {2, 4, 0, 8}; break;
    case kFormWin8: *r = {2, 8, 0, 6}; break;
    case kFormColslab: {
        bool all_packed = true;
        for (const bis_mat *B : *A->cs.slabs) {
            SpmvPlan pb;
            if (bis_status st = spmv_resolve(ctx, B, 0, &pb, true)) return st;
            all_packed = all_packed && (pb.a.pk_mode != 0 || B->nnz == 0);
        }
        *r = {all_packed ? 2 : 4, 8, (int)A->cs.slabs->size(), 7}; // (n_dict: the number of slabs)
        break;
    }
    }
    return BIS_OK;
}

// internal (bis_itrsv.hip): one step x_new = (b - T x_old) * D_inv of the iterative triangular solve.  Where the plain SpMV
// of T resolves to the CRS-value row-block kernel, that kernel runs with the step as its epilogue (MODE 3: the product is
// never written and read back) and *form = -1; every other form -- the wave-per-row and x-window kernels, the dictionary
// forms, win8 / win4, column slabs -- runs as it is, T x_old into x_new, *form = its public number (bis_mat_spmv_stream_info), and
// the caller's epilogue kernel finishes the step in place.
bis_status bis_spmv_itrsv_step(bis_ctx *ctx, const bis_mat *T, const double *x_old, double *x_new, const double *b,
                               const double *D_inv, int *form) {
    SpmvPlan p;
    SpmvReport r{};
    if (bis_status st = spmv_report(ctx, T, &p, &r)) return st;
    if (p.form != kFormRowblock) {
        *form = r.form;
        return bis_spmv_launch(ctx, T, x_old, x_new, nullptr, nullptr);
    }
    *form = -1;
    p.a.mode = 3;
    p.a.x = x_old; p.a.y = x_new; p.a.w = b; p.a.partials = const_cast<double *>(D_inv);
    p.a.stop = ctx->spmv_stop;
    if (bis_status st = spmv_launch_plan(ctx, T, p)) return st;
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

extern "C" {

bis_status bis_mat_spmv_stream_info(bis_ctx *ctx, const bis_mat *A, int *col_bytes, int *val_bytes, int *n_dict, int *form) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A, "bis_mat_spmv_stream_info: bad arguments");
    SpmvPlan p;
    SpmvReport r{};
    if (bis_status st = spmv_report(ctx, A, &p, &r)) return st;
    if (col_bytes) *col_bytes = r.col_bytes;
    if (val_bytes) *val_bytes = r.val_bytes;
    if (n_dict) *n_dict = r.n_dict;
    if (form) *form = r.form;
    return BIS_OK;
}

bis_status bis_mat_spmv_streamed_bytes(bis_ctx *ctx, const bis_mat *A, int64_t *bytes) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && bytes, "bis_mat_spmv_streamed_bytes: bad arguments");
    SpmvPlan p;
    SpmvReport r{};
    if (bis_status st = spmv_report(ctx, A, &p, &r)) return st;
    const int64_t rp = A->rp64 ? 8 : 4;
    // what the row-block kernel streams of a matrix B: columns and values, row pointers, block table (and window bases)
    auto rowblock_bytes = [&](const bis_mat *B) {
        return (int64_t)(r.col_bytes + r.val_bytes) * B->nnz + rp * (B->n_rows + 1) + (int64_t)B->n_blocks * (12 + (r.col_bytes == 2 ? 32 : 0));
    };
    int64_t b = 8 * A->n_cols + 8 * A->n_rows; // x once, y once
    switch (p.form) {
    case kFormLongRows: b += 12 * A->nnz + rp * (A->n_rows + 1); break;
    case kFormWindow: b += 10 * A->nnz + rp * (A->n_rows + 1) + (int64_t)A->n_blocks * 16; break; // (and 4 bytes per tile a block touches)
    case kFormRowblock: b += rowblock_bytes(A); break;
    case kFormRowblockVd: b += rowblock_bytes(A) + 2048; break;
    case kFormRowmajor: b += 3 * A->nnz + rp * (A->n_rows + 1) + (int64_t)A->vd.p->rm_blocks * (A->vd.p->rm_pk->kind == 3 ? 128 : 32) + 2048; break;
    case kFormSellwin: b += bis_spmv_sellwin_bytes(A); break;
    case kFormWin4: b += bis_spmv_win8_bytes(A, 4); break;
    case kFormWin8: b += bis_spmv_win8_bytes(A); break;
    case kFormColslab: // the slabs' CRS copies, and y read and written again by every pass after the first
        for (const bis_mat *B : *A->cs.slabs) b += rowblock_bytes(B);
        b += 16 * A->n_rows * ((int64_t)A->cs.slabs->size() - 1);
        break;
    }
    if (r.form == 3 || r.form == 5) b += 8 * A->n_rows; // the per-row diagonal values
    *bytes = b;
    return BIS_OK;
}

void bis_mat_colslab_info(const bis_mat *A, int *slabs, double *one_pass_ms, double *slab_passes_ms) {
    if (slabs) *slabs = (A && A->cs.state == 1 && A->cs.slabs) ? (int)A->cs.slabs->size() : 0;
    if (one_pass_ms) *one_pass_ms = A ? A->cs.trial_ms[0] : 0.0;
    if (slab_passes_ms) *slab_passes_ms = A ? A->cs.trial_ms[1] : 0.0;
}

bis_status bis_compute_residual(bis_ctx *ctx, const bis_mat *A, const double *x, const double *b,
                                double *res, double *tmp) {
    // kernels.hpp:155-162: tmp = A x ; res = b - tmp
    bis_status st = bis_spmv(ctx, A, x, tmp);
    if (st != BIS_OK) return st;
    return bis_subtract_vectors(ctx, res, b, tmp, A->n_rows, 1.0);
}

} // extern "C"
