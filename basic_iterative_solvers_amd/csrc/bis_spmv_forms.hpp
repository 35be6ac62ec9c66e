// bis_spmv_forms.hpp -- what the units of the row-block SpMV share: the launch arguments the plan (bis_spmv.hip) hands to a form,
// the state structs that the plan and neighbouring forms read, and each form's try / launch / drop functions.
#pragma once

#include "bis_internal.hpp"

#include <memory>

struct SpmvArgs {
    const void *row_ptr; const int32_t *col; const double *val; const double *x; double *y;
    const int32_t *blk_row; const int64_t *blk_nnz; int nb, nb8; const double *w; double *partials;
    size_t lds_bytes; hipStream_t stream; int mode; int remap_arg = -1; int grid = 0;
    const uint16_t *pk = nullptr; int64_t pk_base = 0; const int32_t *seg_base = nullptr; int col_max = 0; int pk_mode = 0;
    bool wide = false; // 2^29 columns or more: 64-bit x addressing, 32-bit column stream
    const int *stop = nullptr;
    const uint8_t *vcode = nullptr; int64_t vd_base = 0; const double *vdict = nullptr; // value dictionary (pk_mode 1 only)
    bool vd_rm_only = false; // lane-per-row kernel only
    int acc_y = 0;           // row sums start from y (a later column slab)
};

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef unsigned short v4us __attribute__((ext_vector_type(4)));

// x[c]: with fewer than 2^29 columns the byte offset fits 32 bits (one shift,
// scalar base + 32-bit vector offset addressing); WIDE keeps 64-bit arithmetic.
template <bool WIDE>
__device__ __forceinline__ double x_at(const char *xb, int c) {
    if (WIDE) return *reinterpret_cast<const double *>(xb + (int64_t)c * 8);
    return *reinterpret_cast<const double *>(xb + (uint32_t)((uint32_t)c << 3));
}

constexpr int kPkSegs = 8, kPkOffBits = 13, kPkSpan = 1 << kPkOffBits;
constexpr int kPk3Segs = 32, kPk3OffBits = 11; // second format: more, narrower windows (reordered matrices)

// The x-window variant is opt-in (spmv_window=1): measured 1.20-1.33 ms against
// 1.00-1.12 ms for the gather kernel on HPCG-256 (profiles/).
inline int spmv_window_mode() { return bis_opts().spmv_window < 0 ? 0 : bis_opts().spmv_window; }
// 0 off, 1 consecutive form, 2 lane-per-row form for y = A x and the fused dot where the matrix qualifies
inline int spmv_valdict_mode() { return bis_opts().spmv_valdict < 0 ? 2 : bis_opts().spmv_valdict; }

// ---- row-block kernels (bis_spmv_rowblock.hip) ----
int spmv_variant(const SpmvArgs &a);                  // the variant id that the options and the column stream select
const char *rowblock_name(int id, const SpmvArgs &a); // the instance's reported name; nullptr for an unknown id
bool bis_spmv_rowblock_launch(bool rp64, int id, const SpmvArgs &a); // false for an unknown id
void bis_spmv_longrows_launch(bis_ctx *ctx, const bis_mat *A, const double *x, double *y); // spmv_wave_per_row_kernel

// ---- packed columns (bis_spmv_colpack.hip) ----
// Per non-zero a 16-bit code (window | offset) against the column windows of its block: 10 instead of 12 streamed bytes per
// non-zero.  Three instances per matrix: A->pk[0] and A->pk[1] on the row-block tables and bis_valdict::rm_pk.
struct bis_colpack {
    uint16_t *codes = nullptr; // index k - base
    int32_t *seg = nullptr;    // [n_blocks * 8], or * 32 (kind 3)
    int64_t base = 0;
    int kind = 0;              // 1: 8 windows x 8192 columns, 3: 32 windows x 2048 columns
    ~bis_colpack();
};
// Codes for the nb blocks of table tab (tab[b] = first non-zero of block b): kind 1 first, then, where try32, kind 3.  base = the
// first non-zero rounded down to `align`.  probe: look before the build (pk_probe_kernel).
bis_status bis_colpack_build(bis_ctx *ctx, const bis_mat *A, const int64_t *tab, int nb, int align, bool probe, bool try32, bis_colpack **out);
// try to build the packed-column stream of table t (0 plain, 1 fused); A->pk[t].state tells the outcome
bis_status bis_spmv_try_pack(bis_ctx *ctx, bis_mat *A, int t);
void bis_spmv_colpack_drop(bis_mat *A); // both tables

// ---- value dictionary (bis_spmv_valdict.hip) ----
// A matrix with at most 256 distinct values (compared bit for bit) keeps them in a 256-entry table and streams one byte per
// non-zero instead of the 8-byte value.  The CRS values stay authoritative.
struct bis_valdict {
    uint8_t *codes = nullptr;  // [nnz_range + pad], index k - base
    double *table = nullptr;   // [256], ascending bit patterns, unused entries 0
    int64_t base = 0;
    int n = 0;
    // ... or all values EXCEPT the diagonal entries (col == row + view_row0) are at most 255: code 255 then stands for "this
    // row's diagonal value", kept in a per-row array (Anderson: random diagonal, constant hopping).  Lane-per-row form only.
    double *diag_val = nullptr; // [n_rows] when diag
    bool diag = false;
    bool rm_only = false;       // only the lane-per-row kernel can use this dictionary (diag, or the row-block tables have no packed columns)
    // lane-per-row form of the dictionary kernel: blocks of 256 rows with their own packed column stream; rm_state like A->vd.state
    int64_t *rm_nnz = nullptr;  // [rm_blocks + 1] row_ptr at every 256th row
    bis_colpack *rm_pk = nullptr;
    int rm_state = 0, rm_blocks = 0;
    ~bis_valdict();
};
bis_status bis_spmv_try_valdict(bis_ctx *ctx, bis_mat *A, bool consecutive_ok);
bis_status bis_spmv_valdict_try_rowmajor(bis_ctx *ctx, bis_mat *A); // the lane-per-row blocks; rm_state tells the outcome
void bis_spmv_valdict_launch_rowblock(const bis_mat *A, const SpmvArgs &a); // spmv_rowblock_vd_kernel
void bis_spmv_valdict_launch_rowmajor(const bis_mat *A, const SpmvArgs &a); // spmv_rowmajor_vd_kernel
void bis_spmv_valdict_drop(bis_mat *A); // the dictionary and its lane-per-row blocks
// value dictionary, consecutive form: the default variant on the packed stream only, and not as a later column slab's pass
inline bool rowblock_is_vd(int id, const SpmvArgs &a) { return a.vcode && !a.acc_y && !a.vd_rm_only && id == 20 && a.pk_mode == 1; }

// ---- x window (bis_spmv_xwin.hip); A->xw is null unless the form is built ----
bis_status bis_spmv_build_window(bis_ctx *ctx, bis_mat *A);
void bis_spmv_xwin_launch(const bis_mat *A, const SpmvArgs &a);
void bis_spmv_xwin_drop(bis_mat *A);
