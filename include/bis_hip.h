/*
 * bis_hip.h -- C ABI of the MI355X (gfx950) implementation of the
 * SpMV + preconditioner-apply + BLAS-1 hot path of
 * DanecLacey/basic_iterative_solvers.
 *
 * This is the drop-in boundary: every entry point replaces one free function
 * of the reference's operator surface (kernels.hpp / sparse_matrix.hpp /
 * methods/jacobi.hpp) or one step of its accelerator plugin protocol (the
 * SMAX seam: utilities/smax_helpers.hpp, kernels.hpp:44-52).  The reference
 * interface each function replaces is cited as file:line relative to the
 * reference tree.  Signatures are plain C: opaque handles, raw device
 * pointers (`double *` obtained from bis_vec_alloc, exactly where the
 * reference passes `double *` from `new double[N]`), sizes and scalars.
 * No C++/torch types cross this boundary.
 *
 * Conventions
 *   - every function returns a bis_status (0 = BIS_OK); bis_last_error()
 *     gives the message.  The C++ host layer (basic_iterative_solvers_amd/
 *     host/) restores the reference's `void` + exit(EXIT_FAILURE) convention
 *     (common.hpp:382-396).
 *   - one host thread per context; kernels are ordered on the context's HIP
 *     stream; only functions that return a host scalar (bis_dot,
 *     bis_euclidean_vec_norm, downloads, bis_sync) block.
 *   - vector arguments may alias exactly where the reference's callers alias
 *     them: result==operand for the elementwise
 *     kernels, x==b for the triangular solves, output==input for
 *     bis_apply_preconditioner.
 *   - there is NO CPU fallback: if no gfx950 device is usable the context
 *     cannot be created and every entry point fails with BIS_ERR_NO_DEVICE.
 */
#ifndef BIS_HIP_H
#define BIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIS_API __attribute__((visibility("default")))

typedef int bis_status;
enum {
    BIS_OK = 0,
    BIS_ERR_NO_DEVICE = 1,   /* no usable HIP device / context missing */
    BIS_ERR_INVALID = 2,     /* bad argument (null handle, negative size ...) */
    BIS_ERR_HIP = 3,         /* a HIP runtime call failed */
    BIS_ERR_ZERO_DIAG = 4,   /* SanityChecker::zero_diag, common.hpp:388-391 */
    BIS_ERR_NO_DIAG = 5,     /* SanityChecker::no_diag,   common.hpp:393-396 */
    BIS_ERR_UNSUPPORTED = 6, /* e.g. a row longer than the kernel supports */
    BIS_ERR_COMM = 7,        /* RCCL / halo-exchange failure */
    BIS_ERR_SYNC = 8         /* a device-side wait gave up (lost hand-off in a
                                triangular sweep): results of the work queued
                                since the last blocking call are invalid */
};

/* PrecondType, common.hpp:38-47 (same ordinals). */
enum {
    BIS_PC_NONE = 0,
    BIS_PC_JACOBI = 1,
    BIS_PC_GAUSS_SEIDEL = 2,
    BIS_PC_BACKWARDS_GAUSS_SEIDEL = 3,
    BIS_PC_SYMMETRIC_GAUSS_SEIDEL = 4,
    BIS_PC_TWO_STAGE_GS = 5,
    BIS_PC_SYMMETRIC_TWO_STAGE_GS = 6,
    BIS_PC_ILU0 = 7,
    /* not in the reference: ILU(0) whose two triangular solves are bis_itrsv with inner_iters steps each */
    BIS_PC_ILU0_ITER = 8,
    /* not in the reference: factorized sparse approximate inverse, M^-1 = Gt G with the factors of bis_mat_fsai */
    BIS_PC_FSAI = 9,
    /* not in the reference: aggregation multigrid, one cycle of a bis_mg hierarchy (bis_mg_create; the V-cycle unless
     * bis_mg_set_cycle chose another) */
    BIS_PC_MG = 10,
    /* not in the reference: block Jacobi, the inverted dense diagonal blocks of a bis_bj handle (bis_bj_create) */
    BIS_PC_BLOCK_JACOBI = 11
};

typedef struct bis_ctx bis_ctx; /* device + stream + scratch (SMAX::Interface
                                   role, preprocessing.hpp:52-65) */
typedef struct bis_mat bis_mat; /* device-resident MatrixCRS,
                                   sparse_matrix.hpp:59-179 */

/* ---- context ------------------------------------------------------------ */
/* `stream` is a hipStream_t to run on (NULL: the context creates its own). */
BIS_API bis_status bis_ctx_create(int device, void *stream, bis_ctx **out);
BIS_API bis_status bis_ctx_destroy(bis_ctx *ctx);
BIS_API const char *bis_last_error(const bis_ctx *ctx);
BIS_API bis_status bis_sync(bis_ctx *ctx);
BIS_API void *bis_ctx_stream(bis_ctx *ctx);
/* "gfx950", CU count, HBM bytes -- for logs and the bench JSON. */
BIS_API bis_status bis_device_info(bis_ctx *ctx, char *arch, size_t arch_len,
                                   int *n_cus, int64_t *hbm_bytes);
/* Tuning knobs, process-wide: "spmv_variant", "spmv_window", "spmv_chunk",
 * "spmv_valdict" (0: no value dictionary, see bis_mat_spmv_stream_info),
 * "trsv_grid" (-1 = default), "force_rp64" (1: 64-bit row pointers at any
 * size), "trsv_tiled" (natural-order triangular sweeps: -1 = the tiled sweep
 * where its plan can be built on the device, i.e. on matrices with a grid
 * hint; 1 = also elsewhere, with the host-built plan; 0 = level-scheduled
 * kernels only; 2 = host-built plan only, for tests).  Matrices created
 * afterwards pick them up. */
BIS_API bis_status bis_set_option(const char *name, int value);
/* The options in effect, for bench / CLI records (no reference counterpart:
 * the reference fixes its configuration at compile time, CMakeLists.txt:19-29):
 * a JSON object of every option that is not at its default, plus "env": the
 * BIS_* environment variables this process found at first use.  Returns the
 * length needed; writes at most cap - 1 characters and a terminator. */
BIS_API int bis_options_describe(char *buf, int cap);
/* number of exported kernel-level symbols, for the load test */
BIS_API int bis_abi_version(void);

/* ---- vectors: replaces `new double[N]` / delete[] in Solver::
 * allocate_structs (solver.hpp:82-110, :130-145) --------------------------- */
BIS_API bis_status bis_vec_alloc(bis_ctx *ctx, int64_t n, double **out);
BIS_API bis_status bis_vec_free(bis_ctx *ctx, double *v);
BIS_API bis_status bis_vec_upload(bis_ctx *ctx, double *dst_dev,
                                  const double *src_host, int64_t n);
BIS_API bis_status bis_vec_download(bis_ctx *ctx, double *dst_host,
                                    const double *src_dev, int64_t n);

/* ---- matrices ------------------------------------------------------------ */
/* MatrixCRS(n_rows, n_cols, nnz) + array fill (sparse_matrix.hpp:76-89) and
 * SMAX register_A (smax_helpers.hpp:10-11): uploads host CRS arrays exactly
 * as given (int32 row_ptr/col, fp64 val, arbitrary column order inside a
 * row) and builds the row-block metadata the SpMV kernel uses.  The structure
 * is checked on the device (row_ptr monotone from 0 to nnz, columns inside
 * [0, n_cols)): BIS_ERR_INVALID instead of a memory fault later. */
BIS_API bis_status bis_mat_create(bis_ctx *ctx, int64_t n_rows, int64_t n_cols,
                                  int64_t nnz, const int32_t *row_ptr,
                                  const int32_t *col, const double *val,
                                  bis_mat **out);
/* Same with 64-bit row pointers (nnz >= 2^31, e.g. HPCG-512: SURVEY.md
 * section 5 defect 6 -- not representable in the reference's MatrixCRS). */
BIS_API bis_status bis_mat_create64(bis_ctx *ctx, int64_t n_rows,
                                    int64_t n_cols, int64_t nnz,
                                    const int64_t *row_ptr, const int32_t *col,
                                    const double *val, bis_mat **out);
BIS_API bis_status bis_mat_destroy(bis_ctx *ctx, bis_mat *A);
BIS_API bis_status bis_mat_info(const bis_mat *A, int64_t *n_rows,
                                int64_t *n_cols, int64_t *nnz);
/* bytes per row pointer on the device: 4, or 8 when nnz >= 2^31 (HPCG-512) or
 * bis_set_option("force_rp64", 1) was in effect when the matrix was made (the
 * tests run the 64-bit instantiations at small sizes that way). */
BIS_API int bis_mat_rp_width(const bis_mat *A);
/* What the SpMV streams per non-zero for this matrix (decided, and built, at
 * the first call of this function or of bis_spmv): col_bytes 4 (CRS columns) or
 * 2 (packed 16-bit column codes); val_bytes 8 (CRS values) or 1 (value
 * dictionary: the matrix has n_dict <= 256 distinct values, compared bit for
 * bit -- every constant-coefficient stencil -- which the kernel keeps in LDS and
 * indexes with a 1-byte code per non-zero; n_dict = 0 without a dictionary);
 * form 0 = the CRS-value kernel, 1 = dictionary kernel, consecutive non-zeros
 * per lane, 2 = dictionary kernel, a lane per row with the codes staged through
 * LDS (rows of at most 40 entries, at most 8 column windows per 256 rows), 3 =
 * the same with the diagonal entries' values in a per-row array beside the
 * dictionary (matrices whose off-diagonal values are few but whose diagonal is
 * not, e.g. the Anderson model: +8 bytes per row), 4 / 5 = forms 2 / 3 with the
 * block's x entries copied into an LDS window by coalesced loads and the codes
 * stored per 64-row slice in lane order (sliced ELL, 12 bytes per 4 non-zeros
 * and lane, short rows padded with an arithmetically neutral entry; option
 * "spmv_sellwin" 0 switches it off; its denser formats report col_bytes 2 and
 * val_bytes 0 (one 16-bit code per non-zero), col_bytes 1 and val_bytes 0 (one
 * byte: the index of the non-zero's (column - row, value) pair) or col_bytes 0
 * (a 32-bit mask of pairs per ROW)), 6 = the window + sliced-ELL form with the
 * 8-byte values streamed (col_bytes 2: the window slot, also where the slots are
 * implied; matrices without a dictionary; option "spmv_win8" 0 switches it off),
 * 7 = the CRS-value kernel in K passes over column slabs (n_dict = K), 8 = form 6
 * with 4-byte values (col_bytes 2, val_bytes 4, "win4 rows=R"): only for a matrix
 * that bis_mat_round_f32 flagged, on whose values the float stream is lossless;
 * option "spmv_win4" 0 switches it off (the matrix then gets form 6).  Form 0
 * also covers the wave-per-row kernel of very long rows (col_bytes 4) and the
 * opt-in x-window kernel (col_bytes 2).  The report names what bis_spmv launches
 * and builds nothing else.
 * All are lossless re-encodings of the CRS arrays, which stay authoritative:
 * same products, same summation order, bit-identical y.  Option
 * "spmv_valdict" 0 switches the dictionary off, 1 allows form 1 only. */
BIS_API bis_status bis_mat_spmv_stream_info(bis_ctx *ctx, const bis_mat *A,
                                            int *col_bytes, int *val_bytes,
                                            int *n_dict, int *form);
/* Bytes one y = A x launch moves at least with the stream format the matrix
 * currently has (bis_mat_spmv_stream_info): the format's own arrays once -- for
 * forms 4 / 5 including the padding of the sliced-ELL stream --, x once
 * (8 n_cols) and y once (8 n_rows).  The denominator-free part of a roofline
 * figure for the kernel that actually runs; the CRS figure of the reference's
 * loop (kernels.hpp:22-42) is 12 nnz + 20 n_rows. */
BIS_API bis_status bis_mat_spmv_streamed_bytes(bis_ctx *ctx, const bis_mat *A,
                                               int64_t *bytes);
/* Structured-grid hint: the rows are the unknowns of an nx x ny x nz grid, x
 * fastest, dof unknowns per node (row = ((z*ny + y)*nx + x)*dof + d) -- e.g.
 * an HPCG-n.mtx read from a file.  The generators set it themselves, and
 * bis_mat_create recognises one-unknown-per-node stencils of 4096 rows or more
 * from the column offsets of a few rows (option "grid_autodetect" 0: off); strict
 * triangles and ILU(0) factors inherit it.  Only the tiled triangular sweep
 * uses it (tiles that extend in all grid directions); a hint that does not
 * describe the matrix costs speed, never correctness (the tile order is
 * verified against the dependencies, else the natural order is used). */
BIS_API bis_status bis_mat_set_grid_hint(bis_mat *A, int64_t nx, int64_t ny,
                                         int64_t nz, int dof);
/* the hint a matrix carries: hint[0..3] = nx, ny, nz, dof; all 0 without one */
BIS_API bis_status bis_mat_grid_hint(const bis_mat *A, int64_t hint[4]);
/* rebuild a matrix' row-block metadata after bis_set_option (tuning) */
BIS_API bis_status bis_mat_retune(bis_ctx *ctx, bis_mat *A);
/* Placement tuning (setup, optional): WHERE in HBM the streamed arrays of a matrix
 * land moves the SpMV time of the same data by up to 20 % (HPCG-256: 0.82 ... 0.98 ms
 * between allocations of one process).  Re-allocates the
 * streamed arrays (values and column stream) up to max_trials times, times the SpMV
 * on each copy and keeps the fastest; the rejected copies are held until the end so
 * that every trial sees different memory.  Transient memory: up to max_trials copies.
 * Not for row views; call it before views of A are made (bis_dist_create) and
 * before the first triangular solve on A (its plan caches views): refused
 * with BIS_ERR_INVALID afterwards.
 * first_ms / best_ms (optional): SpMV time before and after. */
/* The window + sliced-ELL stream of a matrix (the SpMV's form for matrices without a value
 * dictionary: 8-byte values + 2-byte window slots) is placement-tuned when it is built (streams
 * of 1 GiB or more; option "spmv_win8_tune" = trials, 0 off): what the search did -- re-allocations
 * tried, the kernel's time on the first allocation and on the one kept (ms; zeros when the matrix
 * has no such stream or no tuning ran).  For bench / CLI records. */
BIS_API void bis_mat_win8_tuning(const bis_mat *A, int *trials, double *first_ms, double *kept_ms);
/* The layout of that stream (zeros without one): its chunks (4 entries of 64 rows), the chunks that keep their
 * 2-byte window slots (all of them unless *implied), slices (64 rows), blocks; *implied = 1 where the slots of the
 * other chunks are implied by their rows (option "spmv_win8_implicit"): 2048 bytes per chunk instead of 2560.
 * Where the matrix runs form 8 (4-byte values) this, bis_mat_win8_tuning and bis_mat_win8_debug_stream speak of that
 * stream: the same chunks at 1536 bytes, 1024 with implied slots. */
BIS_API void bis_mat_win8_layout(const bis_mat *A, int64_t *chunks, int64_t *explicit_chunks, int64_t *slices, int *blocks, int *implied);
/* Column slabs (the SpMV's form for a matrix WITHOUT locality: rows along which the slab index never falls --
 * ascending columns, the usual case --, a column stream that does not
 * pack, an x that does not fit an XCD's L2 -- config 5's unstructured input as generated): K CRS copies of
 * column ranges whose x slices fit the L2, multiplied in K passes that continue each row's left-to-right sum
 * (kernels.hpp:25-39: the same sum, bit for bit).  Built at the first SpMV; kept where a trial -- three timed
 * launches each way -- measures the passes at least 15 % faster than the one pass (option "spmv_colslab": 0
 * never, k >= 2: k slabs without a trial).  *slabs: K, 0 when the matrix has none; the trial's times (ms,
 * zeros when none ran).  For bench / CLI records. */
BIS_API void bis_mat_colslab_info(const bis_mat *A, int *slabs, double *one_pass_ms, double *slab_passes_ms);
/* debugging / tuning aid (tools/win8_offsets.py): address and size of that stream; set != NULL: the
 * kernel reads the stream from `set` from now on (memory of the caller, into which it has copied the
 * stream), set == NULL: back to the library's own buffer. */
BIS_API bis_status bis_mat_win8_debug_stream(bis_mat *A, void **ptr, size_t *bytes, void *set);
BIS_API bis_status bis_mat_tune_placement(bis_ctx *ctx, bis_mat *A, int max_trials,
                                          double *first_ms, double *best_ms);
/* device addresses of the CRS arrays (tuning / zero-copy interop).  A caller that
 * writes VALUES through them must call bis_mat_retune afterwards: the library
 * caches re-encodings of the values (dictionary code streams, the tiled sweeps'
 * entry streams) that bis_mat_retune and bis_mat_scale_sym drop. */
BIS_API bis_status bis_mat_debug_ptrs(const bis_mat *A, void **row_ptr,
                                      void **col, void **val);
/* copy the device CRS back (tests: bit-exact CRS checks); any pointer may be
 * NULL.  row_ptr is returned as int64. */
BIS_API bis_status bis_mat_download(bis_ctx *ctx, const bis_mat *A,
                                    int64_t *row_ptr, int32_t *col,
                                    double *val);

/* Synthetic inputs generated directly in HBM (stands in
 * for MatrixCOO::scamac_generate, sparse_matrix.hpp:577-721, and for reading
 * HPCG-n.mtx).  Rows [row0,row1) of the global matrix with GLOBAL column
 * indices; n_cols = global row count.
 *   HPCG: 27-point, a_ii=26, a_ij=-1, open boundaries, ascending columns.
 *   Anderson: 7-point periodic L^3, off-diagonals -t, diagonal
 *   W*(u(seed,row)-1/2)+shift, ascending columns. */
BIS_API bis_status bis_mat_gen_hpcg(bis_ctx *ctx, int64_t nx, int64_t ny,
                                    int64_t nz, int64_t row0, int64_t row1,
                                    bis_mat **out);
BIS_API bis_status bis_mat_gen_anderson(bis_ctx *ctx, int64_t L, double t,
                                        double W, double shift, uint64_t seed,
                                        int64_t row0, int64_t row1,
                                        bis_mat **out);

/* FEM-like unstructured input (stands in for reading
 * SuiteSparse Flan_1565.mtx in config 5): nx*ny*nz nodes with 3 unknowns each,
 * 3x3-block couplings to the 27-point neighbours that survive a symmetric coin
 * flip (keep_percent), symmetric negative off-diagonals, strictly dominant
 * diagonal (SPD); ~3*(1+26*keep/100) non-zeros per interior row. */
BIS_API bis_status bis_mat_gen_fem(bis_ctx *ctx, int64_t nx, int64_t ny,
                                   int64_t nz, int keep_percent, uint64_t seed,
                                   int64_t row0, int64_t row1, bis_mat **out);

/* Unstructured input (BASELINE config 5 "SuiteSparse unstructured", read in the
 * reference through sparse_matrix.hpp:225-357; the .mtx is not fetchable): the
 * FEM-like matrix above under a seeded random symmetric permutation of its rows,
 * B = P A P^T, columns ascending inside a row, NO grid hint -- the triangular
 * sweeps and ILU(0) of this matrix take the general (level-scheduled / chunked)
 * kernels like any matrix read from a file.  perm[new] = old: stable ascending
 * order of hash(seed ^ K3, old); written to perm_dev_out (n int32) if non-NULL. */
BIS_API bis_status bis_mat_gen_unstr(bis_ctx *ctx, int64_t nx, int64_t ny,
                                     int64_t nz, int keep_percent, uint64_t seed,
                                     int32_t *perm_dev_out, bis_mat **out);

/* Setup steps kept on the device:
 * split_LU (utilities/LU_factors.hpp:122-309): strict lower / strict upper
 * parts of A, row order preserved; and the diagonal extraction of
 * peel_diag_crs (:827-869): D and 1/D.  Fails with BIS_ERR_ZERO_DIAG /
 * BIS_ERR_NO_DIAG like the reference's SanityChecker. */
BIS_API bis_status bis_mat_split_strict(bis_ctx *ctx, const bis_mat *A,
                                        bis_mat **L_strict, bis_mat **U_strict,
                                        double *D, double *D_inv);

/* -scale on the device: extract_scale
 * (utilities/LU_factors.hpp:880-898), s_r = 1/sqrt(|a_rr|) written to scale[r]
 * (rows without a diagonal entry keep the caller's value), then scale_mat
 * (preprocessing.hpp:15-24), a_rc *= (s_r * s_c), in place.  BIS_ERR_ZERO_DIAG
 * with the reference's message if |a_rr| < 1e-16.  The values only change, so
 * the packed column stream and the row-block tables stay valid. */
BIS_API bis_status bis_mat_scale_sym(bis_ctx *ctx, bis_mat *A, double *scale);

/* Single-precision preconditioner storage (not in the reference).  Rounds every
 * value of A to binary32 IN PLACE in the fp64 CRS array: v becomes
 * (double)(float)v -- IEEE round to nearest even, subnormals kept, -0.0 kept,
 * NaN / Inf unchanged.  *max_rel_change (may be NULL): max |v32 - v| / |v| over
 * the finite v != 0, reduced in a fixed order (the same bits on every run).
 * A value that is finite in fp64 but not in fp32 makes the call fail with
 * BIS_ERR_UNSUPPORTED and leaves the matrix untouched (a census pass runs before
 * the rounding pass).  BIS_ERR_INVALID for a null matrix or a row-range view;
 * nnz == 0 is BIS_OK.  Blocking; idempotent (a second call changes no bit and
 * reports 0).
 * This is the one lossy step, explicit and once only.  Everything derived from
 * the values is dropped as by bis_mat_scale_sym, and the matrix is flagged
 * fp32-exact: its SpMV may then stream 4-byte values (form 8 of
 * bis_mat_spmv_stream_info), a lossless re-encoding on such values -- y is
 * bit-identical to every other form on the rounded matrix.  bis_mat_scale_sym
 * and bis_mat_retune clear the flag; row views inherit it; nothing else does
 * (permutations, splits, factorisations give unflagged matrices: round again).
 * No matrix is ever examined or rounded without this call.
 * The fp64 CRS arrays stay, holding the rounded values, so sweeps, bis_spmm,
 * downloads, ILU(0) and the row-block kernels work unchanged on the rounded
 * matrix: the feature saves memory TRAFFIC of the SpMV, not memory.
 * Meant for preconditioner factors (G, Gt of bis_mat_fsai; the strict triangles
 * of bis_mat_ilu0 for BIS_PC_ILU0_ITER); the Krylov method stays in fp64. */
BIS_API bis_status bis_mat_round_f32(bis_ctx *ctx, bis_mat *A, double *max_rel_change);

/* Multi-colour symmetric reordering on the device (the
 * role of SMAX's permute_mat, utilities/smax_helpers.hpp:44-80): greedy
 * first-fit colouring in natural row order, rows grouped by colour (stable),
 * B = P A P^T with perm[new] = old written to perm_dev (device, n int32; e.g.
 * storage from bis_vec_alloc).  The strict triangles of B have one dependency
 * level per colour.  BIS_ERR_UNSUPPORTED if more than 64 colours are needed.
 * bis_vec_gather: out[i] = in[perm[i]] (permute b, x_0; out != in). */
BIS_API bis_status bis_mat_multicolour(bis_ctx *ctx, const bis_mat *A,
                                       bis_mat **B, int32_t *perm_dev,
                                       int *n_colours);
BIS_API bis_status bis_vec_gather(bis_ctx *ctx, double *out, const double *in,
                                  const int32_t *perm_dev, int64_t n);
/* Breadth-first (rcm = 0) or reverse Cuthill-McKee (rcm = 1) ordering on the
 * device (SMAX PERM_MODE BFS / RCM roles, CMakeLists.txt:128-133): perm[new] =
 * old written to perm_dev (n int32).  Level-synchronous, and entry for entry
 * the permutation of the sequential queue algorithm (components from the
 * lowest-numbered / lowest-degree unseen vertex, neighbours in ascending index
 * / ascending (degree, index) order).  Structurally symmetric patterns with
 * at most 64 connected components; otherwise BIS_ERR_UNSUPPORTED (the host
 * layer then runs the sequential version).
 * bis_mat_permute: B = P A P^T for any permutation (entries keep their order
 * inside a row, columns renumbered); BIS_ERR_INVALID if perm is not one. */
BIS_API bis_status bis_mat_bfs_order(bis_ctx *ctx, const bis_mat *A, int rcm,
                                     int32_t *perm_dev);
BIS_API bis_status bis_mat_permute(bis_ctx *ctx, const bis_mat *A,
                                   const int32_t *perm_dev, bis_mat **B);
/* out[perm[i]] = in[i]: the inverse permutation without forming it -- returns
 * x* of a permuted solve in the caller's original row order (the reference's
 * SMAX path leaves x* permuted, smax_helpers.hpp:44-80).  out != in. */
BIS_API bis_status bis_vec_scatter(bis_ctx *ctx, double *out, const double *in,
                                   const int32_t *perm_dev, int64_t n);

/* ILU(0) on the device: the arithmetic of the
 * reference's serial factor_ILU0_old (utilities/LU_factors.hpp:320-539),
 * scheduled by the dependency levels of A's strict lower triangle (its
 * level-parallel factor_ILU0_new, :541-768, needs SMAX).  Outputs the strict
 * factors with ascending columns, L_D = 1 and U_D = diag(U); the reference's
 * pivot guard uses ILU0_PIVOT_TOLERANCE / ILU0_PIVOT_REPLACEMENT. */
BIS_API bis_status bis_mat_ilu0(bis_ctx *ctx, const bis_mat *A, double pivot_tol,
                                double pivot_repl, bis_mat **L_strict,
                                bis_mat **U_strict, double *L_D, double *U_D);
/* bis_mat_ilu0_kernel names the elimination kernel that factorised the L_strict
 * returned by bis_mat_ilu0: "ilu0_persistent_kernel", "ilu0_level_wave_kernel"
 * or "ilu0_level_kernel" (static string; "" for any other matrix). */
BIS_API const char *bis_mat_ilu0_kernel(const bis_mat *L_strict);

/* ILU(k) with level-of-fill (bis_iluk.hip); no reference counterpart.  A must be square with a stored diagonal entry in
 * every row and no column repeated inside a row; 0 <= level <= 16.
 * Levels: lev(i,j) = 0 where A stores (i,j), otherwise the minimum over p < min(i,j) of lev(i,p) + lev(p,j) + 1 (infinite
 * without such a p).  Equivalently (Hysom & Pothen) lev(i,j) + 1 is the number of edges of the shortest path i -> j in the
 * graph of A all of whose interior vertices are < min(i,j); the device finds it by one breadth-first search per row, on A
 * for the upper and on A^T for the lower triangle (on A alone where the pattern is structurally symmetric).
 * Symbolic: P holds exactly the positions with lev(i,j) <= level, columns ascending, A's value where A stores the
 * position and +0.0 elsewhere; *n_fill (may be NULL) = nnz(P) - nnz(A).  P has 64-bit row pointers when A has them or its
 * entry count needs them, and no grid hint for level >= 1 (a filled stencil is no stencil).  For level 0, P is A with
 * sorted rows.
 * Numeric: row-wise IKJ elimination on the pattern of P, pivots k < i of row i in ascending order; for each,
 * skip if |u_kk| < 1e-16, else l_ik = w_ik / u_kk and w_ij = fma(-l_ik, u_kj, w_ij) for EVERY j > k that rows i and k of
 * P share -- bis_mat_ilu0's arithmetic and kernels without its rule that a position whose current value is 0.0 is left
 * alone; then |u_ii| < pivot_tol becomes sign(u_ii) * pivot_repl.  Outputs as bis_mat_ilu0: the strict factors with
 * ascending columns, L_D = 1, U_D = diag(U); BIS_PC_ILU0 and BIS_PC_ILU0_ITER take them unchanged.  Without a grid hint
 * the factors run the level-scheduled and chained sweeps.
 * bis_mat_iluk with level == 0 IS bis_mat_ilu0 (same checks, bits, grid hint and kernel, the non-zero rule included);
 * *n_fill = 0.
 * BIS_ERR_INVALID: null arguments, A not square, a row-range view, level outside 0..16; BIS_ERR_NO_DIAG: a row without a
 * stored diagonal entry; BIS_ERR_UNSUPPORTED: a column repeated inside a row, or a row whose search visits more than
 * max_visit vertices (bis_iluk_limits; the message names the row -- nothing is truncated).  *P, *L_strict, *U_strict and
 * *n_fill are written on success only.  n = 0: BIS_OK.  Blocking.  No floating-point value is accumulated with atomics
 * and the pattern does not depend on the order in which the search claims vertices: two calls give the same bits.
 * bis_mat_iluk_kernel: the symbolic instance that made P or L_strict, "iluk_search_kernel RP=32 two searches" or
 * "... one search, transposed" (static string; "" for the factors of level 0 and for any other matrix); bis_mat_ilu0_kernel names the
 * numeric kernel as for ILU(0).  bis_iluk_limits: max_level = 16, max_visit = 4096 (either may be NULL). */
BIS_API bis_status bis_mat_iluk_symbolic(bis_ctx *ctx, const bis_mat *A, int level, bis_mat **P, int64_t *n_fill);
BIS_API bis_status bis_mat_iluk(bis_ctx *ctx, const bis_mat *A, int level, double pivot_tol, double pivot_repl,
                                bis_mat **L_strict, bis_mat **U_strict, double *L_D, double *U_D, int64_t *n_fill);
BIS_API const char *bis_mat_iluk_kernel(const bis_mat *L_strict);
BIS_API bis_status bis_iluk_limits(int *max_level, int *max_visit);

/* Factorized sparse approximate inverse (FSAI, Kolotilina-Yeremin) on the pattern of tril(A); no reference counterpart.
 * Only the entries of A with column <= row are read; the result is the FSAI of the symmetric matrix they define.  For row
 * i let J be the columns <= i of row i in ascending order (the last one is i, |J| = m <= 64) and S = A[J,J], S[p,q]
 * (q <= p) taken from row J[p], column J[q], an absent entry counting as 0.  With S = C C^T (Cholesky, fp64) row i of G on
 * the columns J is g = C^-T e_m (one back substitution on the last unit vector; g = y / sqrt(y_m) for S y = e_m), so that
 * diag(G A G^T) = 1 and M^-1 = G^T G is symmetric positive definite.  A row one of whose pivots is <= 0 or not finite
 * becomes e_i / sqrt(|a_ii|) (on the same pattern, the other entries 0) and counts in *n_fallback_rows (may be NULL).
 * G is lower triangular with its diagonal and Gt = G^T upper triangular; both are ordinary matrices with ascending
 * columns and A's row-pointer width, without a grid hint: bis_spmv / bis_spmm apply them, BIS_PC_FSAI takes G as L_strict
 * and Gt as U_strict.  The rows are independent (one wave each, fsai_rows_kernel) and nothing is accumulated with
 * floating-point atomics: two calls give the same bits, whatever the order of the entries inside A's rows.
 * BIS_ERR_INVALID: null arguments, A not square or a row-range view; BIS_ERR_ZERO_DIAG: a row without a diagonal entry
 * or with a_ii = 0; BIS_ERR_UNSUPPORTED: more than 64 entries left of and on the diagonal of a row, a column repeated
 * inside a row, a pattern that is not structurally symmetric.  *G and *Gt are written on success only.  n = 0: BIS_OK.
 * Blocking.  bis_mat_fsai_kernel: the instance that computed G, "fsai_rows_kernel M=32 RP=32" (M = 16, 32 or 64 by the
 * longest lower row; static string, "" for any other matrix). */
BIS_API bis_status bis_mat_fsai(bis_ctx *ctx, const bis_mat *A, bis_mat **G, bis_mat **Gt, int64_t *n_fallback_rows);
BIS_API const char *bis_mat_fsai_kernel(const bis_mat *G);

/* ---- sparse matrix-matrix product and transpose (bis_spgemm.hip); no reference counterpart --------------------------------
 * bis_spgemm: C = A B for A (n x m) and B (m x p), either may be rectangular; nothing is assumed about the order of the
 * columns inside the rows of A or B, or about repeats.
 * Enumeration: for row i the products are taken in this order: position s in row i of A (CRS order, j = col[s]), then
 * position t in row j of B (k = col[t]).
 * Pattern: entry (i, k) of C exists iff at least one product lands on it -- also where the values cancel to 0.
 * Value: the sum of a_ij b_jk in enumeration order, the first product starting the sum, every product and every addition
 * rounded separately in fp64 (no fused multiply-add).
 * Rows: columns ascend inside a row, without repeats.  Row pointers: 64-bit when nnz(C) needs them or option force_rp64
 * is set.  C carries no grid hint and no fp32 flag.
 * Two paths give these bits.  With u_i = sum over the entries (i, j) of A of nnz(B_j): a row with u_i <= spgemm_row_cap
 * (option; default and at most 4096) takes the row path -- a workgroup per row of C (one wave up to 256 products, four
 * waves beyond) sorts the candidate columns in LDS and gives every output entry to a lane that walks A's row in order and
 * bisects the rows of B; it needs strictly ascending rows of B, so any other B sends every row to the fallback.  Every
 * other row (and every row with spgemm_row_cap = 0) takes the fallback: whole rows in batches of at most spgemm_batch
 * products (option; default 2^26; a longer row is a batch of its own), expanded, sorted by a stable 64-bit radix sort and
 * summed run by run.  Its temporary memory grows with the batch, not with the total number of products.  Nothing is
 * truncated or refused for its length.
 * Blocking.  No floating-point atomics, no inter-workgroup waits: two calls give the same bits.
 * BIS_ERR_INVALID: null arguments, n_cols(A) != n_rows(B), a row-range view.  n = 0 or no product at all: BIS_OK, a C
 * without entries.  *C is written on success only.
 * bis_spgemm_kernel: the path(s) that made C: "spgemm_row_kernel", "spgemm_sort_fallback" or
 * "spgemm_row_kernel + spgemm_sort_fallback" (static string; "" for a C without entries and for any other matrix).
 * bis_spgemm_limits (any pointer may be NULL): wave_cap = 256, row_cap = 4096 (the default of spgemm_row_cap),
 * row_cap_max = 4096 (larger settings count as this), batch = 2^26 (the default of spgemm_batch).
 *
 * bis_mat_transpose: At = A^T with the values of A bit for bit.  Row c of At lists the entries of column c of A in
 * ascending row order; repeats of a column inside one row of A stay adjacent, in that row's order.  Row pointers by the
 * library's rule, no grid hint.  A stable sort places the entries: the result does not depend on the schedule.
 * BIS_ERR_INVALID: null arguments, a row-range view.  *At is written on success only.  Blocking. */
BIS_API bis_status bis_spgemm(bis_ctx *ctx, const bis_mat *A, const bis_mat *B, bis_mat **C);
BIS_API bis_status bis_mat_transpose(bis_ctx *ctx, const bis_mat *A, bis_mat **At);
BIS_API const char *bis_spgemm_kernel(const bis_mat *C);
BIS_API bis_status bis_spgemm_limits(int *wave_cap, int *row_cap, int *row_cap_max, int64_t *batch);

/* ---- aggregation multigrid (bis_mg.hip); no reference counterpart ------------------------------------------------------
 * Unsmoothed aggregation, one V(nu,nu) cycle with Jacobi-type smoothing as the preconditioner (or a W- or K-cycle of the same
 * hierarchy: bis_mg_set_cycle): SpMVs and streaming passes only, no dependency between rows, any row order.
 *
 * Parameters (NULL = the defaults): max_levels 10 (1..16); coarse_limit 256 (>= 1): a level of at most this many rows is
 * not coarsened; coarsening 0 = grid aggregates where the level has a grid hint whose product is its size, MIS aggregates
 * otherwise, 1 = grid only (BIS_ERR_INVALID where a level has no such hint), 2 = MIS only; nu 1 (>= 1): sweeps before and
 * after the coarse correction; coarse_sweeps 4 (>= 1): sweeps on the coarsest level; omega 0: l1-Jacobi,
 * w_i = 1 / sum_j |a_ij| with the sum taken left to right in CRS order from 0, omega > 0: damped Jacobi,
 * w_i = omega / a_ii (the first entry of row i on the diagonal); coarse_scale 1.0: factor on the coarse correction.
 *
 * Levels.  Level 0 is A itself: not copied, the caller keeps it alive and unchanged while the hierarchy lives.  Level l
 * (n_l rows) is the coarsest if n_l <= coarse_limit, or if it is level max_levels - 1, or if its aggregates number more
 * than 0.8 n_l (5 n_{l+1} > 4 n_l: the step is dropped, level l + 1 is not built).  kind[l]: 1 grid, 2 MIS, 0 coarsest.
 *
 * Grid aggregates of a level with hint (nx, ny, nz, dof), row = ((z ny + y) nx + x) dof + d:
 * agg = (((z/2) cy + y/2) cx + x/2) dof + d, cx = (nx+1)/2, cy, cz alike; the coarse matrix gets the hint (cx, cy, cz, dof).
 *
 * MIS aggregates (any structurally symmetric pattern without repeated entries; otherwise BIS_ERR_UNSUPPORTED, as
 * bis_mat_bfs_order).  The roots are the greedy maximal independent set of the off-diagonal pattern taken in descending
 * order of the key (hash32(i), i), hash32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * on 32-bit unsigned x.  Found in rounds (an undecided row whose key is the largest among its undecided neighbours becomes
 * a root, its undecided neighbours members), which gives that set whatever the schedule; the host reads one counter per
 * round.  A row without off-diagonal entries is a root.  A member joins the root among its neighbours with the largest
 * |a_ij|, the lowest column among equals.  Aggregates are numbered by ascending root row.
 *
 * Galerkin operator for the piecewise-constant prolongation: entry (I, J) of level l + 1 is the sum of the fine entries
 * (r, c, v) with agg[r] = I, agg[c] = J, taken in fine CRS order (ascending r, then the order inside row r), the first value
 * starting the sum and every further one added to it in fp64.  Only pairs (I, J) with a fine entry exist; columns ascend
 * inside a row; the row-pointer width follows the library's rule (option force_rp64 honoured).  The two mirror entries of a
 * symmetric A are summed in different orders: the coarse matrices are symmetric to rounding only.
 *
 * BIS_ERR_INVALID: null arguments, A not square, a row-range view, bad parameters; BIS_ERR_ZERO_DIAG: a row of some level
 * without a diagonal entry or with a zero there; n = 0: BIS_OK (one level without rows).  *out is written on success only.
 * Blocking; everything runs on the device without floating-point atomics: two calls give the same bits.  Setup also
 * resolves every level's SpMV form and allocates the cycle's scratch: bis_mg_apply allocates nothing and never blocks. */
typedef struct bis_mg bis_mg;
typedef struct {
    int max_levels;
    int64_t coarse_limit;
    int coarsening;
    int nu;
    int coarse_sweeps;
    double omega;
    double coarse_scale;
} bis_mg_params;
BIS_API bis_status bis_mg_create(bis_ctx *ctx, const bis_mat *A, const bis_mg_params *params, bis_mg **out);
BIS_API bis_status bis_mg_destroy(bis_ctx *ctx, bis_mg *mg);
/* out = M^-1 in: one cycle (the V-cycle below unless bis_mg_set_cycle chose another), stream-ordered; out may alias in (the
 * right-hand side is then copied first).  On level l with
 * right-hand side b, every product, subtraction and addition rounded separately (no fused multiply-add), y = A x by bis_spmv:
 *   x = w o b;  then nu - 1 sweeps  y = A x, x_i = x_i + w_i (b_i - y_i);
 *   y = A x;  r_c[I] = sum over the rows i of aggregate I in ascending order of (b_i - y_i), the first difference starting the
 *   sum;  e_c = the cycle of level l + 1 on r_c;  x_i = x_i + coarse_scale e_c[agg[i]];  then nu sweeps as above.
 * The coarsest level: x = w o b, then coarse_sweeps - 1 sweeps. */
BIS_API bis_status bis_mg_apply(bis_ctx *ctx, const bis_mg *mg, double *out, const double *in);
/* The cycle of an existing hierarchy (a fresh one is V).  With L levels there are L - 1 transitions, transition t from level t
 * to level N = t + 1.  Transition t uses `cycle` iff t < L - 2 (the one onto the coarsest level is always the plain one) and
 * (cycle_levels == 0 or t < cycle_levels); every other transition is the V step.  At most two levels: V's bits under any
 * setting.  The hierarchy, the operators and the smoother stay; only "e_c = the cycle of level N on r_c" above is replaced,
 * every product, quotient, difference and sum below rounded separately, A_N x by bis_spmv:
 *   W:  e_1 = cycle(N, r_c);  y = A_N e_1;  r_2 = r_c - y;  e_2 = cycle(N, r_2);  e_c = e_1 + e_2.  Linear and fixed, like V.
 *   K (Notay's K-cycle: two steps of a Krylov method preconditioned by the cycle of level N; BIS_MG_CYCLE_K takes conjugate
 *   directions, for SPD A under CG; BIS_MG_CYCLE_K_GCR minimises the residual, for any A):
 *     c = cycle(N, r_c);  v = A_N c;  t = c (K) or v (K_GCR);  rho1 = (t, v), alpha1 = (t, r_c);
 *     rho1 zero or not finite: e_c = 0, exactly, whatever the rest computes;  s1 = alpha1 / rho1;  r~ = r_c - s1 v;
 *     d = cycle(N, r~);  w = A_N d;  t2 = d (K) or w (K_GCR);  gamma = (t2, v), beta = (t2, w), alpha2 = (t2, r~);
 *     rho2 = beta - (gamma gamma) / rho1;  not rho2 > 0 (NaN included): c1 = s1, c2 = 0;  otherwise c2 = alpha2 / rho2,
 *     c1 = s1 - (gamma c2) / rho1;  e_c,i = (c1 c_i) + (c2 d_i).
 *   The dot products are sums of fused multiply-adds in a fixed order that depends on the length only (per-workgroup partial
 *   sums, summed in index order by the workgroup that arrives last); the coefficients stay in device scalars that every
 *   transition owns.  There is no early exit: the launch sequence is fixed, nothing is read back, two applies give the same
 *   bits.  A K-cycle is not a fixed linear operator: a method that assumes one (left-preconditioned GMRES) is not for it;
 *   flexible GMRES (bis_fgmres_*) is.
 * bis_mg_set_cycle blocks and allocates the extra scratch (two vectors on the coarse level of a W transition, three of a K
 * transition), so bis_mg_apply still allocates nothing and never blocks; setting V again restores V's bits.
 * BIS_ERR_INVALID: null arguments, cycle outside 0..3, cycle_levels < 0 (nothing changes).  bis_mg_cycle reports what is
 * set; either pointer may be NULL. */
enum { BIS_MG_CYCLE_V = 0, BIS_MG_CYCLE_W = 1, BIS_MG_CYCLE_K = 2, BIS_MG_CYCLE_K_GCR = 3 };
BIS_API bis_status bis_mg_set_cycle(bis_ctx *ctx, bis_mg *mg, int cycle, int cycle_levels);
BIS_API bis_status bis_mg_cycle(const bis_mg *mg, int *cycle, int *cycle_levels);
/* The hierarchy as the preconditioner of type BIS_PC_MG: an n x n matrix without entries that mg owns (bis_mat_destroy on it
 * does nothing) and that leads back to mg; every entry point but the preconditioner dispatch sees the zero matrix. */
BIS_API const bis_mat *bis_mg_operand(const bis_mg *mg);
/* *levels, and per level (arrays of 16) rows, non-zeros and the aggregate kind; any pointer may be NULL. */
BIS_API bis_status bis_mg_info(const bis_mg *mg, int *levels, int64_t *rows, int64_t *nnz, int *kind);
/* Level l's matrix (level 0: A), owned by mg: for bis_mat_download, bis_mat_grid_hint, bis_mat_spmv_stream_info.  NULL
 * outside the hierarchy. */
BIS_API const bis_mat *bis_mg_level_matrix(const bis_mg *mg, int level);
/* agg[0, n_l) of a level that is not the coarsest, and w[0, n_l) of any level, to host arrays.  Blocking. */
BIS_API bis_status bis_mg_level_aggregates(bis_ctx *ctx, const bis_mg *mg, int level, int32_t *host);
BIS_API bis_status bis_mg_level_weights(bis_ctx *ctx, const bis_mg *mg, int level, double *host);
/* Smoothed aggregation: bis_mg_create with one Jacobi-smoothed prolongator per transition.  prolong_omega 0 means 4/3;
 * otherwise it must lie in (0, 2) (else BIS_ERR_INVALID).  Everything bis_mg_create documents holds -- level rule, 0.8 rule,
 * grid / MIS aggregates, weights, error table, the hint (cx, cy, cz, dof) on grid levels, blocking, reproducible bits --
 * except the transfer operators and the Galerkin product of every transition, built from the level matrix A (n rows), its
 * aggregates agg and n_c:
 *   rho = max_i (s_i / |a_ii|), s_i = sum_j |a_ij| summed left to right from 0 (the sum of the l1 weights), a_ii the first
 *   diagonal entry of row i, the quotient rounded: Gershgorin's bound on the spectral radius of D^-1 A.
 *   omega_l = prolong_omega / rho (one division).
 *   T: n x n_c with t_{i,agg[i]} = 1.  Q = A T by bis_spgemm's rule (the products a_ij 1 are exact).
 *   P has Q's pattern, structural zeros kept: c_i = omega_l / a_ii, p_iJ = t_iJ - c_i q_iJ (the product rounded, then the
 *   difference; t_iJ = 0 off the aggregate).  R = bis_mat_transpose(P).
 *   A_c = bis_spgemm(R, bis_spgemm(A, P)), in that association.
 * Entries that cancel stay in the pattern, so A_c is structurally symmetric whenever A is: MIS aggregates of the next
 * level can be taken.
 * The cycle is bis_mg_apply's with the two transfers replaced, every product and addition rounded separately:
 *   r_c[I] = sum over row I of R of R_{I,t} (b - y)_{col t}: lane q of a wave of 64 sums the products at the positions
 *   q, q + 64, ... of the row in that order from 0, and the 64 sums are added pairwise, lane q with lane q + 32, then
 *   + 16, ..., + 1;
 *   x_i = x_i + coarse_scale (sum over row i of P of P_{i,t} e_c[col t]), the row taken left to right, the first product
 *   starting the sum.
 * bis_mg_set_cycle and everything that takes BIS_PC_MG work on such a hierarchy unchanged.
 * bis_mg_level_prolongator / _restrictor: P and R of the transition from `level`, owned by the hierarchy; NULL on the
 * coarsest level, outside the hierarchy and on a hierarchy made by bis_mg_create.  bis_mg_level_prolong_omega: omega_l of
 * such a transition (BIS_ERR_INVALID where the prolongator is NULL).  bis_mg_info's nnz counts the level operators only. */
BIS_API bis_status bis_mg_create_smoothed(bis_ctx *ctx, const bis_mat *A, const bis_mg_params *params, double prolong_omega, bis_mg **out);
BIS_API const bis_mat *bis_mg_level_prolongator(const bis_mg *mg, int level);
BIS_API const bis_mat *bis_mg_level_restrictor(const bis_mg *mg, int level);
BIS_API bis_status bis_mg_level_prolong_omega(const bis_mg *mg, int level, double *omega_l);
/* The smoother of an existing hierarchy (a fresh one relaxes with its weights w: BIS_MG_SMOOTH_JACOBI, the sweeps above).
 * BIS_MG_SMOOTH_CHEBYSHEV replaces every "sweep" above -- in nu, nu - 1, coarse_sweeps - 1 and the first one from x = 0 -- by
 * one Chebyshev polynomial of degree `degree` in W A, W = diag(w), built for the interval [lambda_max / ratio, lambda_max]
 * of every level: as many SpMVs and streaming passes as `degree` Jacobi sweeps, no dependency between rows, and the V- and
 * W-cycle stay fixed, symmetric positive definite operators.  max_levels = 1 makes the cycle a polynomial preconditioner.
 *
 * Spectrum of level l (operator A, weights w, n rows):
 *   bound = max_i w_i s_i, s_i = sum_j |a_ij| summed left to right in CRS order from 0 (the sum w_i was made from where
 *   omega = 0), the product rounded.  Gershgorin's bound on the spectrum of W A; per-workgroup maxima, then one pass: exact
 *   whatever the order.  A bound that is not positive and finite: BIS_ERR_INVALID.
 *   estimate = 0 for est_steps = 0; otherwise lambda_{est_steps} of the power iteration on W A in the W^-1 inner product, run
 *   with bis_spmv, bis_dot, bis_elemwise_div_vectors / _mult_vectors (scale 1) and bis_scale: v_i = hash32(i) / 2^32 - 0.5
 *   (hash32 as above), then per step y = A v;  lambda_k = (v, y) / (v, v / w);  v = w o y;  v = v (1 / sqrt((v, v))).
 *   A Rayleigh quotient: for SPD A it never exceeds lambda_max(W A).  Not finite or not positive: it counts as 0.
 *   lambda_max = bound if estimate = 0, otherwise min(bound, safety estimate);  lambda_min = lambda_max / ratio.
 * Coefficients of level l, on the host in fp64, every operation its own rounded step:
 *   theta = (lambda_max + lambda_min) / 2, delta = (lambda_max - lambda_min) / 2, sigma = theta / delta, rho_0 = 1 / sigma;
 *   c1[0] = 0, c2[0] = 1 / theta;  k = 1 .. degree - 1: rho_k = 1 / (2 sigma - rho_{k-1}), c1[k] = rho_k rho_{k-1},
 *   c2[k] = (2 rho_k) / delta.
 * One polynomial on the current x, every product, difference and sum rounded separately (no fused multiply-add):
 *   k = 0 .. degree - 1:  y = A x by bis_spmv;  per row t = b - y, u = w t, d = (c1[k] d) + (c2[k] u), x = x + d;
 *   at k = 0, d = c2[0] u: the d of an earlier polynomial is not read.
 *   From x = 0 (the first sweep of every level visit) step 0 needs no SpMV: d = c2[0] (w b), x = d.
 * The coefficients are fixed when bis_mg_set_smoother returns and travel as kernel arguments.
 *
 * bis_mg_set_smoother blocks (it synchronises the stream first), computes the spectrum and the coefficients of every level
 * and allocates one more vector (d) per level, so bis_mg_apply still allocates nothing and never blocks.  d is live inside
 * one smoothing call only: the second visit of a level in a W or K transition reuses it.  It composes with bis_mg_set_cycle
 * in either order, on plain and smoothed hierarchies.  Setting JACOBI frees d and restores Jacobi's bits; for JACOBI the
 * other fields are ignored.  A failure leaves the hierarchy on Jacobi.
 * BIS_ERR_INVALID, nothing changed: null arguments, kind outside 0..1, degree outside 1..8, ratio not finite or <= 1,
 * est_steps outside 0..100, safety not finite or < 1.
 * bis_mg_smoother_info: what is set (a Jacobi hierarchy reports {0, 0, 0, 0, 0}).  bis_mg_level_spectrum (any pointer may be
 * NULL) and bis_mg_level_cheb_coeffs (arrays of `degree`; either may be NULL): BIS_ERR_INVALID on a Jacobi hierarchy and
 * on a level outside the hierarchy. */
enum { BIS_MG_SMOOTH_JACOBI = 0, BIS_MG_SMOOTH_CHEBYSHEV = 1 };
typedef struct {
    int kind;
    int degree;
    double ratio;
    int est_steps;
    double safety;
} bis_mg_smoother;
BIS_API bis_status bis_mg_set_smoother(bis_ctx *ctx, bis_mg *mg, const bis_mg_smoother *smoother);
BIS_API bis_status bis_mg_smoother_info(const bis_mg *mg, bis_mg_smoother *out);
BIS_API bis_status bis_mg_level_spectrum(const bis_mg *mg, int level, double *bound, double *estimate, double *lambda_max,
                                         double *lambda_min);
BIS_API bis_status bis_mg_level_cheb_coeffs(const bis_mg *mg, int level, double *c1, double *c2);

/* ---- block Jacobi (bis_bjacobi.hip); no reference counterpart -------------------------------------------------------------
 * M^-1 = diag(B_0^-1, B_1^-1, ...): the dense diagonal blocks of A over blocks of consecutive rows, inverted once on the
 * device and applied as a block-diagonal product.  No dependency between rows, any row order, 1..8 right-hand sides; SPD for
 * SPD A (with symmetrize, symmetric bit for bit).  Blocks of nx rows on a grid: line Jacobi.
 *
 * Blocks.  block_ptr == NULL: uniform blocks of block_size (1..32) consecutive rows, the last one shorter if n is not a
 * multiple.  Otherwise block b covers rows [block_ptr[b], block_ptr[b + 1]), block_ptr (host, n_blocks + 1 entries) starting
 * at 0, ascending strictly, ending at n, every block of 1..32 rows; block_size is then ignored.
 *
 * Extraction.  Block b covers rows and columns [s, e).  It starts as zeros; every entry of rows s .. e - 1 whose column lies
 * in [s, e) is added to its place in the row's storage order (repeated entries sum left to right); entries outside the range
 * are not read.
 *
 * Inversion.  Gauss-Jordan with partial pivoting on [B | I], every operation rounded on its own (no fused multiply-add).
 * Step k = 0 .. m - 1: the pivot row is the first row i >= k with the largest |a_ik| (p = k, then i ascending, p = i where
 * |a_ik| > |a_pk|); rows k and p are swapped; r = 1 / a_kk; row k becomes row k * r (all 2 m columns, a_kk included); every
 * other row i becomes a_ij - (f * a_kj) over all 2 m columns with f = a_ik taken before the update, the product rounded,
 * then the difference.  The right half is R = B^-1.  A pivot that is 0 or not finite: BIS_ERR_ZERO_DIAG.
 * symmetrize = 1: every R_ij becomes (R_ij + R_ji) * 0.5, so R equals its transpose bit for bit.
 *
 * Apply.  out_i = sum_j R_ij * in_j over the block's columns in ascending order: the first product starts the sum, every
 * further product is rounded and then added, every addition rounded (no fused multiply-add).  Column j of
 * bis_bj_mapply (1..8 interleaved columns, bis_spmm's layout) has the bits of bis_bj_apply on column j.  Both are
 * stream-ordered, allocate nothing and allow out == in (OUT == IN).  Streamed bytes: 8 sum_b m_b^2 + 16 n n_rhs; a handle
 * with a block_ptr also reads 12 bytes of index per block.
 *
 * BIS_ERR_INVALID: null arguments (params included), A not square, a row-range view, block_size outside 1..32, a block_ptr
 * that does not start at 0, does not ascend strictly, does not end at n or has a block of more than 32 rows, n_rhs outside
 * 1..8.  *out is written on success only, and a failing bis_bj_create leaves nothing allocated.  n = 0: BIS_OK, nothing is
 * launched.  bis_bj_create blocks; everything runs on the device without floating-point atomics: two creates and two
 * applies give the same bits.  A is not kept: the handle may outlive it. */
typedef struct bis_bj bis_bj;
typedef struct {
    int block_size;           /* 1..32: uniform blocks of consecutive rows, the last one shorter if n is not a multiple;
                                 ignored when block_ptr is given */
    const int32_t *block_ptr; /* host, n_blocks + 1 entries, block_ptr[0] = 0, strictly ascending, last = n,
                                 every block 1..32 rows; NULL: uniform */
    int64_t n_blocks;
    int symmetrize;           /* 1: every inverse block R becomes (R + R^T) * 0.5 elementwise (bit-symmetric) */
} bis_bj_params;
BIS_API bis_status bis_bj_create(bis_ctx *ctx, const bis_mat *A, const bis_bj_params *params, bis_bj **out);
BIS_API bis_status bis_bj_destroy(bis_ctx *ctx, bis_bj *bj);
BIS_API bis_status bis_bj_apply(bis_ctx *ctx, const bis_bj *bj, double *out, const double *in);
BIS_API bis_status bis_bj_mapply(bis_ctx *ctx, const bis_bj *bj, double *OUT, const double *IN, int n_rhs);
/* The handle as the preconditioner of type BIS_PC_BLOCK_JACOBI: an n x n matrix without entries that bj owns (bis_mat_destroy
 * on it does nothing) and that leads back to bj; every entry point but the preconditioner dispatch sees the zero matrix. */
BIS_API const bis_mat *bis_bj_operand(const bis_bj *bj);
/* Number of blocks, rows of the largest block, sum of m_b^2; any pointer may be NULL.  BIS_ERR_INVALID: null handle. */
BIS_API bis_status bis_bj_info(const bis_bj *bj, int64_t *n_blocks, int *max_block, int64_t *value_count);
/* The inverse blocks to the host: block b row-major at host_values[host_offsets[b]], host_offsets (n_blocks + 1 entries)
 * the running sum of m_b^2; either pointer may be NULL.  Blocking. */
BIS_API bis_status bis_bj_blocks(bis_ctx *ctx, const bis_bj *bj, double *host_values, int64_t *host_offsets);

/* ---- the operator surface (kernels.hpp) ------------------------------------ */
/* spmv / native_spmv, kernels.hpp:22-52: y = A x. */
BIS_API bis_status bis_spmv(bis_ctx *ctx, const bis_mat *A, const double *x,
                            double *y);
/* ---- several right-hand sides (no reference counterpart) ---------------------
 * Y = A X for n_rhs vectors stored interleaved (row-major n x n_rhs):
 * X[c*n_rhs + j], Y[r*n_rhs + j]; X has n_cols*n_rhs entries, Y n_rows*n_rhs.
 * 1 <= n_rhs <= 8.  The matrix is streamed once for all vectors.
 * Arithmetic: for every row r and column j, acc = 0.0, then for the row's
 * entries e in CRS storage order acc += val[e] * X[col[e]*n_rhs + j], the
 * product and the addition rounded separately (no fma), rows of any length in
 * the same left-to-right order.  Column j of the result therefore equals
 * bis_spmv on column j bit for bit on every matrix whose bis_spmv does not run
 * "spmv_wave_per_row_kernel" (that kernel alone uses fma and a lane tree).
 * n_rhs == 1 forwards to bis_spmv.  n_rhs < 1, n_rhs > 8, null pointers or
 * X == Y: BIS_ERR_INVALID; n_rows == 0: BIS_OK.  Stream-ordered, non-blocking,
 * allocates nothing (it works on the row-block tables bis_mat_create built). */
BIS_API bis_status bis_spmm(bis_ctx *ctx, const bis_mat *A, const double *X, double *Y, int n_rhs);
/* what the last bis_spmm on A launched, with its template instance:
 * "spmm_rowblock_kernel K=4 V=2 RP=32" (V: doubles per gather load),
 * "spmm_lane_serial_kernel K=3 RP=32" (a row too long for the LDS tile),
 * "bis_spmv K=1" (static string; "" before the first call). */
BIS_API const char *bis_mat_spmm_kernel(const bis_mat *A);
/* 12 nnz + rp_width (n_rows + 1) + 8 n_rhs (n_cols + n_rows): the bytes one bis_spmm moves at least */
BIS_API bis_status bis_mat_spmm_streamed_bytes(const bis_mat *A, int n_rhs, int64_t *bytes);
/* column j of an interleaved block <-> a plain vector of n entries (strided copies, stream-ordered) */
BIS_API bis_status bis_mvec_set_col(bis_ctx *ctx, double *X, int64_t n, int n_rhs, int j, const double *v);
BIS_API bis_status bis_mvec_get_col(bis_ctx *ctx, double *v, const double *X, int64_t n, int n_rhs, int j);

/* sptrsv / native_sptrsv, kernels.hpp:54-86: x = (D + L_strict)^-1 b,
 * natural row order arithmetic; x may alias b. */
BIS_API bis_status bis_sptrsv(bis_ctx *ctx, const bis_mat *L_strict, double *x,
                              const double *D, const double *b);
/* bsptrsv / native_bsptrsv, kernels.hpp:88-117: x = (D + U_strict)^-1 b. */
BIS_API bis_status bis_bsptrsv(bis_ctx *ctx, const bis_mat *U_strict,
                               double *x, const double *D, const double *b);
/* subtract_vectors, kernels.hpp:119-126: r = a - scale*b. */
BIS_API bis_status bis_subtract_vectors(bis_ctx *ctx, double *r,
                                        const double *a, const double *b,
                                        int64_t n, double scale);
/* sum_vectors, kernels.hpp:128-135: r = a + scale*b. */
BIS_API bis_status bis_sum_vectors(bis_ctx *ctx, double *r, const double *a,
                                   const double *b, int64_t n, double scale);
/* elemwise_mult_vectors, kernels.hpp:137-144: r = a*scale*b. */
BIS_API bis_status bis_elemwise_mult_vectors(bis_ctx *ctx, double *r,
                                             const double *a, const double *b,
                                             int64_t n, double scale);
/* elemwise_div_vectors, kernels.hpp:146-153: r = a/(scale*b). */
BIS_API bis_status bis_elemwise_div_vectors(bis_ctx *ctx, double *r,
                                            const double *a, const double *b,
                                            int64_t n, double scale);
/* compute_residual, kernels.hpp:155-162: tmp = A x; res = b - tmp. */
BIS_API bis_status bis_compute_residual(bis_ctx *ctx, const bis_mat *A,
                                        const double *x, const double *b,
                                        double *res, double *tmp);
/* euclidean_vec_norm, kernels.hpp:194-203 (blocking, host result). */
BIS_API bis_status bis_euclidean_vec_norm(bis_ctx *ctx, const double *v,
                                          int64_t n, double *result_host);
/* dot, kernels.hpp:205-212 (blocking, host result). */
BIS_API bis_status bis_dot(bis_ctx *ctx, const double *a, const double *b,
                           int64_t n, double *result_host);
/* stream-ordered variants: the scalar stays on the device (sum of squares,
 * not its root, for the norm) -- for fused / multi-GPU schedules. */
BIS_API bis_status bis_dot_dev(bis_ctx *ctx, const double *a, const double *b,
                               int64_t n, double *result_dev);
BIS_API bis_status bis_sumsq_dev(bis_ctx *ctx, const double *v, int64_t n,
                                 double *result_dev);
/* Device-scalar forms of the axpy-class kernels and the scalar algebra around
 * them: the factor is read from device memory when the kernel runs, so a
 * Krylov iteration needs no host round trip per dot product.  GMRES: the
 * modified Gram-Schmidt step (gmres.hpp:6-53: h = (w,v_j); w -= h v_j; ... ;
 * v_{n+1} = w * (1/||w||)) is j+2 stream-ordered reductions and ONE download
 * of the Hessenberg column instead of j+2 blocking dots; BiCGSTAB
 * (bicgstab.hpp:8-83): alpha, omega, beta stay on the device.  Same kernels,
 * same IEEE operations in the same order as the host-scalar forms: results
 * are bit-identical to them. */
/* One pass for "w -= (*scale_dev) * u; *result_dev = (w, v)" -- the axpy of
 * Gram-Schmidt step j fused with the dot of step j+1 (gmres.hpp:13-14,:25), or,
 * with v = NULL, with the sum of squares of the finished w (:36-38).  Bit-
 * identical to bis_subtract_vectors_dev followed by bis_dot_dev. */
BIS_API bis_status bis_axpy_dot_dev(bis_ctx *ctx, double *w, const double *u,
                                    const double *scale_dev, const double *v,
                                    int64_t n, double *result_dev);
BIS_API bis_status bis_subtract_vectors_dev(bis_ctx *ctx, double *r, const double *a,
                                            const double *b, int64_t n,
                                            const double *scale_dev);
BIS_API bis_status bis_sum_vectors_dev(bis_ctx *ctx, double *r, const double *a,
                                       const double *b, int64_t n,
                                       const double *scale_dev);
BIS_API bis_status bis_scale_dev(bis_ctx *ctx, double *r, const double *v,
                                 const double *scalar_dev, int64_t n);
/* out = a / b  (alpha, omega: bicgstab.hpp:34, :51) */
BIS_API bis_status bis_scalar_div(bis_ctx *ctx, double *out_dev, const double *a_dev,
                                  const double *b_dev);
/* out = (a / b) * (c / d)  (beta: bicgstab.hpp:71) */
BIS_API bis_status bis_scalar_ratio_product(bis_ctx *ctx, double *out_dev,
                                            const double *a_dev, const double *b_dev,
                                            const double *c_dev, const double *d_dev);
/* norm = sqrt(sumsq), inv = 1.0 / norm  (kernels.hpp:202, gmres.hpp:44-46) */
BIS_API bis_status bis_scalar_sqrt_inv(bis_ctx *ctx, double *norm_dev, double *inv_dev,
                                       const double *sumsq_dev);
/* scale, kernels.hpp:214-220: r = v*scalar. */
BIS_API bis_status bis_scale(bis_ctx *ctx, double *r, const double *v,
                             double scalar, int64_t n);
/* init_vector, kernels.hpp:236-241. */
BIS_API bis_status bis_init_vector(bis_ctx *ctx, double *v, double val,
                                   int64_t n);
/* copy_vector, kernels.hpp:252-257. */
BIS_API bis_status bis_copy_vector(bis_ctx *ctx, double *out, const double *in,
                                   int64_t n);
/* normalize_x, methods/jacobi.hpp:27-40:
 * x_new = (b - (x_new - D*x_old))/D. */
BIS_API bis_status bis_normalize_x(bis_ctx *ctx, double *x_new,
                                   const double *x_old, const double *D,
                                   const double *b, int64_t n);
/* dgemm_transpose1 as used at gmres.hpp:358 (kernels.hpp:259-271 with
 * n_cols_B = 1): out[i] = sum_{k<n_vec} V[k*ldv+i]*y[k]; y is a HOST array of
 * n_vec (<= 64) coefficients.  (The reference reads y[n_vec] one past the
 * end at a restart; the defined semantics is that term = 0.) */
BIS_API bis_status bis_multi_axpy(bis_ctx *ctx, const double *V, int64_t ldv,
                                  const double *y_host, int n_vec, double *out,
                                  int64_t n);
/* two_stage_gauss_seidel, kernels.hpp:312-333 (inner_iters =
 * PRECOND_INNER_ITERS). */
BIS_API bis_status bis_two_stage_gauss_seidel(bis_ctx *ctx,
                                              const bis_mat *strict,
                                              double *tmp, double *work,
                                              const double *D_inv,
                                              const double *input,
                                              double *output, int64_t n,
                                              int inner_iters);
/* Iterative triangular solve (no reference counterpart; the reference has the idea for Gauss-Seidel only,
 * two_stage_gauss_seidel): x ~ (D + T_strict)^-1 b for a strictly lower OR upper triangular T_strict (the same code: no
 * row depends on another inside a step), by n_sweeps Jacobi-Richardson steps.  D_inv holds 1 / D.  The arithmetic:
 *     x_0[i]     = D_inv[i] * b[i]
 *     s_i        = (T_strict x_k)[i]              exactly the value bis_spmv(T_strict, x_k) gives: same products, same order
 *     x_{k+1}[i] = (b[i] - s_i) * D_inv[i]        subtraction and multiplication rounded separately (no fma)
 * for k = 0 .. n_sweeps - 1.  T_strict is nilpotent: with as many steps as it has dependency levels the result is the
 * exact solve's up to rounding; fewer steps give the truncated Neumann series sum_{j <= n_sweeps} (-D^-1 T)^j D^-1 b.
 * x and work (n entries each) alternate as x_k; the result is in x for every n_sweeps >= 0 (work is not touched when
 * n_sweeps = 0 and may then be NULL).  x must not alias b, work or D_inv, work must not alias b or D_inv:
 * BIS_ERR_INVALID.  Stream-ordered, non-blocking; nothing is allocated once the SpMV form of T_strict exists (it is
 * built at the first bis_spmv / bis_itrsv / bis_mat_spmv_stream_info on T_strict, as for bis_spmv).
 * A step is one launch where that form is the CRS-value row-block kernel (the step is its epilogue), else the SpMV
 * in its form followed by one elementwise launch.  bis_itrsv_kernel names the path the last step on T_strict took:
 * "itrsv_fused_rowblock" or "itrsv spmv+epilogue form=F", F the form number of bis_mat_spmv_stream_info (static
 * string; "" before the first step). */
BIS_API bis_status bis_itrsv(bis_ctx *ctx, const bis_mat *T_strict, const double *D_inv,
                             const double *b, double *x, double *work, int n_sweeps);
BIS_API const char *bis_itrsv_kernel(const bis_mat *T_strict);
/* apply_preconditioner, kernels.hpp:336-414: output = M^-1 input
 * (outer_iters = PRECOND_OUTER_ITERS, inner_iters = PRECOND_INNER_ITERS).
 * BIS_PC_ILU0_ITER (8): tmp = bis_itrsv(L_strict, L_D, input, inner_iters), then output = bis_itrsv(U_strict,
 * A_D_inv, tmp, inner_iters).  L_D is the vector of ones of bis_mat_ilu0, its own reciprocal; for this type the
 * A_D_inv argument carries 1 / U_D (bis_elemwise_div_vectors(A_D_inv, L_D, U_D) after bis_mat_ilu0); A_D and U_D are
 * not read.  Scratch: tmp holds the lower solve's result and work (n entries, as for the two-stage types) is the
 * alternate buffer of both solves; the steps finish in place, so no third buffer is needed.  tmp and work must be
 * distinct from each other and from output and input (BIS_ERR_INVALID); output may alias input.
 * BIS_PC_FSAI (9): tmp = bis_spmv(L_strict, input), then output = bis_spmv(U_strict, tmp), with G in the L_strict and Gt
 * in the U_strict argument (bis_mat_fsai).  The diagonal arguments and work are not read; tmp is required and must be
 * distinct from input and output (BIS_ERR_INVALID); output may alias input.
 * BIS_PC_MG (10): output = bis_mg_apply(input) of the hierarchy whose operand (bis_mg_operand) is in the L_strict argument;
 * the operand must have n rows (BIS_ERR_INVALID), no other argument is read, output may alias input; outer_iters != 1:
 * BIS_ERR_UNSUPPORTED.
 * BIS_PC_BLOCK_JACOBI (11): output = bis_bj_apply(input) of the handle whose operand (bis_bj_operand) is in the L_strict
 * argument, under the rules of BIS_PC_MG: n rows or BIS_ERR_INVALID, nothing else read, output may alias input,
 * outer_iters != 1: BIS_ERR_UNSUPPORTED. */
BIS_API bis_status bis_apply_preconditioner(
    bis_ctx *ctx, int precond_type, int64_t n, const bis_mat *L_strict,
    const bis_mat *U_strict, const double *A_D, const double *A_D_inv,
    const double *L_D, const double *U_D, double *output, double *input,
    double *tmp, double *work, int outer_iters, int inner_iters);

/* ---- triangular sweeps and the preconditioner apply on several right-hand sides (no reference counterpart) ----
 * bis_spmm's layout throughout: n x n_rhs interleaved blocks, V[i*n_rhs + j], 1 <= n_rhs <= 8; D, D_inv, A_D ... are
 * plain n-vectors shared by all columns.
 *
 * bis_sptrsm / bis_bsptrsm: X_j = (D + T_strict)^-1 B_j for a strictly lower / upper triangular T_strict.  Arithmetic:
 * for every row r in dependency order and every column j, acc = 0.0; for the row's entries e in CRS storage order
 * acc = fma(val[e], X[col[e]*n_rhs + j], acc); then X[r*n_rhs + j] = (B[r*n_rhs + j] - acc) / D[r] -- native_sptrsv's
 * arithmetic (kernels.hpp:54-117) with the product and the sum fused, on every matrix.  Column j equals bis_sptrsv /
 * bis_bsptrsv on column j bit for bit wherever the single-vector sweep runs that chain: its tiled, chained, per-level,
 * wave-per-row and lane-per-row forms.  Its row-block form (a triangle of at most 64 contiguous blocks of mutually
 * independent rows: spmv_rowblock_kernel with the triangular epilogue) rounds each product before it adds, so there the
 * two agree bit for bit only where the products are exact (HPCG's and the FDM stencils' -1 entries), and to rounding
 * otherwise.  The columns never mix.
 * X may alias B.  n_rhs == 1 forwards to bis_sptrsv / bis_bsptrsv.  BIS_ERR_INVALID: n_rhs outside 1..8, null
 * pointers, a triangle that is not strictly lower / upper; n_rows == 0: BIS_OK.  Stream-ordered, non-blocking; nothing
 * is allocated after the first call on a side (which analyses the triangle: a plan of the multi-vector sweeps' own,
 * independent of the single-vector sweep's) -- except that the persistent form's scratch (8n + 8 words) and position
 * table are made at that form's first launch, which is a later call only where trsm_form switches forms.  Level-scheduled forms only -- one launch per level for triangles of at
 * most 64 levels, one persistent launch (a wave per row, lanes = (entry, column)) for every other; option trsm_form:
 * 1 / 2 forces the first / second.  A wait of the persistent form that gives up raises the context's fault word: the
 * next blocking call returns BIS_ERR_SYNC.  Inside a device schedule that has stopped the launches are no-ops.
 * bis_mat_sweepm_kernel: what the last multi-vector sweep of that side launched, with its instance
 * ("trsm_wave_kernel K=8 RP=32", "trsm_level_kernel K=3 RP=32", "bis_sptrsv K=1" / "bis_bsptrsv K=1"; static string,
 * "" before the first). */
BIS_API bis_status bis_sptrsm(bis_ctx *ctx, const bis_mat *L_strict, double *X, const double *D, const double *B, int n_rhs);
BIS_API bis_status bis_bsptrsm(bis_ctx *ctx, const bis_mat *U_strict, double *X, const double *D, const double *B, int n_rhs);
BIS_API const char *bis_mat_sweepm_kernel(const bis_mat *T, int backward);
/* R[i,j] = A[i,j] / (1.0 * D[i]) (elemwise_div_vectors per column) and R[i,j] = A[i,j] * 1.0 * D[i] (elemwise_mult_vectors
 * per column).  R may alias A. */
BIS_API bis_status bis_mvec_div_diag(bis_ctx *ctx, double *R, const double *A, const double *D, int64_t n, int n_rhs);
BIS_API bis_status bis_mvec_mul_diag(bis_ctx *ctx, double *R, const double *A, const double *D, int64_t n, int n_rhs);
/* bis_itrsv on every column: the same recurrence, the product from bis_spmm, one elementwise launch per step for
 * x = (b - s) * D_inv (subtraction and multiplication rounded separately).  Column j equals bis_itrsv on column j bit
 * for bit wherever bis_spmm's column j equals bis_spmv's: every matrix that does not run the wave-per-row SpMV.  X and
 * WORK are n x n_rhs blocks; the alias rules are bis_itrsv's.  n_rhs == 1 forwards to bis_itrsv. */
BIS_API bis_status bis_mitrsv(bis_ctx *ctx, const bis_mat *T_strict, const double *D_inv, const double *B, double *X,
                              double *WORK, int n_sweeps, int n_rhs);
/* bis_apply_preconditioner, call for call, on interleaved blocks: NONE a copy, JACOBI bis_mvec_div_diag, GS / BGS one
 * sweep, SGS sweep + bis_mvec_mul_diag + sweep, ILU0 two sweeps, ILU0_ITER two bis_mitrsv (scratch and alias rules of the
 * single-vector case; OUT may alias IN).  Column j equals bis_apply_preconditioner on column j bit for bit (the sweeps:
 * with bis_sptrsm's proviso; ILU0_ITER: with bis_mitrsv's).  BIS_PC_TWO_STAGE_GS, BIS_PC_SYMMETRIC_TWO_STAGE_GS and outer_iters != 1:
 * BIS_ERR_UNSUPPORTED.  TMP, WORK: n x n_rhs blocks, needed by SGS / ILU0 / ILU0_ITER / FSAI (TMP) and ILU0_ITER (WORK).
 * FSAI: two bis_spmm, TMP distinct from IN and OUT; column j equals the single-vector apply wherever bis_spmm's column j
 * equals bis_spmv's (every matrix that does not run the wave-per-row SpMV).  BIS_PC_MG has no multi-vector form:
 * BIS_ERR_UNSUPPORTED here and in bis_mcg_set_preconditioner, bis_mbicgstab_set_preconditioner, bis_mgmres_set_preconditioner.
 * BIS_PC_BLOCK_JACOBI has one: OUT = bis_bj_mapply(IN) of the handle whose operand is in L_strict (n rows, or BIS_ERR_INVALID);
 * nothing else is read, OUT may alias IN, and the three lock-step set_preconditioner calls take it and allocate no TMP or WORK. */
BIS_API bis_status bis_mapply_preconditioner(
    bis_ctx *ctx, int precond_type, int64_t n, int n_rhs, const bis_mat *L_strict,
    const bis_mat *U_strict, const double *A_D, const double *A_D_inv,
    const double *L_D, const double *U_D, double *OUT, double *IN,
    double *TMP, double *WORK, int outer_iters, int inner_iters);

/* ---- named kernels: the reference's plugin protocol --------------------------
 * The reference's accelerator seam (SMAX) registers each kernel once under a
 * name with persistent operands, runs it by name, and rebinds operands after
 * the solver's pointer swaps: utilities/smax_helpers.hpp:7-42
 * (register_kernel / register_A / register_B / register_C /
 * set_mat_upper_triang), kernels.hpp:48,82,113 (kernel(name)->run(0, offset,
 * 0)), jacobi.hpp:93 / kernels.hpp:329 (swap_operands), cg.hpp:136-152
 * (args->x->val = ...).  Same protocol here.  SPMV: C = A * B.  SPTRSV: solve
 * (D + A) B = C with A strictly triangular (the reference hands SMAX a
 * triangle with the diagonal inside; here D is a separate vector, as in the
 * native path, registered with bis_kernel_register_D). */
enum { BIS_KERNEL_SPMV = 0, BIS_KERNEL_SPTRSV = 1 };
BIS_API bis_status bis_register_kernel(bis_ctx *ctx, const char *name, int type);
BIS_API bis_status bis_kernel_register_A(bis_ctx *ctx, const char *name,
                                         const bis_mat *A);
BIS_API bis_status bis_kernel_register_B(bis_ctx *ctx, const char *name,
                                         int64_t size, double *vec);
BIS_API bis_status bis_kernel_register_C(bis_ctx *ctx, const char *name,
                                         int64_t size, double *vec);
BIS_API bis_status bis_kernel_register_D(bis_ctx *ctx, const char *name,
                                         const double *diag);
BIS_API bis_status bis_kernel_set_mat_upper_triang(bis_ctx *ctx,
                                                   const char *name, int flag);
/* offsets in elements, as in run(A_offset, B_offset, C_offset); A_offset must
 * be 0 (the reference never passes anything else). */
BIS_API bis_status bis_kernel_run(bis_ctx *ctx, const char *name,
                                  int64_t A_offset, int64_t B_offset,
                                  int64_t C_offset);
BIS_API bis_status bis_kernel_swap_operands(bis_ctx *ctx, const char *name);

/* ---- stationary solvers as device schedules (methods/jacobi.hpp:43-52, :79-107;
 * methods/gauss_seidel.hpp:26-52, :76-105, :119-129) -------------------------
 * Jacobi, Gauss-Seidel and symmetric Gauss-Seidel as SOLVERS: iteration, true
 * residual b - A x of every iterate (record_residual_norm), its norm and
 * check_stopping_criteria (solver.hpp:177-192) run on the device; no host read
 * per iteration.  Jacobi makes ONE SpMV per iteration -- the product A x_k that
 * samples iteration k's residual is the one iteration k+1 starts from -- and
 * fuses residual, norm partials and the step into one pass; the sampled norms are
 * bit-identical to bis_compute_residual + bis_euclidean_vec_norm of a 16-byte
 * aligned residual vector, whatever the alignment of b, D and x.  GS / SGS run
 * the reference's operations unchanged, stream-ordered.  After the stop test has
 * fired the remaining enqueued launches are no-ops (SpMVs and sweeps included).
 * x: x_0 on entry; read the result with bis_stat_solution (Jacobi alternates
 * between x and a buffer of its own).  D = diagonal of A; L_strict / U_strict
 * (bis_mat_split_strict) are needed for GS / SGS only. */
enum { BIS_STAT_JACOBI = 0, BIS_STAT_GS = 1, BIS_STAT_SGS = 2 };
typedef struct bis_stat bis_stat;
BIS_API bis_status bis_stat_create(bis_ctx *ctx, int kind, const bis_mat *A,
                                   const bis_mat *L_strict, const bis_mat *U_strict,
                                   const double *D, const double *b, double *x,
                                   bis_stat **out);
/* Reuse: bis_stat_init may be called again at any time, on a handle that is live, has stopped or holds NaN.  It reads b
 * and x as they are at that call (x as the new x_0; Jacobi's iterate is in x again, whichever buffer held it), discards
 * every earlier state -- iteration count, history, stop and converged flags -- and the solve that follows is, bit for
 * bit, that of a new handle on the same operands.  There is no set_preconditioner: the kind is fixed at creation. */
/* init_residual: ||b - A x_0|| (returned), stopping threshold tol * that. */
BIS_API bis_status bis_stat_init(bis_ctx *ctx, bis_stat *s, double tol,
                                 double *r0_norm_host);
/* enqueue n_iters iterations (no synchronisation) */
BIS_API bis_status bis_stat_iterate(bis_ctx *ctx, bis_stat *s, int n_iters);
/* blocking: iterations executed, converged flag, residual history [0..iters] */
BIS_API bis_status bis_stat_status(bis_ctx *ctx, bis_stat *s, int *iters,
                                   int *converged, double *hist_host, int hist_cap);
/* blocking: the iterate the last history entry belongs to, copied to x_out */
BIS_API bis_status bis_stat_solution(bis_ctx *ctx, bis_stat *s, double *x_out);
BIS_API bis_status bis_stat_destroy(bis_ctx *ctx, bis_stat *s);

/* ---- fused CG schedule (cg.hpp:6-54 + :162-166, same arithmetic, fewer
 * passes; SURVEY.md section 8d "fused lower bound") -------------------------- */
typedef struct bis_cg bis_cg;
/* Binds the operands of one CG solve: A, optional Jacobi diagonal (NULL: no
 * preconditioner), b, and x (in/out: x_0 on entry).  Owns p, r, z, tmp. */
BIS_API bis_status bis_cg_create(bis_ctx *ctx, const bis_mat *A,
                                 const double *A_D, const double *b, double *x,
                                 bis_cg **out);
BIS_API bis_status bis_cg_destroy(bis_ctx *ctx, bis_cg *cg);
/* General preconditioner for the fused CG (single GPU or distributed handle):
 * z = M^-1 r through bis_apply_preconditioner (kernels.hpp:336-414) with the
 * given operands (all LOCAL to this rank), instead of None / Jacobi.  Pass B
 * then updates r and (r,r) only; the sweep(s) and a stream-ordered (r,z) follow;
 * everything stays on the device as before.  Call before bis_cg_init.
 * BIS_PC_FSAI needs the two factors (G, Gt of bis_mat_fsai, of this rank's diagonal block on a distributed handle) and
 * nothing else: no diagonals, no work vector.  BIS_PC_MG needs the hierarchy's operand (bis_mg_operand, of the solver's
 * size) in L_strict and nothing else; on a distributed handle, or with outer_iters != 1: BIS_ERR_UNSUPPORTED.
 * BIS_PC_BLOCK_JACOBI: the same with the operand of a bis_bj handle (bis_bj_operand); no work vector is allocated, and a
 * distributed handle refuses it (blocks may straddle ranks). */
BIS_API bis_status bis_cg_set_preconditioner(bis_ctx *ctx, bis_cg *cg, int precond_type,
                                             const bis_mat *L_strict, const bis_mat *U_strict,
                                             const double *A_D, const double *A_D_inv,
                                             const double *L_D, const double *U_D,
                                             int outer_iters, int inner_iters);
/* Reuse: bis_cg_init may be called again at any time, on a handle that is live, has stopped or holds NaN.  It reads b
 * and x as they are at that call, discards every earlier state -- r, z, p, the scalars, the iteration count, the
 * history, the stop and converged flags -- and the solve that follows is, bit for bit, that of a new handle with the
 * same operands and preconditioner.  The preconditioner stays as set: bis_cg_set_preconditioner after the first
 * bis_cg_init (or bis_cg_iterate) is refused with BIS_ERR_INVALID, on a used handle as well. */
/* init_residual (cg.hpp:100-118) + init_stopping_criteria (solver.hpp:173):
 * r0 = b - A x0, z0 = M^-1 r0, p0 = z0; returns ||r0||_2 (blocking). */
BIS_API bis_status bis_cg_init(bis_ctx *ctx, bis_cg *cg, double tol,
                               double *r0_norm_host);
/* Runs up to `n_iters` iterations stream-ordered, no host round trip inside:
 * alpha/beta stay on the device, the stopping test of solver.hpp:177-192
 * (converged | NaN/inf) is evaluated on the device after every iteration and
 * later iterations become no-ops once it fires.  Residual norms are appended
 * to the solve's device history.  Non-blocking. */
BIS_API bis_status bis_cg_iterate(bis_ctx *ctx, bis_cg *cg, int n_iters);
/* Blocking: iterations actually performed so far, converged flag, and the
 * residual history (||r_0||..||r_k||, k = iterations) copied to hist_host
 * (capacity hist_cap doubles; may be NULL). */
BIS_API bis_status bis_cg_status(bis_ctx *ctx, bis_cg *cg, int *iters,
                                 int *converged, double *hist_host,
                                 int hist_cap);

/* ---- k CG solves in lock-step on one matrix stream (no reference counterpart) --
 * Per column j exactly the recurrences, the recorded norm, the history and the
 * stop test (threshold tol * ||r0_j||) of bis_cg_*; one iteration is bis_spmm on
 * P, the k sums (AP_j, P_j), pass B on R / Z with 2 k sums, pass C on X / P.
 * Scalars, histories and flags live on the device per column; every reduction
 * is summed in index order by the last arriver (deterministic; not bis_cg's
 * tree: parity with bis_cg holds at the history gate, not bit for bit).  The
 * columns never mix: no bit of a column depends on another column's data.  A
 * column that has stopped (converged or diverged) is frozen as bis_cg freezes:
 * pass C of the stopping iteration still updates its x, after that nothing of
 * it changes.  When every column has stopped, every later launch is a no-op.
 * A square; A_D NULL (no preconditioner) or the diagonal (Jacobi), n entries,
 * shared by all columns; B, X: n x n_rhs interleaved (bis_spmm's layout); X
 * holds the n_rhs start vectors on entry and is updated in place. */
typedef struct bis_mcg bis_mcg;
BIS_API bis_status bis_mcg_create(bis_ctx *ctx, const bis_mat *A, const double *A_D, const double *B, double *X,
                                  int n_rhs, bis_mcg **out);
/* General preconditioner, as bis_cg_set_preconditioner: Z = M^-1 R through bis_mapply_preconditioner.  Pass B then
 * updates R and (r,r) only; the apply, the k sums (r_j, z_j) with the per-column bookkeeping, and pass C follow.  The
 * handle owns the Z, TMP and WORK blocks the type needs.  Call before bis_mcg_init: BIS_ERR_INVALID afterwards; the
 * two-stage types and outer_iters != 1: BIS_ERR_UNSUPPORTED.  A stopped column stays frozen as without the call (the
 * apply may still compute its z, which nothing reads).  BIS_PC_FSAI (also in bis_mbicgstab_set_preconditioner and
 * bis_mgmres_set_preconditioner): the two factors and the TMP block, no diagonals and no WORK. */
BIS_API bis_status bis_mcg_set_preconditioner(bis_ctx *ctx, bis_mcg *m, int precond_type,
                                              const bis_mat *L_strict, const bis_mat *U_strict,
                                              const double *A_D, const double *A_D_inv,
                                              const double *L_D, const double *U_D,
                                              int outer_iters, int inner_iters);
/* Reuse: bis_mcg_init may be called again at any time, whatever the columns' states (live, stopped at different
 * iterations, NaN).  It reads B and X as they are at that call and discards every earlier state of every column --
 * the frozen bits, counts, histories and scalars included; the solve that follows is, bit for bit, that of a new
 * handle.  bis_mcg_set_preconditioner stays refused (BIS_ERR_INVALID) once bis_mcg_init has run. */
/* r0 = b - A x0, z0, p0 per column; r0_norms_host (n_rhs entries, may be NULL) receives ||r0_j||_2 (blocking) */
BIS_API bis_status bis_mcg_init(bis_ctx *ctx, bis_mcg *m, double tol, double *r0_norms_host);
BIS_API bis_status bis_mcg_iterate(bis_ctx *ctx, bis_mcg *m, int n_iters); /* non-blocking */
/* blocking: column j's iterations, converged flag and residual history [0..iters] */
BIS_API bis_status bis_mcg_status(bis_ctx *ctx, bis_mcg *m, int j, int *iters, int *converged, double *hist_host,
                                  int hist_cap);
BIS_API bis_status bis_mcg_destroy(bis_ctx *ctx, bis_mcg *m);

/* ---- k BiCGSTAB solves in lock-step (no reference counterpart) -----------------
 * Per column j the left-preconditioned iteration of methods/bicgstab.hpp:8-83 with
 * its init (:147-169: the shadow residual and p_0 are the PRECONDITIONED initial
 * residual, rho_0 = (r_0, M^-1 r_0)), the recorded norm ||r_j|| and the stop test
 * (threshold tol * ||r0_j||) of solver.hpp:177-192.  One iteration issues two
 * bis_mapply_preconditioner and two bis_spmm calls for all columns, and five
 * elementwise / reduction passes over n x n_rhs blocks between them; the
 * elementwise arithmetic is that of bis_subtract_vectors / bis_sum_vectors (one
 * fma) and bis_scalar_ratio_product.  Scalars, histories and flags live on the
 * device per column; nothing is read back inside bis_mbicgstab_iterate.  Layout,
 * reductions (last arriver, index order: deterministic, not bis_dot's tree) and the
 * independence of the columns are bis_mcg_*'s: no bit of a column depends on
 * another column's data; parity with a BiCGSTAB made of the single-vector calls
 * holds at the history gate, not bit for bit.  A column that has stopped is frozen:
 * the stopping iteration has updated its x (the reference's x_new of that
 * iteration), after that nothing of it changes; when every column has stopped,
 * every later launch is a no-op.  A breakdown (rho, (r0~, v) or (z, z) reaching 0)
 * gives a non-finite norm: that column stops with converged = 0, the others go on.
 * Arguments, error codes and the order of calls are bis_mcg_*'s, call for call:
 * A square, 1 <= n_rhs <= 8; B, X n x n_rhs interleaved, X holds the start vectors
 * and is updated in place; set_preconditioner before init (BIS_ERR_INVALID after),
 * two-stage types and outer_iters != 1 BIS_ERR_UNSUPPORTED, a missing operand
 * BIS_ERR_INVALID; without the call the solve is unpreconditioned (and keeps no
 * Y / S~ blocks: Y is P, S~ is S).  n = 0: BIS_OK, nothing is launched. */
typedef struct bis_mbicgstab bis_mbicgstab;
BIS_API bis_status bis_mbicgstab_create(bis_ctx *ctx, const bis_mat *A, const double *B, double *X, int n_rhs,
                                        bis_mbicgstab **out);
BIS_API bis_status bis_mbicgstab_set_preconditioner(bis_ctx *ctx, bis_mbicgstab *m, int precond_type,
                                                    const bis_mat *L_strict, const bis_mat *U_strict,
                                                    const double *A_D, const double *A_D_inv,
                                                    const double *L_D, const double *U_D,
                                                    int outer_iters, int inner_iters);
/* Reuse: as bis_mcg_init -- bis_mbicgstab_init may be called again at any time, reads B and X as they are then, and
 * discards every earlier state of every column (frozen bits, a breakdown's NaN, counts, histories, scalars); the
 * solve that follows is, bit for bit, that of a new handle.  bis_mbicgstab_set_preconditioner stays refused
 * (BIS_ERR_INVALID) once bis_mbicgstab_init has run. */
/* r0_norms_host (n_rhs entries, may be NULL) receives ||r0_j||_2 (blocking) */
BIS_API bis_status bis_mbicgstab_init(bis_ctx *ctx, bis_mbicgstab *m, double tol, double *r0_norms_host);
BIS_API bis_status bis_mbicgstab_iterate(bis_ctx *ctx, bis_mbicgstab *m, int n_iters); /* non-blocking */
/* blocking: column j's iterations, converged flag and residual history [0..iters] */
BIS_API bis_status bis_mbicgstab_status(bis_ctx *ctx, bis_mbicgstab *m, int j, int *iters, int *converged,
                                        double *hist_host, int hist_cap);
BIS_API bis_status bis_mbicgstab_destroy(bis_ctx *ctx, bis_mbicgstab *m);

/* ---- k restarted GMRES(m) solves in lock-step (no reference counterpart) -------
 * Per column j the left-preconditioned GMRES(m) of methods/gmres.hpp: init
 * R = B - A X, history entry 0 the UNPRECONDITIONED ||R_j||, threshold
 * tol * ||R_j||, then R = M^-1 R, beta_j = ||R_j||, V_0 = R / beta_j.  At position
 * n of a cycle (n = iterations mod restart_len, the same for every live column):
 * W = M^-1 A V_n, modified Gram-Schmidt in the reference's order (h_i = (W, V_i),
 * W -= h_i V_i, i = 0 .. n; one fma per element, fma-accumulated dots),
 * h_{n+1} = ||W||, V_{n+1} = W / h_{n+1}; the new Hessenberg column is rotated by
 * the stored Givens rotations, the new one is c = a / den, s = b / den with
 * den = sqrt(a^2 + b^2); the history entry is |g_{n+1}|, the estimate of the
 * preconditioned residual; the stop test is bis_mcg_*'s (< threshold, non-finite,
 * NaN).  At the end of a cycle the columns that go on restart: y by back
 * substitution (y[n] = 0 where the reference reads one past the end),
 * X += sum y_i V_i, R = M^-1 (B - A X), beta_j = ||R_j||, which is written as ONE
 * MORE history entry (Solver::init_residual) and tested against the threshold,
 * V_0 = R / beta_j.  So a column's history has iters + 1 + restarts entries:
 * bis_mgmres_status returns that count as n_hist.
 * One iteration at position n issues one bis_spmm, one bis_mapply_preconditioner
 * (in place), n + 2 fused Gram-Schmidt / reduction passes and one scale for all
 * columns (56 + 32 n bytes per row and column besides the SpMM and the apply);
 * coefficients, rotations, g, y, histories and flags live on the device per column
 * and nothing is read back inside bis_mgmres_iterate.  Layout, reductions (last
 * arriver, index order: deterministic, not bis_dot's tree) and the independence of
 * the columns are bis_mcg_*'s: no bit of a column depends on another column's data
 * (its bits depend on n, n_rhs, restart_len and its own data); parity with a GMRES
 * made of the single-vector calls holds at the history gate, not bit for bit.
 * X is only ever updated by adding V y: while a column is live inside a cycle its
 * X is x_old (bis_mgmres_solution gives the explicit iterate).  A column that stops
 * gets the y of its own cycle's steps added to X before the bis_mgmres_iterate call
 * that stopped it has enqueued its last kernel; after that nothing of it changes.
 * When every column has stopped, every later launch is a no-op.  b_j = 0 with
 * x0_j = 0 (beta = 0) stops at iteration 1, not converged; a lucky breakdown
 * (h_{n+1} = 0) gives the estimate 0 and converges in that iteration.
 * Memory: the basis is restart_len + 1 blocks, one more block W, so
 * (restart_len + 2) n n_rhs doubles, plus at most two blocks of scratch for the
 * preconditioner (SGS, ILU0: one; ILU0_ITER: two) and
 * n_rhs (restart_len^2 + 6 restart_len + 5) doubles of per-column state.
 * Arguments, error codes and the order of calls are bis_mbicgstab_*'s: A square,
 * 1 <= n_rhs <= 8, 1 <= restart_len <= 64 (bis_multi_axpy's limit); B, X
 * n x n_rhs interleaved, X holds the start vectors and is updated in place;
 * set_preconditioner before init (BIS_ERR_INVALID after), two-stage types and
 * outer_iters != 1 BIS_ERR_UNSUPPORTED, a missing operand BIS_ERR_INVALID; without
 * the call the solve is unpreconditioned.  n = 0: BIS_OK, nothing is launched. */
typedef struct bis_mgmres bis_mgmres;
BIS_API bis_status bis_mgmres_create(bis_ctx *ctx, const bis_mat *A, const double *B, double *X, int n_rhs,
                                     int restart_len, bis_mgmres **out);
BIS_API bis_status bis_mgmres_set_preconditioner(bis_ctx *ctx, bis_mgmres *m, int precond_type,
                                                 const bis_mat *L_strict, const bis_mat *U_strict,
                                                 const double *A_D, const double *A_D_inv,
                                                 const double *L_D, const double *U_D,
                                                 int outer_iters, int inner_iters);
/* Reuse: bis_mgmres_init may be called again at any time, inside a cycle as well.  It reads B and X as they are at
 * that call and discards every earlier state of every column: the cycle position starts at 0 again, the basis, the
 * rotations, g, the pending combine, the frozen bits, counts and histories are dropped, NaN included;
 * bis_mgmres_solution straight after it gives X.  The solve that follows is, bit for bit, that of a new handle.
 * bis_mgmres_set_preconditioner stays refused (BIS_ERR_INVALID) once bis_mgmres_init has run. */
/* r0_norms_host (n_rhs entries, may be NULL) receives the unpreconditioned ||r0_j||_2 (blocking) */
BIS_API bis_status bis_mgmres_init(bis_ctx *ctx, bis_mgmres *m, double tol, double *r0_norms_host);
/* non-blocking; the cycle position persists across calls (no call boundary restarts a cycle) */
BIS_API bis_status bis_mgmres_iterate(bis_ctx *ctx, bis_mgmres *m, int n_iters);
/* blocking: the explicit x of every column into X_out (n x n_rhs interleaved, not X itself): X_j for a stopped column,
 * X_j + V y at the current step for a live one (the reference's save_x_star for a run that ends on an iteration
 * budget).  The handle's state does not change. */
BIS_API bis_status bis_mgmres_solution(bis_ctx *ctx, bis_mgmres *m, double *X_out);
/* blocking: column j's iterations, converged flag, the number of history entries (iters + 1 + restarts) and the
 * first min(n_hist, hist_cap) of them */
BIS_API bis_status bis_mgmres_status(bis_ctx *ctx, bis_mgmres *m, int j, int *iters, int *converged, int *n_hist,
                                     double *hist_host, int hist_cap);
BIS_API bis_status bis_mgmres_destroy(bis_ctx *ctx, bis_mgmres *m);

/* ---- restarted flexible GMRES(m) on one right-hand side, a device schedule (no reference counterpart) -------
 * Saad's FGMRES: the preconditioner stands on the RIGHT and the preconditioned basis
 * Z_n = M_n^-1 V_n is kept, so M_n may be a different operator at every step -- a
 * K-cycle of bis_mg_* (BIS_MG_CYCLE_K, BIS_MG_CYCLE_K_GCR), any inner iteration --
 * where bis_mgmres_* and the host's -gm assume one fixed M.  The residual that is
 * minimised, estimated and recorded is the TRUE residual || b - A x ||, the quantity
 * bis_cg_* records and the stopping test is written for.
 * init: R = b - A x; history entry 0 is ||R||; threshold = tol ||R||; beta = ||R||;
 * V_0 = R (1 / beta).  At position n of a cycle (n = iterations mod restart_len):
 * Z_n = M^-1 V_n by bis_apply_preconditioner, straight into block n of Z (V_n
 * survives: with outer_iters > 1 the apply writes its input, and is handed a copy);
 * W = A Z_n by bis_spmv; modified Gram-Schmidt against V_0 .. V_n in the reference's
 * order (h_i = (W, V_i), W -= h_i V_i; one fma per element, fma-accumulated dots);
 * h_{n+1} = ||W||, V_{n+1} = W (1 / h_{n+1}); the new Hessenberg column is rotated by
 * the stored Givens rotations, the new one is c = a / den, s = b / den with
 * den = sqrt(a^2 + b^2); g_{n+1} = -s g_n, g_n = c g_n; the history entry is
 * |g_{n+1}|, here the estimate of the true residual norm; the stop test is
 * bis_mgmres_*'s (< threshold, non-finite, NaN).  At the end of a cycle, or at a
 * stop: y by back substitution, x_i += sum_c y_c Z_c[i] (the sum from 0 over
 * ascending c by fma, then added to x_i).  Restart: R = b - A x, beta = ||R|| with
 * NO preconditioner apply; beta is written as ONE MORE history entry and tested
 * against the threshold, V_0 = R (1 / beta).  So the history has iters + 1 +
 * restarts entries: bis_fgmres_status returns that count as n_hist.
 * Without a preconditioner FGMRES is GMRES: the histories of bis_fgmres_* and of
 * bis_mgmres_* with n_rhs = 1 agree at the history gate (their reductions add in
 * different orders).  With one, history entry k of the two differs: there the
 * preconditioned, here the true residual.
 * One iteration at position n issues one apply, one SpMV, n + 2 fused Gram-Schmidt /
 * reduction passes and one scale, all single-vector kernels on 16-byte accesses
 * (56 + 32 n bytes per row besides the SpMV and the apply); the reductions go by
 * per-workgroup partial sums that the workgroup arriving last adds in index order
 * (no floating-point atomics: two runs give the same bits); coefficients, rotations,
 * g, y, the history and the flags live on the device and nothing is read back inside
 * bis_fgmres_iterate.  x changes only at a restart or a stop; in between
 * bis_fgmres_solution gives x + Z y.  After the stop no later call changes x, the
 * history or the status: every launch of the schedule returns at once (launches of
 * the preconditioner queued behind the stop may still run; their results are
 * discarded).  b = 0 with x0 = 0 (beta = 0) stops at iteration 1, not converged; a
 * lucky breakdown (h_{n+1} = 0) gives the estimate 0 and converges in that iteration.
 * Memory: V is restart_len + 1 blocks, Z restart_len blocks, one more block W:
 * (2 restart_len + 2) n doubles with a preconditioner, (restart_len + 2) n without
 * (BIS_PC_NONE, or no set_preconditioner call: Z_n IS V_n, no Z storage and no copy;
 * n counts rounded up to even, so that every block starts on 16 bytes), plus the
 * preconditioner's scratch (SGS, ILU0, FSAI: one block; the two-stage types and
 * ILU0_ITER: two; MG: the hierarchy's own) and restart_len^2 + 6 restart_len + 5
 * doubles of state.
 * Arguments, error codes and the order of calls are bis_mgmres_*'s with n_rhs = 1:
 * A square, 1 <= restart_len <= 64; b and x n-vectors on 16-byte boundaries
 * (bis_vec_alloc's are), x holds the start vector and is updated in place;
 * set_preconditioner before init (BIS_ERR_INVALID after); a missing operand
 * BIS_ERR_INVALID; n = 0: BIS_OK, nothing is launched.  The one difference:
 * set_preconditioner takes EVERY type and every outer_iters / inner_iters that
 * bis_apply_preconditioner takes -- the two-stage types, outer_iters > 1, and
 * BIS_PC_MG (the hierarchy's operand in L_strict) with any cycle -- and refuses what
 * that call refuses with its status: an MG operand of another size
 * BIS_ERR_INVALID, MG with outer_iters != 1 BIS_ERR_UNSUPPORTED.
 * BIS_PC_BLOCK_JACOBI (the operand of a bis_bj handle in L_strict): as BIS_PC_MG. */
typedef struct bis_fgmres bis_fgmres;
BIS_API bis_status bis_fgmres_create(bis_ctx *ctx, const bis_mat *A, const double *b, double *x, int restart_len,
                                     bis_fgmres **out);
BIS_API bis_status bis_fgmres_set_preconditioner(bis_ctx *ctx, bis_fgmres *s, int precond_type,
                                                 const bis_mat *L_strict, const bis_mat *U_strict,
                                                 const double *A_D, const double *A_D_inv,
                                                 const double *L_D, const double *U_D,
                                                 int outer_iters, int inner_iters);
/* Reuse: bis_fgmres_init may be called again at any time, inside a cycle as well.  It reads b and x as they are at
 * that call and discards every earlier state: the cycle position starts at 0 again, V, Z, the rotations, g, a pending
 * combine, the count and the history are dropped, NaN included; bis_fgmres_solution straight after it gives x.  The
 * solve that follows is, bit for bit, that of a new handle.  bis_fgmres_set_preconditioner stays refused
 * (BIS_ERR_INVALID) once bis_fgmres_init has run. */
/* r0_norm_host (may be NULL) receives ||b - A x0||_2 (blocking) */
BIS_API bis_status bis_fgmres_init(bis_ctx *ctx, bis_fgmres *s, double tol, double *r0_norm_host);
/* non-blocking; the cycle position persists across calls (no call boundary restarts a cycle) */
BIS_API bis_status bis_fgmres_iterate(bis_ctx *ctx, bis_fgmres *s, int n_iters);
/* blocking: the explicit iterate into x_out (n entries on a 16-byte boundary, not x itself): x once the solve has
 * stopped, x + Z y at the current step while it is live.  The handle's state does not change. */
BIS_API bis_status bis_fgmres_solution(bis_ctx *ctx, bis_fgmres *s, double *x_out);
/* blocking: iterations, converged flag, the number of history entries (iters + 1 + restarts) and the first
 * min(n_hist, hist_cap) of them */
BIS_API bis_status bis_fgmres_status(bis_ctx *ctx, bis_fgmres *s, int *iters, int *converged, int *n_hist,
                                     double *hist_host, int hist_cap);
BIS_API bis_status bis_fgmres_destroy(bis_ctx *ctx, bis_fgmres *s);

/* ---- MINRES on the device (no reference counterpart) ---------------------------
 * Preconditioned MINRES (Paige-Saunders) for a SYMMETRIC A, definite or not, and one
 * fixed symmetric positive definite M: the method for shift-and-invert systems
 * (H - sigma I) x = b with sigma inside the spectrum, where CG is not defined.  One
 * SpMV, one apply and two reductions per iteration, seven n-vectors at any iteration
 * count; the residual norm never increases; on SPD matrices it does what CG does.
 * Without a preconditioner z = M^-1 r is r itself.
 * init: r1 = b - A x0; y = M^-1 r1; beta1 = sqrt((r1, y)); r2 = r1; w = w2 = 0;
 * oldb = 0, beta = beta1, dbar = 0, epsln = 0, phibar = beta1, cs = -1, sn = 0.
 * History entry 0 is beta1, the value bis_minres_init returns; threshold = tol beta1.
 * Iteration k = 1, 2, ...:
 *     v = y (1/beta);  y = A v;  if k >= 2: y = y - (beta/oldb) r1
 *     alpha = (v, y);  y = y - (alpha/beta) r2;  r1 <- r2;  r2 <- y;  y = M^-1 r2
 *     oldb = beta;  beta = sqrt((r2, y))
 *     oldeps = epsln;  delta = cs dbar + sn alpha;  gbar = sn dbar - cs alpha;
 *     epsln = sn beta;  dbar = -cs beta
 *     gamma = sqrt(gbar^2 + beta^2);  cs = gbar/gamma;  sn = beta/gamma;
 *     phi = cs phibar;  phibar = sn phibar
 *     w1 <- w2;  w2 <- w;  w = (v - oldeps w1 - delta w2) (1/gamma);  x = x + phi w
 *     history[k] = phibar;  stop if phibar < threshold (converged) or phibar is not
 *     finite (not converged)
 * phibar_k is ||r_k|| in the M^-1 norm; without a preconditioner it is ||b - A x_k||_2.
 * Rounding: every "vector - scalar * vector" above and x + phi w is one fma per
 * element (the product is not rounded); the factors beta/oldb, alpha/beta, 1/gamma and
 * 1/beta are formed first, one division each, and the scalings by 1/gamma and 1/beta
 * are multiplications of their own.  The fused dots are bis_dot's: its grid, index map,
 * two fma chains per lane and its order of the block and partial sums, which the
 * workgroup that arrives last adds (no floating-point atomics, no waiting): two runs
 * give the same bits.  The scalar lines round every operation separately.  So the
 * history and x are, bit for bit, those of the same iteration made of bis_spmv,
 * bis_dot, bis_subtract_vectors / bis_sum_vectors, bis_scale and
 * bis_apply_preconditioner with the scalar lines in IEEE double on the host.
 * Edge cases: beta = 0 with gamma != 0 is a lucky breakdown, phibar = 0, converged in
 * that iteration; (r2, y) < 0 (M not positive definite) makes beta NaN and the solve
 * stops, not converged, with that NaN in the history; b = 0 with x0 = 0 stops at
 * iteration 1, not converged, as bis_fgmres_* does.
 * Schedule per iteration: the SpMV; pass B (the r1 term with the partial sums of (v, y)
 * fused); pass C (the r2 term; without a preconditioner the sums of (y, y) fused; with
 * Jacobi, outer_iters = 1 and A_D on a 16-byte boundary (bis_vec_alloc's are; any
 * other A_D takes the general path, same bits) the division by D and (r2, y)
 * fused; every other type: bis_apply_preconditioner, then the dot as one more
 * pass), whose last workgroup does
 * the scalar lines, the history, the count and the stop test in one lane; pass D (w,
 * x and the next v in one pass).  r1 <- r2 <- y and w1 <- w2 <- w rotate buffers by
 * the iteration number, they are never copies.  Beside the SpMV and the apply that is
 * 120 bytes per row and iteration (B 32, C 24, D 64; the fused CG moves 92), 136 with
 * Jacobi or with the dot pass of the other types.  Memory: 7 n doubles (n rounded up
 * to even) and the history, plus the preconditioner's scratch (SGS, ILU0, FSAI: one
 * n-vector; the two-stage types and ILU0_ITER: two; MG: the hierarchy's own).
 * Scalars, history and the stop flag stay on the device; bis_minres_iterate reads
 * nothing back.  After the stop every launch returns at once except pass D of the
 * stopping iteration, so x is the iterate the last history entry belongs to, and no
 * later call changes x, the history or the status (launches of the preconditioner
 * queued behind the stop may still run; nothing reads their results).
 * bis_minres_set_preconditioner takes the arguments of bis_fgmres_set_preconditioner:
 * every type, outer_iters and inner_iters that bis_apply_preconditioner takes for one
 * vector, BIS_PC_MG (the hierarchy's operand in L_strict) and BIS_PC_BLOCK_JACOBI (the
 * handle's operand there; create it with symmetrize = 1) included.  The library does
 * NOT check that M is symmetric positive definite.  GS and BGS alone, an ILU(0) of a
 * nonsymmetric factorisation, the two-stage types with few inner steps and the MG
 * K-cycles (BIS_MG_CYCLE_K, BIS_MG_CYCLE_K_GCR) are not such operators: MINRES with
 * them is undefined (use bis_fgmres_*).  Call it before bis_minres_init.
 * Errors: null arguments, a non-square A, b or x off a 16-byte boundary,
 * set_preconditioner after init, a missing operand, an MG operand of another size:
 * BIS_ERR_INVALID; MG with outer_iters != 1: BIS_ERR_UNSUPPORTED; n = 0: BIS_OK,
 * nothing is launched; *out is written on success only. */
typedef struct bis_minres bis_minres;
BIS_API bis_status bis_minres_create(bis_ctx *ctx, const bis_mat *A, const double *b, double *x, bis_minres **out);
BIS_API bis_status bis_minres_set_preconditioner(bis_ctx *ctx, bis_minres *s, int precond_type,
                                                 const bis_mat *L_strict, const bis_mat *U_strict,
                                                 const double *A_D, const double *A_D_inv,
                                                 const double *L_D, const double *U_D,
                                                 int outer_iters, int inner_iters);
/* Reuse: bis_minres_init may be called again at any time (after a failed bis_minres_iterate it must be).  It reads b
 * and x as they are at that call and discards every earlier state: the buffer rotations of r1, r2, y and w1, w2, w
 * start at iteration 1 again, w and w2 are zero, the scalars, the count, the history and the flags are dropped, NaN
 * included.  The solve that follows is, bit for bit, that of a new handle.  bis_minres_set_preconditioner stays
 * refused (BIS_ERR_INVALID) once bis_minres_init has run. */
/* blocking; r0_norm_host (may be NULL) receives beta1 */
BIS_API bis_status bis_minres_init(bis_ctx *ctx, bis_minres *s, double tol, double *r0_norm_host);
/* non-blocking: enqueues n_iters iterations */
BIS_API bis_status bis_minres_iterate(bis_ctx *ctx, bis_minres *s, int n_iters);
/* blocking: iterations, converged flag, history entries 0 .. iterations (at most hist_cap of them; may be NULL) */
BIS_API bis_status bis_minres_status(bis_ctx *ctx, bis_minres *s, int *iters, int *converged, double *hist_host,
                                     int hist_cap);
BIS_API bis_status bis_minres_destroy(bis_ctx *ctx, bis_minres *s);

/* ---- IDR(s) on the device (no reference counterpart) ---------------------------
 * Right-preconditioned IDR(s) with biorthogonalisation (Sonneveld and van Gijzen),
 * 1 <= s <= 8, for a nonsymmetric A and one right-hand side: short recurrences, no
 * restart, one SpMV, one preconditioner apply and one history entry per iteration,
 * 3 s + 3 n-vectors at any iteration count.
 * State: the n-vectors r, v, t; the column blocks P (the shadow space), G, U of s
 * n-vectors each; the s x s lower-triangular M; f, c, alpha (s entries each), omega
 * and ||r||.  One iteration is one position of a cycle of s + 1 positions:
 *   init:  r = b - A x;  history[0] = ||r||;  threshold = tol history[0];  G = U = 0;
 *          M = I;  omega = 1;  f = P^T r;  position 0
 *   position k < s:
 *     c[k..s):  forward substitution  M[k.., k..] c = f[k..]
 *     v   = r - sum_{j >= k} c_j G_j
 *     v^  = M^-1 v                        (bis_apply_preconditioner; v^ is v without one)
 *     U_k = omega v^ + sum_{j >= k} c_j U_j
 *     G_k = A U_k                         (bis_spmv)
 *     q   = P^T G_k                       (s dots in one pass over G_k)
 *     alpha_i = (q_i - sum_{l < i} M_il alpha_l) / M_ii         for i < k
 *     M_ik    =  q_i - sum_{l < k} M_il alpha_l                 for i >= k
 *     G_k -= sum_{i < k} alpha_i G_i;   U_k -= sum_{i < k} alpha_i U_i
 *     beta = f_k / M_kk;   r -= beta G_k;   x += beta U_k;   f_i -= beta M_ik for i > k
 *     history[it] = ||r||;  stop test
 *   position s:
 *     v^ = M^-1 r;  t = A v^;  tt = (t, t), tr = (t, r);  omega = tr / tt;
 *     rho = |tr| / (sqrt(tt) ||r||);  if rho < 0.7: omega = omega 0.7 / rho
 *     x += omega v^;  r -= omega t;  history[it] = ||r||;  stop test;  f = P^T r;
 *     position 0
 * The alpha line is the one deliberate change from the published loop, which takes
 * one dot (p_i, G_k) and updates G_k and U_k once for every i < k in turn.  M is
 * lower triangular (p_i is orthogonal to G_l for l > i), so every alpha follows from
 * the ONE multi-dot q by a forward substitution, and the new column of M from the
 * same q: one reduction pass and one update pass at every k instead of 2 (k - 1).
 * In exact arithmetic it is the same method; the two forms, restated in numpy, needed
 * the same number of products to within 3 on the tests' inputs.
 * The stop test is the other handles': ||r|| < threshold stops the solve as
 * converged, a non-finite ||r|| as not converged with that value in the history.
 * The published breakdowns M_kk = 0 and tt = 0 arrive there through beta or omega
 * (no separate flag).  b = 0 with x0 = 0 stops at iteration 1, not converged (0/0);
 * A = I converges at iteration 1 with history entry 0.  The history is the
 * recurrence of the TRUE residual b - A x (right preconditioning), the quantity
 * bis_fgmres_* records.  M^-1 must be ONE fixed operator: the recurrences assume
 * G_k = A M^-1 (...) with the same M at every step.  Nothing checks this; an MG
 * K-cycle (BIS_MG_CYCLE_K, BIS_MG_CYCLE_K_GCR) is not such an operator (use
 * bis_fgmres_*).
 * The shadow space: P[i][j] = (h + 0.5) 2^-31 - 1 for row i, column j, with
 * h = hash32(hash32(i) ^ ((j + 1) 0x9e3779b9 mod 2^32)) and the hash32 of the MIS key
 * above: uniform in (-1, 1), exact in fp64, the same on every device and host, not
 * orthonormalised.  bis_idr_set_shadow replaces it by the caller's n x s matrix
 * P_host (HOST memory, column-major, leading dimension n); the call blocks and
 * copies, and is refused (BIS_ERR_INVALID) once bis_idr_init has run.
 * Schedule at a position k < s, beside the SpMV and the apply: the pass for v (with
 * U_k in the same pass where there is no preconditioner), the pass for U_k, the
 * multi-dot q with s accumulators per lane, whose last workgroup does the alpha / M /
 * beta / f lines in one lane, and the update of G_k, U_k, r and x with the partial
 * sums of (r, r) fused, whose last workgroup writes the history, does the stop test
 * and computes the next c.  Position s: one pass for (tt, tr), whose last workgroup
 * computes omega, and the update of x and r with (r, r) and f = P^T r fused.  All on
 * 16-byte accesses with a scalar path for an odd tail; every "vector -+ scalar *
 * vector" is one fma per element, sums over columns run over ascending column index,
 * the small algebra rounds every operation separately.  A position k < s moves
 * 3 s + 13 vectors, 24 s + 104 bytes per row whatever k is (200 at s = 4, against
 * 56 + 32 n of bis_fgmres_* at position n); position s moves s + 8.  4 s + 3 launches
 * per cycle without a preconditioner, 5 s + 3 and the applies' own with one.  The
 * reductions go by per-workgroup partial sums that the workgroup arriving last adds
 * in index order (no floating-point atomics, no waiting; the grid depends on n
 * only): two runs give the same bits.  Scalars, M, the history and the stop flag
 * stay on the device; bis_idr_iterate reads nothing back and knows the cycle
 * position from the number of iterations enqueued, which persists across calls.
 * After the stop every launch of the schedule returns at once, so no later call
 * changes x, the history or the status, and x is the iterate the last history entry
 * belongs to (launches of the preconditioner queued behind the stop may still run;
 * nothing reads their results).
 * Memory: (3 s + 3) n doubles (n rounded up to even: every column starts on 16 bytes
 * and is an SpMV operand), 96 doubles of state and the history, plus the
 * preconditioner's scratch (SGS, ILU0, FSAI: one n-vector; the two-stage types and
 * ILU0_ITER: two; MG, block Jacobi: the handle's own).
 * bis_idr_set_preconditioner takes the arguments of bis_fgmres_set_preconditioner:
 * every type, outer_iters and inner_iters that bis_apply_preconditioner takes for
 * one vector, BIS_PC_MG and BIS_PC_BLOCK_JACOBI (the operand in L_strict) included.
 * Call it before bis_idr_init.
 * Errors: null arguments, s outside 1 .. 8, a non-square A, b or x off a 16-byte
 * boundary, set_preconditioner or set_shadow after init, a missing operand, an MG
 * operand of another size: BIS_ERR_INVALID; MG with outer_iters != 1:
 * BIS_ERR_UNSUPPORTED; n = 0: BIS_OK, nothing is launched; *out is written on
 * success only. */
typedef struct bis_idr bis_idr;
BIS_API bis_status bis_idr_create(bis_ctx *ctx, const bis_mat *A, const double *b, double *x, int s, bis_idr **out);
BIS_API bis_status bis_idr_set_preconditioner(bis_ctx *ctx, bis_idr *h, int precond_type,
                                              const bis_mat *L_strict, const bis_mat *U_strict,
                                              const double *A_D, const double *A_D_inv,
                                              const double *L_D, const double *U_D,
                                              int outer_iters, int inner_iters);
/* blocking: P = P_host (n x s, column-major, leading dimension n); before bis_idr_init */
BIS_API bis_status bis_idr_set_shadow(bis_ctx *ctx, bis_idr *h, const double *P_host);
/* Reuse: bis_idr_init may be called again at any time, inside a cycle as well.  It reads b and x as they are at that
 * call and discards every earlier state: the position starts at 0 again, G and U are zero, M = I, omega = 1, the count,
 * the history and the flags are dropped, NaN included; P stays.  The solve that follows is, bit for bit, that of a new
 * handle.  bis_idr_set_preconditioner and bis_idr_set_shadow stay refused (BIS_ERR_INVALID) once bis_idr_init has run. */
/* blocking; r0_norm_host (may be NULL) receives ||b - A x0||_2 */
BIS_API bis_status bis_idr_init(bis_ctx *ctx, bis_idr *h, double tol, double *r0_norm_host);
/* non-blocking: enqueues n_iters iterations; the cycle position persists across calls */
BIS_API bis_status bis_idr_iterate(bis_ctx *ctx, bis_idr *h, int n_iters);
/* blocking: iterations, converged flag, history entries 0 .. iterations (at most hist_cap of them; may be NULL) */
BIS_API bis_status bis_idr_status(bis_ctx *ctx, bis_idr *h, int *iters, int *converged, double *hist_host,
                                  int hist_cap);
BIS_API bis_status bis_idr_destroy(bis_ctx *ctx, bis_idr *h);

/* ---- LSMR on the device (no reference counterpart) -----------------------------
 * LSMR (Fong and Saunders, 2011) for the least-squares problem
 *     min ||A x - b||_2^2 + lambda^2 ||x||_2^2
 * with A of size m x n and any of m > n, m < n, m = n: over-determined,
 * under-determined, inconsistent and rank-deficient systems, and Tikhonov-regularised
 * ones (lambda >= 0, default 0).  It is MINRES on the normal equations without forming
 * them: short recurrences, two m-vectors and four n-vectors at any iteration count, two
 * products per iteration -- bis_spmv with A and bis_spmv with At, the matrix
 * bis_mat_transpose makes (the caller passes it, or the handle makes and owns it).
 * Both products go through the SpMV's launcher: every SpMV form applies to both.
 * From x0 the iterates stay in x0 + range(At): with x0 = 0 and lambda = 0 the limit is
 * the minimum-norm solution.
 * Column scaling: with d (n entries, d > 0; bis_lsmr_set_col_scaling) the iteration
 * runs on A D, D = diag(d), in the variable y = D^-1 x, and DAMPING ACTS ON y: the
 * problem solved is min ||A D y - b||^2 + lambda^2 ||y||^2, x = D y.  With lambda = 0
 * that is the problem above (the same x when A has full column rank; the solution of
 * least ||D^-1 x|| otherwise).
 * init: u~ = b - A x0;  beta1 = sqrt((u~, u~));  ib = 1/beta1;
 *       p = (At u~) ib;  p = p d where a scaling is set;  alpha1 = sqrt((p, p));
 *       ia = 1/alpha1;  v = p ia;  h = v;  hbar = 0;
 *       zetabar = alpha1 beta1;  alphabar = alpha1;  rho = rhobar = cbar = 1;  sbar = 0;
 *       betadd = beta1;  betad = 0;  rhodold = 1;  tautildeold = thetatilde = zeta = 0;
 *       dsum = 0.
 * History entry 0 is zetabar in the column `ar` and beta1 in the column `r`.
 * Iteration k = 1, 2, ... (u~ = beta u is kept un-normalised):
 *     t_m = A w                        w = v, or w = d v (elementwise) with a scaling
 *     u~  = fma(-(alpha ib), u~, t_m);  beta = sqrt((u~, u~));  ib = 1/beta
 *     t_n = At u~
 *     p   = t_n ib;  p = p d with a scaling;  v~ = fma(-beta, v, p);
 *     alpha = sqrt((v~, v~));  ia = 1/alpha
 *     (chat, shat, alphahat) = rot(alphabar, lambda)
 *     rhoold = rho;  (c, s, rho) = rot(alphahat, beta);
 *     thetanew = s alpha;  alphabar = c alpha
 *     rhobarold = rhobar;  zetaold = zeta;  thetabar = sbar rho;
 *     (cbar, sbar, rhobar) = rot(cbar rho, thetanew);
 *     zeta = cbar zetabar;  zetabar = -sbar zetabar
 *     betaacute = chat betadd;  betacheck = -shat betadd;
 *     betahat = c betaacute;  betadd = -s betaacute
 *     thetatildeold = thetatilde;  (ctildeold, stildeold, rhotildeold) = rot(rhodold, thetabar);
 *     thetatilde = stildeold rhobar;  rhodold = ctildeold rhobar;
 *     betad = -stildeold betad + ctildeold betahat
 *     tautildeold = (zetaold - thetatildeold tautildeold) / rhotildeold
 *     taud = (zeta - thetatilde tautildeold) / rhodold
 *     dsum = dsum + betacheck^2
 *     ar[k] = |zetabar|;  r[k] = sqrt(dsum + (betad - taud)^2 + betadd^2);  stop test
 *     v = v~ ia
 *     hbar = fma(-thetabar rho / (rhoold rhobarold), hbar, h)
 *     x    = fma(zeta / (rho rhobar), hbar, x)      with a scaling: fma(..., d hbar, x)
 *     h    = fma(-thetanew / rho, h, v)
 *     w    = d v                                    with a scaling
 * rot(a, b): den = sqrt(a^2 + b^2), c = a/den, s = b/den; den = 0 gives c = 1, s = 0.
 * The next iteration's alpha ib is formed (one product) in the same place.  Every
 * scalar operation is rounded separately; a division whose divisor is 0 gives 0.
 * What the two history columns estimate, with Abar = A D (D = I without a scaling),
 * y = D^-1 x and rbar = [b - A x; -lambda y]:
 *     ar[k] ~ ||Abar^T (b - A x_k) - lambda^2 y_k||_2, the residual of the normal
 *             equations of the (scaled, damped) problem; it never increases;
 *     r[k]  ~ ||rbar_k|| = sqrt(||b - A x_k||^2 + lambda^2 ||y_k||^2).
 * So with a scaling ar measures the gradient in the scaled variable, D A^T r, not
 * A^T r, and with damping r is not ||b - A x|| but the norm of the stacked residual.
 * Both are recurrences, not explicit norms; entry 0 of each is explicit.
 * Stop: ar[k] < tol_ar ar[0] (reason 2), r[k] < tol_r r[0] (reason 1), or a non-finite
 * entry (reason 4, not converged).  A tolerance of 0 never fires.  r is tested before
 * ar, a non-finite entry and a breakdown before both.
 * Breakdown (reason 3, converged): beta = 0 or alpha = 0 in an iteration ends the
 * solve in that iteration with ar entry 0; the reciprocal of zero is never formed, 0
 * stands for it.  ar[0] = 0 -- x0 is a least-squares solution already (b = 0 with
 * x0 = 0 is one case) -- is the same breakdown at alpha1: bis_lsmr_init marks the
 * solve stopped and converged with 0 iterations, and x is never written.
 * Schedule per iteration: SpMV A, pass U (the u~ line with its sum fused, the last
 * workgroup forms beta and ib), SpMV At, pass V (the p and v~ lines with the sum
 * fused; v~ lives in t_n; the last workgroup's lane 0 does every scalar line, the
 * history and the stop test), pass H (v, hbar, x, h and w in one pass).  Beside the two
 * products that is 24 bytes per row of A and 88 per column (U 24; V 24; H 64), with a
 * scaling 24 + 112.  All on 16-byte accesses with a scalar path for an odd tail, on
 * the grids of the BLAS-1 layer.  The sums are bis_dot's: its grid, index map, two fma
 * chains per lane and its order of the block and partial sums, which the workgroup
 * that arrives last adds (no floating-point atomics, no waiting): two runs give the
 * same bits.  Scalars, history and the stop flag stay on the device; bis_lsmr_iterate
 * reads nothing back.  After the stop every launch returns at once except pass H of
 * the stopping iteration: x is the iterate of the last history entry at every step
 * (there is no pending combine), and no later call changes x, the histories or the
 * status.
 * Memory: u~ and t_m (m doubles each), v, h, hbar, t_n (n each), w with a scaling (m
 * and n rounded up to even), At when the handle made it, the two history columns.
 * There is no set_preconditioner: a left or right M^-1 on a rectangular problem is not
 * what bis_apply_preconditioner provides (its operators are square, of A's size); the
 * diagonal right scaling above is the one conditioning device, and bis_mat_row_norms of
 * At (the column norms of A) with bis_lsmr_scaling_from_norms gives the usual choice.
 * No tuning option.
 * Errors: a null context: BIS_ERR_NO_DEVICE, the out-parameters are left alone.  Null
 * arguments or a null handle, an At that is not n x m with A's number of entries, b,
 * x or d off a 16-byte boundary, lambda negative or not finite, a setter after
 * bis_lsmr_init, bis_lsmr_iterate before it: BIS_ERR_INVALID with a message naming the
 * call.  m = 0 or n = 0: BIS_OK, nothing is launched.  *out is written on success only. */
typedef struct bis_lsmr bis_lsmr;
/* At: A^T as bis_mat_transpose makes it, or NULL: the handle makes it and owns it */
BIS_API bis_status bis_lsmr_create(bis_ctx *ctx, const bis_mat *A, const bis_mat *At, const double *b /* m */,
                                   double *x /* n, in/out */, bis_lsmr **out);
/* before bis_lsmr_init; lambda >= 0 and finite */
BIS_API bis_status bis_lsmr_set_damping(bis_ctx *ctx, bis_lsmr *h, double lambda);
/* before bis_lsmr_init; d: n entries on the device, read at every iteration (the caller keeps it alive); NULL clears */
BIS_API bis_status bis_lsmr_set_col_scaling(bis_ctx *ctx, bis_lsmr *h, const double *d);
/* Reuse: bis_lsmr_init may be called again at any time (after a failed bis_lsmr_iterate it must be).  It reads b and x
 * as they are at that call and discards every earlier state: v, h, hbar, w, the scalars, the count, both history
 * columns and the flags, NaN included; damping, scaling and At stay.  The solve that follows is, bit for bit, that of
 * a new handle.  The setters stay refused (BIS_ERR_INVALID) once bis_lsmr_init has run. */
/* blocking; r0_host and ar0_host (each may be NULL) receive beta1 and zetabar = alpha1 beta1 */
BIS_API bis_status bis_lsmr_init(bis_ctx *ctx, bis_lsmr *h, double tol_r, double tol_ar, double *r0_host, double *ar0_host);
/* non-blocking: enqueues n_iters iterations */
BIS_API bis_status bis_lsmr_iterate(bis_ctx *ctx, bis_lsmr *h, int n_iters);
/* blocking: iterations, converged flag, reason (0 live, 1 tol_r, 2 tol_ar, 3 breakdown, 4 non-finite) and entries
 * 0 .. iterations of the two history columns (at most hist_cap of each; each pointer may be NULL) */
BIS_API bis_status bis_lsmr_status(bis_ctx *ctx, bis_lsmr *h, int *iters, int *converged, int *reason,
                                   double *hist_ar_host, double *hist_r_host, int hist_cap);
BIS_API bis_status bis_lsmr_destroy(bis_ctx *ctx, bis_lsmr *h);
/* out[i] = sqrt(sum_k a_ik^2) for the n_rows rows of A (out on the device): one fma chain per row over its entries in
 * CRS order, from 0; an empty row gives 0; no atomics.  The column norms of A are the row norms of its transpose.
 * Non-blocking. */
BIS_API bis_status bis_mat_row_norms(bis_ctx *ctx, const bis_mat *A, double *out);
/* d[i] = 1 / norms[i], and 1 where norms[i] is 0 (n entries, both on the device; d may be norms): the column scaling
 * that gives A D columns of norm 1.  Non-blocking. */
BIS_API bis_status bis_lsmr_scaling_from_norms(bis_ctx *ctx, const double *norms, int64_t n, double *d);

/* ---- thick-restart Lanczos eigensolver on the device (no reference counterpart) ----
 * The k extreme eigenpairs A x = lambda x of a symmetric matrix (symmetry is the
 * caller's promise, as for bis_minres_*): the smallest (BIS_EIGS_SA), the largest
 * (BIS_EIGS_LA) or the largest in magnitude (BIS_EIGS_LM), by thick-restart Lanczos (Wu
 * and Simon, 2000) with full re-orthogonalisation, as a device schedule: nothing is read
 * back inside bis_eigs_iterate.
 * Parameters: k wanted pairs; m = ncv the basis size, 1 <= k < m <= min(n, 64) (64 is
 * one wave: the restart runs in one); ncv = 0 asks for min(n, 64, max(2k + 1, 20));
 * tol the convergence tolerance.  OP is A, or whatever the caller applies between
 * bis_eigs_op_begin and bis_eigs_op_end (shift-and-invert: OP = (A - sigma I)^-1 by a
 * bis_minres_* solve, lambda = sigma + 1 / theta).
 * Storage: V_0 .. V_m, m + 1 basis blocks ld = n rounded up to even apart; the work
 * vector W; the small state alpha (m), beta (m) and, after a restart, theta (l) and
 * the coupling s (l).  Memory: (m + 2) n-vectors.
 * Start: V_0 = v0 / ||v0||, v0 the caller's vector (bis_eigs_set_start) or column 0 of
 * the hashed shadow space of bis_idr_*: v0[i] = (h + 0.5) 2^-31 - 1,
 * h = hash32(hash32(i) ^ 0x9e3779b9).  l = 0.  A zero or non-finite ||v0|| stops the
 * solve in bis_eigs_init, not converged, reason BAD_START.
 * Step j (l <= j < m), one product each:
 *     1. W = OP V_j
 *     2. h = V_{0..j}^T W
 *     3. W = W - V_{0..j} h        one fma per element and block, ascending block index
 *     4. c = V_{0..j}^T W
 *     5. W = W - V_{0..j} c        the same, with (W, W) in the same pass
 *     6. alpha_j = h_j + c_j ;  beta_j = sqrt((W, W))
 *     7. V_{j+1} = W / beta_j
 * Two classical Gram-Schmidt passes always: there is no data-dependent second pass.
 * Of h and c only alpha_j and beta_j are kept; the other entries are the known
 * structure (s at j = l, beta_{j-1} otherwise) up to rounding.
 * Breakdown: beta_j <= eps ||OP V_j||_2 (the norm is summed with the first group of
 * line 2) is an invariant subspace: beta_j is set to 0 and no reciprocal is formed.
 * The cycle closes with m_eff = j + 1 (the restart below on the leading m_eff rows and
 * columns), every estimate is 0 and the solve stops, reason INVARIANT: converged when
 * m_eff >= k, otherwise not converged with nconv = m_eff values.  The test is not
 * beta_j == 0: in floating point the two passes leave rounding noise of the order
 * eps^2 ||OP V_j|| of a beta_j that is 0 in exact arithmetic, its normalisation is a
 * unit vector inside the subspace that is not orthogonal to the basis, and the Ritz
 * values that follow are wrong (diag(1..6) from e_1 + e_2 returned -29 and -21 with
 * estimates below 1e-10).  A beta_j that is not 0 in exact arithmetic and yet below
 * eps ||OP V_j|| could not be told from that noise either.  With ncv = n the last
 * step of the first cycle always ends this way.
 * Restart, after step m - 1, in one wave:
 *     1. T (m x m): diag(theta_0 .. theta_{l-1}); row and column l hold s; from (l, l)
 *        on the tridiagonal of alpha_l .. alpha_{m-1} and beta_l .. beta_{m-2}.
 *     2. T = Y diag(theta) Y^T by cyclic Jacobi: sweeps over (p, q), p < q, in row
 *        order; tau = (t_qq - t_pp) / (2 t_pq); t = 1 / (tau + sign(tau) sqrt(1 + tau^2))
 *        with sign(0) = +1; c = 1 / sqrt(1 + t^2); s = t c; t_pp -= t t_pq;
 *        t_qq += t t_pq; rows and columns p, q of T and columns p, q of Y are rotated,
 *        (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q), in Rutishauser's form
 *        (x_p - s (x_q + rho x_p), x_q + s (x_p - rho x_q)), rho = s / (1 + c): the
 *        rounding errors are those of a correction, not of a product (Y^T Y - I stays
 *        at 5 eps where the plain form reaches 84 eps at m = 64); t_pq is set to 0
 *        exactly.  An entry that is 0 already is skipped.  Before each sweep off(T), the root of the
 *        sum of the squares of the off-diagonal entries themselves (never
 *        ||T||_F^2 - sum t_ii^2), is tested: off(T) <= eps ||T||_F ends the sweeps.
 *        30 sweeps without that stop the solve, not converged, reason JACOBI.
 *     3. theta sorted ascending (stable), then ranked: SA as sorted, LA descending, LM
 *        descending |theta| (stable on the sorted list).
 *     4. est_i = |beta_{m-1} Y[m-1, i]| for the first k in rank order; pair i has
 *        converged when est_i <= tol max(|theta_i|, eps^(2/3)) (ARPACK's test).
 *     5. History entry `restart`: max_{i<k} est_i, and in the second column how many of
 *        the k have converged.  All k: stop, converged (reason CONVERGED).
 *     6. Otherwise keep l = min(k + (m - k) / 2, m - 1) pairs in rank order (a constant
 *        of the handle): theta <- theta_keep, s_i = beta_{m-1} Y[m-1, keep_i], and
 *        V_{0..l) <- V_{0..m) Y_keep, V_l <- V_m, in place (a lane reads its row of
 *        all m blocks, then writes l blocks; one fma per block from 0, ascending).
 * The same compression, with the first k (min(k, m_eff)) ranked columns, runs at a
 * stop: after any restart the first basis blocks are the Ritz vectors in rank order,
 * which is what bis_eigs_vectors copies.
 * Single-vector Lanczos finds one vector per distinct eigenvalue: of a multiple
 * eigenvalue it returns one copy, the others appear late or never (block Lanczos is
 * not part of this handle).
 * Schedule per step: the product; per group of at most 8 basis blocks one multi-dot
 * launch (W read once per group); one update launch; the same again with (W, W) fused,
 * whose last workgroup's lane 0 does line 6; the scaling; then the one-wave Ritz launch
 * and the compression, which return at once unless the cycle closes or a breakdown was
 * met.  Beside the product that is four reads of the j + 1 basis blocks and
 * 2 ceil((j + 1) / 8) + 6 passes over W.  The vector passes walk 16 bytes per lane in
 * grid-stride loops on the grids of the BLAS-1 layer with one lane for an odd last
 * element (the compression: 8 bytes, a lane holds a row of up to 64 blocks).  No kernel
 * waits for another workgroup; partial sums are added in index order: two runs give
 * the same bits.  After a stop every launch returns at once.
 * Errors: a null context: BIS_ERR_NO_DEVICE, the out-parameters are left alone.  n < 2,
 * k < 1, ncv <= k, ncv > min(n, 64), a rectangular A, a null handle, bis_eigs_iterate on
 * a handle without a matrix, bis_eigs_op_end without bis_eigs_op_begin (or two begins),
 * bis_eigs_vectors before the first restart, bis_eigs_set_start after bis_eigs_init:
 * BIS_ERR_INVALID with a message naming the call and the argument. */
typedef struct bis_eigs bis_eigs;
enum { BIS_EIGS_SA = 0, BIS_EIGS_LA = 1, BIS_EIGS_LM = 2 };
/* the stop reasons of bis_eigs_status */
enum { BIS_EIGS_LIVE = 0, BIS_EIGS_CONVERGED = 1, BIS_EIGS_INVARIANT = 2, BIS_EIGS_JACOBI = 3, BIS_EIGS_BAD_START = 4 };
/* A: square, or NULL: the caller applies the operator (n is then the size; with A it must be A's); ncv = 0: the default */
BIS_API bis_status bis_eigs_create(bis_ctx *ctx, const bis_mat *A, int64_t n, int k, int ncv, int which, bis_eigs **out);
/* before bis_eigs_init; v0_dev: n entries on the device, read by bis_eigs_init (the caller keeps it alive); NULL: the default */
BIS_API bis_status bis_eigs_set_start(bis_ctx *ctx, bis_eigs *h, const double *v0_dev);
/* blocking.  It may be called again at any time: every earlier state (basis, scalars, counts, history, flags) is
 * discarded and the solve that follows is, bit for bit, that of a new handle. */
BIS_API bis_status bis_eigs_init(bis_ctx *ctx, bis_eigs *h, double tol);
/* non-blocking: enqueues n_cycles whole cycles (the first has m products, later ones m - l); BIS_ERR_INVALID on a handle
 * without a matrix.  It is a loop of bis_eigs_op_begin, bis_spmv, bis_eigs_op_end. */
BIS_API bis_status bis_eigs_iterate(bis_ctx *ctx, bis_eigs *h, int n_cycles);
/* One product of the caller's, on any handle: between the two calls the caller enqueues out = OP in on the context's
 * stream (n entries each; in is a basis block, out the work vector).  bis_eigs_op_end enqueues the rest of the step, and
 * the restart when the cycle closes.  Both non-blocking. */
BIS_API bis_status bis_eigs_op_begin(bis_ctx *ctx, bis_eigs *h, const double **in_dev, double **out_dev);
BIS_API bis_status bis_eigs_op_end(bis_ctx *ctx, bis_eigs *h);
/* blocking; every pointer may be NULL.  values_host and est_host (k entries each): the Ritz values and residual estimates
 * of the last restart in rank order; hist_host and hist_nconv_host: entries 0 .. restarts - 1 of the two history columns
 * (at most hist_cap of each). */
BIS_API bis_status bis_eigs_status(bis_ctx *ctx, bis_eigs *h, int *products, int *restarts, int *stopped, int *converged,
                                   int *reason, int *nconv, double *values_host, double *est_host, double *hist_host,
                                   double *hist_nconv_host, int hist_cap);
/* X_dev[i + ldx c] = Ritz vector c (c < k) in rank order: the first k basis blocks.  Valid after at least one restart,
 * refused before; at a live solve they are the kept vectors of the last restart. */
BIS_API bis_status bis_eigs_vectors(bis_ctx *ctx, bis_eigs *h, double *X_dev, int64_t ldx);
BIS_API bis_status bis_eigs_destroy(bis_ctx *ctx, bis_eigs *h);

/* ---- thick-restart Lanczos bidiagonalisation for singular triplets (no reference counterpart) ----
 * The k largest (BIS_SVDS_LM) or smallest (BIS_SVDS_SM) singular triplets
 * A v = sigma u, A^T u = sigma v of a rows x cols matrix of any shape, by Golub-Kahan-
 * Lanczos bidiagonalisation with thick restart (Baglama and Reichel 2005; Hernandez,
 * Roman and Tomas 2008) and full re-orthogonalisation of both bases, as a device
 * schedule: nothing is read back inside bis_svds_iterate.  It works on A and A^T
 * directly: A^T A is never formed (it would lose every sigma below sqrt(eps) sigma_max),
 * nor the augmented matrix (twice the vectors, every sigma twice).
 * Orientation: ns = min(rows, cols), nl = max(rows, cols).  The handle bidiagonalises
 * the tall orientation: F = A, F^T = A^T when rows >= cols, F = A^T, F^T = A otherwise,
 * so the start vector and the basis P live in the ns-dimensional space, where a
 * generic vector has no null-space component.  Of a triplet (sigma, q, p) of F, with q
 * of nl and p of ns entries, the caller gets u = q, v = p when rows >= cols and u = p,
 * v = q otherwise.  A^T is a bis_mat the caller passes (as bis_mat_transpose makes it)
 * or one the handle makes and owns; both products go through the SpMV launcher.
 * Parameters: k wanted triplets; m = ncv, 1 <= k < m <= min(ns, 64) (64 is one wave);
 * ncv = 0 asks for min(ns, 64, max(2k + 1, 20)); tol; ns >= 2.
 * Storage: P_0 .. P_m of ns entries and Q_0 .. Q_{m-1} of nl entries, each basis with
 * its own leading dimension (the length rounded up to even).  A product writes into
 * its destination block, which is orthogonalised and scaled in place: there is no
 * work vector.  Memory: (m + 1) ns + m nl doubles.  The small state: alpha (m), beta
 * (m), after a restart sigma (l) and the coupling s (l), and sigma_ref.
 * Start: P_0 = v0 / ||v0||, v0 the caller's vector of ns entries (bis_svds_set_start)
 * or column 0 of the hashed shadow space of bis_idr_* (the default of bis_eigs_*).
 * l = 0, sigma_ref = 0.  A zero or non-finite ||v0|| stops the solve in bis_svds_init,
 * not converged, reason BAD_START.
 * Step j (l <= j < m), two products:
 *   left half
 *     1. Q_j = F P_j
 *     2. twice, when j > 0:  h = Q_{0..j-1}^T Q_j;  Q_j = Q_j - Q_{0..j-1} h
 *     3. alpha_j = ||Q_j||_2 (summed in the second update's pass; with j = 0 in a pass
 *        of its own);  Q_j = Q_j / alpha_j
 *   right half
 *     4. P_{j+1} = F^T Q_j
 *     5. twice:  h = P_{0..j}^T P_{j+1};  P_{j+1} = P_{j+1} - P_{0..j} h
 *     6. beta_j = ||P_{j+1}||_2;  P_{j+1} = P_{j+1} / beta_j
 * Two classical Gram-Schmidt passes always, no data-dependent branch; one fma per
 * element and block in ascending block index.  The coefficients h are discarded: the
 * entries of B = Q^T F P are the two norms and the known structure (s in column l,
 * beta above the diagonal).
 * Breakdown.  beta_j <= eps ||F^T Q_j||_2 (the norm before the passes, summed with
 * the first group of dots): span(P_0..P_j) is an invariant subspace of F^T F;
 * beta_j is set to 0 and no reciprocal is formed; the cycle closes with m_eff = j + 1,
 * every estimate is 0 and the solve stops, reason INVARIANT: converged when m_eff >= k,
 * otherwise not converged with nconv = m_eff values.  With ncv = ns the first cycle
 * always ends this way.  alpha_j <= eps ||F P_j||_2: F maps span(P_0..P_j) into
 * span(Q_0..Q_{j-1}); alpha_j and beta_j are set to 0, Q_j counts as 0, m_eff = j + 1,
 * estimates 0, reason INVARIANT.  The singular value 0 that this exposes has a zero
 * vector on the long side (u when rows >= cols, v otherwise): only its short-side
 * vector, a null vector of F, means anything.  The test is "<= eps times the norm before
 * the passes", not "== 0", for the reason given with bis_eigs_*.
 * Restart, after step m - 1 or at a breakdown, in one wave:
 *     1. B (m_eff x m_eff): rows i < l hold sigma_i on the diagonal and s_i in column
 *        l; from (l, l) on alpha_i on the diagonal and beta_i at (i, i + 1).
 *     2. B = X Sigma Y^T by one-sided (Hestenes) Jacobi: G = B, Y = I; a rotation of
 *        the columns p < q of G and of Y makes g_p^T g_q = 0:
 *        a = g_p^T g_p, b = g_q^T g_q, c = g_p^T g_q, each summed in row order from 0,
 *        every operation rounded separately; the pair is skipped when c = 0, when
 *        |c| <= sqrt(m_eff) eps sqrt(a) sqrt(b), or when sqrt(a) or sqrt(b) is at most
 *        eps ||B||_F (||B||_F^2: the column sums in row order, added in column order):
 *        such a column is the rounding noise of a zero singular value, every rotation
 *        renews the noise, and a singular B (an alpha breakdown leaves its last row 0)
 *        would rotate for ever.  Otherwise zeta = (b - a) / (2 c),
 *        t = 1 / (zeta + sqrt(1 + zeta^2)) for zeta >= 0 and 1 / (zeta - sqrt(1 + zeta^2))
 *        otherwise, cs = 1 / sqrt(1 + t^2), sn = t cs,
 *        (x_p, x_q) <- (cs x_p - sn x_q, sn x_p + cs x_q).
 *        Order of the pairs: round-robin.  With n2 = m_eff rounded up to even, a sweep is
 *        n2 - 1 rounds r = 0 .. n2 - 2 of n2 / 2 disjoint pairs, one lane per pair:
 *        lane 0 holds {n2 - 1, r}, lane i > 0 holds {(r + i) mod (n2 - 1),
 *        (r - i) mod (n2 - 1)}; p is the smaller index; a pair with an index >= m_eff
 *        (the bye of an odd m_eff) does nothing.  A sweep without a rotation ends the
 *        iteration; 30 sweeps that all rotated stop the solve, not converged, reason
 *        JACOBI.  (With a threshold of eps alone a 30-sweep limit was met; with
 *        sqrt(m_eff) eps the restatement needs at most 11.)  Then
 *        sigma_i = ||g_i||_2, set to 0 when it is at most eps ||B||_F, and
 *        x_i = g_i / sigma_i; a zero column gives a zero x_i.
 *     3. sigma sorted ascending (stable), then ranked: SM as sorted, LM descending
 *        (stable on the sorted list).
 *     4. sigma_ref = the largest sigma of any restart so far, this one included: an
 *        estimate of ||A||_2 that SM, which discards the large values, keeps.
 *     5. est_i = |beta_{m_eff-1} X[m_eff-1, i]| for the first k in rank order; triplet
 *        i has converged when est_i <= tol sigma_ref: the backward error relative to
 *        ||A||_2 (a test relative to sigma_i cannot be met for small sigma_i).
 *     6. History entry `restart`: max_{i<k} est_i, and in the second column how many of
 *        the k have converged.  All k: stop, converged (reason CONVERGED).
 *     7. Otherwise keep l = min(k + (m - k) / 2, m - 1) triplets in rank order (a
 *        constant of the handle): sigma <- sigma_keep, s_i = beta_{m-1} X[m-1, keep_i],
 *        P_{0..l) <- P_{0..m) Y_keep, P_l <- P_m, Q_{0..l) <- Q_{0..m) X_keep, each
 *        basis once, in place, row by row (a lane reads its row of all m blocks, then
 *        writes l; one fma per block from 0, ascending).  The next cycle starts at
 *        j = l: F P_l is orthogonalised against the kept Q, which is where the s_i live.
 *     8. The same compression with the first min(k, m_eff) ranked columns runs at a
 *        stop: after any restart the leading blocks are the singular vectors in rank
 *        order, which is what bis_svds_vectors copies.
 * Products: 2m in the first cycle, 2(m - l) in later ones.
 * Schedule per half step: the product; per group of at most 8 basis blocks one
 * multi-dot launch (the new vector read once per group); one update launch; the same
 * again with the norm fused, whose last workgroup's lane 0 forms alpha_j or beta_j,
 * the product count and the breakdown test; the in-place scaling; then the one-wave
 * launch and the two compressions, which return at once unless the cycle closes or a
 * breakdown was met.  The vector passes walk 16 bytes per lane in grid-stride loops on
 * the grids of the BLAS-1 layer with one lane for an odd last element (the compression:
 * 8 bytes, a lane holds a row of up to 64 blocks).  Scalars, B's entries, histories and
 * flags stay on the device.  No kernel waits for another workgroup; partial sums are
 * added in index order: two runs give the same bits.  After a stop every launch returns
 * at once.
 * Limitation: SM uses plain, not harmonic, Ritz values.  It converges on
 * well-conditioned matrices and is slow on ill-conditioned ones (on a 1301 x 700 matrix
 * of condition 1.3e4 the restatement did not converge in 2000 restarts for SM, where
 * LM took 2); a harmonic restart is not part of this handle.  Of a multiple singular
 * value one copy is found, as with bis_eigs_*.
 * Errors: a null context: BIS_ERR_NO_DEVICE, the out-parameters are left alone.
 * k < 1, ncv <= k, ncv > min(ns, 64), ns < 2, an At whose shape is not that of A^T, a
 * null handle, bis_svds_iterate on a handle without a matrix, bis_svds_op_end without
 * bis_svds_op_begin (or two begins), bis_svds_vectors before the first restart,
 * bis_svds_set_start after bis_svds_init: BIS_ERR_INVALID with a message naming the
 * call and the argument. */
typedef struct bis_svds bis_svds;
enum { BIS_SVDS_LM = 0, BIS_SVDS_SM = 1 };
/* the stop reasons of bis_svds_status */
enum { BIS_SVDS_LIVE = 0, BIS_SVDS_CONVERGED = 1, BIS_SVDS_INVARIANT = 2, BIS_SVDS_JACOBI = 3, BIS_SVDS_BAD_START = 4 };
/* A: rows x cols, or NULL: the caller applies both products (rows and cols are then the shape; with A they must be A's).
 * At: A^T, or NULL: the handle makes it with bis_mat_transpose and owns it.  ncv = 0: the default */
BIS_API bis_status bis_svds_create(bis_ctx *ctx, const bis_mat *A, const bis_mat *At, int64_t rows, int64_t cols, int k, int ncv,
                                   int which, bis_svds **out);
/* before bis_svds_init; v0_dev: min(rows, cols) entries on the device, read by bis_svds_init (the caller keeps it alive);
 * NULL: the default */
BIS_API bis_status bis_svds_set_start(bis_ctx *ctx, bis_svds *h, const double *v0_dev);
/* blocking.  It may be called again at any time: every earlier state (bases, scalars, sigma_ref, counts, history, flags)
 * is discarded and the solve that follows is, bit for bit, that of a new handle. */
BIS_API bis_status bis_svds_init(bis_ctx *ctx, bis_svds *h, double tol);
/* non-blocking: enqueues n_cycles whole cycles; BIS_ERR_INVALID on a handle without a matrix.  It is a loop of
 * bis_svds_op_begin, bis_spmv (with A or At as *transposed says), bis_svds_op_end. */
BIS_API bis_status bis_svds_iterate(bis_ctx *ctx, bis_svds *h, int n_cycles);
/* One product of the caller's, on any handle: between the two calls the caller enqueues out = A in (*transposed = 0: in has
 * cols entries, out rows) or out = A^T in (*transposed = 1: in has rows entries, out cols) on the context's stream, in terms
 * of the caller's A, not of F.  in and out are basis blocks.  bis_svds_op_end enqueues the rest of the half step, and the
 * restart when the cycle closes.  Both non-blocking. */
BIS_API bis_status bis_svds_op_begin(bis_ctx *ctx, bis_svds *h, const double **in_dev, double **out_dev, int *transposed);
BIS_API bis_status bis_svds_op_end(bis_ctx *ctx, bis_svds *h);
/* blocking; every pointer may be NULL.  values_host and est_host (k entries each): the singular values and residual
 * estimates of the last restart in rank order; hist_host and hist_nconv_host: entries 0 .. restarts - 1 of the two history
 * columns (at most hist_cap of each). */
BIS_API bis_status bis_svds_status(bis_ctx *ctx, bis_svds *h, int *products, int *restarts, int *stopped, int *converged,
                                   int *reason, int *nconv, double *sigma_ref, double *values_host, double *est_host,
                                   double *hist_host, double *hist_nconv_host, int hist_cap);
/* U_dev[i + ldu c] = left vector c (rows entries), V_dev[i + ldv c] = right vector c (cols entries), c < k in rank order:
 * the leading blocks of the two bases.  Either pointer may be NULL.  Valid after at least one restart, refused before; at
 * a live solve they are the kept vectors of the last restart. */
BIS_API bis_status bis_svds_vectors(bis_ctx *ctx, bis_svds *h, double *U_dev, int64_t ldu, double *V_dev, int64_t ldv);
BIS_API bis_status bis_svds_destroy(bis_ctx *ctx, bis_svds *h);

/* ---- measurement ------------------------------------------------------------ */
/* HIP-event timing of the kernels launched on the context's stream.  While
 * enabled, each bis_spmv launch (and the SpMV inside bis_cg_iterate) is
 * bracketed by a hipEvent pair; bis_profile_read returns launches and the
 * summed duration in milliseconds and resets the counters (blocking). */
BIS_API bis_status bis_profile_enable(bis_ctx *ctx, int on);
/* ... and every bis_sptrsv / bis_bsptrsv call (all launches of the call, on the
 * context's stream): count and summed milliseconds since the last read.
 * bis_mat_sweep_kernel names the kernel the last sweep of that direction ran on
 * the triangle (static string; "" before the first sweep) -- the timer-tree
 * counterpart of the reference's LIKWID regions `sptrsv` / `backwards-sptrsv`
 * (kernels.hpp:56-58, :90-92). */
BIS_API bis_status bis_profile_read_sweeps(bis_ctx *ctx, int64_t *sweeps, double *sweep_ms);
BIS_API const char *bis_mat_sweep_kernel(const bis_mat *T, int backward);
/* bis_mat_spmv_kernel names the kernel and template instance the last bis_spmv
 * (fused = 0) or the last SpMV inside bis_cg_iterate (fused = 1) launched for A:
 * "spmv_rowblock_kernel U=4 PK=1 BR=1", "spmv_rowblock_vd_kernel",
 * "spmv_rowmajor_vd_kernel", "spmv_window_kernel", "spmv_wave_per_row_kernel",
 * "sellwin fmt=4", "win8 rows=2", "colslab K=6" (static string; "" before the
 * first call) -- which of the forced or fallen-back paths actually ran. */
BIS_API const char *bis_mat_spmv_kernel(const bis_mat *A, int fused);
BIS_API bis_status bis_profile_read(bis_ctx *ctx, int64_t *spmv_launches,
                                    double *spmv_ms);

/* ---- multi-GPU: 1-D row-block partition --------------
 * One process per GPU.  Rank g owns the contiguous global rows
 * [row_starts[g], row_starts[g+1]) of A and the matching slice of every
 * vector.  The reference has no counterpart (single process, OpenMP): this is
 * the layer that replaces its shared-memory loops across devices.  Only two
 * exchange shapes exist: the halo exchange of boundary x entries before an
 * SpMV and the sum all-reduce of 1-2 scalars after a dot / norm. */

/* Host-only planning step (needs no device; unit-tested on CPU).  Input: the
 * local rows in CRS with GLOBAL column indices.  Output: the sorted list of
 * distinct remote columns ("halo", grouped by owner rank because owners hold
 * contiguous row ranges), how many of them each peer owns (recv_counts
 * [n_ranks]), and interior[2] = the longest run [a,b) of local rows that
 * reference no remote column (the part of the SpMV that can overlap the
 * exchange).  halo_cols may be NULL to query n_halo only; halo_cap is its
 * capacity. */
BIS_API bis_status bis_halo_plan(int64_t n_local, const int64_t *row_ptr,
                                 const int32_t *col_global, int n_ranks,
                                 int rank, const int64_t *row_starts,
                                 int64_t *n_halo, int32_t *halo_cols,
                                 int64_t halo_cap, int64_t *recv_counts,
                                 int64_t *interior);

typedef struct bis_dist bis_dist;

/* Diagonal of a row block that still carries GLOBAL column indices (call it
 * before bis_dist_create renumbers them): D[r] = a(r, row_offset + r), the
 * last diagonal entry of a row wins (peel_diag_crs, utilities/LU_factors.hpp:
 * 827-869); D_inv (optional) = 1/D.  BIS_ERR_NO_DIAG / BIS_ERR_ZERO_DIAG with
 * the reference's SanityChecker texts.  This is what gives every rank the
 * Jacobi preconditioner of its rows (config 3: -cg -p j across GPUs). */
BIS_API bis_status bis_mat_diag(bis_ctx *ctx, const bis_mat *A_local,
                                int64_t row_offset, double *D, double *D_inv);
/* The square diagonal block of a row block (entries with row_offset <= col <
 * row_offset + n_rows, columns renumbered to local, order inside a row kept).
 * Triangular sweeps do not cross ranks (a sequential wavefront, SURVEY.md
 * section 8e): a row-partitioned solve preconditions with Gauss-Seidel /
 * SGS / ILU(0) of THIS block on every rank -- block-Jacobi of the sweeps, a
 * different preconditioner from the single-GPU one (its own parity target:
 * tests/dist_worker.py).  Feed it to bis_mat_split_strict / bis_mat_ilu0 and
 * hand the factors to bis_cg_set_preconditioner. */
BIS_API bis_status bis_mat_diag_block(bis_ctx *ctx, const bis_mat *A_local,
                                      int64_t row_offset, bis_mat **block);

/* Transport, provided by the launcher or by bis_dist_use_rccl.  Buffers are
 * DEVICE pointers; the operation must be ordered on `stream` (a hipStream_t).
 * Return 0 on success. */
typedef struct {
    void *user;
    /* in-place sum all-reduce of `count` doubles */
    int (*allreduce_sum)(void *user, void *stream, double *buf, int count);
    /* send send_counts[p] doubles to each peer p from sendbuf (packed in peer
     * order), receive recv_counts[p] doubles from each peer p into recvbuf
     * (packed in peer order) */
    int (*exchange)(void *user, void *stream, const double *sendbuf,
                    const int64_t *send_counts, double *recvbuf,
                    const int64_t *recv_counts, int n_ranks);
} bis_comm_ops;

/* Builds the distributed operator from the local rows (GLOBAL column
 * indices).  A_local is consumed: its columns are renumbered in place to
 * [0,n_local) for owned columns and n_local + k for the k-th halo column, and
 * the handle stays owned by the bis_dist. */
BIS_API bis_status bis_dist_create(bis_ctx *ctx, bis_mat *A_local, int rank,
                                   int n_ranks, const int64_t *row_starts,
                                   bis_dist **out);
BIS_API bis_status bis_dist_destroy(bis_ctx *ctx, bis_dist *d);
/* n_local rows / entries owned, n_ext = n_local + n_halo: every vector that
 * is an SpMV INPUT must be allocated with n_ext entries (the halo tail is
 * filled by the exchange). */
BIS_API bis_status bis_dist_vec_len(const bis_dist *d, int64_t *n_local,
                                    int64_t *n_ext);
/* What this rank needs: the halo columns (global indices, sorted) and the
 * per-owner counts.  The launcher routes each owner its sub-list once at
 * setup (any host-side all-to-all), then calls bis_dist_set_send_lists. */
BIS_API bis_status bis_dist_halo_info(const bis_dist *d, int64_t *n_halo,
                                      int32_t *halo_cols, int64_t halo_cap,
                                      int64_t *recv_counts);
/* What the peers need from this rank: send_counts[p] global column indices
 * per peer p, concatenated in peer order (all inside this rank's row range). */
BIS_API bis_status bis_dist_set_send_lists(bis_ctx *ctx, bis_dist *d,
                                           const int64_t *send_counts,
                                           const int32_t *send_cols_global);
BIS_API bis_status bis_dist_set_comm(bis_ctx *ctx, bis_dist *d,
                                     const bis_comm_ops *ops);
/* RCCL transport over xGMI (ncclSend/ncclRecv pairs for the halo, ncclAllReduce
 * for scalars).  unique_id is the 128-byte ncclUniqueId made by
 * bis_rccl_unique_id on rank 0 and broadcast by the launcher. */
BIS_API bis_status bis_rccl_unique_id(bis_ctx *ctx, void *out128);
BIS_API bis_status bis_dist_use_rccl(bis_ctx *ctx, bis_dist *d,
                                     const void *unique_id128);
/* What the partition costs this rank: halo entries received and boundary
 * entries sent per SpMV (8 bytes each), rows of the interior run that overlaps
 * the exchange, the number of peers it talks to, and the size of the RCCL
 * communicator it joined (ncclCommCount; 0 when the transport is not RCCL). */
BIS_API bis_status bis_dist_stats(const bis_dist *d, int64_t *n_halo,
                                  int64_t *n_send, int64_t *interior_rows,
                                  int *n_neighbours, int *rccl_ranks);
/* bis_mat_spmv_stream_info of this rank's interior rows (the launch that
 * overlaps the halo exchange): which SpMV kernel the partitioned path runs. */
BIS_API bis_status bis_dist_spmv_stream_info(bis_ctx *ctx, const bis_dist *d,
                                             int *col_bytes, int *val_bytes,
                                             int *n_dict, int *form);
/* bis_mat_spmv_streamed_bytes of this rank's distributed SpMV: the stream formats
 * of its three row ranges (boundary, interior, boundary), x = [owned | halo] and
 * y once. */
BIS_API bis_status bis_dist_spmv_streamed_bytes(bis_ctx *ctx, const bis_dist *d,
                                                int64_t *bytes);
/* While bis_profile_enable is on, every halo exchange (on the communication
 * stream) and every scalar all-reduce (on the compute stream) is bracketed by
 * HIP events; returns counts and summed milliseconds and resets (blocking). */
BIS_API bis_status bis_dist_profile_read(bis_ctx *ctx, bis_dist *d,
                                         int64_t *n_exchange, double *exchange_ms,
                                         int64_t *n_allreduce, double *allreduce_ms);
/* y_local = (A x)_local.  x_ext has n_ext entries (owned part filled by the
 * caller); the halo exchange runs on a second stream under the interior rows'
 * SpMV, the boundary rows follow. */
BIS_API bis_status bis_dist_spmv(bis_ctx *ctx, bis_dist *d, double *x_ext,
                                 double *y_local);
/* global dot: local reduction + all-reduce; result_dev (device) always,
 * result_host if non-NULL (blocking). */
BIS_API bis_status bis_dist_dot(bis_ctx *ctx, bis_dist *d, const double *a,
                                const double *b, double *result_dev,
                                double *result_host);
/* Fused CG on the distributed operator: same schedule and handle as bis_cg_*
 * (bis_cg_init / bis_cg_iterate / bis_cg_status / bis_cg_destroy), with the
 * (Ap,p) all-reduce and the batched {(r,z),(r,r)} all-reduce per iteration.
 * b, x, A_D are local slices (n_local entries). */
BIS_API bis_status bis_dist_cg_create(bis_ctx *ctx, bis_dist *d,
                                      const double *A_D, const double *b,
                                      double *x, bis_cg **out);

#ifdef __cplusplus
}
#endif
#endif /* BIS_HIP_H */
