// common.hpp -- host-side common definitions of the MI355X build: the enums,
// CLI argument block, compile-time configuration and timer tree that the
// reference keeps in common.hpp (:38-111, :206-354), plus the glue to the
// C-ABI device library (include/bis_hip.h).  Vectors handled by this layer are
// DEVICE pointers obtained from dalloc(); nothing here computes on the CPU.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <sys/time.h>
#include <vector>

#include "bis_hip.h"

// Compile-time configuration: same names and defaults as the reference's
// CMake cache (CMakeLists.txt:19-29).
#ifndef MAX_ITERS
#define MAX_ITERS 1000
#endif
#ifndef TOL
#define TOL 1e-14
#endif
#ifndef RES_CHECK_LEN
#define RES_CHECK_LEN 1
#endif
#ifndef PRECOND_OUTER_ITERS
#define PRECOND_OUTER_ITERS 1
#endif
#ifndef PRECOND_INNER_ITERS
#define PRECOND_INNER_ITERS 0
#endif
#ifndef INIT_X_VAL
#define INIT_X_VAL 0.1
#endif
#ifndef B_VAL
#define B_VAL 1.0
#endif
#ifndef ILU0_PIVOT_TOLERANCE
#define ILU0_PIVOT_TOLERANCE 1e-8
#endif
#ifndef ILU0_PIVOT_REPLACEMENT
#define ILU0_PIVOT_REPLACEMENT 1e-4
#endif

using Interface = void *; // the SMAX seam of the reference (common.hpp:18-24) is the C ABI here
#define SMAX_ARGS(...)

enum class PrecondType { // ordinals == BIS_PC_* == reference common.hpp:38-47; ILU0Iter (8), FSAI (9), MG (10) and BlockJacobi (11) are this build's additions
    None, Jacobi, GaussSeidel, BackwardsGaussSeidel, SymmetricGaussSeidel, TwoStageGS,
    SymmetricTwoStageGS, ILU0, ILU0Iter, FSAI, MG, BlockJacobi
};

// -inner K: inner sweeps of the two-stage Gauss-Seidel types and of -p ilu0it, at run time; the default is the
// compile-time PRECOND_INNER_ITERS, so a command line without the flag runs what it always ran
inline int &precond_inner_iters() { static int k = PRECOND_INNER_ITERS; return k; }
// -pprec 32|64: the values of the factors that -p fsai and -p ilu0it apply by SpMV are rounded to fp32 after the
// factorisation (bis_mat_round_f32); 64, the default, leaves them as they are
inline int &precond_value_bits() { static int b = 64; return b; }
// -mg nu=1,cs=4,limit=256,levels=10,scale=1,omega=0,coarsening=auto|grid|mis: the parameters of -p mg (bis_mg_params; these are its defaults)
inline bis_mg_params &precond_mg_params() { static bis_mg_params p = {10, 256, 0, 1, 4, 0.0, 1.0}; return p; }
// -mg cycle=v|w|k|kgcr,klev=N: the cycle of -p mg and the number of transitions it covers (bis_mg_set_cycle; 0: all but the last)
struct MGCycle { int cycle = BIS_MG_CYCLE_V, levels = 0; };
inline MGCycle &precond_mg_cycle() { static MGCycle c; return c; }
// -mg smooth=1[,pomega=X]: smoothed aggregation (bis_mg_create_smoothed) with the prolongator's factor X in (0, 2); 0: the library's 4/3
struct MGSmooth { bool smooth = false; double pomega = 0.0; };
inline MGSmooth &precond_mg_smooth() { static MGSmooth s; return s; }
// -mg smoother=jacobi|cheb[,degree=N,ratio=X,est=S,safety=X]: the smoother of -p mg (bis_mg_set_smoother); ratio 4 is the
// default the CPU table of docs/EXPERIMENTS.md chose; without smoother=cheb nothing is called
inline bis_mg_smoother &precond_mg_smoother() { static bis_mg_smoother s = {BIS_MG_SMOOTH_JACOBI, 2, 4.0, 10, 1.1}; return s; }
// -bs N: rows per block of -p bj (bis_bj_params.block_size); 0: not given, the dof of the matrix' grid hint where that is above 1
inline int &precond_block_size() { static int b = 0; return b; }
// -fill K: level-of-fill of -p ilu0 / -p ilu0it (bis_mat_iluk); 0, the default, is ILU(0) as it always ran
inline int &precond_fill_level() { static int k = 0; return k; }
// -ids S: the dimension s of the shadow space of -idr (bis_idr_create), 1..8
inline int &idr_shadow_dim() { static int s = 4; return s; }
// -eig K [-which sa|la|lm] [-ncv M]: the wanted pairs, the end of the spectrum (BIS_EIGS_SA / _LA / _LM) and the basis size
// (0: the handle's default, filled in once the handle is made) of bis_eigs_create
inline int &eigs_k() { static int k = 0; return k; }
inline int &eigs_which() { static int w = 0; return w; }
inline int &eigs_ncv() { static int m = 0; return m; }
// -svd K [-which lm|sm] [-ncv M]: the wanted triplets, the end of the spectrum (BIS_SVDS_LM / _SM) and the basis size (0: the
// handle's default, filled in once the handle is made) of bis_svds_create
inline int &svds_k() { static int k = 0; return k; }
inline int &svds_which() { static int w = 0; return w; }
inline int &svds_ncv() { static int m = 0; return m; }
enum class SolverType { Jacobi, GaussSeidel, SymmetricGaussSeidel, GMRES, ConjugateGradient, BiCGSTAB, FGMRES, MINRES, IDR, LSMR, Eigs, SVDS }; // FGMRES, MINRES, IDR, LSMR, Eigs, SVDS: this build's additions (-fgm, -mr, -idr, -lsmr, -eig K, -svd K)

inline std::string to_string(PrecondType t) {
    static const char *n[] = {"none", "jacobi", "gauss-seidel", "backwards-gauss-seidel",
                              "symmetric-gauss-seidel", "two-stage gauss-seidel",
                              "symmetric two-stage gauss-seidel", "incomplete LU(0)"};
    if (t == PrecondType::ILU0Iter)
        return "incomplete LU(" + std::to_string(precond_fill_level()) + "), iterative solves (" + std::to_string(precond_inner_iters()) + ")";
    if (t == PrecondType::ILU0 && precond_fill_level() > 0) return "incomplete LU(" + std::to_string(precond_fill_level()) + ")";
    if (t == PrecondType::FSAI) return "factorized sparse approximate inverse";
    if (t == PrecondType::MG) return "aggregation multigrid";
    if (t == PrecondType::BlockJacobi) return "block jacobi";
    return n[static_cast<int>(t)];
}
inline std::string to_string(SolverType t) {
    static const char *n[] = {"jacobi", "gauss-seidel", "symmetric-gauss-seidel", "gmres",
                              "conjugate-gradient", "bicgstab", "fgmres", "minres"};
    if (t == SolverType::IDR) return "idr(" + std::to_string(idr_shadow_dim()) + ")";
    if (t == SolverType::LSMR) return "lsmr";
    if (t == SolverType::Eigs) {
        static const char *w[] = {"sa", "la", "lm"};
        return "lanczos(" + std::to_string(eigs_k()) + ", ncv=" + std::to_string(eigs_ncv()) + ", " + w[eigs_which()] + ")";
    }
    if (t == SolverType::SVDS) {
        static const char *w[] = {"lm", "sm"};
        return "lanczos-svd(" + std::to_string(svds_k()) + ", ncv=" + std::to_string(svds_ncv()) + ", " + w[svds_which()] + ")";
    }
    return n[static_cast<int>(t)];
}

struct Args {
    std::string matrix_file_name{};
    SolverType method{};
    PrecondType preconditioner{};
    int restart_length = 10;
    int inner_iters = PRECOND_INNER_ITERS; // -inner K (precond_inner_iters())
    int pprec = 64;                        // -pprec 32|64 (precond_value_bits())
    int fill_level = 0;                    // -fill K (precond_fill_level())
    bool fill_given = false;
    bool ids_given = false;                // -ids S (idr_shadow_dim())
    double damp = 0.0;                     // -damp L: the Tikhonov parameter of -lsmr (bis_lsmr_set_damping)
    bool damp_given = false;
    bool colscale = false;                 // -colscale: -lsmr runs on A D, d = 1 / the column norms of A (bis_lsmr_set_col_scaling)
    bool precond_given = false, perm_given = false; // -p, -perm appeared (refused with -lsmr and -eig)
    bool which_given = false, ncv_given = false, scale_given = false; // -which, -ncv (options of -eig and -svd), -scale appeared
    bool num_scale = false;
    bool unfused = false; // -unfused: CG / Jacobi / GS / SGS run the reference's kernel-by-kernel schedule (blocking reductions) instead of the device schedules
    bool host_scalars = false; // -hostscalars: GMRES / BiCGSTAB return every dot product to the host like the reference
                               // (default: Gram-Schmidt coefficients, alpha / omega / beta stay on the device)
    std::string perm_mode = "none"; // -perm mc: multi-colour reordering (SMAX PERM_MODE role)
    std::string dump_perm;          // -dump-perm FILE: write perm[new]=old
    std::string dump_x;             // -dump-x FILE: write x* (natural row order, also after -perm)
    std::string crs_cache;          // -cache FILE: binary CRS next to a .mtx input (read if present, else written)
    bool perm_host = false;         // -perm-host: colour and permute on the host (fallback path)
    int trsv_mode = -1;             // -trsv tiled|level|chain|wave: natural-order sweeps with the tiled kernel also where its plan is built on the host / never (default: tiled where the matrix has a grid hint)
    long long grid_hint[4] = {0, 0, 0, 0}; // -grid NX,NY,NZ[,DOF]: a matrix read from a file is a stencil on this grid, x fastest (bis_mat_set_grid_hint)
    int device = 0;
};

// ---- device glue ---------------------------------------------------------------
namespace bis {
inline bis_ctx *&ctx_slot() { static bis_ctx *c = nullptr; return c; }
inline bis_ctx *ctx() {
    if (!ctx_slot()) {
        fprintf(stderr, "ERROR: no device context (bis::init not called)\n");
        exit(EXIT_FAILURE);
    }
    return ctx_slot();
}
// the reference's kernels are void and exit on fatal conditions
// (common.hpp:382-396); restore that convention on top of bis_status
inline void check(bis_status st, const char *what) {
    if (st != BIS_OK) {
        fprintf(stderr, "ERROR: %s: %s (status %d)\n", what, bis_last_error(ctx_slot()), st);
        exit(EXIT_FAILURE);
    }
}
inline void init(int device) {
    bis_status st = bis_ctx_create(device, nullptr, &ctx_slot());
    if (st != BIS_OK) {
        fprintf(stderr, "ERROR: no usable gfx950 device (status %d); this build has no CPU path\n", st);
        exit(EXIT_FAILURE);
    }
}
inline void shutdown() { if (ctx_slot()) { bis_ctx_destroy(ctx_slot()); ctx_slot() = nullptr; } }
inline bool timers_sync() { static int v = getenv("BIS_TIMERS_SYNC") ? atoi(getenv("BIS_TIMERS_SYNC")) : 1; return v != 0; }
} // namespace bis

inline double *dalloc(long n) { double *p = nullptr; bis::check(bis_vec_alloc(bis::ctx(), n, &p), "bis_vec_alloc"); return p; }
inline void dfree(double *p) { if (p) bis_vec_free(bis::ctx(), p); }
inline void to_device(double *dst, const double *src, long n) { bis::check(bis_vec_upload(bis::ctx(), dst, src, n), "bis_vec_upload"); }
inline void to_host(double *dst, const double *src, long n) { bis::check(bis_vec_download(bis::ctx(), dst, src, n), "bis_vec_download"); }

// ---- timers (reference common.hpp:206-354, utilities.hpp:110-152) -----------------
class Stopwatch {
    long double wtime = 0;
    timeval begin{}, end{};
  public:
    void start() { gettimeofday(&begin, 0); }
    void stop() {
        // kernels are asynchronous: drain the stream so the timer tree means
        // what it means in the reference (BIS_TIMERS_SYNC=0 turns this off)
        if (bis::timers_sync() && bis::ctx_slot()) bis_sync(bis::ctx_slot());
        gettimeofday(&end, 0);
        wtime += (end.tv_sec - begin.tv_sec) + (end.tv_usec - begin.tv_usec) * 1e-6;
    }
    long double check() {
        gettimeofday(&end, 0);
        return (end.tv_sec - begin.tv_sec) + (end.tv_usec - begin.tv_usec) * 1e-6;
    }
    long double get_wtime() const { return wtime; }
};

struct Timers {
    std::map<std::string, Stopwatch> t;
    Stopwatch &operator[](const std::string &k) { return t[k]; }
    Stopwatch *per_iteration_time = &t["per_iteration"];
};

#define TIME(timers, name, routine)                                                                \
    do {                                                                                           \
        Stopwatch &sw_ = (*(timers))[name];                                                        \
        sw_.start();                                                                               \
        routine;                                                                                   \
        sw_.stop();                                                                                \
    } while (0);

#ifdef DEBUG_MODE
#define IF_DEBUG_MODE(s) s;
#else
#define IF_DEBUG_MODE(s)
#endif

struct SanityChecker { // reference common.hpp:388-396
    static void zero_diag(int row) { fprintf(stderr, "Zero detected on diagonal at row index %d\n", row); exit(EXIT_FAILURE); }
    static void no_diag(int row) { fprintf(stderr, "No diagonal to extract at row index %d\n", row); exit(EXIT_FAILURE); }
};
