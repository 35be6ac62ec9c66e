// bis_minres.hip -- preconditioned MINRES (Paige-Saunders) for symmetric, possibly indefinite A and a fixed symmetric
// positive definite M, on one right-hand side, as a sync-free device schedule of the kind bis_cg.hip is: one SpMV, one
// preconditioner apply and two global reductions per iteration, seven n-vectors at any iteration count.
//   init:  r2 = b - A x ; y = M^-1 r2 (none: y IS r2) ; beta1 = sqrt((r2, y)) ; hist[0] = beta1 ; threshold = tol beta1 ;
//          v = y (1 / beta1) ; w1 = w2 = 0 ; oldb = 0, beta = beta1, dbar = epsln = 0, phibar = beta1, cs = -1, sn = 0
//   iteration k = 1, 2, ...:
//     SpMV    t = A v                                                   bis_spmv_launch (returns at once after the stop)
//     pass B  t -= (beta / oldb) r1  (k >= 2) ; (v, t)                  the last workgroup: alpha, alpha / beta
//     pass C  t -= (alpha / beta) r2 ; r1 <- r2 ; r2 <- t ; y = M^-1 r2 ; (r2, y)
//               none:    y IS r2, the sum is (t, t), fused
//               Jacobi:  y = t / (1.0 D) and (t, y) fused                (outer_iters = 1, D on a 16-byte boundary)
//               others:  bis_apply_preconditioner, then the dot as one more pass
//             the last workgroup's lane 0: oldb = beta ; beta = sqrt((r2, y)) ; oldeps = epsln ;
//               delta = cs dbar + sn alpha ; gbar = sn dbar - cs alpha ; epsln = sn beta ; dbar = -cs beta ;
//               gamma = sqrt(gbar^2 + beta^2) ; cs = gbar / gamma ; sn = beta / gamma ; phi = cs phibar ; phibar = sn phibar ;
//               hist[k] = phibar ; stop if phibar < threshold (converged) or phibar is not finite (not converged)
//     pass D  w = (v - oldeps w1 - delta w2) (1 / gamma) ; x += phi w ; w1 <- w2 ; w2 <- w ; v = y (1 / beta)
// Rounding.  Every "vector -= scalar * vector" and "x += phi w" is ONE fma per element (the product is not rounded); the
// scalar factor is formed first and rounded: beta / oldb, alpha / beta, 1 / gamma, 1 / beta are each one division.  The
// scalings by 1 / gamma and 1 / beta are separate multiplications.  The fused dots are bis_dot's: the same grid and index
// map, two fma chains per lane (the two halves of its 16 bytes), the same block and partial sums -- so with the scalar
// algebra of the last lane, which rounds every operation separately (no contraction), the schedule gives the bits of the
// same iteration made of bis_spmv, bis_dot, bis_subtract_vectors / bis_sum_vectors, bis_scale and bis_apply_preconditioner.
// r1 <- r2 <- t and w1 <- w2 <- w are rotations of two sets of three buffers by the enqueue index, never copies.  With a
// preconditioner y is written into the buffer r1 leaves in pass B, and the next SpMV writes the buffer y leaves in pass D.
// Traffic per row and iteration beside the SpMV and the apply: pass B reads t, r1, v and writes t (32 B; 24 B at k = 1),
// pass C reads t, r2 and writes t (24 B), pass D reads v, w1, w2, x, y and writes w, x, v (64 B): 120 bytes.  Jacobi: +16
// (D read, y written).  Other types: +16 for the dot pass (r2, y read), beside the apply's own traffic.
// Memory: v, three r buffers, three w buffers = 7 n doubles (n rounded up to even), the history (65536 doubles), plus the
// preconditioner's scratch (SGS, ILU0, FSAI: one n-vector; the two-stage types and ILU0_ITER: two; MG: the hierarchy's own).
// The reductions are bis_internal.hpp's: per-workgroup partial sums, the workgroup that arrives last adds them in index
// order.  No kernel waits for another workgroup; no floating-point atomics; two runs give the same bits.  After the stop
// every launch of the schedule returns at once, except pass D of the stopping iteration: x is the iterate the last history
// entry belongs to.  (Launches of a preconditioner queued behind the stop may still run; nothing reads their results.)
#include "bis_solver.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

struct bis_minres : bis_solver_core { // flags: [0] iterations, [1] stopped, [2] converged, [3] the iteration of the stop
    const bis_mat *A = nullptr;
    const double *b = nullptr;
    double *x = nullptr;
    int64_t n = 0, ld = 0;  // ld: n rounded up to even
    double *v = nullptr;
    double *R[3] = {nullptr, nullptr, nullptr}; // r1, r2 and the SpMV's output / y, rotating
    double *W[3] = {nullptr, nullptr, nullptr}; // w1, w2, w, rotating
    double *sc = nullptr;   // device scalars (S_*)
    // counters: two last-arriver counter sets: pass B, pass C
};

namespace {

constexpr int kT = kSolverT;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxDotBlocks); // passes B and C run on bis_pair_grid(n, kMaxDotBlocks)

enum { S_BETA = 0, S_BOB /* beta / oldb */, S_ALPHA, S_AOB /* alpha / beta */, S_DBAR, S_EPSLN, S_PHIBAR, S_CS, S_SN, S_STOP,
       S_OLDEPS, S_DELTA, S_IGAMMA, S_PHI, S_IBETA, S_COUNT = 16 };
enum { C_NONE = 0, C_JACOBI, C_UPDATE_ONLY, C_DOT_ONLY };

// the scalar algebra of one iteration after (r2, y) is known: one lane
__device__ void mr_book(double rzy, double *sc, int *flags, double *hist, int hist_cap) {
#pragma clang fp contract(off)
    const double alpha = sc[S_ALPHA], oldb = sc[S_BETA], cs = sc[S_CS], sn = sc[S_SN], dbar = sc[S_DBAR];
    const double beta = sqrt(rzy); // (r2, y) < 0: M is not positive definite, NaN, the solve stops below
    const double oldeps = sc[S_EPSLN];
    const double delta = cs * dbar + sn * alpha;
    const double gbar = sn * dbar - cs * alpha;
    const double gamma = sqrt(gbar * gbar + beta * beta);
    const double cs_new = gbar / gamma, sn_new = beta / gamma;
    const double phi = cs_new * sc[S_PHIBAR], phibar = sn_new * sc[S_PHIBAR];
    sc[S_BETA] = beta;
    sc[S_BOB] = beta / oldb;
    sc[S_EPSLN] = sn * beta;
    sc[S_DBAR] = -cs * beta;
    sc[S_CS] = cs_new;
    sc[S_SN] = sn_new;
    sc[S_PHIBAR] = phibar;
    sc[S_OLDEPS] = oldeps;
    sc[S_DELTA] = delta;
    sc[S_IGAMMA] = 1.0 / gamma;
    sc[S_PHI] = phi;
    sc[S_IBETA] = 1.0 / beta;
    const int it = flags[0] + 1;
    flags[0] = it;
    if (it < hist_cap) hist[it] = phibar;
    const bool conv = phibar < sc[S_STOP];
    const bool not_finite = fabs(phibar) > DBL_MAX || phibar != phibar;
    if (conv || not_finite) { flags[1] = 1; flags[2] = conv && !not_finite ? 1 : 0; flags[3] = it; } // pass D of iteration `it` still runs
}

// pass B: t -= (beta / oldb) r1 (not at k = 1: r1 is not read), (v, t); the last workgroup: alpha and alpha / beta
__global__ __launch_bounds__(kT) void mr_b_kernel(int64_t n, int has_r1, double *sc, const int *flags,
                                                  double *__restrict__ t, const double *__restrict__ r1,
                                                  const double *__restrict__ v, double *partials, unsigned *counter) {
    __shared__ double lds[kT / 64];
    if (flags[1]) return;
    const double c = has_r1 ? sc[S_BOB] : 0.0;
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *t2 = reinterpret_cast<double2 *>(t);
    const double2 *r1v = reinterpret_cast<const double2 *>(r1);
    const double2 *v2 = reinterpret_cast<const double2 *>(v);
    double acc0 = 0.0, acc1 = 0.0; // bis_dot's two chains per lane
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 tv = t2[i];
        if (has_r1) {
            const double2 rv = r1v[i];
            tv.x = fma(-c, rv.x, tv.x);
            tv.y = fma(-c, rv.y, tv.y);
            t2[i] = tv;
        }
        const double2 vv = v2[i];
        acc0 = fma(vv.x, tv.x, acc0);
        acc1 = fma(vv.y, tv.y, acc1);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double tv = t[n - 1];
        if (has_r1) {
            tv = fma(-c, r1[n - 1], tv);
            t[n - 1] = tv;
        }
        acc0 = fma(v[n - 1], tv, acc0);
    }
    const double acc[1] = {acc0 + acc1};
    double total[1];
    if (!reduce_last<1>(acc, lds, partials, counter, total)) return;
    if (threadIdx.x != 0) return;
    sc[S_ALPHA] = total[0];
    sc[S_AOB] = total[0] / sc[S_BETA];
}

// pass C.  C_NONE: t -= (alpha / beta) r2, (t, t).  C_JACOBI: the same, y = t / (1.0 D), (t, y).  C_UPDATE_ONLY: the update
// alone (the apply and C_DOT_ONLY follow).  C_DOT_ONLY: (t, y).  Every mode with a sum ends in the bookkeeping.
template <int MODE>
__global__ __launch_bounds__(kT) void mr_c_kernel(int64_t n, double *sc, int *flags, double *__restrict__ t,
                                                  const double *__restrict__ r2, const double *__restrict__ D,
                                                  double *__restrict__ y, double *partials, unsigned *counter, double *hist,
                                                  int hist_cap) {
    __shared__ double lds[kT / 64];
    if (flags[1]) return;
    const double c = MODE == C_DOT_ONLY ? 0.0 : sc[S_AOB];
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *t2 = reinterpret_cast<double2 *>(t);
    const double2 *q2 = reinterpret_cast<const double2 *>(r2);
    const double2 *D2 = reinterpret_cast<const double2 *>(D);
    double2 *y2 = reinterpret_cast<double2 *>(y);
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 tv = t2[i];
        if (MODE != C_DOT_ONLY) {
            const double2 rv = q2[i];
            tv.x = fma(-c, rv.x, tv.x);
            tv.y = fma(-c, rv.y, tv.y);
            t2[i] = tv;
        }
        if (MODE == C_UPDATE_ONLY) continue;
        double2 yv = tv;
        if (MODE == C_JACOBI) {
            const double2 dv = D2[i];
            yv.x = tv.x / (1.0 * dv.x); // bis_elemwise_div_vectors' arithmetic
            yv.y = tv.y / (1.0 * dv.y);
            y2[i] = yv;
        } else if (MODE == C_DOT_ONLY) {
            yv = y2[i];
        }
        acc0 = fma(tv.x, yv.x, acc0);
        acc1 = fma(tv.y, yv.y, acc1);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double tv = t[n - 1];
        if (MODE != C_DOT_ONLY) {
            tv = fma(-c, r2[n - 1], tv);
            t[n - 1] = tv;
        }
        if (MODE != C_UPDATE_ONLY) {
            double yv = tv;
            if (MODE == C_JACOBI) { yv = tv / (1.0 * D[n - 1]); y[n - 1] = yv; }
            else if (MODE == C_DOT_ONLY) yv = y[n - 1];
            acc0 = fma(tv, yv, acc0);
        }
    }
    if (MODE == C_UPDATE_ONLY) return;
    const double acc[1] = {acc0 + acc1};
    double total[1];
    if (!reduce_last<1>(acc, lds, partials, counter, total)) return;
    // every other workgroup has read its scalars and the stop flag before it arrived: they may change now
    if (threadIdx.x == 0) mr_book(total[0], sc, flags, hist, hist_cap);
}

// pass D: w = (v - oldeps w1 - delta w2) (1 / gamma); x += phi w; v = y (1 / beta).  `it` = the iteration this launch
// belongs to: when the stop test fired in THIS iteration the pass still runs, later launches are no-ops.
__global__ __launch_bounds__(kT) void mr_d_kernel(int64_t n, const double *__restrict__ sc, const int *__restrict__ flags, int it,
                                                  double *__restrict__ v, const double *__restrict__ w1,
                                                  const double *__restrict__ w2, double *__restrict__ w,
                                                  double *__restrict__ x, const double *__restrict__ y) {
    if (flags[1] && flags[3] != it) return;
    const double oldeps = sc[S_OLDEPS], delta = sc[S_DELTA], igamma = sc[S_IGAMMA], phi = sc[S_PHI], ibeta = sc[S_IBETA];
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *v2 = reinterpret_cast<double2 *>(v);
    const double2 *a2 = reinterpret_cast<const double2 *>(w1);
    const double2 *b2 = reinterpret_cast<const double2 *>(w2);
    double2 *w_2 = reinterpret_cast<double2 *>(w);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    const double2 *y2 = reinterpret_cast<const double2 *>(y);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 vv = v2[i], av = a2[i], bv = b2[i], yv = y2[i];
        double2 xv = x2[i], wv;
        wv.x = fma(-delta, bv.x, fma(-oldeps, av.x, vv.x)) * igamma;
        wv.y = fma(-delta, bv.y, fma(-oldeps, av.y, vv.y)) * igamma;
        xv.x = fma(phi, wv.x, xv.x);
        xv.y = fma(phi, wv.y, xv.y);
        w_2[i] = wv;
        x2[i] = xv;
        v2[i] = make_double2(yv.x * ibeta, yv.y * ibeta);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double wv = fma(-delta, w2[i], fma(-oldeps, w1[i], v[i])) * igamma;
        w[i] = wv;
        x[i] = fma(phi, wv, x[i]);
        v[i] = y[i] * ibeta;
    }
}

// pass C reads D 16 bytes per lane: a diagonal off a 16-byte boundary takes the general path (the apply, then the dot pass)
inline bool fused_jacobi(const bis_minres *s) { return s->pc.type == BIS_PC_JACOBI && s->pc.outer == 1 && aligned16(s->pc.AD); }

} // namespace

extern "C" {

bis_status bis_minres_create(bis_ctx *ctx, const bis_mat *A, const double *b, double *x, bis_minres **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && b && x && out, "bis_minres_create: bad arguments");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_minres_create: square matrix required");
    BIS_REQUIRE(ctx, aligned16(b) && aligned16(x), "bis_minres_create: b and x must be 16-byte aligned");
    bis_minres *s = new bis_minres;
    s->A = A; s->b = b; s->x = x;
    s->n = A->n_rows;
    s->ld = (s->n + 1) & ~(int64_t)1;
    bis_status st = bis_vec_alloc(ctx, s->ld, &s->v);
    for (int i = 0; i < 3 && st == BIS_OK; ++i) st = bis_vec_alloc(ctx, s->ld, &s->R[i]);
    for (int i = 0; i < 3 && st == BIS_OK; ++i) st = bis_vec_alloc(ctx, s->ld, &s->W[i]);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, S_COUNT, &s->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, s, 4, 1, 2, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st != BIS_OK) { bis_minres_destroy(ctx, s); return st; }
    *out = s;
    return BIS_OK;
}

bis_status bis_minres_set_preconditioner(bis_ctx *ctx, bis_minres *s, int precond_type, const bis_mat *L_strict,
                                         const bis_mat *U_strict, const double *A_D, const double *A_D_inv, const double *L_D,
                                         const double *U_D, int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (!s) return bis_pc_no_handle(ctx, "bis_minres", 0, precond_type);
    return bis_pc_bind(ctx, &s->pc, {"bis_minres", s->n, s->ld, 0, bis_solver_live(*s), 0},
                       {precond_type, L_strict, U_strict, A_D, A_D_inv, L_D, U_D, outer_iters, inner_iters}, {});
}

bis_status bis_minres_destroy(bis_ctx *ctx, bis_minres *s) {
    BIS_CTX_OK(ctx);
    if (!s) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *p : {s->v, s->R[0], s->R[1], s->R[2], s->W[0], s->W[1], s->W[2], s->sc}) hipFree(p);
    bis_solver_core_free(s);
    delete s;
    return BIS_OK;
}

// Iteration k (1-based) reads r1 in R[(k + 1) % 3] and r2 in R[(k + 2) % 3]; the SpMV writes t = R[k % 3], the new r2.  y is
// t itself without a preconditioner, else it goes to r1's buffer, which the next SpMV overwrites.  w1, w2, w likewise.
bis_status bis_minres_init(bis_ctx *ctx, bis_minres *s, double tol, double *r0_norm_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_minres_init: null handle");
    s->enqueued = 0;
    const int64_t n = s->n;
    if (n == 0) {
        if (r0_norm_host) *r0_norm_host = 0.0;
        return BIS_OK;
    }
    double *r2 = s->R[0], *y = s->pc.type == BIS_PC_NONE ? r2 : s->R[2]; // what iteration 0 would have left
    bis_status st = bis_compute_residual(ctx, s->A, s->x, s->b, r2, s->v);
    if (st == BIS_OK && s->pc.type != BIS_PC_NONE) st = bis_pc_apply(ctx, s->pc, n, 0, y, r2);
    double rzy = 0.0;
    if (st == BIS_OK) st = bis_dot(ctx, r2, y, n, &rzy);
    if (st != BIS_OK) return st;
    const double beta1 = sqrt(rzy);
    st = bis_scale(ctx, s->v, y, 1.0 / beta1, n);
    if (st != BIS_OK) return st;
    double sc[S_COUNT] = {0};
    sc[S_BETA] = beta1;
    sc[S_PHIBAR] = beta1;
    sc[S_CS] = -1.0;
    sc[S_STOP] = tol * beta1;
    const int flags[4] = {0, 0, 0, 0};
    for (int i = 0; i < 3; ++i) BIS_HIP_CHECK(ctx, hipMemsetAsync(s->W[i], 0, sizeof(double) * (size_t)s->ld, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc, sc, sizeof sc, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->flags, flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->hist, &beta1, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BIS_SYNC_CHECK(ctx);
    s->initialised = true;
    if (r0_norm_host) *r0_norm_host = beta1;
    return BIS_OK;
}

bis_status bis_minres_iterate(bis_ctx *ctx, bis_minres *s, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && n_iters >= 0 && s->enqueued + n_iters < kMaxIters, "bis_minres_iterate: bad arguments");
    const int64_t n = s->n;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, s->initialised, "bis_minres_iterate: call bis_minres_init first");
    const int g = bis_pair_grid(n, kMaxDotBlocks), g_wide = bis_pair_grid(n, kMaxEwBlocks);
    bis_status st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, s->flags); // the SpMV returns at once when the solve has stopped
    unsigned *cnt_b = s->counters, *cnt_c = s->counters + kCounterSet;
#define BIS_MR_C(MODE, Y)                                                                                                      \
    hipLaunchKernelGGL((mr_c_kernel<MODE>), dim3(g), dim3(kT), 0, ctx->stream, n, s->sc, s->flags, t, (const double *)r2,     \
                       s->pc.AD, Y, ctx->partials, cnt_c, s->hist, s->hist_cap)
    for (int done = 0; done < n_iters; ++done) {
        const int k = s->enqueued + done + 1;
        double *t = s->R[k % 3], *r1 = s->R[(k + 1) % 3], *r2 = s->R[(k + 2) % 3];
        double *w = s->W[k % 3], *w1 = s->W[(k + 1) % 3], *w2 = s->W[(k + 2) % 3];
        double *y = t;
        st = bis_spmv_launch(ctx, s->A, s->v, t, nullptr, nullptr);
        if (st != BIS_OK) { s->enqueued += done; return st; }
        hipLaunchKernelGGL(mr_b_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k >= 2 ? 1 : 0, s->sc, (const int *)s->flags, t,
                           (const double *)r1, (const double *)s->v, ctx->partials, cnt_b);
        if (s->pc.type == BIS_PC_NONE) {
            BIS_MR_C(C_NONE, (double *)nullptr);
        } else if (fused_jacobi(s)) {
            y = r1;
            BIS_MR_C(C_JACOBI, y);
        } else {
            y = r1;
            BIS_MR_C(C_UPDATE_ONLY, (double *)nullptr);
            st = bis_pc_apply(ctx, s->pc, n, 0, y, t);
            if (st != BIS_OK) { s->enqueued += done; return st; } // (the device's count stays behind: call bis_minres_init again)
            BIS_MR_C(C_DOT_ONLY, y);
        }
        hipLaunchKernelGGL(mr_d_kernel, dim3(g_wide), dim3(kT), 0, ctx->stream, n, (const double *)s->sc, (const int *)s->flags, k,
                           s->v, (const double *)w1, (const double *)w2, w, s->x, (const double *)y);
    }
#undef BIS_MR_C
    s->enqueued += n_iters; // the launches were issued whatever the check below says: k keeps matching the device's count
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_minres_status(bis_ctx *ctx, bis_minres *s, int *iters, int *converged, double *hist_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_minres_status: null handle");
    int flags[4] = {0, 0, 0, 0};
    if (bis_status st = bis_solver_read_flags(ctx, *s, 0, 4, flags)) return st;
    if (iters) *iters = flags[0];
    if (converged) *converged = flags[2];
    if (hist_host && hist_cap > 0 && s->initialised) return bis_solver_copy_hist(ctx, *s, 0, std::min(flags[0] + 1, hist_cap), hist_host);
    return BIS_OK;
}

} // extern "C"
