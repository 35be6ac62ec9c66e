// bis_mcg.hip -- k CG solves on one matrix, advanced in lock-step so that the matrix is streamed once per iteration for
// all of them (bis_spmm).  Per column j the recurrences, the recorded norm and the stop test are those of bis_cg.hip
// (cg.hpp:6-54, :162-166, solver.hpp:177-192):
//   T       = A P                                  bis_spmm (k == 1: bis_spmv)
//   pap_j   = (T_j, P_j)                           pass A', a pass of its own
//   alpha_j = rz_j / pap_j ; r = fma(-alpha_j, t, r) ; z = r / (1.0 * D) (or z == r) ; (r,z)_j, (r,r)_j      pass B
//   beta_j  = rz_new_j / rz_j ; norm, history, stop test of cg_book with the threshold tol * ||r0_j||        pass B's last workgroup
//   x = fma(alpha_j, p, x) ; p = fma(beta_j, p, z)                                                            pass C
// All vectors are n x k interleaved (V[i*k + j]); scalars, histories and flags live on the device per column.  The columns
// never mix: a lane of the elementwise passes owns ONE column (the first (256 / k) k lanes of a workgroup work, lane t on
// column t % k, on the flat index range -- consecutive lanes touch consecutive doubles), its partial sums are folded per
// column, and the last-arriver reductions (bis_internal.hpp) sum every column's partials in index order.  So a column's
// bits depend on (n, k, its own data) only.  A stopped column is frozen as bis_cg freezes: pass C of the stopping iteration
// still updates its x, then no lane touches it again; when every column has stopped, every later launch returns at once,
// the SpMM included.  The reduction tree is not bis_cg's (other workgroup ranges): parity with bis_cg is at the history
// gate, not bit for bit.
//
// With a general preconditioner (bis_mcg_set_preconditioner) the schedule is bis_cg.hip's general-preconditioner branch per
// column: pass B updates R and the k sums (r,r) only (mcg_update_pc_kernel), Z = M^-1 R through bis_mapply_preconditioner
// (multi-vector sweeps, bis_sptrsm.hip), then the k sums (r_j, z_j) and the per-column bookkeeping (mcg_rz_kernel), then
// pass C.  The sweeps and the elementwise kernels of the apply may still compute a frozen column's z: nothing of that
// column is read afterwards.  Without the call, the None / Jacobi schedule above is launched exactly as before.
#include "bis_lockstep.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

struct bis_mcg : bis_solver_core {
    const bis_mat *A = nullptr;
    const double *A_D = nullptr; // nullptr: no preconditioner
    const double *B = nullptr;
    double *X = nullptr;
    int64_t n = 0;
    int k = 0;
    double *P = nullptr, *R = nullptr, *Z = nullptr, *T = nullptr; // n x k; Z aliases R without a preconditioner
    double *sc = nullptr;   // [k][M_COUNT]
    // flags: [0..3]: [1] every column has stopped, [3] the iteration at which the last one did; then per column
    // [4 + 4 j ...]: iters, done, converged, iteration at which its stop test fired.  hist: [k][hist_cap]
    // counters: three last-arriver counter sets (pass A', pass B, the (r,z) pass of a general preconditioner)
    // pc: the general preconditioner, once set: Z = M^-1 R through bis_pc_apply; its scratch: n x k blocks
};

namespace {

using namespace bis_lockstep;

enum { M_RZ = 0, M_PAP, M_ALPHA, M_BETA, M_RR, M_STOP, M_RR_NEW /* general preconditioner: (r,r) between pass B and the bookkeeping */, M_COUNT = 8 };

// cg_book of bis_cg.hip for one column
__device__ __forceinline__ void mcg_book(double rz_new, double rr, double *sc, int *flags, double *hist, int hist_cap) {
    const double rz_old = sc[M_RZ];
    sc[M_BETA] = rz_new / rz_old;          // cg.hpp:47
    sc[M_RZ] = rz_new;
    sc[M_RR] = rr;
    const double norm = sqrt(rr);          // cg.hpp:164
    const int it = flags[0] + 1;
    flags[0] = it;
    if (it < hist_cap) hist[it] = norm;
    const bool conv = fabs(norm) < sc[M_STOP];
    const bool diverged = fabs(norm) > DBL_MAX || norm != norm;
    if (conv || diverged) { flags[1] = 1; flags[2] = conv ? 1 : 0; flags[3] = it; }
}

// pass A': pap_j = (T_j, P_j)
__global__ __launch_bounds__(kT) void mcg_pap_kernel(int64_t n, int k, const double *__restrict__ T, const double *__restrict__ P,
                                                     double *sc, const int *flags, double *partials, size_t stride, unsigned *counter) {
    __shared__ double lds[kT];
    if (flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    unsigned frozen = 0;
    for (int c = 0; c < k; ++c) frozen |= flags[4 + 4 * c + 1] ? 1u << c : 0u;
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[1] = {0.0};
    if (live) {
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs)
            acc[0] = fma(__builtin_nontemporal_load(T + e), P[e], acc[0]); // (A P is dead after pass B: no need to keep its lines)
    }
    if (!fold_and_arrive<1>(acc, k, act, lds, partials, stride, counter)) return;
    double out[kMaxK];
    sum_partials<1>(k, partials, stride, lds, out);
    if (t == 0)
        for (int c = 0; c < k; ++c)
            if (!(frozen >> c & 1u)) sc[c * M_COUNT + M_PAP] = out[c];
}

// pass B (INIT: the start of the solve instead -- r = b - A x0, z = M^-1 r, p = z, the scalars, history entry 0, flags)
template <bool JACOBI, bool INIT>
__global__ __launch_bounds__(kT) void mcg_update_kernel(int64_t n, int k, double *sc, int *flags, const double *__restrict__ T,
                                                        const double *__restrict__ D, const double *__restrict__ B,
                                                        double *__restrict__ R, double *__restrict__ Z, double *__restrict__ P,
                                                        double *partials, size_t stride, unsigned *counter, double *hist,
                                                        int hist_cap, double tol) {
    __shared__ double lds[2 * kT];
    if (!INIT && flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    unsigned frozen = 0;
    if (!INIT)
        for (int c = 0; c < k; ++c) frozen |= flags[4 + 4 * c + 1] ? 1u << c : 0u;
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[2] = {0.0, 0.0}; // (r,z), (r,r)
    if (live) {
        const double alpha = INIT ? 0.0 : sc[j * M_COUNT + M_RZ] / sc[j * M_COUNT + M_PAP]; // cg.hpp:19-23
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act, e0 = (int64_t)blockIdx.x * act + t;
        int64_t i = e0 / k;
        const int64_t di = gs / k;
        for (int64_t e = e0; e < total; e += gs, i += di) {
            const double tv = __builtin_nontemporal_load(T + e);
            double rv;
            if (INIT) rv = B[e] - tv;                 // compute_residual, kernels.hpp:155-162
            else rv = fma(-alpha, tv, R[e]);          // cg.hpp:31
            R[e] = rv;
            double zv = rv;
            if (JACOBI) { zv = rv / (1.0 * D[i]); Z[e] = zv; } // kernels.hpp:151
            if (INIT) P[e] = zv;
            acc[0] = fma(rv, zv, acc[0]);
            acc[1] = fma(rv, rv, acc[1]);
        }
    }
    if (!fold_and_arrive<2>(acc, k, act, lds, partials, stride, counter)) return;
    // every other workgroup has read its columns' scalars and flags before it arrived: they may change now
    double out[2 * kMaxK];
    sum_partials<2>(k, partials, stride, lds, out);
    if (t != 0) return;
    bool all = true;
    for (int c = 0; c < k; ++c) {
        double *scc = sc + c * M_COUNT;
        int *fc = flags + 4 + 4 * c;
        if (INIT) {
            const double norm0 = sqrt(out[k + c]);
            scc[M_RZ] = out[c];
            scc[M_RR] = out[k + c];
            scc[M_STOP] = tol * norm0;             // init_stopping_criteria, solver.hpp:173-175
            scc[M_PAP] = scc[M_ALPHA] = scc[M_BETA] = 0.0;
            hist[(size_t)c * hist_cap] = norm0;
            fc[0] = fc[1] = fc[2] = fc[3] = 0;
        } else if (!(frozen >> c & 1u)) {
            scc[M_ALPHA] = scc[M_RZ] / scc[M_PAP];  // pass C applies it to x
            mcg_book(out[c], out[k + c], scc, fc, hist + (size_t)c * hist_cap, hist_cap);
        }
        all = all && fc[1];
    }
    if (INIT) { flags[0] = flags[1] = flags[2] = flags[3] = 0; }
    else if (all) { // the last column has stopped, in this iteration: pass C of it still runs, nothing after it
        int it_last = 0;
        for (int c = 0; c < k; ++c) it_last = max(it_last, flags[4 + 4 * c + 3]);
        flags[3] = it_last;
        flags[1] = 1;
    }
}

// General preconditioner, pass B: r = fma(-alpha_j, t, r) and (r,r)_j only (INIT: r = b - A x0); z and (r,z) follow after
// the apply.  The last workgroup parks alpha_j and (r,r)_j for mcg_rz_kernel and pass C.
template <bool INIT>
__global__ __launch_bounds__(kT) void mcg_update_pc_kernel(int64_t n, int k, double *sc, const int *flags, const double *__restrict__ T,
                                                           const double *__restrict__ B, double *__restrict__ R, double *partials,
                                                           size_t stride, unsigned *counter) {
    __shared__ double lds[kT];
    if (!INIT && flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    unsigned frozen = 0;
    if (!INIT)
        for (int c = 0; c < k; ++c) frozen |= flags[4 + 4 * c + 1] ? 1u << c : 0u;
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[1] = {0.0};
    if (live) {
        const double alpha = INIT ? 0.0 : sc[j * M_COUNT + M_RZ] / sc[j * M_COUNT + M_PAP]; // cg.hpp:19-23
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            const double tv = __builtin_nontemporal_load(T + e);
            double rv;
            if (INIT) rv = B[e] - tv;                 // compute_residual, kernels.hpp:155-162
            else rv = fma(-alpha, tv, R[e]);          // cg.hpp:31
            R[e] = rv;
            acc[0] = fma(rv, rv, acc[0]);
        }
    }
    if (!fold_and_arrive<1>(acc, k, act, lds, partials, stride, counter)) return;
    // every other workgroup has read its columns' scalars and flags before it arrived: they may change now
    double out[kMaxK];
    sum_partials<1>(k, partials, stride, lds, out);
    if (t != 0) return;
    for (int c = 0; c < k; ++c) {
        if (frozen >> c & 1u) continue;
        double *scc = sc + c * M_COUNT;
        if (!INIT) scc[M_ALPHA] = scc[M_RZ] / scc[M_PAP]; // pass C applies it to x
        scc[M_RR_NEW] = out[c];
    }
}

// General preconditioner, after Z = M^-1 R: the k sums (r_j, z_j), then the per-column bookkeeping of pass B's last
// workgroup (INIT: p = z and the start of the solve instead).
template <bool INIT>
__global__ __launch_bounds__(kT) void mcg_rz_kernel(int64_t n, int k, double *sc, int *flags, const double *__restrict__ R,
                                                    const double *__restrict__ Z, double *__restrict__ P, double *partials,
                                                    size_t stride, unsigned *counter, double *hist, int hist_cap, double tol) {
    __shared__ double lds[kT];
    if (!INIT && flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    unsigned frozen = 0;
    if (!INIT)
        for (int c = 0; c < k; ++c) frozen |= flags[4 + 4 * c + 1] ? 1u << c : 0u;
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[1] = {0.0};
    if (live) {
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            const double zv = Z[e];
            if (INIT) P[e] = zv;
            acc[0] = fma(R[e], zv, acc[0]);
        }
    }
    if (!fold_and_arrive<1>(acc, k, act, lds, partials, stride, counter)) return;
    double out[kMaxK];
    sum_partials<1>(k, partials, stride, lds, out);
    if (t != 0) return;
    bool all = true;
    for (int c = 0; c < k; ++c) {
        double *scc = sc + c * M_COUNT;
        int *fc = flags + 4 + 4 * c;
        if (INIT) {
            const double norm0 = sqrt(scc[M_RR_NEW]);
            scc[M_RZ] = out[c];
            scc[M_RR] = scc[M_RR_NEW];
            scc[M_STOP] = tol * norm0;             // init_stopping_criteria, solver.hpp:173-175
            scc[M_PAP] = scc[M_ALPHA] = scc[M_BETA] = 0.0;
            hist[(size_t)c * hist_cap] = norm0;
            fc[0] = fc[1] = fc[2] = fc[3] = 0;
        } else if (!(frozen >> c & 1u)) {
            mcg_book(out[c], scc[M_RR_NEW], scc, fc, hist + (size_t)c * hist_cap, hist_cap);
        }
        all = all && fc[1];
    }
    if (INIT) { flags[0] = flags[1] = flags[2] = flags[3] = 0; }
    else if (all) { // the last column has stopped, in this iteration: pass C of it still runs, nothing after it
        int it_last = 0;
        for (int c = 0; c < k; ++c) it_last = max(it_last, flags[4 + 4 * c + 3]);
        flags[3] = it_last;
        flags[1] = 1;
    }
}

// pass C: x += alpha_j p ; p = z + beta_j p.  `it`: the iteration this launch belongs to -- a column whose stop test fired
// in THIS iteration still gets its x update (bis_cg.hip, pass C).
__global__ __launch_bounds__(kT) void mcg_p_update_kernel(int64_t n, int k, const double *__restrict__ sc, const int *__restrict__ flags,
                                                          int it, const double *__restrict__ Z, double *__restrict__ X,
                                                          double *__restrict__ P) {
    if (flags[1] && flags[3] != it) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    if (t >= act) return;
    const int *fj = flags + 4 + 4 * j;
    if (fj[1] && fj[3] != it) return;
    const double alpha = sc[j * M_COUNT + M_ALPHA], beta = sc[j * M_COUNT + M_BETA];
    const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
    for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
        const double pv = P[e];
        // x is touched here and nowhere else in the iteration: keep it out of the caches p, r and A p live in
        const double xv = fma(alpha, pv, __builtin_nontemporal_load(X + e));
        __builtin_nontemporal_store(xv, X + e);
        P[e] = fma(beta, pv, Z[e]);
    }
}

} // namespace

extern "C" {

bis_status bis_mcg_create(bis_ctx *ctx, const bis_mat *A, const double *A_D, const double *B, double *X, int n_rhs, bis_mcg **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && B && X && out, "bis_mcg_create: bad arguments");
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kMaxK, "bis_mcg_create: n_rhs must be between 1 and 8");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mcg_create: square matrix required");
    bis_mcg *m = new bis_mcg;
    m->A = A; m->A_D = A_D; m->B = B; m->X = X;
    m->n = A->n_rows;
    m->k = n_rhs;
    const int64_t nk = m->n * n_rhs;
    bis_status st = bis_vec_alloc(ctx, nk, &m->P);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, nk, &m->R);
    if (st == BIS_OK && A_D) st = bis_vec_alloc(ctx, nk, &m->Z);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, nk, &m->T);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, (int64_t)M_COUNT * n_rhs, &m->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, m, 4 + 4 * (size_t)n_rhs, n_rhs, 3, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, (size_t)2 * kMaxK * kMaxReduceBlocks);
    if (st != BIS_OK) { bis_mcg_destroy(ctx, m); return st; }
    if (!A_D) m->Z = m->R; // z aliases r without a preconditioner
    *out = m;
    return BIS_OK;
}

bis_status bis_mcg_set_preconditioner(bis_ctx *ctx, bis_mcg *m, int precond_type, const bis_mat *L_strict, const bis_mat *U_strict,
                                      const double *A_D, const double *A_D_inv, const double *L_D, const double *U_D,
                                      int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (!m) return bis_pc_no_handle(ctx, "bis_mcg", 1, precond_type);
    return bis_pc_bind(ctx, &m->pc, {"bis_mcg", m->n, m->n, m->k, bis_solver_live(*m), 0},
                       {precond_type, L_strict, U_strict, A_D, A_D_inv, L_D, U_D, outer_iters, inner_iters},
                       {{&m->Z, m->n * m->k, m->Z == m->R}}); // z aliased r (no preconditioner at creation): it needs its own storage now
}

bis_status bis_mcg_destroy(bis_ctx *ctx, bis_mcg *m) {
    BIS_CTX_OK(ctx);
    if (!m) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    hipFree(m->P);
    hipFree(m->R);
    if (m->Z != m->R) hipFree(m->Z);
    hipFree(m->T);
    hipFree(m->sc);
    bis_solver_core_free(m);
    delete m;
    return BIS_OK;
}

bis_status bis_mcg_init(bis_ctx *ctx, bis_mcg *m, double tol, double *r0_norms_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m, "bis_mcg_init: null handle");
    const int64_t n = m->n;
    const int k = m->k;
    m->enqueued = 0;
    if (n == 0) {
        if (r0_norms_host) for (int j = 0; j < k; ++j) r0_norms_host[j] = 0.0;
        return BIS_OK;
    }
    bis_status st = bis_ensure_partials(ctx, (size_t)2 * kMaxK * kMaxReduceBlocks);
    if (st == BIS_OK) st = bis_spmm_launch(ctx, m->A, m->X, m->T, k); // init_residual, cg.hpp:100-118
    if (st != BIS_OK) return st;
    const int g = lockstep_grid(n, k);
    if (m->pc.set) { // general preconditioner: r0 and (r,r), z0 = M^-1 r0, then p0 = z0, (r,z) and the start of the solve
        hipLaunchKernelGGL(mcg_update_pc_kernel<true>, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->T, m->B, m->R,
                           ctx->partials, (size_t)kMaxReduceBlocks, m->counters + kCounterSet);
        st = bis_pc_apply(ctx, m->pc, n, k, m->Z, m->R);
        if (st != BIS_OK) return st;
        hipLaunchKernelGGL(mcg_rz_kernel<true>, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->R, m->Z, m->P,
                           ctx->partials, (size_t)kMaxReduceBlocks, m->counters + 2 * kCounterSet, m->hist, m->hist_cap, tol);
    } else {
#define BIS_MCG_INIT(J)                                                                                                      \
    hipLaunchKernelGGL((mcg_update_kernel<J, true>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->T, m->A_D,  \
                       m->B, m->R, m->Z, m->P, ctx->partials, (size_t)kMaxReduceBlocks, m->counters + kCounterSet, m->hist,  \
                       m->hist_cap, tol)
    if (m->A_D) BIS_MCG_INIT(true); else BIS_MCG_INIT(false);
#undef BIS_MCG_INIT
    }
    m->initialised = true;
    BIS_HIP_CHECK(ctx, hipGetLastError());
    double norms[kMaxK] = {0};
    for (int j = 0; j < k; ++j)
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(&norms[j], m->hist + (size_t)j * m->hist_cap, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BIS_SYNC_CHECK(ctx);
    if (r0_norms_host) for (int j = 0; j < k; ++j) r0_norms_host[j] = norms[j];
    return BIS_OK;
}

bis_status bis_mcg_iterate(bis_ctx *ctx, bis_mcg *m, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && n_iters >= 0 && m->enqueued + n_iters < kMaxIters, "bis_mcg_iterate: bad arguments");
    const int64_t n = m->n;
    const int k = m->k;
    if (n == 0) return BIS_OK;
    const int g = lockstep_grid(n, k);
    bis_status st = bis_ensure_partials(ctx, (size_t)2 * kMaxK * kMaxReduceBlocks);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, m->flags); // the SpMM (k == 1: the SpMV) returns at once when every column has stopped
    for (int done = 0; done < n_iters; ++done) {
        const int it = m->enqueued + done + 1;
        st = bis_spmm_launch(ctx, m->A, m->P, m->T, k);
        if (st != BIS_OK) { m->enqueued += done; return st; }
        hipLaunchKernelGGL(mcg_pap_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->T, m->P, m->sc, m->flags, ctx->partials,
                           (size_t)kMaxReduceBlocks, m->counters);
        if (m->pc.set) { // general preconditioner: bis_cg.hip's schedule (cg_enqueue_iteration, cg->pc.set) per column
            hipLaunchKernelGGL(mcg_update_pc_kernel<false>, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->T, m->B, m->R,
                               ctx->partials, (size_t)kMaxReduceBlocks, m->counters + kCounterSet);
            st = bis_pc_apply(ctx, m->pc, n, k, m->Z, m->R);
            if (st != BIS_OK) { m->enqueued += done; return st; }
            hipLaunchKernelGGL(mcg_rz_kernel<false>, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->R, m->Z, m->P,
                               ctx->partials, (size_t)kMaxReduceBlocks, m->counters + 2 * kCounterSet, m->hist, m->hist_cap, 0.0);
        } else {
#define BIS_MCG_UPDATE(J)                                                                                                    \
    hipLaunchKernelGGL((mcg_update_kernel<J, false>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->T, m->A_D, \
                       m->B, m->R, m->Z, m->P, ctx->partials, (size_t)kMaxReduceBlocks, m->counters + kCounterSet, m->hist,  \
                       m->hist_cap, 0.0)
        if (m->A_D) BIS_MCG_UPDATE(true); else BIS_MCG_UPDATE(false);
#undef BIS_MCG_UPDATE
        }
        hipLaunchKernelGGL(mcg_p_update_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, it, m->Z, m->X, m->P);
    }
    BIS_HIP_CHECK(ctx, hipGetLastError());
    m->enqueued += n_iters;
    return BIS_OK;
}

bis_status bis_mcg_status(bis_ctx *ctx, bis_mcg *m, int j, int *iters, int *converged, double *hist_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && j >= 0 && j < m->k, "bis_mcg_status: bad arguments");
    int flags[4] = {0, 0, 0, 0};
    if (bis_status st = bis_solver_read_flags(ctx, *m, 4 + 4 * j, 4, flags)) return st;
    if (iters) *iters = flags[0];
    if (converged) *converged = flags[2];
    if (hist_host && hist_cap > 0) return bis_solver_copy_hist(ctx, *m, j, std::min(flags[0] + 1, hist_cap), hist_host);
    return BIS_OK;
}

} // extern "C"
