// bis_mbicgstab.hip -- k BiCGSTAB solves on one matrix, advanced in lock-step so that the matrix and the triangles of the
// preconditioner are streamed twice per iteration for all of them (bis_spmm, bis_mapply_preconditioner) instead of 2 k times.
// Per column j the recurrences are bicgstab.hpp's left-preconditioned iteration (bicgstab.hpp:8-83, init :147-169), the
// recorded norm and the stop test those of solver.hpp:177-192 with the threshold tol * ||r0_j||:
//   init:  R = B - A X ; hist_j[0] = ||R_j|| ; P = M^-1 R ; R0 = P ; rho_j = (R_j, P_j)
//          (the shadow residual is the PRECONDITIONED initial residual, as in the reference: init_residual copies it after the apply)
//   Y  = M^-1 P                                   bis_mapply_preconditioner (NONE: no copy, Y is P)
//   V  = A Y                                      bis_spmm (k == 1: bis_spmv)
//   d1_j = (R0_j, V_j) ; alpha_j = rho_j / d1_j   pass 1
//   S  = fma(-alpha_j, V, R)                      pass 2, in place: S lives in R's storage until pass 4
//   St = M^-1 S ; Z = A St                        (NONE: St is S)
//   d2_j = (Z_j, S_j), d3_j = (Z_j, Z_j) ; omega_j = d2_j / d3_j                              pass 3
//   X  = fma(omega_j, St, fma(alpha_j, Y, X)) ; R = fma(-omega_j, Z, S) ; (R0_j, R_j), (R_j, R_j)   pass 4
//          last workgroup: beta_j = (rho'_j / rho_j) * (alpha_j / omega_j) ; rho_j = rho'_j ; norm, history, stop and
//          divergence test of bis_mcg.hip's mcg_book
//   P  = fma(beta_j, fma(-omega_j, V, P), R)      pass 5
// The elementwise arithmetic is that of the single-vector calls (bis_blas1.hip: a +- s b is one fma, beta as
// bis_scalar_ratio_product computes it).  Layout, lane-to-column map and reductions are bis_mcg.hip's (bis_lockstep.hpp): the
// columns never mix, a column's bits depend on (n, k, its own data) only, and the reduction tree is not bis_dot's -- parity
// with a single-vector BiCGSTAB is at the history gate, not bit for bit.  A stopped column is frozen: pass 4 of the stopping
// iteration has updated its x (the reference takes x_new of that iteration), then no lane touches it again; the sweeps and
// the SpMM may still compute its dead values.  When every column has stopped, every later launch returns at once.  A
// breakdown (rho, d1 or d3 reaching 0) gives a non-finite norm, which the divergence test turns into "stopped, not
// converged" for that column alone.  No kernel here waits for another workgroup: there is the arrive ticket and nothing else.
#include "bis_lockstep.hpp"

#include <cfloat>
#include <cmath>

struct bis_mbicgstab : bis_solver_core {
    const bis_mat *A = nullptr;
    const double *B = nullptr;
    double *X = nullptr;
    int64_t n = 0;
    int k = 0;
    // n x k blocks.  Y and St exist with a preconditioner only (without one Y is P and St is S = R's storage)
    double *R = nullptr, *R0 = nullptr, *P = nullptr, *V = nullptr, *Z = nullptr, *Y = nullptr, *St = nullptr;
    double *sc = nullptr;   // [k][B_COUNT]
    // flags: bis_mcg's layout: [1] every column has stopped, [3] the iteration at which the last one did; then per column
    // [4 + 4 j ...]: iters, done, converged, iteration at which its stop test fired.  hist: [k][hist_cap]
    // counters: one last-arriver counter set per reduction: passes 1, 3, 4.  pc's scratch: n x k blocks
};

namespace {

using namespace bis_lockstep;

enum { B_RHO = 0, B_D1, B_ALPHA, B_D2, B_D3, B_OMEGA, B_BETA, B_RR, B_STOP, B_COUNT = 10 };

__device__ __forceinline__ unsigned frozen_mask(const int *flags, int k) {
    unsigned frozen = 0;
    for (int c = 0; c < k; ++c) frozen |= flags[4 + 4 * c + 1] ? 1u << c : 0u;
    return frozen;
}

// pass 1: d1_j = (R0_j, V_j), alpha_j = rho_j / d1_j.  INIT: the end of the start of the solve instead -- P = M^-1 R is in
// place (COPY: no preconditioner, P = R here), R0 = P, rho_j = (R_j, P_j).
template <bool INIT, bool COPY>
__global__ __launch_bounds__(kT) void mbi_d1_kernel(int64_t n, int k, double *sc, const int *flags, const double *R, double *R0,
                                                    double *P, const double *__restrict__ V, double *partials, size_t stride,
                                                    unsigned *counter) {
    __shared__ double lds[kT];
    if (!INIT && flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    const unsigned frozen = INIT ? 0u : frozen_mask(flags, k);
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[1] = {0.0};
    if (live) {
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            if (INIT) {
                const double rv = R[e];
                double pv = rv;
                if (COPY) P[e] = pv; else pv = P[e];
                R0[e] = pv;                                   // solver.hpp:99 after bicgstab.hpp:157
                acc[0] = fma(rv, pv, acc[0]);                 // bicgstab.hpp:167
            } else {
                acc[0] = fma(R0[e], V[e], acc[0]);            // bicgstab.hpp:34
            }
        }
    }
    if (!fold_and_arrive<1>(acc, k, act, lds, partials, stride, counter)) return;
    double out[kMaxK];
    sum_partials<1>(k, partials, stride, lds, out);
    if (t != 0) return;
    for (int c = 0; c < k; ++c) {
        if (frozen >> c & 1u) continue;
        double *scc = sc + c * B_COUNT;
        if (INIT) scc[B_RHO] = out[c];
        else { scc[B_D1] = out[c]; scc[B_ALPHA] = scc[B_RHO] / out[c]; }
    }
}

// pass 2: s = r - alpha_j v, in r's storage
__global__ __launch_bounds__(kT) void mbi_s_kernel(int64_t n, int k, const double *__restrict__ sc, const int *__restrict__ flags,
                                                   const double *__restrict__ V, double *__restrict__ R) {
    if (flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    if (t >= act || flags[4 + 4 * j + 1]) return;
    const double alpha = sc[j * B_COUNT + B_ALPHA];
    const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
    for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) R[e] = fma(-alpha, V[e], R[e]); // bicgstab.hpp:39
}

// pass 3: d2_j = (Z_j, S_j), d3_j = (Z_j, Z_j), omega_j = d2_j / d3_j
__global__ __launch_bounds__(kT) void mbi_omega_kernel(int64_t n, int k, double *sc, const int *flags, const double *__restrict__ Z,
                                                       const double *__restrict__ S, double *partials, size_t stride, unsigned *counter) {
    __shared__ double lds[2 * kT];
    if (flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    const unsigned frozen = frozen_mask(flags, k);
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[2] = {0.0, 0.0};
    if (live) {
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            const double zv = Z[e];
            acc[0] = fma(zv, S[e], acc[0]);                   // bicgstab.hpp:51
            acc[1] = fma(zv, zv, acc[1]);
        }
    }
    if (!fold_and_arrive<2>(acc, k, act, lds, partials, stride, counter)) return;
    double out[2 * kMaxK];
    sum_partials<2>(k, partials, stride, lds, out);
    if (t != 0) return;
    for (int c = 0; c < k; ++c) {
        if (frozen >> c & 1u) continue;
        double *scc = sc + c * B_COUNT;
        scc[B_D2] = out[c];
        scc[B_D3] = out[k + c];
        scc[B_OMEGA] = out[c] / out[k + c];
    }
}

// pass 4: x = (x + alpha_j y) + omega_j st ; r = s - omega_j z ; rho'_j = (R0_j, R_j), (R_j, R_j); the last workgroup does the
// per-column bookkeeping.  PC = false: y is p and st is s (the arguments Y, St are not read).
// INIT: the start of the solve instead -- r = b - A x0 (V holds A x0), (R_j, R_j), history entry 0, the threshold, the flags.
template <bool INIT, bool PC>
__global__ __launch_bounds__(kT) void mbi_update_kernel(int64_t n, int k, double *sc, int *flags, const double *__restrict__ Bv,
                                                        const double *__restrict__ Y, const double *__restrict__ St,
                                                        const double *__restrict__ P, const double *__restrict__ Z,
                                                        const double *__restrict__ R0, double *__restrict__ R,
                                                        double *__restrict__ X, double *partials, size_t stride, unsigned *counter,
                                                        double *hist, int hist_cap, double tol) {
    __shared__ double lds[2 * kT];
    if (!INIT && flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    const unsigned frozen = INIT ? 0u : frozen_mask(flags, k);
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[2] = {0.0, 0.0}; // (r0,r), (r,r)
    if (live) {
        const double alpha = INIT ? 0.0 : sc[j * B_COUNT + B_ALPHA], omega = INIT ? 0.0 : sc[j * B_COUNT + B_OMEGA];
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            // (A x0 in INIT, z otherwise: dead after this pass -- no need to keep its lines)
            const double zv = __builtin_nontemporal_load(Z + e);
            double rv;
            if (INIT) {
                rv = Bv[e] - zv;                              // compute_residual, kernels.hpp:155-162
            } else {
                const double sv = R[e];
                const double yv = PC ? Y[e] : P[e], stv = PC ? St[e] : sv;
                // x is touched here and nowhere else in the iteration: keep it out of the caches the other blocks live in
                const double hv = fma(alpha, yv, __builtin_nontemporal_load(X + e));     // bicgstab.hpp:54
                __builtin_nontemporal_store(fma(omega, stv, hv), X + e);                 // bicgstab.hpp:61
                rv = fma(-omega, zv, sv);                     // bicgstab.hpp:64
                acc[0] = fma(R0[e], rv, acc[0]);              // bicgstab.hpp:68
            }
            R[e] = rv;
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
        double *scc = sc + c * B_COUNT;
        int *fc = flags + 4 + 4 * c;
        if (INIT) {
            const double norm0 = sqrt(out[k + c]);
            for (int q = 0; q < B_COUNT; ++q) scc[q] = 0.0;
            scc[B_RR] = out[k + c];
            scc[B_STOP] = tol * norm0;                        // init_stopping_criteria, solver.hpp:173-175
            hist[(size_t)c * hist_cap] = norm0;
            fc[0] = fc[1] = fc[2] = fc[3] = 0;
        } else if (!(frozen >> c & 1u)) {
            const double rho_new = out[c], rr = out[k + c];
            scc[B_BETA] = (rho_new / scc[B_RHO]) * (scc[B_ALPHA] / scc[B_OMEGA]); // bicgstab.hpp:70
            scc[B_RHO] = rho_new;
            scc[B_RR] = rr;
            const double norm = sqrt(rr);                     // bicgstab.hpp:221
            const int it = fc[0] + 1;
            fc[0] = it;
            double *h = hist + (size_t)c * hist_cap;
            if (it < hist_cap) h[it] = norm;
            const bool conv = fabs(norm) < scc[B_STOP];       // check_stopping_criteria, solver.hpp:177-192
            const bool diverged = fabs(norm) > DBL_MAX || norm != norm;
            if (conv || diverged) { fc[1] = 1; fc[2] = conv ? 1 : 0; fc[3] = it; }
        }
        all = all && fc[1];
    }
    if (INIT) { flags[0] = flags[1] = flags[2] = flags[3] = 0; }
    else if (all) { // the last column has stopped, in this iteration: nothing runs after this pass
        int it_last = 0;
        for (int c = 0; c < k; ++c) it_last = max(it_last, flags[4 + 4 * c + 3]);
        flags[3] = it_last;
        flags[1] = 1;
    }
}

// pass 5: p = r + beta_j (p - omega_j v), for the columns that go on
__global__ __launch_bounds__(kT) void mbi_p_kernel(int64_t n, int k, const double *__restrict__ sc, const int *__restrict__ flags,
                                                   const double *__restrict__ V, const double *__restrict__ R, double *__restrict__ P) {
    if (flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    if (t >= act || flags[4 + 4 * j + 1]) return;
    const double omega = sc[j * B_COUNT + B_OMEGA], beta = sc[j * B_COUNT + B_BETA];
    const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
    for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
        const double tv = fma(-omega, __builtin_nontemporal_load(V + e), P[e]); // bicgstab.hpp:75 (v is dead after this pass)
        P[e] = fma(beta, tv, R[e]);                                              // bicgstab.hpp:78
    }
}

constexpr size_t kPartials = (size_t)2 * kMaxK * kMaxReduceBlocks;

} // namespace

extern "C" {

bis_status bis_mbicgstab_create(bis_ctx *ctx, const bis_mat *A, const double *B, double *X, int n_rhs, bis_mbicgstab **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && B && X && out, "bis_mbicgstab_create: bad arguments");
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kMaxK, "bis_mbicgstab_create: n_rhs must be between 1 and 8");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mbicgstab_create: square matrix required");
    bis_mbicgstab *m = new bis_mbicgstab;
    m->A = A; m->B = B; m->X = X;
    m->n = A->n_rows;
    m->k = n_rhs;
    const int64_t nk = m->n * n_rhs;
    bis_status st = BIS_OK;
    for (double **v : {&m->R, &m->R0, &m->P, &m->V, &m->Z})
        if (st == BIS_OK) st = bis_vec_alloc(ctx, nk, v);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, (int64_t)B_COUNT * n_rhs, &m->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, m, 4 + 4 * (size_t)n_rhs, n_rhs, 3, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, kPartials);
    if (st != BIS_OK) { bis_mbicgstab_destroy(ctx, m); return st; }
    *out = m;
    return BIS_OK;
}

bis_status bis_mbicgstab_set_preconditioner(bis_ctx *ctx, bis_mbicgstab *m, int precond_type, const bis_mat *L_strict,
                                            const bis_mat *U_strict, const double *A_D, const double *A_D_inv, const double *L_D,
                                            const double *U_D, int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (!m) return bis_pc_no_handle(ctx, "bis_mbicgstab", 1, precond_type);
    const int64_t nk = m->n * m->k;
    const bool need_blocks = precond_type != BIS_PC_NONE;
    return bis_pc_bind(ctx, &m->pc, {"bis_mbicgstab", m->n, m->n, m->k, bis_solver_live(*m), 0},
                       {precond_type, L_strict, U_strict, A_D, A_D_inv, L_D, U_D, outer_iters, inner_iters},
                       {{&m->Y, nk, need_blocks && !m->Y}, {&m->St, nk, need_blocks && !m->St}});
}

bis_status bis_mbicgstab_destroy(bis_ctx *ctx, bis_mbicgstab *m) {
    BIS_CTX_OK(ctx);
    if (!m) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *v : {m->R, m->R0, m->P, m->V, m->Z, m->Y, m->St, m->sc}) hipFree(v);
    bis_solver_core_free(m);
    delete m;
    return BIS_OK;
}

bis_status bis_mbicgstab_init(bis_ctx *ctx, bis_mbicgstab *m, double tol, double *r0_norms_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m, "bis_mbicgstab_init: null handle");
    const int64_t n = m->n;
    const int k = m->k;
    m->enqueued = 0;
    if (n == 0) {
        if (r0_norms_host) for (int j = 0; j < k; ++j) r0_norms_host[j] = 0.0;
        return BIS_OK;
    }
    const bool pc = m->pc.type != BIS_PC_NONE;
    bis_status st = bis_ensure_partials(ctx, kPartials);
    if (st == BIS_OK) st = bis_spmm_launch(ctx, m->A, m->X, m->Z, k); // init_residual, bicgstab.hpp:148
    if (st != BIS_OK) return st;
    const int g = lockstep_grid(n, k);
    const size_t stride = (size_t)kMaxReduceBlocks;
    hipLaunchKernelGGL((mbi_update_kernel<true, false>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->B,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, m->Z, (const double *)nullptr, m->R,
                       (double *)nullptr, ctx->partials, stride, m->counters + 2 * kCounterSet, m->hist, m->hist_cap, tol);
    if (pc) {
        st = bis_pc_apply(ctx, m->pc, n, k, m->P, m->R); // bicgstab.hpp:157
        if (st != BIS_OK) return st;
        hipLaunchKernelGGL((mbi_d1_kernel<true, false>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->R, m->R0, m->P,
                           (const double *)nullptr, ctx->partials, stride, m->counters);
    } else {
        hipLaunchKernelGGL((mbi_d1_kernel<true, true>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->R, m->R0, m->P,
                           (const double *)nullptr, ctx->partials, stride, m->counters);
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

bis_status bis_mbicgstab_iterate(bis_ctx *ctx, bis_mbicgstab *m, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && n_iters >= 0 && m->enqueued + n_iters < kMaxIters, "bis_mbicgstab_iterate: bad arguments");
    const int64_t n = m->n;
    const int k = m->k;
    if (n == 0) return BIS_OK;
    const int g = lockstep_grid(n, k);
    const size_t stride = (size_t)kMaxReduceBlocks;
    const bool pc = m->pc.type != BIS_PC_NONE;
    double *Y = pc ? m->Y : m->P, *St = pc ? m->St : m->R;
    bis_status st = bis_ensure_partials(ctx, kPartials);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, m->flags); // the SpMM and the sweeps return at once when every column has stopped
    for (int done = 0; done < n_iters; ++done) {
        if (pc) st = bis_pc_apply(ctx, m->pc, n, k, m->Y, m->P);
        if (st == BIS_OK) st = bis_spmm_launch(ctx, m->A, Y, m->V, k);
        if (st != BIS_OK) { m->enqueued += done; return st; }
        hipLaunchKernelGGL((mbi_d1_kernel<false, false>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->R, m->R0, m->P,
                           m->V, ctx->partials, stride, m->counters);
        hipLaunchKernelGGL(mbi_s_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->V, m->R);
        if (pc) st = bis_pc_apply(ctx, m->pc, n, k, m->St, m->R);
        if (st == BIS_OK) st = bis_spmm_launch(ctx, m->A, St, m->Z, k);
        if (st != BIS_OK) { m->enqueued += done; return st; }
        hipLaunchKernelGGL(mbi_omega_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->Z, m->R, ctx->partials, stride,
                           m->counters + kCounterSet);
#define BIS_MBI_UPDATE(PC)                                                                                                     \
    hipLaunchKernelGGL((mbi_update_kernel<false, PC>), dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->B, m->Y,   \
                       m->St, m->P, m->Z, m->R0, m->R, m->X, ctx->partials, stride, m->counters + 2 * kCounterSet, m->hist,   \
                       m->hist_cap, 0.0)
        if (pc) BIS_MBI_UPDATE(true); else BIS_MBI_UPDATE(false);
#undef BIS_MBI_UPDATE
        hipLaunchKernelGGL(mbi_p_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, m->sc, m->flags, m->V, m->R, m->P);
    }
    BIS_HIP_CHECK(ctx, hipGetLastError());
    m->enqueued += n_iters;
    return BIS_OK;
}

bis_status bis_mbicgstab_status(bis_ctx *ctx, bis_mbicgstab *m, int j, int *iters, int *converged, double *hist_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && j >= 0 && j < m->k, "bis_mbicgstab_status: bad arguments");
    int flags[4] = {0, 0, 0, 0};
    if (bis_status st = bis_solver_read_flags(ctx, *m, 4 + 4 * j, 4, flags)) return st;
    if (iters) *iters = flags[0];
    if (converged) *converged = flags[2];
    if (hist_host && hist_cap > 0) return bis_solver_copy_hist(ctx, *m, j, std::min(flags[0] + 1, hist_cap), hist_host);
    return BIS_OK;
}

} // extern "C"
