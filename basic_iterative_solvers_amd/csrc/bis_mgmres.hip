// bis_mgmres.hip -- k restarted GMRES(m) solves on one matrix, advanced in lock-step so that the matrix and the triangles of
// the preconditioner are streamed once per iteration for all of them (bis_spmm, bis_mapply_preconditioner in place), the
// Gram-Schmidt coefficients stay on the device and the Givens / least-squares algebra runs there, one lane per column.
// Per column j the iteration is gmres.hpp's left-preconditioned GMRES(m) (host/methods/gmres.hpp, the oracle's run_gmres):
//   init:     W = B - A X ; hist_j[0] = ||W_j|| (unpreconditioned) ; threshold_j = tol hist_j[0]
//             W = M^-1 W ; beta_j = ||W_j|| ; g_j = (beta_j, 0, ...) ; V_0 = W / beta_j
//   position n of a cycle (the host knows n: every live column shares the iteration count, n = enqueued mod m):
//             W = M^-1 A V_n                              bis_spmm, bis_mapply_preconditioner with OUT = IN
//             h_0 = (W, V_0)                              pass 0
//             W -= h_{i-1} V_{i-1} ; h_i = (W, V_i)       passes 1 .. n   (one fma per element and pass, fma-accumulated dots)
//             W -= h_n V_n ; (W, W)                       pass n + 1; the last workgroup, lane j for column j:
//                 h_{n+1} = sqrt, its inverse; the stored rotations on (h_0 .. h_n); den = sqrt(a^2 + b^2), c = a / den,
//                 s = b / den; column n of the rotated triangle; g_{n+1} = -s g_n, g_n = c g_n; history entry |g_{n+1}|;
//                 the stop and divergence test of bis_mcg.hip's mcg_book; y by back substitution when the column stops or
//                 the cycle ends (the column is then "pending")
//             V_{n+1} = W / h_{n+1}                       scale (not at the end of a cycle: V_m is never read)
//   cycle end (n + 1 == m): X_j += sum_{i < n_j} y_i V_i  combine, pending columns only (the stopped ones with the steps of
//                                                         their own cycle), the last workgroup clears the pending flags
//             W = M^-1 (B - A X) ; beta_j = ||W_j||, ONE MORE history entry (Solver::init_residual after a restart), the stop
//             test on beta_j ; V_0 = W / beta_j           for the columns that have not stopped
// The combine also runs at the end of every bis_mgmres_iterate call (it returns at once when nothing is pending), so a
// stopped column's X is final when the call has enqueued its last kernel; after that no lane touches the column's X, basis,
// state or history.  When every column has stopped, every later launch returns at once.  Layout, lane-to-column map and
// reductions are bis_mcg.hip's (bis_lockstep.hpp): the columns never mix, a column's bits depend on (n, k, m, its own data)
// only, and no kernel waits for another workgroup -- there is the arrive ticket and nothing else.  The loads of the V_i and
// W streams are plain loads: whether non-temporal ones help here has not been measured.
// Elementwise and reduction traffic at position n, per row and column: pass 0 reads W, V_0 (16 B), each of the n middle
// passes reads W, V_{i-1}, V_i and writes W (32 B), the last reads W, V_n and writes W (24 B), the scale reads W and
// writes V_{n+1} (16 B): 56 + 32 n bytes.
#include "bis_gmres_state.hpp"
#include "bis_lockstep.hpp"

struct bis_mgmres : bis_solver_core {
    const bis_mat *A = nullptr;
    const double *B = nullptr;
    double *X = nullptr;
    int64_t n = 0;
    int k = 0, m = 0;
    double *V = nullptr;    // m + 1 blocks of n x k
    double *W = nullptr;    // n x k
    double *st = nullptr;   // [k][state_size(m)]: the per-column Givens / least-squares state (gmres_layout)
    // flags: bis_mcg's layout in the first 4 + 4 k ints; then per column [4 + 4 k + 4 j ...] the X_* words: pending, steps of
    // the pending combine, history entries written, steps done in the current cycle.  hist: [k][hist_cap].  counters: three
    // last-arriver counter sets: Gram-Schmidt passes, residual / norm passes, combine.  pc's scratch: n x k blocks
};

namespace {

using namespace bis_lockstep;

enum { BK_INIT0 = 1, BK_BETA = 2, BK_RESTART = 4 };

__device__ __forceinline__ unsigned frozen_mask(const int *flags, int k) {
    unsigned frozen = 0;
    for (int c = 0; c < k; ++c) frozen |= flags[4 + 4 * c + 1] ? 1u << c : 0u;
    return frozen;
}

// flags[1] / flags[3] when the last column has stopped (thread 0 of the last workgroup, after the lanes' bookkeeping)
__device__ __forceinline__ void mgm_all_stopped(int *flags, int k, const int *sdone) {
    bool all = true;
    for (int c = 0; c < k; ++c) all = all && sdone[c];
    if (!all) return;
    int it_last = 0;
    for (int c = 0; c < k; ++c) it_last = max(it_last, flags[4 + 4 * c + 3]);
    flags[3] = it_last;
    flags[1] = 1;
}

// One Gram-Schmidt pass at position n.  MODE 0: h_0 = (W, V_0) (Vnext = V_0).  MODE 1: W -= h_{ci} Vprev, h_{ci+1} = (W, Vnext).
// MODE 2: W -= h_{ci} Vprev, (W, W), and the last workgroup does the columns' bookkeeping (ci = n).
template <int MODE>
__global__ __launch_bounds__(kT) void mgm_gs_kernel(int64_t n, int k, gmres_layout L, int pos, int ci, double *st, int *flags,
                                                    double *__restrict__ W, const double *__restrict__ Vprev,
                                                    const double *__restrict__ Vnext, double *partials, size_t stride,
                                                    unsigned *counter, double *hist, int hist_cap) {
    __shared__ double lds[kT];
    __shared__ double colsum[kMaxK];
    __shared__ int sdone[kMaxK];
    if (flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    const unsigned frozen = frozen_mask(flags, k);
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[1] = {0.0};
    if (live) {
        const double hc = MODE == 0 ? 0.0 : st[(size_t)j * L.size() + L.h() + ci];
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            double w = W[e];
            if (MODE != 0) {
                w = fma(-hc, Vprev[e], w);                    // subtract_vectors(w, w, v_i, h_i), gmres.hpp:25
                W[e] = w;
            }
            acc[0] = fma(w, MODE == 2 ? w : Vnext[e], acc[0]); // dot(w, v_i), :13-14 ; euclidean_vec_norm, :36-38
        }
    }
    if (!fold_and_arrive<1>(acc, k, act, lds, partials, stride, counter)) return;
    // every other workgroup has read its columns' coefficients and flags before it arrived: they may change now
    double out[kMaxK];
    sum_partials<1>(k, partials, stride, lds, out);
    if (t == 0)
        for (int c = 0; c < k; ++c) colsum[c] = out[c];
    __syncthreads();
    if (t < k) {
        double *s = st + (size_t)t * L.size();
        if (!(frozen >> t & 1u)) {
            if (MODE == 2)
                gmres_book(L, colsum[t], pos, s, flags + 4 + 4 * t, flags + 4 + 4 * k + 4 * t, hist + (size_t)t * hist_cap, hist_cap);
            else
                s[L.h() + (MODE == 0 ? 0 : ci + 1)] = colsum[t];
        }
        if (MODE == 2) sdone[t] = flags[4 + 4 * t + 1];
    }
    if (MODE != 2) return;
    __syncthreads();
    if (t == 0) mgm_all_stopped(flags, k, sdone);
}

// Start of the solve and of every cycle.  RESID: W = B - W (W holds A X), else W is read only.  REDUCE: (W_j, W_j) and the
// last workgroup's bookkeeping -- BK_INIT0: history entry 0, the threshold, the flags; BK_BETA: beta_j, g_j, 1 / beta_j;
// BK_RESTART: the extra history entry and the stop test on beta_j.
template <bool RESID, bool REDUCE>
__global__ __launch_bounds__(kT) void mgm_resid_kernel(int64_t n, int k, gmres_layout L, int book, double tol, double *st, int *flags,
                                                       const double *__restrict__ Bv, double *__restrict__ W, double *partials,
                                                       size_t stride, unsigned *counter, double *hist, int hist_cap) {
    __shared__ double lds[kT];
    __shared__ double colsum[kMaxK];
    __shared__ int sdone[kMaxK];
    const bool init0 = book & BK_INIT0;
    if (!init0 && flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    const unsigned frozen = init0 ? 0u : frozen_mask(flags, k);
    const bool live = t < act && !(frozen >> j & 1u);
    double acc[1] = {0.0};
    if (live) {
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            double r = W[e];
            if (RESID) {
                r = Bv[e] - r;                                // compute_residual, kernels.hpp:155-162
                W[e] = r;
            }
            if (REDUCE) acc[0] = fma(r, r, acc[0]);
        }
    }
    if (!REDUCE) return;
    if (!fold_and_arrive<1>(acc, k, act, lds, partials, stride, counter)) return;
    double out[kMaxK];
    sum_partials<1>(k, partials, stride, lds, out);
    if (t == 0)
        for (int c = 0; c < k; ++c) colsum[c] = out[c];
    __syncthreads();
    if (t < k) {
        double *s = st + (size_t)t * L.size();
        int *fc = flags + 4 + 4 * t, *xc = flags + 4 + 4 * k + 4 * t;
        double *h = hist + (size_t)t * hist_cap;
        const double norm = sqrt(colsum[t]);
        if (init0) {
            for (int q = 0; q < L.size(); ++q) s[q] = 0.0;
            h[0] = norm;                                      // the unpreconditioned norm opens the history
            s[L.stop()] = tol * norm;                         // init_stopping_criteria, solver.hpp:173-175
            fc[0] = fc[1] = fc[2] = fc[3] = 0;
            xc[X_PENDING] = 0; xc[X_STEPS] = 0; xc[X_NHIST] = 1; xc[X_POS] = 0;
        }
        if ((book & BK_BETA) && !(frozen >> t & 1u)) {
            s[L.beta()] = norm;
            s[L.g()] = norm;
            s[L.inv()] = 1.0 / norm;
            xc[X_POS] = 0;
            if (book & BK_RESTART) {
                const int nh = xc[X_NHIST];
                if (nh < hist_cap) h[nh] = norm;              // Solver::init_residual after a restart
                xc[X_NHIST] = nh + 1;
                const bool conv = norm < s[L.stop()];
                const bool diverged = norm > DBL_MAX || norm != norm;
                if (conv || diverged) { fc[1] = 1; fc[2] = conv ? 1 : 0; fc[3] = fc[0]; }
            }
        }
        sdone[t] = init0 ? 0 : fc[1];
    }
    __syncthreads();
    if (t != 0) return;
    if (init0) flags[0] = flags[1] = flags[2] = flags[3] = 0;
    else mgm_all_stopped(flags, k, sdone);
}

// Vdst = W * (1 / norm_j) for the columns that go on (scale, gmres.hpp:44-46)
__global__ __launch_bounds__(kT) void mgm_scale_kernel(int64_t n, int k, gmres_layout L, const double *__restrict__ st,
                                                       const int *__restrict__ flags, const double *__restrict__ W,
                                                       double *__restrict__ Vdst) {
    if (flags[1]) return;
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    if (t >= act || flags[4 + 4 * j + 1]) return;
    const double inv = st[(size_t)j * L.size() + L.inv()];
    const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
    for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) Vdst[e] = W[e] * inv;
}

// X_j += sum_{i < steps_j} y_{j,i} V_i[., j] for the pending columns (multi_axpy and sum_vectors of get_explicit_x); the last
// workgroup clears the pending flags.  SOL: OUT_j = X_j + sum over the steps of the current cycle with the y of
// mgm_ysol_kernel for a live column, OUT_j = X_j for a stopped one; nothing of the handle changes.
template <bool SOL>
__global__ __launch_bounds__(kT) void mgm_combine_kernel(int64_t n, int k, gmres_layout L, const double *st, int *flags,
                                                         const double *__restrict__ V, const double *X, double *OUT,
                                                         unsigned *counter) {
    __shared__ double ys[kMaxK * kMaxRestart];
    __shared__ int steps[kMaxK];
    const int act = (kT / k) * k, t = threadIdx.x, j = t % k;
    int *xc = flags + 4 + 4 * k;
    if (t < k) {
        if (SOL) steps[t] = flags[4 + 4 * t + 1] ? 0 : xc[4 * t + X_POS];
        else steps[t] = xc[4 * t + X_PENDING] ? xc[4 * t + X_STEPS] : -1;
    }
    __syncthreads();
    if (!SOL) {
        bool any = false;
        for (int c = 0; c < k; ++c) any = any || steps[c] >= 0;
        if (!any) return;
    }
    for (int q = t; q < k * L.m; q += kT) {
        const int c = q / L.m, i = q - c * L.m;
        ys[c * kMaxRestart + i] = i < steps[c] ? st[(size_t)c * L.size() + (SOL ? L.ysol() : L.y()) + i] : 0.0;
    }
    __syncthreads();
    const int ns = steps[j];
    if (t < act && (SOL || ns >= 0)) {
        const double *y = ys + j * kMaxRestart;
        const int64_t total = n * k, gs = (int64_t)gridDim.x * act;
        for (int64_t e = (int64_t)blockIdx.x * act + t; e < total; e += gs) {
            double acc = 0.0;
            for (int i = 0; i < ns; ++i) acc = fma(V[(int64_t)i * total + e], y[i], acc); // multi_axpy_kernel's order
            const double xv = X[e];
            if (SOL) OUT[e] = ns > 0 ? xv + acc : xv;
            else OUT[e] = xv + acc;                           // sum_vectors(x, x_old, Vy)
        }
    }
    if (SOL) return;
    // every workgroup has read the pending flags and the y it needs before it arrives
    if (t == 0 && arrive_last_set(counter, blockIdx.x, gridDim.x))
        for (int c = 0; c < k; ++c) xc[4 * c + X_PENDING] = 0;
}

// the y of a live column at its current position, for bis_mgmres_solution: lane j, column j, into the state's ysol
__global__ void mgm_ysol_kernel(int k, gmres_layout L, double *st, const int *flags) {
    const int t = threadIdx.x;
    if (t >= k || flags[4 + 4 * t + 1]) return;
    double *s = st + (size_t)t * L.size();
    gmres_backsub(L, s, flags[4 + 4 * k + 4 * t + X_POS], s + L.ysol());
}

constexpr size_t kPartials = (size_t)kMaxK * kMaxReduceBlocks;
constexpr size_t kStride = (size_t)kMaxReduceBlocks;

// W holds A X: the residual, its preconditioned norm, V_0 -- at init (restart = false) and at the start of every later cycle
bis_status mgm_start_cycle(bis_ctx *ctx, bis_mgmres *m, bool restart, double tol) {
    const int64_t n = m->n;
    const int k = m->k, g = lockstep_grid(n, k);
    const gmres_layout L{m->m};
    const bool pc = m->pc.type != BIS_PC_NONE;
    const int first = restart ? 0 : BK_INIT0, beta = BK_BETA | (restart ? BK_RESTART : 0);
    unsigned *counter = m->counters + kCounterSet;
#define BIS_MGM_RESID(RESID, REDUCE, BOOK)                                                                                     \
    hipLaunchKernelGGL((mgm_resid_kernel<RESID, REDUCE>), dim3(g), dim3(kT), 0, ctx->stream, n, k, L, BOOK, tol, m->st,        \
                       m->flags, m->B, m->W, ctx->partials, kStride, counter, m->hist, m->hist_cap)
    if (!pc) {
        BIS_MGM_RESID(true, true, first | beta);
    } else {
        if (restart) BIS_MGM_RESID(true, false, 0); else BIS_MGM_RESID(true, true, first);
        bis_status st = bis_pc_apply(ctx, m->pc, n, k, m->W, m->W); // W = M^-1 W
        if (st != BIS_OK) return st;
        BIS_MGM_RESID(false, true, beta);
    }
#undef BIS_MGM_RESID
    hipLaunchKernelGGL(mgm_scale_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, L, m->st, m->flags, m->W, m->V);
    return BIS_OK;
}

} // namespace

extern "C" {

bis_status bis_mgmres_create(bis_ctx *ctx, const bis_mat *A, const double *B, double *X, int n_rhs, int restart_len,
                             bis_mgmres **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && B && X && out, "bis_mgmres_create: bad arguments");
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kMaxK, "bis_mgmres_create: n_rhs must be between 1 and 8");
    BIS_REQUIRE(ctx, restart_len >= 1 && restart_len <= kMaxRestart, "bis_mgmres_create: restart_len must be between 1 and 64");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mgmres_create: square matrix required");
    bis_mgmres *m = new bis_mgmres;
    m->A = A; m->B = B; m->X = X;
    m->n = A->n_rows;
    m->k = n_rhs;
    m->m = restart_len;
    const int64_t nk = m->n * n_rhs;
    const gmres_layout L{restart_len};
    bis_status st = bis_vec_alloc(ctx, nk * (restart_len + 1), &m->V);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, nk, &m->W);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, (int64_t)L.size() * n_rhs, &m->st);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, m, 4 + 8 * (size_t)n_rhs, n_rhs, 3, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, kPartials);
    if (st != BIS_OK) { bis_mgmres_destroy(ctx, m); return st; }
    *out = m;
    return BIS_OK;
}

bis_status bis_mgmres_set_preconditioner(bis_ctx *ctx, bis_mgmres *m, int precond_type, const bis_mat *L_strict,
                                         const bis_mat *U_strict, const double *A_D, const double *A_D_inv, const double *L_D,
                                         const double *U_D, int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (!m) return bis_pc_no_handle(ctx, "bis_mgmres", 1, precond_type);
    return bis_pc_bind(ctx, &m->pc, {"bis_mgmres", m->n, m->n, m->k, bis_solver_live(*m), 0},
                       {precond_type, L_strict, U_strict, A_D, A_D_inv, L_D, U_D, outer_iters, inner_iters}, {});
}

bis_status bis_mgmres_destroy(bis_ctx *ctx, bis_mgmres *m) {
    BIS_CTX_OK(ctx);
    if (!m) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *v : {m->V, m->W, m->st}) hipFree(v);
    bis_solver_core_free(m);
    delete m;
    return BIS_OK;
}

bis_status bis_mgmres_init(bis_ctx *ctx, bis_mgmres *m, double tol, double *r0_norms_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m, "bis_mgmres_init: null handle");
    const int64_t n = m->n;
    const int k = m->k;
    m->enqueued = 0;
    if (n == 0) {
        if (r0_norms_host) for (int j = 0; j < k; ++j) r0_norms_host[j] = 0.0;
        return BIS_OK;
    }
    bis_status st = bis_ensure_partials(ctx, kPartials);
    if (st == BIS_OK) st = bis_spmm_launch(ctx, m->A, m->X, m->W, k); // init_residual, gmres.hpp
    if (st == BIS_OK) st = mgm_start_cycle(ctx, m, false, tol);
    if (st != BIS_OK) return st;
    m->initialised = true;
    BIS_HIP_CHECK(ctx, hipGetLastError());
    double norms[kMaxK] = {0};
    for (int j = 0; j < k; ++j)
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(&norms[j], m->hist + (size_t)j * m->hist_cap, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BIS_SYNC_CHECK(ctx);
    if (r0_norms_host) for (int j = 0; j < k; ++j) r0_norms_host[j] = norms[j];
    return BIS_OK;
}

bis_status bis_mgmres_iterate(bis_ctx *ctx, bis_mgmres *m, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && n_iters >= 0 && m->enqueued + n_iters < kMaxIters, "bis_mgmres_iterate: bad arguments");
    const int64_t n = m->n;
    const int k = m->k, len = m->m;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, m->initialised, "bis_mgmres_iterate: call bis_mgmres_init first");
    const int g = lockstep_grid(n, k);
    const gmres_layout L{len};
    const int64_t blk = n * k;
    const bool pc = m->pc.type != BIS_PC_NONE;
    bis_status st = bis_ensure_partials(ctx, kPartials);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, m->flags); // the SpMM and the sweeps return at once when every column has stopped
#define BIS_MGM_GS(MODE, CI, VPREV, VNEXT)                                                                                     \
    hipLaunchKernelGGL((mgm_gs_kernel<MODE>), dim3(g), dim3(kT), 0, ctx->stream, n, k, L, pos, CI, m->st, m->flags, m->W,     \
                       (const double *)(VPREV), (const double *)(VNEXT), ctx->partials, kStride, m->counters, m->hist, m->hist_cap)
#define BIS_MGM_COMBINE()                                                                                                      \
    hipLaunchKernelGGL((mgm_combine_kernel<false>), dim3(g), dim3(kT), 0, ctx->stream, n, k, L, (const double *)m->st,        \
                       m->flags, (const double *)m->V, (const double *)m->X, m->X, m->counters + 2 * kCounterSet)
    bool combined = false;
    for (int done = 0; done < n_iters; ++done) {
        const int pos = (m->enqueued + done) % len; // every live column is at this position of its cycle
        st = bis_spmm_launch(ctx, m->A, m->V + pos * blk, m->W, k);
        if (st == BIS_OK && pc) st = bis_pc_apply(ctx, m->pc, m->n, m->k, m->W, m->W);
        if (st != BIS_OK) { m->enqueued += done; return st; }
        BIS_MGM_GS(0, 0, nullptr, m->V);
        for (int i = 1; i <= pos; ++i) BIS_MGM_GS(1, i - 1, m->V + (i - 1) * blk, m->V + i * blk);
        BIS_MGM_GS(2, pos, m->V + pos * blk, nullptr);
        combined = pos + 1 == len;
        if (!combined) {
            hipLaunchKernelGGL(mgm_scale_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, k, L, (const double *)m->st,
                               (const int *)m->flags, (const double *)m->W, m->V + (pos + 1) * blk);
            continue;
        }
        BIS_MGM_COMBINE();                                    // get_explicit_x of check_restart, and of the columns that stopped
        st = bis_spmm_launch(ctx, m->A, m->X, m->W, k);
        if (st == BIS_OK) st = mgm_start_cycle(ctx, m, true, 0.0);
        if (st != BIS_OK) { m->enqueued += done + 1; return st; }
    }
    if (!combined) BIS_MGM_COMBINE(); // a column that stopped inside the cycle: its X is final when this call returns
#undef BIS_MGM_GS
#undef BIS_MGM_COMBINE
    BIS_HIP_CHECK(ctx, hipGetLastError());
    m->enqueued += n_iters;
    return BIS_OK;
}

bis_status bis_mgmres_solution(bis_ctx *ctx, bis_mgmres *m, double *X_out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && (m->n == 0 || X_out), "bis_mgmres_solution: bad arguments");
    BIS_REQUIRE(ctx, X_out != m->X, "bis_mgmres_solution: X_out must not be the solve's X");
    if (m->n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, m->initialised, "bis_mgmres_solution: call bis_mgmres_init first");
    const gmres_layout L{m->m};
    hipLaunchKernelGGL(mgm_ysol_kernel, dim3(1), dim3(64), 0, ctx->stream, m->k, L, m->st, (const int *)m->flags);
    hipLaunchKernelGGL((mgm_combine_kernel<true>), dim3(lockstep_grid(m->n, m->k)), dim3(kT), 0, ctx->stream, m->n, m->k, L,
                       (const double *)m->st, m->flags, (const double *)m->V, (const double *)m->X, X_out, (unsigned *)nullptr);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    BIS_SYNC_CHECK(ctx);
    return BIS_OK;
}

bis_status bis_mgmres_status(bis_ctx *ctx, bis_mgmres *m, int j, int *iters, int *converged, int *n_hist, double *hist_host,
                             int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, m && j >= 0 && j < m->k, "bis_mgmres_status: bad arguments");
    int flags[4] = {0, 0, 0, 0}, ext[4] = {0, 0, 0, 0};
    bis_status st = bis_solver_read_flags(ctx, *m, 4 + 4 * j, 4, flags);
    if (st == BIS_OK) st = bis_solver_read_flags(ctx, *m, 4 + 4 * m->k + 4 * j, 4, ext);
    if (st != BIS_OK) return st;
    const int cnt = std::min(ext[X_NHIST], m->hist_cap);
    if (iters) *iters = flags[0];
    if (converged) *converged = flags[2];
    if (n_hist) *n_hist = cnt;
    if (hist_host && hist_cap > 0) return bis_solver_copy_hist(ctx, *m, j, std::min(cnt, hist_cap), hist_host);
    return BIS_OK;
}

} // extern "C"
