// bis_fgmres.hip -- restarted flexible GMRES(m) (Saad's FGMRES) on one right-hand side as a device schedule: the
// preconditioner stands on the RIGHT and the preconditioned basis Z_n = M_n^-1 V_n is kept, so M_n may differ at every step
// (a K-cycle of bis_mg_*, any inner iteration) and the residual that is minimised, estimated and recorded is the true
// residual || b - A x ||.  The Gram-Schmidt coefficients stay on the device and the Givens / least-squares algebra runs
// there, in one lane of the workgroup that arrives last at a reduction (bis_mgmres.hip's arithmetic on one column).
//   init:     W = b - A x ; hist[0] = ||W|| ; threshold = tol ||W|| ; beta = ||W|| ; g = (beta, 0, ...) ; V_0 = W (1 / beta)
//   position n of a cycle (n = enqueued mod m):
//             Z_n = M^-1 V_n                              bis_apply_preconditioner, straight into block n of Z (BIS_PC_NONE:
//                                                         Z_n IS V_n -- no Z storage, no copy)
//             W = A Z_n                                   bis_spmv
//             h_0 = (W, V_0)                              pass 0
//             W -= h_{i-1} V_{i-1} ; h_i = (W, V_i)       passes 1 .. n   (one fma per element and pass, fma-accumulated dots)
//             W -= h_n V_n ; (W, W)                       pass n + 1; the last workgroup's lane 0: h_{n+1} = sqrt, its inverse;
//                 the stored rotations on (h_0 .. h_n); den = sqrt(a^2 + b^2), c = a / den, s = b / den; column n of the
//                 rotated triangle; g_{n+1} = -s g_n, g_n = c g_n; history entry |g_{n+1}|; the stop test (< threshold,
//                 non-finite, NaN); y by back substitution when the solve stops or the cycle ends (x is then "pending")
//             V_{n+1} = W (1 / h_{n+1})                   scale (not at the end of a cycle: V_m is never read)
//   cycle end (n + 1 == m), or a stop:
//             x_i += sum_{c < steps} y_c Z_c[i]           combine: the sum from 0 over ascending c by fma, then added to x_i;
//                                                         the last workgroup clears the pending flag
//   restart:  W = b - A x ; beta = ||W|| (no apply), ONE MORE history entry and the stop test on it ; V_0 = W (1 / beta)
// The combine also runs at the end of every bis_fgmres_iterate call (it returns at once when nothing is pending), so x is
// final when the call that stopped the solve has enqueued its last kernel.  After the stop every launch of the schedule
// returns at once (the sweeps of a preconditioner do not look at the flag: they may still run, into Z or W, which nothing
// reads any more).  No kernel waits for another workgroup: there is the arrive ticket and nothing else, and the partial sums
// are added in index order, so two runs give the same bits.
// Vectors are walked 16 bytes per lane (double2) in a grid-stride loop, the odd last element by one lane; the blocks of V
// and Z are ld = n rounded up to even apart, so every block starts on 16 bytes.  Grids are the BLAS-1 layer's
// (bis_blas1.hip): one lane per 16 bytes, reductions at most kMaxDotBlocks workgroups, elementwise passes at most 16384.
// Elementwise and reduction traffic at position n, per row: pass 0 reads W, V_0 (16 B), each of the n middle passes reads W,
// V_{i-1}, V_i and writes W (32 B), the last reads W, V_n and writes W (24 B), the scale reads W and writes V_{n+1} (16 B):
// 56 + 32 n bytes, as bis_mgmres_* per column.
#include "bis_gmres_state.hpp"
#include "bis_solver.hpp"

struct bis_fgmres : bis_solver_core { // flags: F_*
    const bis_mat *A = nullptr;
    const double *b = nullptr;
    double *x = nullptr;
    int64_t n = 0, ld = 0;  // ld: distance of two blocks of V / Z (n rounded up to even)
    int m = 0;
    double *V = nullptr;    // m + 1 blocks
    double *Z = nullptr;    // m blocks (null without a preconditioner: Z_n is V_n)
    double *W = nullptr;
    double *st = nullptr;   // the Givens / least-squares state (gmres_layout)
    // counters: three last-arriver counter sets: Gram-Schmidt passes, residual pass, combine
};

namespace {

constexpr int kT = kSolverT;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxDotBlocks); // every pass that arrives runs on bis_pair_grid(n, kMaxDotBlocks)

// flags: iterations, stopped, converged, the iteration of the stop; x awaits its combine, the steps of that combine, history
// entries written, steps done in the current cycle
enum { F_ITERS = 0, F_DONE, F_CONV, F_STOP_IT, F_PENDING, F_STEPS, F_NHIST, F_POS, F_COUNT };

// gmres_book's words: the column's four are the first four flags, its extra four follow
static_assert(F_PENDING == 4 + X_PENDING && F_STEPS == 4 + X_STEPS && F_NHIST == 4 + X_NHIST && F_POS == 4 + X_POS, "flag layout");

// One Gram-Schmidt pass at position pos.  MODE 0: h_0 = (W, V_0) (Vnext = V_0).  MODE 1: W -= h_ci Vprev, h_{ci+1} = (W, Vnext).
// MODE 2: W -= h_ci Vprev, (W, W), and the last workgroup does the bookkeeping (ci = pos).
template <int MODE>
__global__ __launch_bounds__(kT) void fgm_gs_kernel(int64_t n, gmres_layout L, int pos, int ci, double *st, int *flags,
                                                    double *__restrict__ W, const double *__restrict__ Vprev,
                                                    const double *__restrict__ Vnext, double *partials, unsigned *counter,
                                                    double *hist, int hist_cap) {
    __shared__ double lds[kT / 64];
    if (flags[F_DONE]) return;
    const double hc = MODE == 0 ? 0.0 : st[L.h() + ci];
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *W2 = reinterpret_cast<double2 *>(W);
    const double2 *P2 = reinterpret_cast<const double2 *>(Vprev);
    const double2 *N2 = reinterpret_cast<const double2 *>(Vnext);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 w = W2[i];
        if (MODE != 0) {
            const double2 p = P2[i];
            w.x = fma(-hc, p.x, w.x);
            w.y = fma(-hc, p.y, w.y);
            W2[i] = w;
        }
        if (MODE == 2) {
            acc = fma(w.x, w.x, acc);
            acc = fma(w.y, w.y, acc);
        } else {
            const double2 q = N2[i];
            acc = fma(w.x, q.x, acc);
            acc = fma(w.y, q.y, acc);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double w = W[n - 1];
        if (MODE != 0) {
            w = fma(-hc, Vprev[n - 1], w);
            W[n - 1] = w;
        }
        acc = fma(w, MODE == 2 ? w : Vnext[n - 1], acc);
    }
    const double sums[1] = {acc};
    double total[1];
    if (!reduce_last<1>(sums, lds, partials, counter, total)) return;
    // every other workgroup has read its coefficient and the flags before it arrived: they may change now
    if (threadIdx.x != 0) return;
    if (MODE == 2) gmres_book(L, total[0], pos, st, flags, flags + 4, hist, hist_cap);
    else st[L.h() + (MODE == 0 ? 0 : ci + 1)] = total[0];
}

// Start of the solve (INIT) and of every later cycle: W = b - W (W holds A x), (W, W), and the last workgroup's
// bookkeeping -- INIT: the state and the flags cleared, history entry 0, the threshold; both: beta, g, 1 / beta; a restart: the
// extra history entry and the stop test on beta.
template <bool INIT>
__global__ __launch_bounds__(kT) void fgm_resid_kernel(int64_t n, gmres_layout L, double tol, double *st, int *flags,
                                                       const double *__restrict__ b, double *__restrict__ W, double *partials,
                                                       unsigned *counter, double *hist, int hist_cap) {
    __shared__ double lds[kT / 64];
    if (!INIT && flags[F_DONE]) return;
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *W2 = reinterpret_cast<double2 *>(W);
    const double2 *b2 = reinterpret_cast<const double2 *>(b);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 bv = b2[i], av = W2[i];
        double2 r;
        r.x = bv.x - av.x;
        r.y = bv.y - av.y;
        W2[i] = r;
        acc = fma(r.x, r.x, acc);
        acc = fma(r.y, r.y, acc);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double r = b[n - 1] - W[n - 1];
        W[n - 1] = r;
        acc = fma(r, r, acc);
    }
    const double sums[1] = {acc};
    double total[1];
    if (!reduce_last<1>(sums, lds, partials, counter, total)) return;
    if (threadIdx.x != 0) return;
    const double norm = sqrt(total[0]);
    if (INIT) {
        for (int q = 0; q < L.size(); ++q) st[q] = 0.0;
        for (int q = 0; q < F_COUNT; ++q) flags[q] = 0;
        hist[0] = norm;
        st[L.stop()] = tol * norm;
        flags[F_NHIST] = 1;
    }
    st[L.beta()] = norm;
    st[L.g()] = norm;
    st[L.inv()] = 1.0 / norm;
    flags[F_POS] = 0;
    if (!INIT) {
        const int nh = flags[F_NHIST];
        if (nh < hist_cap) hist[nh] = norm;
        flags[F_NHIST] = nh + 1;
        const bool conv = norm < st[L.stop()];
        const bool diverged = norm > DBL_MAX || norm != norm;
        if (conv || diverged) { flags[F_DONE] = 1; flags[F_CONV] = conv ? 1 : 0; flags[F_STOP_IT] = flags[F_ITERS]; }
    }
}

// Vdst = W (1 / norm)
__global__ __launch_bounds__(kT) void fgm_scale_kernel(int64_t n, gmres_layout L, const double *__restrict__ st,
                                                       const int *__restrict__ flags, const double *__restrict__ W,
                                                       double *__restrict__ Vdst) {
    if (flags[F_DONE]) return;
    const double inv = st[L.inv()];
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *W2 = reinterpret_cast<const double2 *>(W);
    double2 *V2 = reinterpret_cast<double2 *>(Vdst);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 w = W2[i];
        w.x *= inv;
        w.y *= inv;
        V2[i] = w;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) Vdst[n - 1] = W[n - 1] * inv;
}

// x += sum_{c < steps} y_c Z_c when x is pending (a cycle ended, or the solve stopped), in one pass over the steps blocks;
// the last workgroup clears the pending flag.  SOL: OUT = X + the sum over the steps of the current cycle with the y of
// fgm_ysol_kernel while the solve is live, OUT = X once it has stopped; nothing of the handle changes.
template <bool SOL>
__global__ __launch_bounds__(kT) void fgm_combine_kernel(int64_t n, int64_t ld, gmres_layout L, const double *st, int *flags,
                                                         const double *__restrict__ Z, const double *X, double *OUT,
                                                         unsigned *counter) {
    __shared__ double ys[kMaxRestart];
    if (!SOL && !flags[F_PENDING]) return; // nothing to add: every launch behind the stop's own combine ends here
    const int steps = SOL ? (flags[F_DONE] ? 0 : flags[F_POS]) : flags[F_STEPS];
    if ((int)threadIdx.x < steps) ys[threadIdx.x] = st[(SOL ? L.ysol() : L.y()) + threadIdx.x];
    __syncthreads();
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *Z2 = reinterpret_cast<const double2 *>(Z);
    const double2 *X2 = reinterpret_cast<const double2 *>(X);
    double2 *O2 = reinterpret_cast<double2 *>(OUT);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 acc = make_double2(0.0, 0.0);
        for (int c = 0; c < steps; ++c) {
            const double2 z = Z2[(int64_t)c * ld2 + i];
            acc.x = fma(z.x, ys[c], acc.x);
            acc.y = fma(z.y, ys[c], acc.y);
        }
        double2 xv = X2[i];
        if (steps > 0) { xv.x += acc.x; xv.y += acc.y; }
        O2[i] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double acc = 0.0;
        for (int c = 0; c < steps; ++c) acc = fma(Z[(int64_t)c * ld + n - 1], ys[c], acc);
        OUT[n - 1] = steps > 0 ? X[n - 1] + acc : X[n - 1];
    }
    if (SOL) return;
    // every workgroup has read the pending flag, the steps and the y before it arrives
    if (threadIdx.x == 0 && arrive_last_set(counter, blockIdx.x, gridDim.x)) flags[F_PENDING] = 0;
}

// the y of a live solve at its current position, for bis_fgmres_solution: into the state's ysol
__global__ void fgm_ysol_kernel(gmres_layout L, double *st, const int *flags) {
    if (threadIdx.x != 0 || flags[F_DONE]) return;
    gmres_backsub(L, st, flags[F_POS], st + L.ysol());
}

} // namespace

extern "C" {

bis_status bis_fgmres_create(bis_ctx *ctx, const bis_mat *A, const double *b, double *x, int restart_len, bis_fgmres **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && b && x && out, "bis_fgmres_create: bad arguments");
    BIS_REQUIRE(ctx, restart_len >= 1 && restart_len <= kMaxRestart, "bis_fgmres_create: restart_len must be between 1 and 64");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_fgmres_create: square matrix required");
    BIS_REQUIRE(ctx, aligned16(b) && aligned16(x), "bis_fgmres_create: b and x must be 16-byte aligned");
    bis_fgmres *s = new bis_fgmres;
    s->A = A; s->b = b; s->x = x;
    s->n = A->n_rows;
    s->ld = (s->n + 1) & ~(int64_t)1;
    s->m = restart_len;
    const gmres_layout L{restart_len};
    bis_status st = bis_vec_alloc(ctx, s->ld * (restart_len + 1), &s->V);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, s->ld, &s->W);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, L.size(), &s->st);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, s, F_COUNT, 1, 3, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st != BIS_OK) { bis_fgmres_destroy(ctx, s); return st; }
    *out = s;
    return BIS_OK;
}

bis_status bis_fgmres_set_preconditioner(bis_ctx *ctx, bis_fgmres *s, int precond_type, const bis_mat *L_strict,
                                         const bis_mat *U_strict, const double *A_D, const double *A_D_inv, const double *L_D,
                                         const double *U_D, int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (!s) return bis_pc_no_handle(ctx, "bis_fgmres", 0, precond_type);
    return bis_pc_bind(ctx, &s->pc, {"bis_fgmres", s->n, s->ld, 0, bis_solver_live(*s), 0},
                       {precond_type, L_strict, U_strict, A_D, A_D_inv, L_D, U_D, outer_iters, inner_iters},
                       {{&s->Z, s->ld * s->m, precond_type != BIS_PC_NONE && !s->Z}});
}

bis_status bis_fgmres_destroy(bis_ctx *ctx, bis_fgmres *s) {
    BIS_CTX_OK(ctx);
    if (!s) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *v : {s->V, s->Z, s->W, s->st}) hipFree(v);
    bis_solver_core_free(s);
    delete s;
    return BIS_OK;
}

// W holds A x: the residual, its norm and the bookkeeping, then V_0
static void fgm_start_cycle(bis_ctx *ctx, bis_fgmres *s, bool restart, double tol) {
    const int64_t n = s->n;
    const gmres_layout L{s->m};
    const int g = bis_pair_grid(n, kMaxDotBlocks);
    unsigned *counter = s->counters + kCounterSet;
    if (restart)
        hipLaunchKernelGGL((fgm_resid_kernel<false>), dim3(g), dim3(kT), 0, ctx->stream, n, L, tol, s->st, s->flags, s->b, s->W,
                           ctx->partials, counter, s->hist, s->hist_cap);
    else
        hipLaunchKernelGGL((fgm_resid_kernel<true>), dim3(g), dim3(kT), 0, ctx->stream, n, L, tol, s->st, s->flags, s->b, s->W,
                           ctx->partials, counter, s->hist, s->hist_cap);
    hipLaunchKernelGGL(fgm_scale_kernel, dim3(bis_pair_grid(n, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, n, L, (const double *)s->st,
                       (const int *)s->flags, (const double *)s->W, s->V);
}

bis_status bis_fgmres_init(bis_ctx *ctx, bis_fgmres *s, double tol, double *r0_norm_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_fgmres_init: null handle");
    s->enqueued = 0;
    if (s->n == 0) {
        if (r0_norm_host) *r0_norm_host = 0.0;
        return BIS_OK;
    }
    bis_status st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st == BIS_OK) st = bis_spmv_launch(ctx, s->A, s->x, s->W, nullptr, nullptr);
    if (st != BIS_OK) return st;
    fgm_start_cycle(ctx, s, false, tol);
    s->initialised = true;
    BIS_HIP_CHECK(ctx, hipGetLastError());
    double norm = 0.0;
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&norm, s->hist, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BIS_SYNC_CHECK(ctx);
    if (r0_norm_host) *r0_norm_host = norm;
    return BIS_OK;
}

bis_status bis_fgmres_iterate(bis_ctx *ctx, bis_fgmres *s, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && n_iters >= 0 && s->enqueued + n_iters < kMaxIters, "bis_fgmres_iterate: bad arguments");
    const int64_t n = s->n, ld = s->ld;
    const int len = s->m;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, s->initialised, "bis_fgmres_iterate: call bis_fgmres_init first");
    const int g = bis_pair_grid(n, kMaxDotBlocks), g_wide = bis_pair_grid(n, kMaxEwBlocks);
    const gmres_layout L{len};
    const bool pc = s->pc.type != BIS_PC_NONE;
    bis_status st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, s->flags); // the SpMV returns at once when the solve has stopped
#define BIS_FGM_GS(MODE, CI, VPREV, VNEXT)                                                                                     \
    hipLaunchKernelGGL((fgm_gs_kernel<MODE>), dim3(g), dim3(kT), 0, ctx->stream, n, L, pos, CI, s->st, s->flags, s->W,        \
                       (const double *)(VPREV), (const double *)(VNEXT), ctx->partials, s->counters, s->hist, s->hist_cap)
#define BIS_FGM_COMBINE()                                                                                                      \
    hipLaunchKernelGGL((fgm_combine_kernel<false>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, L, (const double *)s->st,       \
                       s->flags, (const double *)(pc ? s->Z : s->V), (const double *)s->x, s->x, s->counters + 2 * kCounterSet)
    bool combined = false;
    for (int done = 0; done < n_iters; ++done) {
        const int pos = (s->enqueued + done) % len;
        double *Vn = s->V + pos * ld, *Zn = Vn;
        if (pc) { // Z_n = M^-1 V_n; V_n must survive: outer_iters > 1 writes its input (and puts it back), so it gets a copy
            Zn = s->Z + pos * ld;
            double *in = Vn;
            if (s->pc.outer > 1) {
                st = bis_copy_vector(ctx, s->W, Vn, n);
                in = s->W;
            }
            if (st == BIS_OK) st = bis_pc_apply(ctx, s->pc, n, 0, Zn, in);
        }
        if (st == BIS_OK) st = bis_spmv_launch(ctx, s->A, Zn, s->W, nullptr, nullptr);
        if (st != BIS_OK) { s->enqueued += done; return st; }
        BIS_FGM_GS(0, 0, nullptr, s->V);
        for (int i = 1; i <= pos; ++i) BIS_FGM_GS(1, i - 1, s->V + (i - 1) * ld, s->V + i * ld);
        BIS_FGM_GS(2, pos, Vn, nullptr);
        combined = pos + 1 == len;
        if (!combined) {
            hipLaunchKernelGGL(fgm_scale_kernel, dim3(g_wide), dim3(kT), 0, ctx->stream, n, L, (const double *)s->st,
                               (const int *)s->flags, (const double *)s->W, s->V + (pos + 1) * ld);
            continue;
        }
        BIS_FGM_COMBINE();
        st = bis_spmv_launch(ctx, s->A, s->x, s->W, nullptr, nullptr);
        if (st != BIS_OK) { s->enqueued += done + 1; return st; }
        fgm_start_cycle(ctx, s, true, 0.0);
    }
    if (!combined) BIS_FGM_COMBINE(); // a stop inside the cycle: x is final when this call returns
#undef BIS_FGM_GS
#undef BIS_FGM_COMBINE
    BIS_HIP_CHECK(ctx, hipGetLastError());
    s->enqueued += n_iters;
    return BIS_OK;
}

bis_status bis_fgmres_solution(bis_ctx *ctx, bis_fgmres *s, double *x_out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && (s->n == 0 || x_out), "bis_fgmres_solution: bad arguments");
    BIS_REQUIRE(ctx, x_out != s->x, "bis_fgmres_solution: x_out must not be the solve's x");
    if (s->n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, aligned16(x_out), "bis_fgmres_solution: x_out must be 16-byte aligned");
    BIS_REQUIRE(ctx, s->initialised, "bis_fgmres_solution: call bis_fgmres_init first");
    const gmres_layout L{s->m};
    hipLaunchKernelGGL(fgm_ysol_kernel, dim3(1), dim3(64), 0, ctx->stream, L, s->st, (const int *)s->flags);
    hipLaunchKernelGGL((fgm_combine_kernel<true>), dim3(bis_pair_grid(s->n, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, s->n, s->ld, L,
                       (const double *)s->st, s->flags, (const double *)(s->pc.type != BIS_PC_NONE ? s->Z : s->V), (const double *)s->x,
                       x_out, (unsigned *)nullptr);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    BIS_SYNC_CHECK(ctx);
    return BIS_OK;
}

bis_status bis_fgmres_status(bis_ctx *ctx, bis_fgmres *s, int *iters, int *converged, int *n_hist, double *hist_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_fgmres_status: null handle");
    int flags[F_COUNT] = {0};
    if (bis_status st = bis_solver_read_flags(ctx, *s, 0, F_COUNT, flags)) return st;
    const int cnt = std::min(flags[F_NHIST], s->hist_cap);
    if (iters) *iters = flags[F_ITERS];
    if (converged) *converged = flags[F_CONV];
    if (n_hist) *n_hist = cnt;
    if (hist_host && hist_cap > 0) return bis_solver_copy_hist(ctx, *s, 0, std::min(cnt, hist_cap), hist_host);
    return BIS_OK;
}

} // extern "C"
