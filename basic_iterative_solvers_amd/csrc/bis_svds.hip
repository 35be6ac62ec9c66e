// bis_svds.hip -- Golub-Kahan-Lanczos bidiagonalisation with thick restart and full re-orthogonalisation for the k largest or
// smallest singular triplets of a rectangular matrix, as a sync-free device schedule of the kind bis_eigs.hip is.
// include/bis_hip.h states the algorithm line by line; here is how it is laid out.  F is the tall orientation of A (A itself
// when rows >= cols, A^T otherwise).  Two bases: P_0 .. P_m of ns = min(rows, cols) entries and Q_0 .. Q_{m-1} of nl =
// max(rows, cols), each with its own leading dimension (the length rounded up to even).  No work vector: a product writes
// into its destination block W (Q_j in the left half of step j, P_{j+1} in the right half), which is orthogonalised against
// the nb blocks before it in the same basis (j in the left half, j + 1 in the right) and scaled in place.  The passes over
// n-vectors are bis_lanczos.hpp's, shared with bis_eigs.hip:
//     W = F P_j  or  F^T Q_j                  bis_spmv_launch on A or At, or the caller between op_begin / op_end
//     h = B_{0..nb)^T W                       lanczos_dots_kernel, one launch per group of at most 8 blocks: W is read once per group
//     W -= B_{0..nb) h                        lanczos_update_kernel<false>: one launch, one fma per element and block, ascending
//     h = B_{0..nb)^T W                       lanczos_dots_kernel again
//     W -= B_{0..nb) h                        lanczos_update_kernel<true>: (W, W) fused; the last workgroup's lane 0 (svds_close):
//                                             alpha_j or beta_j = sqrt((W, W)), the product count, the breakdown test
//     W = W / alpha_j  or  W / beta_j         lanczos_scale_kernel, in place
//     svds_restart_kernel (one wave), lanczos_compress_kernel on P and on Q: they act when the cycle closes (the right half
//     of j = m - 1, known on the host) or when the update before them met a breakdown (flags[6], known on the device only);
//     otherwise they return at once.
// With j = 0 the left half has nothing to orthogonalise against: one lanczos_update_kernel<true> launch sums the norm.
// The restart kernel is one wave: G (B rotated into X Sigma) and Y, 64 x 65 doubles each, sit in LDS, column c of either at
// [c * 65 + r]; the one-sided Jacobi sweeps walk a round-robin schedule, one lane per pair of columns, so the m_eff / 2 pairs of
// a round rotate at once and the lanes' column-strided accesses fall into different banks.  The compressions work in place,
// row by row, 8 bytes per lane (a lane holds a row of up to 64 blocks).
// After a stop every launch returns at once (the products through bis_stop_guard).
#include "bis_lanczos.hpp"

// flags: bis_lanczos.hpp, and [10] 1 + the block of Q that counts as 0 (an alpha breakdown)
struct bis_svds : bis_lanczos_core {
    const bis_mat *A = nullptr, *At = nullptr; // both null: the caller applies the products
    bis_mat *At_owned = nullptr;                // bis_mat_transpose(A) when the caller passed none
    int64_t rows = 0, cols = 0, ns = 0, nl = 0, ldp = 0, ldq = 0;
    bool flip = false;   // rows < cols: F = A^T
    double *P = nullptr; // m + 1 blocks of ldp
    double *Q = nullptr; // m blocks of ldq
    int half = 0;        // 0: the next product is F P_j, 1: F^T Q_j
};

namespace {

enum { S_ALPHA = 0, S_BETA = kM, S_SIGMA = 2 * kM, S_S = 3 * kM, S_H = 4 * kM, S_VAL = 5 * kM, S_EST = 6 * kM,
       S_TOL = 7 * kM, S_NRM0, S_WW0 /* (W, W) before the passes */, S_SREF, S_Y = 8 * kM /* Y_keep, row b at S_Y + kM b */,
       S_X = S_Y + kM * kM /* X_keep */, S_COUNT = S_X + kM * kM };

// how lanczos_update_kernel<true> closes a half step: ww = (W, W) after the passes; half = 0 forms alpha_j, half = 1 beta_j
struct svds_close {
    double *sc;
    int *flags;
    int j, half, nb;
    __device__ void operator()(double ww) const {
        double nrm = sqrt(ww);
        // the norm before the passes; without passes (the left half of step 0) it is the norm itself
        const double before = nb ? sqrt(sc[S_WW0]) : nrm;
        // a breakdown: the norm is 0, or the rounding noise that two passes leave of it.  No reciprocal: the restart launch
        // behind this half step closes the cycle at j + 1.
        const bool invariant = nrm <= DBL_EPSILON * before;
        if (invariant) nrm = 0.0;
        sc[(half ? S_BETA : S_ALPHA) + j] = nrm;
        if (!half && invariant) sc[S_BETA + j] = 0.0; // (an earlier cycle's beta_j)
        flags[0] += 1;
        if (invariant) {
            flags[1] = 1;
            flags[6] = j + 1;
            flags[10] = half ? 0 : j + 1;
        }
    }
};

// The restart: one wave.  close: the cycle closes here with m_eff = m (the host knows); otherwise the launch acts only on a
// breakdown (flags[6] = m_eff).  l_in: the triplets kept by the restart before (0 in the first cycle); l_keep: the triplets a
// restart keeps.  G(r, c) at G[c * kLd + r], Y(r, c) at Y[c * kLd + r]: a lane walks its pair's two columns.
__global__ __launch_bounds__(64) void svds_restart_kernel(double *sc, int *flags, int close, int m, int l_in, int l_keep, int k,
                                                          int which, double *hist, int hist_cap) {
#pragma clang fp contract(off)
    __shared__ double G[kM * kLd], Y[kM * kLd]; // kLd: the lanes' columns fall into different banks
    __shared__ double sig[kM], key[kM];
    __shared__ int order[kM], rank[kM], rotated[kM];
    const int lane = threadIdx.x;
    const int pending = flags[6];
    if (!pending && (flags[1] || !close)) {
        if (lane == 0) flags[7] = 0;
        return;
    }
    const int me = pending ? pending : m; // m_eff
    // ---- B ----
    if (lane < me)
        for (int r = 0; r < me; ++r) { G[lane * kLd + r] = 0.0; Y[lane * kLd + r] = r == lane ? 1.0 : 0.0; }
    __syncthreads();
    if (lane < me) {
        if (lane < l_in) {
            G[lane * kLd + lane] = sc[S_SIGMA + lane];
            G[l_in * kLd + lane] = sc[S_S + lane];
        } else {
            G[lane * kLd + lane] = sc[S_ALPHA + lane];
            if (lane + 1 < me) G[(lane + 1) * kLd + lane] = sc[S_BETA + lane];
        }
    }
    __syncthreads();
    const double beta_last = sc[S_BETA + me - 1];
    // eps ||B||_F: column sums of squares in row order, added in column order
    {
        double a = 0.0;
        if (lane < me)
            for (int r = 0; r < me; ++r) a += G[lane * kLd + r] * G[lane * kLd + r];
        sig[lane] = a;
    }
    __syncthreads();
    double floor_ = 0.0;
    for (int c = 0; c < me; ++c) floor_ += sig[c];
    floor_ = DBL_EPSILON * sqrt(floor_);
    __syncthreads();
    // ---- one-sided Jacobi, round-robin ----
    const int n2 = (me + 1) & ~1, n1 = n2 - 1;
    const double thr = sqrt((double)me) * DBL_EPSILON;
    bool finished = false;
    for (int sweep = 0; sweep < kMaxSweeps && !finished; ++sweep) {
        int rot = 0;
        for (int r = 0; r < n1; ++r) {
            if (lane < n2 / 2) {
                const int x = lane == 0 ? n1 : (r + lane) % n1, y = lane == 0 ? r : (r - lane + n1) % n1;
                const int p = min(x, y), q = max(x, y);
                if (q < me) {
                    double *gp = G + p * kLd, *gq = G + q * kLd;
                    double a = 0.0, b = 0.0, c = 0.0;
                    for (int i = 0; i < me; ++i) {
                        const double u = gp[i], v = gq[i];
                        a += u * u; b += v * v; c += u * v;
                    }
                    if (c != 0.0 && fabs(c) > thr * sqrt(a) * sqrt(b) && sqrt(a) > floor_ && sqrt(b) > floor_) {
                        const double zeta = (b - a) / (2.0 * c);
                        const double root = sqrt(1.0 + zeta * zeta);
                        const double t = 1.0 / (zeta >= 0.0 ? zeta + root : zeta - root);
                        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
                        double *yp = Y + p * kLd, *yq = Y + q * kLd;
                        for (int i = 0; i < me; ++i) {
                            const double u = gp[i], v = gq[i];
                            gp[i] = cs * u - sn * v;
                            gq[i] = sn * u + cs * v;
                            const double e = yp[i], f = yq[i];
                            yp[i] = cs * e - sn * f;
                            yq[i] = sn * e + cs * f;
                        }
                        rot = 1;
                    }
                }
            }
            __syncthreads();
        }
        rotated[lane] = rot;
        __syncthreads();
        int any = 0;
        for (int i = 0; i < 64; ++i) any |= rotated[i];
        __syncthreads();
        if (!any) finished = true;
    }
    // ---- sigma_i = ||g_i||, x_i = g_i / sigma_i (G becomes X) ----
    if (lane < me) {
        double *g = G + lane * kLd;
        double a = 0.0;
        for (int i = 0; i < me; ++i) a += g[i] * g[i];
        double s = sqrt(a);
        if (!(s > floor_)) s = 0.0; // the rounding noise of a zero singular value is a zero column
        sig[lane] = s;
        for (int i = 0; i < me; ++i) g[i] = s != 0.0 ? g[i] / s : 0.0;
    }
    __syncthreads();
    // ---- order, estimates, the test: lane 0 ----
    const int n_ranked = min(k, me);
    if (lane == 0) {
        for (int i = 0; i < me; ++i) order[i] = i;
        lanczos_sort(order, sig, me); // ascending, stable
        for (int i = 0; i < me; ++i) key[i] = which == 1 ? 0.0 : -sig[order[i]];
        int pos[kM];
        for (int i = 0; i < me; ++i) pos[i] = i;
        if (which != 1) lanczos_sort(pos, key, me);
        for (int i = 0; i < me; ++i) rank[i] = order[pos[i]]; // the column of X and Y of rank i
        const double sref = fmax(sc[S_SREF], sig[order[me - 1]]);
        sc[S_SREF] = sref;
        const double tol = sc[S_TOL];
        double worst = 0.0;
        int nconv = 0;
        for (int i = 0; i < n_ranked; ++i) {
            const double est = fabs(beta_last * G[rank[i] * kLd + me - 1]);
            sc[S_VAL + i] = sig[rank[i]];
            sc[S_EST + i] = est;
            worst = fmax(worst, est);
            if (est <= tol * sref) ++nconv;
        }
        key[0] = lanczos_verdict(flags, hist, hist_cap, pending, finished, nconv, worst, k, me, l_keep) ? 1.0 : 0.0;
    }
    __syncthreads();
    const bool stop = key[0] != 0.0;
    const int l_out = stop ? n_ranked : l_keep;
    // Y_keep and X_keep (me x l_out), and the state of the next cycle
    if (lane < l_out) {
        const int col = rank[lane];
        if (!stop) {
            sc[S_SIGMA + lane] = sig[col];
            sc[S_S + lane] = beta_last * G[col * kLd + me - 1];
        }
        for (int b = 0; b < me; ++b) {
            sc[S_Y + kM * b + lane] = Y[col * kLd + b];
            sc[S_X + kM * b + lane] = G[col * kLd + b];
        }
    }
}

// what follows a product: the rest of the half step, and the restart when the cycle closes
void svds_enqueue_half(bis_ctx *ctx, bis_svds *s) {
    const int j = s->j, half = s->half;
    const int64_t n = half ? s->ns : s->nl, ld = half ? s->ldp : s->ldq;
    double *B = half ? s->P : s->Q;
    double *W = B + (int64_t)(half ? j + 1 : j) * ld;
    const int nb = half ? j + 1 : j;
    const int *flags = s->flags;
    // both passes leave their coefficients in h; the block is scaled in place
    lanczos_enqueue_passes(ctx, s, n, ld, B, nb, W, s->sc + S_H, s->sc + S_H, s->sc + S_WW0, svds_close{s->sc, s->flags, j, half, nb},
                           s->sc + (half ? S_BETA : S_ALPHA) + j, W);
    const int close = half && j == s->m - 1;
    hipLaunchKernelGGL(svds_restart_kernel, dim3(1), dim3(64), 0, ctx->stream, s->sc, s->flags, close, s->m, s->l_cur, s->l, s->k,
                       s->which, s->hist, s->hist_cap);
    // P: Y_keep, and P_m moves to P_l at a restart; Q: X_keep, and the block of an alpha breakdown counts as 0
    hipLaunchKernelGGL(lanczos_compress_kernel<false>, dim3(lane_grid(s->ns)), dim3(kT), 0, ctx->stream, s->ns, s->ldp, flags,
                       (const double *)(s->sc + S_Y), s->P);
    hipLaunchKernelGGL(lanczos_compress_kernel<true>, dim3(lane_grid(s->nl)), dim3(kT), 0, ctx->stream, s->nl, s->ldq, flags,
                       (const double *)(s->sc + S_X), s->Q);
    if (!half) {
        s->half = 1;
    } else {
        s->half = 0;
        if (close) {
            s->j = s->l;
            s->l_cur = s->l;
        } else {
            s->j = j + 1;
        }
    }
    s->enqueued += 1;
}

// the operands of the next product: in, out and whether it is A^T's (in terms of the caller's A)
inline void svds_next_product(const bis_svds *s, const double **in, double **out, int *transposed) {
    if (s->half == 0) {
        *in = s->P + (int64_t)s->j * s->ldp;
        *out = s->Q + (int64_t)s->j * s->ldq;
    } else {
        *in = s->Q + (int64_t)s->j * s->ldq;
        *out = s->P + (int64_t)(s->j + 1) * s->ldp;
    }
    *transposed = s->half ^ (s->flip ? 1 : 0);
}

} // namespace

extern "C" {

bis_status bis_svds_create(bis_ctx *ctx, const bis_mat *A, const bis_mat *At, int64_t rows, int64_t cols, int k, int ncv,
                           int which, bis_svds **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, out, "bis_svds_create: bad arguments");
    BIS_REQUIRE(ctx, A || !At, "bis_svds_create: At without A");
    BIS_REQUIRE(ctx, !A || (A->n_rows == rows && A->n_cols == cols), "bis_svds_create: rows and cols must be the shape of A");
    BIS_REQUIRE(ctx, !A || !A->view, "bis_svds_create: a row-range view is not an operand");
    BIS_REQUIRE(ctx, !At || (At->n_rows == cols && At->n_cols == rows && At->nnz == A->nnz && !At->view),
                "bis_svds_create: At must be the transpose of A (cols x rows, as many entries)");
    const int64_t ns = std::min(rows, cols), nl = std::max(rows, cols);
    BIS_REQUIRE(ctx, ns >= 2, "bis_svds_create: min(rows, cols) must be at least 2");
    BIS_REQUIRE(ctx, k >= 1, "bis_svds_create: k must be at least 1");
    BIS_REQUIRE(ctx, which == BIS_SVDS_LM || which == BIS_SVDS_SM, "bis_svds_create: which must be BIS_SVDS_LM or BIS_SVDS_SM");
    const int64_t cap = std::min<int64_t>(ns, kM);
    if (ncv == 0) ncv = (int)std::min<int64_t>(cap, std::max(2 * k + 1, 20));
    BIS_REQUIRE(ctx, ncv > k, "bis_svds_create: ncv must exceed k (k < ncv <= min(rows, cols, 64))");
    BIS_REQUIRE(ctx, ncv <= cap, "bis_svds_create: ncv must not exceed min(rows, cols, 64) (k < ncv <= min(rows, cols, 64))");
    bis_svds *s = new bis_svds;
    s->A = A;
    s->At = At;
    s->rows = rows;
    s->cols = cols;
    s->ns = ns;
    s->nl = nl;
    s->flip = rows < cols;
    s->ldp = (ns + 1) & ~(int64_t)1;
    s->ldq = (nl + 1) & ~(int64_t)1;
    s->k = k;
    s->m = ncv;
    s->l = std::min(k + (ncv - k) / 2, ncv - 1);
    s->which = which;
    bis_status st = BIS_OK;
    if (A && !At) {
        st = bis_mat_transpose(ctx, A, &s->At_owned);
        s->At = s->At_owned;
    }
    if (st == BIS_OK) st = bis_vec_alloc(ctx, s->ldp * (s->m + 1), &s->P);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, s->ldq * s->m, &s->Q);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, S_COUNT, &s->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, s, kFlags, 2, 1, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) { bis_svds_destroy(ctx, s); return st; }
    *out = s;
    return BIS_OK;
}

bis_status bis_svds_set_start(bis_ctx *ctx, bis_svds *s, const double *v0) {
    return lanczos_set_start(ctx, s, v0, "bis_svds");
}

bis_status bis_svds_destroy(bis_ctx *ctx, bis_svds *s) {
    BIS_CTX_OK(ctx);
    if (!s) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *p : {s->P, s->Q, s->sc}) hipFree(p);
    if (s->At_owned) bis_mat_destroy(ctx, s->At_owned);
    bis_solver_core_free(s);
    delete s;
    return BIS_OK;
}

bis_status bis_svds_init(bis_ctx *ctx, bis_svds *s, double tol) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_svds_init: null handle");
    s->half = 0;
    // every earlier state goes: both bases and scalars here, the rest in lanczos_init
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->P, 0, sizeof(double) * (size_t)s->ldp * (s->m + 1), ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->Q, 0, sizeof(double) * (size_t)s->ldq * s->m, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->sc, 0, sizeof(double) * S_COUNT, ctx->stream));
    return lanczos_init(ctx, s, s->ns, s->ldp, s->P, s->P, tol, S_TOL, S_NRM0); // P_0 is scaled in place
}

bis_status bis_svds_op_begin(bis_ctx *ctx, bis_svds *s, const double **in_dev, double **out_dev, int *transposed) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && in_dev && out_dev && transposed, "bis_svds_op_begin: bad arguments");
    BIS_REQUIRE(ctx, s->initialised, "bis_svds_op_begin: call bis_svds_init first");
    BIS_REQUIRE(ctx, !s->op_open, "bis_svds_op_begin: the product before it was not closed with bis_svds_op_end");
    BIS_REQUIRE(ctx, s->enqueued + 1 < kMaxIters, "bis_svds_op_begin: too many products since bis_svds_init");
    s->op_open = true;
    svds_next_product(s, in_dev, out_dev, transposed);
    return BIS_OK;
}

bis_status bis_svds_op_end(bis_ctx *ctx, bis_svds *s) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_svds_op_end: null handle");
    BIS_REQUIRE(ctx, s->op_open, "bis_svds_op_end: call bis_svds_op_begin first");
    s->op_open = false;
    if (bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks)) return st;
    svds_enqueue_half(ctx, s);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_svds_iterate(bis_ctx *ctx, bis_svds *s, int n_cycles) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && n_cycles >= 0, "bis_svds_iterate: bad arguments");
    BIS_REQUIRE(ctx, s->A, "bis_svds_iterate: the handle has no matrix (caller-applied operator): use bis_svds_op_begin / bis_svds_op_end");
    BIS_REQUIRE(ctx, s->initialised, "bis_svds_iterate: call bis_svds_init first");
    BIS_REQUIRE(ctx, !s->op_open, "bis_svds_iterate: a product is open: call bis_svds_op_end first");
    BIS_REQUIRE(ctx, (int64_t)s->enqueued + (int64_t)n_cycles * 2 * s->m < kMaxIters, "bis_svds_iterate: too many products since bis_svds_init");
    if (bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks)) return st;
    bis_stop_guard stop_guard(ctx, s->flags); // the products return at once when the solve has stopped
    for (int cycle = 0; cycle < n_cycles; ++cycle) {
        do { // to the end of the cycle the handle is in
            const double *in = nullptr;
            double *out = nullptr;
            int transposed = 0;
            svds_next_product(s, &in, &out, &transposed);
            if (bis_status st = bis_spmv_launch(ctx, transposed ? s->At : s->A, in, out, nullptr, nullptr)) return st;
            svds_enqueue_half(ctx, s);
        } while (s->half != 0 || s->j != s->l_cur || s->l_cur == 0);
    }
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_svds_status(bis_ctx *ctx, bis_svds *s, int *products, int *restarts, int *stopped, int *converged, int *reason,
                           int *nconv, double *sigma_ref, double *values_host, double *est_host, double *hist_host,
                           double *hist_nconv_host, int hist_cap) {
    if (bis_status st = lanczos_status(ctx, s, "bis_svds", products, restarts, stopped, converged, reason, nconv, S_VAL, values_host,
                                       S_EST, est_host, hist_host, hist_nconv_host, hist_cap))
        return st;
    if (sigma_ref) BIS_HIP_CHECK(ctx, hipMemcpy(sigma_ref, s->sc + S_SREF, sizeof(double), hipMemcpyDeviceToHost));
    return BIS_OK;
}

bis_status bis_svds_vectors(bis_ctx *ctx, bis_svds *s, double *U, int64_t ldu, double *V, int64_t ldv) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_svds_vectors: null handle");
    BIS_REQUIRE(ctx, (!U || ldu >= s->rows) && (!V || ldv >= s->cols), "bis_svds_vectors: bad arguments (ldu >= rows, ldv >= cols)");
    int restarts = 0;
    if (bis_status st = bis_solver_read_flags(ctx, *s, 3, 1, &restarts)) return st;
    BIS_REQUIRE(ctx, s->initialised && restarts >= 1, "bis_svds_vectors: no restart yet: the bases hold no singular vectors");
    // the left vectors have `rows` entries: Q's when A is F, P's when A is F^T
    const double *left = s->flip ? s->P : s->Q, *right = s->flip ? s->Q : s->P;
    const int64_t ld_left = s->flip ? s->ldp : s->ldq, ld_right = s->flip ? s->ldq : s->ldp;
    if (U)
        BIS_HIP_CHECK(ctx, hipMemcpy2DAsync(U, sizeof(double) * (size_t)ldu, left, sizeof(double) * (size_t)ld_left,
                                            sizeof(double) * (size_t)s->rows, (size_t)s->k, hipMemcpyDeviceToDevice, ctx->stream));
    if (V)
        BIS_HIP_CHECK(ctx, hipMemcpy2DAsync(V, sizeof(double) * (size_t)ldv, right, sizeof(double) * (size_t)ld_right,
                                            sizeof(double) * (size_t)s->cols, (size_t)s->k, hipMemcpyDeviceToDevice, ctx->stream));
    return BIS_OK;
}

} // extern "C"
