// bis_eigs.hip -- thick-restart Lanczos (Wu and Simon) with full re-orthogonalisation for the k extreme eigenpairs of a
// symmetric matrix, as a sync-free device schedule of the kind bis_fgmres.hip is.  include/bis_hip.h states the algorithm
// line by line; here is how it is laid out.  m = ncv basis blocks V_0 .. V_m (ld = n rounded up to even apart) and the work
// vector W: (m + 2) n-vectors.  The passes over n-vectors are bis_lanczos.hpp's, shared with bis_svds.hip.  One step j (one
// operator product, the handle's own bis_spmv or the caller's):
//     W = OP V_j                                                      bis_spmv_launch, or the caller between op_begin / op_end
//     h = V_{0..j}^T W      lanczos_dots_kernel, one launch per group of at most 8 basis blocks: W is read once per group
//     W -= V_{0..j} h       lanczos_update_kernel<false>: one launch, one fma per element and block, ascending block index
//     c = V_{0..j}^T W      lanczos_dots_kernel again
//     W -= V_{0..j} c       lanczos_update_kernel<true>: (W, W) fused; the last workgroup's lane 0 (eigs_close): alpha_j =
//                           h_j + c_j, beta_j = sqrt((W, W)), the product count, the breakdown beta_j <= eps || OP V_j ||
//     V_{j+1} = W / beta_j  lanczos_scale_kernel
//     eigs_ritz_kernel (one wave) and lanczos_compress_kernel: they act when the cycle closes (j = m - 1, known on the host)
//     or when the update before them met a breakdown (flags[6], known on the device only); otherwise they return at once.
// Traffic per step besides the product: four reads of the j + 1 basis blocks (two by the dots, two by the updates) and
// 2 ceil((j + 1) / 8) + 6 passes over W (the dots' reads, the updates' read and write each, the scale's read and write).
// The Ritz kernel is one wave: T and Y (64 x 64 doubles each) sit in LDS, lane c owns column c of T and row c of Y, the
// rotations of the cyclic Jacobi sweeps follow each other.  The compression V_{0..l) <- V_{0..m) Y_keep works in place, row by
// row: a lane reads its row of all m blocks into registers and then writes l blocks; Y_keep sits in LDS (64 x 64 doubles).
// After a stop every launch returns at once (the products through bis_stop_guard).
#include "bis_lanczos.hpp"

// flags: bis_lanczos.hpp
struct bis_eigs : bis_lanczos_core {
    const bis_mat *A = nullptr; // null: the caller applies the operator
    int64_t n = 0, ld = 0;
    double *V = nullptr; // m + 1 blocks of ld
    double *W = nullptr;
};

namespace {

enum { S_ALPHA = 0, S_BETA = kM, S_THETA = 2 * kM, S_S = 3 * kM, S_H = 4 * kM, S_C = 5 * kM, S_VAL = 6 * kM, S_EST = 7 * kM,
       S_TOL = 8 * kM, S_EPS23, S_NRM0, S_WW0 /* (W, W) before the passes */, S_Y = 9 * kM /* Y_keep, row b at S_Y + kM b */, S_COUNT = S_Y + kM * kM };

// how lanczos_update_kernel<true> closes step j: ww = (W, W) after both passes
struct eigs_close {
    double *sc;
    int *flags;
    int j;
    __device__ void operator()(double ww) const {
        double beta = sqrt(ww);
        // an invariant subspace: beta_j is 0, or the rounding noise that two passes leave of it (eps^2 || OP V_j ||, where a
        // genuine beta_j is orders above eps || OP V_j ||).  No reciprocal: the Ritz launch behind this step closes the cycle
        // at j + 1 with beta_j = 0.
        const bool invariant = beta <= DBL_EPSILON * sqrt(sc[S_WW0]);
        if (invariant) beta = 0.0;
        sc[S_ALPHA + j] = sc[S_H + j] + sc[S_C + j];
        sc[S_BETA + j] = beta;
        flags[0] += 1;
        if (invariant) {
            flags[1] = 1;
            flags[6] = j + 1;
        }
    }
};

// The restart: one wave.  close: the cycle closes here with m_eff = m (the host knows); otherwise the launch acts only on a
// breakdown (flags[6] = m_eff).  l_in: the pairs kept by the restart before (0 in the first cycle); l_keep: the pairs a
// restart keeps.  T(r, c) at T[c * kLd + r]; lane c owns column c of T and row c of Y (Y(r, c) at Y[r * kLd + c]).
__global__ __launch_bounds__(64) void eigs_ritz_kernel(double *sc, int *flags, int close, int m, int l_in, int l_keep, int k,
                                                       int which, double *hist, int hist_cap) {
#pragma clang fp contract(off)
    __shared__ double T[kM * kLd], Y[kM * kLd]; // kLd: the lanes of a column-strided access fall into different banks
    __shared__ double red[kM], key[kM], theta[kM];
    __shared__ int order[kM], rank[kM];
    const int lane = threadIdx.x;
    const int pending = flags[6];
    if (!pending && (flags[1] || !close)) {
        if (lane == 0) flags[7] = 0;
        return;
    }
    const int me = pending ? pending : m; // m_eff
    // ---- T ----
    for (int r = 0; r < me; ++r)
        if (lane < me) { T[lane * kLd + r] = 0.0; Y[r * kLd + lane] = r == lane ? 1.0 : 0.0; }
    __syncthreads();
    if (lane < me) {
        if (lane < l_in) {
            T[lane * kLd + lane] = sc[S_THETA + lane];
            T[l_in * kLd + lane] = sc[S_S + lane];
            T[lane * kLd + l_in] = sc[S_S + lane];
        } else {
            T[lane * kLd + lane] = sc[S_ALPHA + lane];
            if (lane + 1 < me) {
                T[(lane + 1) * kLd + lane] = sc[S_BETA + lane];
                T[lane * kLd + lane + 1] = sc[S_BETA + lane];
            }
        }
    }
    __syncthreads();
    const double beta_last = sc[S_BETA + me - 1];
    // ||T||_F: column sums of squares in row order, added in column order
    {
        double a = 0.0;
        if (lane < me)
            for (int r = 0; r < me; ++r) a += T[lane * kLd + r] * T[lane * kLd + r];
        red[lane] = a;
    }
    __syncthreads();
    double fro = 0.0;
    for (int c = 0; c < me; ++c) fro += red[c];
    fro = sqrt(fro);
    __syncthreads();
    // ---- cyclic Jacobi ----
    bool diagonal = false;
    for (int sweep = 0; sweep <= kMaxSweeps; ++sweep) {
        double a = 0.0; // off(T) from the off-diagonal entries themselves
        if (lane < me)
            for (int r = 0; r < me; ++r)
                if (r != lane) a += T[lane * kLd + r] * T[lane * kLd + r];
        red[lane] = a;
        __syncthreads();
        double off = 0.0;
        for (int c = 0; c < me; ++c) off += red[c];
        off = sqrt(off);
        __syncthreads();
        if (off <= DBL_EPSILON * fro) { diagonal = true; break; }
        if (sweep == kMaxSweeps) break;
        for (int p = 0; p < me - 1; ++p)
            for (int q = p + 1; q < me; ++q) {
                const double apq = T[q * kLd + p];
                if (apq == 0.0) continue; // (the same in every lane)
                const double app = T[p * kLd + p], aqq = T[q * kLd + q];
                const double tau = (aqq - app) / (2.0 * apq);
                const double root = sqrt(1.0 + tau * tau);
                const double t = 1.0 / (tau >= 0.0 ? tau + root : tau - root);
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, rho = s / (1.0 + c);
                __syncthreads();
                if (lane < me) {
                    if (lane != p && lane != q) {
                        const double tp = T[lane * kLd + p], tq = T[lane * kLd + q];
                        const double np_ = tp - s * (tq + rho * tp), nq_ = tq + s * (tp - rho * tq);
                        T[lane * kLd + p] = np_; T[p * kLd + lane] = np_;
                        T[lane * kLd + q] = nq_; T[q * kLd + lane] = nq_;
                    } else if (lane == p) {
                        T[p * kLd + p] = app - t * apq;
                        T[q * kLd + p] = 0.0;
                    } else {
                        T[q * kLd + q] = aqq + t * apq;
                        T[p * kLd + q] = 0.0;
                    }
                    const double yp = Y[lane * kLd + p], yq = Y[lane * kLd + q];
                    Y[lane * kLd + p] = yp - s * (yq + rho * yp);
                    Y[lane * kLd + q] = yq + s * (yp - rho * yq);
                }
                __syncthreads();
            }
    }
    // ---- order, estimates, the test: lane 0 ----
    if (lane < me) theta[lane] = T[lane * kLd + lane];
    __syncthreads();
    const int n_ranked = min(k, me);
    if (lane == 0) {
        for (int i = 0; i < me; ++i) order[i] = i;
        lanczos_sort(order, theta, me); // ascending, stable
        // rank the ascending list: SA as it is, LA descending, LM descending |theta| (stable on the ascending list)
        for (int i = 0; i < me; ++i) {
            const double th = theta[order[i]];
            key[i] = which == 0 ? 0.0 : which == 1 ? -th : -fabs(th);
        }
        int pos[kM];
        for (int i = 0; i < me; ++i) pos[i] = i;
        if (which != 0) lanczos_sort(pos, key, me);
        for (int i = 0; i < me; ++i) rank[i] = order[pos[i]]; // the column of Y of rank i
        const double tol = sc[S_TOL], floor_ = sc[S_EPS23];
        double worst = 0.0;
        int nconv = 0;
        for (int i = 0; i < n_ranked; ++i) {
            const double th = theta[rank[i]];
            const double est = fabs(beta_last * Y[(me - 1) * kLd + rank[i]]);
            sc[S_VAL + i] = th;
            sc[S_EST + i] = est;
            worst = fmax(worst, est);
            if (est <= tol * fmax(fabs(th), floor_)) ++nconv;
        }
        key[0] = lanczos_verdict(flags, hist, hist_cap, pending, diagonal, nconv, worst, k, me, l_keep) ? 1.0 : 0.0;
    }
    __syncthreads();
    const bool stop = key[0] != 0.0;
    const int l_out = stop ? n_ranked : l_keep;
    // Y_keep (me x l_out), and the state of the next cycle
    if (lane < l_out) {
        const int col = rank[lane];
        if (!stop) {
            sc[S_THETA + lane] = theta[col];
            sc[S_S + lane] = beta_last * Y[(me - 1) * kLd + col];
        }
        for (int b = 0; b < me; ++b) sc[S_Y + kM * b + lane] = Y[b * kLd + col];
    }
}

// what follows a product in W: the rest of step j, and the restart when the cycle closes
void eigs_enqueue_step(bis_ctx *ctx, bis_eigs *s) {
    const int64_t n = s->n, ld = s->ld;
    const int j = s->j;
    const int *flags = s->flags;
    lanczos_enqueue_passes(ctx, s, n, ld, s->V, j + 1, s->W, s->sc + S_H, s->sc + S_C, s->sc + S_WW0, eigs_close{s->sc, s->flags, j},
                           s->sc + S_BETA + j, s->V + (int64_t)(j + 1) * ld);
    const int close = j == s->m - 1;
    hipLaunchKernelGGL(eigs_ritz_kernel, dim3(1), dim3(64), 0, ctx->stream, s->sc, s->flags, close, s->m, s->l_cur, s->l, s->k,
                       s->which, s->hist, s->hist_cap);
    hipLaunchKernelGGL(lanczos_compress_kernel<false>, dim3(lane_grid(n)), dim3(kT), 0, ctx->stream, n, ld, flags,
                       (const double *)(s->sc + S_Y), s->V);
    if (close) {
        s->j = s->l;
        s->l_cur = s->l;
    } else {
        s->j = j + 1;
    }
    s->enqueued += 1;
}

} // namespace

extern "C" {

bis_status bis_eigs_create(bis_ctx *ctx, const bis_mat *A, int64_t n, int k, int ncv, int which, bis_eigs **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, out, "bis_eigs_create: bad arguments");
    BIS_REQUIRE(ctx, !A || A->n_rows == A->n_cols, "bis_eigs_create: square matrix required");
    BIS_REQUIRE(ctx, !A || A->n_rows == n, "bis_eigs_create: n must be the size of A");
    BIS_REQUIRE(ctx, !A || !A->view, "bis_eigs_create: a row-range view is not an operand");
    BIS_REQUIRE(ctx, n >= 2, "bis_eigs_create: n must be at least 2");
    BIS_REQUIRE(ctx, k >= 1, "bis_eigs_create: k must be at least 1");
    BIS_REQUIRE(ctx, which >= BIS_EIGS_SA && which <= BIS_EIGS_LM, "bis_eigs_create: which must be BIS_EIGS_SA, _LA or _LM");
    const int64_t cap = std::min<int64_t>(n, kM);
    if (ncv == 0) ncv = (int)std::min<int64_t>(cap, std::max(2 * k + 1, 20));
    BIS_REQUIRE(ctx, ncv > k, "bis_eigs_create: ncv must exceed k (k < ncv <= min(n, 64))");
    BIS_REQUIRE(ctx, ncv <= cap, "bis_eigs_create: ncv must not exceed min(n, 64) (k < ncv <= min(n, 64))");
    bis_eigs *s = new bis_eigs;
    s->A = A;
    s->n = n;
    s->ld = (n + 1) & ~(int64_t)1;
    s->k = k;
    s->m = ncv;
    s->l = std::min(k + (ncv - k) / 2, ncv - 1);
    s->which = which;
    bis_status st = bis_vec_alloc(ctx, s->ld * (s->m + 1), &s->V);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, s->ld, &s->W);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, S_COUNT, &s->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, s, kFlags, 2, 1, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) { bis_eigs_destroy(ctx, s); return st; }
    *out = s;
    return BIS_OK;
}

bis_status bis_eigs_set_start(bis_ctx *ctx, bis_eigs *s, const double *v0) {
    return lanczos_set_start(ctx, s, v0, "bis_eigs");
}

bis_status bis_eigs_destroy(bis_ctx *ctx, bis_eigs *s) {
    BIS_CTX_OK(ctx);
    if (!s) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *p : {s->V, s->W, s->sc}) hipFree(p);
    bis_solver_core_free(s);
    delete s;
    return BIS_OK;
}

bis_status bis_eigs_init(bis_ctx *ctx, bis_eigs *s, double tol) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_eigs_init: null handle");
    // every earlier state goes: basis, work vector and scalars here, the rest in lanczos_init
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->V, 0, sizeof(double) * (size_t)s->ld * (s->m + 1), ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->W, 0, sizeof(double) * (size_t)s->ld, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->sc, 0, sizeof(double) * S_COUNT, ctx->stream));
    static const double eps23 = std::pow(DBL_EPSILON, 2.0 / 3.0);
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc + S_EPS23, &eps23, sizeof eps23, hipMemcpyHostToDevice, ctx->stream));
    return lanczos_init(ctx, s, s->n, s->ld, s->W, s->V, tol, S_TOL, S_NRM0);
}

bis_status bis_eigs_op_begin(bis_ctx *ctx, bis_eigs *s, const double **in_dev, double **out_dev) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && in_dev && out_dev, "bis_eigs_op_begin: bad arguments");
    BIS_REQUIRE(ctx, s->initialised, "bis_eigs_op_begin: call bis_eigs_init first");
    BIS_REQUIRE(ctx, !s->op_open, "bis_eigs_op_begin: the product before it was not closed with bis_eigs_op_end");
    BIS_REQUIRE(ctx, s->enqueued + 1 < kMaxIters, "bis_eigs_op_begin: too many products since bis_eigs_init");
    s->op_open = true;
    *in_dev = s->V + (int64_t)s->j * s->ld;
    *out_dev = s->W;
    return BIS_OK;
}

bis_status bis_eigs_op_end(bis_ctx *ctx, bis_eigs *s) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_eigs_op_end: null handle");
    BIS_REQUIRE(ctx, s->op_open, "bis_eigs_op_end: call bis_eigs_op_begin first");
    s->op_open = false;
    if (bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks)) return st;
    eigs_enqueue_step(ctx, s);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_eigs_iterate(bis_ctx *ctx, bis_eigs *s, int n_cycles) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && n_cycles >= 0, "bis_eigs_iterate: bad arguments");
    BIS_REQUIRE(ctx, s->A, "bis_eigs_iterate: the handle has no matrix (caller-applied operator): use bis_eigs_op_begin / bis_eigs_op_end");
    BIS_REQUIRE(ctx, s->initialised, "bis_eigs_iterate: call bis_eigs_init first");
    BIS_REQUIRE(ctx, !s->op_open, "bis_eigs_iterate: a product is open: call bis_eigs_op_end first");
    BIS_REQUIRE(ctx, (int64_t)s->enqueued + (int64_t)n_cycles * s->m < kMaxIters, "bis_eigs_iterate: too many products since bis_eigs_init");
    if (bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks)) return st;
    bis_stop_guard stop_guard(ctx, s->flags); // the products return at once when the solve has stopped
    for (int cycle = 0; cycle < n_cycles; ++cycle) {
        do { // to the end of the cycle the handle is in
            if (bis_status st = bis_spmv_launch(ctx, s->A, s->V + (int64_t)s->j * s->ld, s->W, nullptr, nullptr)) return st;
            eigs_enqueue_step(ctx, s);
        } while (s->j != s->l_cur || s->l_cur == 0);
    }
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_eigs_status(bis_ctx *ctx, bis_eigs *s, int *products, int *restarts, int *stopped, int *converged, int *reason,
                           int *nconv, double *values_host, double *est_host, double *hist_host, double *hist_nconv_host,
                           int hist_cap) {
    return lanczos_status(ctx, s, "bis_eigs", products, restarts, stopped, converged, reason, nconv, S_VAL, values_host, S_EST,
                          est_host, hist_host, hist_nconv_host, hist_cap);
}

bis_status bis_eigs_vectors(bis_ctx *ctx, bis_eigs *s, double *X, int64_t ldx) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && X && ldx >= s->n, "bis_eigs_vectors: bad arguments (ldx >= n)");
    int restarts = 0;
    if (bis_status st = bis_solver_read_flags(ctx, *s, 3, 1, &restarts)) return st;
    BIS_REQUIRE(ctx, s->initialised && restarts >= 1, "bis_eigs_vectors: no restart yet: the basis holds no Ritz vectors");
    BIS_HIP_CHECK(ctx, hipMemcpy2DAsync(X, sizeof(double) * (size_t)ldx, s->V, sizeof(double) * (size_t)s->ld,
                                        sizeof(double) * (size_t)s->n, (size_t)s->k, hipMemcpyDeviceToDevice, ctx->stream));
    return BIS_OK;
}

} // extern "C"
