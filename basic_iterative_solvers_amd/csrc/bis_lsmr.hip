// bis_lsmr.hip -- LSMR (Fong and Saunders) for min ||A x - b||^2 + lambda^2 ||x||^2 with a rectangular A of any shape, on
// one right-hand side, as a sync-free device schedule of the kind bis_minres.hip is: two SpMVs (A and At, both through
// bis_spmv_launch), three streaming passes and two global reductions per iteration, two m-vectors and four n-vectors at any
// iteration count.  With a column scaling d the iteration runs on A D, D = diag(d), with y = D^-1 x; damping acts on y.
//   init:  u~ = b - A x ; beta = sqrt((u~, u~)) ; ib = 1 / beta ; p = (At u~) ib [; p = p d] ; alpha = sqrt((p, p)) ;
//          ia = 1 / alpha ; v = p ia ; h = v ; hbar = 0 [; w = d v] ; zetabar = alpha beta ; alphabar = alpha ;
//          rho = rhobar = cbar = 1 ; sbar = 0 ; hist_ar[0] = zetabar ; hist_r[0] = beta
//   iteration k = 1, 2, ... (u~ = beta u is kept un-normalised: no pass exists only to scale an m-vector):
//     SpMV    t_m = A w                      w is v without a scaling                     bis_spmv_launch
//     pass U  u~ = fma(-(alpha ib), u~, t_m) ; (u~, u~)          the last workgroup: beta = sqrt, ib = 1 / beta
//     SpMV    t_n = At u~
//     pass V  p = t_n ib [; p = p d] ; v~ = fma(-beta, v, p) -> t_n ; (v~, v~)
//             the last workgroup's lane 0: alpha = sqrt, ia = 1 / alpha, the three rotations, zeta, zetabar, the coefficients
//             of pass H, the ||rbar|| recurrences, the two history entries, the stop test (ls_book)
//     pass H  v = v~ ia ; hbar = fma(-c_hbar, hbar, h) ; x = fma(c_x, [d] hbar, x) ; h = fma(-c_h, h, v) [; w = d v]
// The reciprocal of zero is never formed: 0 stands for it, and beta = 0 or alpha = 0 ends the solve in that iteration
// (a breakdown: converged, hist_ar entry 0).  Every division of the scalar algebra whose divisor is 0 gives 0.
// Traffic per iteration beside the two SpMVs: pass U reads u~, t_m and writes u~ (24 B per row of A); pass V reads t_n, v
// and writes v~ (24 B per column); pass H reads v~, hbar, h, x and writes v, hbar, x, h (64 B per column): 24 m + 88 n
// bytes.  With a scaling pass V also reads d and pass H reads d and writes w: 24 m + 112 n.
// The fused sums are bis_dot's: its grid and index map, two fma chains per lane (the two halves of its 16 bytes), the same
// block and partial sums, added by the workgroup that arrives last in index order (reduce_last): no floating-point
// atomics, no kernel waits for another workgroup, two runs give the same bits.  The scalar algebra rounds every operation
// separately.  After the stop every launch returns at once (the SpMVs through bis_stop_guard) except pass H of the stopping
// iteration: x is the iterate of the last history entry.
// Memory: u~, t_m (m doubles each), v, h, hbar, t_n (n each), w with a scaling, At when the handle made it, the history
// (2 x 65536 doubles); m and n rounded up to even.
#include "bis_solver.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

struct bis_lsmr : bis_solver_core { // flags: [0] iterations, [1] stopped, [2] converged, [3] the iteration of the stop, [4] reason
    const bis_mat *A = nullptr, *At = nullptr;
    bis_mat *At_owned = nullptr; // bis_mat_transpose(A) when the caller passed none
    const double *b = nullptr;
    double *x = nullptr;
    int64_t m = 0, n = 0;
    double lambda = 0.0;
    const double *d = nullptr; // the column scaling (the caller's) or null
    double *u = nullptr, *tm = nullptr;                                // m
    double *v = nullptr, *h = nullptr, *hbar = nullptr, *tn = nullptr; // n
    double *w = nullptr;                                               // n, with a scaling only
    double *sc = nullptr;                                              // device scalars (S_*)
    // counters: two last-arriver counter sets: pass U, pass V
};

namespace {

constexpr int kT = kSolverT;
constexpr int kFlags = 8;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxDotBlocks); // passes U and V run on bis_pair_grid(., kMaxDotBlocks)

enum { S_CU = 0 /* alpha ib */, S_BETA, S_IB, S_IA, S_ABAR, S_ZBAR, S_RHO, S_RHOBAR, S_CBAR, S_SBAR, S_LAMBDA, S_C_HBAR, S_C_X,
       S_C_H, S_BDD, S_BD, S_RHODOLD, S_TAUTOLD, S_THETAT, S_ZETA, S_DSUM, S_STOP_R, S_STOP_AR, S_COUNT = 24 };
enum { R_LIVE = 0, R_TOL_R, R_TOL_AR, R_BREAKDOWN, R_NOT_FINITE };

__device__ __forceinline__ double div0(double a, double b) { return b == 0.0 ? 0.0 : a / b; }
__device__ __forceinline__ bool not_finite(double a) { return fabs(a) > DBL_MAX || a != a; }
// den = sqrt(a^2 + b^2), c = a / den, s = b / den; den = 0: c = 1, s = 0
__device__ __forceinline__ void rot(double a, double b, double &c, double &s, double &den) {
#pragma clang fp contract(off)
    den = sqrt(a * a + b * b);
    if (den == 0.0) { c = 1.0; s = 0.0; return; }
    c = a / den;
    s = b / den;
}

// the scalar algebra of one iteration after (v~, v~) is known: one lane
__device__ void ls_book(double vv, double *sc, int *flags, double *hist, int hist_cap) {
#pragma clang fp contract(off)
    const double alpha = sqrt(vv), ia = div0(1.0, alpha), beta = sc[S_BETA], ib = sc[S_IB];
    double chat, shat, alphahat, c, s, rho, cbar, sbar, rhobar, ctold, stold, rhotold;
    rot(sc[S_ABAR], sc[S_LAMBDA], chat, shat, alphahat);
    const double rhoold = sc[S_RHO];
    rot(alphahat, beta, c, s, rho);
    const double thetanew = s * alpha;
    const double rhobarold = sc[S_RHOBAR], zetaold = sc[S_ZETA], zetabar_in = sc[S_ZBAR];
    const double thetabar = sc[S_SBAR] * rho;
    rot(sc[S_CBAR] * rho, thetanew, cbar, sbar, rhobar);
    const double zeta = cbar * zetabar_in, zetabar = -sbar * zetabar_in;
    // the ||rbar|| estimate
    const double betaacute = chat * sc[S_BDD], betacheck = -shat * sc[S_BDD];
    const double betahat = c * betaacute, betadd = -s * betaacute;
    const double thetatildeold = sc[S_THETAT];
    rot(sc[S_RHODOLD], thetabar, ctold, stold, rhotold);
    const double thetatilde = stold * rhobar, rhodold = ctold * rhobar;
    const double betad = -stold * sc[S_BD] + ctold * betahat;
    const double tautildeold = div0(zetaold - thetatildeold * sc[S_TAUTOLD], rhotold);
    const double taud = div0(zeta - thetatilde * tautildeold, rhodold);
    const double dsum = sc[S_DSUM] + betacheck * betacheck;
    const double diff = betad - taud;
    const double normr = sqrt(dsum + diff * diff + betadd * betadd), normar = fabs(zetabar);
    sc[S_IA] = ia;
    sc[S_CU] = alpha * ib;
    sc[S_ABAR] = c * alpha;
    sc[S_ZBAR] = zetabar;
    sc[S_RHO] = rho;
    sc[S_RHOBAR] = rhobar;
    sc[S_CBAR] = cbar;
    sc[S_SBAR] = sbar;
    sc[S_C_HBAR] = div0(thetabar * rho, rhoold * rhobarold);
    sc[S_C_X] = div0(zeta, rho * rhobar);
    sc[S_C_H] = div0(thetanew, rho);
    sc[S_BDD] = betadd;
    sc[S_BD] = betad;
    sc[S_RHODOLD] = rhodold;
    sc[S_TAUTOLD] = tautildeold;
    sc[S_THETAT] = thetatilde;
    sc[S_ZETA] = zeta;
    sc[S_DSUM] = dsum;
    const int it = flags[0] + 1;
    flags[0] = it;
    if (it < hist_cap) { hist[it] = normar; hist[(size_t)hist_cap + it] = normr; }
    int reason = R_LIVE;
    if (not_finite(normar) || not_finite(normr)) reason = R_NOT_FINITE;
    else if (beta == 0.0 || alpha == 0.0) reason = R_BREAKDOWN;
    else if (normr < sc[S_STOP_R]) reason = R_TOL_R;
    else if (normar < sc[S_STOP_AR]) reason = R_TOL_AR;
    if (reason != R_LIVE) { // pass H of iteration `it` still runs
        flags[1] = 1;
        flags[2] = reason == R_NOT_FINITE ? 0 : 1;
        flags[3] = it;
        flags[4] = reason;
    }
}

// pass U: u~ = fma(-(alpha ib), u~, t_m), (u~, u~); the last workgroup: beta and 1 / beta
__global__ __launch_bounds__(kT) void ls_u_kernel(int64_t m, double *sc, const int *flags, double *__restrict__ u,
                                                  const double *__restrict__ tm, double *partials, unsigned *counter) {
    __shared__ double lds[kT / 64];
    if (flags[1]) return;
    const double c = sc[S_CU];
    const int64_t m2 = m >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *u2 = reinterpret_cast<double2 *>(u);
    const double2 *t2 = reinterpret_cast<const double2 *>(tm);
    double acc0 = 0.0, acc1 = 0.0; // bis_dot's two chains per lane
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < m2; i += gs) {
        double2 uv = u2[i];
        const double2 tv = t2[i];
        uv.x = fma(-c, uv.x, tv.x);
        uv.y = fma(-c, uv.y, tv.y);
        u2[i] = uv;
        acc0 = fma(uv.x, uv.x, acc0);
        acc1 = fma(uv.y, uv.y, acc1);
    }
    if ((m & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double uv = fma(-c, u[m - 1], tm[m - 1]);
        u[m - 1] = uv;
        acc0 = fma(uv, uv, acc0);
    }
    const double acc[1] = {acc0 + acc1};
    double total[1];
    if (!reduce_last<1>(acc, lds, partials, counter, total)) return;
    if (threadIdx.x != 0) return;
    const double beta = sqrt(total[0]);
    sc[S_BETA] = beta;
    sc[S_IB] = div0(1.0, beta);
}

// pass V: p = t_n ib [d], v~ = fma(-beta, v, p) into t_n, (v~, v~); the last workgroup: the bookkeeping
template <bool SCALED>
__global__ __launch_bounds__(kT) void ls_v_kernel(int64_t n, double *sc, int *flags, double *__restrict__ tn,
                                                  const double *__restrict__ v, const double *__restrict__ d, double *partials,
                                                  unsigned *counter, double *hist, int hist_cap) {
    __shared__ double lds[kT / 64];
    if (flags[1]) return;
    const double ib = sc[S_IB], beta = sc[S_BETA];
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *t2 = reinterpret_cast<double2 *>(tn);
    const double2 *v2 = reinterpret_cast<const double2 *>(v);
    const double2 *d2 = reinterpret_cast<const double2 *>(d);
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 tv = t2[i];
        const double2 vv = v2[i];
        tv.x *= ib;
        tv.y *= ib;
        if (SCALED) {
            const double2 dv = d2[i];
            tv.x *= dv.x;
            tv.y *= dv.y;
        }
        tv.x = fma(-beta, vv.x, tv.x);
        tv.y = fma(-beta, vv.y, tv.y);
        t2[i] = tv;
        acc0 = fma(tv.x, tv.x, acc0);
        acc1 = fma(tv.y, tv.y, acc1);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double tv = tn[n - 1] * ib;
        if (SCALED) tv *= d[n - 1];
        tv = fma(-beta, v[n - 1], tv);
        tn[n - 1] = tv;
        acc0 = fma(tv, tv, acc0);
    }
    const double acc[1] = {acc0 + acc1};
    double total[1];
    if (!reduce_last<1>(acc, lds, partials, counter, total)) return;
    // every other workgroup has read its scalars and the stop flag before it arrived: they may change now
    if (threadIdx.x == 0) ls_book(total[0], sc, flags, hist, hist_cap);
}

// pass H: v = v~ ia; hbar = fma(-c_hbar, hbar, h); x = fma(c_x, [d] hbar, x); h = fma(-c_h, h, v) [; w = d v].  `it` = the
// iteration this launch belongs to: when the stop test fired in THIS iteration the pass still runs, later launches are no-ops.
template <bool SCALED>
__global__ __launch_bounds__(kT) void ls_h_kernel(int64_t n, const double *__restrict__ sc, const int *__restrict__ flags, int it,
                                                  const double *__restrict__ vt, double *__restrict__ v, double *__restrict__ h,
                                                  double *__restrict__ hbar, double *__restrict__ x,
                                                  const double *__restrict__ d, double *__restrict__ w) {
    if (flags[1] && flags[3] != it) return;
    const double ia = sc[S_IA], c_hbar = sc[S_C_HBAR], c_x = sc[S_C_X], c_h = sc[S_C_H];
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *vt2 = reinterpret_cast<const double2 *>(vt);
    double2 *v2 = reinterpret_cast<double2 *>(v);
    double2 *h2 = reinterpret_cast<double2 *>(h);
    double2 *hb2 = reinterpret_cast<double2 *>(hbar);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    const double2 *d2 = reinterpret_cast<const double2 *>(d);
    double2 *w2 = reinterpret_cast<double2 *>(w);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 tv = vt2[i];
        double2 hv = h2[i], bv = hb2[i], xv = x2[i];
        const double2 vv = make_double2(tv.x * ia, tv.y * ia);
        bv.x = fma(-c_hbar, bv.x, hv.x);
        bv.y = fma(-c_hbar, bv.y, hv.y);
        if (SCALED) {
            const double2 dv = d2[i];
            xv.x = fma(c_x, dv.x * bv.x, xv.x);
            xv.y = fma(c_x, dv.y * bv.y, xv.y);
            w2[i] = make_double2(dv.x * vv.x, dv.y * vv.y);
        } else {
            xv.x = fma(c_x, bv.x, xv.x);
            xv.y = fma(c_x, bv.y, xv.y);
        }
        hv.x = fma(-c_h, hv.x, vv.x);
        hv.y = fma(-c_h, hv.y, vv.y);
        v2[i] = vv;
        hb2[i] = bv;
        x2[i] = xv;
        h2[i] = hv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double vv = vt[i] * ia;
        const double bv = fma(-c_hbar, hbar[i], h[i]);
        if (SCALED) {
            x[i] = fma(c_x, d[i] * bv, x[i]);
            w[i] = d[i] * vv;
        } else {
            x[i] = fma(c_x, bv, x[i]);
        }
        h[i] = fma(-c_h, h[i], vv);
        v[i] = vv;
        hbar[i] = bv;
    }
}

// out[r] = sqrt(sum_k a_rk^2): one lane per row, one fma chain in CRS order from 0
template <typename RP>
__global__ __launch_bounds__(kT) void row_norms_kernel(int64_t n_rows, const RP *__restrict__ row_ptr,
                                                       const double *__restrict__ val, double *__restrict__ out) {
    const int64_t gs = (int64_t)gridDim.x * kT;
    for (int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x; r < n_rows; r += gs) {
        double s = 0.0;
        for (int64_t k = row_ptr[r], e = row_ptr[r + 1]; k < e; ++k) s = fma(val[k], val[k], s);
        out[r] = sqrt(s);
    }
}

// d[i] = 1 / norms[i], 1 where the norm is 0 (d may be norms)
__global__ __launch_bounds__(kT) void scaling_kernel(int64_t n, const double *norms, double *d) {
    const int64_t gs = (int64_t)gridDim.x * kT;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += gs) d[i] = norms[i] == 0.0 ? 1.0 : 1.0 / norms[i];
}

inline bool lsmr_empty(const bis_lsmr *s) { return s->m == 0 || s->n == 0; }

} // namespace

extern "C" {

bis_status bis_mat_row_norms(bis_ctx *ctx, const bis_mat *A, double *out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && (out || A->n_rows == 0), "bis_mat_row_norms: bad arguments");
    BIS_REQUIRE(ctx, !A->view, "bis_mat_row_norms: a row-range view is not an operand");
    if (A->n_rows == 0) return BIS_OK;
    if (A->rp64)
        hipLaunchKernelGGL(row_norms_kernel<int64_t>, dim3(lane_grid(A->n_rows)), dim3(kT), 0, ctx->stream, A->n_rows,
                           (const int64_t *)A->row_ptr, (const double *)A->val, out);
    else
        hipLaunchKernelGGL(row_norms_kernel<int32_t>, dim3(lane_grid(A->n_rows)), dim3(kT), 0, ctx->stream, A->n_rows,
                           (const int32_t *)A->row_ptr, (const double *)A->val, out);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_lsmr_scaling_from_norms(bis_ctx *ctx, const double *norms, int64_t n, double *d) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n >= 0 && ((norms && d) || n == 0), "bis_lsmr_scaling_from_norms: bad arguments");
    if (n == 0) return BIS_OK;
    hipLaunchKernelGGL(scaling_kernel, dim3(lane_grid(n)), dim3(kT), 0, ctx->stream, n, norms, d);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_lsmr_create(bis_ctx *ctx, const bis_mat *A, const bis_mat *At, const double *b, double *x, bis_lsmr **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && out, "bis_lsmr_create: bad arguments");
    BIS_REQUIRE(ctx, (b || A->n_rows == 0) && (x || A->n_cols == 0), "bis_lsmr_create: bad arguments");
    BIS_REQUIRE(ctx, !At || (At->n_rows == A->n_cols && At->n_cols == A->n_rows && At->nnz == A->nnz),
                "bis_lsmr_create: At must be n x m with the entries of A");
    BIS_REQUIRE(ctx, aligned16(b) && aligned16(x), "bis_lsmr_create: b and x must be 16-byte aligned");
    bis_lsmr *s = new bis_lsmr;
    s->A = A; s->At = At; s->b = b; s->x = x;
    s->m = A->n_rows;
    s->n = A->n_cols;
    const int64_t ldm = (s->m + 1) & ~(int64_t)1, ldn = (s->n + 1) & ~(int64_t)1;
    bis_status st = BIS_OK;
    if (!lsmr_empty(s)) {
        if (!At) {
            st = bis_mat_transpose(ctx, A, &s->At_owned);
            s->At = s->At_owned;
        }
        for (double **p : {&s->u, &s->tm})
            if (st == BIS_OK) st = bis_vec_alloc(ctx, ldm, p);
        for (double **p : {&s->v, &s->h, &s->hbar, &s->tn})
            if (st == BIS_OK) st = bis_vec_alloc(ctx, ldn, p);
    }
    if (st == BIS_OK) st = bis_vec_alloc(ctx, S_COUNT, &s->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, s, kFlags, 2, 2, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st != BIS_OK) { bis_lsmr_destroy(ctx, s); return st; }
    *out = s;
    return BIS_OK;
}

bis_status bis_lsmr_set_damping(bis_ctx *ctx, bis_lsmr *s, double lambda) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_lsmr_set_damping: null handle");
    BIS_REQUIRE(ctx, !bis_solver_live(*s), "bis_lsmr_set_damping: call it before bis_lsmr_init");
    BIS_REQUIRE(ctx, lambda >= 0.0 && lambda <= DBL_MAX, "bis_lsmr_set_damping: lambda must be finite and not negative");
    s->lambda = lambda;
    return BIS_OK;
}

bis_status bis_lsmr_set_col_scaling(bis_ctx *ctx, bis_lsmr *s, const double *d) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_lsmr_set_col_scaling: null handle");
    BIS_REQUIRE(ctx, !bis_solver_live(*s), "bis_lsmr_set_col_scaling: call it before bis_lsmr_init");
    BIS_REQUIRE(ctx, aligned16(d), "bis_lsmr_set_col_scaling: d must be 16-byte aligned");
    if (d && !s->w && !lsmr_empty(s))
        if (bis_status st = bis_vec_alloc(ctx, (s->n + 1) & ~(int64_t)1, &s->w)) return st;
    s->d = d;
    return BIS_OK;
}

bis_status bis_lsmr_destroy(bis_ctx *ctx, bis_lsmr *s) {
    BIS_CTX_OK(ctx);
    if (!s) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *p : {s->u, s->tm, s->v, s->h, s->hbar, s->tn, s->w, s->sc}) hipFree(p);
    if (s->At_owned) bis_mat_destroy(ctx, s->At_owned);
    bis_solver_core_free(s);
    delete s;
    return BIS_OK;
}

bis_status bis_lsmr_init(bis_ctx *ctx, bis_lsmr *s, double tol_r, double tol_ar, double *r0_host, double *ar0_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_lsmr_init: null handle");
    s->enqueued = 0;
    const int64_t m = s->m, n = s->n;
    if (lsmr_empty(s)) {
        if (r0_host) *r0_host = 0.0;
        if (ar0_host) *ar0_host = 0.0;
        return BIS_OK;
    }
    double uu = 0.0, pp = 0.0;
    bis_status st = bis_compute_residual(ctx, s->A, s->x, s->b, s->u, s->tm);
    if (st == BIS_OK) st = bis_dot(ctx, s->u, s->u, m, &uu);
    if (st != BIS_OK) return st;
    const double beta = sqrt(uu), ib = beta == 0.0 ? 0.0 : 1.0 / beta;
    st = bis_spmv_launch(ctx, s->At, s->u, s->tn, nullptr, nullptr);
    if (st == BIS_OK) st = bis_scale(ctx, s->tn, s->tn, ib, n);
    if (st == BIS_OK && s->d) st = bis_elemwise_mult_vectors(ctx, s->tn, s->tn, s->d, n, 1.0);
    if (st == BIS_OK) st = bis_dot(ctx, s->tn, s->tn, n, &pp);
    if (st != BIS_OK) return st;
    const double alpha = sqrt(pp), ia = alpha == 0.0 ? 0.0 : 1.0 / alpha;
    st = bis_scale(ctx, s->v, s->tn, ia, n);
    if (st == BIS_OK) st = bis_copy_vector(ctx, s->h, s->v, n);
    if (st == BIS_OK && s->d) st = bis_elemwise_mult_vectors(ctx, s->w, s->v, s->d, n, 1.0);
    if (st != BIS_OK) return st;
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->hbar, 0, sizeof(double) * (size_t)n, ctx->stream));
    const double zetabar = alpha * beta;
    double sc[S_COUNT] = {0};
    sc[S_CU] = alpha * ib;
    sc[S_BETA] = beta;
    sc[S_IB] = ib;
    sc[S_IA] = ia;
    sc[S_ABAR] = alpha;
    sc[S_ZBAR] = zetabar;
    sc[S_RHO] = sc[S_RHOBAR] = sc[S_CBAR] = 1.0;
    sc[S_LAMBDA] = s->lambda;
    sc[S_BDD] = beta;
    sc[S_RHODOLD] = 1.0;
    sc[S_STOP_R] = tol_r * beta;
    sc[S_STOP_AR] = tol_ar * zetabar;
    int flags[kFlags] = {0};
    if (zetabar == 0.0) { // x0 is a least-squares solution already: nothing to iterate on
        flags[1] = flags[2] = 1;
        flags[4] = R_BREAKDOWN;
    } else if (!std::isfinite(zetabar) || !std::isfinite(beta)) {
        flags[1] = 1;
        flags[4] = R_NOT_FINITE;
    }
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc, sc, sizeof sc, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->flags, flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->hist, &zetabar, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->hist + s->hist_cap, &beta, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BIS_SYNC_CHECK(ctx);
    s->initialised = true;
    if (r0_host) *r0_host = beta;
    if (ar0_host) *ar0_host = zetabar;
    return BIS_OK;
}

bis_status bis_lsmr_iterate(bis_ctx *ctx, bis_lsmr *s, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s && n_iters >= 0 && s->enqueued + n_iters < kMaxIters, "bis_lsmr_iterate: bad arguments");
    if (lsmr_empty(s)) return BIS_OK;
    BIS_REQUIRE(ctx, s->initialised, "bis_lsmr_iterate: call bis_lsmr_init first");
    const int64_t m = s->m, n = s->n;
    const int g_u = bis_pair_grid(m, kMaxDotBlocks), g_v = bis_pair_grid(n, kMaxDotBlocks), g_h = bis_pair_grid(n, kMaxEwBlocks);
    bis_status st = bis_ensure_partials(ctx, kMaxDotBlocks);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, s->flags); // the SpMVs return at once when the solve has stopped
    unsigned *cnt_u = s->counters, *cnt_v = s->counters + kCounterSet;
    const double *w = s->d ? s->w : s->v;
    for (int done = 0; done < n_iters; ++done) {
        const int k = s->enqueued + done + 1;
        st = bis_spmv_launch(ctx, s->A, w, s->tm, nullptr, nullptr);
        if (st != BIS_OK) { s->enqueued += done; return st; } // (the device's count stays behind: call bis_lsmr_init again)
        hipLaunchKernelGGL(ls_u_kernel, dim3(g_u), dim3(kT), 0, ctx->stream, m, s->sc, (const int *)s->flags, s->u,
                           (const double *)s->tm, ctx->partials, cnt_u);
        st = bis_spmv_launch(ctx, s->At, s->u, s->tn, nullptr, nullptr);
        if (st != BIS_OK) { s->enqueued += done; return st; }
        if (s->d) {
            hipLaunchKernelGGL((ls_v_kernel<true>), dim3(g_v), dim3(kT), 0, ctx->stream, n, s->sc, s->flags, s->tn,
                               (const double *)s->v, s->d, ctx->partials, cnt_v, s->hist, s->hist_cap);
            hipLaunchKernelGGL((ls_h_kernel<true>), dim3(g_h), dim3(kT), 0, ctx->stream, n, (const double *)s->sc,
                               (const int *)s->flags, k, (const double *)s->tn, s->v, s->h, s->hbar, s->x, s->d, s->w);
        } else {
            hipLaunchKernelGGL((ls_v_kernel<false>), dim3(g_v), dim3(kT), 0, ctx->stream, n, s->sc, s->flags, s->tn,
                               (const double *)s->v, (const double *)nullptr, ctx->partials, cnt_v, s->hist, s->hist_cap);
            hipLaunchKernelGGL((ls_h_kernel<false>), dim3(g_h), dim3(kT), 0, ctx->stream, n, (const double *)s->sc,
                               (const int *)s->flags, k, (const double *)s->tn, s->v, s->h, s->hbar, s->x,
                               (const double *)nullptr, (double *)nullptr);
        }
    }
    s->enqueued += n_iters; // the launches were issued whatever the check below says: k keeps matching the device's count
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_lsmr_status(bis_ctx *ctx, bis_lsmr *s, int *iters, int *converged, int *reason, double *hist_ar_host,
                           double *hist_r_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_lsmr_status: null handle");
    int flags[kFlags] = {0};
    if (bis_status st = bis_solver_read_flags(ctx, *s, 0, kFlags, flags)) return st;
    if (iters) *iters = flags[0];
    if (converged) *converged = flags[2];
    if (reason) *reason = flags[4];
    if (hist_cap > 0 && s->initialised) {
        const int cnt = std::min(flags[0] + 1, hist_cap);
        if (hist_ar_host)
            if (bis_status st = bis_solver_copy_hist(ctx, *s, 0, cnt, hist_ar_host)) return st;
        if (hist_r_host)
            if (bis_status st = bis_solver_copy_hist(ctx, *s, 1, cnt, hist_r_host)) return st;
    }
    return BIS_OK;
}

} // extern "C"
