// bis_idr.hip -- right-preconditioned IDR(s) with biorthogonalisation (Sonneveld / van Gijzen), 1 <= s <= 8, for a
// nonsymmetric A and one fixed M, on one right-hand side, as a sync-free device schedule of the kind bis_minres.hip is: one
// SpMV, one preconditioner apply and one history entry per iteration, 3 s + 3 n-vectors at any iteration count, no restart.
// An iteration is one position of a cycle of s + 1 positions (include/bis_hip.h states the method):
//   position k < s:
//     pass V   v = r - sum_{j >= k} c_j G_j                              idr_v_kernel   (no preconditioner: U_k in the same pass)
//     apply    t = M^-1 v                                                bis_pc_apply   (v^ IS v without a preconditioner)
//     pass U   U_k = omega v^ + sum_{j >= k} c_j U_j                     idr_u_kernel
//     SpMV     G_k = A U_k                                               bis_spmv_launch
//     pass Q   q = P^T G_k, s sums in one pass over G_k                  idr_dots_kernel; the last workgroup's lane 0: alpha by
//              forward substitution, column k of M, beta, the f update
//     pass W   G_k -= sum_{i < k} alpha_i G_i ; U_k -= sum_{i < k} alpha_i U_i ; r -= beta G_k ; x += beta U_k ; (r, r)
//              idr_w_kernel; the last workgroup's lane 0: history, count, stop test, c of position k + 1
//   position s:
//     apply    v = M^-1 r (none: v^ IS r) ; SpMV t = A v^
//     pass T   (t, t), (t, r)                                            idr_tt_kernel; lane 0: omega with the 0.7 safeguard
//     pass O   x += omega v^ ; r -= omega t ; (r, r) and f = P^T r       idr_o_kernel; lane 0: history, count, stop test, f, c
// The host knows the position from the enqueued count, so the launch sequence is fixed: 4 s + 3 launches per cycle without
// a preconditioner, 5 s + 3 with one (beside the apply's own).  Every "vector -+ scalar * vector" is one fma per element;
// sums over columns run over ascending column index.  Bytes per row at a position k < s, beside the SpMV and the apply:
// V (s - k + 2) 8, U (s - k + 2) 8, Q (s + 1) 8, W (2 k + 8) 8 -- (3 s + 13) 8 = 24 s + 104 whatever k is; position s:
// T 16, O (s + 6) 8.  The column count of a pass is a template parameter: the s accumulators of Q and O must live in
// registers (a runtime-indexed array goes to scratch), and with the count known the loads of all columns of an element are
// issued before the first fma (one s_waitcnt per element instead of one per column).
// Reductions are bis_internal.hpp's: per-workgroup partial sums (s of them per workgroup in Q, s + 1 in O), the workgroup
// that arrives last adds them in index order, its lane 0 does the small algebra in plain C++ with every operation rounded on
// its own.  No kernel waits for another workgroup, no floating-point atomics, the grid depends on n only: two runs give the
// same bits.  After the stop every launch of the schedule returns at once; x and r change in the pass whose sums decide the
// stop, so x is the iterate of the last history entry.  (Launches of a preconditioner queued behind the stop may still run;
// nothing reads their results.)
// Memory: r, v, t and the column blocks P, G, U = (3 s + 3) n doubles (n rounded up to even: every column starts on 16
// bytes and is an SpMV operand), 96 doubles of state, the history (65536 doubles), plus the preconditioner's scratch.
#include "bis_solver.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

struct bis_idr : bis_solver_core { // flags: [0] iterations, [1] stopped, [2] converged
    const bis_mat *A = nullptr;
    const double *b = nullptr;
    double *x = nullptr;
    int64_t n = 0, ld = 0; // ld: n rounded up to even
    int s = 0;
    double *r = nullptr, *v = nullptr, *t = nullptr;
    double *P = nullptr, *G = nullptr, *U = nullptr; // s columns of ld doubles each
    double *sc = nullptr; // device state (S_*)
    // counters: one last-arriver counter set; the reducing passes follow each other on the stream
};

namespace {

constexpr int kT = kSolverT;
constexpr int kMaxS = 8;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxReduceBlocks); // every reducing pass runs on bis_pair_grid(n, kMaxReduceBlocks)

// state: scalars, then c, alpha, f (kMaxS each) and the lower triangle M, row i at S_M + kMaxS i
enum { S_OMEGA = 0, S_NORM /* || r || */, S_STOP, S_BETA, S_C = 8, S_ALPHA = 16, S_F = 24, S_M = 32, S_COUNT = 96 };

// P[i][j] = (h + 0.5) 2^-31 - 1, h = hash32(hash32(i) ^ (j + 1) 0x9e3779b9): exact in fp64.  The padding row of an odd n is 0.
__global__ __launch_bounds__(kT) void idr_shadow_kernel(double *P, int64_t n, int64_t ld, int s) {
    const int64_t total = ld * s;
    for (int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kT) {
        const int64_t i = idx % ld, j = idx / ld;
        const uint32_t h = bis_hash32(bis_hash32((uint32_t)i) ^ ((uint32_t)(j + 1) * 0x9e3779b9u));
        P[idx] = i < n ? ((double)h + 0.5) * 0x1p-31 - 1.0 : 0.0;
    }
}

// ---- the small algebra: one lane, every operation rounded on its own ------------------------------------------------
// c[k .. s): forward substitution M[k.., k..] c = f[k..]
__device__ void idr_solve_c(double *sc, int k, int s) {
#pragma clang fp contract(off)
    for (int i = k; i < s; ++i) {
        double a = sc[S_F + i];
        for (int l = k; l < i; ++l) a -= sc[S_M + kMaxS * i + l] * sc[S_C + l];
        sc[S_C + i] = a / sc[S_M + kMaxS * i + i];
    }
}

// after q = P^T G_k: alpha_i for i < k, column k of M, beta, f_i for i > k
__device__ void idr_book_q(const double *q, double *sc, int k, int s) {
#pragma clang fp contract(off)
    for (int i = 0; i < k; ++i) {
        double a = q[i];
        for (int l = 0; l < i; ++l) a -= sc[S_M + kMaxS * i + l] * sc[S_ALPHA + l];
        sc[S_ALPHA + i] = a / sc[S_M + kMaxS * i + i];
    }
    for (int i = k; i < s; ++i) {
        double a = q[i];
        for (int l = 0; l < k; ++l) a -= sc[S_M + kMaxS * i + l] * sc[S_ALPHA + l];
        sc[S_M + kMaxS * i + k] = a;
    }
    const double beta = sc[S_F + k] / sc[S_M + kMaxS * k + k]; // M_kk = 0: the published breakdown, NaN or Inf from here on
    sc[S_BETA] = beta;
    for (int i = k + 1; i < s; ++i) sc[S_F + i] -= beta * sc[S_M + kMaxS * i + k];
}

// one history entry from (r, r), the count and the stop test
__device__ void idr_book_norm(double rr, double *sc, int *flags, double *hist, int hist_cap) {
    const double norm = sqrt(rr);
    sc[S_NORM] = norm;
    const int it = flags[0] + 1;
    flags[0] = it;
    if (it < hist_cap) hist[it] = norm;
    const bool conv = norm < sc[S_STOP];
    const bool not_finite = fabs(norm) > DBL_MAX || norm != norm;
    if (conv || not_finite) { flags[1] = 1; flags[2] = conv && !not_finite ? 1 : 0; }
}

// ---- position k < s -------------------------------------------------------------------------------------------------
// pass V: v = r - sum_j c_j G_j over the NC columns from k on (Gk, Uk, c point at column k); WITH_U (no preconditioner):
// U_k = omega v + sum_j c_j U_j in the same pass, U_k in place
template <int NC, bool WITH_U>
__global__ __launch_bounds__(kT) void idr_v_kernel(int64_t n, int64_t ld, const double *__restrict__ sc, int k,
                                                   const int *__restrict__ flags, const double *__restrict__ r,
                                                   const double *__restrict__ Gk, double *Uk, double *__restrict__ v) {
    if (flags[1]) return;
    double c[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) c[j] = sc[S_C + k + j];
    const double omega = sc[S_OMEGA];
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *r2 = reinterpret_cast<const double2 *>(r);
    const double2 *G2 = reinterpret_cast<const double2 *>(Gk);
    double2 *U2 = reinterpret_cast<double2 *>(Uk);
    double2 *v2 = reinterpret_cast<double2 *>(v);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 g[NC], u[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            g[j] = G2[i + j * ld2];
            if (WITH_U) u[j] = U2[i + j * ld2];
        }
        double2 vv = r2[i];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            vv.x = fma(-c[j], g[j].x, vv.x);
            vv.y = fma(-c[j], g[j].y, vv.y);
        }
        v2[i] = vv;
        if (WITH_U) {
            double2 uu = make_double2(omega * vv.x, omega * vv.y);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                uu.x = fma(c[j], u[j].x, uu.x);
                uu.y = fma(c[j], u[j].y, uu.y);
            }
            U2[i] = uu;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        double vv = r[i];
#pragma unroll
        for (int j = 0; j < NC; ++j) vv = fma(-c[j], Gk[i + j * ld], vv);
        v[i] = vv;
        if (WITH_U) {
            double uu = omega * vv;
#pragma unroll
            for (int j = 0; j < NC; ++j) uu = fma(c[j], Uk[i + j * ld], uu);
            Uk[i] = uu;
        }
    }
}

// pass U (with a preconditioner): U_k = omega vh + sum_j c_j U_j, U_k in place
template <int NC>
__global__ __launch_bounds__(kT) void idr_u_kernel(int64_t n, int64_t ld, const double *__restrict__ sc, int k,
                                                   const int *__restrict__ flags, const double *__restrict__ vh, double *Uk) {
    if (flags[1]) return;
    double c[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) c[j] = sc[S_C + k + j];
    const double omega = sc[S_OMEGA];
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *v2 = reinterpret_cast<const double2 *>(vh);
    double2 *U2 = reinterpret_cast<double2 *>(Uk);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 u[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) u[j] = U2[i + j * ld2];
        const double2 vv = v2[i];
        double2 uu = make_double2(omega * vv.x, omega * vv.y);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            uu.x = fma(c[j], u[j].x, uu.x);
            uu.y = fma(c[j], u[j].y, uu.y);
        }
        U2[i] = uu;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        double uu = omega * vh[i];
#pragma unroll
        for (int j = 0; j < NC; ++j) uu = fma(c[j], Uk[i + j * ld], uu);
        Uk[i] = uu;
    }
}

// the multi-dot q = P^T g: g is read once, S accumulators per lane.  k >= 0: pass Q of position k (idr_book_q);
// k < 0: bis_idr_init's f = P^T r with the c of position 0.
template <int S>
__global__ __launch_bounds__(kT) void idr_dots_kernel(int64_t n, int64_t ld, double *sc, int k, const int *flags,
                                                      const double *__restrict__ P, const double *__restrict__ g,
                                                      double *partials, unsigned *counter) {
    __shared__ double lds[S * (kT / 64)];
    if (flags[1]) return;
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *P2 = reinterpret_cast<const double2 *>(P);
    const double2 *g2 = reinterpret_cast<const double2 *>(g);
    double acc[S];
#pragma unroll
    for (int j = 0; j < S; ++j) acc[j] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 p[S];
#pragma unroll
        for (int j = 0; j < S; ++j) p[j] = P2[i + j * ld2];
        const double2 gv = g2[i];
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] = fma(p[j].y, gv.y, fma(p[j].x, gv.x, acc[j]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] = fma(P[n - 1 + j * ld], g[n - 1], acc[j]);
    }
    double q[S];
    if (!reduce_last<S>(acc, lds, partials, counter, q)) return;
    if (threadIdx.x != 0) return;
    if (k >= 0) {
        idr_book_q(q, sc, k, S);
    } else {
        for (int j = 0; j < S; ++j) sc[S_F + j] = q[j];
        idr_solve_c(sc, 0, S);
    }
}

// pass W: G_k -= sum_{i < NK} alpha_i G_i ; U_k -= sum_{i < NK} alpha_i U_i ; r -= beta G_k ; x += beta U_k ; (r, r).
// NK = k.  The last workgroup: the history entry, the stop test, c of position k + 1.
template <int NK>
__global__ __launch_bounds__(kT) void idr_w_kernel(int64_t n, int64_t ld, double *sc, int s, int *flags,
                                                   double *G, double *U, double *__restrict__ r,
                                                   double *__restrict__ x, double *partials, unsigned *counter, double *hist,
                                                   int hist_cap) {
    __shared__ double lds[kT / 64];
    if (flags[1]) return;
    double a[NK > 0 ? NK : 1];
#pragma unroll
    for (int j = 0; j < NK; ++j) a[j] = sc[S_ALPHA + j];
    const double beta = sc[S_BETA];
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *G2 = reinterpret_cast<const double2 *>(G);
    const double2 *U2 = reinterpret_cast<const double2 *>(U);
    double2 *Gk2 = reinterpret_cast<double2 *>(G) + NK * ld2;
    double2 *Uk2 = reinterpret_cast<double2 *>(U) + NK * ld2;
    double2 *r2 = reinterpret_cast<double2 *>(r);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 g[NK > 0 ? NK : 1], u[NK > 0 ? NK : 1];
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            g[j] = G2[i + j * ld2];
            u[j] = U2[i + j * ld2];
        }
        double2 gk = Gk2[i], uk = Uk2[i], rv = r2[i], xv = x2[i];
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            gk.x = fma(-a[j], g[j].x, gk.x);
            gk.y = fma(-a[j], g[j].y, gk.y);
            uk.x = fma(-a[j], u[j].x, uk.x);
            uk.y = fma(-a[j], u[j].y, uk.y);
        }
        rv.x = fma(-beta, gk.x, rv.x);
        rv.y = fma(-beta, gk.y, rv.y);
        xv.x = fma(beta, uk.x, xv.x);
        xv.y = fma(beta, uk.y, xv.y);
        if (NK > 0) {
            Gk2[i] = gk;
            Uk2[i] = uk;
        }
        r2[i] = rv;
        x2[i] = xv;
        acc[0] = fma(rv.y, rv.y, fma(rv.x, rv.x, acc[0]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        double *Gk = G + NK * ld, *Uk = U + NK * ld;
        double gk = Gk[i], uk = Uk[i];
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            gk = fma(-a[j], G[i + j * ld], gk);
            uk = fma(-a[j], U[i + j * ld], uk);
        }
        const double rv = fma(-beta, gk, r[i]);
        if (NK > 0) {
            Gk[i] = gk;
            Uk[i] = uk;
        }
        r[i] = rv;
        x[i] = fma(beta, uk, x[i]);
        acc[0] = fma(rv, rv, acc[0]);
    }
    double rr[1];
    if (!reduce_last<1>(acc, lds, partials, counter, rr)) return;
    // every other workgroup has read its scalars and the stop flag before it arrived: they may change now
    if (threadIdx.x != 0) return;
    idr_book_norm(rr[0], sc, flags, hist, hist_cap);
    idr_solve_c(sc, NK + 1, s);
}

// ---- position s -----------------------------------------------------------------------------------------------------
// pass T: (t, t) and (t, r); the last workgroup: omega = (t, r) / (t, t), scaled up where t and r are close to orthogonal
__global__ __launch_bounds__(kT) void idr_tt_kernel(int64_t n, double *sc, const int *flags, const double *__restrict__ t,
                                                    const double *__restrict__ r, double *partials, unsigned *counter) {
    __shared__ double lds[2 * (kT / 64)];
    if (flags[1]) return;
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *t2 = reinterpret_cast<const double2 *>(t);
    const double2 *r2 = reinterpret_cast<const double2 *>(r);
    double acc[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 tv = t2[i], rv = r2[i];
        acc[0] = fma(tv.y, tv.y, fma(tv.x, tv.x, acc[0]));
        acc[1] = fma(tv.y, rv.y, fma(tv.x, rv.x, acc[1]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        acc[0] = fma(t[n - 1], t[n - 1], acc[0]);
        acc[1] = fma(t[n - 1], r[n - 1], acc[1]);
    }
    double d[2];
    if (!reduce_last<2>(acc, lds, partials, counter, d)) return;
    if (threadIdx.x != 0) return;
    {
#pragma clang fp contract(off)
        const double tt = d[0], tr = d[1];
        double omega = tr / tt; // tt = 0: the published breakdown, NaN or Inf from here on
        const double rho = fabs(tr) / (sqrt(tt) * sc[S_NORM]);
        if (rho < 0.7) omega = omega * 0.7 / rho;
        sc[S_OMEGA] = omega;
    }
}

// pass O: x += omega vh ; r -= omega t ; (r, r) and f = P^T r.  The last workgroup: the history entry, the stop test, f and
// the c of position 0.
template <int S>
__global__ __launch_bounds__(kT) void idr_o_kernel(int64_t n, int64_t ld, double *sc, int *flags, const double *__restrict__ P,
                                                   const double *vh, const double *__restrict__ t, double *r,
                                                   double *__restrict__ x, double *partials, unsigned *counter, double *hist,
                                                   int hist_cap) {
    __shared__ double lds[(S + 1) * (kT / 64)];
    if (flags[1]) return;
    const double omega = sc[S_OMEGA];
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *P2 = reinterpret_cast<const double2 *>(P);
    const double2 *v2 = reinterpret_cast<const double2 *>(vh);
    const double2 *t2 = reinterpret_cast<const double2 *>(t);
    double2 *r2 = reinterpret_cast<double2 *>(r);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double acc[S + 1];
#pragma unroll
    for (int j = 0; j <= S; ++j) acc[j] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 p[S];
#pragma unroll
        for (int j = 0; j < S; ++j) p[j] = P2[i + j * ld2];
        const double2 vv = v2[i], tv = t2[i]; // (vh may be r itself: read before r is written)
        double2 rv = r2[i], xv = x2[i];
        xv.x = fma(omega, vv.x, xv.x);
        xv.y = fma(omega, vv.y, xv.y);
        rv.x = fma(-omega, tv.x, rv.x);
        rv.y = fma(-omega, tv.y, rv.y);
        x2[i] = xv;
        r2[i] = rv;
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] = fma(p[j].y, rv.y, fma(p[j].x, rv.x, acc[j]));
        acc[S] = fma(rv.y, rv.y, fma(rv.x, rv.x, acc[S]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double vv = vh[i];
        const double rv = fma(-omega, t[i], r[i]);
        x[i] = fma(omega, vv, x[i]);
        r[i] = rv;
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] = fma(P[i + j * ld], rv, acc[j]);
        acc[S] = fma(rv, rv, acc[S]);
    }
    double d[S + 1];
    if (!reduce_last<S + 1>(acc, lds, partials, counter, d)) return;
    if (threadIdx.x != 0) return;
    idr_book_norm(d[S], sc, flags, hist, hist_cap);
    for (int j = 0; j < S; ++j) sc[S_F + j] = d[j];
    idr_solve_c(sc, 0, S);
}

// LAUNCH(N) with the runtime N as a constant: 1 .. 8 (column counts, s), 0 .. 7 (k)
#define BIS_IDR_CASES_1_7(LAUNCH)                                                                                              \
    case 1: LAUNCH(1); break;                                                                                                  \
    case 2: LAUNCH(2); break;                                                                                                  \
    case 3: LAUNCH(3); break;                                                                                                  \
    case 4: LAUNCH(4); break;                                                                                                  \
    case 5: LAUNCH(5); break;                                                                                                  \
    case 6: LAUNCH(6); break;                                                                                                  \
    case 7: LAUNCH(7); break;
#define BIS_IDR_DISPATCH_1_8(N, LAUNCH)                                                                                        \
    switch (N) {                                                                                                               \
        BIS_IDR_CASES_1_7(LAUNCH)                                                                                              \
    case 8: LAUNCH(8); break;                                                                                                  \
    }
#define BIS_IDR_DISPATCH_0_7(N, LAUNCH)                                                                                        \
    switch (N) {                                                                                                               \
    case 0: LAUNCH(0); break;                                                                                                  \
        BIS_IDR_CASES_1_7(LAUNCH)                                                                                              \
    }

// f = P^T r and the c of position 0 (k < 0), or pass Q of position k
void idr_launch_dots(bis_ctx *ctx, const bis_idr *h, int k, const double *g, int grid) {
#define BIS_IDR_L(S)                                                                                                           \
    hipLaunchKernelGGL((idr_dots_kernel<S>), dim3(grid), dim3(kT), 0, ctx->stream, h->n, h->ld, h->sc, k,                      \
                       (const int *)h->flags, (const double *)h->P, g, ctx->partials, h->counters)
    BIS_IDR_DISPATCH_1_8(h->s, BIS_IDR_L)
#undef BIS_IDR_L
}

} // namespace

extern "C" {

bis_status bis_idr_create(bis_ctx *ctx, const bis_mat *A, const double *b, double *x, int s, bis_idr **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && b && x && out && s >= 1 && s <= kMaxS, "bis_idr_create: bad arguments (1 <= s <= 8)");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_idr_create: square matrix required");
    BIS_REQUIRE(ctx, aligned16(b) && aligned16(x), "bis_idr_create: b and x must be 16-byte aligned");
    bis_idr *h = new bis_idr;
    h->A = A; h->b = b; h->x = x;
    h->n = A->n_rows;
    h->ld = (h->n + 1) & ~(int64_t)1;
    h->s = s;
    bis_status st = BIS_OK;
    for (double **p : {&h->r, &h->v, &h->t})
        if (st == BIS_OK) st = bis_vec_alloc(ctx, h->ld, p);
    for (double **p : {&h->P, &h->G, &h->U})
        if (st == BIS_OK) st = bis_vec_alloc(ctx, h->ld * s, p);
    if (st == BIS_OK) st = bis_vec_alloc(ctx, S_COUNT, &h->sc);
    if (st == BIS_OK) st = bis_solver_core_alloc(ctx, h, 4, 1, 1, kCounterSet);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, (size_t)(kMaxS + 1) * kMaxReduceBlocks);
    if (st == BIS_OK && h->n > 0) {
        hipLaunchKernelGGL(idr_shadow_kernel, dim3(bis_pair_grid(2 * h->ld * s, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, h->P, h->n, h->ld, s);
        if (hipGetLastError() != hipSuccess) st = BIS_ERR_HIP;
    }
    if (st != BIS_OK) { bis_idr_destroy(ctx, h); return st; }
    *out = h;
    return BIS_OK;
}

bis_status bis_idr_set_preconditioner(bis_ctx *ctx, bis_idr *h, int precond_type, const bis_mat *L_strict,
                                      const bis_mat *U_strict, const double *A_D, const double *A_D_inv, const double *L_D,
                                      const double *U_D, int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (!h) return bis_pc_no_handle(ctx, "bis_idr", 0, precond_type);
    return bis_pc_bind(ctx, &h->pc, {"bis_idr", h->n, h->ld, 0, bis_solver_live(*h), 0},
                       {precond_type, L_strict, U_strict, A_D, A_D_inv, L_D, U_D, outer_iters, inner_iters}, {});
}

bis_status bis_idr_set_shadow(bis_ctx *ctx, bis_idr *h, const double *P_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, h && (P_host || h->n == 0), "bis_idr_set_shadow: bad arguments");
    BIS_REQUIRE(ctx, !bis_solver_live(*h), "bis_idr_set_shadow: call it before bis_idr_init / bis_idr_iterate");
    if (h->n == 0) return BIS_OK;
    BIS_HIP_CHECK(ctx, hipMemcpy2DAsync(h->P, sizeof(double) * (size_t)h->ld, P_host, sizeof(double) * (size_t)h->n,
                                        sizeof(double) * (size_t)h->n, (size_t)h->s, hipMemcpyHostToDevice, ctx->stream));
    BIS_SYNC_CHECK(ctx); // the caller's array is free again
    return BIS_OK;
}

bis_status bis_idr_destroy(bis_ctx *ctx, bis_idr *h) {
    BIS_CTX_OK(ctx);
    if (!h) return BIS_OK;
    hipStreamSynchronize(ctx->stream);
    for (double *p : {h->r, h->v, h->t, h->P, h->G, h->U, h->sc}) hipFree(p);
    bis_solver_core_free(h);
    delete h;
    return BIS_OK;
}

bis_status bis_idr_init(bis_ctx *ctx, bis_idr *h, double tol, double *r0_norm_host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, h, "bis_idr_init: null handle");
    h->enqueued = 0;
    const int64_t n = h->n;
    if (n == 0) {
        if (r0_norm_host) *r0_norm_host = 0.0;
        return BIS_OK;
    }
    bis_status st = bis_compute_residual(ctx, h->A, h->x, h->b, h->r, h->v);
    double r0 = 0.0;
    if (st == BIS_OK) st = bis_euclidean_vec_norm(ctx, h->r, n, &r0);
    if (st == BIS_OK) st = bis_ensure_partials(ctx, (size_t)(kMaxS + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) return st;
    double sc[S_COUNT] = {0};
    sc[S_OMEGA] = 1.0;
    sc[S_NORM] = r0;
    sc[S_STOP] = tol * r0;
    for (int i = 0; i < kMaxS; ++i) sc[S_M + kMaxS * i + i] = 1.0;
    const int flags[4] = {0, 0, 0, 0};
    const size_t block = sizeof(double) * (size_t)h->ld * h->s;
    BIS_HIP_CHECK(ctx, hipMemsetAsync(h->G, 0, block, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(h->U, 0, block, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(h->counters, 0, sizeof(unsigned) * kCounterSet, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(h->sc, sc, sizeof sc, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(h->flags, flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(h->hist, &r0, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    idr_launch_dots(ctx, h, -1, h->r, bis_pair_grid(n, kMaxReduceBlocks)); // f = P^T r, c = f (M = I)
    BIS_HIP_CHECK(ctx, hipGetLastError());
    BIS_SYNC_CHECK(ctx);
    h->initialised = true;
    if (r0_norm_host) *r0_norm_host = r0;
    return BIS_OK;
}

bis_status bis_idr_iterate(bis_ctx *ctx, bis_idr *h, int n_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, h && n_iters >= 0 && h->enqueued + n_iters < kMaxIters, "bis_idr_iterate: bad arguments");
    const int64_t n = h->n, ld = h->ld;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, h->initialised, "bis_idr_iterate: call bis_idr_init first");
    const int s = h->s, g = bis_pair_grid(n, kMaxReduceBlocks), g_wide = bis_pair_grid(n, kMaxEwBlocks);
    const bool pc = h->pc.type != BIS_PC_NONE;
    bis_status st = bis_ensure_partials(ctx, (size_t)(kMaxS + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) return st;
    bis_stop_guard stop_guard(ctx, h->flags); // the SpMV returns at once when the solve has stopped
    const int *flags = h->flags;
    const double *sc = h->sc;
    for (int done = 0; done < n_iters; ++done) {
        const int k = (h->enqueued + done) % (s + 1);
        // (after a failure the device's count stays behind the host's position: call bis_idr_init again)
        if (k < s) {
            double *Gk = h->G + k * ld, *Uk = h->U + k * ld;
            const int nc = s - k;
            if (!pc) {
#define BIS_IDR_L(NC)                                                                                                          \
    hipLaunchKernelGGL((idr_v_kernel<NC, true>), dim3(g_wide), dim3(kT), 0, ctx->stream, n, ld, sc, k, flags,                  \
                       (const double *)h->r, (const double *)Gk, Uk, h->v)
                BIS_IDR_DISPATCH_1_8(nc, BIS_IDR_L)
#undef BIS_IDR_L
            } else {
#define BIS_IDR_L(NC)                                                                                                          \
    hipLaunchKernelGGL((idr_v_kernel<NC, false>), dim3(g_wide), dim3(kT), 0, ctx->stream, n, ld, sc, k, flags,                 \
                       (const double *)h->r, (const double *)Gk, (double *)nullptr, h->v)
                BIS_IDR_DISPATCH_1_8(nc, BIS_IDR_L)
#undef BIS_IDR_L
                st = bis_pc_apply(ctx, h->pc, n, 0, h->t, h->v);
                if (st != BIS_OK) { h->enqueued += done; return st; }
#define BIS_IDR_L(NC)                                                                                                          \
    hipLaunchKernelGGL((idr_u_kernel<NC>), dim3(g_wide), dim3(kT), 0, ctx->stream, n, ld, sc, k, flags, (const double *)h->t, Uk)
                BIS_IDR_DISPATCH_1_8(nc, BIS_IDR_L)
#undef BIS_IDR_L
            }
            st = bis_spmv_launch(ctx, h->A, Uk, Gk, nullptr, nullptr);
            if (st != BIS_OK) { h->enqueued += done; return st; }
            idr_launch_dots(ctx, h, k, Gk, g);
#define BIS_IDR_L(NK)                                                                                                          \
    hipLaunchKernelGGL((idr_w_kernel<NK>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, h->sc, s, h->flags,                       \
                       h->G, h->U, h->r, h->x, ctx->partials, h->counters, h->hist, h->hist_cap)
            BIS_IDR_DISPATCH_0_7(k, BIS_IDR_L)
#undef BIS_IDR_L
        } else {
            const double *vh = h->r;
            if (pc) {
                st = bis_pc_apply(ctx, h->pc, n, 0, h->v, h->r); // (with outer_iters > 1 the apply restores its input)
                if (st != BIS_OK) { h->enqueued += done; return st; }
                vh = h->v;
            }
            st = bis_spmv_launch(ctx, h->A, vh, h->t, nullptr, nullptr);
            if (st != BIS_OK) { h->enqueued += done; return st; }
            hipLaunchKernelGGL(idr_tt_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, h->sc, flags, (const double *)h->t,
                               (const double *)h->r, ctx->partials, h->counters);
#define BIS_IDR_L(S)                                                                                                           \
    hipLaunchKernelGGL((idr_o_kernel<S>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, h->sc, h->flags, (const double *)h->P,     \
                       vh, (const double *)h->t, h->r, h->x, ctx->partials, h->counters, h->hist, h->hist_cap)
            BIS_IDR_DISPATCH_1_8(s, BIS_IDR_L)
#undef BIS_IDR_L
        }
    }
    h->enqueued += n_iters; // the launches were issued whatever the check below says: the position keeps matching the device's count
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_idr_status(bis_ctx *ctx, bis_idr *h, int *iters, int *converged, double *hist_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, h, "bis_idr_status: null handle");
    int flags[4] = {0, 0, 0, 0};
    if (bis_status st = bis_solver_read_flags(ctx, *h, 0, 4, flags)) return st;
    if (iters) *iters = flags[0];
    if (converged) *converged = flags[2];
    if (hist_host && hist_cap > 0 && h->initialised) return bis_solver_copy_hist(ctx, *h, 0, std::min(flags[0] + 1, hist_cap), hist_host);
    return BIS_OK;
}

} // extern "C"
