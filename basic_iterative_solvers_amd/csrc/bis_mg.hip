// bis_mg.hip -- aggregation multigrid preconditioner (unsmoothed aggregation, V(nu,nu) with Jacobi-type smoothing); not in the
// reference.  The definitions a restatement needs are in include/bis_hip.h; this file follows them step by step.
//
// Setup (bis_mg_create, blocking, all on the device): per level the smoother weights and the diagonal check, the aggregate
// of every row (from the grid hint, or a maximal independent set of the off-diagonal pattern found in rounds with one
// counter read per round), the members lists (a stable radix sort of (aggregate, row)), and the Galerkin operator
// P^T A P for the piecewise-constant P: a stable 64-bit radix sort of (agg[r] << 32 | agg[c], value) over the fine entries,
// then one lane per coarse entry sums its run left to right.  No floating-point atomics and no inter-workgroup waits: two
// calls give the same bits.
//
// Smoothed aggregation (bis_mg_create_smoothed): the same levels, aggregates and weights, but every transition gets a
// Jacobi-smoothed prolongator P = T - omega_l D^-1 A T (Q = A T by bis_spgemm, then P from Q in place), R = P^T
// (bis_mat_transpose) and the Galerkin operator R (A P) by two more products; the cycle then restricts with a wave per row
// of R and prolongs with a lane per row of P.
//
// Apply (bis_mg_apply, stream-ordered, allocates nothing): per level bis_spmv and three streaming kernels -- relax
// (x += w o (b - y), and its from-zero form x = w o b), restrict (r_c[I] = sum over the members of b_i - y_i, a lane per
// aggregate) and prolong (x_i += scale e_c[agg[i]]).  Products, subtractions and additions are rounded separately.
//
// Cycles (bis_mg_set_cycle, blocking, allocates the extra scratch): V is the above.  A W or K transition replaces the one
// coarse solve e_c = cycle(l + 1, r_c) by two of them: W adds the cycle of the residual r_c - A e_1; K (Notay's K-cycle) takes
// two steps of a Krylov method preconditioned by the cycle of level l + 1 -- conjugate directions (for CG) or GCR.  Three more
// streaming kernels: r = a - s b with s on the device, the multi-dot pass (2 or 3 sums over 3 or 4 operands in one read, the last
// workgroup to arrive sums the partials in index order and computes the step's coefficients into the transition's own device
// scalars) and the combine x = c1 x + c2 d.  The launch sequence is fixed, nothing is read back.
//
// Chebyshev smoother (bis_mg_set_smoother, blocking, allocates one more vector d per level): every sweep becomes one polynomial
// of degree m in W A for [lambda_max / ratio, lambda_max] -- m SpMVs and m streaming steps d = c1 d + c2 w o (b - y), x += d,
// the first step of a level visit from x = 0 without its SpMV.  lambda_max per level: the row-sum bound max_i w_i sum_j |a_ij|
// (one kernel and a one-workgroup maximum), optionally tightened by a power iteration run with the public single-vector calls;
// the coefficients are computed on the host and travel as kernel arguments.  A hierarchy that never saw the call launches what
// it always did.
#include "bis_internal.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>

constexpr int kMgMaxDegree = 8;

struct bis_mg_level {
    const bis_mat *A = nullptr; // level 0: the caller's matrix; otherwise `owned`
    bis_mat *owned = nullptr;
    int64_t n = 0;
    int kind = 0;               // aggregates towards the next level: 0 none (the coarsest level), 1 grid, 2 MIS
    int64_t n_coarse = 0;
    double *w = nullptr;        // smoother weights [n]
    int32_t *agg = nullptr;     // [n] aggregate of every row
    int32_t *agg_ptr = nullptr; // [n_coarse + 1]
    int32_t *agg_idx = nullptr; // [n] members by aggregate, ascending rows inside one
    double *x = nullptr, *b = nullptr, *y = nullptr; // cycle scratch; level 0 owns y only (x, b are the caller's vectors)
    // the coarse level of a W or K transition only (bis_mg_set_cycle): kr = r_2 or r~, kd = e_2 or d, kv = v (K; w lives in y)
    double *kr = nullptr, *kd = nullptr, *kv = nullptr;
    // a smoothed hierarchy only (bis_mg_create_smoothed): the transfer operators towards the next level and their omega_l
    bis_mat *P = nullptr, *R = nullptr;
    double pomega = 0.0;
    // the Chebyshev smoother only (bis_mg_set_smoother): cd = the polynomial's direction d, live inside one smoothing call;
    // cheb_degree > 0 is what switches this level's sweeps over
    double *cd = nullptr;
    int cheb_degree = 0;
    double cheb_c1[kMgMaxDegree] = {0}, cheb_c2[kMgMaxDegree] = {0};
    double sp_bound = 0.0, sp_estimate = 0.0, sp_lmax = 0.0, sp_lmin = 0.0;
};

struct bis_mg {
    bis_mg_params p;
    bool smoothed = false;      // bis_mg_create_smoothed made it
    double prolong_omega = 0.0; // ... with this factor (4/3 for the caller's 0)
    std::vector<bis_mg_level> lv;
    bis_mat *operand = nullptr;
    double *b0 = nullptr; // level 0: the copy of the right-hand side when out aliases in
    int cycle = BIS_MG_CYCLE_V, cycle_levels = 0;
    bis_mg_smoother sm = {BIS_MG_SMOOTH_JACOBI, 0, 0.0, 0, 0.0};
    // W and K transitions (allocated by the first bis_mg_set_cycle that leaves V)
    double *ksc = nullptr;       // device scalars: [0, 4) = {1, 1, 0, 1}: W's constants; transition t: [kMgScBase + kMgScPer t, ...), MG_SC_*
    double *kpartials = nullptr; // [3 kMaxReduceBlocks] the multi-dot pass' per-workgroup sums
    unsigned *kcounters = nullptr; // [4 + kArriveSubs] its arrival counters (every launch re-arms them)
};

namespace {

constexpr int kMgT = 256;
constexpr int kMgMaxBlocks = kMaxEwBlocks; // elementwise passes: the wide grid of bis_blas1.hip's kernels
constexpr int kMgMaxLevels = 16;
// a transition's device scalars: c1, c2 and the "e_c = 0" flag are adjacent (the combine kernel reads the three)
enum { MG_SC_C1 = 0, MG_SC_C2, MG_SC_ZERO, MG_SC_S1, MG_SC_RHO1, MG_SC_COUNT };
constexpr int kMgScBase = 8, kMgScPer = 8;

typedef double mg_v2d __attribute__((ext_vector_type(2)));
typedef int mg_v2i __attribute__((ext_vector_type(2)));

inline int mg_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kMgT - 1) / kMgT, kMgMaxBlocks)); }

// ---- the cycle's kernels -----------------------------------------------------------------------------------------------
// x = w o b: the first sweep from x = 0 (one rounding).  Inputs are touched once per pass: non-temporal loads; the store
// stays plain -- the next kernel (an SpMV, or the prolongation of the level above) reads what this one wrote.
template <bool VEC>
__global__ __launch_bounds__(kMgT) void mg_relax0_kernel(double *x, const double *w, const double *b, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *x2 = reinterpret_cast<mg_v2d *>(x);
        const mg_v2d *w2 = reinterpret_cast<const mg_v2d *>(w), *b2 = reinterpret_cast<const mg_v2d *>(b);
        for (; i < n2; i += stride) {
            const mg_v2d wv = __builtin_nontemporal_load(w2 + i), bv = __builtin_nontemporal_load(b2 + i);
            mg_v2d r;
            r.x = __dmul_rn(wv.x, bv.x);
            r.y = __dmul_rn(wv.y, bv.y);
            x2[i] = r;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = __dmul_rn(w[n - 1], b[n - 1]);
    } else {
        for (; i < n; i += stride) x[i] = __dmul_rn(__builtin_nontemporal_load(w + i), __builtin_nontemporal_load(b + i));
    }
}

// x += w o (b - y), y = A x: t = b - y, u = w t, x = x + u, each rounded
__device__ __forceinline__ double mg_relax1(double x, double w, double b, double y) { return __dadd_rn(x, __dmul_rn(w, __dsub_rn(b, y))); }

template <bool VEC>
__global__ __launch_bounds__(kMgT) void mg_relax_kernel(double *x, const double *w, const double *b, const double *y, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *x2 = reinterpret_cast<mg_v2d *>(x);
        const mg_v2d *w2 = reinterpret_cast<const mg_v2d *>(w), *b2 = reinterpret_cast<const mg_v2d *>(b),
                     *y2 = reinterpret_cast<const mg_v2d *>(y);
        for (; i < n2; i += stride) {
            const mg_v2d xv = __builtin_nontemporal_load(x2 + i), wv = __builtin_nontemporal_load(w2 + i),
                         bv = __builtin_nontemporal_load(b2 + i), yv = __builtin_nontemporal_load(y2 + i);
            mg_v2d r;
            r.x = mg_relax1(xv.x, wv.x, bv.x, yv.x);
            r.y = mg_relax1(xv.y, wv.y, bv.y, yv.y);
            x2[i] = r;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = mg_relax1(x[n - 1], w[n - 1], b[n - 1], y[n - 1]);
    } else {
        for (; i < n; i += stride)
            x[i] = mg_relax1(__builtin_nontemporal_load(x + i), __builtin_nontemporal_load(w + i), __builtin_nontemporal_load(b + i),
                             __builtin_nontemporal_load(y + i));
    }
}

// r_c[I] = sum over the members i of aggregate I, ascending, of (b_i - y_i): a lane per aggregate, the first difference
// starts the sum, every further one is added to it (each subtraction and each addition rounded)
__global__ __launch_bounds__(kMgT) void mg_restrict_kernel(const int32_t *__restrict__ agg_ptr, const int32_t *__restrict__ agg_idx,
                                                           const double *__restrict__ b, const double *__restrict__ y,
                                                           double *__restrict__ rc, int64_t nc) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t I = (int64_t)blockIdx.x * kMgT + threadIdx.x; I < nc; I += stride) {
        const int32_t s = agg_ptr[I], e = agg_ptr[I + 1];
        double acc = 0.0;
        for (int32_t k = s; k < e; ++k) {
            const int32_t i = __builtin_nontemporal_load(agg_idx + k);
            const double d = __dsub_rn(__builtin_nontemporal_load(b + i), __builtin_nontemporal_load(y + i));
            acc = k == s ? d : __dadd_rn(acc, d);
        }
        rc[I] = acc;
    }
}

// x_i += scale e_c[agg[i]] (the product rounded, then the sum)
template <bool VEC>
__global__ __launch_bounds__(kMgT) void mg_prolong_kernel(double *x, const int32_t *__restrict__ agg, const double *__restrict__ ec,
                                                          double scale, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *x2 = reinterpret_cast<mg_v2d *>(x);
        const mg_v2i *a2 = reinterpret_cast<const mg_v2i *>(agg);
        for (; i < n2; i += stride) {
            const mg_v2d xv = __builtin_nontemporal_load(x2 + i);
            const mg_v2i av = __builtin_nontemporal_load(a2 + i);
            mg_v2d r;
            r.x = __dadd_rn(xv.x, __dmul_rn(scale, ec[av.x]));
            r.y = __dadd_rn(xv.y, __dmul_rn(scale, ec[av.y]));
            x2[i] = r;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = __dadd_rn(x[n - 1], __dmul_rn(scale, ec[agg[n - 1]]));
    } else {
        for (; i < n; i += stride) x[i] = __dadd_rn(__builtin_nontemporal_load(x + i), __dmul_rn(scale, ec[agg[i]]));
    }
}

// ---- the transfers of a smoothed hierarchy ----------------------------------------------------------------------------
__device__ __forceinline__ int64_t mg_rp_at(const void *rp, int w64, int64_t i) {
    return w64 ? static_cast<const int64_t *>(rp)[i] : (int64_t) static_cast<const int32_t *>(rp)[i];
}

// r_c[I] = sum over row I of R of R_t (b - y)_{col t}: a wave per row.  Lane q sums the products at q, q + 64, ... in that
// order from 0; the 64 sums are added lane q + 32 to lane q, then + 16, ..., + 1.  b and y are read directly: nothing is
// materialised between the SpMV and this pass.
__global__ __launch_bounds__(kMgT) void mg_restrict_sa_kernel(const void *rp, int w64, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                              const double *__restrict__ b, const double *__restrict__ y, double *__restrict__ rc,
                                                              int64_t nc) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kMgT / 64);
    for (int64_t I = (int64_t)blockIdx.x * (kMgT / 64) + (threadIdx.x >> 6); I < nc; I += waves) {
        double acc = 0.0;
        for (int64_t t = mg_rp_at(rp, w64, I) + lane, e = mg_rp_at(rp, w64, I + 1); t < e; t += 64) {
            const int32_t c = __builtin_nontemporal_load(col + t);
            acc = __dadd_rn(acc, bis_mul_sep(__builtin_nontemporal_load(val + t), __dsub_rn(b[c], y[c])));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc = __dadd_rn(acc, __shfl_down(acc, off, 64));
        if (lane == 0) rc[I] = acc;
    }
}

// x_i += scale (sum over row i of P of P_t e_c[col t]): a lane per row (the rows are short), left to right, the first
// product starting the sum; then the product with scale and the sum with x_i, each rounded
__global__ __launch_bounds__(kMgT) void mg_prolong_sa_kernel(double *x, const void *rp, int w64, const int32_t *__restrict__ col,
                                                             const double *__restrict__ val, const double *__restrict__ ec, double scale, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        const int64_t s = mg_rp_at(rp, w64, i), e = mg_rp_at(rp, w64, i + 1);
        if (s == e) continue;
        double acc = bis_mul_sep(__builtin_nontemporal_load(val + s), ec[__builtin_nontemporal_load(col + s)]);
        for (int64_t t = s + 1; t < e; ++t)
            acc = __dadd_rn(acc, bis_mul_sep(__builtin_nontemporal_load(val + t), ec[__builtin_nontemporal_load(col + t)]));
        x[i] = __dadd_rn(x[i], bis_mul_sep(scale, acc));
    }
}

// ---- the W and K transitions' kernels ----------------------------------------------------------------------------------
// r = a - s b, s read from device memory when the kernel runs (the product rounded, then the difference): K's
// r~ = r_c - s1 v, and W's r_2 = r_c - y with s = 1 (1 y is y: the plain difference)
template <bool VEC>
__global__ __launch_bounds__(kMgT) void mg_axmy_kernel(double *r, const double *a, const double *b, const double *s_dev, int64_t n) {
    const double s = *s_dev;
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *r2 = reinterpret_cast<mg_v2d *>(r);
        const mg_v2d *a2 = reinterpret_cast<const mg_v2d *>(a), *b2 = reinterpret_cast<const mg_v2d *>(b);
        for (; i < n2; i += stride) {
            const mg_v2d av = __builtin_nontemporal_load(a2 + i), bv = __builtin_nontemporal_load(b2 + i);
            mg_v2d o;
            o.x = __dsub_rn(av.x, __dmul_rn(s, bv.x));
            o.y = __dsub_rn(av.y, __dmul_rn(s, bv.y));
            r2[i] = o;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) r[n - 1] = __dsub_rn(a[n - 1], __dmul_rn(s, b[n - 1]));
    } else {
        for (; i < n; i += stride) r[i] = __dsub_rn(__builtin_nontemporal_load(a + i), __dmul_rn(s, __builtin_nontemporal_load(b + i)));
    }
}

// x_i = (c1 x_i) + (c2 d_i), coef = {c1, c2, zero}; zero != 0: x = 0 whatever x and d hold (the guarded K step).  W's
// e_1 + e_2 is this with {1, 1, 0}: both products are exact, the sum is the plain one.
__device__ __forceinline__ double mg_combine1(double x, double d, double c1, double c2) { return __dadd_rn(__dmul_rn(c1, x), __dmul_rn(c2, d)); }

template <bool VEC>
__global__ __launch_bounds__(kMgT) void mg_combine_kernel(double *x, const double *d, const double *coef, int64_t n) {
    const double c1 = coef[MG_SC_C1], c2 = coef[MG_SC_C2];
    const bool zero = coef[MG_SC_ZERO] != 0.0;
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *x2 = reinterpret_cast<mg_v2d *>(x);
        const mg_v2d *d2 = reinterpret_cast<const mg_v2d *>(d);
        for (; i < n2; i += stride) {
            mg_v2d o;
            o.x = 0.0;
            o.y = 0.0;
            if (!zero) {
                const mg_v2d xv = __builtin_nontemporal_load(x2 + i), dv = __builtin_nontemporal_load(d2 + i);
                o.x = mg_combine1(xv.x, dv.x, c1, c2);
                o.y = mg_combine1(xv.y, dv.y, c1, c2);
            }
            x2[i] = o;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = zero ? 0.0 : mg_combine1(x[n - 1], d[n - 1], c1, c2);
    } else {
        for (; i < n; i += stride)
            x[i] = zero ? 0.0 : mg_combine1(__builtin_nontemporal_load(x + i), __builtin_nontemporal_load(d + i), c1, c2);
    }
}

// The K step's dot products in one pass.  With t = GCR ? q : p:
//   NS = 2, operands (p, q, -, r) = (c, v, -, r_c):   (t, v), (t, r_c)             -> rho1, alpha1 -> s1
//   NS = 3, operands (p, q, u, r) = (d, w, v, r~):    (t, v), (t, w), (t, r~)      -> gamma, beta, alpha2 -> c1, c2
// A lane sums its products by fused multiply-add in index order, the workgroup's lanes are summed by block_sum, and the
// last workgroup to arrive sums the workgroups' partials in index order: the bits depend on (n, the data) only.  No
// workgroup waits for another.  Thread 0 of that workgroup then does the step's scalar algebra (every operation rounded).
template <int NS>
__device__ __forceinline__ void mg_kdots_acc(double (&acc)[3], double p, double q, double u, double r, bool gcr) {
    const double t = gcr ? q : p;
    if (NS == 2) {
        acc[0] = fma(t, q, acc[0]);
        acc[1] = fma(t, r, acc[1]);
    } else {
        acc[0] = fma(t, u, acc[0]);
        acc[1] = fma(t, q, acc[1]);
        acc[2] = fma(t, r, acc[2]);
    }
}

template <int NS, bool VEC>
__global__ __launch_bounds__(kMgT) void mg_kdots_kernel(const double *p, const double *q, const double *u, const double *r, int64_t n, int gcr_,
                                                        double *partials, unsigned *counters, double *sc) {
    __shared__ double lds[kMgT / 64];
    __shared__ bool last;
    const bool gcr = gcr_ != 0;
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (VEC) {
        const int64_t n2 = n >> 1;
        const mg_v2d *p2 = reinterpret_cast<const mg_v2d *>(p), *q2 = reinterpret_cast<const mg_v2d *>(q),
                     *u2 = reinterpret_cast<const mg_v2d *>(u), *r2 = reinterpret_cast<const mg_v2d *>(r);
        for (; i < n2; i += stride) {
            const mg_v2d pv = __builtin_nontemporal_load(p2 + i), qv = __builtin_nontemporal_load(q2 + i),
                         rv = __builtin_nontemporal_load(r2 + i);
            mg_v2d uv = qv;
            if (NS == 3) uv = __builtin_nontemporal_load(u2 + i);
            mg_kdots_acc<NS>(acc, pv.x, qv.x, uv.x, rv.x, gcr);
            mg_kdots_acc<NS>(acc, pv.y, qv.y, uv.y, rv.y, gcr);
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) mg_kdots_acc<NS>(acc, p[n - 1], q[n - 1], NS == 3 ? u[n - 1] : 0.0, r[n - 1], gcr);
    } else {
        for (; i < n; i += stride)
            mg_kdots_acc<NS>(acc, __builtin_nontemporal_load(p + i), __builtin_nontemporal_load(q + i),
                             NS == 3 ? __builtin_nontemporal_load(u + i) : 0.0, __builtin_nontemporal_load(r + i), gcr);
    }
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        if (k) __syncthreads();
        s[k] = block_sum<kMgT>(acc[k], lds);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) publish(partials + (size_t)k * kMaxReduceBlocks + blockIdx.x, s[k]);
        last = arrive_last2(counters, counters + 4, blockIdx.x, gridDim.x);
    }
    __syncthreads();
    if (!last) return;
    double tot[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double a = 0.0;
        for (int b = threadIdx.x; b < (int)gridDim.x; b += kMgT) a += fetch(partials + (size_t)k * kMaxReduceBlocks + b);
        __syncthreads();
        tot[k] = block_sum<kMgT>(a, lds);
    }
    if (threadIdx.x != 0) return;
    if (NS == 2) {
        const double rho1 = tot[0], alpha1 = tot[1];
        const bool bad = rho1 == 0.0 || !(fabs(rho1) <= DBL_MAX); // zero or not finite: e_c = 0
        sc[MG_SC_RHO1] = rho1;
        sc[MG_SC_ZERO] = bad ? 1.0 : 0.0;
        sc[MG_SC_S1] = bad ? 0.0 : __ddiv_rn(alpha1, rho1);
        sc[MG_SC_C1] = 0.0;
        sc[MG_SC_C2] = 0.0;
    } else {
        const double gamma = tot[0], beta = tot[1], alpha2 = tot[2], rho1 = sc[MG_SC_RHO1], s1 = sc[MG_SC_S1];
        double c1 = 0.0, c2 = 0.0;
        if (sc[MG_SC_ZERO] == 0.0) {
            const double rho2 = __dsub_rn(beta, __ddiv_rn(__dmul_rn(gamma, gamma), rho1));
            c1 = s1;
            if (rho2 > 0.0) { // (false for NaN)
                c2 = __ddiv_rn(alpha2, rho2);
                c1 = __dsub_rn(s1, __ddiv_rn(__dmul_rn(gamma, c2), rho1));
            }
        }
        sc[MG_SC_C1] = c1;
        sc[MG_SC_C2] = c2;
    }
}

bis_status launch_relax0(bis_ctx *ctx, double *x, const double *w, const double *b, int64_t n) {
    const bool vec = aligned16(x) && aligned16(w) && aligned16(b) && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
    if (vec) hipLaunchKernelGGL((mg_relax0_kernel<true>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, w, b, n);
    else hipLaunchKernelGGL((mg_relax0_kernel<false>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, w, b, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}
bis_status launch_relax(bis_ctx *ctx, double *x, const double *w, const double *b, const double *y, int64_t n) {
    const bool vec = aligned16(x) && aligned16(w) && aligned16(b) && aligned16(y) && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
    if (vec) hipLaunchKernelGGL((mg_relax_kernel<true>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, w, b, y, n);
    else hipLaunchKernelGGL((mg_relax_kernel<false>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, w, b, y, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}
bis_status launch_prolong(bis_ctx *ctx, double *x, const int32_t *agg, const double *ec, double scale, int64_t n) {
    const bool vec = aligned16(x) && (reinterpret_cast<uintptr_t>(agg) & 7) == 0 && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
    if (vec) hipLaunchKernelGGL((mg_prolong_kernel<true>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, agg, ec, scale, n);
    else hipLaunchKernelGGL((mg_prolong_kernel<false>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, agg, ec, scale, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status launch_axmy(bis_ctx *ctx, double *r, const double *a, const double *b, const double *s_dev, int64_t n) {
    const bool vec = aligned16(r) && aligned16(a) && aligned16(b) && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
    if (vec) hipLaunchKernelGGL((mg_axmy_kernel<true>), dim3(grid), dim3(kMgT), 0, ctx->stream, r, a, b, s_dev, n);
    else hipLaunchKernelGGL((mg_axmy_kernel<false>), dim3(grid), dim3(kMgT), 0, ctx->stream, r, a, b, s_dev, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}
bis_status launch_combine(bis_ctx *ctx, double *x, const double *d, const double *coef, int64_t n) {
    const bool vec = aligned16(x) && aligned16(d) && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
    if (vec) hipLaunchKernelGGL((mg_combine_kernel<true>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, d, coef, n);
    else hipLaunchKernelGGL((mg_combine_kernel<false>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, d, coef, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}
// u == nullptr: the first step's two sums over (p, q, r); otherwise the second step's three over (p, q, u, r)
bis_status launch_kdots(bis_ctx *ctx, const bis_mg *mg, const double *p, const double *q, const double *u, const double *r, int64_t n, bool gcr,
                        double *sc) {
    const bool vec = aligned16(p) && aligned16(q) && aligned16(u) && aligned16(r) && n >= 2;
    const int64_t items = vec ? n >> 1 : n;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + kMgT - 1) / kMgT, kMaxReduceBlocks));
#define MG_KDOTS(NS, V) hipLaunchKernelGGL((mg_kdots_kernel<NS, V>), dim3(grid), dim3(kMgT), 0, ctx->stream, p, q, u, r, n, gcr ? 1 : 0, \
                                           mg->kpartials, mg->kcounters, sc)
    if (u) { if (vec) MG_KDOTS(3, true); else MG_KDOTS(3, false); }
    else { if (vec) MG_KDOTS(2, true); else MG_KDOTS(2, false); }
#undef MG_KDOTS
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

// ---- setup kernels -----------------------------------------------------------------------------------------------------
// the MIS key (include/bis_hip.h): (hash32(i), i)
__device__ __forceinline__ unsigned long long mg_key(int32_t i) { return ((unsigned long long)bis_hash32((uint32_t)i) << 32) | (uint32_t)i; }

enum { MG_AUX_BAD_DIAG, MG_AUX_UNDECIDED, MG_AUX_COUNT };

// w_i and the diagonal check of one level: omega == 0: 1 / sum_j |a_ij| summed left to right in CRS order; omega > 0:
// omega / a_ii (the first entry of the row on the diagonal).  A row without a diagonal entry, or with a zero there, is counted.
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_weights_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col,
                                                          const double *__restrict__ val, int64_t n, double omega, double *w,
                                                          unsigned *aux) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        double sum = 0.0, d = 0.0;
        bool have = false;
        for (int64_t k = (int64_t)rp[i], e = (int64_t)rp[i + 1]; k < e; ++k) {
            const double a = val[k];
            sum = __dadd_rn(sum, fabs(a));
            if (!have && (int64_t)col[k] == i) { d = a; have = true; }
        }
        if (!have || d == 0.0) { atomicAdd(&aux[MG_AUX_BAD_DIAG], 1u); w[i] = 0.0; }
        else w[i] = omega > 0.0 ? omega / d : 1.0 / sum;
    }
}

// row = ((z ny + y) nx + x) dof + d  ->  (((z/2) cy + y/2) cx + x/2) dof + d
__global__ __launch_bounds__(kMgT) void mg_grid_agg_kernel(int64_t n, int64_t nx, int64_t ny, int64_t dof, int64_t cx, int64_t cy,
                                                           int32_t *agg) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        const int64_t d = i % dof, node = i / dof;
        const int64_t x = node % nx, t = node / nx, y = t % ny, z = t / ny;
        agg[i] = (int32_t)((((z >> 1) * cy + (y >> 1)) * cx + (x >> 1)) * dof + d);
    }
}

// MIS round, first half: an undecided row whose key is the largest among its undecided neighbours becomes a root of this
// round (state = tag).  A neighbour that becomes a root in the same pass still counts as undecided (state 0 or tag: the same
// decision whichever the reader sees), and two neighbours cannot both be the largest.  States: 0 undecided, 2 member,
// >= 4 root (4 + the round it was found in).
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_mis_select_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, int64_t n, int *state,
                                                             int tag) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        if (__hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) continue;
        const unsigned long long mine = mg_key((int32_t)i);
        bool largest = true;
        for (int64_t k = (int64_t)rp[i], e = (int64_t)rp[i + 1]; k < e && largest; ++k) {
            const int32_t j = col[k];
            if ((int64_t)j == i) continue;
            const int sj = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((sj == 0 || sj == tag) && mg_key(j) > mine) largest = false;
        }
        if (largest) __hip_atomic_store(&state[i], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// ... second half: an undecided row next to a root of this round becomes a member; the rows still undecided are counted
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_mis_join_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, int64_t n, int *state,
                                                           int tag, unsigned *aux) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    unsigned left = 0;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        if (__hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) continue;
        bool member = false;
        for (int64_t k = (int64_t)rp[i], e = (int64_t)rp[i + 1]; k < e && !member; ++k) {
            const int32_t j = col[k];
            if ((int64_t)j == i) continue;
            member = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag;
        }
        if (member) __hip_atomic_store(&state[i], 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else ++left;
    }
    // one ticket per wave, not per row: the counter is one address (only "zero or not" is read, a saturated count would do)
    for (int off = 32; off > 0; off >>= 1) left += __shfl_down(left, off, 64);
    if ((threadIdx.x & 63) == 0 && left != 0) atomicAdd(&aux[MG_AUX_UNDECIDED], left);
}
__global__ __launch_bounds__(kMgT) void mg_root_flag_kernel(const int *__restrict__ state, int64_t n, int32_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) flag[i] = state[i] >= 4 ? 1 : 0;
}
// roots are numbered by ascending row (root_no: the exclusive scan of the flags); a member joins the root neighbour with the
// largest |a_ij|, the lowest column among equals
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_mis_assign_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col,
                                                             const double *__restrict__ val, int64_t n, const int *__restrict__ state,
                                                             const int32_t *__restrict__ root_no, int32_t *agg) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        if (state[i] >= 4) { agg[i] = root_no[i]; continue; }
        double best = -1.0;
        int32_t best_j = -1;
        for (int64_t k = (int64_t)rp[i], e = (int64_t)rp[i + 1]; k < e; ++k) {
            const int32_t j = col[k];
            if ((int64_t)j == i || state[j] < 4) continue;
            const double a = fabs(val[k]);
            if (best_j < 0 || a > best || (a == best && j < best_j)) { best = a; best_j = j; }
        }
        agg[i] = best_j >= 0 ? root_no[best_j] : 0; // (a member has a root neighbour: the rounds made it one)
    }
}

__global__ __launch_bounds__(kMgT) void mg_iota_keys_kernel(const int32_t *__restrict__ agg, int64_t n, uint32_t *key, int32_t *idx) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) { key[i] = (uint32_t)agg[i]; idx[i] = (int32_t)i; }
}
// out[I] = the first position p in the ascending key[0, m) with key[p] >= I, for I in [0, count)
template <typename K, typename O>
__global__ __launch_bounds__(kMgT) void mg_lower_bound_kernel(const K *__restrict__ key, int64_t m, int64_t count, int shift, O *out) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t I = (int64_t)blockIdx.x * kMgT + threadIdx.x; I < count; I += stride) {
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(key[mid] >> shift) < I) lo = mid + 1; else hi = mid;
        }
        out[I] = (O)lo;
    }
}
// every fine entry (r, c, v) -> key agg[r] << 32 | agg[c]; the values are copied beside it (the sort moves them)
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_entry_keys_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, int64_t n,
                                                             const int32_t *__restrict__ agg, unsigned long long *key) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t r = (int64_t)blockIdx.x * kMgT + threadIdx.x; r < n; r += stride) {
        const unsigned long long hi = (unsigned long long)(uint32_t)agg[r] << 32;
        for (int64_t k = (int64_t)rp[r], e = (int64_t)rp[r + 1]; k < e; ++k) key[k] = hi | (uint32_t)agg[col[k]];
    }
}
__global__ __launch_bounds__(kMgT) void mg_head_flag_kernel(const unsigned long long *__restrict__ key, int64_t m, int64_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t k = (int64_t)blockIdx.x * kMgT + threadIdx.x; k < m; k += stride) flag[k] = (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
}
// pos: the inclusive scan of the head flags (entry k belongs to run pos[k] - 1).  The head of run e records where the run starts and the run's (row, column).
__global__ __launch_bounds__(kMgT) void mg_heads_kernel(const unsigned long long *__restrict__ key, const int64_t *__restrict__ pos, int64_t m,
                                                        int64_t *start, int32_t *row_c, int32_t *col_c) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t k = (int64_t)blockIdx.x * kMgT + threadIdx.x; k < m; k += stride) {
        if (k != 0 && key[k] == key[k - 1]) continue;
        const int64_t e = pos[k] - 1;
        start[e] = k;
        row_c[e] = (int32_t)(key[k] >> 32);
        col_c[e] = (int32_t)(key[k] & 0xffffffffull);
    }
}
// a lane per coarse entry: the sum of its run in the sorted (= fine CRS) order, the first value starting it
__global__ __launch_bounds__(kMgT) void mg_run_sum_kernel(const double *__restrict__ v, const int64_t *__restrict__ start, int64_t m_c,
                                                          int64_t m, double *val_c) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t e = (int64_t)blockIdx.x * kMgT + threadIdx.x; e < m_c; e += stride) {
        const int64_t s = start[e], t = e + 1 < m_c ? start[e + 1] : m;
        double acc = v[s];
        for (int64_t k = s + 1; k < t; ++k) acc = __dadd_rn(acc, v[k]);
        val_c[e] = acc;
    }
}

// smoothed aggregation: d_i = the first diagonal entry of row i, q_i = (sum_j |a_ij|, left to right from 0) / |d_i|
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_rho_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                      int64_t n, double *d, double *q) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        double sum = 0.0, dii = 0.0;
        bool have = false;
        for (int64_t k = (int64_t)rp[i], e = (int64_t)rp[i + 1]; k < e; ++k) {
            const double a = val[k];
            sum = __dadd_rn(sum, fabs(a));
            if (!have && (int64_t)col[k] == i) { dii = a; have = true; }
        }
        d[i] = dii;
        q[i] = __ddiv_rn(sum, fabs(dii)); // (the weights' pass refused a row without a diagonal entry, or with a zero there)
    }
}
// T: row i holds the one entry (agg[i], 1)
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_tentative_kernel(const int32_t *__restrict__ agg, int64_t n, RP *rp, int32_t *col, double *val) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i <= n; i += stride) {
        rp[i] = (RP)i;
        if (i < n) { col[i] = agg[i]; val[i] = 1.0; }
    }
}
// Q = A T becomes P in place: p_iJ = t_iJ - c_i q_iJ, c_i = omega_l / a_ii
__global__ __launch_bounds__(kMgT) void mg_smooth_p_kernel(const void *rp, int w64, const int32_t *__restrict__ col, double *val,
                                                           const int32_t *__restrict__ agg, const double *__restrict__ d, double omega_l, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        const double c = __ddiv_rn(omega_l, d[i]);
        const int32_t mine = agg[i];
        for (int64_t k = mg_rp_at(rp, w64, i), e = mg_rp_at(rp, w64, i + 1); k < e; ++k)
            val[k] = __dsub_rn(col[k] == mine ? 1.0 : 0.0, bis_mul_sep(c, val[k]));
    }
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

#define MG_CHECK(call)                                                                                                 \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) { ctx->err = std::string("bis_mg_create: " #call ": ") + hipGetErrorString(e_); return BIS_ERR_HIP; } \
    } while (0)

bis_status read_aux(bis_ctx *ctx, const unsigned *aux, unsigned *host) {
    MG_CHECK(hipGetLastError());
    MG_CHECK(hipMemcpyAsync(host, aux, sizeof(unsigned) * MG_AUX_COUNT, hipMemcpyDeviceToHost, ctx->stream));
    MG_CHECK(hipStreamSynchronize(ctx->stream));
    return BIS_OK;
}

// weights of level L and its diagonal check
template <typename RP>
bis_status level_weights(bis_ctx *ctx, bis_mg_level &L, double omega, unsigned *aux) {
    MG_CHECK(hipMalloc(&L.w, sizeof(double) * (size_t)std::max<int64_t>(L.n, 2)));
    MG_CHECK(hipMemsetAsync(aux, 0, sizeof(unsigned) * MG_AUX_COUNT, ctx->stream));
    hipLaunchKernelGGL(mg_weights_kernel<RP>, dim3(mg_grid(L.n)), dim3(kMgT), 0, ctx->stream, (const RP *)L.A->row_ptr, L.A->col, L.A->val,
                       L.n, omega, L.w, aux);
    unsigned h[MG_AUX_COUNT] = {0};
    if (bis_status st = read_aux(ctx, aux, h)) return st;
    if (h[MG_AUX_BAD_DIAG]) {
        ctx->err = "bis_mg_create: a row without a diagonal entry, or with a zero on the diagonal";
        return BIS_ERR_ZERO_DIAG;
    }
    return BIS_OK;
}

// MIS aggregates of level L into agg; *n_coarse = the number of roots
template <typename RP>
bis_status mis_aggregates(bis_ctx *ctx, const bis_mg_level &L, int32_t *agg, int64_t *n_coarse, unsigned *aux) {
    const int64_t n = L.n;
    const RP *rp = (const RP *)L.A->row_ptr;
    bool symmetric = true;
    if (bis_status st = bis_mat_pattern_symmetric(ctx, L.A, &symmetric)) return st;
    if (!symmetric) {
        ctx->err = "bis_mg_create: MIS aggregates need a structurally symmetric pattern without repeated entries";
        return BIS_ERR_UNSUPPORTED;
    }
    DevBuf state, flag, root_no, tmp;
    MG_CHECK(state.alloc(sizeof(int) * (size_t)n));
    MG_CHECK(flag.alloc(sizeof(int32_t) * (size_t)n));
    MG_CHECK(root_no.alloc(sizeof(int32_t) * (size_t)n));
    MG_CHECK(hipMemsetAsync(state.p, 0, sizeof(int) * (size_t)n, ctx->stream));
    const dim3 grid(mg_grid(n));
    for (int round = 0;; ++round) { // every round decides at least the undecided row with the largest key
        const int tag = 4 + round;
        MG_CHECK(hipMemsetAsync(aux, 0, sizeof(unsigned) * MG_AUX_COUNT, ctx->stream));
        hipLaunchKernelGGL(mg_mis_select_kernel<RP>, grid, dim3(kMgT), 0, ctx->stream, rp, L.A->col, n, state.as<int>(), tag);
        hipLaunchKernelGGL(mg_mis_join_kernel<RP>, grid, dim3(kMgT), 0, ctx->stream, rp, L.A->col, n, state.as<int>(), tag, aux);
        unsigned h[MG_AUX_COUNT] = {0};
        if (bis_status st = read_aux(ctx, aux, h)) return st;
        if (h[MG_AUX_UNDECIDED] == 0) break;
        if ((int64_t)round > n) { ctx->err = "bis_mg_create: the MIS rounds do not end (internal)"; return BIS_ERR_INVALID; }
    }
    hipLaunchKernelGGL(mg_root_flag_kernel, grid, dim3(kMgT), 0, ctx->stream, state.as<int>(), n, flag.as<int32_t>());
    size_t bytes = 0;
    MG_CHECK(rocprim::exclusive_scan(nullptr, bytes, flag.as<int32_t>(), root_no.as<int32_t>(), (int32_t)0, (size_t)n, rocprim::plus<int32_t>(),
                                     ctx->stream));
    MG_CHECK(tmp.alloc(bytes));
    MG_CHECK(rocprim::exclusive_scan(tmp.p, bytes, flag.as<int32_t>(), root_no.as<int32_t>(), (int32_t)0, (size_t)n, rocprim::plus<int32_t>(),
                                     ctx->stream));
    hipLaunchKernelGGL(mg_mis_assign_kernel<RP>, grid, dim3(kMgT), 0, ctx->stream, rp, L.A->col, L.A->val, n, state.as<int>(),
                       root_no.as<int32_t>(), agg);
    int32_t last[2] = {0, 0};
    MG_CHECK(hipGetLastError());
    MG_CHECK(hipMemcpyAsync(&last[0], root_no.as<int32_t>() + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MG_CHECK(hipMemcpyAsync(&last[1], flag.as<int32_t>() + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MG_CHECK(hipStreamSynchronize(ctx->stream));
    *n_coarse = (int64_t)last[0] + last[1];
    return BIS_OK;
}

// agg_ptr / agg_idx of level L from its aggregates: a stable sort of (aggregate, row)
bis_status members_lists(bis_ctx *ctx, bis_mg_level &L) {
    const int64_t n = L.n, nc = L.n_coarse;
    DevBuf key, key_out, idx, tmp;
    MG_CHECK(key.alloc(4 * (size_t)n));
    MG_CHECK(key_out.alloc(4 * (size_t)n));
    MG_CHECK(idx.alloc(4 * (size_t)n));
    MG_CHECK(hipMalloc(&L.agg_idx, 4 * (size_t)n));
    MG_CHECK(hipMalloc(&L.agg_ptr, 4 * (size_t)(nc + 1)));
    hipLaunchKernelGGL(mg_iota_keys_kernel, dim3(mg_grid(n)), dim3(kMgT), 0, ctx->stream, L.agg, n, key.as<uint32_t>(), idx.as<int32_t>());
    size_t bytes = 0;
    MG_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key.as<uint32_t>(), key_out.as<uint32_t>(), idx.as<int32_t>(), L.agg_idx, (size_t)n, 0, 32,
                                       ctx->stream));
    MG_CHECK(tmp.alloc(bytes));
    MG_CHECK(rocprim::radix_sort_pairs(tmp.p, bytes, key.as<uint32_t>(), key_out.as<uint32_t>(), idx.as<int32_t>(), L.agg_idx, (size_t)n, 0, 32,
                                       ctx->stream)); // stable: ascending rows inside an aggregate
    hipLaunchKernelGGL((mg_lower_bound_kernel<uint32_t, int32_t>), dim3(mg_grid(nc + 1)), dim3(kMgT), 0, ctx->stream, key_out.as<uint32_t>(), n,
                       nc + 1, 0, L.agg_ptr);
    MG_CHECK(hipGetLastError());
    MG_CHECK(hipStreamSynchronize(ctx->stream)); // (the temporaries go out of scope)
    return BIS_OK;
}

// the Galerkin operator of level L for its aggregates
template <typename RP>
bis_status galerkin(bis_ctx *ctx, const bis_mg_level &L, bis_mat **out) {
    const int64_t n = L.n, m = L.A->nnz, nc = L.n_coarse;
    const RP *rp = (const RP *)L.A->row_ptr;
    DevBuf key, key_out, val_out, tmp, start, row_c;
    MG_CHECK(key.alloc(8 * (size_t)m));
    MG_CHECK(key_out.alloc(8 * (size_t)m));
    MG_CHECK(val_out.alloc(8 * (size_t)m));
    hipLaunchKernelGGL(mg_entry_keys_kernel<RP>, dim3(mg_grid(n)), dim3(kMgT), 0, ctx->stream, rp, L.A->col, n, L.agg,
                       key.as<unsigned long long>());
    size_t bytes = 0;
    MG_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key.as<unsigned long long>(), key_out.as<unsigned long long>(), (const double *)L.A->val,
                                       val_out.as<double>(), (size_t)m, 0, 64, ctx->stream));
    MG_CHECK(tmp.alloc(bytes));
    MG_CHECK(rocprim::radix_sort_pairs(tmp.p, bytes, key.as<unsigned long long>(), key_out.as<unsigned long long>(), (const double *)L.A->val,
                                       val_out.as<double>(), (size_t)m, 0, 64, ctx->stream)); // stable: a run keeps the fine CRS order
    // the unsorted keys are done with: their buffer takes the head flags and, scanned in place, the runs' numbers + 1
    int64_t *pos = key.as<int64_t>();
    hipLaunchKernelGGL(mg_head_flag_kernel, dim3(mg_grid(m)), dim3(kMgT), 0, ctx->stream, key_out.as<unsigned long long>(), m, pos);
    size_t bytes2 = 0;
    MG_CHECK(rocprim::inclusive_scan(nullptr, bytes2, pos, pos, (size_t)m, rocprim::plus<int64_t>(), ctx->stream));
    if (bytes2 > bytes) { hipFree(tmp.p); tmp.p = nullptr; MG_CHECK(tmp.alloc(bytes2)); }
    MG_CHECK(rocprim::inclusive_scan(tmp.p, bytes2, pos, pos, (size_t)m, rocprim::plus<int64_t>(), ctx->stream));
    int64_t last_pos = 0;
    MG_CHECK(hipMemcpyAsync(&last_pos, pos + (m - 1), sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    MG_CHECK(hipStreamSynchronize(ctx->stream));
    const int64_t m_c = last_pos; // (the runs up to and including the last entry's)
    MG_CHECK(start.alloc(8 * (size_t)m_c));
    MG_CHECK(row_c.alloc(4 * (size_t)m_c));
    bis_mat *C = nullptr;
    if (bis_status st = bis_mat_alloc(ctx, nc, nc, m_c, bis_want_rp64(m_c), &C)) return st;
    hipLaunchKernelGGL(mg_heads_kernel, dim3(mg_grid(m)), dim3(kMgT), 0, ctx->stream, key_out.as<unsigned long long>(), pos, m,
                       start.as<int64_t>(), row_c.as<int32_t>(), C->col);
    hipLaunchKernelGGL(mg_run_sum_kernel, dim3(mg_grid(m_c)), dim3(kMgT), 0, ctx->stream, val_out.as<double>(), start.as<int64_t>(), m_c, m,
                       C->val);
    if (C->rp64)
        hipLaunchKernelGGL((mg_lower_bound_kernel<int32_t, int64_t>), dim3(mg_grid(nc + 1)), dim3(kMgT), 0, ctx->stream, row_c.as<int32_t>(), m_c,
                           nc + 1, 0, (int64_t *)C->row_ptr);
    else
        hipLaunchKernelGGL((mg_lower_bound_kernel<int32_t, int32_t>), dim3(mg_grid(nc + 1)), dim3(kMgT), 0, ctx->stream, row_c.as<int32_t>(), m_c,
                           nc + 1, 0, (int32_t *)C->row_ptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string("bis_mg_create: Galerkin product: ") + hipGetErrorString(e);
        bis_mat_destroy(ctx, C);
        return BIS_ERR_HIP;
    }
    *out = C;
    return BIS_OK;
}

struct MatHold { // destroys the matrix unless it was handed on
    bis_ctx *ctx;
    bis_mat *m = nullptr;
    ~MatHold() { if (m) { hipStreamSynchronize(ctx->stream); bis_mat_destroy(ctx, m); } }
    bis_mat *release() { bis_mat *r = m; m = nullptr; return r; }
};

// the transition of level L of a smoothed hierarchy: omega_l, P and R into L, the Galerkin operator R (A P) into *out
template <typename RP>
bis_status smoothed_transition(bis_ctx *ctx, double prolong_omega, bis_mg_level &L, bis_mat **out) {
    const int64_t n = L.n, nc = L.n_coarse;
    DevBuf d, q, red, tmp;
    MG_CHECK(d.alloc(8 * (size_t)n));
    MG_CHECK(q.alloc(8 * (size_t)n));
    MG_CHECK(red.alloc(8));
    hipLaunchKernelGGL(mg_rho_kernel<RP>, dim3(mg_grid(n)), dim3(kMgT), 0, ctx->stream, (const RP *)L.A->row_ptr, L.A->col, L.A->val, n,
                       d.as<double>(), q.as<double>());
    MG_CHECK(hipGetLastError());
    size_t bytes = 0;
    MG_CHECK(rocprim::reduce(nullptr, bytes, q.as<double>(), red.as<double>(), 0.0, (size_t)n, rocprim::maximum<double>(), ctx->stream));
    MG_CHECK(tmp.alloc(bytes));
    MG_CHECK(rocprim::reduce(tmp.p, bytes, q.as<double>(), red.as<double>(), 0.0, (size_t)n, rocprim::maximum<double>(), ctx->stream));
    double rho = 0.0;
    MG_CHECK(hipMemcpyAsync(&rho, red.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    MG_CHECK(hipStreamSynchronize(ctx->stream));
    if (!(rho > 0.0) || !(rho <= DBL_MAX)) {
        ctx->err = "bis_mg_create_smoothed: the bound on the spectral radius of D^-1 A is not a positive finite number";
        return BIS_ERR_INVALID;
    }
    const double omega_l = prolong_omega / rho;
    MatHold T{ctx}, P{ctx}, R{ctx}, AP{ctx}, C{ctx};
    if (bis_status st = bis_mat_alloc(ctx, n, nc, n, bis_want_rp64(n), &T.m)) return st;
    if (T.m->rp64) hipLaunchKernelGGL(mg_tentative_kernel<int64_t>, dim3(mg_grid(n + 1)), dim3(kMgT), 0, ctx->stream, L.agg, n, (int64_t *)T.m->row_ptr,
                                      T.m->col, T.m->val);
    else hipLaunchKernelGGL(mg_tentative_kernel<int32_t>, dim3(mg_grid(n + 1)), dim3(kMgT), 0, ctx->stream, L.agg, n, (int32_t *)T.m->row_ptr,
                            T.m->col, T.m->val);
    MG_CHECK(hipGetLastError());
    if (bis_status st = bis_spgemm(ctx, L.A, T.m, &P.m)) return st; // Q
    hipLaunchKernelGGL(mg_smooth_p_kernel, dim3(mg_grid(n)), dim3(kMgT), 0, ctx->stream, P.m->row_ptr, P.m->rp64 ? 1 : 0, P.m->col, P.m->val, L.agg,
                       d.as<double>(), omega_l, n);
    MG_CHECK(hipGetLastError());
    MG_CHECK(hipStreamSynchronize(ctx->stream));
    bis_mat_values_changed(P.m);
    if (bis_status st = bis_mat_transpose(ctx, P.m, &R.m)) return st;
    if (bis_status st = bis_spgemm(ctx, L.A, P.m, &AP.m)) return st;
    if (bis_status st = bis_spgemm(ctx, R.m, AP.m, &C.m)) return st;
    L.P = P.release();
    L.R = R.release();
    L.pomega = omega_l;
    *out = C.release();
    return BIS_OK;
}

void free_level(bis_ctx *ctx, bis_mg_level &L) {
    hipFree(L.w); hipFree(L.agg); hipFree(L.agg_ptr); hipFree(L.agg_idx); hipFree(L.x); hipFree(L.b); hipFree(L.y);
    hipFree(L.kr); hipFree(L.kd); hipFree(L.kv); hipFree(L.cd);
    if (L.owned) bis_mat_destroy(ctx, L.owned);
    if (L.P) bis_mat_destroy(ctx, L.P);
    if (L.R) bis_mat_destroy(ctx, L.R);
    L = bis_mg_level();
}

void mg_free(bis_ctx *ctx, bis_mg *mg) {
    hipStreamSynchronize(ctx->stream);
    for (bis_mg_level &L : mg->lv) free_level(ctx, L);
    if (mg->operand) { mg->operand->mg = nullptr; bis_mat_destroy(ctx, mg->operand); }
    hipFree(mg->b0);
    hipFree(mg->ksc); hipFree(mg->kpartials); hipFree(mg->kcounters);
    delete mg;
}

bis_status mg_build(bis_ctx *ctx, const bis_mat *A, bis_mg *mg) {
    const bis_mg_params &p = mg->p;
    DevBuf auxb;
    MG_CHECK(auxb.alloc(sizeof(unsigned) * MG_AUX_COUNT));
    unsigned *aux = auxb.as<unsigned>();
    mg->lv.reserve(kMgMaxLevels);
    mg->lv.emplace_back();
    mg->lv[0].A = A;
    mg->lv[0].n = A->n_rows;
    while (true) {
        bis_mg_level &L = mg->lv.back();
        if (L.n == 0) break;
        if (bis_status st = L.A->rp64 ? level_weights<int64_t>(ctx, L, p.omega, aux) : level_weights<int32_t>(ctx, L, p.omega, aux)) return st;
        if (L.n <= p.coarse_limit || (int)mg->lv.size() >= p.max_levels) break;
        // the aggregates of this level
        const int64_t *g = L.A->grid;
        bool grid_ok = g[0] > 0 && g[1] > 0 && g[2] > 0 && g[3] > 0 && g[0] * g[1] * g[2] * g[3] == L.n;
        if (p.coarsening == 1 && !grid_ok) {
            ctx->err = "bis_mg_create: coarsening = grid, and a level has no grid hint that matches its size";
            return BIS_ERR_INVALID;
        }
        if (p.coarsening == 2) grid_ok = false;
        MG_CHECK(hipMalloc(&L.agg, 4 * (size_t)L.n));
        int64_t nc = 0, cg[4] = {0, 0, 0, 0};
        if (grid_ok) {
            cg[0] = (g[0] + 1) / 2; cg[1] = (g[1] + 1) / 2; cg[2] = (g[2] + 1) / 2; cg[3] = g[3];
            nc = cg[0] * cg[1] * cg[2] * cg[3];
            hipLaunchKernelGGL(mg_grid_agg_kernel, dim3(mg_grid(L.n)), dim3(kMgT), 0, ctx->stream, L.n, g[0], g[1], g[3], cg[0], cg[1], L.agg);
            MG_CHECK(hipGetLastError());
        } else {
            if (bis_status st = L.A->rp64 ? mis_aggregates<int64_t>(ctx, L, L.agg, &nc, aux) : mis_aggregates<int32_t>(ctx, L, L.agg, &nc, aux))
                return st;
        }
        if (nc <= 0 || 5 * nc > 4 * L.n) { // n_{l+1} > 0.8 n_l: the step is dropped, this level is the coarsest
            MG_CHECK(hipStreamSynchronize(ctx->stream));
            hipFree(L.agg);
            L.agg = nullptr;
            break;
        }
        L.kind = grid_ok ? 1 : 2;
        L.n_coarse = nc;
        bis_mat *C = nullptr;
        if (mg->smoothed) {
            if (bis_status st = L.A->rp64 ? smoothed_transition<int64_t>(ctx, mg->prolong_omega, L, &C)
                                          : smoothed_transition<int32_t>(ctx, mg->prolong_omega, L, &C))
                return st;
        } else {
            if (bis_status st = members_lists(ctx, L)) return st;
            if (bis_status st = L.A->rp64 ? galerkin<int64_t>(ctx, L, &C) : galerkin<int32_t>(ctx, L, &C)) return st;
        }
        if (grid_ok) for (int k = 0; k < 4; ++k) C->grid[k] = cg[k];
        if (bis_status st = bis_mat_finalize(ctx, C)) { bis_mat_destroy(ctx, C); return st; }
        mg->lv.emplace_back(); // (reserved: L stays valid, but is not used below)
        bis_mg_level &N = mg->lv.back();
        N.A = N.owned = C;
        N.n = nc;
    }
    // every level's SpMV form, and the cycle's scratch
    for (size_t l = 0; l < mg->lv.size(); ++l) {
        bis_mg_level &L = mg->lv[l];
        if (L.n == 0) continue;
        if (bis_status st = bis_mat_spmv_stream_info(ctx, L.A, nullptr, nullptr, nullptr, nullptr)) return st;
        const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(L.n, 2);
        MG_CHECK(hipMalloc(&L.y, bytes));
        if (l > 0) { MG_CHECK(hipMalloc(&L.x, bytes)); MG_CHECK(hipMalloc(&L.b, bytes)); }
    }
    MG_CHECK(hipMalloc(&mg->b0, sizeof(double) * (size_t)std::max<int64_t>(A->n_rows, 2)));
    if (bis_status st = bis_mat_alloc(ctx, A->n_rows, A->n_rows, 0, false, &mg->operand)) return st;
    const size_t rpb = sizeof(int32_t) * (size_t)(A->n_rows + 1);
    MG_CHECK(hipMemsetAsync(mg->operand->row_ptr, 0, rpb, ctx->stream));
    if (bis_status st = bis_mat_finalize(ctx, mg->operand)) return st;
    mg->operand->mg = mg;
    MG_CHECK(hipStreamSynchronize(ctx->stream));
    return BIS_OK;
}

// ---- the Chebyshev smoother's kernels (after everything the plain cycle launches: those keep their place in the code object) ----
// The Chebyshev smoother's steps (bis_mg_set_smoother).  From x = 0: d = c2 (w b), x = d.  The inputs are read once:
// non-temporal loads; x and d are stored plainly -- the next SpMV and the next step read them.
template <bool VEC>
__global__ __launch_bounds__(kMgT) void mg_cheb0_kernel(double *x, double *d, const double *w, const double *b, double c2, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *x2 = reinterpret_cast<mg_v2d *>(x), *d2 = reinterpret_cast<mg_v2d *>(d);
        const mg_v2d *w2 = reinterpret_cast<const mg_v2d *>(w), *b2 = reinterpret_cast<const mg_v2d *>(b);
        for (; i < n2; i += stride) {
            const mg_v2d wv = __builtin_nontemporal_load(w2 + i), bv = __builtin_nontemporal_load(b2 + i);
            mg_v2d r;
            r.x = __dmul_rn(c2, __dmul_rn(wv.x, bv.x));
            r.y = __dmul_rn(c2, __dmul_rn(wv.y, bv.y));
            d2[i] = r;
            x2[i] = r;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = d[n - 1] = __dmul_rn(c2, __dmul_rn(w[n - 1], b[n - 1]));
    } else {
        for (; i < n; i += stride) x[i] = d[i] = __dmul_rn(c2, __dmul_rn(__builtin_nontemporal_load(w + i), __builtin_nontemporal_load(b + i)));
    }
}

// The general step with y = A x: t = b - y, u = w t, d = (c1 d) + (c2 u), x = x + d, each rounded.  FIRST (step 0 of a
// polynomial): d = c2 u -- the d of the polynomial before is neither read nor multiplied.
template <bool FIRST>
__device__ __forceinline__ double mg_cheb1(double d, double w, double b, double y, double c1, double c2) {
    // (bis_mul_sep: a product that feeds a sum -- here, or x + d in the caller -- would otherwise be contracted into it)
    const double cu = bis_mul_sep(c2, __dmul_rn(w, __dsub_rn(b, y)));
    return FIRST ? cu : __dadd_rn(bis_mul_sep(c1, d), cu);
}

template <bool FIRST, bool VEC>
__global__ __launch_bounds__(kMgT) void mg_cheb_kernel(double *x, double *d, const double *w, const double *b, const double *y, double c1,
                                                       double c2, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        mg_v2d *x2 = reinterpret_cast<mg_v2d *>(x), *d2 = reinterpret_cast<mg_v2d *>(d);
        const mg_v2d *w2 = reinterpret_cast<const mg_v2d *>(w), *b2 = reinterpret_cast<const mg_v2d *>(b),
                     *y2 = reinterpret_cast<const mg_v2d *>(y);
        for (; i < n2; i += stride) {
            const mg_v2d wv = __builtin_nontemporal_load(w2 + i), bv = __builtin_nontemporal_load(b2 + i),
                         yv = __builtin_nontemporal_load(y2 + i), xv = x2[i];
            mg_v2d dv = xv; // (FIRST: any value, not used)
            if (!FIRST) dv = d2[i];
            mg_v2d dn, xn;
            dn.x = mg_cheb1<FIRST>(dv.x, wv.x, bv.x, yv.x, c1, c2);
            dn.y = mg_cheb1<FIRST>(dv.y, wv.y, bv.y, yv.y, c1, c2);
            xn.x = __dadd_rn(xv.x, dn.x);
            xn.y = __dadd_rn(xv.y, dn.y);
            d2[i] = dn;
            x2[i] = xn;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const int64_t j = n - 1;
            const double dn = mg_cheb1<FIRST>(FIRST ? 0.0 : d[j], w[j], b[j], y[j], c1, c2);
            d[j] = dn;
            x[j] = __dadd_rn(x[j], dn);
        }
    } else {
        for (; i < n; i += stride) {
            const double dn = mg_cheb1<FIRST>(FIRST ? 0.0 : d[i], __builtin_nontemporal_load(w + i), __builtin_nontemporal_load(b + i),
                                              __builtin_nontemporal_load(y + i), c1, c2);
            d[i] = dn;
            x[i] = __dadd_rn(x[i], dn);
        }
    }
}

bis_status launch_cheb0(bis_ctx *ctx, double *x, double *d, const double *w, const double *b, double c2, int64_t n) {
    const bool vec = aligned16(x) && aligned16(d) && aligned16(w) && aligned16(b) && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
    if (vec) hipLaunchKernelGGL((mg_cheb0_kernel<true>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, d, w, b, c2, n);
    else hipLaunchKernelGGL((mg_cheb0_kernel<false>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, d, w, b, c2, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}
bis_status launch_cheb(bis_ctx *ctx, bool first, double *x, double *d, const double *w, const double *b, const double *y, double c1, double c2,
                       int64_t n) {
    const bool vec = aligned16(x) && aligned16(d) && aligned16(w) && aligned16(b) && aligned16(y) && n >= 2;
    const int grid = mg_grid(vec ? n >> 1 : n);
#define MG_CHEB(F, V) hipLaunchKernelGGL((mg_cheb_kernel<F, V>), dim3(grid), dim3(kMgT), 0, ctx->stream, x, d, w, b, y, c1, c2, n)
    if (first) { if (vec) MG_CHEB(true, true); else MG_CHEB(true, false); }
    else { if (vec) MG_CHEB(false, true); else MG_CHEB(false, false); }
#undef MG_CHEB
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

// steps [from, degree) of one Chebyshev polynomial on x
bis_status cheb_steps(bis_ctx *ctx, const bis_mg_level &L, double *x, const double *b, int from) {
    for (int k = from; k < L.cheb_degree; ++k) {
        if (bis_status st = bis_spmv_launch(ctx, L.A, x, L.y, nullptr, nullptr)) return st;
        if (bis_status st = launch_cheb(ctx, k == 0, x, L.cd, L.w, b, L.y, L.cheb_c1[k], L.cheb_c2[k], L.n)) return st;
    }
    return BIS_OK;
}

// the first sweep of a level visit, from x = 0: x = w o b, or the polynomial without its first SpMV
bis_status smooth0(bis_ctx *ctx, const bis_mg_level &L, double *x, const double *b) {
    if (!L.cheb_degree) return launch_relax0(ctx, x, L.w, b, L.n);
    if (bis_status st = launch_cheb0(ctx, x, L.cd, L.w, b, L.cheb_c2[0], L.n)) return st;
    return cheb_steps(ctx, L, x, b, 1);
}

// `sweeps` further sweeps x += w o (b - A x), or as many polynomials
bis_status smooth(bis_ctx *ctx, const bis_mg_level &L, double *x, const double *b, int sweeps) {
    for (int s = 0; s < sweeps; ++s) {
        if (L.cheb_degree) {
            if (bis_status st = cheb_steps(ctx, L, x, b, 0)) return st;
            continue;
        }
        if (bis_status st = bis_spmv_launch(ctx, L.A, x, L.y, nullptr, nullptr)) return st;
        if (bis_status st = launch_relax(ctx, x, L.w, b, L.y, L.n)) return st;
    }
    return BIS_OK;
}

// the cycle of transition t (level t -> t + 1): the one onto the coarsest level is always the plain one
int transition_cycle(int cycle, int cycle_levels, size_t levels, size_t t) {
    return (t + 2 < levels && (cycle_levels == 0 || t < (size_t)cycle_levels)) ? cycle : BIS_MG_CYCLE_V;
}

bis_status cycle(bis_ctx *ctx, const bis_mg *mg, size_t l, double *x, const double *b);

// e_c = N.x for the restricted residual N.b of transition t = l: the plain call, or the W / K step around two of them
bis_status coarse_solve(bis_ctx *ctx, const bis_mg *mg, size_t l) {
    const bis_mg_level &N = mg->lv[l + 1];
    const int kind = transition_cycle(mg->cycle, mg->cycle_levels, mg->lv.size(), l);
    if (bis_status st = cycle(ctx, mg, l + 1, N.x, N.b)) return st; // e_1, or c
    if (kind == BIS_MG_CYCLE_V) return BIS_OK;
    if (kind == BIS_MG_CYCLE_W) {
        if (bis_status st = bis_spmv_launch(ctx, N.A, N.x, N.y, nullptr, nullptr)) return st;
        if (bis_status st = launch_axmy(ctx, N.kr, N.b, N.y, mg->ksc + 3, N.n)) return st; // r_2 = r_c - y
        if (bis_status st = cycle(ctx, mg, l + 1, N.kd, N.kr)) return st;                  // e_2
        return launch_combine(ctx, N.x, N.kd, mg->ksc, N.n);                               // e_c = e_1 + e_2
    }
    const bool gcr = kind == BIS_MG_CYCLE_K_GCR;
    double *sc = mg->ksc + kMgScBase + kMgScPer * l;
    if (bis_status st = bis_spmv_launch(ctx, N.A, N.x, N.kv, nullptr, nullptr)) return st;           // v = A c
    if (bis_status st = launch_kdots(ctx, mg, N.x, N.kv, nullptr, N.b, N.n, gcr, sc)) return st;     // rho1, alpha1 -> s1
    if (bis_status st = launch_axmy(ctx, N.kr, N.b, N.kv, sc + MG_SC_S1, N.n)) return st;            // r~ = r_c - s1 v
    if (bis_status st = cycle(ctx, mg, l + 1, N.kd, N.kr)) return st;                                // d
    if (bis_status st = bis_spmv_launch(ctx, N.A, N.kd, N.y, nullptr, nullptr)) return st;           // w = A d
    if (bis_status st = launch_kdots(ctx, mg, N.kd, N.y, N.kv, N.kr, N.n, gcr, sc)) return st;       // gamma, beta, alpha2 -> c1, c2
    return launch_combine(ctx, N.x, N.kd, sc, N.n);                                                  // e_c = c1 c + c2 d
}

bis_status cycle(bis_ctx *ctx, const bis_mg *mg, size_t l, double *x, const double *b) {
    const bis_mg_level &L = mg->lv[l];
    if (bis_status st = smooth0(ctx, L, x, b)) return st;
    if (l + 1 == mg->lv.size()) return smooth(ctx, L, x, b, mg->p.coarse_sweeps - 1);
    if (bis_status st = smooth(ctx, L, x, b, mg->p.nu - 1)) return st;
    const bis_mg_level &N = mg->lv[l + 1];
    if (bis_status st = bis_spmv_launch(ctx, L.A, x, L.y, nullptr, nullptr)) return st;
    if (L.R) // a smoothed hierarchy: the transfers are R and P
        hipLaunchKernelGGL(mg_restrict_sa_kernel, dim3(mg_grid(N.n * 64)), dim3(kMgT), 0, ctx->stream, L.R->row_ptr, L.R->rp64 ? 1 : 0, L.R->col,
                           L.R->val, b, L.y, N.b, N.n);
    else
        hipLaunchKernelGGL(mg_restrict_kernel, dim3(mg_grid(N.n)), dim3(kMgT), 0, ctx->stream, L.agg_ptr, L.agg_idx, b, L.y, N.b, N.n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    if (bis_status st = coarse_solve(ctx, mg, l)) return st;
    if (L.P) {
        hipLaunchKernelGGL(mg_prolong_sa_kernel, dim3(mg_grid(L.n)), dim3(kMgT), 0, ctx->stream, x, L.P->row_ptr, L.P->rp64 ? 1 : 0, L.P->col, L.P->val,
                           N.x, mg->p.coarse_scale, L.n);
        BIS_HIP_CHECK(ctx, hipGetLastError());
    } else if (bis_status st = launch_prolong(ctx, x, L.agg, N.x, mg->p.coarse_scale, L.n)) return st;
    return smooth(ctx, L, x, b, mg->p.nu);
}

// ---- the Chebyshev smoother's setup (bis_mg_set_smoother) ---------------------------------------------------------------
// the Chebyshev smoother's bound on the spectrum of W A: per workgroup the maximum of w_i (sum_j |a_ij|, left to right from 0),
// the product rounded; mg_max_kernel (one workgroup) then takes the maximum of those.  A maximum does not depend on the order.
__device__ __forceinline__ double mg_block_max(double m, double *lds) {
    lds[threadIdx.x] = m;
    __syncthreads();
    for (int off = kMgT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) lds[threadIdx.x] = fmax(lds[threadIdx.x], lds[threadIdx.x + off]);
        __syncthreads();
    }
    return lds[0];
}
template <typename RP>
__global__ __launch_bounds__(kMgT) void mg_bound_kernel(const RP *__restrict__ rp, const double *__restrict__ val, const double *__restrict__ w,
                                                        int64_t n, double *partial) {
    __shared__ double lds[kMgT];
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    double m = -DBL_MAX;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) {
        double sum = 0.0;
        for (int64_t k = (int64_t)rp[i], e = (int64_t)rp[i + 1]; k < e; ++k) sum = __dadd_rn(sum, fabs(val[k]));
        m = fmax(m, __dmul_rn(w[i], sum));
    }
    m = mg_block_max(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}
__global__ __launch_bounds__(kMgT) void mg_max_kernel(const double *__restrict__ partial, int count, double *out) {
    __shared__ double lds[kMgT];
    double m = -DBL_MAX;
    for (int k = threadIdx.x; k < count; k += kMgT) m = fmax(m, partial[k]);
    m = mg_block_max(m, lds);
    if (threadIdx.x == 0) out[0] = m;
}
// the power iteration's start: v_i = hash32(i) / 2^32 - 0.5 (exact)
__global__ __launch_bounds__(kMgT) void mg_hash_vector_kernel(double *v, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kMgT;
    for (int64_t i = (int64_t)blockIdx.x * kMgT + threadIdx.x; i < n; i += stride) v[i] = (double)bis_hash32((uint32_t)i) * 0x1p-32 - 0.5;
}
#define MG_SM_CHECK(call)                                                                                              \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) { ctx->err = std::string("bis_mg_set_smoother: " #call ": ") + hipGetErrorString(e_); return BIS_ERR_HIP; } \
    } while (0)

bis_status level_bound(bis_ctx *ctx, const bis_mg_level &L, double *bound) {
    const int grid = mg_grid(L.n);
    DevBuf partial, out;
    MG_SM_CHECK(partial.alloc(sizeof(double) * (size_t)grid));
    MG_SM_CHECK(out.alloc(sizeof(double)));
    if (L.A->rp64)
        hipLaunchKernelGGL(mg_bound_kernel<int64_t>, dim3(grid), dim3(kMgT), 0, ctx->stream, (const int64_t *)L.A->row_ptr, L.A->val, L.w, L.n,
                           partial.as<double>());
    else
        hipLaunchKernelGGL(mg_bound_kernel<int32_t>, dim3(grid), dim3(kMgT), 0, ctx->stream, (const int32_t *)L.A->row_ptr, L.A->val, L.w, L.n,
                           partial.as<double>());
    hipLaunchKernelGGL(mg_max_kernel, dim3(1), dim3(kMgT), 0, ctx->stream, partial.as<double>(), grid, out.as<double>());
    MG_SM_CHECK(hipGetLastError());
    MG_SM_CHECK(hipMemcpyAsync(bound, out.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MG_SM_CHECK(hipStreamSynchronize(ctx->stream));
    return BIS_OK;
}

// lambda_steps of the power iteration on W A in the W^-1 inner product, by the blocking single-vector calls
bis_status level_estimate(bis_ctx *ctx, const bis_mg_level &L, int steps, double *estimate) {
    const int64_t n = L.n;
    DevBuf v, y, t;
    const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(n, 2);
    MG_SM_CHECK(v.alloc(bytes));
    MG_SM_CHECK(y.alloc(bytes));
    MG_SM_CHECK(t.alloc(bytes));
    hipLaunchKernelGGL(mg_hash_vector_kernel, dim3(mg_grid(n)), dim3(kMgT), 0, ctx->stream, v.as<double>(), n);
    MG_SM_CHECK(hipGetLastError());
    double lambda = 0.0;
    for (int k = 0; k < steps; ++k) {
        double num = 0.0, den = 0.0, nn = 0.0;
        if (bis_status st = bis_spmv(ctx, L.A, v.as<double>(), y.as<double>())) return st;
        if (bis_status st = bis_dot(ctx, v.as<double>(), y.as<double>(), n, &num)) return st;
        if (bis_status st = bis_elemwise_div_vectors(ctx, t.as<double>(), v.as<double>(), L.w, n, 1.0)) return st;
        if (bis_status st = bis_dot(ctx, v.as<double>(), t.as<double>(), n, &den)) return st;
        lambda = num / den;
        if (bis_status st = bis_elemwise_mult_vectors(ctx, v.as<double>(), L.w, y.as<double>(), n, 1.0)) return st;
        if (bis_status st = bis_dot(ctx, v.as<double>(), v.as<double>(), n, &nn)) return st;
        if (bis_status st = bis_scale(ctx, v.as<double>(), v.as<double>(), 1.0 / std::sqrt(nn), n)) return st;
    }
    MG_SM_CHECK(hipStreamSynchronize(ctx->stream)); // (the temporaries go out of scope)
    *estimate = lambda;
    return BIS_OK;
}

// the header's recurrence, every operation its own rounded step (hipcc contracts host code by default)
void cheb_coefficients(double lmax, double lmin, int degree, double *c1, double *c2) {
#pragma clang fp contract(off)
    const double theta = (lmax + lmin) / 2.0;
    const double delta = (lmax - lmin) / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    c1[0] = 0.0;
    c2[0] = 1.0 / theta;
    for (int k = 1; k < degree; ++k) {
        const double two_sigma = 2.0 * sigma;
        const double rho_new = 1.0 / (two_sigma - rho);
        c1[k] = rho_new * rho;
        const double two_rho = 2.0 * rho_new;
        c2[k] = two_rho / delta;
        rho = rho_new;
    }
}

void smoother_to_jacobi(bis_mg *mg) {
    for (bis_mg_level &L : mg->lv) {
        hipFree(L.cd);
        L.cd = nullptr;
        L.cheb_degree = 0;
    }
    mg->sm = bis_mg_smoother{BIS_MG_SMOOTH_JACOBI, 0, 0.0, 0, 0.0};
}

bis_status smoother_setup(bis_ctx *ctx, bis_mg *mg, const bis_mg_smoother &s) {
    for (bis_mg_level &L : mg->lv) {
        if (L.n == 0) continue;
        double bound = 0.0, lambda = 0.0;
        if (bis_status st = level_bound(ctx, L, &bound)) return st;
        if (!(bound > 0.0) || !(bound <= DBL_MAX)) {
            ctx->err = "bis_mg_set_smoother: the bound on the spectrum of W A is not a positive finite number";
            return BIS_ERR_INVALID;
        }
        if (s.est_steps > 0)
            if (bis_status st = level_estimate(ctx, L, s.est_steps, &lambda)) return st;
        const double estimate = (lambda > 0.0 && lambda <= DBL_MAX) ? lambda : 0.0;
        L.sp_bound = bound;
        L.sp_estimate = estimate;
        L.sp_lmax = estimate == 0.0 ? bound : std::min(bound, s.safety * estimate);
        L.sp_lmin = L.sp_lmax / s.ratio;
        cheb_coefficients(L.sp_lmax, L.sp_lmin, s.degree, L.cheb_c1, L.cheb_c2);
        MG_SM_CHECK(hipMalloc(&L.cd, sizeof(double) * (size_t)std::max<int64_t>(L.n, 2)));
    }
    return BIS_OK;
}
#undef MG_SM_CHECK

} // namespace

extern "C" {

static bis_status mg_create(bis_ctx *ctx, const bis_mat *A, const bis_mg_params *params, bool smoothed, double prolong_omega, bis_mg **out);

bis_status bis_mg_create(bis_ctx *ctx, const bis_mat *A, const bis_mg_params *params, bis_mg **out) {
    return mg_create(ctx, A, params, false, 0.0, out);
}

bis_status bis_mg_create_smoothed(bis_ctx *ctx, const bis_mat *A, const bis_mg_params *params, double prolong_omega, bis_mg **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, prolong_omega == 0.0 || (prolong_omega > 0.0 && prolong_omega < 2.0), "bis_mg_create_smoothed: prolong_omega is 0 (4/3) or in (0, 2)");
    return mg_create(ctx, A, params, true, prolong_omega == 0.0 ? 4.0 / 3.0 : prolong_omega, out);
}

static bis_status mg_create(bis_ctx *ctx, const bis_mat *A, const bis_mg_params *params, bool smoothed, double prolong_omega, bis_mg **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && out, "bis_mg_create: bad arguments");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mg_create: square matrix required");
    BIS_REQUIRE(ctx, !A->view, "bis_mg_create: a row-range view has no diagonal block of its own");
    bis_mg_params p = {10, 256, 0, 1, 4, 0.0, 1.0};
    if (params) p = *params;
    BIS_REQUIRE(ctx, p.max_levels >= 1 && p.max_levels <= kMgMaxLevels && p.coarse_limit >= 1 && p.coarsening >= 0 && p.coarsening <= 2 &&
                         p.nu >= 1 && p.coarse_sweeps >= 1 && p.omega >= 0.0 && p.omega == p.omega && p.coarse_scale == p.coarse_scale,
                "bis_mg_create: bad parameters (1 <= max_levels <= 16, coarse_limit >= 1, coarsening 0..2, nu >= 1, coarse_sweeps >= 1, omega >= 0)");
    bis_mg *mg = new bis_mg;
    mg->p = p;
    mg->smoothed = smoothed;
    mg->prolong_omega = prolong_omega;
    const bis_status st = mg_build(ctx, A, mg);
    if (st != BIS_OK) { mg_free(ctx, mg); return st; }
    *out = mg;
    return BIS_OK;
}

bis_status bis_mg_destroy(bis_ctx *ctx, bis_mg *mg) {
    BIS_CTX_OK(ctx);
    if (mg) mg_free(ctx, mg);
    return BIS_OK;
}

bis_status bis_mg_apply(bis_ctx *ctx, const bis_mg *mg, double *out, const double *in) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, mg, "bis_mg_apply: bad arguments");
    const int64_t n = mg->lv[0].n;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, out && in, "bis_mg_apply: null vector");
    const double *b = in;
    if (out == in) { // the sweeps read the right-hand side after the first one wrote x
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(mg->b0, in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        b = mg->b0;
    }
    return cycle(ctx, mg, 0, out, b);
}

bis_status bis_mg_set_cycle(bis_ctx *ctx, bis_mg *mg, int cycle, int cycle_levels) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, mg, "bis_mg_set_cycle: bad arguments");
    BIS_REQUIRE(ctx, cycle >= BIS_MG_CYCLE_V && cycle <= BIS_MG_CYCLE_K_GCR && cycle_levels >= 0,
                "bis_mg_set_cycle: cycle 0..3 (V, W, K, K-GCR), cycle_levels >= 0");
#define MG_SET_CHECK(call)                                                                                             \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) { ctx->err = std::string("bis_mg_set_cycle: " #call ": ") + hipGetErrorString(e_); return BIS_ERR_HIP; } \
    } while (0)
    MG_SET_CHECK(hipStreamSynchronize(ctx->stream)); // applies in flight read the scratch that may go
    mg->cycle = BIS_MG_CYCLE_V;                      // (what holds if an allocation below fails)
    mg->cycle_levels = 0;
    if (cycle != BIS_MG_CYCLE_V && !mg->ksc) {
        MG_SET_CHECK(hipMalloc(&mg->kpartials, sizeof(double) * 3 * kMaxReduceBlocks));
        MG_SET_CHECK(hipMalloc(&mg->kcounters, sizeof(unsigned) * (4 + kArriveSubs)));
        MG_SET_CHECK(hipMemsetAsync(mg->kcounters, 0, sizeof(unsigned) * (4 + kArriveSubs), ctx->stream));
        double *sc = nullptr;
        const size_t count = kMgScBase + kMgScPer * kMgMaxLevels;
        MG_SET_CHECK(hipMalloc(&sc, sizeof(double) * count));
        std::vector<double> init(count, 0.0);
        init[0] = init[1] = init[3] = 1.0; // W: {c1, c2, zero} = {1, 1, 0}, and the factor 1 of r_2 = r_c - 1 y
        const hipError_t e = hipMemcpy(sc, init.data(), sizeof(double) * count, hipMemcpyHostToDevice);
        if (e != hipSuccess) { hipFree(sc); MG_SET_CHECK(e); }
        mg->ksc = sc;
    }
    for (size_t t = 0; t + 1 < mg->lv.size(); ++t) {
        bis_mg_level &N = mg->lv[t + 1];
        const int kind = transition_cycle(cycle, cycle_levels, mg->lv.size(), t);
        const bool two = kind != BIS_MG_CYCLE_V, kv = kind == BIS_MG_CYCLE_K || kind == BIS_MG_CYCLE_K_GCR;
        const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(N.n, 2);
        if (!two) { hipFree(N.kr); hipFree(N.kd); N.kr = N.kd = nullptr; }
        if (!kv) { hipFree(N.kv); N.kv = nullptr; }
        if (two && !N.kr) MG_SET_CHECK(hipMalloc(&N.kr, bytes));
        if (two && !N.kd) MG_SET_CHECK(hipMalloc(&N.kd, bytes));
        if (kv && !N.kv) MG_SET_CHECK(hipMalloc(&N.kv, bytes));
    }
    MG_SET_CHECK(hipStreamSynchronize(ctx->stream));
#undef MG_SET_CHECK
    mg->cycle = cycle;
    mg->cycle_levels = cycle_levels;
    return BIS_OK;
}

bis_status bis_mg_cycle(const bis_mg *mg, int *cycle, int *cycle_levels) {
    if (!mg) return BIS_ERR_INVALID;
    if (cycle) *cycle = mg->cycle;
    if (cycle_levels) *cycle_levels = mg->cycle_levels;
    return BIS_OK;
}

bis_status bis_mg_set_smoother(bis_ctx *ctx, bis_mg *mg, const bis_mg_smoother *smoother) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, mg && smoother, "bis_mg_set_smoother: bad arguments");
    const bis_mg_smoother s = *smoother;
    BIS_REQUIRE(ctx, s.kind == BIS_MG_SMOOTH_JACOBI || s.kind == BIS_MG_SMOOTH_CHEBYSHEV, "bis_mg_set_smoother: kind 0 (Jacobi) or 1 (Chebyshev)");
    if (s.kind == BIS_MG_SMOOTH_CHEBYSHEV)
        BIS_REQUIRE(ctx, s.degree >= 1 && s.degree <= kMgMaxDegree && s.ratio > 1.0 && s.ratio <= DBL_MAX && s.est_steps >= 0 && s.est_steps <= 100 &&
                             s.safety >= 1.0 && s.safety <= DBL_MAX,
                    "bis_mg_set_smoother: degree 1..8, ratio > 1 and finite, est_steps 0..100, safety >= 1 and finite");
    hipError_t e = hipStreamSynchronize(ctx->stream); // applies in flight read the scratch that may go
    if (e != hipSuccess) { ctx->err = std::string("bis_mg_set_smoother: ") + hipGetErrorString(e); return BIS_ERR_HIP; }
    smoother_to_jacobi(mg); // (what holds if something below fails)
    if (s.kind == BIS_MG_SMOOTH_JACOBI) return BIS_OK;
    if (bis_status st = smoother_setup(ctx, mg, s)) {
        hipStreamSynchronize(ctx->stream);
        smoother_to_jacobi(mg);
        return st;
    }
    for (bis_mg_level &L : mg->lv) L.cheb_degree = L.n ? s.degree : 0;
    mg->sm = s;
    return BIS_OK;
}

bis_status bis_mg_smoother_info(const bis_mg *mg, bis_mg_smoother *out) {
    if (!mg || !out) return BIS_ERR_INVALID;
    *out = mg->sm;
    return BIS_OK;
}

bis_status bis_mg_level_spectrum(const bis_mg *mg, int level, double *bound, double *estimate, double *lambda_max, double *lambda_min) {
    if (!mg || mg->sm.kind != BIS_MG_SMOOTH_CHEBYSHEV || level < 0 || (size_t)level >= mg->lv.size()) return BIS_ERR_INVALID;
    const bis_mg_level &L = mg->lv[(size_t)level];
    if (bound) *bound = L.sp_bound;
    if (estimate) *estimate = L.sp_estimate;
    if (lambda_max) *lambda_max = L.sp_lmax;
    if (lambda_min) *lambda_min = L.sp_lmin;
    return BIS_OK;
}

bis_status bis_mg_level_cheb_coeffs(const bis_mg *mg, int level, double *c1, double *c2) {
    if (!mg || mg->sm.kind != BIS_MG_SMOOTH_CHEBYSHEV || level < 0 || (size_t)level >= mg->lv.size()) return BIS_ERR_INVALID;
    const bis_mg_level &L = mg->lv[(size_t)level];
    for (int k = 0; k < mg->sm.degree; ++k) {
        if (c1) c1[k] = L.cheb_c1[k];
        if (c2) c2[k] = L.cheb_c2[k];
    }
    return BIS_OK;
}

const bis_mat *bis_mg_operand(const bis_mg *mg) { return mg ? mg->operand : nullptr; }

bis_status bis_mg_info(const bis_mg *mg, int *levels, int64_t *rows, int64_t *nnz, int *kind) {
    if (!mg) return BIS_ERR_INVALID;
    if (levels) *levels = (int)mg->lv.size();
    for (size_t l = 0; l < mg->lv.size(); ++l) {
        if (rows) rows[l] = mg->lv[l].n;
        if (nnz) nnz[l] = mg->lv[l].A->nnz;
        if (kind) kind[l] = mg->lv[l].kind;
    }
    return BIS_OK;
}

const bis_mat *bis_mg_level_matrix(const bis_mg *mg, int level) {
    return (mg && level >= 0 && (size_t)level < mg->lv.size()) ? mg->lv[(size_t)level].A : nullptr;
}

const bis_mat *bis_mg_level_prolongator(const bis_mg *mg, int level) {
    return (mg && level >= 0 && (size_t)level < mg->lv.size()) ? mg->lv[(size_t)level].P : nullptr;
}

const bis_mat *bis_mg_level_restrictor(const bis_mg *mg, int level) {
    return (mg && level >= 0 && (size_t)level < mg->lv.size()) ? mg->lv[(size_t)level].R : nullptr;
}

bis_status bis_mg_level_prolong_omega(const bis_mg *mg, int level, double *omega_l) {
    if (!bis_mg_level_prolongator(mg, level) || !omega_l) return BIS_ERR_INVALID;
    *omega_l = mg->lv[(size_t)level].pomega;
    return BIS_OK;
}

bis_status bis_mg_level_aggregates(bis_ctx *ctx, const bis_mg *mg, int level, int32_t *host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, mg && host && level >= 0 && (size_t)level < mg->lv.size(), "bis_mg_level_aggregates: bad arguments");
    const bis_mg_level &L = mg->lv[(size_t)level];
    BIS_REQUIRE(ctx, L.kind != 0, "bis_mg_level_aggregates: the coarsest level has no aggregates");
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(host, L.agg, sizeof(int32_t) * (size_t)L.n, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return BIS_OK;
}

bis_status bis_mg_level_weights(bis_ctx *ctx, const bis_mg *mg, int level, double *host) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, mg && host && level >= 0 && (size_t)level < mg->lv.size(), "bis_mg_level_weights: bad arguments");
    const bis_mg_level &L = mg->lv[(size_t)level];
    if (L.n == 0) return BIS_OK;
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(host, L.w, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return BIS_OK;
}

} // extern "C"
