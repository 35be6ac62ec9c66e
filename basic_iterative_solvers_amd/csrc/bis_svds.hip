// bis_svds.hip -- Golub-Kahan-Lanczos bidiagonalisation with thick restart and full re-orthogonalisation for the k largest or
// smallest singular triplets of a rectangular matrix, as a sync-free device schedule of the kind bis_eigs.hip is.
// include/bis_hip.h states the algorithm line by line; here is how it is laid out.  F is the tall orientation of A (A itself
// when rows >= cols, A^T otherwise).  Two bases: P_0 .. P_m of ns = min(rows, cols) entries and Q_0 .. Q_{m-1} of nl =
// max(rows, cols), each with its own leading dimension (the length rounded up to even).  No work vector: a product writes
// into its destination block W (Q_j in the left half of step j, P_{j+1} in the right half), which is orthogonalised against
// the nb blocks before it in the same basis (j in the left half, j + 1 in the right) and scaled in place:
//     W = F P_j  or  F^T Q_j                  bis_spmv_launch on A or At, or the caller between op_begin / op_end
//     h = B_{0..nb)^T W                       svds_dots_kernel, one launch per group of at most 8 blocks: W is read once per group
//     W -= B_{0..nb) h                        svds_update_kernel<false>: one launch, one fma per element and block, ascending
//     h = B_{0..nb)^T W                       svds_dots_kernel again
//     W -= B_{0..nb) h                        svds_update_kernel<true>: (W, W) fused; the last workgroup's lane 0: alpha_j or
//                                             beta_j = sqrt((W, W)), the product count, the breakdown test
//     W = W / alpha_j  or  W / beta_j         svds_scale_kernel
//     svds_restart_kernel (one wave), svds_compress_kernel on P and on Q: they act when the cycle closes (the right half of
//     j = m - 1, known on the host) or when the update before them met a breakdown (flags[6], known on the device only);
//     otherwise they return at once.
// With j = 0 the left half has nothing to orthogonalise against: one svds_update_kernel<true> launch sums the norm.
// The restart kernel is one wave: G (B rotated into X Sigma) and Y, 64 x 65 doubles each, sit in LDS, column c of either at
// [c * 65 + r]; the one-sided Jacobi sweeps walk a round-robin schedule, one lane per pair of columns, so the m_eff / 2 pairs of
// a round rotate at once and the lanes' column-strided accesses fall into different banks.  The compressions work in place,
// row by row, 8 bytes per lane (a lane holds a row of up to 64 blocks), as eigs_compress_kernel does.
// The sums are bis_dot's index map with one fma chain per lane and basis block, the block and partial sums of reduce_last:
// no floating-point atomics, no kernel waits for another workgroup, two runs give the same bits.  After a stop every
// launch returns at once (the products through bis_stop_guard).  The unit shares no kernel with bis_eigs.hip.
#include "bis_solver.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

// flags: [0] products, [1] stopped, [2] converged, [3] restarts, [4] reason, [5] nconv, [6] m_eff of a breakdown that waits
// for the restart kernel, [7] the basis blocks the compressions after this restart launch read (0: they return at once),
// [8] the blocks they write, [9] whether P_m moves to P_l, [10] 1 + the block of Q that counts as 0 (an alpha breakdown)
struct bis_svds : bis_solver_core {
    const bis_mat *A = nullptr, *At = nullptr; // both null: the caller applies the products
    bis_mat *At_owned = nullptr;                // bis_mat_transpose(A) when the caller passed none
    int64_t rows = 0, cols = 0, ns = 0, nl = 0, ldp = 0, ldq = 0;
    bool flip = false; // rows < cols: F = A^T
    int k = 0, m = 0, l = 0, which = 0;
    const double *v0 = nullptr; // the caller's start vector or null
    double *P = nullptr;        // m + 1 blocks of ldp
    double *Q = nullptr;        // m blocks of ldq
    double *sc = nullptr;       // device state (S_*)
    int j = 0;                  // the step the next product belongs to
    int half = 0;               // 0: the next product is F P_j, 1: F^T Q_j
    int l_cur = 0;              // 0 in the first cycle, l afterwards
    bool op_open = false;       // between op_begin and op_end
};

namespace {

constexpr int kT = kSolverT;
constexpr int kM = 64;      // the largest basis: one wave
constexpr int kLd = kM + 1; // the restart kernel's leading dimension in LDS
constexpr int kGroup = 8;
constexpr int kFlags = 12;
constexpr int kMaxSweeps = 30;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxReduceBlocks); // every reducing pass runs on bis_pair_grid(n, kMaxReduceBlocks)

enum { S_ALPHA = 0, S_BETA = kM, S_SIGMA = 2 * kM, S_S = 3 * kM, S_H = 4 * kM, S_VAL = 5 * kM, S_EST = 6 * kM,
       S_TOL = 7 * kM, S_NRM0, S_WW0 /* (W, W) before the passes */, S_SREF, S_Y = 8 * kM /* Y_keep, row b at S_Y + kM b */,
       S_X = S_Y + kM * kM /* X_keep */, S_COUNT = S_X + kM * kM };
enum { R_LIVE = 0, R_CONVERGED, R_INVARIANT, R_JACOBI, R_BAD_START };

// the header's hash32 (bis_idr.hip's idr_hash32)
__device__ __forceinline__ uint32_t svds_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// column 0 of IDR's hashed shadow space: v[i] = (h + 0.5) 2^-31 - 1, h = hash32(hash32(i) ^ 0x9e3779b9); the padding is 0
__global__ __launch_bounds__(kT) void svds_start_kernel(double *v, int64_t n, int64_t ld) {
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < ld; i += (int64_t)gridDim.x * kT) {
        const uint32_t h = svds_hash32(svds_hash32((uint32_t)i) ^ 0x9e3779b9u);
        v[i] = i < n ? ((double)h + 0.5) * 0x1p-31 - 1.0 : 0.0;
    }
}

// out[i] = (B_i, W) for i < nb <= 8, B_i = Bb + i ld: W is read once.  ww_out (the first group of the first pass; null
// otherwise): *ww_out = (W, W), the square of the product's norm, from the same read.
__global__ __launch_bounds__(kT) void svds_dots_kernel(int64_t n, int64_t ld, const int *flags, const double *__restrict__ Bb,
                                                       int nb, const double *__restrict__ W, double *out, double *ww_out,
                                                       double *partials, unsigned *counter) {
    __shared__ double lds[(kGroup + 1) * (kT / 64)];
    if (flags[1]) return;
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *B2 = reinterpret_cast<const double2 *>(Bb);
    const double2 *W2 = reinterpret_cast<const double2 *>(W);
    double acc[kGroup + 1];
#pragma unroll
    for (int b = 0; b <= kGroup; ++b) acc[b] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 w = W2[i];
#pragma unroll
        for (int b = 0; b < kGroup; ++b)
            if (b < nb) {
                const double2 v = B2[i + b * ld2];
                acc[b] = fma(v.y, w.y, fma(v.x, w.x, acc[b]));
            }
        acc[kGroup] = fma(w.y, w.y, fma(w.x, w.x, acc[kGroup]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int b = 0; b < kGroup; ++b)
            if (b < nb) acc[b] = fma(Bb[n - 1 + b * ld], W[n - 1], acc[b]);
        acc[kGroup] = fma(W[n - 1], W[n - 1], acc[kGroup]);
    }
    double q[kGroup + 1];
    if (!reduce_last<kGroup + 1>(acc, lds, partials, counter, q)) return;
    if (threadIdx.x != 0) return;
    for (int b = 0; b < nb; ++b) out[b] = q[b];
    if (ww_out) *ww_out = q[kGroup];
}

// W -= sum_{b < nb} coef_b B_b, ascending b (nb = 0: W stays).  LAST: (W, W) fused, the last workgroup's lane 0 closes the
// half step: half = 0 forms alpha_j, half = 1 beta_j
template <bool LAST>
__global__ __launch_bounds__(kT) void svds_update_kernel(int64_t n, int64_t ld, double *sc, int *flags, int j, int half, int nb,
                                                         const double *__restrict__ B, const double *coef,
                                                         double *__restrict__ W, double *partials, unsigned *counter) {
    __shared__ double lds[kT / 64];
    __shared__ double cf[kM];
    if (flags[1]) return;
    if ((int)threadIdx.x < nb) cf[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *B2 = reinterpret_cast<const double2 *>(B);
    double2 *W2 = reinterpret_cast<double2 *>(W);
    double acc0 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 w = W2[i];
        for (int b0 = 0; b0 < nb; b0 += kGroup) {
            double2 v[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (b0 + u < nb) v[u] = B2[i + (int64_t)(b0 + u) * ld2];
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (b0 + u < nb) {
                    w.x = fma(-cf[b0 + u], v[u].x, w.x);
                    w.y = fma(-cf[b0 + u], v[u].y, w.y);
                }
        }
        if (nb) W2[i] = w;
        if (LAST) acc0 = fma(w.y, w.y, fma(w.x, w.x, acc0));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double w = W[n - 1];
        for (int b = 0; b < nb; ++b) w = fma(-cf[b], B[n - 1 + (int64_t)b * ld], w);
        if (nb) W[n - 1] = w;
        if (LAST) acc0 = fma(w, w, acc0);
    }
    if (!LAST) return;
    const double acc[1] = {acc0};
    double total[1];
    if (!reduce_last<1>(acc, lds, partials, counter, total)) return;
    // every other workgroup has read the stop flag before it arrived: it may change now
    if (threadIdx.x != 0) return;
    double nrm = sqrt(total[0]);
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

// v = v / *den in place (the header's Q_j / alpha_j, P_{j+1} / beta_j and P_0 = v0 / ||v0||)
__global__ __launch_bounds__(kT) void svds_scale_kernel(int64_t n, const int *flags, const double *den, double *v) {
    if (flags[1]) return;
    const double d = *den;
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    double2 *v2 = reinterpret_cast<double2 *>(v);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 x = v2[i];
        v2[i] = make_double2(x.x / d, x.y / d);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[n - 1] = v[n - 1] / d;
}

// stable insertion sort of idx[0 .. m) by key, ascending; one lane
__device__ void svds_sort(int *idx, const double *key, int m) {
    for (int i = 1; i < m; ++i) {
        const int t = idx[i];
        const double kt = key[t];
        int p = i - 1;
        while (p >= 0 && key[idx[p]] > kt) { idx[p + 1] = idx[p]; --p; }
        idx[p + 1] = t;
    }
}

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
        svds_sort(order, sig, me); // ascending, stable
        for (int i = 0; i < me; ++i) key[i] = which == 1 ? 0.0 : -sig[order[i]];
        int pos[kM];
        for (int i = 0; i < me; ++i) pos[i] = i;
        if (which != 1) svds_sort(pos, key, me);
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
        const int restart = flags[3];
        if (restart < hist_cap) { hist[restart] = worst; hist[(size_t)hist_cap + restart] = (double)nconv; }
        flags[3] = restart + 1;
        flags[5] = nconv;
        flags[6] = 0;
        int reason = R_LIVE, conv = 0;
        if (pending) { reason = R_INVARIANT; conv = me >= k; flags[5] = n_ranked; }
        else if (!finished) reason = R_JACOBI;
        else if (nconv == k) { reason = R_CONVERGED; conv = 1; }
        if (reason != R_LIVE) {
            flags[1] = 1;
            flags[2] = conv;
            flags[4] = reason;
        }
        // what the compressions do: at a stop the wanted vectors, otherwise the kept ones and P_l <- P_m
        flags[7] = me;
        flags[8] = reason != R_LIVE ? n_ranked : l_keep;
        flags[9] = reason == R_LIVE;
        key[0] = reason != R_LIVE ? 1.0 : 0.0;
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

// V_{0..l_out) <- V_{0..me) C in place, row by row (C: Y_keep or X_keep in sc at c_off), then, move_tail (the basis P at a
// restart): V_{l_out} <- V_me; the counts come from the restart launch before it (flags[7..9]).  zero_flag: the basis Q, whose
// block flags[10] - 1 counts as 0.  One fma per block, ascending block index, from 0.
__global__ __launch_bounds__(kT) void svds_compress_kernel(int64_t n, int64_t ld, const int *flags, const double *sc, int c_off,
                                                           int is_p, double *V) {
    __shared__ double Cs[kM * kM];
    const int me = flags[7];
    if (me == 0) return;
    const int l_out = flags[8], move = is_p ? flags[9] : 0, zero = is_p ? -1 : flags[10] - 1;
    for (int e = threadIdx.x; e < me * kM; e += kT) Cs[e] = sc[c_off + e];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        double row[kM];
#pragma unroll
        for (int b = 0; b < kM; ++b) row[b] = b < me && b != zero ? V[i + (int64_t)b * ld] : 0.0;
        const double tail = move ? V[i + (int64_t)me * ld] : 0.0;
        for (int c = 0; c < l_out; ++c) {
            double a = 0.0;
#pragma unroll
            for (int b = 0; b < kM; ++b)
                if (b < me) a = fma(row[b], Cs[b * kM + c], a);
            V[i + (int64_t)c * ld] = a;
        }
        if (move) V[i + (int64_t)l_out * ld] = tail;
    }
}

inline int lane_grid(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + kT - 1) / kT, 1), kMaxEwBlocks); }

// what follows a product: the rest of the half step, and the restart when the cycle closes
void svds_enqueue_half(bis_ctx *ctx, bis_svds *s) {
    const int j = s->j, half = s->half;
    const int64_t n = half ? s->ns : s->nl, ld = half ? s->ldp : s->ldq;
    double *B = half ? s->P : s->Q;
    double *W = B + (int64_t)(half ? j + 1 : j) * ld;
    const int nb = half ? j + 1 : j;
    const int g = bis_pair_grid(n, kMaxReduceBlocks), g_wide = bis_pair_grid(n, kMaxEwBlocks);
    const int *flags = s->flags;
    double *coef = s->sc + S_H;
    for (int pass = nb ? 0 : 1; pass < 2; ++pass) {
        for (int b0 = 0; b0 < nb; b0 += kGroup)
            hipLaunchKernelGGL(svds_dots_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, ld, flags, (const double *)(B + b0 * ld),
                               std::min(kGroup, nb - b0), (const double *)W, coef + b0,
                               pass == 0 && b0 == 0 ? s->sc + S_WW0 : (double *)nullptr, ctx->partials, s->counters);
        if (pass == 0)
            hipLaunchKernelGGL((svds_update_kernel<false>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, s->sc, s->flags, j, half, nb,
                               (const double *)B, (const double *)coef, W, ctx->partials, s->counters);
        else
            hipLaunchKernelGGL((svds_update_kernel<true>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, s->sc, s->flags, j, half, nb,
                               (const double *)B, (const double *)coef, W, ctx->partials, s->counters);
    }
    hipLaunchKernelGGL(svds_scale_kernel, dim3(g_wide), dim3(kT), 0, ctx->stream, n, flags,
                       (const double *)(s->sc + (half ? S_BETA : S_ALPHA) + j), W);
    const int close = half && j == s->m - 1;
    hipLaunchKernelGGL(svds_restart_kernel, dim3(1), dim3(64), 0, ctx->stream, s->sc, s->flags, close, s->m, s->l_cur, s->l, s->k,
                       s->which, s->hist, s->hist_cap);
    hipLaunchKernelGGL(svds_compress_kernel, dim3(lane_grid(s->ns)), dim3(kT), 0, ctx->stream, s->ns, s->ldp, flags,
                       (const double *)s->sc, (int)S_Y, 1, s->P);
    hipLaunchKernelGGL(svds_compress_kernel, dim3(lane_grid(s->nl)), dim3(kT), 0, ctx->stream, s->nl, s->ldq, flags,
                       (const double *)s->sc, (int)S_X, 0, s->Q);
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
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_svds_set_start: null handle");
    BIS_REQUIRE(ctx, !bis_solver_live(*s), "bis_svds_set_start: call it before bis_svds_init");
    BIS_REQUIRE(ctx, aligned16(v0), "bis_svds_set_start: v0 must be 16-byte aligned");
    s->v0 = v0;
    return BIS_OK;
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
    s->enqueued = 0;
    s->j = 0;
    s->half = 0;
    s->l_cur = 0;
    s->op_open = false;
    const int64_t n = s->ns, ld = s->ldp;
    bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) return st;
    // every earlier state goes: both bases, scalars, flags, counters, history
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->P, 0, sizeof(double) * (size_t)ld * (s->m + 1), ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->Q, 0, sizeof(double) * (size_t)s->ldq * s->m, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->sc, 0, sizeof(double) * S_COUNT, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->flags, 0, sizeof(int) * kFlags, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->counters, 0, sizeof(unsigned) * kCounterSet, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->hist, 0, sizeof(double) * 2 * (size_t)s->hist_cap, ctx->stream));
    if (s->v0)
        st = bis_copy_vector(ctx, s->P, s->v0, n);
    else
        hipLaunchKernelGGL(svds_start_kernel, dim3(lane_grid(ld)), dim3(kT), 0, ctx->stream, s->P, n, ld);
    double vv = 0.0;
    if (st == BIS_OK) st = bis_dot(ctx, s->P, s->P, n, &vv);
    if (st != BIS_OK) return st;
    const double nrm = sqrt(vv);
    double head[2] = {tol, nrm};
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc + S_TOL, head, sizeof head, hipMemcpyHostToDevice, ctx->stream));
    if (!(nrm > 0.0) || !std::isfinite(nrm)) {
        int flags[kFlags] = {0};
        flags[1] = 1;
        flags[4] = R_BAD_START;
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->flags, flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(svds_scale_kernel, dim3(bis_pair_grid(n, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, n, (const int *)s->flags,
                           (const double *)(s->sc + S_NRM0), s->P);
        BIS_HIP_CHECK(ctx, hipGetLastError());
    }
    BIS_SYNC_CHECK(ctx);
    s->initialised = true;
    return BIS_OK;
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
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_svds_status: null handle");
    int flags[kFlags] = {0};
    if (bis_status st = bis_solver_read_flags(ctx, *s, 0, kFlags, flags)) return st;
    if (products) *products = flags[0];
    if (restarts) *restarts = flags[3];
    if (stopped) *stopped = flags[1];
    if (converged) *converged = flags[2];
    if (reason) *reason = flags[4];
    if (nconv) *nconv = flags[5];
    if (sigma_ref) BIS_HIP_CHECK(ctx, hipMemcpy(sigma_ref, s->sc + S_SREF, sizeof(double), hipMemcpyDeviceToHost));
    if (values_host) BIS_HIP_CHECK(ctx, hipMemcpy(values_host, s->sc + S_VAL, sizeof(double) * s->k, hipMemcpyDeviceToHost));
    if (est_host) BIS_HIP_CHECK(ctx, hipMemcpy(est_host, s->sc + S_EST, sizeof(double) * s->k, hipMemcpyDeviceToHost));
    if (hist_cap > 0 && s->initialised) {
        const int cnt = std::min(flags[3], hist_cap);
        if (hist_host && cnt > 0)
            if (bis_status st = bis_solver_copy_hist(ctx, *s, 0, cnt, hist_host)) return st;
        if (hist_nconv_host && cnt > 0)
            if (bis_status st = bis_solver_copy_hist(ctx, *s, 1, cnt, hist_nconv_host)) return st;
    }
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
