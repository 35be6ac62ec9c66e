// bis_eigs.hip -- thick-restart Lanczos (Wu and Simon) with full re-orthogonalisation for the k extreme eigenpairs of a
// symmetric matrix, as a sync-free device schedule of the kind bis_fgmres.hip is.  include/bis_hip.h states the algorithm
// line by line; here is how it is laid out.  m = ncv basis blocks V_0 .. V_m (ld = n rounded up to even apart) and the work
// vector W: (m + 2) n-vectors.  One step j (one operator product, the handle's own bis_spmv or the caller's):
//     W = OP V_j                                                      bis_spmv_launch, or the caller between op_begin / op_end
//     h = V_{0..j}^T W      eigs_dots_kernel, one launch per group of at most 8 basis blocks: W is read once per group
//     W -= V_{0..j} h       eigs_update_kernel<false>: one launch, one fma per element and block, ascending block index
//     c = V_{0..j}^T W      eigs_dots_kernel again
//     W -= V_{0..j} c       eigs_update_kernel<true>: (W, W) fused; the last workgroup's lane 0: alpha_j = h_j + c_j,
//                           beta_j = sqrt((W, W)), the product count, the breakdown beta_j <= eps || OP V_j ||
//     V_{j+1} = W / beta_j  eigs_scale_kernel
//     eigs_ritz_kernel (one wave) and eigs_compress_kernel: they act when the cycle closes (j = m - 1, known on the host) or
//     when the update before them met a breakdown (flags[6], known on the device only); otherwise they return at once.
// Traffic per step besides the product: four reads of the j + 1 basis blocks (two by the dots, two by the updates) and
// 2 ceil((j + 1) / 8) + 6 passes over W (the dots' reads, the updates' read and write each, the scale's read and write).
// The Ritz kernel is one wave: T and Y (64 x 64 doubles each) sit in LDS, lane c owns column c of T and row c of Y, the
// rotations of the cyclic Jacobi sweeps follow each other.  The compression V_{0..l) <- V_{0..m) Y_keep works in place, row by
// row: a lane reads its row of all m blocks into registers and then writes l blocks; Y_keep sits in LDS (64 x 64 doubles).
// It walks 8 bytes per lane, not 16: a row of 64 blocks is 128 registers, a pair of rows would be 256.
// The sums are bis_dot's index map with one fma chain per lane and basis block (idr_dots_kernel's accumulators), the block
// and partial sums of reduce_last: no floating-point atomics, no kernel waits for another workgroup, two runs give the same
// bits.  After a stop every launch returns at once (the products through bis_stop_guard).
#include "bis_solver.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

// flags: [0] products, [1] stopped, [2] converged, [3] restarts, [4] reason, [5] nconv, [6] m_eff of a breakdown that waits
// for the Ritz kernel, [7] the basis blocks the compression after this Ritz launch reads (0: it returns at once), [8] the
// blocks it writes, [9] whether it moves V_m to V_l
struct bis_eigs : bis_solver_core {
    const bis_mat *A = nullptr; // null: the caller applies the operator
    int64_t n = 0, ld = 0;
    int k = 0, m = 0, l = 0, which = 0;
    const double *v0 = nullptr; // the caller's start vector or null
    double *V = nullptr;        // m + 1 blocks of ld
    double *W = nullptr;
    double *sc = nullptr; // device state (S_*)
    int j = 0;            // the step the next product belongs to
    int l_cur = 0;        // 0 in the first cycle, l afterwards
    bool op_open = false; // between op_begin and op_end
};

namespace {

constexpr int kT = kSolverT;
constexpr int kM = 64; // kMaxRestart: one wave
constexpr int kLd = kM + 1; // the Ritz kernel's leading dimension in LDS
constexpr int kGroup = 8;
constexpr int kFlags = 12;
constexpr int kMaxSweeps = 30;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxReduceBlocks); // every reducing pass runs on bis_pair_grid(n, kMaxReduceBlocks)

enum { S_ALPHA = 0, S_BETA = kM, S_THETA = 2 * kM, S_S = 3 * kM, S_H = 4 * kM, S_C = 5 * kM, S_VAL = 6 * kM, S_EST = 7 * kM,
       S_TOL = 8 * kM, S_EPS23, S_NRM0, S_WW0 /* (W, W) before the passes */, S_Y = 9 * kM /* Y_keep, row b at S_Y + kM b */, S_COUNT = S_Y + kM * kM };
enum { R_LIVE = 0, R_CONVERGED, R_INVARIANT, R_JACOBI, R_BAD_START };

// the header's hash32 (bis_idr.hip's idr_hash32)
__device__ __forceinline__ uint32_t eigs_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// column 0 of IDR's hashed shadow space: v[i] = (h + 0.5) 2^-31 - 1, h = hash32(hash32(i) ^ 0x9e3779b9); the padding is 0
__global__ __launch_bounds__(kT) void eigs_start_kernel(double *v, int64_t n, int64_t ld) {
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < ld; i += (int64_t)gridDim.x * kT) {
        const uint32_t h = eigs_hash32(eigs_hash32((uint32_t)i) ^ 0x9e3779b9u);
        v[i] = i < n ? ((double)h + 0.5) * 0x1p-31 - 1.0 : 0.0;
    }
}

// out[b0 + i] = (V_{b0 + i}, W) for i < nb <= 8: W is read once.  ww_out (the first group of the first pass; null otherwise):
// *ww_out = (W, W), the square of || OP V_j ||, from the same read.
__global__ __launch_bounds__(kT) void eigs_dots_kernel(int64_t n, int64_t ld, const int *flags, const double *__restrict__ Vb,
                                                       int nb, const double *__restrict__ W, double *out, double *ww_out,
                                                       double *partials, unsigned *counter) {
    __shared__ double lds[(kGroup + 1) * (kT / 64)];
    if (flags[1]) return;
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *V2 = reinterpret_cast<const double2 *>(Vb);
    const double2 *W2 = reinterpret_cast<const double2 *>(W);
    double acc[kGroup + 1];
#pragma unroll
    for (int b = 0; b <= kGroup; ++b) acc[b] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 w = W2[i];
#pragma unroll
        for (int b = 0; b < kGroup; ++b)
            if (b < nb) {
                const double2 v = V2[i + b * ld2];
                acc[b] = fma(v.y, w.y, fma(v.x, w.x, acc[b]));
            }
        acc[kGroup] = fma(w.y, w.y, fma(w.x, w.x, acc[kGroup]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int b = 0; b < kGroup; ++b)
            if (b < nb) acc[b] = fma(Vb[n - 1 + b * ld], W[n - 1], acc[b]);
        acc[kGroup] = fma(W[n - 1], W[n - 1], acc[kGroup]);
    }
    double q[kGroup + 1];
    if (!reduce_last<kGroup + 1>(acc, lds, partials, counter, q)) return;
    if (threadIdx.x != 0) return;
    for (int b = 0; b < nb; ++b) out[b] = q[b];
    if (ww_out) *ww_out = q[kGroup];
}

// W -= sum_{b < nb} coef_b V_b, ascending b.  LAST: (W, W) fused, the last workgroup's lane 0 closes step j
template <bool LAST>
__global__ __launch_bounds__(kT) void eigs_update_kernel(int64_t n, int64_t ld, double *sc, int *flags, int j,
                                                         const double *__restrict__ V, const double *coef,
                                                         double *__restrict__ W, double *partials, unsigned *counter) {
    __shared__ double lds[kT / 64];
    __shared__ double cf[kM];
    if (flags[1]) return;
    const int nb = j + 1;
    if (threadIdx.x < nb) cf[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
    const int64_t n2 = n >> 1, ld2 = ld >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *V2 = reinterpret_cast<const double2 *>(V);
    double2 *W2 = reinterpret_cast<double2 *>(W);
    double acc0 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        double2 w = W2[i];
        for (int b0 = 0; b0 < nb; b0 += kGroup) {
            double2 v[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (b0 + u < nb) v[u] = V2[i + (int64_t)(b0 + u) * ld2];
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (b0 + u < nb) {
                    w.x = fma(-cf[b0 + u], v[u].x, w.x);
                    w.y = fma(-cf[b0 + u], v[u].y, w.y);
                }
        }
        W2[i] = w;
        if (LAST) acc0 = fma(w.y, w.y, fma(w.x, w.x, acc0));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double w = W[n - 1];
        for (int b = 0; b < nb; ++b) w = fma(-cf[b], V[n - 1 + (int64_t)b * ld], w);
        W[n - 1] = w;
        if (LAST) acc0 = fma(w, w, acc0);
    }
    if (!LAST) return;
    const double acc[1] = {acc0};
    double total[1];
    if (!reduce_last<1>(acc, lds, partials, counter, total)) return;
    // every other workgroup has read the stop flag before it arrived: it may change now
    if (threadIdx.x != 0) return;
    double beta = sqrt(total[0]);
    // an invariant subspace: beta_j is 0, or the rounding noise that two passes leave of it (eps^2 || OP V_j ||, where a
    // genuine beta_j is orders above eps || OP V_j ||).  No reciprocal: the Ritz launch behind this step closes the cycle at
    // j + 1 with beta_j = 0.
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

// dst = src / *den (the header's V_{j+1} = W / beta_j and V_0 = v0 / ||v0||)
__global__ __launch_bounds__(kT) void eigs_scale_kernel(int64_t n, const int *flags, const double *den, const double *__restrict__ src,
                                                        double *__restrict__ dst) {
    if (flags[1]) return;
    const double d = *den;
    const int64_t n2 = n >> 1, gs = (int64_t)gridDim.x * kT;
    const double2 *s2 = reinterpret_cast<const double2 *>(src);
    double2 *d2 = reinterpret_cast<double2 *>(dst);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n2; i += gs) {
        const double2 v = s2[i];
        d2[i] = make_double2(v.x / d, v.y / d);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1] / d;
}

// stable insertion sort of idx[0 .. m) by key, ascending; one lane
__device__ void eigs_sort(int *idx, const double *key, int m) {
    for (int i = 1; i < m; ++i) {
        const int t = idx[i];
        const double kt = key[t];
        int p = i - 1;
        while (p >= 0 && key[idx[p]] > kt) { idx[p + 1] = idx[p]; --p; }
        idx[p + 1] = t;
    }
}

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
        eigs_sort(order, theta, me); // ascending, stable
        // rank the ascending list: SA as it is, LA descending, LM descending |theta| (stable on the ascending list)
        for (int i = 0; i < me; ++i) {
            const double th = theta[order[i]];
            key[i] = which == 0 ? 0.0 : which == 1 ? -th : -fabs(th);
        }
        int pos[kM];
        for (int i = 0; i < me; ++i) pos[i] = i;
        if (which != 0) eigs_sort(pos, key, me);
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
        const int restart = flags[3];
        if (restart < hist_cap) { hist[restart] = worst; hist[(size_t)hist_cap + restart] = (double)nconv; }
        flags[3] = restart + 1;
        flags[5] = nconv;
        flags[6] = 0;
        int reason = R_LIVE, conv = 0;
        if (pending) { reason = R_INVARIANT; conv = me >= k; flags[5] = n_ranked; }
        else if (!diagonal) reason = R_JACOBI;
        else if (nconv == k) { reason = R_CONVERGED; conv = 1; }
        if (reason != R_LIVE) {
            flags[1] = 1;
            flags[2] = conv;
            flags[4] = reason;
        }
        // what the compression does: at a stop the wanted vectors, otherwise the kept ones and V_l <- V_m
        flags[7] = me;
        flags[8] = reason != R_LIVE ? n_ranked : l_keep;
        flags[9] = reason == R_LIVE;
        key[0] = reason != R_LIVE ? 1.0 : 0.0;
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

// V_{0..l_out) <- V_{0..me) Y_keep in place, row by row, then V_{l_out} <- V_me (a restart); the counts come from the Ritz
// launch before it (flags[7..9]).  One fma per block, ascending block index, from 0.
__global__ __launch_bounds__(kT) void eigs_compress_kernel(int64_t n, int64_t ld, const int *flags, const double *sc, double *V) {
    __shared__ double Ys[kM * kM];
    const int me = flags[7];
    if (me == 0) return;
    const int l_out = flags[8], move = flags[9];
    for (int e = threadIdx.x; e < me * kM; e += kT) Ys[e] = sc[S_Y + e];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        double row[kM];
#pragma unroll
        for (int b = 0; b < kM; ++b) row[b] = b < me ? V[i + (int64_t)b * ld] : 0.0;
        const double tail = move ? V[i + (int64_t)me * ld] : 0.0;
        for (int c = 0; c < l_out; ++c) {
            double a = 0.0;
#pragma unroll
            for (int b = 0; b < kM; ++b)
                if (b < me) a = fma(row[b], Ys[b * kM + c], a);
            V[i + (int64_t)c * ld] = a;
        }
        if (move) V[i + (int64_t)l_out * ld] = tail;
    }
}

inline int lane_grid(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + kT - 1) / kT, 1), kMaxEwBlocks); }

// what follows a product in W: the rest of step j, and the restart when the cycle closes
void eigs_enqueue_step(bis_ctx *ctx, bis_eigs *s) {
    const int64_t n = s->n, ld = s->ld;
    const int j = s->j, g = bis_pair_grid(n, kMaxReduceBlocks), g_wide = bis_pair_grid(n, kMaxEwBlocks);
    const int *flags = s->flags;
    for (int pass = 0; pass < 2; ++pass) {
        double *coef = s->sc + (pass == 0 ? S_H : S_C);
        for (int b0 = 0; b0 <= j; b0 += kGroup)
            hipLaunchKernelGGL(eigs_dots_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, ld, flags, (const double *)(s->V + b0 * ld),
                               std::min(kGroup, j + 1 - b0), (const double *)s->W, coef + b0,
                               pass == 0 && b0 == 0 ? s->sc + S_WW0 : (double *)nullptr, ctx->partials, s->counters);
        if (pass == 0)
            hipLaunchKernelGGL((eigs_update_kernel<false>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, s->sc, s->flags, j,
                               (const double *)s->V, (const double *)coef, s->W, ctx->partials, s->counters);
        else
            hipLaunchKernelGGL((eigs_update_kernel<true>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, s->sc, s->flags, j,
                               (const double *)s->V, (const double *)coef, s->W, ctx->partials, s->counters);
    }
    hipLaunchKernelGGL(eigs_scale_kernel, dim3(g_wide), dim3(kT), 0, ctx->stream, n, flags, (const double *)(s->sc + S_BETA + j),
                       (const double *)s->W, s->V + (int64_t)(j + 1) * ld);
    const int close = j == s->m - 1;
    hipLaunchKernelGGL(eigs_ritz_kernel, dim3(1), dim3(64), 0, ctx->stream, s->sc, s->flags, close, s->m, s->l_cur, s->l, s->k,
                       s->which, s->hist, s->hist_cap);
    hipLaunchKernelGGL(eigs_compress_kernel, dim3(lane_grid(n)), dim3(kT), 0, ctx->stream, n, ld, flags, (const double *)s->sc, s->V);
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
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_eigs_set_start: null handle");
    BIS_REQUIRE(ctx, !bis_solver_live(*s), "bis_eigs_set_start: call it before bis_eigs_init");
    BIS_REQUIRE(ctx, aligned16(v0), "bis_eigs_set_start: v0 must be 16-byte aligned");
    s->v0 = v0;
    return BIS_OK;
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
    s->enqueued = 0;
    s->j = 0;
    s->l_cur = 0;
    s->op_open = false;
    const int64_t n = s->n, ld = s->ld;
    bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) return st;
    // every earlier state goes: basis, work vector, scalars, flags, counters, history
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->V, 0, sizeof(double) * (size_t)ld * (s->m + 1), ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->W, 0, sizeof(double) * (size_t)ld, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->sc, 0, sizeof(double) * S_COUNT, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->flags, 0, sizeof(int) * kFlags, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->counters, 0, sizeof(unsigned) * kCounterSet, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->hist, 0, sizeof(double) * 2 * (size_t)s->hist_cap, ctx->stream));
    if (s->v0)
        st = bis_copy_vector(ctx, s->W, s->v0, n);
    else
        hipLaunchKernelGGL(eigs_start_kernel, dim3(lane_grid(ld)), dim3(kT), 0, ctx->stream, s->W, n, ld);
    double vv = 0.0;
    if (st == BIS_OK) st = bis_dot(ctx, s->W, s->W, n, &vv);
    if (st != BIS_OK) return st;
    const double nrm = sqrt(vv);
    double head[3] = {tol, std::pow(DBL_EPSILON, 2.0 / 3.0), nrm};
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc + S_TOL, head, sizeof head, hipMemcpyHostToDevice, ctx->stream));
    if (!(nrm > 0.0) || !std::isfinite(nrm)) {
        int flags[kFlags] = {0};
        flags[1] = 1;
        flags[4] = R_BAD_START;
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->flags, flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(eigs_scale_kernel, dim3(bis_pair_grid(n, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, n, (const int *)s->flags,
                           (const double *)(s->sc + S_NRM0), (const double *)s->W, s->V);
        BIS_HIP_CHECK(ctx, hipGetLastError());
    }
    BIS_SYNC_CHECK(ctx);
    s->initialised = true;
    return BIS_OK;
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
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, "bis_eigs_status: null handle");
    int flags[kFlags] = {0};
    if (bis_status st = bis_solver_read_flags(ctx, *s, 0, kFlags, flags)) return st;
    if (products) *products = flags[0];
    if (restarts) *restarts = flags[3];
    if (stopped) *stopped = flags[1];
    if (converged) *converged = flags[2];
    if (reason) *reason = flags[4];
    if (nconv) *nconv = flags[5];
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
