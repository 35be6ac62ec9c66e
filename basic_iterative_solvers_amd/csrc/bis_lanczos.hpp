// bis_lanczos.hpp -- what the two thick-restart Lanczos units share (bis_eigs.hip, bis_svds.hip): the passes over n-vectors
// of one step (block dots, block update, scale), the hashed start vector, the in-place compression of a basis at a restart,
// the restart kernel's verdict once the small dense problem is solved, and the host side of a handle's life cycle that
// does not depend on the method.  Each unit compiles its own copy (an unnamed namespace) and keeps its restart kernel, how
// the last update closes a step (a functor handed to lanczos_update_kernel), its step schedule and its *_vectors call.
// The sums are bis_dot's index map with one fma chain per lane and basis block (idr_dots_kernel's accumulators), the block
// and partial sums of reduce_last: no floating-point atomics, no kernel waits for another workgroup, two runs give the same
// bits.
#pragma once

#include "bis_solver.hpp"

#include <cfloat>
#include <cmath>

// flags: [0] products, [1] stopped, [2] converged, [3] restarts, [4] reason, [5] nconv, [6] m_eff of a breakdown that waits
// for the restart kernel, [7] the basis blocks the compressions after this restart launch read (0: they return at once),
// [8] the blocks they write, [9] whether the block behind the basis (V_m, P_m) moves to block l.  ([10]: bis_svds.hip)
struct bis_lanczos_core : bis_solver_core {
    int k = 0, m = 0, l = 0, which = 0;
    const double *v0 = nullptr; // the caller's start vector or null
    double *sc = nullptr;       // device state (the unit's S_*)
    int j = 0;                  // the step the next product belongs to
    int l_cur = 0;              // 0 in the first cycle, l afterwards
    bool op_open = false;       // between op_begin and op_end
};

namespace {

constexpr int kT = kSolverT;
constexpr int kM = 64;      // the largest basis (kMaxRestart): one wave
constexpr int kLd = kM + 1; // the restart kernel's leading dimension in LDS
constexpr int kGroup = 8;
constexpr int kFlags = 12;
constexpr int kMaxSweeps = 30;
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxReduceBlocks); // every reducing pass runs on bis_pair_grid(n, kMaxReduceBlocks)

enum { R_LIVE = 0, R_CONVERGED, R_INVARIANT, R_JACOBI, R_BAD_START };

// column 0 of IDR's hashed shadow space: v[i] = (h + 0.5) 2^-31 - 1, h = hash32(hash32(i) ^ 0x9e3779b9); the padding is 0
__global__ __launch_bounds__(kT) void lanczos_start_kernel(double *v, int64_t n, int64_t ld) {
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < ld; i += (int64_t)gridDim.x * kT) {
        const uint32_t h = bis_hash32(bis_hash32((uint32_t)i) ^ 0x9e3779b9u);
        v[i] = i < n ? ((double)h + 0.5) * 0x1p-31 - 1.0 : 0.0;
    }
}

// out[i] = (B_i, W) for i < nb <= 8, B_i = Bb + i ld: W is read once.  ww_out (the first group of the first pass; null
// otherwise): *ww_out = (W, W), the square of the product's norm, from the same read.
__global__ __launch_bounds__(kT) void lanczos_dots_kernel(int64_t n, int64_t ld, const int *flags, const double *__restrict__ Bb,
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

// W -= sum_{b < nb} coef_b B_b, ascending b (nb = 0: W stays).  LAST: (W, W) fused, and lane 0 of the workgroup that arrives
// last hands it to close, which closes the (half) step: the unit's scalars, the product count, the breakdown test.  Without
// LAST close is not called.
template <bool LAST, class Close>
__global__ __launch_bounds__(kT) void lanczos_update_kernel(int64_t n, int64_t ld, const int *flags, int nb,
                                                            const double *__restrict__ B, const double *coef,
                                                            double *__restrict__ W, double *partials, unsigned *counter, Close close) {
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
    close(total[0]);
}

// dst = src / *den; in place with src == dst
__global__ __launch_bounds__(kT) void lanczos_scale_kernel(int64_t n, const int *flags, const double *den, const double *src, double *dst) {
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
__device__ void lanczos_sort(int *idx, const double *key, int m) {
    for (int i = 1; i < m; ++i) {
        const int t = idx[i];
        const double kt = key[t];
        int p = i - 1;
        while (p >= 0 && key[idx[p]] > kt) { idx[p + 1] = idx[p]; --p; }
        idx[p + 1] = t;
    }
}

// Lane 0 of a restart kernel, once the small problem is solved (jacobi_ok) and the nconv of the k wanted values that passed
// the test and the worst of their estimates are known: the history entry, the restart count, the reason ladder (pending: a
// breakdown closed the cycle at m_eff = me), and what the compressions behind this launch do.  Returns whether the solve
// stopped.
__device__ bool lanczos_verdict(int *flags, double *hist, int hist_cap, int pending, bool jacobi_ok, int nconv, double worst,
                                int k, int me, int l_keep) {
    const int n_ranked = min(k, me);
    const int restart = flags[3];
    if (restart < hist_cap) { hist[restart] = worst; hist[(size_t)hist_cap + restart] = (double)nconv; }
    flags[3] = restart + 1;
    flags[5] = nconv;
    flags[6] = 0;
    int reason = R_LIVE, conv = 0;
    if (pending) { reason = R_INVARIANT; conv = me >= k; flags[5] = n_ranked; }
    else if (!jacobi_ok) reason = R_JACOBI;
    else if (nconv == k) { reason = R_CONVERGED; conv = 1; }
    if (reason != R_LIVE) {
        flags[1] = 1;
        flags[2] = conv;
        flags[4] = reason;
    }
    // at a stop the wanted vectors, otherwise the kept ones and the block behind the basis moves to block l
    flags[7] = me;
    flags[8] = reason != R_LIVE ? n_ranked : l_keep;
    flags[9] = reason == R_LIVE;
    return reason != R_LIVE;
}

// V_{0..l_out) <- V_{0..me) C in place, row by row (C: me x l_out, row b at C + kM b); the counts come from the restart launch
// before it (flags[7..9]).  Without ZERO (V, P) a restart also moves the block behind the basis, V_{l_out} <- V_me; with ZERO
// (Q, which has no such block) block flags[10] - 1 counts as 0.  A template argument: as kernel arguments the two choices
// cost the eigensolver's closing step 4 to 7 % (docs/EXPERIMENTS.md §43).  One fma per block, ascending block index, from 0.
// It walks 8 bytes per lane, not 16: a row of 64 blocks is 128 registers, a pair of rows would be 256.
template <bool ZERO>
__global__ __launch_bounds__(kT) void lanczos_compress_kernel(int64_t n, int64_t ld, const int *flags, const double *C, double *V) {
    __shared__ double Cs[kM * kM];
    const int me = flags[7];
    if (me == 0) return;
    const int l_out = flags[8], move = ZERO ? 0 : flags[9], zero = ZERO ? flags[10] - 1 : -1;
    for (int e = threadIdx.x; e < me * kM; e += kT) Cs[e] = C[e];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        double row[kM];
#pragma unroll
        for (int b = 0; b < kM; ++b) row[b] = b < me && (!ZERO || b != zero) ? V[i + (int64_t)b * ld] : 0.0;
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

// ---- the host side: `unit` is "bis_eigs" or "bis_svds", the head of every message -------------------------------------------

// What follows a product in W (n entries, the block of leading dimension ld behind B_0 .. B_{nb-1} or a vector of its own): two
// passes of block dots (coefficients to h, then to c; the first launch also sums (W, W) into *ww) and block update, the
// second update closing the step with `close`; then dst = W / *den.  nb = 0: the closing update alone, which sums the norm.
template <class Close>
void lanczos_enqueue_passes(bis_ctx *ctx, bis_lanczos_core *s, int64_t n, int64_t ld, const double *B, int nb, double *W, double *h,
                            double *c, double *ww, Close close, const double *den, double *dst) {
    const int g = bis_pair_grid(n, kMaxReduceBlocks);
    const int *flags = s->flags;
    for (int pass = nb ? 0 : 1; pass < 2; ++pass) {
        double *coef = pass == 0 ? h : c;
        for (int b0 = 0; b0 < nb; b0 += kGroup)
            hipLaunchKernelGGL(lanczos_dots_kernel, dim3(g), dim3(kT), 0, ctx->stream, n, ld, flags, B + b0 * ld, std::min(kGroup, nb - b0),
                               (const double *)W, coef + b0, pass == 0 && b0 == 0 ? ww : (double *)nullptr, ctx->partials, s->counters);
        if (pass == 0)
            hipLaunchKernelGGL((lanczos_update_kernel<false, Close>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, flags, nb, B,
                               (const double *)coef, W, ctx->partials, s->counters, close);
        else
            hipLaunchKernelGGL((lanczos_update_kernel<true, Close>), dim3(g), dim3(kT), 0, ctx->stream, n, ld, flags, nb, B,
                               (const double *)coef, W, ctx->partials, s->counters, close);
    }
    hipLaunchKernelGGL(lanczos_scale_kernel, dim3(bis_pair_grid(n, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, n, flags, den,
                       (const double *)W, dst);
}

bis_status lanczos_set_start(bis_ctx *ctx, bis_lanczos_core *s, const double *v0, const char *unit) {
    const std::string u(unit);
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, u + "_set_start: null handle");
    BIS_REQUIRE(ctx, !bis_solver_live(*s), u + "_set_start: call it before " + u + "_init");
    BIS_REQUIRE(ctx, aligned16(v0), u + "_set_start: v0 must be 16-byte aligned");
    s->v0 = v0;
    return BIS_OK;
}

// The end of *_init, after the unit has cleared its bases and its state: flags, counters and history go, w (n entries, ld
// with the padding) takes the caller's start vector or the hashed one, sc[s_tol] = tol, sc[s_nrm0] = ||w||, and either the
// solve stops at once (R_BAD_START: a zero or non-finite norm) or dst = w / ||w||.  Blocks.
bis_status lanczos_init(bis_ctx *ctx, bis_lanczos_core *s, int64_t n, int64_t ld, double *w, double *dst, double tol, int s_tol,
                        int s_nrm0) {
    s->enqueued = 0;
    s->j = 0;
    s->l_cur = 0;
    s->op_open = false;
    bis_status st = bis_ensure_partials(ctx, (size_t)(kGroup + 1) * kMaxReduceBlocks);
    if (st != BIS_OK) return st;
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->flags, 0, sizeof(int) * kFlags, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->counters, 0, sizeof(unsigned) * kCounterSet, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(s->hist, 0, sizeof(double) * 2 * (size_t)s->hist_cap, ctx->stream));
    if (s->v0)
        st = bis_copy_vector(ctx, w, s->v0, n);
    else
        hipLaunchKernelGGL(lanczos_start_kernel, dim3(lane_grid(ld)), dim3(kT), 0, ctx->stream, w, n, ld);
    double vv = 0.0;
    if (st == BIS_OK) st = bis_dot(ctx, w, w, n, &vv);
    if (st != BIS_OK) return st;
    const double nrm = sqrt(vv);
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc + s_tol, &tol, sizeof tol, hipMemcpyHostToDevice, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->sc + s_nrm0, &nrm, sizeof nrm, hipMemcpyHostToDevice, ctx->stream));
    if (!(nrm > 0.0) || !std::isfinite(nrm)) {
        int flags[kFlags] = {0};
        flags[1] = 1;
        flags[4] = R_BAD_START;
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(s->flags, flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(lanczos_scale_kernel, dim3(bis_pair_grid(n, kMaxEwBlocks)), dim3(kT), 0, ctx->stream, n,
                           (const int *)s->flags, (const double *)(s->sc + s_nrm0), (const double *)w, dst);
        BIS_HIP_CHECK(ctx, hipGetLastError());
    }
    BIS_SYNC_CHECK(ctx);
    s->initialised = true;
    return BIS_OK;
}

// what both *_status calls report; the values and estimates sit at sc + s_val and sc + s_est
bis_status lanczos_status(bis_ctx *ctx, bis_lanczos_core *s, const char *unit, int *products, int *restarts, int *stopped,
                          int *converged, int *reason, int *nconv, int s_val, double *values_host, int s_est, double *est_host,
                          double *hist_host, double *hist_nconv_host, int hist_cap) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, s, std::string(unit) + "_status: null handle");
    int flags[kFlags] = {0};
    if (bis_status st = bis_solver_read_flags(ctx, *s, 0, kFlags, flags)) return st;
    int *const out[6] = {products, stopped, converged, restarts, reason, nconv}; // flags[0..5]
    for (int i = 0; i < 6; ++i)
        if (out[i]) *out[i] = flags[i];
    if (values_host) BIS_HIP_CHECK(ctx, hipMemcpy(values_host, s->sc + s_val, sizeof(double) * s->k, hipMemcpyDeviceToHost));
    if (est_host) BIS_HIP_CHECK(ctx, hipMemcpy(est_host, s->sc + s_est, sizeof(double) * s->k, hipMemcpyDeviceToHost));
    if (hist_cap > 0 && s->initialised) {
        const int cnt = std::min(flags[3], hist_cap);
        if (hist_host && cnt > 0)
            if (bis_status st = bis_solver_copy_hist(ctx, *s, 0, cnt, hist_host)) return st;
        if (hist_nconv_host && cnt > 0)
            if (bis_status st = bis_solver_copy_hist(ctx, *s, 1, cnt, hist_nconv_host)) return st;
    }
    return BIS_OK;
}

} // namespace
