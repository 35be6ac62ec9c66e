// bis_gmres_state.hpp -- the Givens / least-squares state of one GMRES column and its bookkeeping, shared by the lock-step
// solver (bis_mgmres.hip: one state per column) and the flexible one (bis_fgmres.hip: one column).
#pragma once

#include "bis_internal.hpp"

#include <cfloat>
#include <cmath>

constexpr int kMaxRestart = 64; // bis_multi_axpy's limit

// per-column state, in doubles: h (m + 1: the current Hessenberg column, then rotated in place), cs (m), sn (m), g (m + 1),
// y (m), the y of *_solution (m), 1 / norm for the scale, beta, threshold, the rotated triangle (m x m, entry (r, c) at
// c m + r)
struct gmres_layout {
    int m;
    __host__ __device__ int h() const { return 0; }
    __host__ __device__ int cs() const { return m + 1; }
    __host__ __device__ int sn() const { return 2 * m + 1; }
    __host__ __device__ int g() const { return 3 * m + 1; }
    __host__ __device__ int y() const { return 4 * m + 2; }
    __host__ __device__ int ysol() const { return 5 * m + 2; }
    __host__ __device__ int inv() const { return 6 * m + 2; }
    __host__ __device__ int beta() const { return 6 * m + 3; }
    __host__ __device__ int stop() const { return 6 * m + 4; }
    __host__ __device__ int rt() const { return 6 * m + 5; }
    __host__ __device__ int size() const { return 6 * m + 5 + m * m; }
};

// a column's flag words: fc = iterations, stopped, converged, the iteration of the stop (bis_mcg's four); xc = these
enum { X_PENDING = 0 /* x awaits its combine */, X_STEPS /* of that combine */, X_NHIST /* history entries written */,
       X_POS /* steps done in the current cycle */ };

// y_r = (g_r - sum_{c > r} R_rc y_c) / R_rr for r = steps - 1 .. 0 (get_explicit_x, gmres.hpp: y[steps] counts as 0)
static __device__ void gmres_backsub(const gmres_layout L, const double *s, int steps, double *y) {
    const double *rt = s + L.rt(), *g = s + L.g();
    for (int r = steps - 1; r >= 0; --r) {
        double sum = 0.0;
        for (int c = r + 1; c < steps; ++c) sum = fma(rt[c * L.m + r], y[c], sum);
        y[r] = (g[r] - sum) / rt[r * L.m + r];
    }
}

// one column's bookkeeping after the sum-of-squares pass of position n (least_squares, update_g, check_restart)
static __device__ void gmres_book(const gmres_layout L, double ss, int n, double *s, int *fc, int *xc, double *hist, int hist_cap) {
    double *h = s + L.h(), *cs = s + L.cs(), *sn = s + L.sn(), *g = s + L.g(), *rt = s + L.rt();
    const int m = L.m;
    const double hn1 = sqrt(ss);
    s[L.inv()] = 1.0 / hn1;
    h[n + 1] = hn1;
    for (int i = 0; i < n; ++i) { // the stored rotations on the new column
        const double a = h[i], b = h[i + 1];
        h[i] = cs[i] * a + sn[i] * b;
        h[i + 1] = cs[i] * b - sn[i] * a;
    }
    const double a = h[n], b = h[n + 1];
    const double den = sqrt(a * a + b * b);
    const double c_n = a / den, s_n = b / den;
    cs[n] = c_n;
    sn[n] = s_n;
    for (int i = 0; i < n; ++i) rt[n * m + i] = h[i];
    rt[n * m + n] = c_n * a + s_n * b;
    const double gn = g[n];
    g[n + 1] = -s_n * gn;
    g[n] = c_n * gn;
    const double est = fabs(g[n + 1]);
    const int it = fc[0] + 1;
    fc[0] = it;
    const int nh = xc[X_NHIST];
    if (nh < hist_cap) hist[nh] = est;
    xc[X_NHIST] = nh + 1;
    xc[X_POS] = n + 1;
    const bool conv = est < s[L.stop()];
    const bool diverged = est > DBL_MAX || est != est;
    if (conv || diverged) { fc[1] = 1; fc[2] = conv ? 1 : 0; fc[3] = it; }
    if (conv || diverged || n + 1 == m) {
        gmres_backsub(L, s, n + 1, s + L.y());
        xc[X_STEPS] = n + 1;
        xc[X_PENDING] = 1;
    }
}
