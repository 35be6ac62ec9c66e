// bis_fsai.hip -- factorized sparse approximate inverse (FSAI, Kolotilina-Yeremin) on the pattern of tril(A); not in the
// reference.  G is lower triangular with G A G^T ~ I on that pattern, M^-1 = G^T G; the apply is two SpMVs (bis_precond.hip).
//
// Definition (include/bis_hip.h): for row i, J = the columns <= i of row i (ascending, m <= 64 of them, the last is i),
// S = A[J,J] read from the lower triangle only (S[p,q], q <= p, from row J[p], column J[q]; absent = 0), S = C C^T, and row i
// of G is g = C^-T e_m.  A pivot <= 0 or not finite: g = e_i / sqrt(|a_ii|), counted.
//
// The rows are independent: ONE WAVE PER ROW, no levels and no flags.  The packed lower triangle of S lives in LDS
// (M(M+1)/2 doubles per wave, M = 16, 32 or 64 by the longest lower row of the matrix: 0.5 / 2.1 / 16.6 KB per wave, four
// waves per workgroup); one lane per (p,q) pair gathers it by binary search in row J[p] of a column-sorted copy of A
// (bis_ilu0.hip's sort); the Cholesky factorisation runs column by column with the lanes over the rows of the column
// (left-looking: lane r forms S[r,j] - sum_k C[r,k] C[j,k] in ascending k); the back substitution runs from the last row up,
// lane p accumulating sum_r C[r,p] g[r] in descending r.  Every sum has one fixed order: the bits do not depend on the
// schedule, on the grid, or on the order of the entries inside A's rows.
// Gt = G^T is gathered, not scattered: entry (i,j) of A's upper triangle looks (j,i) up in G by binary search, so there are
// no atomics; a miss means the pattern is not structurally symmetric.
#include "bis_internal.hpp"

#include <algorithm>

namespace {

constexpr int kFsaiT = 256;
constexpr int kFsaiMaxRow = 64;
// aux words (device, unsigned long long): totals of the two scans, then the checks' results
enum { FA_TOT_L, FA_TOT_U, FA_STATUS, FA_MAX_LOWER, FA_FALLBACK, FA_MISS, FA_COUNT };
enum { FS_ZERO_DIAG = 1, FS_DUP = 2 };

__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// per row of the sorted copy: entries left of and on the diagonal (cl), on and right of it (cu); their sums per block of
// kFsaiT rows; the checks: a diagonal entry that is missing or 0, a repeated column, the longest lower row
template <typename RP>
__global__ __launch_bounds__(kFsaiT) void fsai_count_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ wcol,
                                                            const double *__restrict__ wval, const int64_t *__restrict__ dpos,
                                                            const int64_t *__restrict__ ustart, int64_t n, int64_t *blk_l, int64_t *blk_u,
                                                            unsigned long long *aux) {
    __shared__ double lds[kFsaiT / 64];
    const int64_t i = (int64_t)blockIdx.x * kFsaiT + threadIdx.x;
    int64_t cl = 0, cu = 0;
    if (i < n) {
        const int64_t s = rp[i], e = rp[i + 1], d = dpos[i], u = ustart[i];
        cl = u - s;
        cu = e - u + (d >= 0 ? 1 : 0);
        unsigned status = 0;
        if (d < 0 || wval[d] == 0.0) status |= FS_ZERO_DIAG;
        for (int64_t p = s + 1; p < e; ++p)
            if (wcol[p] == wcol[p - 1]) status |= FS_DUP;
        if (status) atomicOr(&aux[FA_STATUS], (unsigned long long)status);
        atomicMax(&aux[FA_MAX_LOWER], (unsigned long long)cl);
    }
    // counts fit a double exactly (< 2^53)
    const double sl = block_sum<kFsaiT>((double)cl, lds);
    __syncthreads();
    const double su = block_sum<kFsaiT>((double)cu, lds);
    if (threadIdx.x == 0) { blk_l[blockIdx.x] = (int64_t)sl; blk_u[blockIdx.x] = (int64_t)su; }
}

// exclusive scan of the block sums, single workgroup; totals to aux[FA_TOT_L], aux[FA_TOT_U]
__global__ __launch_bounds__(256) void fsai_scan_kernel(int64_t *blk_l, int64_t *blk_u, int n_blk, unsigned long long *aux) {
    __shared__ int64_t sl[256], su[256];
    int64_t run_l = 0, run_u = 0;
    for (int base = 0; base < n_blk; base += 256) {
        const int i = base + threadIdx.x;
        const int64_t vl = i < n_blk ? blk_l[i] : 0, vu = i < n_blk ? blk_u[i] : 0;
        sl[threadIdx.x] = vl;
        su[threadIdx.x] = vu;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            int64_t al = 0, au = 0;
            if ((int)threadIdx.x >= off) { al = sl[threadIdx.x - off]; au = su[threadIdx.x - off]; }
            __syncthreads();
            sl[threadIdx.x] += al;
            su[threadIdx.x] += au;
            __syncthreads();
        }
        if (i < n_blk) { blk_l[i] = run_l + sl[threadIdx.x] - vl; blk_u[i] = run_u + su[threadIdx.x] - vu; }
        run_l += sl[255];
        run_u += su[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) { aux[FA_TOT_L] = (unsigned long long)run_l; aux[FA_TOT_U] = (unsigned long long)run_u; }
}

// the row pointers of G and Gt from the scanned block sums (every row has its diagonal entry here: the checks passed)
template <typename RP>
__global__ __launch_bounds__(kFsaiT) void fsai_rowptr_kernel(const RP *__restrict__ rp, const int64_t *__restrict__ ustart, int64_t n,
                                                             const int64_t *__restrict__ blk_l, const int64_t *__restrict__ blk_u, RP *rpG,
                                                             RP *rpGt) {
    __shared__ int64_t sl[kFsaiT], su[kFsaiT];
    const int64_t i = (int64_t)blockIdx.x * kFsaiT + threadIdx.x;
    int64_t cl = 0, cu = 0;
    if (i < n) {
        const int64_t u = ustart[i];
        cl = u - (int64_t)rp[i];
        cu = (int64_t)rp[i + 1] - u + 1;
    }
    sl[threadIdx.x] = cl;
    su[threadIdx.x] = cu;
    __syncthreads();
    for (int off = 1; off < kFsaiT; off <<= 1) {
        int64_t al = 0, au = 0;
        if ((int)threadIdx.x >= off) { al = sl[threadIdx.x - off]; au = su[threadIdx.x - off]; }
        __syncthreads();
        sl[threadIdx.x] += al;
        su[threadIdx.x] += au;
        __syncthreads();
    }
    if (i < n) {
        const int64_t pl = blk_l[blockIdx.x] + sl[threadIdx.x] - cl, pu = blk_u[blockIdx.x] + su[threadIdx.x] - cu;
        rpG[i] = (RP)pl;
        rpGt[i] = (RP)pu;
        if (i == n - 1) { rpG[n] = (RP)(pl + cl); rpGt[n] = (RP)(pu + cu); }
    }
}

// row p of the packed lower triangle that holds pair t: the largest p with p (p + 1) / 2 <= t (t < 2080)
__device__ __forceinline__ int tri_row(int t) {
    int p = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((p + 1) * (p + 2) / 2 <= t) ++p;
    while (p * (p + 1) / 2 > t) --p;
    return p;
}

// One wave per row (see the head of the file).  Every row has 1 <= m <= M entries up to its diagonal, the last of them
// the diagonal: the host has checked it.
template <typename RP, int M>
__global__ __launch_bounds__(kFsaiT) void fsai_rows_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ wcol,
                                                           const double *__restrict__ wval, const int64_t *__restrict__ ustart, int64_t n,
                                                           const RP *__restrict__ rpG, int32_t *__restrict__ colG, double *__restrict__ valG,
                                                           unsigned long long *aux) {
    constexpr int kTri = M * (M + 1) / 2;
    __shared__ double S_all[kFsaiT / 64][kTri];
    __shared__ int32_t J_all[kFsaiT / 64][M];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *S = S_all[wave];
    int32_t *J = J_all[wave];
    for (int64_t i = (int64_t)blockIdx.x * (kFsaiT / 64) + wave; i < n; i += (int64_t)gridDim.x * (kFsaiT / 64)) {
        const int64_t s = rp[i];
        const int m = min((int)(ustart[i] - s), M);
        if (lane < m) J[lane] = wcol[s + lane];
        const double a_ii = wval[s + m - 1];
        wave_lds_sync();
        // gather: S[p,q] = A[J[p], J[q]] from the lower part of row J[p]
        const int n_pairs = m * (m + 1) / 2;
        for (int t = lane; t < n_pairs; t += 64) {
            const int p = tri_row(t), q = t - p * (p + 1) / 2;
            const int r = J[p], c = J[q];
            int64_t lo = rp[r];
            const int64_t end = ustart[r];
            int64_t hi = end;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (wcol[mid] < c) lo = mid + 1; else hi = mid;
            }
            S[t] = (lo < end && wcol[lo] == c) ? wval[lo] : 0.0;
        }
        wave_lds_sync();
        // S = C C^T in place, column by column; lane r owns row r
        bool bad = false;
        const double *Sr = S + lane * (lane + 1) / 2;
        for (int j = 0; j < m; ++j) {
            const bool act = lane >= j && lane < m;
            double acc = 0.0;
            if (act) {
                const double *Sj = S + j * (j + 1) / 2;
                acc = Sr[j];
                for (int k = 0; k < j; ++k) acc = fma(-Sr[k], Sj[k], acc);
            }
            const double d = __shfl(acc, j, 64); // the pivot's square
            if (!(d > 0.0) || !isfinite(d)) { bad = true; break; } // (wave-uniform)
            const double c_jj = sqrt(d);
            if (act) S[lane * (lane + 1) / 2 + j] = lane == j ? c_jj : acc / c_jj;
            wave_lds_sync();
        }
        // C^T g = e_m from the last row up; lane p holds sum_{r > p} C[r,p] g[r]
        double g = 0.0;
        if (!bad) {
            double acc = 0.0;
            for (int r = m - 1; r >= 0; --r) {
                const double *Crow = S + r * (r + 1) / 2;
                const double mine = ((r == m - 1 ? 1.0 : 0.0) - acc) / Crow[r]; // the value of lane r counts
                const double g_r = __shfl(mine, r, 64);
                if (lane == r) g = g_r;
                if (lane < r) acc = fma(Crow[lane], g_r, acc);
            }
        } else {
            if (lane == m - 1) g = 1.0 / sqrt(fabs(a_ii));
            if (lane == 0) atomicAdd(&aux[FA_FALLBACK], 1ull);
        }
        if (lane < m) {
            const int64_t o = (int64_t)rpG[i] + lane;
            colG[o] = J[lane];
            valG[o] = g;
        }
        wave_lds_sync(); // J and S are rewritten for the next row
    }
}

// Gt[i,j] = G[j,i] for every entry (i, j >= i) of the sorted copy: a wave per row, a lane per entry, binary search in row j of G
template <typename RP>
__global__ __launch_bounds__(kFsaiT) void fsai_transpose_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ wcol,
                                                                const int64_t *__restrict__ ustart, int64_t n, const RP *__restrict__ rpG,
                                                                const int32_t *__restrict__ colG, const double *__restrict__ valG,
                                                                const RP *__restrict__ rpGt, int32_t *__restrict__ colGt,
                                                                double *__restrict__ valGt, unsigned long long *aux) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (kFsaiT / 64) + wave; i < n; i += (int64_t)gridDim.x * (kFsaiT / 64)) {
        const int64_t a = ustart[i] - 1, e = rp[i + 1]; // from the diagonal entry on
        const int64_t o = (int64_t)rpGt[i] - a;
        for (int64_t k = a + lane; k < e; k += 64) {
            const int j = wcol[k];
            int64_t lo = rpG[j];
            const int64_t end = rpG[j + 1];
            int64_t hi = end;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)colG[mid] < i) lo = mid + 1; else hi = mid;
            }
            const bool hit = lo < end && (int64_t)colG[lo] == i;
            if (!hit) atomicOr(&aux[FA_MISS], 1ull);
            colGt[o + k] = j;
            valGt[o + k] = hit ? valG[lo] : 0.0;
        }
    }
}

const char *fsai_kernel_name(int M, bool rp64) {
    switch (M) {
    case 16: return rp64 ? "fsai_rows_kernel M=16 RP=64" : "fsai_rows_kernel M=16 RP=32";
    case 32: return rp64 ? "fsai_rows_kernel M=32 RP=64" : "fsai_rows_kernel M=32 RP=32";
    default: return rp64 ? "fsai_rows_kernel M=64 RP=64" : "fsai_rows_kernel M=64 RP=32";
    }
}

template <typename RP>
bis_status fsai_t(bis_ctx *ctx, const bis_mat *A, bis_mat **G_out, bis_mat **Gt_out, int64_t *n_fallback) {
    const int64_t n = A->n_rows;
    const int n_blk = (int)((n + kFsaiT - 1) / kFsaiT);
    bis_mat *W = nullptr, *G = nullptr, *Gt = nullptr;
    int64_t *dpos = nullptr, *ustart = nullptr, *blk = nullptr;
    auto cleanup = [&](bis_status rc) {
        hipFree(dpos);
        hipFree(ustart);
        hipFree(blk);
        if (W) bis_mat_destroy(ctx, W);
        if (rc != BIS_OK) {
            if (G) bis_mat_destroy(ctx, G);
            if (Gt) bis_mat_destroy(ctx, Gt);
        }
        return rc;
    };
    auto hip_fail = [&](hipError_t e) {
        ctx->err = std::string("bis_mat_fsai: ") + hipGetErrorString(e);
        return cleanup(BIS_ERR_HIP);
    };
    bis_status st = bis_mat_sorted_copy(ctx, A, &W, &dpos, &ustart);
    if (st != BIS_OK) return st;
    hipError_t e = hipMalloc(&blk, sizeof(int64_t) * (size_t)(2 * n_blk + FA_COUNT));
    if (e != hipSuccess) return hip_fail(e);
    int64_t *blk_l = blk, *blk_u = blk + n_blk;
    unsigned long long *aux = (unsigned long long *)(blk + 2 * n_blk);
    e = hipMemsetAsync(aux, 0, sizeof(unsigned long long) * FA_COUNT, ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    const RP *rp = (const RP *)W->row_ptr;
    if (n > 0) {
        hipLaunchKernelGGL(fsai_count_kernel<RP>, dim3(n_blk), dim3(kFsaiT), 0, ctx->stream, rp, W->col, W->val, dpos, ustart, n, blk_l,
                           blk_u, aux);
        hipLaunchKernelGGL(fsai_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, blk_l, blk_u, n_blk, aux);
    }
    unsigned long long h_aux[FA_COUNT] = {0};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_aux, aux, sizeof h_aux, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    if (h_aux[FA_STATUS] & FS_ZERO_DIAG) {
        ctx->err = "bis_mat_fsai: a row without a diagonal entry, or with a zero on the diagonal";
        return cleanup(BIS_ERR_ZERO_DIAG);
    }
    if (h_aux[FA_MAX_LOWER] > (unsigned long long)kFsaiMaxRow) {
        ctx->err = "bis_mat_fsai: a row with more than 64 entries up to its diagonal";
        return cleanup(BIS_ERR_UNSUPPORTED);
    }
    if (h_aux[FA_STATUS] & FS_DUP) {
        ctx->err = "bis_mat_fsai: a column repeated inside a row";
        return cleanup(BIS_ERR_UNSUPPORTED);
    }
    if (h_aux[FA_TOT_L] != h_aux[FA_TOT_U]) {
        ctx->err = "bis_mat_fsai: the pattern is not structurally symmetric";
        return cleanup(BIS_ERR_UNSUPPORTED);
    }
    st = bis_mat_alloc(ctx, n, n, (int64_t)h_aux[FA_TOT_L], A->rp64, &G);
    if (st == BIS_OK) st = bis_mat_alloc(ctx, n, n, (int64_t)h_aux[FA_TOT_U], A->rp64, &Gt);
    if (st != BIS_OK) return cleanup(st);
    const int max_lower = (int)h_aux[FA_MAX_LOWER];
    const int M = max_lower <= 16 ? 16 : max_lower <= 32 ? 32 : 64;
    if (n > 0) {
        RP *rpG = (RP *)G->row_ptr, *rpGt = (RP *)Gt->row_ptr;
        hipLaunchKernelGGL(fsai_rowptr_kernel<RP>, dim3(n_blk), dim3(kFsaiT), 0, ctx->stream, rp, ustart, n, blk_l, blk_u, rpG, rpGt);
        // a grid-stride over the rows: n / 4 workgroups of any n stay below HIP's 2^32 threads per launch
        const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, 1 << 22));
#define BIS_FSAI_ROWS(MM)                                                                                                          \
    hipLaunchKernelGGL((fsai_rows_kernel<RP, MM>), grid, dim3(kFsaiT), 0, ctx->stream, rp, W->col, W->val, ustart, n, rpG, G->col, \
                       G->val, aux)
        if (M == 16) BIS_FSAI_ROWS(16);
        else if (M == 32) BIS_FSAI_ROWS(32);
        else BIS_FSAI_ROWS(64);
#undef BIS_FSAI_ROWS
        hipLaunchKernelGGL(fsai_transpose_kernel<RP>, grid, dim3(kFsaiT), 0, ctx->stream, rp, W->col, ustart, n, rpG, G->col, G->val, rpGt,
                           Gt->col, Gt->val, aux);
        e = hipGetLastError();
    } else {
        e = hipMemsetAsync(G->row_ptr, 0, sizeof(RP), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(Gt->row_ptr, 0, sizeof(RP), ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_aux, aux, sizeof h_aux, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    if (h_aux[FA_MISS]) {
        ctx->err = "bis_mat_fsai: the pattern is not structurally symmetric";
        return cleanup(BIS_ERR_UNSUPPORTED);
    }
    st = bis_mat_finalize(ctx, G);
    if (st == BIS_OK) st = bis_mat_finalize(ctx, Gt);
    if (st != BIS_OK) return cleanup(st);
    if (n > 0) G->fsai_kernel = fsai_kernel_name(M, A->rp64);
    if (n_fallback) *n_fallback = (int64_t)h_aux[FA_FALLBACK];
    *G_out = G;
    *Gt_out = Gt;
    return cleanup(BIS_OK);
}

} // namespace

extern "C" {

const char *bis_mat_fsai_kernel(const bis_mat *G) { return G ? G->fsai_kernel : ""; }

bis_status bis_mat_fsai(bis_ctx *ctx, const bis_mat *A, bis_mat **G, bis_mat **Gt, int64_t *n_fallback_rows) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && G && Gt, "bis_mat_fsai: bad arguments");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mat_fsai: square matrix required");
    BIS_REQUIRE(ctx, !A->view, "bis_mat_fsai: a row-range view has no diagonal block of its own");
    return A->rp64 ? fsai_t<int64_t>(ctx, A, G, Gt, n_fallback_rows) : fsai_t<int32_t>(ctx, A, G, Gt, n_fallback_rows);
}

} // extern "C"
