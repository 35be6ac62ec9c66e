// bis_itrsv.hip -- iterative triangular solve: x ~ (D + T)^-1 b by a fixed number of Jacobi-Richardson steps on the
// strict triangle T, and the ILU(0) apply built on it (BIS_PC_ILU0_ITER in bis_apply_preconditioner, bis_sptrsv.hip).
//
//   x_0 = D_inv * b;   x_{k+1} = (b - T x_k) * D_inv,   k = 0 .. n_sweeps - 1
//
// T is nilpotent, so the iteration is exact after as many steps as T has dependency levels; a preconditioner stops far
// earlier.  What it buys: a step has no dependency between rows -- it is one SpMV-shaped pass at the SpMV's rate, where
// the exact sweeps (bis_sptrsv.hip, bis_trsv_chain.hip, bis_trsv_tiled.hip) pay a dependent latency per level or chain row.
//
// Two paths per step, chosen by the form the SpMV of T resolves to (bis_spmv.hip, spmv_resolve):
//   * CRS-value row-block kernel: the step is that kernel's epilogue (MODE 3) -- T x_k is never written and read back;
//   * every other form (dictionary forms, win8 / win4, column slabs, x-window, wave-per-row): the SpMV runs as it is into the
//     buffer x_{k+1} will occupy, and itrsv_epilogue_kernel finishes the step there in place: 32 B per row read, 8 written.
// The row sum is bis_spmv's in both, the subtraction and the multiplication are rounded separately in both: the paths
// agree bit for bit with each other and with bis_spmv followed by (b - y) * D_inv.
#include "bis_internal.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int kItThreads = 256;
constexpr int kItMaxBlocks = 16384; // an elementwise pass: the wide grid of bis_blas1.hip's kernels

typedef double it_v2d __attribute__((ext_vector_type(2)));

// x[i] = (b[i] - x[i]) * D_inv[i] in place, x holding T x_k on entry.  All three inputs are touched once: non-temporal
// loads; the store stays plain -- the next step's SpMV gathers from what this one wrote.
template <bool VEC>
__global__ __launch_bounds__(kItThreads) void itrsv_epilogue_kernel(double *x, const double *b, const double *D_inv, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kItThreads;
    int64_t i = (int64_t)blockIdx.x * kItThreads + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        it_v2d *x2 = reinterpret_cast<it_v2d *>(x);
        const it_v2d *b2 = reinterpret_cast<const it_v2d *>(b), *d2 = reinterpret_cast<const it_v2d *>(D_inv);
        for (; i < n2; i += stride) {
            const it_v2d s = __builtin_nontemporal_load(x2 + i), bv = __builtin_nontemporal_load(b2 + i),
                         dv = __builtin_nontemporal_load(d2 + i);
            it_v2d r;
            r.x = __dmul_rn(__dsub_rn(bv.x, s.x), dv.x);
            r.y = __dmul_rn(__dsub_rn(bv.y, s.y), dv.y);
            x2[i] = r;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = __dmul_rn(__dsub_rn(b[n - 1], x[n - 1]), D_inv[n - 1]);
    } else {
        for (; i < n; i += stride)
            x[i] = __dmul_rn(__dsub_rn(__builtin_nontemporal_load(b + i), __builtin_nontemporal_load(x + i)),
                             __builtin_nontemporal_load(D_inv + i));
    }
}

bis_status launch_epilogue(bis_ctx *ctx, double *x, const double *b, const double *D_inv, int64_t n) {
    const bool vec = aligned16(x) && aligned16(b) && aligned16(D_inv) && n >= 2;
    const int64_t items = vec ? n >> 1 : n;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + kItThreads - 1) / kItThreads, kItMaxBlocks));
    if (vec) hipLaunchKernelGGL((itrsv_epilogue_kernel<true>), dim3(grid), dim3(kItThreads), 0, ctx->stream, x, b, D_inv, n);
    else hipLaunchKernelGGL((itrsv_epilogue_kernel<false>), dim3(grid), dim3(kItThreads), 0, ctx->stream, x, b, D_inv, n);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

// "itrsv spmv+epilogue form=F", F the public SpMV form number (bis_mat_spmv_stream_info): static strings, built once
const char *epilogue_name(int form) {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (int f = 0; f <= 8; ++f) v.push_back("itrsv spmv+epilogue form=" + std::to_string(f));
        return v;
    }();
    return names[(size_t)std::max(0, std::min(form, 8))].c_str();
}

} // namespace

extern "C" {

const char *bis_itrsv_kernel(const bis_mat *T) { return T ? T->itrsv_kernel : ""; }

bis_status bis_itrsv(bis_ctx *ctx, const bis_mat *T, const double *D_inv, const double *b, double *x, double *work,
                     int n_sweeps) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, T && n_sweeps >= 0 && T->n_rows == T->n_cols, "bis_itrsv: bad arguments (a square triangle, n_sweeps >= 0)");
    const int64_t n = T->n_rows;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, D_inv && b && x && (work || n_sweeps == 0), "bis_itrsv: null vector");
    BIS_REQUIRE(ctx, x != b && x != work && x != D_inv, "bis_itrsv: x must not alias b, work or D_inv");
    BIS_REQUIRE(ctx, n_sweeps == 0 || (work != b && work != D_inv), "bis_itrsv: work must not alias b or D_inv");
    // x and work alternate; x_0 starts where an even number of swaps is left, so that x_{n_sweeps} lands in x
    double *cur = (n_sweeps & 1) ? work : x, *nxt = (n_sweeps & 1) ? x : work;
    bis_status st = bis_elemwise_mult_vectors(ctx, cur, D_inv, b, n, 1.0); // x_0 = D_inv * b (one rounding)
    for (int k = 0; st == BIS_OK && k < n_sweeps; ++k) {
        int form = -1;
        st = bis_spmv_itrsv_step(ctx, T, cur, nxt, b, D_inv, &form);
        if (st == BIS_OK && form >= 0) st = launch_epilogue(ctx, nxt, b, D_inv, n);
        if (st == BIS_OK) const_cast<bis_mat *>(T)->itrsv_kernel = form < 0 ? "itrsv_fused_rowblock" : epilogue_name(form);
        std::swap(cur, nxt);
    }
    return st;
}

} // extern "C"
