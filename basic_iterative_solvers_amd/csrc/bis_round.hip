// bis_round.hip -- bis_mat_round_f32: the values of a matrix rounded to binary32, in place in the fp64 CRS array.  gfx950 only.
//
// A preconditioner's factors (FSAI's G and Gt, the ILU(0) triangles of -p ilu0it) are applied by SpMV and are bound by the
// bytes of their values; the outer Krylov method stays in fp64 and does not need 53 bits of them.  The rounding is the one
// explicit, lossy step: every value becomes (double)(float)v -- IEEE round to nearest even, subnormals kept, -0.0 kept,
// NaN / Inf unchanged.  Afterwards the matrix is flagged f32_exact and its SpMV may stream 4-byte values (form 8, "win4",
// bis_spmv_win8.hip), which on such values is a LOSSLESS re-encoding like every other form: bit-identical y.
// Two passes.  The census counts the values that are finite in fp64 and not after the rounding (|v| >= 2^128 - 2^103) and
// finds max |v32 - v| / |v| over v != 0: per-workgroup partials in index order, then one workgroup -- no floating-point
// atomics, the same result on every run (as the reductions of bis_blas1.hip).  Only a census without overflow is followed by
// the rounding pass, so a refused matrix is untouched.
#include "bis_internal.hpp"

#include <algorithm>

namespace {

constexpr int kRoundBlocks = 2048;

__device__ __forceinline__ double round_f32(double v) { return (double)(float)v; } // v_cvt_f32_f64: RNE, fp32 denormals kept (the HIP default)

// partial[b] = max relative change over the block's grid-stride share, over[b] = its count of overflowing values
__global__ __launch_bounds__(256) void round_census_kernel(const double *__restrict__ val, int64_t nnz, double *__restrict__ partial,
                                                           unsigned long long *__restrict__ over) {
    __shared__ double s_max[4];
    __shared__ unsigned long long s_cnt[4];
    double m = 0.0;
    unsigned long long c = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) {
        const double v = val[k], r = round_f32(v);
        const bool finite = fabs(v) <= 1.7976931348623157e308; // (false for NaN)
        if (finite && !(fabs(r) <= 1.7976931348623157e308)) ++c;
        else if (finite && v != 0.0) m = fmax(m, fabs(r - v) / fabs(v));
    }
    for (int o = 32; o > 0; o >>= 1) { // (max and integer sums: any order gives the same bits)
        m = fmax(m, __shfl_xor(m, o));
        c += __shfl_xor(c, o);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_max[w] = m; s_cnt[w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
        over[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

// one workgroup: result[0] = max of the partials, count[0] = sum of the counts
__global__ __launch_bounds__(256) void round_finish_kernel(const double *__restrict__ partial, const unsigned long long *__restrict__ over,
                                                           int n, double *__restrict__ result, unsigned long long *__restrict__ count) {
    __shared__ double s_max[4];
    __shared__ unsigned long long s_cnt[4];
    double m = 0.0;
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < n; i += 256) { m = fmax(m, partial[i]); c += over[i]; }
    for (int o = 32; o > 0; o >>= 1) {
        m = fmax(m, __shfl_xor(m, o));
        c += __shfl_xor(c, o);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_max[w] = m; s_cnt[w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        result[0] = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
        count[0] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

__global__ __launch_bounds__(256) void round_apply_kernel(double *__restrict__ val, int64_t nnz) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) val[k] = round_f32(val[k]);
}

} // namespace

extern "C" bis_status bis_mat_round_f32(bis_ctx *ctx, bis_mat *A, double *max_rel_change) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && !A->view, "bis_mat_round_f32: bad arguments (an owning matrix, not a row-range view)");
    if (max_rel_change) *max_rel_change = 0.0;
    if (A->nnz == 0) return BIS_OK;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((A->nnz + 255) / 256, kRoundBlocks));
    // the values start at the matrix' own first entry (an owning matrix: row_ptr[0] = 0)
    double *partial = nullptr;
    unsigned long long *over = nullptr;
    auto cleanup = [&](bis_status st) { hipFree(partial); hipFree(over); return st; };
    BIS_HIP_CHECK(ctx, hipMalloc(&partial, sizeof(double) * (size_t)(grid + 1)));
    if (hipMalloc(&over, sizeof(unsigned long long) * (size_t)(grid + 1)) != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = "bis_mat_round_f32: out of device memory";
        return cleanup(BIS_ERR_HIP);
    }
    hipLaunchKernelGGL(round_census_kernel, dim3(grid), dim3(256), 0, ctx->stream, A->val, A->nnz, partial, over);
    hipLaunchKernelGGL(round_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, partial, over, grid, partial + grid, over + grid);
    double h_max = 0.0;
    unsigned long long h_over = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&h_max, partial + grid, sizeof h_max, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_over, over + grid, sizeof h_over, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); // (also: sweeps in flight still read the plans dropped below)
    if (e != hipSuccess) { ctx->err = std::string("bis_mat_round_f32: ") + hipGetErrorString(e); return cleanup(BIS_ERR_HIP); }
    if (h_over != 0) {
        char msg[128];
        snprintf(msg, sizeof msg, "bis_mat_round_f32: %llu value(s) finite in fp64 overflow in fp32; the matrix is unchanged", h_over);
        ctx->err = msg;
        return cleanup(BIS_ERR_UNSUPPORTED);
    }
    bis_mat_values_changed(A); // the values change in place: dictionary, code streams (win8, slabs), sweep plans go, as in bis_mat_scale_sym
    hipLaunchKernelGGL(round_apply_kernel, dim3(grid), dim3(256), 0, ctx->stream, A->val, A->nnz);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("bis_mat_round_f32: ") + hipGetErrorString(e); return cleanup(BIS_ERR_HIP); }
    A->f32_exact = true;
    if (max_rel_change) *max_rel_change = h_max;
    return cleanup(bis_fault_check(ctx));
}
