// bis_mprecond.hip -- the preconditioner apply on n x k interleaved blocks (1 <= k <= 8, bis_spmm's layout): the
// dispatcher of bis_precond.hip call for call, over the multi-vector sweeps (bis_sptrsm.hip), the multi-vector iterative
// triangular solve (bis_mitrsv: bis_itrsv.hip's recurrence on bis_spmm) and elementwise kernels with a diagonal shared by
// all columns.  Column j of every result is the single-vector call on column j bit for bit (bis_mitrsv: wherever
// bis_spmm's column j is bis_spmv's, see include/bis_hip.h).  Every kernel here is a no-op once the device schedule it
// was launched from has stopped (ctx->spmv_stop), like the sweeps and the SpMM.
#include "bis_internal.hpp"

#include <algorithm>

namespace {

constexpr int kMpT = 256;
constexpr int kMpMaxBlocks = 16384; // an elementwise pass: the wide grid of bis_blas1.hip's kernels
constexpr int kMpMaxK = 8;

enum { MP_DIV, MP_MUL, MP_COPY, MP_ITRSV };

// r[i,j] = a[i,j] / (1.0 * d[i])           MP_DIV   elemwise_div_vectors, kernels.hpp:151
//          (a[i,j] * 1.0) * d[i]           MP_MUL   elemwise_mult_vectors, kernels.hpp:142
//          a[i,j]                          MP_COPY
//          (a[i,j] - r[i,j]) * d[i]        MP_ITRSV the step's epilogue, r holding T x_k on entry: subtraction and
//                                                   multiplication rounded separately (itrsv_epilogue_kernel)
// r may alias a (same-index access only).
template <int OP>
__global__ __launch_bounds__(kMpT) void mvec_diag_kernel(double *r, const double *a, const double *__restrict__ d, int64_t n, int k,
                                                         const int *stop) {
    if (stop && stop[1]) return;
    const int64_t total = n * k, stride = (int64_t)gridDim.x * kMpT;
    for (int64_t e = (int64_t)blockIdx.x * kMpT + threadIdx.x; e < total; e += stride) {
        const double av = a[e];
        if (OP == MP_COPY) { r[e] = av; continue; }
        const double dv = d[e / k];
        if (OP == MP_DIV) r[e] = av / (1.0 * dv);
        else if (OP == MP_MUL) r[e] = (av * 1.0) * dv;
        else r[e] = __dmul_rn(__dsub_rn(av, r[e]), dv);
    }
}

template <int OP>
bis_status launch_diag(bis_ctx *ctx, double *r, const double *a, const double *d, int64_t n, int k) {
    if (n == 0) return BIS_OK;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n * k + kMpT - 1) / kMpT, kMpMaxBlocks));
    hipLaunchKernelGGL((mvec_diag_kernel<OP>), dim3(grid), dim3(kMpT), 0, ctx->stream, r, a, d, n, k, ctx->spmv_stop);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

} // namespace

extern "C" {

bis_status bis_mvec_div_diag(bis_ctx *ctx, double *R, const double *A, const double *D, int64_t n, int n_rhs) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n >= 0 && n_rhs >= 1 && n_rhs <= kMpMaxK && (n == 0 || (R && A && D)), "bis_mvec_div_diag: bad arguments (1 <= n_rhs <= 8)");
    return launch_diag<MP_DIV>(ctx, R, A, D, n, n_rhs);
}

bis_status bis_mvec_mul_diag(bis_ctx *ctx, double *R, const double *A, const double *D, int64_t n, int n_rhs) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n >= 0 && n_rhs >= 1 && n_rhs <= kMpMaxK && (n == 0 || (R && A && D)), "bis_mvec_mul_diag: bad arguments (1 <= n_rhs <= 8)");
    return launch_diag<MP_MUL>(ctx, R, A, D, n, n_rhs);
}

bis_status bis_mitrsv(bis_ctx *ctx, const bis_mat *T, const double *D_inv, const double *B, double *X, double *WORK, int n_sweeps,
                      int n_rhs) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kMpMaxK, "bis_mitrsv: n_rhs must be between 1 and 8");
    BIS_REQUIRE(ctx, T && n_sweeps >= 0 && T->n_rows == T->n_cols, "bis_mitrsv: bad arguments (a square triangle, n_sweeps >= 0)");
    const int64_t n = T->n_rows;
    if (n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, D_inv && B && X && (WORK || n_sweeps == 0), "bis_mitrsv: null vector");
    BIS_REQUIRE(ctx, X != B && X != WORK && X != D_inv, "bis_mitrsv: X must not alias B, WORK or D_inv");
    BIS_REQUIRE(ctx, n_sweeps == 0 || (WORK != B && WORK != D_inv), "bis_mitrsv: WORK must not alias B or D_inv");
    if (n_rhs == 1) return bis_itrsv(ctx, T, D_inv, B, X, WORK, n_sweeps);
    // X and WORK alternate; x_0 starts where an even number of swaps is left, so that x_{n_sweeps} lands in X
    double *cur = (n_sweeps & 1) ? WORK : X, *nxt = (n_sweeps & 1) ? X : WORK;
    bis_status st = launch_diag<MP_MUL>(ctx, cur, B, D_inv, n, n_rhs); // x_0 = D_inv * b (one rounding)
    for (int s = 0; st == BIS_OK && s < n_sweeps; ++s) {
        st = bis_spmm_launch(ctx, T, cur, nxt, n_rhs);
        if (st == BIS_OK) st = launch_diag<MP_ITRSV>(ctx, nxt, B, D_inv, n, n_rhs);
        std::swap(cur, nxt);
    }
    return st;
}

bis_status bis_mapply_preconditioner(bis_ctx *ctx, int pc, int64_t n, int n_rhs, const bis_mat *L_strict, const bis_mat *U_strict,
                                     const double *A_D, const double *A_D_inv, const double *L_D, const double *U_D, double *OUT,
                                     double *IN, double *TMP, double *WORK, int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    if (pc == BIS_PC_MG) { ctx->err = "bis_mapply_preconditioner: the multigrid preconditioner has no multi-vector form"; return BIS_ERR_UNSUPPORTED; }
    BIS_REQUIRE(ctx, n >= 0 && outer_iters >= 1 && pc >= BIS_PC_NONE && (pc <= BIS_PC_FSAI || pc == BIS_PC_BLOCK_JACOBI),
                "bis_mapply_preconditioner: bad arguments");
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kMpMaxK, "bis_mapply_preconditioner: n_rhs must be between 1 and 8");
    if (pc == BIS_PC_BLOCK_JACOBI) { // the handle whose operand is in L_strict (bis_bj_operand); nothing else is read
        BIS_REQUIRE(ctx, L_strict && L_strict->bj && L_strict->n_rows == n, "bis_mapply_preconditioner: block Jacobi needs the operand of a handle of size n in L_strict");
        if (outer_iters != 1) { ctx->err = "bis_mapply_preconditioner: outer_iters must be 1 on interleaved blocks"; return BIS_ERR_UNSUPPORTED; }
        return bis_bj_mapply(ctx, L_strict->bj, OUT, IN, n_rhs);
    }
    if (pc == BIS_PC_TWO_STAGE_GS || pc == BIS_PC_SYMMETRIC_TWO_STAGE_GS) {
        ctx->err = "bis_mapply_preconditioner: the two-stage Gauss-Seidel types have no multi-vector form";
        return BIS_ERR_UNSUPPORTED;
    }
    if (outer_iters != 1) {
        ctx->err = "bis_mapply_preconditioner: outer_iters must be 1 on interleaved blocks";
        return BIS_ERR_UNSUPPORTED;
    }
    BIS_REQUIRE(ctx, n == 0 || (OUT && IN), "bis_mapply_preconditioner: null OUT or IN");
    const int k = n_rhs;
    switch (pc) {
    case BIS_PC_JACOBI:
        BIS_REQUIRE(ctx, n == 0 || A_D, "bis_mapply_preconditioner: Jacobi needs A_D");
        return launch_diag<MP_DIV>(ctx, OUT, IN, A_D, n, k);                       // kernels.hpp:357
    case BIS_PC_GAUSS_SEIDEL:
        return bis_sptrsm(ctx, L_strict, OUT, A_D, IN, k);                         // :359
    case BIS_PC_BACKWARDS_GAUSS_SEIDEL:
        return bis_bsptrsm(ctx, U_strict, OUT, A_D, IN, k);                        // :361
    case BIS_PC_SYMMETRIC_GAUSS_SEIDEL: {
        BIS_REQUIRE(ctx, n == 0 || (TMP && A_D), "bis_mapply_preconditioner: SGS needs TMP and A_D");
        bis_status st = bis_sptrsm(ctx, L_strict, TMP, A_D, IN, k);                // :365
        if (st == BIS_OK) st = launch_diag<MP_MUL>(ctx, TMP, TMP, A_D, n, k);      // :369
        if (st == BIS_OK) st = bis_bsptrsm(ctx, U_strict, OUT, A_D, TMP, k);       // :373
        return st;
    }
    case BIS_PC_ILU0: {
        BIS_REQUIRE(ctx, n == 0 || TMP, "bis_mapply_preconditioner: ILU0 needs TMP");
        bis_status st = bis_sptrsm(ctx, L_strict, TMP, L_D, IN, k);                // :390
        if (st == BIS_OK) st = bis_bsptrsm(ctx, U_strict, OUT, U_D, TMP, k);       // :394
        return st;
    }
    case BIS_PC_ILU0_ITER: { // both solves as bis_mitrsv; A_D_inv carries 1 / U_D (bis_apply_preconditioner)
        BIS_REQUIRE(ctx, L_strict && U_strict && inner_iters >= 0 && (n == 0 || (TMP && WORK && TMP != WORK && TMP != OUT &&
                         TMP != IN && WORK != OUT && WORK != IN)),
                    "bis_mapply_preconditioner: ILU0_ITER needs both factors, inner_iters >= 0, and TMP, WORK distinct from each other, OUT and IN");
        bis_status st = bis_mitrsv(ctx, L_strict, L_D, IN, TMP, WORK, inner_iters, k);
        if (st == BIS_OK) st = bis_mitrsv(ctx, U_strict, A_D_inv, TMP, OUT, WORK, inner_iters, k);
        return st;
    }
    case BIS_PC_FSAI: { // OUT = Gt (G IN), two bis_spmm: G in L_strict, Gt in U_strict (bis_mat_fsai)
        BIS_REQUIRE(ctx, L_strict && U_strict && (n == 0 || (TMP && TMP != OUT && TMP != IN)),
                    "bis_mapply_preconditioner: FSAI needs both factors and TMP distinct from OUT and IN");
        bis_status st = bis_spmm_launch(ctx, L_strict, IN, TMP, k);
        if (st == BIS_OK) st = bis_spmm_launch(ctx, U_strict, TMP, OUT, k);
        return st;
    }
    default:
        if (OUT == IN) return BIS_OK;
        return launch_diag<MP_COPY>(ctx, OUT, IN, nullptr, n, k);                  // :398
    }
}

} // extern "C"
