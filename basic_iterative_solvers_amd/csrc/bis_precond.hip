// bis_precond.hip -- the preconditioner dispatcher (reference kernels.hpp:312-414) over the library's own kernels: the
// triangular sweeps (bis_sptrsv.hip), the iterative triangular solves (bis_itrsv.hip), SpMV (the FSAI factors of
// bis_fsai.hip), the multigrid cycle (bis_mg.hip) and the vector kernels.
#include "bis_internal.hpp"

#include <algorithm>

extern "C" {

// two_stage_gauss_seidel, kernels.hpp:312-333.
bis_status bis_two_stage_gauss_seidel(bis_ctx *ctx, const bis_mat *strict, double *tmp,
                                      double *work, const double *D_inv, const double *input,
                                      double *output, int64_t n, int inner_iters) {
    BIS_CTX_OK(ctx);
    bis_status st = bis_elemwise_mult_vectors(ctx, work, D_inv, input, n, 1.0);   // :317
    if (st == BIS_OK) st = bis_copy_vector(ctx, output, work, n);                  // :319
    for (int inner = 1; st == BIS_OK && inner <= inner_iters; ++inner) {
        st = bis_spmv(ctx, strict, work, tmp);                                     // :323
        if (st == BIS_OK) st = bis_elemwise_mult_vectors(ctx, tmp, D_inv, tmp, n, -1.0); // :325
        std::swap(work, tmp);                                                      // :327
        if (st == BIS_OK) st = bis_sum_vectors(ctx, output, output, work, n, 1.0); // :331
    }
    return st;
}

// apply_preconditioner, kernels.hpp:336-414.
bis_status bis_apply_preconditioner(bis_ctx *ctx, int pc, int64_t n, const bis_mat *L_strict,
                                    const bis_mat *U_strict, const double *A_D,
                                    const double *A_D_inv, const double *L_D, const double *U_D,
                                    double *output, double *input, double *tmp, double *work,
                                    int outer_iters, int inner_iters) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n >= 0 && outer_iters >= 1, "bis_apply_preconditioner: bad arguments");
    if (pc == BIS_PC_MG) { // (not in the reference) the cycle of the hierarchy whose operand is in L_strict (bis_mg_operand); nothing else is read
        BIS_REQUIRE(ctx, L_strict && L_strict->mg && L_strict->n_rows == n, "bis_apply_preconditioner: MG needs the operand of a hierarchy of size n in L_strict");
        if (outer_iters != 1) { ctx->err = "bis_apply_preconditioner: MG with outer_iters != 1 is not built"; return BIS_ERR_UNSUPPORTED; }
        return bis_mg_apply(ctx, L_strict->mg, output, input);
    }
    if (pc == BIS_PC_BLOCK_JACOBI) { // (not in the reference) the inverse blocks of the handle whose operand is in L_strict (bis_bj_operand); nothing else is read
        BIS_REQUIRE(ctx, L_strict && L_strict->bj && L_strict->n_rows == n, "bis_apply_preconditioner: block Jacobi needs the operand of a handle of size n in L_strict");
        if (outer_iters != 1) { ctx->err = "bis_apply_preconditioner: block Jacobi with outer_iters != 1 is not built"; return BIS_ERR_UNSUPPORTED; }
        return bis_bj_apply(ctx, L_strict->bj, output, input);
    }
    if (pc == BIS_PC_ILU0_ITER)
        BIS_REQUIRE(ctx, L_strict && U_strict && inner_iters >= 0 && (n == 0 || (tmp && work && tmp != work && tmp != output &&
                         tmp != input && work != output && work != input)),
                    "bis_apply_preconditioner: ILU0_ITER needs both factors, inner_iters >= 0, and tmp, work distinct from each other, output and input");
    if (pc == BIS_PC_FSAI)
        BIS_REQUIRE(ctx, L_strict && U_strict && (n == 0 || (tmp && tmp != output && tmp != input)),
                    "bis_apply_preconditioner: FSAI needs both factors and tmp distinct from output and input");
    double *input_storage = nullptr;
    bis_status st = BIS_OK;
    if (outer_iters > 1) { // :348-352 (the one place the reference allocates in a kernel)
        st = bis_vec_alloc(ctx, n, &input_storage);
        if (st == BIS_OK) st = bis_copy_vector(ctx, input_storage, input, n);
    }
    for (int i = 0; st == BIS_OK && i < outer_iters; ++i) {
        switch (pc) {
        case BIS_PC_JACOBI:
            st = bis_elemwise_div_vectors(ctx, output, input, A_D, n, 1.0);        // :357
            break;
        case BIS_PC_GAUSS_SEIDEL:
            st = bis_sptrsv(ctx, L_strict, output, A_D, input);                    // :359
            break;
        case BIS_PC_BACKWARDS_GAUSS_SEIDEL:
            st = bis_bsptrsv(ctx, U_strict, output, A_D, input);                   // :361
            break;
        case BIS_PC_SYMMETRIC_GAUSS_SEIDEL:
            st = bis_sptrsv(ctx, L_strict, tmp, A_D, input);                       // :365
            if (st == BIS_OK) st = bis_elemwise_mult_vectors(ctx, tmp, tmp, A_D, n, 1.0); // :369
            if (st == BIS_OK) st = bis_bsptrsv(ctx, U_strict, output, A_D, tmp);   // :373
            break;
        case BIS_PC_TWO_STAGE_GS:
            st = bis_two_stage_gauss_seidel(ctx, L_strict, tmp, work, A_D_inv, input, output, n,
                                            inner_iters);                          // :376
            break;
        case BIS_PC_SYMMETRIC_TWO_STAGE_GS:
            st = bis_two_stage_gauss_seidel(ctx, L_strict, tmp, work, A_D_inv, input, output, n,
                                            inner_iters);                          // :379
            if (st == BIS_OK) st = bis_elemwise_mult_vectors(ctx, output, output, A_D, n, 1.0); // :382
            if (st == BIS_OK)
                st = bis_two_stage_gauss_seidel(ctx, U_strict, tmp, work, A_D_inv, output, output,
                                                n, inner_iters);                   // :384
            break;
        case BIS_PC_ILU0:
            st = bis_sptrsv(ctx, L_strict, tmp, L_D, input);                       // :390
            if (st == BIS_OK) st = bis_bsptrsv(ctx, U_strict, output, U_D, tmp);   // :394
            break;
        case BIS_PC_ILU0_ITER: // (not in the reference) both solves as bis_itrsv; A_D_inv carries 1 / U_D
            st = bis_itrsv(ctx, L_strict, L_D, input, tmp, work, inner_iters);
            if (st == BIS_OK) st = bis_itrsv(ctx, U_strict, A_D_inv, tmp, output, work, inner_iters);
            break;
        case BIS_PC_FSAI: // (not in the reference) output = Gt (G input): G in L_strict, Gt in U_strict (bis_mat_fsai)
            st = bis_spmv(ctx, L_strict, input, tmp);
            if (st == BIS_OK) st = bis_spmv(ctx, U_strict, tmp, output);
            break;
        default:
            st = bis_copy_vector(ctx, output, input, n);                           // :398
        }
        if (st == BIS_OK && outer_iters > 1 && i != outer_iters - 1)
            st = bis_copy_vector(ctx, input, output, n);                           // :401-403
    }
    if (st == BIS_OK && outer_iters > 1) st = bis_copy_vector(ctx, input, input_storage, n); // :406-408
    if (input_storage) bis_vec_free(ctx, input_storage);
    return st;
}

} // extern "C"
