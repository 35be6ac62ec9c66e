// bis_precond.hip -- the preconditioner dispatcher (reference kernels.hpp:312-414) over the library's own kernels: the
// triangular sweeps (bis_sptrsv.hip), the iterative triangular solves (bis_itrsv.hip), SpMV (the FSAI factors of
// bis_fsai.hip), the multigrid cycle (bis_mg.hip) and the vector kernels.
#include "bis_pc.hpp"

#include <algorithm>

// ---- the binding of the solver handles (bis_pc.hpp) ----------------------------------------------------------------------
// The one place that says what bis_apply_preconditioner / bis_mapply_preconditioner below read for a type.
bis_pc_needs bis_pc_needs_of(int pc) {
    const bool two = pc == BIS_PC_TWO_STAGE_GS || pc == BIS_PC_SYMMETRIC_TWO_STAGE_GS;
    const bool ilu = pc == BIS_PC_ILU0 || pc == BIS_PC_ILU0_ITER;
    const bool lower = pc == BIS_PC_GAUSS_SEIDEL || pc == BIS_PC_SYMMETRIC_GAUSS_SEIDEL || two || ilu || pc == BIS_PC_FSAI;
    const bool upper = pc == BIS_PC_BACKWARDS_GAUSS_SEIDEL || pc == BIS_PC_SYMMETRIC_GAUSS_SEIDEL ||
                       pc == BIS_PC_SYMMETRIC_TWO_STAGE_GS || ilu || pc == BIS_PC_FSAI;
    const bool need_AD = pc == BIS_PC_JACOBI || pc == BIS_PC_GAUSS_SEIDEL || pc == BIS_PC_BACKWARDS_GAUSS_SEIDEL ||
                         pc == BIS_PC_SYMMETRIC_GAUSS_SEIDEL || pc == BIS_PC_SYMMETRIC_TWO_STAGE_GS;
    const bool need_ADinv = two || pc == BIS_PC_ILU0_ITER; // (ILU0_ITER: A_D_inv carries 1 / U_D)
    const bool need_tmp = pc == BIS_PC_SYMMETRIC_GAUSS_SEIDEL || two || ilu || pc == BIS_PC_FSAI;
    return {lower, upper, need_AD, need_ADinv, /*LD*/ ilu, /*UD*/ pc == BIS_PC_ILU0, need_tmp, /*work*/ need_ADinv};
}

bis_status bis_pc_bind(bis_ctx *ctx, bis_pc_binding *b, const bis_pc_site &site, const bis_pc_args &a,
                       std::initializer_list<bis_pc_block> blocks) {
    auto refuse = [&](bis_status st, std::initializer_list<const char *> why) { // ctx->err = "<solver>_set_preconditioner: <why...>"
        ctx->err.assign(site.solver).append("_set_preconditioner: ");
        for (const char *w : why) ctx->err.append(w);
        return st;
    };
    const int pc = a.type;
    const int64_t n = site.n;
    const bool lockstep = site.n_rhs > 0, mg = pc == BIS_PC_MG;
    if (lockstep && mg) return refuse(BIS_ERR_UNSUPPORTED, {"the multigrid preconditioner has no multi-vector form"});
    if (!b || pc < BIS_PC_NONE || pc > BIS_PC_BLOCK_JACOBI || a.outer < 1 || a.inner < 0) return refuse(BIS_ERR_INVALID, {"bad arguments"});
    if (site.live) return refuse(BIS_ERR_INVALID, {"call it before ", site.solver, "_init / ", site.solver, "_iterate"});
    if (lockstep && (pc == BIS_PC_TWO_STAGE_GS || pc == BIS_PC_SYMMETRIC_TWO_STAGE_GS))
        return refuse(BIS_ERR_UNSUPPORTED, {"the two-stage Gauss-Seidel types have no multi-vector form"});
    if (lockstep && a.outer != 1) return refuse(BIS_ERR_UNSUPPORTED, {"outer_iters must be 1 on interleaved blocks"});
    if (site.cg && pc == BIS_PC_FSAI && !(a.L && a.U && a.L->n_rows == n && a.U->n_rows == n))
        return refuse(BIS_ERR_INVALID, {"FSAI needs both factors, of the solver's size"});
    if (mg || pc == BIS_PC_BLOCK_JACOBI) { // bis_apply_preconditioner's checks, in its order
        const char *what = mg ? "MG" : "block Jacobi";
        if (!(a.L && (mg ? a.L->mg != nullptr : a.L->bj != nullptr) && a.L->n_rows == n))
            return refuse(BIS_ERR_INVALID, {what, " needs the operand of a ", mg ? "hierarchy" : "handle", " of the solver's size in L_strict"});
        if (site.cg == 2 || a.outer != 1)
            return refuse(BIS_ERR_UNSUPPORTED, {what, site.cg ? " on a distributed handle, or with outer_iters != 1, is not built" : " with outer_iters != 1 is not built"});
    }
    // the operands the type reads (the dispatchers would refuse them only inside init / iterate)
    const bis_pc_needs need = bis_pc_needs_of(pc);
    if (!site.cg) { // bis_cg's laxity is kept on purpose: it leaves these refusals to the apply inside bis_cg_init
        if ((need.lower && !a.L) || (need.upper && !a.U)) return refuse(BIS_ERR_INVALID, {"the type needs a triangle that is null"});
        if ((need.lower && a.L->n_rows != n) || (need.upper && a.U->n_rows != n)) return refuse(BIS_ERR_INVALID, {"a triangle of another size"});
        if (n != 0 && ((need.AD && !a.AD) || (need.ADinv && !a.ADinv) || (need.LD && !a.LD) || (need.UD && !a.UD)))
            return refuse(BIS_ERR_INVALID, {"the type needs a diagonal that is null"});
    }
    // every allocation first: a failure leaves the handle as it was
    const int64_t scratch = site.ld * std::max(1, site.n_rhs);
    double *tmp = nullptr, *work = nullptr, *made[4] = {nullptr, nullptr, nullptr, nullptr};
    bis_status st = blocks.size() <= 4 ? BIS_OK : BIS_ERR_INVALID;
    int i = 0;
    for (const bis_pc_block &blk : blocks) {
        if (st == BIS_OK && blk.wanted) st = bis_vec_alloc(ctx, blk.count, &made[i]);
        ++i;
    }
    if (st == BIS_OK && need.tmp && !b->tmp) st = bis_vec_alloc(ctx, scratch, &tmp);
    if (st == BIS_OK && need.work && !b->work) st = bis_vec_alloc(ctx, scratch, &work);
    if (st != BIS_OK) {
        for (double *p : {made[0], made[1], made[2], made[3], tmp, work}) hipFree(p);
        return st;
    }
    i = 0;
    for (const bis_pc_block &blk : blocks) {
        if (made[i]) *blk.slot = made[i];
        ++i;
    }
    if (tmp) { b->tmp = tmp; b->own_tmp = true; }
    if (work) { b->work = work; b->own_work = true; }
    b->set = true;
    b->type = pc;
    b->L = a.L; b->U = a.U;
    b->AD = a.AD; b->ADinv = a.ADinv; b->LD = a.LD; b->UD = a.UD;
    b->outer = a.outer; b->inner = a.inner;
    return BIS_OK;
}

bis_status bis_pc_no_handle(bis_ctx *ctx, const char *solver, int n_rhs, int type) {
    return bis_pc_bind(ctx, nullptr, {solver, 0, 0, n_rhs, false, 0}, {type, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0}, {});
}

bis_status bis_pc_apply(bis_ctx *ctx, const bis_pc_binding &b, int64_t n, int n_rhs, double *out, double *in) {
    if (n_rhs > 0)
        return bis_mapply_preconditioner(ctx, b.type, n, n_rhs, b.L, b.U, b.AD, b.ADinv, b.LD, b.UD, out, in, b.tmp, b.work, b.outer, b.inner);
    return bis_apply_preconditioner(ctx, b.type, n, b.L, b.U, b.AD, b.ADinv, b.LD, b.UD, out, in, b.tmp, b.work, b.outer, b.inner);
}

void bis_pc_release(bis_pc_binding &b) {
    if (b.own_tmp) hipFree(b.tmp);
    if (b.own_work) hipFree(b.work);
    b = bis_pc_binding{};
}

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
