// preprocessing.hpp -- setup phase, reference preprocessing.hpp:26-100:
// allocate + initialise the solver's vectors, optional symmetric diagonal
// scaling, split A into its strict triangles and diagonal (on the device for
// generated matrices, on the host for file input), optional ILU(0) or FSAI
// factors, the multigrid hierarchy or the block-Jacobi handle, initial residual and stopping criterion.
#pragma once

#include "common.hpp"
#include "solver.hpp"
#include "utilities/LU_factors.hpp"
#include "utilities/permute.hpp"

inline void download_to_host(MatrixCRS *A) { // device-generated matrix -> host arrays (setup only)
    if (A->row_ptr) return;
    A->row_ptr = new crs_index[A->n_rows + 1];
    A->col = new int[A->nnz ? A->nnz : 1];
    A->val = new double[A->nnz ? A->nnz : 1];
    bis::check(bis_mat_download(bis::ctx(), A->dev, A->row_ptr, A->col, A->val), "bis_mat_download");
}

inline void scale_mat(MatrixCRS *A, const double *s) { // preprocessing.hpp:15-24
    for (int r = 0; r < A->n_rows; ++r)
        for (crs_index i = A->row_ptr[r]; i < A->row_ptr[r + 1]; ++i) A->val[i] *= (s[r] * s[A->col[i]]);
}

// factor_LU, utilities/LU_factors.hpp:900-934
// -pprec 32: the two matrices the preconditioner applies by SpMV, rounded to fp32 in place (bis_mat_round_f32); their SpMV
// then streams 4-byte values.  Rounding is elementwise, so round(Gt) = round(G)^T bit for bit.
inline void round_precond_factors(Solver *s) {
    if (precond_value_bits() != 32) return;
    double change = 0.0, worst = 0.0;
    for (bis_mat *M : {s->L_strict->dev, s->U_strict->dev}) {
        bis::check(bis_mat_round_f32(bis::ctx(), M, &change), "bis_mat_round_f32");
        worst = change > worst ? change : worst;
    }
    std::cout << "preconditioner values rounded to fp32: max relative change " << worst << std::endl;
}

// -p bj: the inverted diagonal blocks of A (after -scale and -perm); the handle's operand takes the place of the strict lower triangle
inline void factor_block_jacobi(Solver *s) {
    int bs = precond_block_size();
    if (bs == 0) {
        int64_t g[4] = {0, 0, 0, 0};
        bis::check(bis_mat_grid_hint(s->A->dev, g), "bis_mat_grid_hint");
        if (g[0] > 0 && g[3] > 1 && g[3] <= 32) bs = (int)g[3];
    }
    if (bs == 0) {
        fprintf(stderr, "ERROR: -p bj: the matrix carries no grid hint with more than one unknown per node to take the block size from: give -bs N (1 <= N <= 32)\n");
        exit(EXIT_FAILURE);
    }
    // CG and MINRES assume a symmetric M: the inverse blocks are symmetrised there (bit for bit), elsewhere they stay as computed
    const bool sym = s->method == SolverType::ConjugateGradient || s->method == SolverType::MINRES;
    const bis_bj_params p = {bs, nullptr, 0, sym ? 1 : 0};
    const bis_status st = bis_bj_create(bis::ctx(), s->A->dev, &p, &s->bj);
    if (st == BIS_ERR_ZERO_DIAG || st == BIS_ERR_INVALID) { fprintf(stderr, "%s\n", bis_last_error(bis::ctx())); exit(EXIT_FAILURE); }
    bis::check(st, "bis_bj_create");
    s->L_strict->free_host();
    s->L_strict->adopt(const_cast<bis_mat *>(bis_bj_operand(s->bj)));
    int64_t n_blocks = 0, values = 0;
    int max_block = 0;
    bis_bj_info(s->bj, &n_blocks, &max_block, &values);
    const int64_t last = n_blocks > 0 ? (int64_t)s->N - (n_blocks - 1) * bs : 0;
    std::cout << "block Jacobi: " << n_blocks << " blocks of " << bs << " rows (last " << last << "), " << values << " stored values"
              << (s->perm_store ? ", consecutive rows of the permuted matrix" : "") << std::endl;
}

inline void factor_LU(Solver *s) {
    // split + diagonal on the device (bis_mat_split_strict: bit-identical to the reference's split_LU + peel_diag_crs,
    // tests/test_gpu_kernels.py), for generated and for file inputs alike; the host versions of utilities/LU_factors.hpp
    // remain for callers that hold host matrices
    {
        bis_mat *Ls = nullptr, *Us = nullptr;
        const bis_status st = bis_mat_split_strict(bis::ctx(), s->A->dev, &Ls, &Us, s->A_D, s->A_D_inv);
        if (st == BIS_ERR_ZERO_DIAG || st == BIS_ERR_NO_DIAG) { fprintf(stderr, "%s\n", bis_last_error(bis::ctx())); exit(EXIT_FAILURE); }
        bis::check(st, "bis_mat_split_strict");
        s->L_strict->adopt(Ls);
        s->U_strict->adopt(Us);
    }
    if (s->preconditioner == PrecondType::ILU0 || s->preconditioner == PrecondType::ILU0Iter) {
        // The reference's wired-in factor_ILU0_new needs the SMAX library (SURVEY.md
        // section 5, defect 2); this is its serial factor_ILU0_old arithmetic,
        // level-scheduled on the device.  Overwrites L_strict/U_strict, L_D, U_D.
        bis_mat *Ls = nullptr, *Us = nullptr;
        const int fill = precond_fill_level(); // -fill K: ILU(K) with level-of-fill; its factors are applied like ILU(0)'s
        int64_t n_fill = 0;
        if (fill > 0) {
            const bis_status st = bis_mat_iluk(bis::ctx(), s->A->dev, fill, ILU0_PIVOT_TOLERANCE, ILU0_PIVOT_REPLACEMENT, &Ls, &Us,
                                               s->L_D, s->U_D, &n_fill);
            if (st == BIS_ERR_NO_DIAG || st == BIS_ERR_UNSUPPORTED) { fprintf(stderr, "%s\n", bis_last_error(bis::ctx())); exit(EXIT_FAILURE); }
            bis::check(st, "bis_mat_iluk");
        } else
        bis::check(bis_mat_ilu0(bis::ctx(), s->A->dev, ILU0_PIVOT_TOLERANCE, ILU0_PIVOT_REPLACEMENT, &Ls, &Us,
                                s->L_D, s->U_D), "bis_mat_ilu0");
        s->L_strict->free_host();
        s->U_strict->free_host();
        s->L_strict->adopt(Ls);
        s->U_strict->adopt(Us);
        if (fill > 0) {
            const int64_t entries = s->L_strict->nnz + s->U_strict->nnz + (int64_t)s->N;
            std::cout << "ILU(" << fill << "): " << n_fill << " fill entries, L+U+D entries = " << entries << " ("
                      << (s->A->nnz > 0 ? (double)entries / (double)s->A->nnz : 1.0) << " x A)" << std::endl;
        }
        // -p ilu0it multiplies by the pivots' reciprocals: A_D_inv carries 1 / U_D for that type (L_D is the vector of ones)
        if (s->preconditioner == PrecondType::ILU0Iter) elemwise_div_vectors(s->A_D_inv, s->L_D, s->U_D, s->N);
        if (s->preconditioner == PrecondType::ILU0Iter) round_precond_factors(s); // (the diagonals L_D, U_D, 1 / U_D stay fp64)
    }
    if (s->preconditioner == PrecondType::FSAI) {
        // -p fsai: G and Gt = G^T take the places of the strict triangles (bis_apply_preconditioner reads them as two SpMVs)
        bis_mat *G = nullptr, *Gt = nullptr;
        int64_t n_fallback = 0;
        bis::check(bis_mat_fsai(bis::ctx(), s->A->dev, &G, &Gt, &n_fallback), "bis_mat_fsai");
        s->L_strict->free_host();
        s->U_strict->free_host();
        s->L_strict->adopt(G);
        s->U_strict->adopt(Gt);
        if (n_fallback != 0) std::cout << "fsai: " << n_fallback << " rows fell back to 1/sqrt(|a_ii|)" << std::endl;
        round_precond_factors(s);
    }
    if (s->preconditioner == PrecondType::MG) {
        // -p mg: the hierarchy of A (after -scale and -perm); its operand takes the place of the strict lower triangle
        const MGSmooth &sm = precond_mg_smooth();
        const bis_status st = sm.smooth ? bis_mg_create_smoothed(bis::ctx(), s->A->dev, &precond_mg_params(), sm.pomega, &s->mg)
                                        : bis_mg_create(bis::ctx(), s->A->dev, &precond_mg_params(), &s->mg);
        if (st == BIS_ERR_ZERO_DIAG || st == BIS_ERR_UNSUPPORTED || st == BIS_ERR_INVALID) { fprintf(stderr, "%s\n", bis_last_error(bis::ctx())); exit(EXIT_FAILURE); }
        bis::check(st, "bis_mg_create");
        s->L_strict->free_host();
        s->L_strict->adopt(const_cast<bis_mat *>(bis_mg_operand(s->mg)));
        int levels = 0, kind[16];
        int64_t rows[16], nnz[16];
        bis_mg_info(s->mg, &levels, rows, nnz, kind);
        double total = 0.0;
        for (int l = 0; l < levels; ++l) total += (double)nnz[l];
        std::cout << "multigrid: " << levels << " levels, rows";
        for (int l = 0; l < levels; ++l) std::cout << (l ? " / " : " ") << rows[l];
        std::cout << ", operator complexity " << (nnz[0] > 0 ? total / (double)nnz[0] : 1.0) << ", aggregates";
        for (int l = 0; l + 1 < levels; ++l) std::cout << (l ? " / " : " ") << (kind[l] == 1 ? "grid" : "mis");
        if (levels < 2) std::cout << " none";
        if (sm.smooth) std::cout << ", smoothed prolongators (omega " << (sm.pomega == 0.0 ? 4.0 / 3.0 : sm.pomega) << ")";
        std::cout << std::endl;
        const MGCycle &cyc = precond_mg_cycle();
        if (cyc.cycle != BIS_MG_CYCLE_V) { // (a command line without cycle= prints and computes what it always did)
            bis::check(bis_mg_set_cycle(bis::ctx(), s->mg, cyc.cycle, cyc.levels), "bis_mg_set_cycle");
            static const char *names[] = {"V", "W", "K (conjugate)", "K (GCR)"};
            const int covered = std::max(0, cyc.levels == 0 ? levels - 2 : std::min(cyc.levels, levels - 2));
            std::cout << "multigrid cycle: " << names[cyc.cycle] << ", transitions ";
            if (covered > 0) std::cout << "0.." << covered - 1;
            else std::cout << "none (the hierarchy has fewer than three levels: the V-cycle)";
            std::cout << std::endl;
        }
        const bis_mg_smoother &smo = precond_mg_smoother();
        if (smo.kind == BIS_MG_SMOOTH_CHEBYSHEV) { // (a command line without smoother=cheb prints and computes what it always did)
            const bis_status sst = bis_mg_set_smoother(bis::ctx(), s->mg, &smo);
            if (sst == BIS_ERR_INVALID) { fprintf(stderr, "%s\n", bis_last_error(bis::ctx())); exit(EXIT_FAILURE); }
            bis::check(sst, "bis_mg_set_smoother");
            std::cout << "multigrid smoother: Chebyshev, degree " << smo.degree << ", ratio " << smo.ratio << ", est " << smo.est_steps << ", safety "
                      << smo.safety << ", lambda_max";
            for (int l = 0; l < levels; ++l) {
                double lmax = 0.0;
                bis_mg_level_spectrum(s->mg, l, nullptr, nullptr, &lmax, nullptr);
                std::cout << (l ? " / " : " ") << lmax;
            }
            std::cout << std::endl;
        }
    }
    if (s->preconditioner == PrecondType::BlockJacobi) factor_block_jacobi(s);
}

inline void preprocessing(Args *cli_args, Solver *solver, Timers *timers, std::unique_ptr<MatrixCRS> &A) {
    (*timers)["preprocessing_init"].start();
    solver->allocate_structs(A->n_cols);
    solver->init_structs(A->n_cols);
    (*timers)["preprocessing_init"].stop();
    solver->A = std::move(A);

    if (solver->num_scale) { // preprocessing.hpp:39-50: A' = D^-1/2 A D^-1/2, b' = D^-1/2 b
        const int N = solver->A->n_rows;
        // extract_scale + scale_mat on the device (bis_mat_scale_sym); a matrix read from a file keeps its
        // host copy in step so that later host-side steps (host reordering fallback) see the scaled values
        init_vector(solver->A_D_scale, 0.0, N);
        {
            const bis_status sst = bis_mat_scale_sym(bis::ctx(), solver->A->dev, solver->A_D_scale);
            if (sst == BIS_ERR_ZERO_DIAG) { fprintf(stderr, "%s\n", bis_last_error(bis::ctx())); exit(EXIT_FAILURE); }
            bis::check(sst, "bis_mat_scale_sym");
        }
        if (solver->A->row_ptr) { // host copy present
            std::vector<double> s(N, 0.0);
            to_host(s.data(), solver->A_D_scale, N);
            scale_mat(solver->A.get(), s.data());
        }
        // the reference also scales x_0 here, after init_structs has already
        // copied the unscaled x_0 into the iterate; x_0 is not read again
        elemwise_mult_vectors(solver->x_0, solver->A_D_scale, solver->x_0, N);
        elemwise_mult_vectors(solver->b, solver->A_D_scale, solver->b, N);
    }

    if (cli_args->perm_mode == "mc") { // the SMAX permute_mat step (preprocessing.hpp:58-62)
        const int N = solver->A->n_rows;
        int n_colours = 0;
        std::vector<int> perm;
        // device path: colouring, permutation and P A P^T stay in HBM
        double *perm_store = nullptr;
        bis::check(bis_vec_alloc(bis::ctx(), (N + 1) / 2 + 1, &perm_store), "bis_vec_alloc");
        int32_t *perm_dev = reinterpret_cast<int32_t *>(perm_store);
        bis_mat *Bm = nullptr;
        const bis_status mc = cli_args->perm_host ? BIS_ERR_UNSUPPORTED
                                                  : bis_mat_multicolour(bis::ctx(), solver->A->dev, &Bm, perm_dev, &n_colours);
        if (mc == BIS_OK) {
            auto B = std::make_unique<MatrixCRS>();
            B->adopt(Bm);
            solver->A = std::move(B);
            if (solver->num_scale) { // b was rescaled row-wise: permute it (x_0 is constant)
                double *pb = nullptr;
                bis::check(bis_vec_alloc(bis::ctx(), N, &pb), "bis_vec_alloc");
                bis::check(bis_vec_gather(bis::ctx(), pb, solver->b, perm_dev, N), "bis_vec_gather");
                copy_vector(solver->b, pb, N);
                bis::check(bis_vec_free(bis::ctx(), pb), "bis_vec_free");
            }
            if (!cli_args->dump_perm.empty()) {
                std::vector<double> raw((N + 1) / 2 + 1);
                to_host(raw.data(), perm_store, (N + 1) / 2 + 1);
                const int32_t *pp = reinterpret_cast<const int32_t *>(raw.data());
                perm.assign(pp, pp + N);
            }
        } else { // more than 64 colours (or -perm-host): the host version
            download_to_host(solver->A.get());
            std::vector<int> inv_perm;
            multicolour_permutation(solver->A.get(), perm, inv_perm, n_colours);
            auto B = std::make_unique<MatrixCRS>();
            permute_matrix(solver->A.get(), perm, inv_perm, B.get());
            B->upload();
            solver->A = std::move(B);
            if (solver->num_scale) {
                std::vector<double> hb(N), pb(N);
                to_host(hb.data(), solver->b, N);
                for (int i = 0; i < N; ++i) pb[i] = hb[perm[i]];
                to_device(solver->b, pb.data(), N);
            }
        }
        if (mc == BIS_OK) solver->perm_store = perm_store; // kept: x* goes back to the natural order after the solve
        else { bis::check(bis_vec_free(bis::ctx(), perm_store), "bis_vec_free"); solver->keep_permutation(perm); }
        if (!cli_args->dump_perm.empty()) write_permutation(cli_args->dump_perm, perm);
        std::cout << "multi-colour reordering: " << n_colours << " colours" << std::endl;
    } else if (cli_args->perm_mode == "rcm" || cli_args->perm_mode == "bfs") {
        // bandwidth-reducing orderings: they keep the sweeps level-scheduled, with fewer or more levels than the
        // natural order depending on the input.  On the device (level-synchronous BFS, bis_order.hip) for structurally
        // symmetric patterns; the sequential host version otherwise, or with -perm-host.
        const int N = solver->A->n_rows;
        const bool rcm = cli_args->perm_mode == "rcm";
        std::vector<int> perm;
        double *perm_store = dalloc((N + 1) / 2 + 1);
        int32_t *perm_dev = reinterpret_cast<int32_t *>(perm_store);
        bis_status dev = cli_args->perm_host ? BIS_ERR_UNSUPPORTED : bis_mat_bfs_order(bis::ctx(), solver->A->dev, rcm ? 1 : 0, perm_dev);
        if (dev != BIS_OK && dev != BIS_ERR_UNSUPPORTED) bis::check(dev, "bis_mat_bfs_order");
        if (dev == BIS_OK) {
            bis_mat *Bm = nullptr;
            bis::check(bis_mat_permute(bis::ctx(), solver->A->dev, perm_dev, &Bm), "bis_mat_permute");
            auto B = std::make_unique<MatrixCRS>();
            B->adopt(Bm);
            solver->A = std::move(B);
            if (solver->num_scale) { // b was rescaled row-wise: permute it (x_0 is constant)
                double *pb = dalloc(N);
                bis::check(bis_vec_gather(bis::ctx(), pb, solver->b, perm_dev, N), "bis_vec_gather");
                copy_vector(solver->b, pb, N);
                dfree(pb);
            }
            solver->perm_store = perm_store;
            if (!cli_args->dump_perm.empty()) {
                std::vector<double> raw((N + 1) / 2 + 1);
                to_host(raw.data(), perm_store, (N + 1) / 2 + 1);
                const int32_t *pp = reinterpret_cast<const int32_t *>(raw.data());
                perm.assign(pp, pp + N);
            }
        } else {
            dfree(perm_store);
            download_to_host(solver->A.get());
            std::vector<int> inv_perm;
            bfs_like_permutation(solver->A.get(), rcm, perm, inv_perm);
            auto B = std::make_unique<MatrixCRS>();
            permute_matrix(solver->A.get(), perm, inv_perm, B.get());
            B->upload();
            solver->A = std::move(B);
            if (solver->num_scale) {
                std::vector<double> hb(N), pb(N);
                to_host(hb.data(), solver->b, N);
                for (int i = 0; i < N; ++i) pb[i] = hb[perm[i]];
                to_device(solver->b, pb.data(), N);
            }
            solver->keep_permutation(perm);
        }
        if (!cli_args->dump_perm.empty()) write_permutation(cli_args->dump_perm, perm);
        std::cout << (rcm ? "reverse Cuthill-McKee" : "breadth-first") << " reordering" << (dev == BIS_OK ? "" : " (host)") << std::endl;
    } else if (cli_args->perm_mode != "none") {
        fprintf(stderr, "ERROR: unknown -perm mode (available: mc, rcm, bfs)\n");
        exit(EXIT_FAILURE);
    }

    solver->L = std::make_unique<MatrixCRS>();
    solver->L_strict = std::make_unique<MatrixCRS>();
    solver->U = std::make_unique<MatrixCRS>();
    solver->U_strict = std::make_unique<MatrixCRS>();
    // -lsmr, -svd K: A may be rectangular and has no triangles or diagonal to split off (the methods take no preconditioner);
    // -eig K takes none either
    if (solver->method != SolverType::LSMR && solver->method != SolverType::Eigs && solver->method != SolverType::SVDS) TIME(timers, "preprocessing_factor", factor_LU(solver))

    (*timers)["preprocessing_init"].start();
    solver->init_residual();
    solver->init_stopping_criteria();
    (*timers)["preprocessing_init"].stop();
}
