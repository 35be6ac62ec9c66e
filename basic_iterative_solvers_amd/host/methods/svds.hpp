// svds.hpp -- the K largest or smallest singular triplets of a matrix of any shape by thick-restart Lanczos bidiagonalisation
// (no reference counterpart): the method -svd K [-which lm|sm] [-ncv M], built on the device schedule bis_svds_* the way
// EigsSolver is built on bis_eigs_*.  Like -lsmr it takes a rectangular .mtx.  There is no system A x = b: init_residual()
// runs the whole solve in batches of cycles and reads the handle's restart history; the harness then walks that history, one
// "iteration" per restart, so the table shows max_i<K of the residual estimates at every restart.  The tolerance is SVD_TOL,
// relative to the largest singular value seen (the handle's sigma_ref), not the compile-time TOL of the linear solvers.  The
// summary adds the number of products, one line per triplet and max ||A v - sigma u||_2 + ||A^T u - sigma v||_2 over the
// returned vectors, computed with bis_svds_vectors, bis_spmv on A and on its transpose, bis_subtract_vectors and the norm.
// -which sm uses plain Ritz values: slow on ill-conditioned matrices (include/bis_hip.h).  No preconditioner, permutation,
// scaling of the system or call-by-call form (refused in parse_cli).
#pragma once

#include "../solver.hpp"

#define SVD_TOL 1e-10
#define SVD_MAX_CYCLES 1000

class SVDSSolver : public Solver {
  public:
    bis_svds *sv = nullptr;
    bis_mat *At = nullptr;
    double *U = nullptr, *V = nullptr;         // device: the K left and right vectors, the lengths rounded up to even apart
    double *t_m = nullptr, *w_m = nullptr;     // device: residual scratch, n_rows entries
    double *t_n = nullptr, *w_n = nullptr;     // device: residual scratch, n_cols entries
    int k, ncv, which;
    int products = 0, restarts = 0, stopped = 0, device_converged = 0, reason = 0, nconv = 0;
    double sigma_ref = 0.0;
    std::vector<double> hist, values, est;
    double max_residual = 0.0;

    explicit SVDSSolver(const Args *a) : Solver(a), k(svds_k()), ncv(svds_ncv()), which(svds_which()) { tolerance = SVD_TOL; }
    void init_residual() override {
        const int rows = A->n_rows, cols = N;
        bis::check(bis_mat_transpose(bis::ctx(), A->dev, &At), "bis_mat_transpose");
        bis::check(bis_svds_create(bis::ctx(), A->dev, At, rows, cols, k, ncv, which, &sv), "bis_svds_create");
        if (ncv == 0) svds_ncv() = ncv = std::min(std::min(std::min(rows, cols), 64), std::max(2 * k + 1, 20)); // what the handle chose
        bis::check(bis_svds_init(bis::ctx(), sv, tolerance), "bis_svds_init");
        values.assign(k, 0.0);
        est.assign(k, 0.0);
        for (int cycles = 0; cycles < SVD_MAX_CYCLES && !stopped; cycles += 4) {
            bis::check(bis_svds_iterate(bis::ctx(), sv, 4), "bis_svds_iterate");
            bis::check(bis_svds_status(bis::ctx(), sv, &products, &restarts, &stopped, &device_converged, &reason, &nconv, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, 0), "bis_svds_status");
        }
        hist.assign(std::max(restarts, 1), 0.0);
        bis::check(bis_svds_status(bis::ctx(), sv, &products, &restarts, &stopped, &device_converged, &reason, &nconv, &sigma_ref,
                                   values.data(), est.data(), hist.data(), nullptr, (int)hist.size()), "bis_svds_status");
        if ((int)hist.size() > max_iters) hist.resize(max_iters); // the table's capacity
        residual_norm = hist[0];
        collected_residual_norms[collected_residual_norms_count++] = residual_norm;
    }
    void iterate(Timers *) override {}
    void exchange() override {}
    void record_residual_norm() override {
        residual_norm = hist[std::min<size_t>(iter_count, hist.size() - 1)];
        Solver::record_residual_norm();
    }
    // the walk ends with the history (one restart only: the harness' first pass ends it)
    bool check_stopping_criteria() override { return iter_count + 1 >= (int)hist.size(); }
    void save_x_star() override {
        convergence_flag = device_converged != 0;
        iter_count = restarts;
        if (restarts == 0) return; // a bad start vector: there are no vectors
        const long rows = A->n_rows, cols = N;
        const long ldu = (rows + 1) & ~1L, ldv = (cols + 1) & ~1L; // every vector on a 16-byte boundary
        U = dalloc(ldu * k); V = dalloc(ldv * k);
        t_m = dalloc(ldu); w_m = dalloc(ldu); t_n = dalloc(ldv); w_n = dalloc(ldv);
        bis::check(bis_svds_vectors(bis::ctx(), sv, U, ldu, V, ldv), "bis_svds_vectors");
        for (int i = 0; i < k; ++i) {
            if (reason == BIS_SVDS_INVARIANT && i >= nconv) break; // fewer than K vectors span the invariant subspace
            bis::check(bis_spmv(bis::ctx(), A->dev, V + i * ldv, t_m), "bis_spmv");
            subtract_vectors(w_m, t_m, U + i * ldu, rows, values[i]);
            bis::check(bis_spmv(bis::ctx(), At, U + i * ldu, t_n), "bis_spmv");
            subtract_vectors(w_n, t_n, V + i * ldv, cols, values[i]);
            max_residual = std::max(max_residual, euclidean_vec_norm(w_m, rows) + euclidean_vec_norm(w_n, cols));
        }
    }
    void summary_extra() override {
        static const char *why[] = {"live", "converged", "invariant subspace", "jacobi", "bad start vector"};
        std::cout << "Operator products: " << products << ", restarts: " << restarts << ", stop reason: " << why[reason]
                  << ", converged triplets: " << nconv << " of " << k << std::endl;
        std::cout << std::scientific << std::setprecision(16);
        for (int i = 0; i < k; ++i) {
            if (restarts == 0 || (reason == BIS_SVDS_INVARIANT && i >= nconv)) break;
            std::cout << "sigma_" << i << " = " << values[i] << " residual estimate = " << est[i] << std::endl;
        }
        std::cout << "max ||A v - sigma u||_2 + ||A^T u - sigma v||_2 = " << max_residual << std::endl;
    }
    ~SVDSSolver() override {
        if (sv) bis_svds_destroy(bis::ctx(), sv);
        if (At) bis_mat_destroy(bis::ctx(), At);
        for (double *p : {U, V, t_m, w_m, t_n, w_n}) dfree(p);
    }
};
