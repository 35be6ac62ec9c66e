// eigs.hpp -- the K extreme eigenpairs of a symmetric matrix by thick-restart Lanczos (no reference counterpart): the method
// -eig K [-which sa|la|lm] [-ncv M], built on the device schedule bis_eigs_* the way MINRESSolver is built on bis_minres_*.
// There is no system A x = b: init_residual() runs the whole solve in batches of cycles and reads the handle's restart
// history; the harness then walks that history, one "iteration" per restart, so the table shows max_i<K of the residual
// estimates at every restart.  The tolerance is EIG_TOL, not the compile-time TOL of the linear solvers: an estimate of
// 1e-14 |lambda| lies at the rounding level of the products.  The summary adds the number of products, one line per pair and
// max ||A x - lambda x||_2 over the returned vectors, computed with bis_eigs_vectors, bis_spmv, bis_subtract_vectors and the
// norm.  No preconditioner, permutation, scaling of the system or call-by-call form (refused in parse_cli).
#pragma once

#include "../solver.hpp"

#define EIG_TOL 1e-10
#define EIG_MAX_CYCLES 1000

class EigsSolver : public Solver {
  public:
    bis_eigs *eg = nullptr;
    double *X = nullptr; // device: the K Ritz vectors, N rounded up to even apart
    int k, ncv, which;
    int products = 0, restarts = 0, stopped = 0, device_converged = 0, reason = 0, nconv = 0;
    std::vector<double> hist, values, est;
    double max_residual = 0.0;

    explicit EigsSolver(const Args *a) : Solver(a), k(eigs_k()), ncv(eigs_ncv()), which(eigs_which()) { tolerance = EIG_TOL; }
    void init_residual() override {
        bis::check(bis_eigs_create(bis::ctx(), A->dev, N, k, ncv, which, &eg), "bis_eigs_create");
        if (ncv == 0) eigs_ncv() = ncv = std::min(std::min(N, 64), std::max(2 * k + 1, 20)); // what the handle chose
        bis::check(bis_eigs_init(bis::ctx(), eg, tolerance), "bis_eigs_init");
        values.assign(k, 0.0);
        est.assign(k, 0.0);
        for (int cycles = 0; cycles < EIG_MAX_CYCLES && !stopped; cycles += 4) {
            bis::check(bis_eigs_iterate(bis::ctx(), eg, 4), "bis_eigs_iterate");
            bis::check(bis_eigs_status(bis::ctx(), eg, &products, &restarts, &stopped, &device_converged, &reason, &nconv, nullptr,
                                       nullptr, nullptr, nullptr, 0), "bis_eigs_status");
        }
        hist.assign(std::max(restarts, 1), 0.0);
        bis::check(bis_eigs_status(bis::ctx(), eg, &products, &restarts, &stopped, &device_converged, &reason, &nconv, values.data(),
                                   est.data(), hist.data(), nullptr, (int)hist.size()), "bis_eigs_status");
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
        const long ldx = ((long)N + 1) & ~1L; // every vector on a 16-byte boundary
        X = dalloc(ldx * k);
        bis::check(bis_eigs_vectors(bis::ctx(), eg, X, ldx), "bis_eigs_vectors");
        for (int i = 0; i < k; ++i) {
            if (reason == BIS_EIGS_INVARIANT && i >= nconv) break; // fewer than K vectors span the invariant subspace
            bis::check(bis_spmv(bis::ctx(), A->dev, X + i * ldx, tmp), "bis_spmv");
            subtract_vectors(work, tmp, X + i * ldx, N, values[i]);
            max_residual = std::max(max_residual, euclidean_vec_norm(work, N));
        }
    }
    void summary_extra() override {
        static const char *why[] = {"live", "converged", "invariant subspace", "jacobi", "bad start vector"};
        std::cout << "Operator products: " << products << ", restarts: " << restarts << ", stop reason: " << why[reason]
                  << ", converged pairs: " << nconv << " of " << k << std::endl;
        std::cout << std::scientific << std::setprecision(16);
        for (int i = 0; i < k; ++i) {
            if (restarts == 0 || (reason == BIS_EIGS_INVARIANT && i >= nconv)) break;
            std::cout << "lambda_" << i << " = " << values[i] << " residual estimate = " << est[i] << std::endl;
        }
        std::cout << "max ||A x - lambda x||_2 = " << max_residual << std::endl;
    }
    ~EigsSolver() override {
        if (eg) bis_eigs_destroy(bis::ctx(), eg);
        dfree(X);
    }
};
