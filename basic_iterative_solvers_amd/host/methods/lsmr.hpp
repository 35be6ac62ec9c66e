// lsmr.hpp -- LSMR for least-squares problems min ||A x - b||^2 + damp^2 ||x||^2 with a rectangular A (no reference
// counterpart): the method -lsmr [-damp L] [-colscale], built on the device schedule bis_lsmr_* the way MINRESSolver is built
// on bis_minres_*.  It is the one method that takes a matrix with other than as many rows as columns: b = B_VAL has as many
// entries as A has rows, x_0 = INIT_X_VAL as many as it has columns, and the residual buffers of save_x_star are the
// method's own.  The first iterate() enqueues the solve in batches and reads the handle's two histories; the harness then
// walks the `r` column iteration by iteration, so the table, the milestones and -dump-x are -mr's.  The solve also stops
// where the handle stopped by its test on the `ar` column (the residual of the normal equations), which is the only test
// an inconsistent system can meet; the summary prints the last `ar` entry on a line of its own.  With -damp the table is the
// norm of the stacked residual, with -colscale (d = 1 / the column norms of A) `ar` is measured in the scaled variable
// (include/bis_hip.h).  No preconditioner, permutation, scaling of the system or call-by-call form (refused in parse_cli).
#pragma once

#include "../solver.hpp"

class LSMRSolver : public Solver {
  public:
    double *x = nullptr;     // device: the handle's iterate, updated in place (n_cols)
    double *b_m = nullptr;   // device: the right-hand side (n_rows)
    double *res_m = nullptr, *tmp_m = nullptr; // device: b - A x* and its scratch (n_rows)
    double *d = nullptr;     // device: the column scaling of -colscale (n_cols)
    bis_mat *At = nullptr;
    bis_lsmr *ls = nullptr;
    double damp = 0.0;
    bool colscale = false;
    int reason = 0, device_converged = 0;
    std::vector<double> hist_ar, hist_r; // the handle's histories: entries 0 .. iterations

    explicit LSMRSolver(const Args *a) : Solver(a), damp(a->damp), colscale(a->colscale) {}
    void allocate_structs(const int n) override {
        Solver::allocate_structs(n);
        x = dalloc(n);
    }
    void init_structs(const int n) override {
        Solver::init_structs(n);
        copy_vector(x, x_0, n);
    }
    void init_residual() override {
        const int m = A->n_rows;
        b_m = dalloc(m); res_m = dalloc(m); tmp_m = dalloc(m);
        init_vector(b_m, B_VAL, m);
        bis::check(bis_mat_transpose(bis::ctx(), A->dev, &At), "bis_mat_transpose");
        bis::check(bis_lsmr_create(bis::ctx(), A->dev, At, b_m, x, &ls), "bis_lsmr_create");
        bis::check(bis_lsmr_set_damping(bis::ctx(), ls, damp), "bis_lsmr_set_damping");
        if (colscale) {
            d = dalloc(N);
            bis::check(bis_mat_row_norms(bis::ctx(), At, d), "bis_mat_row_norms");
            bis::check(bis_lsmr_scaling_from_norms(bis::ctx(), d, N, d), "bis_lsmr_scaling_from_norms");
            bis::check(bis_lsmr_set_col_scaling(bis::ctx(), ls, d), "bis_lsmr_set_col_scaling");
        }
        double ar0 = 0.0;
        bis::check(bis_lsmr_init(bis::ctx(), ls, tolerance, tolerance, &residual_norm, &ar0), "bis_lsmr_init");
        collected_residual_norms[collected_residual_norms_count++] = residual_norm;
    }
    void iterate(Timers *timers) override {
        if (!hist_r.empty()) return;
        int it = 0, enq = 0;
        hist_r.assign(1, 0.0);
        while (enq < max_iters) {
            const int batch = std::min(50, max_iters - enq);
            TIME(timers, "spmv", bis::check(bis_lsmr_iterate(bis::ctx(), ls, batch), "bis_lsmr_iterate"))
            enq += batch;
            hist_r.resize(enq + 1);
            hist_ar.resize(enq + 1);
            bis::check(bis_lsmr_status(bis::ctx(), ls, &it, &device_converged, &reason, hist_ar.data(), hist_r.data(), enq + 1), "bis_lsmr_status");
            if (it < enq) break; // the device stopped inside this batch
        }
        hist_r.resize(it + 1);
        hist_ar.resize(it + 1);
    }
    void exchange() override {}
    void record_residual_norm() override {
        residual_norm = hist_r[std::min<size_t>(iter_count, hist_r.size() - 1)];
        Solver::record_residual_norm();
    }
    // also where the handle stopped: by its `ar` test, a breakdown or a non-finite entry (an x_0 that is optimal already
    // leaves a history of one entry: the harness' first pass ends the solve)
    bool check_stopping_criteria() override { return Solver::check_stopping_criteria() || iter_count + 1 >= (int)hist_r.size(); }
    void save_x_star() override {
        std::swap(x, x_star);
        bis::check(bis_compute_residual(bis::ctx(), A->dev, x_star, b_m, res_m, tmp_m), "bis_compute_residual");
        residual_norm = euclidean_vec_norm(res_m, A->n_rows);
        collected_residual_norms[collected_residual_norms_count + 1] = residual_norm;
        if (reason != 0) convergence_flag = device_converged != 0;
    }
    void summary_extra() override {
        std::cout << "||A^T(A*x - b)||_2 estimate = " << std::scientific << (hist_ar.empty() ? 0.0 : hist_ar.back())
                  << (colscale ? " (in the scaled variable)" : "") << (damp != 0.0 ? " (damped)" : "") << std::endl;
    }
    ~LSMRSolver() override {
        if (ls) bis_lsmr_destroy(bis::ctx(), ls);
        if (At) bis_mat_destroy(bis::ctx(), At);
        for (double *p : {x, b_m, res_m, tmp_m, d}) dfree(p);
    }
};
