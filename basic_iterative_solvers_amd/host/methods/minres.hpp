// minres.hpp -- (preconditioned) MINRES for symmetric, possibly indefinite matrices (no reference counterpart): the method
// -mr, built on the device schedule bis_minres_* the way ConjugateGradientSolver is built on bis_cg_*.  The first iterate()
// enqueues the solve in batches and reads the handle's history; the harness then walks that history iteration by iteration,
// so the table, the milestones and the summary are -cg's.  The entries are phibar: the residual norm in the M^-1 norm, the
// 2-norm without a preconditioner.  The preconditioner must be one fixed symmetric positive definite operator (nothing
// checks; the K-cycles of -p mg are refused in parse_cli).  There is no call-by-call form (-unfused and -hostscalars are
// refused in parse_cli).
#pragma once

#include "../solver.hpp"

class MINRESSolver : public Solver {
  public:
    double *x = nullptr; // device: the handle's iterate, updated in place
    bis_minres *mr = nullptr;
    std::vector<double> hist; // the handle's history: entries 0 .. iterations

    explicit MINRESSolver(const Args *a) : Solver(a) {}
    void allocate_structs(const int n) override {
        Solver::allocate_structs(n);
        x = dalloc(n);
    }
    void init_structs(const int n) override {
        Solver::init_structs(n);
        copy_vector(x, x_0, n);
    }
    void init_residual() override {
        bis::check(bis_minres_create(bis::ctx(), A->dev, b, x, &mr), "bis_minres_create");
        if (preconditioner != PrecondType::None)
            bis::check(bis_minres_set_preconditioner(bis::ctx(), mr, (int)preconditioner, L_strict ? L_strict->dev : nullptr,
                                                     U_strict ? U_strict->dev : nullptr, A_D, A_D_inv, L_D, U_D,
                                                     PRECOND_OUTER_ITERS, precond_inner_iters()), "bis_minres_set_preconditioner");
        bis::check(bis_minres_init(bis::ctx(), mr, tolerance, &residual_norm), "bis_minres_init");
        collected_residual_norms[collected_residual_norms_count++] = residual_norm;
    }
    void iterate(Timers *timers) override {
        if (!hist.empty()) return;
        // batches with a status read in between: what is enqueued behind the stop returns at once, but it is still launches,
        // and the sweeps of a preconditioner do not see the stop flag at all: batches of 8 there
        const bool sweeps = preconditioner != PrecondType::None && preconditioner != PrecondType::Jacobi;
        int it = 0, conv = 0, enq = 0;
        hist.assign(1, 0.0);
        while (enq < max_iters) {
            const int batch = std::min(sweeps ? 8 : 50, max_iters - enq);
            TIME(timers, "spmv", bis::check(bis_minres_iterate(bis::ctx(), mr, batch), "bis_minres_iterate"))
            enq += batch;
            hist.resize(enq + 1);
            bis::check(bis_minres_status(bis::ctx(), mr, &it, &conv, hist.data(), enq + 1), "bis_minres_status");
            if (it < enq) break; // the device stopped inside this batch
        }
        hist.resize(it + 1);
    }
    void exchange() override {}
    void record_residual_norm() override {
        residual_norm = hist[std::min<size_t>(iter_count, hist.size() - 1)];
        Solver::record_residual_norm();
    }
    void save_x_star() override {
        std::swap(x, x_star);
        Solver::save_x_star();
    }
    ~MINRESSolver() override {
        if (mr) bis_minres_destroy(bis::ctx(), mr);
        dfree(x);
    }
};
