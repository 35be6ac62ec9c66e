// idr.hpp -- (right-preconditioned) IDR(s) for nonsymmetric matrices (no reference counterpart): the method -idr [-ids S],
// built on the device schedule bis_idr_* the way MINRESSolver is built on bis_minres_*.  The first iterate() enqueues the
// solve in batches and reads the handle's history; the harness then walks that history iteration by iteration, so the
// table, the milestones and the summary are -bi's.  An iteration is one position of a cycle of s + 1: one SpMV and one
// preconditioner apply.  The entries are the recurrence of the true residual norm || b - A x ||.  The preconditioner must
// be one fixed operator (nothing checks; the K-cycles of -p mg are refused in parse_cli).  There is no call-by-call form
// (-unfused and -hostscalars are refused in parse_cli).
#pragma once

#include "../solver.hpp"

class IDRSolver : public Solver {
  public:
    double *x = nullptr; // device: the handle's iterate, updated in place
    bis_idr *idr = nullptr;
    std::vector<double> hist; // the handle's history: entries 0 .. iterations

    explicit IDRSolver(const Args *a) : Solver(a) {}
    void allocate_structs(const int n) override {
        Solver::allocate_structs(n);
        x = dalloc(n);
    }
    void init_structs(const int n) override {
        Solver::init_structs(n);
        copy_vector(x, x_0, n);
    }
    void init_residual() override {
        bis::check(bis_idr_create(bis::ctx(), A->dev, b, x, idr_shadow_dim(), &idr), "bis_idr_create");
        if (preconditioner != PrecondType::None)
            bis::check(bis_idr_set_preconditioner(bis::ctx(), idr, (int)preconditioner, L_strict ? L_strict->dev : nullptr,
                                                  U_strict ? U_strict->dev : nullptr, A_D, A_D_inv, L_D, U_D,
                                                  PRECOND_OUTER_ITERS, precond_inner_iters()), "bis_idr_set_preconditioner");
        bis::check(bis_idr_init(bis::ctx(), idr, tolerance, &residual_norm), "bis_idr_init");
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
            TIME(timers, "spmv", bis::check(bis_idr_iterate(bis::ctx(), idr, batch), "bis_idr_iterate"))
            enq += batch;
            hist.resize(enq + 1);
            bis::check(bis_idr_status(bis::ctx(), idr, &it, &conv, hist.data(), enq + 1), "bis_idr_status");
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
    ~IDRSolver() override {
        if (idr) bis_idr_destroy(bis::ctx(), idr);
        dfree(x);
    }
};
