// fgmres.hpp -- restarted flexible GMRES(m), right-preconditioned (no reference counterpart): the method -fgm, built on the
// device schedule bis_fgmres_* the way ConjugateGradientSolver is built on bis_cg_*.  The first iterate() enqueues the
// whole solve in batches and reads the handle's history; the harness then walks that history iteration by iteration, so the
// table, the restart entries (one more line per restart, as GMRESSolver::check_restart writes them) and the summary are
// -gm's.  The preconditioner may change from step to step: -p mg with -mg cycle=k|kgcr belongs here.  There is no
// call-by-call form (-unfused and -hostscalars are refused in parse_cli).
#pragma once

#include "../solver.hpp"

class FGMRESSolver : public Solver {
  public:
    double *x = nullptr; // device: the handle's iterate (x_old of the current cycle)
    bis_fgmres *fg = nullptr;
    std::vector<double> hist; // the handle's history: iters + 1 + restarts entries
    size_t hist_pos = 1;      // entry 0 opened the table in init_residual

    explicit FGMRESSolver(const Args *a) : Solver(a) {}
    void allocate_structs(const int n) override {
        Solver::allocate_structs(n);
        x = dalloc(n);
    }
    void init_structs(const int n) override {
        Solver::init_structs(n);
        copy_vector(x, x_0, n);
    }
    void init_residual() override {
        bis::check(bis_fgmres_create(bis::ctx(), A->dev, b, x, gmres_restart_len, &fg), "bis_fgmres_create");
        if (preconditioner != PrecondType::None)
            bis::check(bis_fgmres_set_preconditioner(bis::ctx(), fg, (int)preconditioner, L_strict ? L_strict->dev : nullptr,
                                                     U_strict ? U_strict->dev : nullptr, A_D, A_D_inv, L_D, U_D,
                                                     PRECOND_OUTER_ITERS, precond_inner_iters()), "bis_fgmres_set_preconditioner");
        bis::check(bis_fgmres_init(bis::ctx(), fg, tolerance, &residual_norm), "bis_fgmres_init");
        collected_residual_norms[collected_residual_norms_count++] = residual_norm;
    }
    void iterate(Timers *timers) override {
        if (!hist.empty()) return;
        // the harness stops a run that does not converge at the first iteration i with i + restarts >= max_iters, and there has
        // been a restart after every full cycle: the device gets exactly that many iterations
        const int m = gmres_restart_len;
        int budget = 1;
        while (budget + budget / m < max_iters) ++budget;
        // batches with a status read in between: what is enqueued behind the stop returns at once, but it is still launches,
        // and the sweeps of a preconditioner do not see the stop flag at all: batches of 8 there
        const int step = preconditioner != PrecondType::None ? 8 : 50;
        int it = 0, conv = 0, n_hist = 0, enq = 0;
        while (enq < budget) {
            const int batch = std::min(step, budget - enq);
            TIME(timers, "spmv", bis::check(bis_fgmres_iterate(bis::ctx(), fg, batch), "bis_fgmres_iterate"))
            enq += batch;
            bis::check(bis_fgmres_status(bis::ctx(), fg, &it, &conv, &n_hist, nullptr, 0), "bis_fgmres_status");
            if (it < enq) break; // the device stopped inside this batch
        }
        hist.assign((size_t)std::max(n_hist, 1), 0.0);
        bis::check(bis_fgmres_status(bis::ctx(), fg, &it, &conv, &n_hist, hist.data(), (int)hist.size()), "bis_fgmres_status");
    }
    double next_entry() {
        const double v = hist[std::min(hist_pos, hist.size() - 1)];
        ++hist_pos;
        return v;
    }
    void record_residual_norm() override {
        residual_norm = next_entry();
        Solver::record_residual_norm();
    }
    void check_restart(Timers *timers) override { // GMRESSolver::check_restart: the handle restarted where it says
        const bool conv = residual_norm < stopping_criteria;
        const bool over = iter_count > max_iters;
        const bool cycle = (iter_count % gmres_restart_len == 0) && iter_count != 0;
        if (!conv && !over && cycle && hist_pos < hist.size()) {
            gmres_restarted = true;
            residual_norm = next_entry(); // beta of the new cycle
            collected_residual_norms[collected_residual_norms_count++] = residual_norm;
            time_per_iteration[collected_residual_norms_count] = timers->per_iteration_time->check();
            ++gmres_restart_count;
        }
    }
    void exchange() override {}
    void save_x_star() override {
        bis::check(bis_fgmres_solution(bis::ctx(), fg, x_star), "bis_fgmres_solution");
        Solver::save_x_star();
    }
    ~FGMRESSolver() override {
        if (fg) bis_fgmres_destroy(bis::ctx(), fg);
        dfree(x);
    }
};
