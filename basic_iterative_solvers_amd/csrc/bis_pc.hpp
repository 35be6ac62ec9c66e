// bis_pc.hpp -- the preconditioner a solver handle keeps from its *_set_preconditioner call (bis_cg, bis_mcg, bis_mbicgstab,
// bis_mgmres, bis_fgmres, bis_minres, bis_idr -- every handle but bis_stat, which has none; the binding is a member of
// bis_solver.hpp's bis_solver_core): one binding, one table of what a type reads, one check-and-bind, one apply, one
// release.  Implemented in bis_precond.hip, next to the dispatcher the table describes.
#pragma once

#include "bis_internal.hpp"

#include <initializer_list>

struct bis_pc_binding {
    bool set = false;  // a set_preconditioner call has succeeded (bis_cg, bis_mcg: until then their creation-time A_D rules)
    int type = BIS_PC_NONE;
    const bis_mat *L = nullptr, *U = nullptr;
    const double *AD = nullptr, *ADinv = nullptr, *LD = nullptr, *UD = nullptr;
    double *tmp = nullptr, *work = nullptr;  // the apply's scratch, where the type needs it
    bool own_tmp = false, own_work = false;  // allocated by bis_pc_bind (bis_cg lends its own tmp)
    int outer = 1, inner = 0;
};

// what a type reads and which scratch its apply needs, for both vector forms (the lock-step handles accept a subset of the types)
struct bis_pc_needs { bool lower, upper, AD, ADinv, LD, UD, tmp, work; };
bis_pc_needs bis_pc_needs_of(int type);

// the nine user arguments of a *_set_preconditioner call
struct bis_pc_args {
    int type;
    const bis_mat *L, *U;
    const double *AD, *ADinv, *LD, *UD;
    int outer, inner;
};

// who binds
struct bis_pc_site {
    const char *solver;  // "bis_mcg": the error text starts "bis_mcg_set_preconditioner: "
    int64_t n, ld;       // the solver's size; the scratch blocks are ld * max(1, n_rhs) doubles
    int n_rhs;           // 0: the single-vector rules; 1..8: the lock-step rules (no MG, no two-stage type, outer_iters == 1)
    bool live;           // initialised or enqueued: refused
    int cg;              // bis_cg's laxer refusals: 0 no, 1 yes, 2 yes and the handle is distributed
};

// a block of the handle's own that the call makes with the scratch: `count` doubles into *slot where `wanted`
struct bis_pc_block { double **slot; int64_t count; bool wanted; };

// Every refusal of a *_set_preconditioner call in its family's order, then every allocation, then the commit: a failure
// leaves the binding and the blocks as they were.
bis_status bis_pc_bind(bis_ctx *ctx, bis_pc_binding *b, const bis_pc_site &site, const bis_pc_args &a,
                       std::initializer_list<bis_pc_block> blocks);
// what the call answers without a handle
bis_status bis_pc_no_handle(bis_ctx *ctx, const char *solver, int n_rhs, int type);
// out = M^-1 in; n_rhs as in bis_pc_site
bis_status bis_pc_apply(bis_ctx *ctx, const bis_pc_binding &b, int64_t n, int n_rhs, double *out, double *in);
// frees the scratch the binding owns
void bis_pc_release(bis_pc_binding &b);
