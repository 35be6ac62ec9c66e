// bis_solver.hpp -- what the device-schedule solver handles share (bis_cg, bis_mcg, bis_mbicgstab, bis_mgmres, bis_fgmres,
// bis_minres, bis_idr, bis_lsmr, bis_eigs, bis_svds, bis_stat): the state of one life cycle (create, [set_preconditioner], init, iterate ..., status,
// destroy) with its allocation, release and the two reads *_status is made of; the scope in which a solve's stop flag
// reaches the shared launchers; the layout of a last-arriver counter set; the scalar last-arriver reduction.  The host
// functions are implemented in bis_solver.hip.
#pragma once

#include "bis_pc.hpp"

#include <algorithm>

// ---- the handle core -------------------------------------------------------------------------------------------------
// Every handle struct derives from it (a plain base: no virtuals) and keeps what only its method needs.
struct bis_solver_core {
    int *flags = nullptr;         // device: the handle's words, zeroed at creation (each handle documents its layout)
    double *hist = nullptr;       // device: [hist_cols][hist_cap] residual history
    int hist_cap = 0;
    int enqueued = 0;             // iterations enqueued since the last *_init
    bool initialised = false;     // *_init has run
    unsigned *counters = nullptr; // device: the last-arriver counter sets, zeroed at creation (bis_stat: none)
    bis_pc_binding pc;            // what *_set_preconditioner bound (bis_stat: nothing)
};

// flags (n_flags ints), the history (hist_cols columns of 65536 entries) and n_counter_sets sets of set_words counters.
// On a failure the caller's *_destroy releases what was made.
bis_status bis_solver_core_alloc(bis_ctx *ctx, bis_solver_core *core, size_t n_flags, int hist_cols, int n_counter_sets,
                                 unsigned set_words);
// frees the three arrays and what the binding owns
void bis_solver_core_free(bis_solver_core *core);
// initialised or enqueued: *_set_preconditioner (and bis_idr_set_shadow) come too late
inline bool bis_solver_live(const bis_solver_core &core) { return core.initialised || core.enqueued != 0; }
// out[0 .. count) = flags[offset ...]: blocks, and answers a fault a kernel raised
bis_status bis_solver_read_flags(bis_ctx *ctx, const bis_solver_core &core, size_t offset, int count, int *out);
// hist_host[0 .. cnt) = column j of the history, cnt clamped to the column's capacity: blocks (no fault check: the read of
// the flags before it made one)
bis_status bis_solver_copy_hist(bis_ctx *ctx, const bis_solver_core &core, int j, int cnt, double *hist_host);

// While it lives, the launchers the iteration goes through (SpMV, SpMM, sweeps, diagonal applies) take flags[1] as the
// stop flag of the solve that is enqueuing; the flag must not outlive the *_iterate call.
struct bis_stop_guard {
    bis_ctx *ctx;
    bis_stop_guard(bis_ctx *c, const int *flags) : ctx(c) { c->spmv_stop = flags; }
    ~bis_stop_guard() { ctx->spmv_stop = nullptr; }
    bis_stop_guard(const bis_stop_guard &) = delete;
    bis_stop_guard &operator=(const bis_stop_guard &) = delete;
};

// ---- grids -----------------------------------------------------------------------------------------------------------
constexpr int kSolverT = 256; // threads per workgroup of the handles' passes
// one lane per 16 bytes (a pair of doubles); a reduction's partials are indexed by workgroup, so its cap is also the
// bound of its counter set
inline int bis_pair_grid(int64_t n, int cap) {
    const int64_t g = ((n >> 1) + kSolverT - 1) / kSolverT;
    return (int)std::min<int64_t>(std::max<int64_t>(g, 1), cap);
}
// one lane per entry, for elementwise passes that walk 8 bytes per lane
inline int lane_grid(int64_t n) {
    return (int)std::min<int64_t>(std::max<int64_t>((n + kSolverT - 1) / kSolverT, 1), kMaxEwBlocks);
}

// ---- one last-arriver counter set ------------------------------------------------------------------------------------
// [0] the top counter, [1 .. 3] padding, [4 ...] one sub counter per kArriveGroup workgroups (arrive_last2).  A handle sizes
// its sets with the cap of the grid it launches the reduction with -- kMaxReduceBlocks or kMaxDotBlocks.  (bis_cg.hip keeps a
// layout of its own: the pap counter sits in the padding of its one set.)
constexpr unsigned kCounterSubBase = 4;
constexpr unsigned bis_counter_set_words(unsigned max_blocks) {
    return kCounterSubBase + (max_blocks + kArriveGroup - 1) / kArriveGroup;
}
// thread 0 only; true in the workgroup that arrives last of n_blocks (n_blocks at most the cap the set was sized with)
__device__ __forceinline__ bool arrive_last_set(unsigned *set, unsigned block, unsigned n_blocks) {
    return arrive_last2(set, set + kCounterSubBase, block, n_blocks);
}

// ---- the scalar reduction --------------------------------------------------------------------------------------------
// NV sums at once, blockDim.x == kSolverT: the workgroup's sums go to partials[v * gridDim.x + blockIdx.x]; returns (in
// every lane) whether this workgroup arrived last -- its thread 0 then holds in total[v] the sum of all partials of v: lane
// t adds the workgroups t, t + 256, ... in index order, the lanes are folded in the fixed order of block_sum.
template <int NV>
__device__ __forceinline__ bool reduce_last(const double (&acc)[NV], double *lds /*[NV * kSolverT / 64]*/, double *partials,
                                            unsigned *counter, double (&total)[NV]) {
    __shared__ bool last;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double sum = block_sum<kSolverT>(acc[v], lds + v * (kSolverT / 64));
        if (threadIdx.x == 0) publish(partials + (size_t)v * gridDim.x + blockIdx.x, sum);
    }
    if (threadIdx.x == 0) last = arrive_last_set(counter, blockIdx.x, gridDim.x);
    __syncthreads();
    if (!last) return false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double a = 0.0;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += kSolverT) a += fetch(partials + (size_t)v * gridDim.x + i);
        total[v] = block_sum<kSolverT>(a, lds + v * (kSolverT / 64));
    }
    return true;
}
