// bis_solver.hip -- the host side of bis_solver.hpp: a solver handle's shared state made, released and read.
#include "bis_solver.hpp"

bis_status bis_solver_core_alloc(bis_ctx *ctx, bis_solver_core *core, size_t n_flags, int hist_cols, int n_counter_sets,
                                 unsigned set_words) {
    core->hist_cap = 1 << 16;
    bis_status st = bis_vec_alloc(ctx, (int64_t)core->hist_cap * hist_cols, &core->hist);
    if (st == BIS_OK) st = bis_alloc_zeroed(ctx, &core->flags, n_flags);
    if (st == BIS_OK && n_counter_sets > 0) st = bis_alloc_zeroed(ctx, &core->counters, (size_t)n_counter_sets * set_words);
    return st;
}

void bis_solver_core_free(bis_solver_core *core) {
    hipFree(core->hist);
    hipFree(core->flags);
    hipFree(core->counters);
    bis_pc_release(core->pc);
}

bis_status bis_solver_read_flags(bis_ctx *ctx, const bis_solver_core &core, size_t offset, int count, int *out) {
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(out, core.flags + offset, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    BIS_SYNC_CHECK(ctx);
    return BIS_OK;
}

bis_status bis_solver_copy_hist(bis_ctx *ctx, const bis_solver_core &core, int j, int cnt, double *hist_host) {
    cnt = std::min(cnt, core.hist_cap);
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(hist_host, core.hist + (size_t)j * core.hist_cap, sizeof(double) * (size_t)cnt,
                                      hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return BIS_OK;
}
