// bis_sptrsm.hip -- triangular sweeps on 1 <= k <= 8 right-hand sides stored interleaved (X[r*k + j], bis_spmm's layout):
// X_j = (D + T)^-1 B_j for a strictly lower (bis_sptrsm) or upper (bis_bsptrsm) triangle T.
//
// Arithmetic (the contract of include/bis_hip.h): for every row r in dependency order and every column j, acc = 0.0, then
// for the row's entries in CRS storage order acc = fma(val[e], X[col[e]*k + j], acc), then X[r*k + j] = (B[r*k + j] - acc)
// / D[r] -- the reference's serial loop (kernels.hpp:54-117) with product and sum fused, which is what the tiled, chained,
// per-level, wave-per-row and lane-per-row forms of bis_sptrsv run: there column j of the result is bis_sptrsv on column
// j bit for bit.  (The row-block form of bis_sptrsv rounds each product before it adds: the same bits only where the
// products are exact, see include/bis_hip.h.)  The columns never mix.
//
// What k vectors buy: the sweeps are latency-bound (one cross-CU hand-off per dependency level, a serial fma chain per
// row).  The hand-off, the poll and the index loads are paid once per row instead of once per row and vector; with k = 8
// the 64-byte line that held one useful operand holds eight; the k chains are independent and run on neighbouring lanes.
//
// Level-scheduled forms only (the tiled and the chained sweep have no multi-vector version), on a plan of their own per
// side (bis_trsm_plan: level-sorted rows, level boundaries, positions of the columns, scratch -- structure only, built
// from bis_trsv_analyse_device at the first call; the single-vector side's plan is never read, so the form that side
// takes does not matter here; the scratch and the positions are made at the persistent form's first launch):
//
//   form       kernel                   taken where                          option trsm_form
//   ---------  -----------------------  -----------------------------------  ----------------
//   per-level  trsm_level_kernel<RP,K>  at most 64 levels (multi-colour      1: at any level count
//                                       orderings): one plain launch per
//                                       level, a lane per (row, j), no
//                                       flags and no polling
//   wave       trsm_wave_kernel<RP,K>   every other triangle: the sentinel   2: at any level count
//                                       fill + ONE persistent launch
//
// trsm_wave_kernel is sptrsv_wave_kernel (bis_sptrsv.hip: read its header and hazard notes) with the lanes of the wave
// laid out as (slot q, column j) = (lane / K, lane % K) for lane < (64 / K) K:
//   * a wave owns one row at a time, the level-sorted positions are dealt round robin: every wave of the grid must be
//     resident (launch bound (256, 4): at most 4 workgroups per CU, capped by what the runtime reports and device_share);
//   * a trip covers 64 / K entries of the row: lane (q, j) loads val and the dependency's position p of entry q and polls
//     scratch word p*K + j with agent-scope relaxed loads until it is not the sentinel -- readiness travels with the data,
//     per word.  The scratch is kept in level order (n K words): for K = 8 the eight words of a dependency are one 64-byte
//     line, and neighbouring rows of a level are neighbouring lines;
//   * the K chains run in CRS order, one per column: in step t every lane takes (val, x) of lane t K + lane % K through
//     ds_bpermute and applies one fma -- lane l carries the chain of column l % K (the copies are identical); the ready
//     prefix of whole slots is folded while later words are still awaited;
//   * lanes j < K compute (b - acc) / d, publish into the scratch with sc1 stores (never the sentinel pattern, NaN
//     canonicalised) and write X with plain stores (nobody polls X: X may alias B) -- both predicated inside one volatile
//     asm, the wave stays converged around them;
//   * every wait is bounded by kSpinLimit and reads the context's fault word every 1024 trips: a wait that gives up
//     publishes NaN and raises the fault word, the call chain reports BIS_ERR_SYNC.  A lost hand-off ends as an error
//     status, never as a hang.
//
// Algorithmic HBM traffic of a sweep: 12 nnz + rp + 8 (1 + 3 k) n bytes (values and positions; row pointers; D; B, X and
// the scratch published once per row) + 8 k n for the sentinel fill.
#include "bis_internal.hpp"
#include "bis_trsv_level.hpp"

#include <algorithm>
#include <string>

struct bis_trsm_plan {
    int32_t *perm = nullptr;  // device, rows sorted by level
    // the persistent form's, made at its first launch on this side (a triangle that only ever runs the per-level form holds neither):
    int32_t *pcol = nullptr;  // device: position (in perm) of every column; null: the scratch stays in row order (no_pos) or nnz == 0
    double *xs = nullptr;     // device scratch, n * 8 + 8 words, the first n k sentinel-filled before each persistent sweep
    bool no_pos = false;      // a row view whose first non-zero is not 0 (absolute indices into the parent's arrays)
    int n_levels = 0;
    int64_t n = 0;
    int64_t max_level_width = 0;
    std::vector<int64_t> level_ptr; // host: positions of the level boundaries in perm
};

void bis_trsm_plan_destroy(bis_trsm_plan *p) {
    if (!p) return;
    hipFree(p->perm);
    hipFree(p->pcol);
    hipFree(p->xs);
    delete p;
}

namespace {

constexpr int kTrsmT = 256;
constexpr int kTrsmMaxK = 8;
constexpr int kFewLevels = 64;
constexpr int kWaveBlocksPerCU = 4;         // resident workgroups per CU the launch bound guarantees

// (kSentinel, kCanonNaN, kSpinLimit, kFaultPollMask, fault_raised and the position-table kernels: bis_trsv_level.hpp)
__global__ __launch_bounds__(256) void trsm_fill_sentinel_kernel(unsigned long long *xs, int64_t n_words) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += stride) xs[i] = kSentinel;
}

// Few, wide levels: one plain launch per level, a lane per (row, j) -- the kernel boundary is the hand-off.  X may alias B.
template <typename RP, int K>
__global__ __launch_bounds__(256) void trsm_level_kernel(const RP *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                         const double *__restrict__ val, const int32_t *__restrict__ perm,
                                                         int64_t begin, int64_t end, const double *__restrict__ D, const double *B,
                                                         double *X, const int *stop) {
    if (stop && stop[1]) return;
    const int64_t total = (end - begin) * K, stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += stride) {
        const int64_t i = begin + q / K;
        const int j = (int)(q % K);
        const int r = perm[i];
        double acc = 0.0;
        for (int64_t e = (int64_t)row_ptr[r]; e < (int64_t)row_ptr[r + 1]; ++e)
            acc = fma(val[e], X[(int64_t)col[e] * K + j], acc);
        X[(int64_t)r * K + j] = (B[(int64_t)r * K + j] - acc) / D[r];
    }
}

// The persistent form: see the file header.  Lanes of one wave never wait for each other (a wave owns ONE row), so the wait
// loop is an ordinary loop; a wave walks its positions in ascending order and waits only for smaller positions, so by
// induction every position completes PROVIDED all waves of the grid are resident.
template <typename RP, int K>
__global__ __launch_bounds__(kTrsmT, kWaveBlocksPerCU) void trsm_wave_kernel(
    const RP *__restrict__ row_ptr, const int32_t *__restrict__ dep /* positions (pcol), or columns */,
    const double *__restrict__ val, const int32_t *__restrict__ perm, int64_t n, const double *__restrict__ D, const double *B,
    double *X, unsigned long long *xs, int by_pos, unsigned *fault, const int *stop) {
    if (stop && stop[1]) return;
    constexpr int S = 64 / K, ACT = S * K; // slots (= entries of the row) per trip, lanes of the layout
    const int lane = threadIdx.x & 63;
    const int q = lane / K, j = lane % K;  // lanes >= ACT (K does not divide 64) load nothing; they carry a copy of column j's chain
    const int64_t n_waves = (int64_t)gridDim.x * (kTrsmT / 64);
    const int64_t wave0 = (int64_t)blockIdx.x * (kTrsmT / 64) + (threadIdx.x >> 6);
    bool aborted = false; // the sweep has failed (this wave or another gave up): no further waiting
    for (int64_t pos = wave0; pos < n; pos += n_waves) {
        const int r = perm[pos];
        const int64_t s = (int64_t)row_ptr[r], e = (int64_t)row_ptr[r + 1];
        const double rhs = B[(int64_t)r * K + j], d = D[r];
        double acc = 0.0; // lane l: the chain of column l % K
        bool lost = false;
        for (int64_t k0 = s; k0 < e && !lost; k0 += S) {
            const int64_t k = k0 + q;
            const bool active = lane < ACT && k < e;
            const int pc = active ? dep[k] : 0;
            const double av = active ? val[k] : 0.0;
            const unsigned long long *word = xs + ((int64_t)pc * K + j);
            unsigned long long v = active ? __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            const int cnt = (int)(e - k0 < S ? e - k0 : S);
            unsigned spins = 0;
            int folded = 0;
            for (;;) {
                const unsigned long long pend = __ballot(active && v == kSentinel);
                // slots are lane-major: every slot before the first pending lane's is complete in all its K columns
                const int upto = pend ? (int)__builtin_ctzll(pend) / K : cnt;
                const double xv = __longlong_as_double((long long)v);
                for (int t = folded; t < upto; ++t) { // CRS order: slots are consumed strictly left to right
                    const int src = t * K + j;
                    acc = fma(__shfl(av, src, 64), __shfl(xv, src, 64), acc);
                }
                if (upto > folded) folded = upto;
                if (!pend) break;
                ++spins;
                if (!aborted && (spins & kFaultPollMask) == 0u) aborted = __builtin_amdgcn_readfirstlane((int)fault_raised(fault)) != 0;
                if (aborted || spins > kSpinLimit) { // bounded: publishes NaN below and raises the context's fault word
                    lost = true;
                    aborted = true;
                    if (lane == 0) __hip_atomic_fetch_or(fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                if (active && v == kSentinel) v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_s_sleep(1);
            }
        }
        const double res = (rhs - acc) / d;
        unsigned long long out = (unsigned long long)__double_as_longlong(res);
        if (res != res || lost) out = kCanonNaN; // never publish the sentinel pattern
        // Lanes j < K publish -- predicated inside volatile asm, not `if (lane < K)`: a divergent branch at the tail of
        // the position loop lets the compiler send the other lanes into the next trip without them (bis_sptrsv.hip).
        {
            unsigned long long *dst = xs + ((by_pos ? pos : (int64_t)r) * K + j);
            unsigned long long *dx = reinterpret_cast<unsigned long long *>(X + ((int64_t)r * K + j));
            const unsigned pflag = lane < K ? 1u : 0u;
            unsigned long long saved_exec;
            asm volatile("v_cmp_ne_u32_e32 vcc, 0, %4\n\ts_and_saveexec_b64 %0, vcc\n\t"
                         "global_store_dwordx2 %1, %3, off sc1\n\tglobal_store_dwordx2 %2, %3, off\n\t"
                         "s_mov_b64 exec, %0"
                         : "=&s"(saved_exec) : "v"(dst), "v"(dx), "v"(out), "v"(pflag) : "vcc", "memory");
        }
    }
}

// The multi-vector plan of this side, built at the first call: the level analysis on the device (which is also the
// structure check).
bis_status trsm_get_plan(bis_ctx *ctx, const bis_mat *T, bool backward, bis_trsm_plan **out) {
    bis_trsm_plan *&slot = bis_trsv_side_of(const_cast<bis_mat *>(T), backward).multi;
    if (slot) { *out = slot; return BIS_OK; }
    const int64_t n = T->n_rows;
    bis_trsm_plan *p = new bis_trsm_plan;
    p->n = n;
    auto fail = [&](bis_status st) { bis_trsm_plan_destroy(p); return st; };
    const hipError_t e = hipMalloc(&p->perm, sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = std::string("sptrsm plan: ") + hipGetErrorString(e);
        return fail(BIS_ERR_HIP);
    }
    bool triangular = true;
    bis_status st = bis_trsv_analyse_device(ctx, T, backward, p->perm, p->level_ptr, p->n_levels, p->max_level_width, triangular);
    if (st == BIS_OK && !triangular) {
        ctx->err = backward ? "bis_bsptrsm: matrix is not strictly upper triangular" : "bis_sptrsm: matrix is not strictly lower triangular";
        st = BIS_ERR_INVALID;
    }
    if (st != BIS_OK) return fail(st);
    slot = p;
    *out = p;
    return BIS_OK;
}

// What only the persistent form needs, at its first launch on this side: the scratch and the position table.  A failure
// leaves the plan as it was (the next call tries again).
bis_status trsm_ensure_scratch(bis_ctx *ctx, const bis_mat *T, bis_trsm_plan *p) {
    const int64_t n = T->n_rows;
    if (!p->xs) {
        const hipError_t e = hipMalloc(&p->xs, sizeof(double) * ((size_t)n * kTrsmMaxK + 8));
        if (e != hipSuccess) { (void)hipGetLastError(); p->xs = nullptr; ctx->err = "sptrsm: out of memory for the scratch block"; return BIS_ERR_HIP; }
    }
    if (p->pcol || p->no_pos || T->nnz <= 0) return BIS_OK;
    // the view's first non-zero: row views share the parent's arrays (absolute indices: they keep the row-order scratch)
    int64_t a64 = 0;
    int32_t a32 = 0;
    hipError_t e = hipMemcpyAsync(T->rp64 ? (void *)&a64 : (void *)&a32, T->row_ptr, T->rp64 ? 8 : 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("sptrsm plan: ") + hipGetErrorString(e); return BIS_ERR_HIP; }
    if ((T->rp64 ? a64 : (int64_t)a32) != 0) { p->no_pos = true; return BIS_OK; }
    int32_t *inv = nullptr, *pcol = nullptr;
    e = hipMalloc(&inv, sizeof(int32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&pcol, sizeof(int32_t) * (size_t)T->nnz);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hipFree(inv);
        ctx->err = "sptrsm: out of memory for the position table";
        return BIS_ERR_HIP;
    }
    hipLaunchKernelGGL(invert_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p->perm, n, inv);
    hipLaunchKernelGGL(cols_to_positions_kernel, dim3((unsigned)std::min<int64_t>((T->nnz + 255) / 256, 8192)), dim3(256), 0,
                       ctx->stream, T->col, inv, T->nnz, pcol);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(inv);
    if (e != hipSuccess) { hipFree(pcol); ctx->err = std::string("sptrsm plan: ") + hipGetErrorString(e); return BIS_ERR_HIP; }
    p->pcol = pcol;
    return BIS_OK;
}

// static names: one per (form, K, RP)
const char *trsm_name(bool wave, int k, bool rp64) {
    static std::string names[2][kTrsmMaxK + 1][2];
    std::string &s = names[wave][k][rp64];
    if (s.empty()) s = std::string(wave ? "trsm_wave_kernel K=" : "trsm_level_kernel K=") + std::to_string(k) + " RP=" + (rp64 ? "64" : "32");
    return s.c_str();
}

template <typename RP, int K>
void launch_level(bis_ctx *ctx, const bis_mat *T, const bis_trsm_plan *p, double *X, const double *D, const double *B) {
    for (int l = 0; l < p->n_levels; ++l) {
        const int64_t lo = p->level_ptr[l], hi = p->level_ptr[l + 1];
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(((hi - lo) * K + 255) / 256, (int64_t)ctx->n_cus * 32));
        hipLaunchKernelGGL((trsm_level_kernel<RP, K>), dim3(grid), dim3(256), 0, ctx->stream, (const RP *)T->row_ptr, T->col, T->val,
                           p->perm, lo, hi, D, B, X, ctx->spmv_stop);
    }
}

// workgroups per CU of the persistent grid: what the runtime reports resident for this instance, at most the 4 the launch
// bound guarantees -- progress needs every wave of the grid resident
template <typename RP, int K>
int wave_resident() {
    static int res = 0;
    if (res == 0) {
        int nb = 0;
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, trsm_wave_kernel<RP, K>, kTrsmT, 0);
        res = (oe == hipSuccess && nb > 0) ? std::min(nb, kWaveBlocksPerCU) : 1;
        (void)hipGetLastError();
    }
    return res;
}

template <typename RP, int K>
void launch_wave(bis_ctx *ctx, const bis_mat *T, const bis_trsm_plan *p, double *X, const double *D, const double *B) {
    const int64_t n = T->n_rows;
    const int fill_grid = (int)std::max<int64_t>(1, std::min<int64_t>((n * K + 255) / 256, 2048));
    hipLaunchKernelGGL(trsm_fill_sentinel_kernel, dim3(fill_grid), dim3(256), 0, ctx->stream, (unsigned long long *)p->xs, n * K);
    // a few levels of rows in flight, one row per wave; device_share = s: s processes keep persistent grids on this device,
    // each keeps to 1 / s of the residency
    const int share = std::max(1, bis_opts().device_share);
    const int64_t wg = (4 * p->max_level_width + 3) / 4 + 1;
    const int64_t cap = std::max<int64_t>(1, (int64_t)ctx->n_cus * wave_resident<RP, K>() / share);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(wg, std::min<int64_t>((n + 3) / 4, cap)));
    hipLaunchKernelGGL((trsm_wave_kernel<RP, K>), dim3((unsigned)grid), dim3(kTrsmT), 0, ctx->stream, (const RP *)T->row_ptr,
                       p->pcol ? p->pcol : T->col, T->val, p->perm, n, D, B, X, (unsigned long long *)p->xs, p->pcol ? 1 : 0,
                       ctx->fault_dev, ctx->spmv_stop);
}

template <typename RP>
void launch_k(bis_ctx *ctx, const bis_mat *T, const bis_trsm_plan *p, bool wave, int k, double *X, const double *D, const double *B) {
#define BIS_TRSM_CASE(K) case K: if (wave) launch_wave<RP, K>(ctx, T, p, X, D, B); else launch_level<RP, K>(ctx, T, p, X, D, B); break;
    switch (k) {
    BIS_TRSM_CASE(2) BIS_TRSM_CASE(3) BIS_TRSM_CASE(4) BIS_TRSM_CASE(5) BIS_TRSM_CASE(6) BIS_TRSM_CASE(7)
    default: if (wave) launch_wave<RP, 8>(ctx, T, p, X, D, B); else launch_level<RP, 8>(ctx, T, p, X, D, B); break;
    }
#undef BIS_TRSM_CASE
}

bis_status trsm_solve(bis_ctx *ctx, const bis_mat *T, bool backward, double *X, const double *D, const double *B, int k) {
    BIS_CTX_OK(ctx);
    const char *who = backward ? "bis_bsptrsm" : "bis_sptrsm";
    BIS_REQUIRE(ctx, k >= 1 && k <= kTrsmMaxK, std::string(who) + ": n_rhs must be between 1 and 8");
    BIS_REQUIRE(ctx, T && (T->n_rows == 0 || (X && D && B)), std::string(who) + ": bad arguments");
    BIS_REQUIRE(ctx, T->n_rows == T->n_cols, std::string(who) + ": square matrix required");
    if (T->n_rows == 0) return BIS_OK;
    bis_trsv_side &side = bis_trsv_side_of(const_cast<bis_mat *>(T), backward);
    if (k == 1) {
        const bis_status st = backward ? bis_bsptrsv(ctx, T, X, D, B) : bis_sptrsv(ctx, T, X, D, B);
        if (st == BIS_OK) side.kernel_m = backward ? "bis_bsptrsv K=1" : "bis_sptrsv K=1";
        return st;
    }
    bis_trsm_plan *p = nullptr;
    if (bis_status st = trsm_get_plan(ctx, T, backward, &p)) return st;
    const int form = bis_opts().trsm_form;
    const bool wave = form == 2 || (form != 1 && p->n_levels > kFewLevels);
    if (wave)
        if (bis_status st = trsm_ensure_scratch(ctx, T, p)) return st;
    if (T->rp64) launch_k<int64_t>(ctx, T, p, wave, k, X, D, B);
    else launch_k<int32_t>(ctx, T, p, wave, k, X, D, B);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    side.kernel_m = trsm_name(wave, k, T->rp64);
    return BIS_OK;
}

} // namespace

extern "C" {

const char *bis_mat_sweepm_kernel(const bis_mat *T, int backward) { return T ? T->trsv[backward ? 1 : 0].kernel_m : ""; }

bis_status bis_sptrsm(bis_ctx *ctx, const bis_mat *L_strict, double *X, const double *D, const double *B, int n_rhs) {
    return trsm_solve(ctx, L_strict, false, X, D, B, n_rhs);
}

bis_status bis_bsptrsm(bis_ctx *ctx, const bis_mat *U_strict, double *X, const double *D, const double *B, int n_rhs) {
    return trsm_solve(ctx, U_strict, true, X, D, B, n_rhs);
}

} // extern "C"
