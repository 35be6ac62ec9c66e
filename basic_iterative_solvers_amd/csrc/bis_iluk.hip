// bis_iluk.hip -- ILU(k) with level-of-fill: the symbolic phase and the assembly of the padded matrix; not in the reference.
// The numeric phase is bis_ilu0.hip's elimination with its non-zero rule switched off (bis_mat_ilu0_impl, fill = true).
//
// Definition (include/bis_hip.h): lev(i,j) = 0 on A's pattern, otherwise the minimum over pivots p < min(i,j) of
// lev(i,p) + lev(p,j) + 1; P keeps the positions with lev <= k.  By the fill-path theorem (Hysom & Pothen) lev(i,j) = l
// exactly when the shortest path i -> j in the graph of A whose interior vertices are all < min(i,j) has l + 1 edges.
// For j > i the interior vertices are < i: a breadth-first search from i that only continues through vertices < i, to
// depth k + 1, finds the upper part of row i.  For j < i they are < j: the same search from j in the graph of A^T finds
// column j of the lower part, and the result is transposed.
//
// The rows are independent: ONE WAVE PER ROW (a workgroup of one wave), no levels, no flags, nothing waits.  The visited
// set is an open-addressing table of kIlukSlots words in LDS, claimed with LDS compare-and-swap (the first claimant wins;
// all claimants of a round have the same depth, so the SET does not depend on who wins); the visited vertices also go to
// a queue in LDS in order of discovery, whose last segment is the next frontier.  Four frontier vertices are expanded
// at a time, 16 lanes over the row of each.  Two passes of the same search: count, prefix sum, fill; a row's results leave
// in ascending order (rank sort over the queue), so the output does not depend on the claim order either.
// Every loop is bounded by a row length, the queue length or the table size.  A row that visits more than kIlukMaxVisit
// vertices makes the call fail; nothing is truncated.
#include "bis_internal.hpp"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int kIlukMaxLevel = 16;
constexpr int kIlukMaxVisit = 4096; // vertices a row's search may visit, the row itself not counted
constexpr int kIlukSlots = 8192;    // the table: twice that, so a probe sequence always ends at an empty slot
constexpr int kIlukT = 256;
// aux words (device, unsigned long long)
enum { KA_STATUS, KA_OVERFLOW_ROW, KA_TOTAL, KA_COUNT };
enum { KS_NO_DIAG = 1, KS_DUP = 2 };

__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned iluk_hash(int32_t v) { return ((unsigned)v * 2654435761u) >> 19; } // 13 bits

// the checks on the sorted copy: a row without a stored diagonal, a column repeated inside a row
template <typename RP>
__global__ __launch_bounds__(kIlukT) void iluk_check_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ wcol,
                                                            const int64_t *__restrict__ dpos, int64_t n, unsigned long long *aux) {
    const int64_t i = (int64_t)blockIdx.x * kIlukT + threadIdx.x;
    if (i >= n) return;
    unsigned status = dpos[i] < 0 ? KS_NO_DIAG : 0;
    for (int64_t p = (int64_t)rp[i] + 1; p < (int64_t)rp[i + 1]; ++p)
        if (wcol[p] == wcol[p - 1]) status |= KS_DUP;
    if (status) atomicOr(&aux[KA_STATUS], (unsigned long long)status);
}

// ---- exclusive prefix sum of n int32 counts into n + 1 int64 offsets: block sums, their scan, the offsets ----------------
__global__ __launch_bounds__(kIlukT) void iluk_blocksum_kernel(const int32_t *__restrict__ cnt, int64_t n, int64_t *blk) {
    __shared__ int64_t s[kIlukT];
    const int64_t i = (int64_t)blockIdx.x * kIlukT + threadIdx.x;
    s[threadIdx.x] = i < n ? (int64_t)cnt[i] : 0;
    __syncthreads();
    for (int off = kIlukT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void iluk_scan_blocks_kernel(int64_t *blk, int n_blk, unsigned long long *aux) {
    __shared__ int64_t s[256];
    int64_t run = 0;
    for (int base = 0; base < n_blk; base += 256) {
        const int i = base + threadIdx.x;
        const int64_t v = i < n_blk ? blk[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int64_t a = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < n_blk) blk[i] = run + s[threadIdx.x] - v;
        run += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) aux[KA_TOTAL] = (unsigned long long)run;
}

__global__ __launch_bounds__(kIlukT) void iluk_offsets_kernel(const int32_t *__restrict__ cnt, int64_t n, const int64_t *__restrict__ blk,
                                                              int64_t *ptr) {
    __shared__ int64_t s[kIlukT];
    const int64_t i = (int64_t)blockIdx.x * kIlukT + threadIdx.x;
    const int64_t c = i < n ? (int64_t)cnt[i] : 0;
    s[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < kIlukT; off <<= 1) {
        const int64_t a = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += a;
        __syncthreads();
    }
    if (i < n) {
        const int64_t at = blk[blockIdx.x] + s[threadIdx.x] - c;
        ptr[i] = at;
        if (i == n - 1) ptr[n] = at + c;
    }
}

// ---- the transpose of a pattern: entries per column, then every entry takes a place in its column's range (integer atomics:
// the order inside a transposed row is arbitrary; the search does not depend on it and the assembly sorts) -------------------
template <typename RP>
__global__ __launch_bounds__(kIlukT) void iluk_colcount_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, int64_t n,
                                                               int32_t *cnt) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (kIlukT / 64) + wave; i < n; i += (int64_t)gridDim.x * (kIlukT / 64))
        for (int64_t p = (int64_t)rp[i] + lane; p < (int64_t)rp[i + 1]; p += 64) atomicAdd(&cnt[col[p]], 1);
}

template <typename RP>
__global__ __launch_bounds__(kIlukT) void iluk_scatter_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, int64_t n,
                                                              const int64_t *__restrict__ ptrT, int32_t *cursor, int32_t *__restrict__ colT) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (kIlukT / 64) + wave; i < n; i += (int64_t)gridDim.x * (kIlukT / 64))
        for (int64_t p = (int64_t)rp[i] + lane; p < (int64_t)rp[i + 1]; p += 64) {
            const int32_t c = col[p];
            colT[ptrT[c] + atomicAdd(&cursor[c], 1)] = (int32_t)i;
        }
}

// ---- the search (see the head of the file).  out_ptr == nullptr: count pass, cnt[i] = results of row i; otherwise the
// results of row i go to out_col[out_ptr[i] ...] in ascending order.  (rp, col) is the graph: A, or the transposed pattern.
template <typename RP>
__global__ __launch_bounds__(64) void iluk_search_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col, int64_t n, int level,
                                                         const int64_t *__restrict__ out_ptr, int32_t *__restrict__ out_col,
                                                         int32_t *__restrict__ cnt, unsigned long long *aux) {
    __shared__ int32_t tab[kIlukSlots];
    __shared__ int32_t queue[kIlukMaxVisit + 1]; // queue[0] is the row itself
    __shared__ int qn;
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        for (int s = lane; s < kIlukSlots; s += 64) tab[s] = -1;
        wave_lds_sync();
        if (lane == 0) {
            tab[iluk_hash((int32_t)i)] = (int32_t)i;
            queue[0] = (int32_t)i;
            qn = 1;
        }
        wave_lds_sync();
        int seg_b = 0, seg_e = 1; // the frontier: what the previous round discovered
        bool overflow = false;
        for (int d = 0; d <= level && seg_b < seg_e && !overflow; ++d) { // round d discovers the vertices of depth d + 1 <= k + 1
            for (int f0 = seg_b; f0 < seg_e; f0 += 4) {
                const int f = f0 + (lane >> 4);
                const int32_t v = f < seg_e ? queue[f] : INT32_MAX;
                if ((int64_t)v <= i) { // a vertex above i is a result: the search does not continue through it
                    const int64_t e = (int64_t)rp[v + 1];
                    for (int64_t p = (int64_t)rp[v] + (lane & 15); p < e; p += 16) {
                        const int32_t t = col[p];
                        unsigned h = iluk_hash(t);
                        for (int probe = 0; probe < kIlukSlots; ++probe) {
                            const int32_t old = atomicCAS(&tab[h], -1, t);
                            if (old == -1) { // claimed: newly seen
                                const int at = atomicAdd(&qn, 1);
                                if (at <= kIlukMaxVisit) queue[at] = t;
                                break;
                            }
                            if (old == t) break;
                            h = (h + 1) & (kIlukSlots - 1);
                        }
                    }
                }
                wave_lds_sync();
                // at most 64 claims per step: the table (8192 slots) never holds more than 4097 + 64 vertices
                if (*(volatile int *)&qn > kIlukMaxVisit + 1) { overflow = true; break; }
            }
            seg_b = seg_e;
            seg_e = min(*(volatile int *)&qn, kIlukMaxVisit + 1);
        }
        if (overflow) {
            if (lane == 0) {
                atomicMin(&aux[KA_OVERFLOW_ROW], (unsigned long long)i);
                if (!out_ptr) cnt[i] = 0;
            }
        } else if (!out_ptr) {
            int c = 0;
            for (int a0 = 0; a0 < seg_e; a0 += 64) {
                const int a = a0 + lane;
                c += __popcll(__ballot(a < seg_e && (int64_t)queue[a] > i));
            }
            if (lane == 0) cnt[i] = c;
        } else {
            const int64_t o = out_ptr[i];
            for (int a = lane; a < seg_e; a += 64) {
                const int32_t key = queue[a];
                if ((int64_t)key <= i) continue;
                int rank = 0;
                for (int b = 0; b < seg_e; ++b) {
                    const int32_t kb = queue[b];
                    rank += ((int64_t)kb > i) & (kb < key);
                }
                out_col[o + rank] = key;
            }
        }
        wave_lds_sync(); // table and queue are rewritten for the next row
    }
}

// ---- P = lower results (transposed, any order: ranked here) + the diagonal + upper results (ascending); A's value where
// A has the position, +0.0 at a fill position.  A wave per row; rpP[i] = ptrL[i] + ptrU[i] + i.
template <typename RP, typename RPP>
__global__ __launch_bounds__(kIlukT) void iluk_assemble_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ wcol,
                                                               const double *__restrict__ wval, int64_t n,
                                                               const int64_t *__restrict__ ptrL, const int32_t *__restrict__ colL,
                                                               const int64_t *__restrict__ ptrU, const int32_t *__restrict__ colU,
                                                               RPP *__restrict__ rpP, int32_t *__restrict__ colP, double *__restrict__ valP) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (kIlukT / 64) + wave; i < n; i += (int64_t)gridDim.x * (kIlukT / 64)) {
        const int64_t sL = ptrL[i], nl = ptrL[i + 1] - sL, sU = ptrU[i], nu = ptrU[i + 1] - sU;
        const int64_t base = sL + sU + i, total = nl + 1 + nu;
        if (lane == 0) {
            rpP[i] = (RPP)base;
            if (i == n - 1) rpP[n] = (RPP)(base + total);
        }
        const int64_t ws = rp[i], we = rp[i + 1];
        for (int64_t q = lane; q < total; q += 64) {
            int32_t c;
            int64_t at;
            if (q < nl) {
                c = colL[sL + q];
                int64_t rank = 0;
                for (int64_t b = 0; b < nl; ++b) rank += colL[sL + b] < c;
                at = base + rank;
            } else if (q == nl) {
                c = (int32_t)i;
                at = base + nl;
            } else {
                c = colU[sU + (q - nl - 1)];
                at = base + q;
            }
            int64_t lo = ws, hi = we;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (wcol[mid] < c) lo = mid + 1; else hi = mid;
            }
            colP[at] = c;
            valP[at] = (lo < we && wcol[lo] == c) ? wval[lo] : 0.0;
        }
    }
}

const char *iluk_kernel_name(bool rp64, bool symmetric) {
    if (symmetric) return rp64 ? "iluk_search_kernel RP=64 one search, transposed" : "iluk_search_kernel RP=32 one search, transposed";
    return rp64 ? "iluk_search_kernel RP=64 two searches" : "iluk_search_kernel RP=32 two searches";
}

template <typename RP>
bis_status iluk_symbolic_t(bis_ctx *ctx, const bis_mat *A, int level, bis_mat **P_out, int64_t *n_fill) {
    const int64_t n = A->n_rows;
    const int n_blk = (int)((n + kIlukT - 1) / kIlukT);
    bis_mat *W = nullptr, *P = nullptr;
    int64_t *dpos = nullptr, *ustart = nullptr;
    std::vector<void *> owned;
    auto cleanup = [&](bis_status rc) {
        hipFree(dpos);
        hipFree(ustart);
        for (void *p : owned) hipFree(p);
        if (W) bis_mat_destroy(ctx, W);
        if (rc != BIS_OK && P) bis_mat_destroy(ctx, P);
        return rc;
    };
    auto hip_fail = [&](hipError_t e) {
        ctx->err = std::string("bis_mat_iluk: ") + hipGetErrorString(e);
        return cleanup(BIS_ERR_HIP);
    };
    hipError_t e = hipSuccess;
    auto dmalloc = [&](size_t bytes) -> void * {
        void *p = nullptr;
        if (e == hipSuccess) e = hipMalloc(&p, std::max<size_t>(bytes, 8));
        if (p) owned.push_back(p);
        return p;
    };
    bis_status st = bis_mat_sorted_copy(ctx, A, &W, &dpos, &ustart);
    if (st != BIS_OK) return st;
    unsigned long long *aux = (unsigned long long *)dmalloc(sizeof(unsigned long long) * KA_COUNT);
    int64_t *blk = (int64_t *)dmalloc(sizeof(int64_t) * (size_t)n_blk);
    int32_t *cnt = (int32_t *)dmalloc(sizeof(int32_t) * (size_t)n);
    int64_t *ptrU = (int64_t *)dmalloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t *ptrL = (int64_t *)dmalloc(sizeof(int64_t) * (size_t)(n + 1));
    if (e != hipSuccess) return hip_fail(e);
    unsigned long long h_aux[KA_COUNT] = {0, ~0ull, 0};
    e = hipMemcpyAsync(aux, h_aux, sizeof h_aux, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    const RP *rp = (const RP *)W->row_ptr;
    hipLaunchKernelGGL(iluk_check_kernel<RP>, dim3(n_blk), dim3(kIlukT), 0, ctx->stream, rp, W->col, dpos, n, aux);
    auto read_aux = [&]() {
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipMemcpyAsync(h_aux, aux, sizeof h_aux, hipMemcpyDeviceToHost, ctx->stream);
        if (r == hipSuccess) r = hipStreamSynchronize(ctx->stream);
        return r;
    };
    if ((e = read_aux()) != hipSuccess) return hip_fail(e);
    if (h_aux[KA_STATUS] & KS_NO_DIAG) {
        ctx->err = "bis_mat_iluk: a row without a stored diagonal entry";
        return cleanup(BIS_ERR_NO_DIAG);
    }
    if (h_aux[KA_STATUS] & KS_DUP) {
        ctx->err = "bis_mat_iluk: a column repeated inside a row";
        return cleanup(BIS_ERR_UNSUPPORTED);
    }
    bool symmetric = false;
    st = bis_mat_pattern_symmetric(ctx, A, &symmetric);
    if (st != BIS_OK) return cleanup(st);

    // grid-stride over the rows everywhere: any n stays below HIP's 2^32 threads per launch
    const dim3 grid_w((unsigned)std::min<int64_t>((n + 3) / 4, 1 << 22)), grid_s((unsigned)std::min<int64_t>(n, 1 << 20));
    // ptr[0..n] = exclusive prefix sums of cnt[0..n); *total = their sum.  Blocking (reads the total).
    auto scan = [&](int64_t *ptr, int64_t *total) {
        hipLaunchKernelGGL(iluk_blocksum_kernel, dim3(n_blk), dim3(kIlukT), 0, ctx->stream, cnt, n, blk);
        hipLaunchKernelGGL(iluk_scan_blocks_kernel, dim3(1), dim3(256), 0, ctx->stream, blk, n_blk, aux);
        hipLaunchKernelGGL(iluk_offsets_kernel, dim3(n_blk), dim3(kIlukT), 0, ctx->stream, cnt, n, blk, ptr);
        const hipError_t r = read_aux();
        *total = (int64_t)h_aux[KA_TOTAL];
        return r;
    };
    auto overflowed = [&]() {
        if (h_aux[KA_OVERFLOW_ROW] == ~0ull) return false;
        ctx->err = "bis_mat_iluk: the level-" + std::to_string(level) + " search of row " + std::to_string(h_aux[KA_OVERFLOW_ROW]) +
                   (symmetric ? "" : " (of A or of its transpose)") + " visits more than " + std::to_string(kIlukMaxVisit) + " vertices";
        return true;
    };
    // the transpose of the pattern (gp, gcol) with n rows: offsets to ptr, columns to a new array
    auto transpose = [&](auto *gp, const int32_t *gcol, int64_t *ptr, int32_t **colT) {
        int64_t total = 0;
        hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n, ctx->stream);
        hipLaunchKernelGGL((iluk_colcount_kernel<std::remove_cv_t<std::remove_pointer_t<decltype(gp)>>>), grid_w, dim3(kIlukT), 0, ctx->stream, gp,
                           gcol, n, cnt);
        hipError_t r = scan(ptr, &total);
        if (r != hipSuccess) return r;
        *colT = (int32_t *)dmalloc(sizeof(int32_t) * (size_t)total);
        if (e != hipSuccess) return e;
        hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n, ctx->stream);
        hipLaunchKernelGGL((iluk_scatter_kernel<std::remove_cv_t<std::remove_pointer_t<decltype(gp)>>>), grid_w, dim3(kIlukT), 0, ctx->stream, gp,
                           gcol, n, ptr, cnt, *colT);
        return hipGetLastError();
    };

    // upper parts: the search on A
    int64_t nnzU = 0, nnzL = 0;
    hipLaunchKernelGGL(iluk_search_kernel<RP>, grid_s, dim3(64), 0, ctx->stream, rp, W->col, n, level, (const int64_t *)nullptr,
                       (int32_t *)nullptr, cnt, aux);
    if ((e = scan(ptrU, &nnzU)) != hipSuccess) return hip_fail(e);
    if (overflowed()) return cleanup(BIS_ERR_UNSUPPORTED);
    int32_t *colU = (int32_t *)dmalloc(sizeof(int32_t) * (size_t)nnzU);
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(iluk_search_kernel<RP>, grid_s, dim3(64), 0, ctx->stream, rp, W->col, n, level, (const int64_t *)ptrU, colU,
                       (int32_t *)nullptr, aux);
    // lower parts: the search on A^T (its upper results are the columns of the lower part), or the first result again
    // where the pattern is structurally symmetric; transposed into rows
    int32_t *colL = nullptr;
    if (symmetric) {
        if ((e = transpose((const int64_t *)ptrU, colU, ptrL, &colL)) != hipSuccess) return hip_fail(e);
        nnzL = nnzU;
    } else {
        int64_t *ptrT = (int64_t *)dmalloc(sizeof(int64_t) * (size_t)(n + 1)), *ptrV = (int64_t *)dmalloc(sizeof(int64_t) * (size_t)(n + 1));
        int32_t *colT = nullptr;
        if (e != hipSuccess) return hip_fail(e);
        if ((e = transpose(rp, W->col, ptrT, &colT)) != hipSuccess) return hip_fail(e);
        hipLaunchKernelGGL(iluk_search_kernel<int64_t>, grid_s, dim3(64), 0, ctx->stream, (const int64_t *)ptrT, colT, n, level,
                           (const int64_t *)nullptr, (int32_t *)nullptr, cnt, aux);
        if ((e = scan(ptrV, &nnzL)) != hipSuccess) return hip_fail(e);
        if (overflowed()) return cleanup(BIS_ERR_UNSUPPORTED);
        int32_t *colV = (int32_t *)dmalloc(sizeof(int32_t) * (size_t)nnzL);
        if (e != hipSuccess) return hip_fail(e);
        hipLaunchKernelGGL(iluk_search_kernel<int64_t>, grid_s, dim3(64), 0, ctx->stream, (const int64_t *)ptrT, colT, n, level,
                           (const int64_t *)ptrV, colV, (int32_t *)nullptr, aux);
        if ((e = transpose((const int64_t *)ptrV, colV, ptrL, &colL)) != hipSuccess) return hip_fail(e);
    }
    const int64_t nnzP = nnzL + n + nnzU;
    const bool p64 = A->rp64 || bis_want_rp64(nnzP);
    st = bis_mat_alloc(ctx, n, n, nnzP, p64, &P); // (no grid hint: the filled triangles are not stencils)
    if (st != BIS_OK) return cleanup(st);
    if (p64)
        hipLaunchKernelGGL((iluk_assemble_kernel<RP, int64_t>), grid_w, dim3(kIlukT), 0, ctx->stream, rp, W->col, W->val, n, ptrL, colL, ptrU,
                           colU, (int64_t *)P->row_ptr, P->col, P->val);
    else
        hipLaunchKernelGGL((iluk_assemble_kernel<RP, int32_t>), grid_w, dim3(kIlukT), 0, ctx->stream, rp, W->col, W->val, n, ptrL, colL, ptrU,
                           colU, (int32_t *)P->row_ptr, P->col, P->val);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    st = bis_mat_finalize(ctx, P);
    if (st != BIS_OK) return cleanup(st);
    P->iluk_kernel = iluk_kernel_name(A->rp64, symmetric);
    *P_out = P;
    *n_fill = nnzP - A->nnz;
    return cleanup(BIS_OK);
}

// n = 0: a matrix without rows
bis_status iluk_empty(bis_ctx *ctx, const bis_mat *A, bis_mat **P_out) {
    bis_mat *P = nullptr;
    bis_status st = bis_mat_alloc(ctx, 0, 0, 0, A->rp64, &P);
    if (st != BIS_OK) return st;
    hipError_t e = hipMemsetAsync(P->row_ptr, 0, A->rp64 ? sizeof(int64_t) : sizeof(int32_t), ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string("bis_mat_iluk: ") + hipGetErrorString(e);
        bis_mat_destroy(ctx, P);
        return BIS_ERR_HIP;
    }
    st = bis_mat_finalize(ctx, P);
    if (st != BIS_OK) { bis_mat_destroy(ctx, P); return st; }
    *P_out = P;
    return BIS_OK;
}

bis_status iluk_symbolic(bis_ctx *ctx, const bis_mat *A, int level, bis_mat **P, int64_t *n_fill) {
    if (A->n_rows == 0) {
        *n_fill = 0;
        return iluk_empty(ctx, A, P);
    }
    return A->rp64 ? iluk_symbolic_t<int64_t>(ctx, A, level, P, n_fill) : iluk_symbolic_t<int32_t>(ctx, A, level, P, n_fill);
}

} // namespace

extern "C" {

const char *bis_mat_iluk_kernel(const bis_mat *L_strict) { return L_strict ? L_strict->iluk_kernel : ""; }

bis_status bis_iluk_limits(int *max_level, int *max_visit) {
    if (max_level) *max_level = kIlukMaxLevel;
    if (max_visit) *max_visit = kIlukMaxVisit;
    return BIS_OK;
}

bis_status bis_mat_iluk_symbolic(bis_ctx *ctx, const bis_mat *A, int level, bis_mat **P, int64_t *n_fill) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && P, "bis_mat_iluk_symbolic: bad arguments");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mat_iluk_symbolic: square matrix required");
    BIS_REQUIRE(ctx, !A->view, "bis_mat_iluk_symbolic: a row-range view has no diagonal block of its own");
    BIS_REQUIRE(ctx, level >= 0 && level <= kIlukMaxLevel, "bis_mat_iluk_symbolic: level outside 0..16");
    bis_mat *Pm = nullptr;
    int64_t fill = 0;
    const bis_status st = iluk_symbolic(ctx, A, level, &Pm, &fill);
    if (st != BIS_OK) return st;
    *P = Pm;
    if (n_fill) *n_fill = fill;
    return BIS_OK;
}

bis_status bis_mat_iluk(bis_ctx *ctx, const bis_mat *A, int level, double pivot_tol, double pivot_repl, bis_mat **L_strict,
                        bis_mat **U_strict, double *L_D, double *U_D, int64_t *n_fill) {
    BIS_CTX_OK(ctx);
    if (level == 0) { // IS bis_mat_ilu0: its checks, its non-zero rule, its grid hint, its kernel
        const bis_status st = bis_mat_ilu0(ctx, A, pivot_tol, pivot_repl, L_strict, U_strict, L_D, U_D);
        if (st == BIS_OK && n_fill) *n_fill = 0;
        return st;
    }
    BIS_REQUIRE(ctx, A && L_strict && U_strict && L_D && U_D, "bis_mat_iluk: bad arguments");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_mat_iluk: square matrix required");
    BIS_REQUIRE(ctx, !A->view, "bis_mat_iluk: a row-range view has no diagonal block of its own");
    BIS_REQUIRE(ctx, level >= 1 && level <= kIlukMaxLevel, "bis_mat_iluk: level outside 0..16");
    if (A->n_rows == 0) { // nothing to fill
        const bis_status st = bis_mat_ilu0(ctx, A, pivot_tol, pivot_repl, L_strict, U_strict, L_D, U_D);
        if (st == BIS_OK && n_fill) *n_fill = 0;
        return st;
    }
    bis_mat *P = nullptr, *Ls = nullptr, *Us = nullptr;
    int64_t fill = 0;
    bis_status st = iluk_symbolic(ctx, A, level, &P, &fill);
    if (st != BIS_OK) return st;
    st = bis_mat_ilu0_impl(ctx, P, pivot_tol, pivot_repl, &Ls, &Us, L_D, U_D, true);
    if (st == BIS_OK) { // blocking, like the symbolic phase
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "bis_mat_iluk: synchronisation failed"; st = BIS_ERR_HIP; }
        else if (bis_status fs = bis_fault_check(ctx)) st = fs;
    }
    if (st == BIS_OK) Ls->iluk_kernel = P->iluk_kernel;
    bis_mat_destroy(ctx, P);
    if (st != BIS_OK) {
        if (Ls) bis_mat_destroy(ctx, Ls);
        if (Us) bis_mat_destroy(ctx, Us);
        return st;
    }
    *L_strict = Ls;
    *U_strict = Us;
    if (n_fill) *n_fill = fill;
    return BIS_OK;
}

} // extern "C"
