// bis_spgemm.hip -- sparse matrix-matrix product C = A B and the transpose, on the device; not in the reference.  The
// definitions a restatement needs are in include/bis_hip.h; this file follows them step by step.
//
// bis_spgemm.  One counting pass gives every row its upper bound u_i = sum over the entries (i, j) of A of nnz(B_j), and
// another looks whether the rows of B ascend strictly.  A row takes one of two paths that give the same bits:
//   row path (spgemm_row_kernel): a workgroup owns a row of C -- one wave for u_i <= 256, four waves up to spgemm_row_cap.
//     It gathers the candidate columns into LDS, sorts them there (bitonic, padded to a power of two) and keeps the first
//     of every run.  The symbolic launch stores the count; after the scan of the counts the numeric launch repeats the
//     sort and gives every output entry to a lane, which walks A's row in CRS order and looks its column up in B's row by
//     bisection (hence: ascending B only).  LDS: 4 bytes per candidate, 16 KiB + 1 KiB at the largest cap of 4096 -- eight
//     workgroups of 256 threads, the most a CU holds, fit the 160 KiB.
//   fallback (spgemm_sort_fallback): whole rows in batches of at most spgemm_batch products: expand (row << 32 | column,
//     product) in enumeration order, a stable 64-bit radix sort, head flags, a scan, one lane per run sums it left to
//     right.  It also runs twice (counts, then values); its temporaries are 48 bytes per product of ONE batch.
// No floating-point atomics, no inter-workgroup waits; the integer atomics only count.
//
// bis_mat_transpose.  A stable radix sort of the entry numbers by column, then a gather: the order inside a row of A^T is
// the CRS order of A whatever the schedule.
#include "bis_internal.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>

namespace {

constexpr int kSpgT = 256;
constexpr int kSpgMaxBlocks = 16384;
constexpr int kSpgWaveCap = 256;       // products per row up to which one wave owns the row
constexpr int kSpgRowCapMax = 4096;    // ... and four waves: 16 KiB of candidate columns
constexpr int kSpgRowCapDefault = 4096;
constexpr int64_t kSpgBatchDefault = (int64_t)1 << 26;
enum { SPG_BIN_EMPTY = 0, SPG_BIN_WAVE, SPG_BIN_WG, SPG_BIN_SORT, SPG_BIN_COUNT };

const char *const kSpgNameRow = "spgemm_row_kernel";
const char *const kSpgNameSort = "spgemm_sort_fallback";
const char *const kSpgNameBoth = "spgemm_row_kernel + spgemm_sort_fallback";

inline int spg_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kSpgT - 1) / kSpgT, kSpgMaxBlocks)); }

__device__ __forceinline__ int64_t rp_at(const void *rp, int w64, int64_t i) {
    return w64 ? static_cast<const int64_t *>(rp)[i] : (int64_t) static_cast<const int32_t *>(rp)[i];
}

// flag = 1 if some row of B does not ascend strictly
__global__ __launch_bounds__(kSpgT) void spg_ascending_kernel(const void *rp, int w64, const int32_t *__restrict__ col, int64_t n, int *flag) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kSpgT + threadIdx.x; i < n; i += stride)
        for (int64_t k = rp_at(rp, w64, i) + 1, e = rp_at(rp, w64, i + 1); k < e; ++k) bad = bad || col[k] <= col[k - 1];
    if (bad) atomicOr(flag, 1);
}

// u_i = sum over the entries (i, j) of A of nnz(B_j)
__global__ __launch_bounds__(kSpgT) void spg_bound_kernel(const void *rpA, int wA, const int32_t *__restrict__ colA, int64_t n, const void *rpB,
                                                          int wB, int64_t *u) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t i = (int64_t)blockIdx.x * kSpgT + threadIdx.x; i < n; i += stride) {
        int64_t sum = 0;
        for (int64_t s = rp_at(rpA, wA, i), e = rp_at(rpA, wA, i + 1); s < e; ++s) {
            const int64_t j = colA[s];
            sum += rp_at(rpB, wB, j + 1) - rp_at(rpB, wB, j);
        }
        u[i] = sum;
    }
}

// the path of every row; uf = u on the fallback rows and 0 elsewhere (its scan places the expanded products); cnt = 0;
// rows per path into counts[] (one ticket per wave and path)
__global__ __launch_bounds__(kSpgT) void spg_bin_kernel(const int64_t *__restrict__ u, int64_t n, int64_t cap, uint8_t *bin, int64_t *uf,
                                                        int64_t *cnt, unsigned long long *counts) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    unsigned local[SPG_BIN_COUNT] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * kSpgT + threadIdx.x; i < n; i += stride) {
        const int64_t ui = u[i];
        const int b = ui == 0 ? SPG_BIN_EMPTY : ui > cap ? SPG_BIN_SORT : ui <= kSpgWaveCap ? SPG_BIN_WAVE : SPG_BIN_WG;
        bin[i] = (uint8_t)b;
        uf[i] = b == SPG_BIN_SORT ? ui : 0;
        cnt[i] = 0;
        ++local[b];
    }
#pragma unroll
    for (int b = 1; b < SPG_BIN_COUNT; ++b) {
        unsigned v = local[b];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&counts[b], (unsigned long long)v);
    }
}

// inclusive scan of one int per thread over the workgroup; returns this thread's inclusive sum, *total the workgroup's
template <int T>
__device__ __forceinline__ int spg_block_scan(int v, int *lds, int *total) {
    lds[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < T; off <<= 1) {
        const int add = (int)threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    const int incl = lds[threadIdx.x];
    *total = lds[T - 1];
    __syncthreads();
    return incl;
}

// The row path: a workgroup of T threads per row of bin MYBIN (at most CAP products).  NUMERIC = false: cnt[row] = the
// number of distinct candidate columns.  NUMERIC = true: the columns, ascending, and their values at rp[row].
template <int T, int CAP, bool NUMERIC>
__global__ __launch_bounds__(T) void spgemm_row_kernel(const void *rpA, int wA, const int32_t *__restrict__ colA, const double *__restrict__ valA,
                                                       const void *rpB, int wB, const int32_t *__restrict__ colB, const double *__restrict__ valB,
                                                       int64_t n, const uint8_t *__restrict__ bin, int mybin, const int64_t *__restrict__ u,
                                                       int64_t *cnt, const int64_t *__restrict__ rpC, int32_t *colC, double *valC) {
    __shared__ int32_t keys[CAP];
    __shared__ int scan[T];
    constexpr int CH = CAP / T;
    const int tid = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        if (bin[row] != mybin) continue; // (the same for the whole workgroup)
        const int64_t as = rp_at(rpA, wA, row), ae = rp_at(rpA, wA, row + 1);
        const int ui = (int)u[row]; // <= CAP
        int N = T;
        while (N < ui) N <<= 1;
        // gather: T entries of A's row at a time, every thread copies the columns of its row of B behind its predecessors'
        int filled = 0;
        for (int64_t base = as; base < ae; base += T) {
            const int64_t s = base + tid;
            int64_t bs = 0;
            int len = 0;
            if (s < ae) {
                const int64_t j = colA[s];
                bs = rp_at(rpB, wB, j);
                len = (int)(rp_at(rpB, wB, j + 1) - bs);
            }
            int total = 0;
            const int incl = spg_block_scan<T>(len, scan, &total);
            const int dst = filled + incl - len;
            for (int q = 0; q < len; ++q) keys[dst + q] = colB[bs + q]; // (dst + len <= ui <= CAP)
            filled += total;
        }
        for (int idx = ui + tid; idx < N; idx += T) keys[idx] = INT32_MAX; // (columns are < n_cols <= INT32_MAX)
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int idx = tid; idx < N; idx += T) {
                    const int other = idx ^ j;
                    if (other > idx) {
                        const int32_t a = keys[idx], b = keys[other];
                        if (((idx & k) == 0) == (a > b)) { keys[idx] = b; keys[other] = a; }
                    }
                }
                __syncthreads();
            }
        // the first of every run of equal columns, counted per thread over N / T consecutive positions
        const int chunk = N / T, start = tid * chunk;
        int32_t mine[CH];
        int c = 0;
        int32_t prev = start > 0 ? keys[start - 1] : -1;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            if (q < chunk) {
                const int32_t k = keys[start + q];
                if (start + q < ui && k != prev) mine[c++] = k;
                prev = k;
            }
        }
        int total = 0;
        const int incl = spg_block_scan<T>(c, scan, &total); // (ends with a barrier: every thread has read its positions)
        if (!NUMERIC) {
            if (tid == 0) cnt[row] = total;
            continue;
        }
#pragma unroll
        for (int q = 0; q < CH; ++q)
            if (q < c) keys[incl - c + q] = mine[q];
        __syncthreads();
        // a lane per output entry: A's row in CRS order, column k looked up in every B row (ascending, no repeats)
        const int64_t out = rpC[row];
        for (int e = tid; e < total; e += T) {
            const int32_t k = keys[e];
            double acc = 0.0;
            bool first = true;
            for (int64_t s = as; s < ae; ++s) {
                const int64_t j = colA[s];
                int64_t lo = rp_at(rpB, wB, j), hi = rp_at(rpB, wB, j + 1);
                const int64_t end = hi;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (colB[mid] < k) lo = mid + 1; else hi = mid;
                }
                if (lo < end && colB[lo] == k) {
                    const double p = bis_mul_sep(valA[s], valB[lo]);
                    acc = first ? p : __dadd_rn(acc, p);
                    first = false;
                }
            }
            colC[out + e] = k;
            valC[out + e] = acc;
        }
        __syncthreads();
    }
}

// ---- the fallback ------------------------------------------------------------------------------------------------------
// the largest r1 in (r0, n] with off[r1] - off[r0] <= batch, or r0 + 1 where row r0 alone is longer: out = {r1, products}
__global__ void spg_cut_kernel(const int64_t *__restrict__ off, int64_t n, int64_t r0, int64_t batch, int64_t *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t base = off[r0];
    int64_t lo = r0 + 1, hi = n; // off[lo] is the first candidate
    if (off[lo] - base <= batch) {
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (off[mid] - base <= batch) lo = mid; else hi = mid - 1;
        }
    }
    out[0] = lo;
    out[1] = off[lo] - base;
}

// a wave per fallback row of [r0, r1): keys row << 32 | column and the rounded products, in enumeration order
__global__ __launch_bounds__(kSpgT) void spg_expand_kernel(const void *rpA, int wA, const int32_t *__restrict__ colA, const double *__restrict__ valA,
                                                           const void *rpB, int wB, const int32_t *__restrict__ colB, const double *__restrict__ valB,
                                                           int64_t r0, int64_t r1, const uint8_t *__restrict__ bin, const int64_t *__restrict__ off,
                                                           unsigned long long *key, double *val) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kSpgT / 64);
    const int64_t base0 = off[r0];
    for (int64_t row = r0 + (int64_t)blockIdx.x * (kSpgT / 64) + (threadIdx.x >> 6); row < r1; row += waves) {
        if (bin[row] != SPG_BIN_SORT) continue;
        int64_t pos = off[row] - base0;
        const unsigned long long hi = (unsigned long long)row << 32;
        for (int64_t base = rp_at(rpA, wA, row), ae = rp_at(rpA, wA, row + 1); base < ae; base += 64) {
            const int64_t s = base + lane;
            int64_t bs = 0, len = 0;
            double a = 0.0;
            if (s < ae) {
                const int64_t j = colA[s];
                bs = rp_at(rpB, wB, j);
                len = rp_at(rpB, wB, j + 1) - bs;
                a = valA[s];
            }
            int64_t incl = len;
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const int64_t dst = pos + incl - len;
            for (int64_t q = 0; q < len; ++q) {
                key[dst + q] = hi | (uint32_t)colB[bs + q];
                val[dst + q] = bis_mul_sep(a, valB[bs + q]);
            }
            pos += __shfl(incl, 63, 64);
        }
    }
}

__global__ __launch_bounds__(kSpgT) void spg_head_flag_kernel(const unsigned long long *__restrict__ key, int64_t m, int64_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t k = (int64_t)blockIdx.x * kSpgT + threadIdx.x; k < m; k += stride) flag[k] = (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
}
// counting pass: every run is an entry of its row
__global__ __launch_bounds__(kSpgT) void spg_count_runs_kernel(const unsigned long long *__restrict__ key, int64_t m, int64_t *cnt) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t k = (int64_t)blockIdx.x * kSpgT + threadIdx.x; k < m; k += stride)
        if (k == 0 || key[k] != key[k - 1]) atomicAdd(reinterpret_cast<unsigned long long *>(cnt + (key[k] >> 32)), 1ull);
}
// pos: the inclusive scan of the head flags.  The head of run e records where the run starts; the first run of a row
// records its number
__global__ __launch_bounds__(kSpgT) void spg_heads_kernel(const unsigned long long *__restrict__ key, const int64_t *__restrict__ pos, int64_t m,
                                                          int64_t *start, int64_t *row_first) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t k = (int64_t)blockIdx.x * kSpgT + threadIdx.x; k < m; k += stride) {
        if (k != 0 && key[k] == key[k - 1]) continue;
        const int64_t e = pos[k] - 1;
        start[e] = k;
        if (k == 0 || (key[k] >> 32) != (key[k - 1] >> 32)) row_first[key[k] >> 32] = e;
    }
}
// a lane per run: its sum in the sorted (= enumeration) order, the first product starting it
__global__ __launch_bounds__(kSpgT) void spg_run_sum_kernel(const unsigned long long *__restrict__ key, const double *__restrict__ v,
                                                            const int64_t *__restrict__ start, int64_t runs, int64_t m,
                                                            const int64_t *__restrict__ row_first, const int64_t *__restrict__ rpC, int32_t *colC,
                                                            double *valC) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t e = (int64_t)blockIdx.x * kSpgT + threadIdx.x; e < runs; e += stride) {
        const int64_t s = start[e], t = e + 1 < runs ? start[e + 1] : m;
        double acc = v[s];
        for (int64_t k = s + 1; k < t; ++k) acc = __dadd_rn(acc, v[k]);
        const int64_t row = (int64_t)(key[s] >> 32), dst = rpC[row] + (e - row_first[row]);
        colC[dst] = (int32_t)(key[s] & 0xffffffffull);
        valC[dst] = acc;
    }
}

template <typename RP>
__global__ __launch_bounds__(kSpgT) void spg_store_rp_kernel(const int64_t *__restrict__ rp, int64_t count, RP *out) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t i = (int64_t)blockIdx.x * kSpgT + threadIdx.x; i < count; i += stride) out[i] = (RP)rp[i];
}

// ---- the transpose's kernels -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpgT) void spg_iota_kernel(const int32_t *__restrict__ col, int64_t m, uint32_t *key, int64_t *idx) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t k = (int64_t)blockIdx.x * kSpgT + threadIdx.x; k < m; k += stride) { key[k] = (uint32_t)col[k]; idx[k] = k; }
}
// position q of A^T holds entry idx[q] of A: its row (the last r with rp[r] <= idx[q]) becomes the column
__global__ __launch_bounds__(kSpgT) void spg_gather_kernel(const void *rp, int w64, const double *__restrict__ val, int64_t n, int64_t m,
                                                           const int64_t *__restrict__ idx, int32_t *colT, double *valT) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t q = (int64_t)blockIdx.x * kSpgT + threadIdx.x; q < m; q += stride) {
        const int64_t k = idx[q];
        int64_t lo = 0, hi = n; // the first r in [0, n] with rp[r] > k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (rp_at(rp, w64, mid) <= k) lo = mid + 1; else hi = mid;
        }
        colT[q] = (int32_t)(lo - 1);
        valT[q] = val[k];
    }
}
// out[c] = the first position p in the ascending key[0, m) with key[p] >= c, for c in [0, count)
template <typename O>
__global__ __launch_bounds__(kSpgT) void spg_lower_bound_kernel(const uint32_t *__restrict__ key, int64_t m, int64_t count, O *out) {
    const int64_t stride = (int64_t)gridDim.x * kSpgT;
    for (int64_t c = (int64_t)blockIdx.x * kSpgT + threadIdx.x; c < count; c += stride) {
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)key[mid] < c) lo = mid + 1; else hi = mid;
        }
        out[c] = (O)lo;
    }
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { hipFree(p); }
    hipError_t alloc(size_t bytes) {
        cap = std::max<size_t>(bytes, 16);
        return hipMalloc(&p, cap);
    }
    hipError_t grow(size_t bytes) { // (the contents go)
        if (bytes <= cap) return hipSuccess;
        hipFree(p);
        p = nullptr;
        return alloc(bytes);
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct MatGuard { // destroys the matrix unless released
    bis_ctx *ctx;
    bis_mat *m = nullptr;
    ~MatGuard() { if (m) { hipStreamSynchronize(ctx->stream); bis_mat_destroy(ctx, m); } }
    bis_mat *release() { bis_mat *r = m; m = nullptr; return r; }
};

#define SPG_CHECK(call)                                                                                                \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) { ctx->err = std::string(kWho) + ": " #call ": " + hipGetErrorString(e_); return BIS_ERR_HIP; } \
    } while (0)

int bits_for(int64_t count) { // bits that hold every value of [0, count)
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < count) ++b;
    return b;
}

// an n x p matrix without entries
bis_status empty_matrix(bis_ctx *ctx, int64_t n, int64_t p, bis_mat **out) {
    static const char *const kWho = "bis_spgemm";
    MatGuard C{ctx};
    const bool rp64 = bis_want_rp64(0);
    if (bis_status st = bis_mat_alloc(ctx, n, p, 0, rp64, &C.m)) return st;
    SPG_CHECK(hipMemsetAsync(C.m->row_ptr, 0, (rp64 ? 8 : 4) * (size_t)(n + 1), ctx->stream));
    if (bis_status st = bis_mat_finalize(ctx, C.m)) return st;
    SPG_CHECK(hipStreamSynchronize(ctx->stream));
    *out = C.release();
    return BIS_OK;
}

// one pass of the fallback over its rows; numeric = false counts the entries of every row into cnt
struct SortScratch {
    DevBuf key, key_out, val, val_out, pos, start, tmp, cut;
};
bis_status sort_pass(bis_ctx *ctx, const bis_mat *A, const bis_mat *B, const uint8_t *bin, const int64_t *off, int64_t batch, bool numeric,
                     int64_t *cnt, int64_t *row_first, const int64_t *rpC, bis_mat *C, SortScratch &s) {
    static const char *const kWho = "bis_spgemm";
    const int64_t n = A->n_rows;
    const int end_bit = std::min(64, 32 + bits_for(n));
    if (!s.cut.p) SPG_CHECK(s.cut.alloc(16));
    for (int64_t r0 = 0; r0 < n;) {
        int64_t h[2] = {0, 0};
        hipLaunchKernelGGL(spg_cut_kernel, dim3(1), dim3(64), 0, ctx->stream, off, n, r0, batch, s.cut.as<int64_t>());
        SPG_CHECK(hipGetLastError());
        SPG_CHECK(hipMemcpyAsync(h, s.cut.p, 16, hipMemcpyDeviceToHost, ctx->stream));
        SPG_CHECK(hipStreamSynchronize(ctx->stream));
        const int64_t r1 = h[0], m = h[1];
        if (r1 <= r0 || r1 > n || m < 0) { ctx->err = "bis_spgemm: the batches do not advance (internal)"; return BIS_ERR_INVALID; }
        if (m > 0) {
            SPG_CHECK(s.key.grow(8 * (size_t)m));
            SPG_CHECK(s.key_out.grow(8 * (size_t)m));
            SPG_CHECK(s.val.grow(8 * (size_t)m));
            SPG_CHECK(s.val_out.grow(8 * (size_t)m));
            unsigned long long *key = s.key.as<unsigned long long>(), *key_out = s.key_out.as<unsigned long long>();
            const int64_t waves = r1 - r0;
            hipLaunchKernelGGL(spg_expand_kernel, dim3(spg_grid(waves * 64)), dim3(kSpgT), 0, ctx->stream, A->row_ptr, A->rp64 ? 1 : 0, A->col,
                               A->val, B->row_ptr, B->rp64 ? 1 : 0, B->col, B->val, r0, r1, bin, off, key, s.val.as<double>());
            SPG_CHECK(hipGetLastError());
            size_t bytes = 0;
            SPG_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key, key_out, s.val.as<double>(), s.val_out.as<double>(), (size_t)m, 0, end_bit,
                                                ctx->stream));
            SPG_CHECK(s.tmp.grow(bytes));
            SPG_CHECK(rocprim::radix_sort_pairs(s.tmp.p, bytes, key, key_out, s.val.as<double>(), s.val_out.as<double>(), (size_t)m, 0, end_bit,
                                                ctx->stream)); // stable: a run keeps the enumeration order
            if (!numeric) {
                hipLaunchKernelGGL(spg_count_runs_kernel, dim3(spg_grid(m)), dim3(kSpgT), 0, ctx->stream, key_out, m, cnt);
                SPG_CHECK(hipGetLastError());
            } else {
                int64_t *pos = s.key.as<int64_t>(); // (the unsorted keys are done with)
                hipLaunchKernelGGL(spg_head_flag_kernel, dim3(spg_grid(m)), dim3(kSpgT), 0, ctx->stream, key_out, m, pos);
                size_t bytes2 = 0;
                SPG_CHECK(rocprim::inclusive_scan(nullptr, bytes2, pos, pos, (size_t)m, rocprim::plus<int64_t>(), ctx->stream));
                SPG_CHECK(s.tmp.grow(bytes2));
                SPG_CHECK(rocprim::inclusive_scan(s.tmp.p, bytes2, pos, pos, (size_t)m, rocprim::plus<int64_t>(), ctx->stream));
                int64_t runs = 0;
                SPG_CHECK(hipMemcpyAsync(&runs, pos + (m - 1), sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
                SPG_CHECK(hipStreamSynchronize(ctx->stream));
                SPG_CHECK(s.start.grow(8 * (size_t)runs));
                hipLaunchKernelGGL(spg_heads_kernel, dim3(spg_grid(m)), dim3(kSpgT), 0, ctx->stream, key_out, pos, m, s.start.as<int64_t>(),
                                   row_first);
                hipLaunchKernelGGL(spg_run_sum_kernel, dim3(spg_grid(runs)), dim3(kSpgT), 0, ctx->stream, key_out, s.val_out.as<double>(),
                                   s.start.as<int64_t>(), runs, m, row_first, rpC, C->col, C->val);
                SPG_CHECK(hipGetLastError());
            }
        }
        r0 = r1;
    }
    return BIS_OK;
}

template <bool NUMERIC>
bis_status row_pass(bis_ctx *ctx, const bis_mat *A, const bis_mat *B, const uint8_t *bin, const int64_t *u, const unsigned long long *rows,
                    int64_t *cnt, const int64_t *rpC, bis_mat *C) {
    static const char *const kWho = "bis_spgemm";
    const int64_t n = A->n_rows;
    const int wA = A->rp64 ? 1 : 0, wB = B->rp64 ? 1 : 0;
    int32_t *colC = C ? C->col : nullptr;
    double *valC = C ? C->val : nullptr;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)std::max(ctx->n_cus, 1) * 64));
    if (rows[SPG_BIN_WAVE])
        hipLaunchKernelGGL((spgemm_row_kernel<64, kSpgWaveCap, NUMERIC>), dim3(grid), dim3(64), 0, ctx->stream, A->row_ptr, wA, A->col, A->val,
                           B->row_ptr, wB, B->col, B->val, n, bin, (int)SPG_BIN_WAVE, u, cnt, rpC, colC, valC);
    if (rows[SPG_BIN_WG])
        hipLaunchKernelGGL((spgemm_row_kernel<256, kSpgRowCapMax, NUMERIC>), dim3(grid), dim3(256), 0, ctx->stream, A->row_ptr, wA, A->col,
                           A->val, B->row_ptr, wB, B->col, B->val, n, bin, (int)SPG_BIN_WG, u, cnt, rpC, colC, valC);
    SPG_CHECK(hipGetLastError());
    return BIS_OK;
}

bis_status spgemm_impl(bis_ctx *ctx, const bis_mat *A, const bis_mat *B, bis_mat **out) {
    static const char *const kWho = "bis_spgemm";
    const int64_t n = A->n_rows, p = B->n_cols;
    if (n == 0 || A->nnz == 0 || B->nnz == 0) return empty_matrix(ctx, n, p, out);
    const int wA = A->rp64 ? 1 : 0, wB = B->rp64 ? 1 : 0;
    int64_t cap = bis_opts().spgemm_row_cap < 0 ? kSpgRowCapDefault : std::min(bis_opts().spgemm_row_cap, kSpgRowCapMax);
    const int64_t batch = bis_opts().spgemm_batch <= 0 ? kSpgBatchDefault : (int64_t)bis_opts().spgemm_batch;

    DevBuf aux, u, uf, off, cnt, rp, bin, tmp, row_first;
    SPG_CHECK(aux.alloc(8 * (1 + SPG_BIN_COUNT)));
    SPG_CHECK(hipMemsetAsync(aux.p, 0, 8 * (1 + SPG_BIN_COUNT), ctx->stream));
    int *unsorted = aux.as<int>();
    unsigned long long *counts = aux.as<unsigned long long>() + 1;
    SPG_CHECK(u.alloc(8 * (size_t)n));
    SPG_CHECK(uf.alloc(8 * (size_t)(n + 1)));
    SPG_CHECK(off.alloc(8 * (size_t)(n + 1)));
    SPG_CHECK(cnt.alloc(8 * (size_t)(n + 1)));
    SPG_CHECK(rp.alloc(8 * (size_t)(n + 1)));
    SPG_CHECK(bin.alloc((size_t)n));
    if (cap > 0) {
        hipLaunchKernelGGL(spg_ascending_kernel, dim3(spg_grid(B->n_rows)), dim3(kSpgT), 0, ctx->stream, B->row_ptr, wB, B->col, B->n_rows, unsorted);
        int h = 0;
        SPG_CHECK(hipGetLastError());
        SPG_CHECK(hipMemcpyAsync(&h, unsorted, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        SPG_CHECK(hipStreamSynchronize(ctx->stream));
        if (h) cap = 0; // the row path bisects the rows of B
    }
    hipLaunchKernelGGL(spg_bound_kernel, dim3(spg_grid(n)), dim3(kSpgT), 0, ctx->stream, A->row_ptr, wA, A->col, n, B->row_ptr, wB, u.as<int64_t>());
    SPG_CHECK(hipMemsetAsync(uf.as<int64_t>() + n, 0, 8, ctx->stream));
    SPG_CHECK(hipMemsetAsync(cnt.as<int64_t>() + n, 0, 8, ctx->stream));
    hipLaunchKernelGGL(spg_bin_kernel, dim3(spg_grid(n)), dim3(kSpgT), 0, ctx->stream, u.as<int64_t>(), n, cap, bin.as<uint8_t>(), uf.as<int64_t>(),
                       cnt.as<int64_t>(), counts);
    SPG_CHECK(hipGetLastError());
    unsigned long long rows[SPG_BIN_COUNT] = {0, 0, 0, 0};
    SPG_CHECK(hipMemcpyAsync(rows, counts, sizeof(rows), hipMemcpyDeviceToHost, ctx->stream));
    SPG_CHECK(hipStreamSynchronize(ctx->stream));
    const bool any_row = rows[SPG_BIN_WAVE] + rows[SPG_BIN_WG] > 0, any_sort = rows[SPG_BIN_SORT] > 0;
    if (!any_row && !any_sort) return empty_matrix(ctx, n, p, out);

    auto scan = [&](const int64_t *in, int64_t *res) -> bis_status { // exclusive, n + 1 items: res[n] = the total
        size_t bytes = 0;
        SPG_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, res, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), ctx->stream));
        SPG_CHECK(tmp.grow(bytes));
        SPG_CHECK(rocprim::exclusive_scan(tmp.p, bytes, in, res, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), ctx->stream));
        return BIS_OK;
    };
    SortScratch scratch;
    // symbolic
    if (any_row)
        if (bis_status st = row_pass<false>(ctx, A, B, bin.as<uint8_t>(), u.as<int64_t>(), rows, cnt.as<int64_t>(), nullptr, nullptr)) return st;
    if (any_sort) {
        if (bis_status st = scan(uf.as<int64_t>(), off.as<int64_t>())) return st;
        SPG_CHECK(row_first.alloc(8 * (size_t)n));
        if (bis_status st = sort_pass(ctx, A, B, bin.as<uint8_t>(), off.as<int64_t>(), batch, false, cnt.as<int64_t>(), row_first.as<int64_t>(),
                                      nullptr, nullptr, scratch))
            return st;
    }
    if (bis_status st = scan(cnt.as<int64_t>(), rp.as<int64_t>())) return st;
    int64_t nnz = 0;
    SPG_CHECK(hipMemcpyAsync(&nnz, rp.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPG_CHECK(hipStreamSynchronize(ctx->stream));
    // numeric
    MatGuard C{ctx};
    if (bis_status st = bis_mat_alloc(ctx, n, p, nnz, bis_want_rp64(nnz), &C.m)) return st;
    if (C.m->rp64) hipLaunchKernelGGL(spg_store_rp_kernel<int64_t>, dim3(spg_grid(n + 1)), dim3(kSpgT), 0, ctx->stream, rp.as<int64_t>(), n + 1,
                                      (int64_t *)C.m->row_ptr);
    else hipLaunchKernelGGL(spg_store_rp_kernel<int32_t>, dim3(spg_grid(n + 1)), dim3(kSpgT), 0, ctx->stream, rp.as<int64_t>(), n + 1,
                            (int32_t *)C.m->row_ptr);
    if (any_row)
        if (bis_status st = row_pass<true>(ctx, A, B, bin.as<uint8_t>(), u.as<int64_t>(), rows, cnt.as<int64_t>(), rp.as<int64_t>(), C.m)) return st;
    if (any_sort)
        if (bis_status st = sort_pass(ctx, A, B, bin.as<uint8_t>(), off.as<int64_t>(), batch, true, cnt.as<int64_t>(), row_first.as<int64_t>(),
                                      rp.as<int64_t>(), C.m, scratch))
            return st;
    SPG_CHECK(hipGetLastError());
    SPG_CHECK(hipStreamSynchronize(ctx->stream));
    if (bis_status st = bis_mat_finalize(ctx, C.m)) return st;
    C.m->spgemm_kernel = any_row && any_sort ? kSpgNameBoth : any_row ? kSpgNameRow : kSpgNameSort;
    *out = C.release();
    return BIS_OK;
}

bis_status transpose_impl(bis_ctx *ctx, const bis_mat *A, bis_mat **out) {
    static const char *const kWho = "bis_mat_transpose";
    const int64_t n = A->n_rows, m = A->n_cols, nnz = A->nnz;
    if (nnz == 0) return empty_matrix(ctx, m, n, out);
    DevBuf key, key_out, idx, idx_out, tmp;
    SPG_CHECK(key.alloc(4 * (size_t)nnz));
    SPG_CHECK(key_out.alloc(4 * (size_t)nnz));
    SPG_CHECK(idx.alloc(8 * (size_t)nnz));
    SPG_CHECK(idx_out.alloc(8 * (size_t)nnz));
    hipLaunchKernelGGL(spg_iota_kernel, dim3(spg_grid(nnz)), dim3(kSpgT), 0, ctx->stream, A->col, nnz, key.as<uint32_t>(), idx.as<int64_t>());
    SPG_CHECK(hipGetLastError());
    const int end_bit = std::min(32, bits_for(m));
    size_t bytes = 0;
    SPG_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key.as<uint32_t>(), key_out.as<uint32_t>(), idx.as<int64_t>(), idx_out.as<int64_t>(),
                                        (size_t)nnz, 0, end_bit, ctx->stream));
    SPG_CHECK(tmp.alloc(bytes));
    SPG_CHECK(rocprim::radix_sort_pairs(tmp.p, bytes, key.as<uint32_t>(), key_out.as<uint32_t>(), idx.as<int64_t>(), idx_out.as<int64_t>(),
                                        (size_t)nnz, 0, end_bit, ctx->stream)); // stable: a column keeps the CRS order of A
    MatGuard T{ctx};
    if (bis_status st = bis_mat_alloc(ctx, m, n, nnz, bis_want_rp64(nnz), &T.m)) return st;
    hipLaunchKernelGGL(spg_gather_kernel, dim3(spg_grid(nnz)), dim3(kSpgT), 0, ctx->stream, A->row_ptr, A->rp64 ? 1 : 0, A->val, n, nnz,
                       idx_out.as<int64_t>(), T.m->col, T.m->val);
    if (T.m->rp64) hipLaunchKernelGGL(spg_lower_bound_kernel<int64_t>, dim3(spg_grid(m + 1)), dim3(kSpgT), 0, ctx->stream, key_out.as<uint32_t>(),
                                      nnz, m + 1, (int64_t *)T.m->row_ptr);
    else hipLaunchKernelGGL(spg_lower_bound_kernel<int32_t>, dim3(spg_grid(m + 1)), dim3(kSpgT), 0, ctx->stream, key_out.as<uint32_t>(), nnz,
                            m + 1, (int32_t *)T.m->row_ptr);
    SPG_CHECK(hipGetLastError());
    SPG_CHECK(hipStreamSynchronize(ctx->stream));
    if (bis_status st = bis_mat_finalize(ctx, T.m)) return st;
    *out = T.release();
    return BIS_OK;
}

} // namespace

extern "C" {

bis_status bis_spgemm(bis_ctx *ctx, const bis_mat *A, const bis_mat *B, bis_mat **C) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && B && C, "bis_spgemm: bad arguments");
    BIS_REQUIRE(ctx, A->n_cols == B->n_rows, "bis_spgemm: the columns of A and the rows of B differ in number");
    BIS_REQUIRE(ctx, !A->view && !B->view, "bis_spgemm: a row-range view is not an operand");
    bis_mat *Cm = nullptr;
    const bis_status st = spgemm_impl(ctx, A, B, &Cm);
    if (st != BIS_OK) return st;
    *C = Cm;
    return BIS_OK;
}

bis_status bis_mat_transpose(bis_ctx *ctx, const bis_mat *A, bis_mat **At) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && At, "bis_mat_transpose: bad arguments");
    BIS_REQUIRE(ctx, !A->view, "bis_mat_transpose: a row-range view is not an operand");
    bis_mat *T = nullptr;
    const bis_status st = transpose_impl(ctx, A, &T);
    if (st != BIS_OK) return st;
    *At = T;
    return BIS_OK;
}

const char *bis_spgemm_kernel(const bis_mat *C) { return C ? C->spgemm_kernel : ""; }

bis_status bis_spgemm_limits(int *wave_cap, int *row_cap, int *row_cap_max, int64_t *batch) {
    if (wave_cap) *wave_cap = kSpgWaveCap;
    if (row_cap) *row_cap = kSpgRowCapDefault;
    if (row_cap_max) *row_cap_max = kSpgRowCapMax;
    if (batch) *batch = kSpgBatchDefault;
    return BIS_OK;
}

} // extern "C"
