// bis_bjacobi.hip -- block Jacobi (no reference counterpart): the dense diagonal blocks of A, inverted once on the device
// (bis_bj_create) and applied as a block-diagonal product (bis_bj_apply, bis_bj_mapply).  Definitions: include/bis_hip.h.
//
// One power-of-two lane group per block, G = the smallest power of two >= the largest block (1 .. 32), 64 / G blocks per wave.
// Every loop that a wave runs together (the elimination steps, the product's columns) is bounded by the handle's largest
// block and predicated by the lane's own block size, so blocks of different sizes in one wave neither diverge around a
// barrier or a cross-lane move nor wait for each other.
//
// Storage of an inverse block R of m rows at its (even) offset: column pairs, lane-major -- R(i, j) and R(i, j + 1) of an even
// j < m - 1 at j m + 2 i and j m + 2 i + 1, the last column of an odd m at (m - 1) m + i; m m values, padded to an even count.
// Lane i of the group reads one 16-byte word per column pair, the group's lanes read consecutive words, and the blocks of
// a wave follow each other: the wave's loads are contiguous.  No index is streamed for uniform blocks.
#include "bis_internal.hpp"

#include <algorithm>

// The header defines every product, difference and sum as rounded on its own.  The __d*_rn intrinsics do not say that to the
// compiler (they are inline functions of plain operators, compiled with contraction allowed, and a * b + c made of them is
// fused): the two kernels use plain operators under "fp contract(off)" instead, as bis_minres.hip's scalar algebra does.

struct bis_bj {
    int64_t n = 0, n_blocks = 0;
    int bs = 0;             // uniform block size; 0 with a block_ptr
    int max_block = 0, G = 1;
    int64_t value_count = 0; // sum of m^2
    int64_t stored = 0;      // doubles in vals (every block padded to an even count)
    double *vals = nullptr;
    int32_t *bptr = nullptr; // device, n_blocks + 1 (block_ptr handles only)
    int64_t *voff = nullptr; // device, n_blocks + 1 (block_ptr handles only)
    std::vector<int32_t> bptr_host; // block_ptr handles only
    bis_mat *operand = nullptr;
};

namespace {

constexpr int kBjT = 256;           // apply: threads per workgroup
constexpr int kBjSetupT = 64;       // setup: one wave per workgroup (its barriers are wave barriers)
constexpr int kBjMaxBlock = 32;
constexpr int kBjMaxGrid = 16384;
constexpr int kBjMaxK = 8;

typedef double bj_v2d __attribute__((ext_vector_type(2)));

__host__ __device__ __forceinline__ int64_t bj_padded(int64_t m) { return m * m + (m & 1); }

// Block `blk` of the handle: first row s, rows m, offset of its values.
template <bool VAR>
__device__ __forceinline__ void bj_block(int64_t blk, int64_t n_blocks, int64_t n, int bs, const int32_t *__restrict__ bptr,
                                         const int64_t *__restrict__ voff, int64_t &s, int &m, int64_t &vbase) {
    if (blk >= n_blocks) { s = 0; m = 0; vbase = 0; return; }
    if (VAR) {
        s = bptr[blk];
        m = bptr[blk + 1] - (int32_t)s;
        vbase = voff[blk];
    } else {
        s = blk * bs;
        m = (int)min((int64_t)bs, n - s);
        vbase = blk * bj_padded(bs);
    }
}

// ---- setup: gather, invert, symmetrise ------------------------------------------------------------------------------
// The group's tile is [B | I] with a row stride of 2 G + 1 doubles (lane i on row i: no bank conflict; a row read by the
// whole group: a broadcast).  Gauss-Jordan with partial pivoting exactly as the header states it; every lane finds the pivot
// row by the same scan, rows are swapped and scaled column-wise by the group, then lane i eliminates its own row.
template <typename RP, bool VAR>
__global__ __launch_bounds__(kBjSetupT) void bj_setup_kernel(const RP *__restrict__ rp, const int32_t *__restrict__ col,
                                                             const double *__restrict__ val, int64_t n, int64_t n_blocks, int bs,
                                                             const int32_t *__restrict__ bptr, const int64_t *__restrict__ voff,
                                                             int G, int max_block, int symmetrize, double *__restrict__ vals,
                                                             int *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ double bj_lds[];
    const int per_wave = kBjSetupT / G, grp = threadIdx.x / G, i = threadIdx.x % G;
    const int S = 2 * G + 1;
    double *T = bj_lds + (size_t)grp * G * S;
    const int64_t stride = (int64_t)gridDim.x * per_wave;
    const int64_t rounds = (n_blocks + stride - 1) / stride; // the same for every thread: the barriers below are uniform
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t blk = it * stride + (int64_t)blockIdx.x * per_wave + grp;
        int64_t s, vbase;
        int m;
        bj_block<VAR>(blk, n_blocks, n, bs, bptr, voff, s, m, vbase);
        const bool own = i < m;
        bool dead = false; // a zero or non-finite pivot: the block stops, the create fails
        __syncthreads();   // (the tile's readers of the round before)
        if (own) {
            for (int j = 0; j < 2 * m; ++j) T[i * S + j] = (j == m + i) ? 1.0 : 0.0;
            const int64_t r = s + i;
            for (RP e = rp[r]; e < rp[r + 1]; ++e) {
                const int64_t c = col[e];
                if (c >= s && c < s + m) T[i * S + (c - s)] = T[i * S + (c - s)] + val[e];
            }
        }
        __syncthreads();
        for (int k = 0; k < max_block; ++k) {
            const bool step = k < m && !dead;
            int p = k;
            if (step) {
                double best = fabs(T[k * S + k]);
                for (int q = k + 1; q < m; ++q) {
                    const double a = fabs(T[q * S + k]);
                    if (a > best) { best = a; p = q; }
                }
                const double piv = T[p * S + k];
                if (piv == 0.0 || !isfinite(piv)) dead = true;
            }
            const bool go = step && !dead;
            __syncthreads();
            if (go && p != k)
                for (int c = i; c < 2 * m; c += G) {
                    const double a = T[k * S + c];
                    T[k * S + c] = T[p * S + c];
                    T[p * S + c] = a;
                }
            __syncthreads();
            const double r = go ? 1.0 / T[k * S + k] : 0.0;
            __syncthreads();
            if (go)
                for (int c = i; c < 2 * m; c += G) T[k * S + c] = T[k * S + c] * r;
            __syncthreads();
            if (go && own && i != k) {
                const double f = T[i * S + k];
                for (int c = 0; c < 2 * m; ++c) T[i * S + c] = T[i * S + c] - f * T[k * S + c];
            }
            __syncthreads();
        }
        if (dead && i == 0) *status = 1;
        if (own && !dead) {
            for (int j = 0; j < m; ++j) {
                double v = T[i * S + m + j];
                if (symmetrize) v = (v + T[j * S + m + i]) * 0.5;
                const int64_t pos = ((j | 1) < m) ? (int64_t)(j & ~1) * m + 2 * i + (j & 1) : (int64_t)j * m + i;
                vals[vbase + pos] = v;
            }
        }
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------
// out(s + i, c) = sum_j R(i, j) in(s + j, c) for K interleaved columns: lane i of the group fetches its own K input entries
// (each entry is read from memory once) and gets the others by cross-lane moves; products and additions rounded one by one,
// j ascending.  Every lane of a wave has read its inputs before any lane writes: out may alias in.
template <int K, bool VAR>
__global__ __launch_bounds__(kBjT) void bj_apply_kernel(const double *__restrict__ vals, int64_t n, int64_t n_blocks, int bs,
                                                        const int32_t *__restrict__ bptr, const int64_t *__restrict__ voff, int G,
                                                        int max_block, double *out, const double *in, const int *stop) {
#pragma clang fp contract(off)
    if (stop && stop[1]) return;
    const int per_wg = kBjT / G, grp = threadIdx.x / G, i = threadIdx.x % G;
    const int lane0 = (threadIdx.x & 63) - i; // the group's first lane in its wave
    const int64_t stride = (int64_t)gridDim.x * per_wg;
    const int64_t rounds = (n_blocks + stride - 1) / stride; // the same for every thread: the cross-lane moves are uniform
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t blk = it * stride + (int64_t)blockIdx.x * per_wg + grp;
        int64_t s, vbase;
        int m;
        bj_block<VAR>(blk, n_blocks, n, bs, bptr, voff, s, m, vbase);
        const bool own = i < m;
        double x[K], acc[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            x[c] = own ? __builtin_nontemporal_load(in + (s + i) * K + c) : 0.0;
            acc[c] = 0.0;
        }
        const double *R = vals + vbase;
        for (int j = 0; j < max_block; j += 2) {
            double r0 = 0.0, r1 = 0.0;
            const bool has0 = own && j < m, has1 = own && j + 1 < m;
            if (has1) {
                const bj_v2d v = __builtin_nontemporal_load(reinterpret_cast<const bj_v2d *>(R + (int64_t)j * m + 2 * i));
                r0 = v.x;
                r1 = v.y;
            } else if (has0) {
                r0 = __builtin_nontemporal_load(R + (int64_t)j * m + i);
            }
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const double x0 = __shfl(x[c], (lane0 + j) & 63, 64), x1 = __shfl(x[c], (lane0 + j + 1) & 63, 64);
                if (has0) {
                    const double p0 = r0 * x0;
                    acc[c] = j == 0 ? p0 : acc[c] + p0;
                }
                if (has1) acc[c] = acc[c] + r1 * x1;
            }
        }
        if (own) {
#pragma unroll
            for (int c = 0; c < K; ++c) out[(s + i) * K + c] = acc[c];
        }
    }
}

template <int K>
void bj_launch_k(bis_ctx *ctx, const bis_bj *bj, int grid, double *out, const double *in) {
    if (bj->bs)
        hipLaunchKernelGGL((bj_apply_kernel<K, false>), dim3(grid), dim3(kBjT), 0, ctx->stream, bj->vals, bj->n, bj->n_blocks, bj->bs,
                           nullptr, nullptr, bj->G, bj->max_block, out, in, ctx->spmv_stop);
    else
        hipLaunchKernelGGL((bj_apply_kernel<K, true>), dim3(grid), dim3(kBjT), 0, ctx->stream, bj->vals, bj->n, bj->n_blocks, 0,
                           bj->bptr, bj->voff, bj->G, bj->max_block, out, in, ctx->spmv_stop);
}

bis_status bj_launch(bis_ctx *ctx, const bis_bj *bj, double *out, const double *in, int k) {
    const int64_t per_wg = kBjT / bj->G;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((bj->n_blocks + per_wg - 1) / per_wg, kBjMaxGrid));
    switch (k) {
    case 1: bj_launch_k<1>(ctx, bj, grid, out, in); break;
    case 2: bj_launch_k<2>(ctx, bj, grid, out, in); break;
    case 3: bj_launch_k<3>(ctx, bj, grid, out, in); break;
    case 4: bj_launch_k<4>(ctx, bj, grid, out, in); break;
    case 5: bj_launch_k<5>(ctx, bj, grid, out, in); break;
    case 6: bj_launch_k<6>(ctx, bj, grid, out, in); break;
    case 7: bj_launch_k<7>(ctx, bj, grid, out, in); break;
    default: bj_launch_k<8>(ctx, bj, grid, out, in); break;
    }
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

void bj_free(bis_ctx *ctx, bis_bj *bj) {
    hipStreamSynchronize(ctx->stream);
    if (bj->operand) { bj->operand->bj = nullptr; bis_mat_destroy(ctx, bj->operand); }
    hipFree(bj->vals);
    hipFree(bj->bptr);
    hipFree(bj->voff);
    delete bj;
}

#define BJ_CHECK(call)                                                                                                 \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) { ctx->err = std::string("bis_bj_create: " #call ": ") + hipGetErrorString(e_); return BIS_ERR_HIP; } \
    } while (0)

bis_status bj_build(bis_ctx *ctx, const bis_mat *A, bis_bj *bj, int symmetrize) {
    const int64_t n = bj->n;
    if (bis_status st = bis_mat_alloc(ctx, n, n, 0, false, &bj->operand)) return st;
    BJ_CHECK(hipMemsetAsync(bj->operand->row_ptr, 0, sizeof(int32_t) * (size_t)(n + 1), ctx->stream));
    if (bis_status st = bis_mat_finalize(ctx, bj->operand)) return st;
    bj->operand->bj = bj;
    if (n == 0) { BJ_CHECK(hipStreamSynchronize(ctx->stream)); return BIS_OK; }
    const bool var = bj->bs == 0;
    if (var) {
        std::vector<int64_t> voff((size_t)bj->n_blocks + 1);
        voff[0] = 0;
        for (int64_t b = 0; b < bj->n_blocks; ++b) voff[b + 1] = voff[b] + bj_padded(bj->bptr_host[b + 1] - bj->bptr_host[b]);
        bj->stored = voff[bj->n_blocks];
        BJ_CHECK(hipMalloc(&bj->bptr, sizeof(int32_t) * voff.size()));
        BJ_CHECK(hipMalloc(&bj->voff, sizeof(int64_t) * voff.size()));
        BJ_CHECK(hipMemcpy(bj->bptr, bj->bptr_host.data(), sizeof(int32_t) * voff.size(), hipMemcpyHostToDevice));
        BJ_CHECK(hipMemcpy(bj->voff, voff.data(), sizeof(int64_t) * voff.size(), hipMemcpyHostToDevice));
    } else {
        bj->stored = bj->n_blocks * bj_padded(bj->bs);
    }
    int *status = nullptr;
    BJ_CHECK(hipMalloc(&bj->vals, sizeof(double) * (size_t)bj->stored));
    BJ_CHECK(hipMemsetAsync(bj->vals, 0, sizeof(double) * (size_t)bj->stored, ctx->stream));
    BJ_CHECK(hipMalloc(&status, sizeof(int)));
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int), ctx->stream);
    if (e == hipSuccess) {
        const int G = bj->G;
        const int64_t per_wave = kBjSetupT / G;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((bj->n_blocks + per_wave - 1) / per_wave, 4 * kBjMaxGrid));
        const size_t lds = sizeof(double) * (size_t)kBjSetupT * (2 * G + 1);
#define BJ_SETUP(RP, VAR)                                                                                              \
        hipLaunchKernelGGL((bj_setup_kernel<RP, VAR>), dim3(grid), dim3(kBjSetupT), lds, ctx->stream, (const RP *)A->row_ptr, A->col, \
                           A->val, n, bj->n_blocks, bj->bs, bj->bptr, bj->voff, G, bj->max_block, symmetrize, bj->vals, status)
        if (A->rp64) { if (var) BJ_SETUP(int64_t, true); else BJ_SETUP(int64_t, false); }
        else { if (var) BJ_SETUP(int32_t, true); else BJ_SETUP(int32_t, false); }
#undef BJ_SETUP
        e = hipGetLastError();
    }
    int h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, status, sizeof h, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(status);
    BJ_CHECK(e);
    if (bis_status fs = bis_fault_check(ctx)) return fs;
    if (h) { ctx->err = "bis_bj_create: a diagonal block has a zero or non-finite pivot"; return BIS_ERR_ZERO_DIAG; }
    return BIS_OK;
}

} // namespace

extern "C" {

bis_status bis_bj_create(bis_ctx *ctx, const bis_mat *A, const bis_bj_params *params, bis_bj **out) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A && params && out, "bis_bj_create: bad arguments");
    BIS_REQUIRE(ctx, A->n_rows == A->n_cols, "bis_bj_create: square matrix required");
    BIS_REQUIRE(ctx, !A->view, "bis_bj_create: a row-range view has no diagonal block of its own");
    const int64_t n = A->n_rows;
    int max_block = 0;
    if (params->block_ptr) {
        const int32_t *bp = params->block_ptr;
        BIS_REQUIRE(ctx, params->n_blocks >= 0 && params->n_blocks <= n && bp[0] == 0,
                    "bis_bj_create: block_ptr must start at 0 (0 <= n_blocks <= n)");
        for (int64_t b = 0; b < params->n_blocks; ++b) {
            const int64_t m = (int64_t)bp[b + 1] - bp[b];
            BIS_REQUIRE(ctx, m >= 1 && m <= kBjMaxBlock, "bis_bj_create: block_ptr must ascend strictly, by at most 32 rows a block");
            max_block = std::max(max_block, (int)m);
        }
        BIS_REQUIRE(ctx, bp[params->n_blocks] == n, "bis_bj_create: block_ptr must end at n");
    } else {
        BIS_REQUIRE(ctx, params->block_size >= 1 && params->block_size <= kBjMaxBlock, "bis_bj_create: block_size must be between 1 and 32");
    }
    bis_bj *bj = new bis_bj;
    bj->n = n;
    if (params->block_ptr) {
        bj->n_blocks = params->n_blocks;
        bj->max_block = max_block;
        bj->bptr_host.assign(params->block_ptr, params->block_ptr + params->n_blocks + 1);
        for (int64_t b = 0; b < bj->n_blocks; ++b) {
            const int64_t m = bj->bptr_host[b + 1] - bj->bptr_host[b];
            bj->value_count += m * m;
        }
    } else {
        bj->bs = params->block_size;
        bj->n_blocks = (n + bj->bs - 1) / bj->bs;
        bj->max_block = (int)std::min<int64_t>(bj->bs, n);
        const int64_t last = n - (bj->n_blocks - 1) * bj->bs;
        bj->value_count = n == 0 ? 0 : (bj->n_blocks - 1) * (int64_t)bj->bs * bj->bs + last * last;
    }
    while (bj->G < bj->max_block) bj->G *= 2;
    const bis_status st = bj_build(ctx, A, bj, params->symmetrize != 0);
    if (st != BIS_OK) { bj_free(ctx, bj); return st; }
    *out = bj;
    return BIS_OK;
}

bis_status bis_bj_destroy(bis_ctx *ctx, bis_bj *bj) {
    BIS_CTX_OK(ctx);
    if (bj) bj_free(ctx, bj);
    return BIS_OK;
}

bis_status bis_bj_apply(bis_ctx *ctx, const bis_bj *bj, double *out, const double *in) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, bj, "bis_bj_apply: bad arguments");
    if (bj->n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, out && in, "bis_bj_apply: null vector");
    return bj_launch(ctx, bj, out, in, 1);
}

bis_status bis_bj_mapply(bis_ctx *ctx, const bis_bj *bj, double *OUT, const double *IN, int n_rhs) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, bj, "bis_bj_mapply: bad arguments");
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kBjMaxK, "bis_bj_mapply: n_rhs must be between 1 and 8");
    if (bj->n == 0) return BIS_OK;
    BIS_REQUIRE(ctx, OUT && IN, "bis_bj_mapply: null OUT or IN");
    return bj_launch(ctx, bj, OUT, IN, n_rhs);
}

const bis_mat *bis_bj_operand(const bis_bj *bj) { return bj ? bj->operand : nullptr; }

bis_status bis_bj_info(const bis_bj *bj, int64_t *n_blocks, int *max_block, int64_t *value_count) {
    if (!bj) return BIS_ERR_INVALID;
    if (n_blocks) *n_blocks = bj->n_blocks;
    if (max_block) *max_block = bj->max_block;
    if (value_count) *value_count = bj->value_count;
    return BIS_OK;
}

bis_status bis_bj_blocks(bis_ctx *ctx, const bis_bj *bj, double *host_values, int64_t *host_offsets) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, bj, "bis_bj_blocks: bad arguments");
    std::vector<double> raw;
    if (host_values && bj->stored) {
        raw.resize((size_t)bj->stored);
        BIS_HIP_CHECK(ctx, hipMemcpyAsync(raw.data(), bj->vals, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, ctx->stream));
        BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    int64_t off = 0, voff = 0;
    for (int64_t b = 0; b < bj->n_blocks; ++b) {
        const int64_t s = bj->bs ? b * bj->bs : bj->bptr_host[b];
        const int64_t m = bj->bs ? std::min<int64_t>(bj->bs, bj->n - s) : bj->bptr_host[b + 1] - s;
        if (host_offsets) host_offsets[b] = off;
        if (host_values)
            for (int64_t i = 0; i < m; ++i)
                for (int64_t j = 0; j < m; ++j)
                    host_values[off + i * m + j] = raw[(size_t)(voff + (((j | 1) < m) ? (j & ~(int64_t)1) * m + 2 * i + (j & 1) : j * m + i))];
        off += m * m;
        voff += bj->bs ? bj_padded(bj->bs) : bj_padded(m);
    }
    if (host_offsets) host_offsets[bj->n_blocks] = off;
    return BIS_OK;
}

} // extern "C"
