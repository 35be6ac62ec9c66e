// bis_spmm.hip -- Y = A X for 1 <= k <= 8 right-hand sides stored interleaved (X[c*k + j], Y[r*k + j]).
//
// The matrix stream is the whole cost of an SpMV; k vectors behind one stream cost 12 nnz + rp (n_rows + 1) +
// 8 k (n_cols + n_rows) bytes instead of k times the one-vector stream, and every gather is 8 k contiguous bytes.
//
// Arithmetic (the contract of include/bis_hip.h): for every row r and column j, acc = 0.0, then for the row's entries in
// CRS storage order acc += val[e] * X[col[e]*k + j], product and addition rounded separately -- phase 2 of
// spmv_rowblock_kernel (bis_spmv_rowblock.hip), so column j of the result is bis_spmv on column j bit for bit wherever bis_spmv
// does not run its wave-per-row kernel.
//
//   spmm_rowblock_kernel<RP, K, V>   a workgroup per block of the PLAIN row-block table (blk_row / blk_nnz, nothing new is
//                                    built).  The block is cut into tiles of whole rows whose products fit kSpmmLds doubles
//                                    of LDS: at most cap(K) = ((3840 / K) & ~3) - 4 non-zeros.  Per tile:
//                                    phase 1: a lane takes 4 consecutive non-zeros (one 16-byte col load, two 16-byte val
//                                             loads, non-temporal), gathers the K doubles of X behind each of them (V = 2:
//                                             16-byte loads -- K even and X 16-byte aligned; V = 1: 8-byte loads) and parks
//                                             the 4 K products in LDS as prod[e*K + j];
//                                    phase 2: a lane per (row, j) pair sums its products left to right and stores
//                                             Y[r*K + j] (neighbouring lanes: neighbouring j, then the next row -- the Y
//                                             stores of a wave are contiguous).
//                                    val / col are read once whatever K.  LDS: 30 KiB of products + 4 (chunk + 2) bytes of
//                                    row offsets (<= 8 KiB at the default chunks): 4 workgroups = 16 waves per CU for every K.
//   spmm_lane_serial_kernel<RP>      the fallback where a row does not fit a tile (longest row + 3 > cap(K)) or the block
//                                    table was built with a chunk above 4096: a lane per (row, j), a serial loop over the
//                                    row in the same order, straight from global memory.
// Which one runs is a function of (max_row_nnz, chunk_nnz, K) and of X's alignment for V: no trial, nothing allocated.
#include "bis_internal.hpp"

#include <string>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int kSpmmT = 256;
constexpr int kSpmmLds = 3840;      // doubles of products per workgroup (30 KiB: with the row offsets under 40 KiB, 4 workgroups per CU)
constexpr int kSpmmMaxChunk = 4096; // row offsets in LDS: the block table's chunk bounds the rows of a block
constexpr int kSpmmMaxK = 8;

inline int spmm_cap(int k) { return ((kSpmmLds / k) & ~3) - 4; }

template <typename RP, int K, int V>
__global__ __launch_bounds__(kSpmmT) void spmm_rowblock_kernel(
    const RP *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ X, double *__restrict__ Y, const int32_t *__restrict__ blk_row,
    const int64_t *__restrict__ blk_nnz, int n_blocks, int cap, const int *stop) {
    if (stop && stop[1]) return; // the solver has stopped: this launch is a no-op
    extern __shared__ __attribute__((aligned(16))) double prod[]; // [(cap + 4) * K], then the row offsets
    int *off = reinterpret_cast<int *>(prod + (size_t)(cap + 4) * K);
    const int b = blockIdx.x;
    if (b >= n_blocks) return;
    const int r0 = blk_row[b], n_r = blk_row[b + 1] - r0;
    const int64_t s4 = blk_nnz[b] & ~(int64_t)3;
    for (int i = threadIdx.x; i <= n_r; i += kSpmmT) off[i] = (int)((int64_t)row_ptr[r0 + i] - s4);
    __syncthreads();
    int ra = 0;
    while (ra < n_r) { // (uniform: every lane walks the same tiles)
        const int a = off[ra], a4 = a & ~3;
        int lo = ra + 1, hi = n_r; // the last row boundary the tile reaches: off[ra + 1] - a4 <= cap by the launch condition
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] - a4 <= cap) lo = mid; else hi = mid - 1;
        }
        const int rb = lo, z = off[rb];
        // phase 1: stream val / col, gather the K doubles of X per non-zero, park the products.  Lanes past the tile's end
        // re-read its last vector (clamped index); the entries of neighbouring rows inside the first and last 4-aligned
        // vector are loaded and gathered (valid columns) but never stored.
        if (z > a) {
            const int k_last = (z - 1) & ~3;
            for (int base = a4; base < z; base += 4 * kSpmmT) {
                const int kk = base + 4 * (int)threadIdx.x;
                const int64_t g = s4 + min(kk, k_last);
                const v4i c = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(col + g));
                const v2d va = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(val + g));
                const v2d vb = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(val + g + 2));
                const int cc[4] = {c.x, c.y, c.z, c.w};
                const double vv[4] = {va.x, va.y, vb.x, vb.y};
                double xv[4][K];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double *xr = X + (size_t)cc[q] * K;
                    if (V == 2) {
#pragma unroll
                        for (int j = 0; j < K; j += 2) {
                            const v2d t = *reinterpret_cast<const v2d *>(xr + j);
                            xv[q][j] = t.x;
                            xv[q][j + 1] = t.y;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < K; ++j) xv[q][j] = xr[j];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = kk + q;
                    if (e >= a && e < z) {
                        double *dst = prod + (size_t)(e - a4) * K;
                        if (K % 2 == 0) {
#pragma unroll
                            for (int j = 0; j < K; j += 2)
                                *reinterpret_cast<v2d *>(dst + j) = v2d{__dmul_rn(vv[q], xv[q][j]), __dmul_rn(vv[q], xv[q][j + 1])};
                        } else {
#pragma unroll
                            for (int j = 0; j < K; ++j) dst[j] = __dmul_rn(vv[q], xv[q][j]);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // phase 2: a lane per (row, j), left-to-right sum in CRS order
        const int pairs = (rb - ra) * K;
        for (int q = threadIdx.x; q < pairs; q += kSpmmT) {
            const int rl = ra + q / K, j = q % K;
            const int lo_e = off[rl] - a4, hi_e = off[rl + 1] - a4;
            double acc = 0.0;
            for (int e = lo_e; e < hi_e; ++e) acc = __dadd_rn(acc, prod[(size_t)e * K + j]);
            Y[(size_t)(r0 + rl) * K + j] = acc;
        }
        __syncthreads(); // the next tile overwrites prod
        ra = rb;
    }
}

// the fallback: a lane per (row, j), the row's entries in order straight from global memory
template <typename RP>
__global__ __launch_bounds__(256) void spmm_lane_serial_kernel(
    const RP *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ X, double *__restrict__ Y, int64_t n_rows, int k, const int *stop) {
    if (stop && stop[1]) return;
    const int64_t total = n_rows * k, gs = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += gs) {
        const int64_t r = q / k;
        const int j = (int)(q - r * k);
        double acc = 0.0;
        for (int64_t e = (int64_t)row_ptr[r]; e < (int64_t)row_ptr[r + 1]; ++e) {
            double pr = val[e] * X[(size_t)col[e] * k + j];
            asm volatile("" : "+v"(pr)); // pin the rounded product: no contraction into an fma with the sum
            acc += pr;
        }
        Y[q] = acc;
    }
}

// column j of an interleaved block <-> a plain vector
__global__ __launch_bounds__(256) void mvec_set_col_kernel(double *__restrict__ X, int64_t n, int k, int j, const double *__restrict__ v) {
    const int64_t gs = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gs) X[i * k + j] = v[i];
}
__global__ __launch_bounds__(256) void mvec_get_col_kernel(double *__restrict__ v, const double *__restrict__ X, int64_t n, int k, int j) {
    const int64_t gs = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gs) v[i] = X[i * k + j];
}

inline int copy_grid(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 8192); }

// static names: one per (path, K, V, RP)
const char *spmm_name(bool rowblock, int k, int v, bool rp64) {
    static std::string names[2][kSpmmMaxK + 1][3][2];
    std::string &s = names[rowblock][k][v][rp64];
    if (s.empty())
        s = rowblock ? "spmm_rowblock_kernel K=" + std::to_string(k) + " V=" + std::to_string(v) + " RP=" + (rp64 ? "64" : "32")
                     : "spmm_lane_serial_kernel K=" + std::to_string(k) + " RP=" + (rp64 ? "64" : "32");
    return s.c_str();
}

template <typename RP, int K>
void launch_rowblock(bis_ctx *ctx, const bis_mat *A, const double *X, double *Y, int v, int cap, size_t lds) {
    if (v == 2)
        hipLaunchKernelGGL((spmm_rowblock_kernel<RP, K, (K % 2 == 0 ? 2 : 1)>), dim3(A->n_blocks), dim3(kSpmmT), lds, ctx->stream,
                           (const RP *)A->row_ptr, A->col, A->val, X, Y, A->blk_row, A->blk_nnz, A->n_blocks, cap, ctx->spmv_stop);
    else
        hipLaunchKernelGGL((spmm_rowblock_kernel<RP, K, 1>), dim3(A->n_blocks), dim3(kSpmmT), lds, ctx->stream,
                           (const RP *)A->row_ptr, A->col, A->val, X, Y, A->blk_row, A->blk_nnz, A->n_blocks, cap, ctx->spmv_stop);
}

template <typename RP>
void launch_rowblock_k(bis_ctx *ctx, const bis_mat *A, const double *X, double *Y, int k, int v, int cap, size_t lds) {
    switch (k) {
    case 2: launch_rowblock<RP, 2>(ctx, A, X, Y, v, cap, lds); break;
    case 3: launch_rowblock<RP, 3>(ctx, A, X, Y, v, cap, lds); break;
    case 4: launch_rowblock<RP, 4>(ctx, A, X, Y, v, cap, lds); break;
    case 5: launch_rowblock<RP, 5>(ctx, A, X, Y, v, cap, lds); break;
    case 6: launch_rowblock<RP, 6>(ctx, A, X, Y, v, cap, lds); break;
    case 7: launch_rowblock<RP, 7>(ctx, A, X, Y, v, cap, lds); break;
    default: launch_rowblock<RP, 8>(ctx, A, X, Y, v, cap, lds); break;
    }
}

} // namespace

bis_status bis_spmm_launch(bis_ctx *ctx, const bis_mat *A, const double *X, double *Y, int k) {
    if (A->n_rows == 0) return BIS_OK;
    bis_mat *Am = const_cast<bis_mat *>(A); // (the kernel's name is a note on the matrix, like spmv_kernel)
    if (k == 1) {
        if (bis_status st = bis_spmv_launch(ctx, A, X, Y, nullptr, nullptr)) return st;
        Am->spmm_kernel = "bis_spmv K=1";
        return BIS_OK;
    }
    const int cap = spmm_cap(k);
    const bool rowblock = A->blk_row && A->blk_nnz && A->max_row_nnz + 3 <= cap && A->chunk_nnz <= kSpmmMaxChunk;
    bis_prof_begin(ctx);
    if (rowblock) {
        const int v = (k % 2 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) ? 2 : 1;
        const size_t lds = sizeof(double) * (size_t)(cap + 4) * k + sizeof(int) * (size_t)(A->chunk_nnz + 2);
        if (A->rp64) launch_rowblock_k<int64_t>(ctx, A, X, Y, k, v, cap, lds);
        else launch_rowblock_k<int32_t>(ctx, A, X, Y, k, v, cap, lds);
        Am->spmm_kernel = spmm_name(true, k, v, A->rp64);
    } else {
        const int grid = (int)std::min<int64_t>((A->n_rows * k + 255) / 256, (int64_t)1 << 20);
        if (A->rp64)
            hipLaunchKernelGGL(spmm_lane_serial_kernel<int64_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int64_t *)A->row_ptr,
                               A->col, A->val, X, Y, A->n_rows, k, ctx->spmv_stop);
        else
            hipLaunchKernelGGL(spmm_lane_serial_kernel<int32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t *)A->row_ptr,
                               A->col, A->val, X, Y, A->n_rows, k, ctx->spmv_stop);
        Am->spmm_kernel = spmm_name(false, k, 0, A->rp64);
    }
    bis_prof_end(ctx);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

extern "C" {

bis_status bis_spmm(bis_ctx *ctx, const bis_mat *A, const double *X, double *Y, int n_rhs) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, A, "bis_spmm: null matrix");
    BIS_REQUIRE(ctx, n_rhs >= 1 && n_rhs <= kSpmmMaxK, "bis_spmm: n_rhs must be between 1 and 8");
    BIS_REQUIRE(ctx, A->n_rows == 0 || (X && Y), "bis_spmm: null X or Y");
    BIS_REQUIRE(ctx, A->n_rows == 0 || X != Y, "bis_spmm: X and Y must not alias");
    return bis_spmm_launch(ctx, A, X, Y, n_rhs);
}

const char *bis_mat_spmm_kernel(const bis_mat *A) { return A ? A->spmm_kernel : ""; }

bis_status bis_mat_spmm_streamed_bytes(const bis_mat *A, int n_rhs, int64_t *bytes) {
    if (!A || !bytes || n_rhs < 1 || n_rhs > kSpmmMaxK) return BIS_ERR_INVALID;
    *bytes = 12 * A->nnz + (A->rp64 ? 8 : 4) * (A->n_rows + 1) + (int64_t)8 * n_rhs * (A->n_cols + A->n_rows);
    return BIS_OK;
}

bis_status bis_mvec_set_col(bis_ctx *ctx, double *X, int64_t n, int n_rhs, int j, const double *v) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n >= 0 && n_rhs >= 1 && j >= 0 && j < n_rhs && (n == 0 || (X && v)), "bis_mvec_set_col: bad arguments");
    if (n == 0) return BIS_OK;
    hipLaunchKernelGGL(mvec_set_col_kernel, dim3(copy_grid(n)), dim3(256), 0, ctx->stream, X, n, n_rhs, j, v);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

bis_status bis_mvec_get_col(bis_ctx *ctx, double *v, const double *X, int64_t n, int n_rhs, int j) {
    BIS_CTX_OK(ctx);
    BIS_REQUIRE(ctx, n >= 0 && n_rhs >= 1 && j >= 0 && j < n_rhs && (n == 0 || (X && v)), "bis_mvec_get_col: bad arguments");
    if (n == 0) return BIS_OK;
    hipLaunchKernelGGL(mvec_get_col_kernel, dim3(copy_grid(n)), dim3(256), 0, ctx->stream, v, X, n, n_rhs, j);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}

} // extern "C"
