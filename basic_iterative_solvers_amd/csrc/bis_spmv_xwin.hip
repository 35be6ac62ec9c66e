// bis_spmv_xwin.hip -- the opt-in x-window form of the row-block SpMV (spmv_window = 1).  Analysis (once per matrix): for
// every row block, the sorted list of the 16-column tiles of x its non-zeros reference (<= 128
// tiles) and, per non-zero, a 16-bit offset into that window.  The SpMV then
//   phase 0  copies the block's x tiles into LDS with coalesced loads (each x
//            entry once per block instead of one L1 gather per non-zero),
//   phase 1  streams val (8 B) + offset (2 B) -- 10 B per non-zero instead of
//            CRS's 12 -- and takes x from LDS,
//   phase 2  sums rows from LDS as before.
// Products, their order and the row sums are those of the CRS kernel; the CRS
// arrays stay authoritative (download, split, triangular solves use them).
// A matrix with a block touching more than 64 tiles keeps the gather kernel.
#include "bis_spmv_forms.hpp"

// per row block the sorted list of 16-column tiles of x it touches, and per non-zero a 16-bit offset into that window
// (replaces the 32-bit col in the SpMV stream)
struct bis_xwin {
    uint16_t *loc = nullptr;     // [nnz_range + pad], index k - loc_base
    int32_t *tiles = nullptr;    // [n_blocks * kWinMaxTiles]
    int32_t *tile_cnt = nullptr; // [n_blocks]
    int64_t loc_base = 0;
    int max_tiles = 0;
    ~bis_xwin() { hipFree(loc); hipFree(tiles); hipFree(tile_cnt); }
};

namespace {

constexpr int kHash = 512;

template <typename RP>
__global__ __launch_bounds__(256) void window_build_kernel(
    const int32_t *__restrict__ col, const int64_t *__restrict__ blk_nnz, int n_blocks,
    int64_t loc_base, uint16_t *__restrict__ loc, int32_t *__restrict__ tiles,
    int32_t *__restrict__ tile_cnt, int *__restrict__ status /* [0]=overflow flag, [1]=max tiles */) {
    __shared__ int htab[kHash];
    __shared__ int list[kWinMaxTiles], sorted[kWinMaxTiles];
    __shared__ int cnt, overflow;
    const int b = blockIdx.x;
    if (b >= n_blocks) return;
    const int64_t s = blk_nnz[b], e = blk_nnz[b + 1];
    for (int i = threadIdx.x; i < kHash; i += 256) htab[i] = -1;
    if (threadIdx.x == 0) { cnt = 0; overflow = 0; }
    __syncthreads();
    for (int64_t k = s + threadIdx.x; k < e; k += 256) {
        const int tile = col[k] / kWinTile;
        unsigned h = ((unsigned)tile * 2654435761u) >> 23; // 9 bits -> kHash
        for (int probe = 0; probe < kHash; ++probe) {
            const int old = atomicCAS(&htab[h], -1, tile);
            if (old == tile) break;
            if (old == -1) {
                const int slot = atomicAdd(&cnt, 1);
                if (slot < kWinMaxTiles) list[slot] = tile; else overflow = 1;
                break;
            }
            h = (h + 1) & (kHash - 1);
            if (probe == kHash - 1) overflow = 1;
        }
    }
    __syncthreads();
    if (overflow) {
        if (threadIdx.x == 0) { tile_cnt[b] = -1; atomicExch(&status[0], 1); }
        return;
    }
    const int n = cnt;
    if ((int)threadIdx.x < n) { // rank sort of distinct values
        const int v = list[threadIdx.x];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += list[j] < v;
        sorted[rank] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < n) tiles[(size_t)b * kWinMaxTiles + threadIdx.x] = sorted[threadIdx.x];
    if (threadIdx.x == 0) { tile_cnt[b] = n; atomicMax(&status[1], n); }
    for (int64_t k = s + threadIdx.x; k < e; k += 256) {
        const int c = col[k], tile = c / kWinTile;
        int lo = 0, hi = n - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted[mid] < tile) lo = mid + 1; else hi = mid; }
        loc[k - loc_base] = (uint16_t)(lo * kWinTile + (c - tile * kWinTile));
    }
}

template <typename RP, int T, int U, bool FUSE_DOT>
__global__ __launch_bounds__(T) void spmv_window_kernel(
    const RP *__restrict__ row_ptr, const uint16_t *__restrict__ loc, int64_t loc_base,
    const double *__restrict__ val, const double *__restrict__ x, double *__restrict__ y,
    const int32_t *__restrict__ blk_row, const int64_t *__restrict__ blk_nnz,
    const int32_t *__restrict__ tiles, const int32_t *__restrict__ tile_cnt, int64_t n_cols,
    int xw_doubles, int n_blocks, int n_blocks_pad8, const double *__restrict__ w,
    double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *xw = smem;                // [xw_doubles]  x window
    double *prod = smem + xw_doubles; // products
    const int b = n_blocks_pad8 > 0 ? xcd_remap(blockIdx.x, n_blocks_pad8) : (int)blockIdx.x;
    if (b >= n_blocks) return;
    const int r0 = blk_row[b], r1 = blk_row[b + 1];
    const int64_t s = blk_nnz[b], e = blk_nnz[b + 1];
    const int64_t s4 = s & ~(int64_t)3;
    const int nt = tile_cnt[b];
    const int my_r = r0 + (int)threadIdx.x;
    RP rp_a = 0, rp_z = 0;
    if (my_r < r1) { rp_a = row_ptr[my_r]; rp_z = row_ptr[my_r + 1]; }

    // issue the first stage of the val/offset stream before the window fill
    v4us lc[U];
    v2d va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t k = s4 + 4 * (int64_t)threadIdx.x + (int64_t)u * 4 * T;
        if (k < e) {
            lc[u] = *reinterpret_cast<const v4us *>(loc + (k - loc_base));
            va[u] = *reinterpret_cast<const v2d *>(val + k);
            vb[u] = *reinterpret_cast<const v2d *>(val + k + 2);
        }
    }
    // phase 0: x tiles -> LDS (coalesced 128 B per tile)
    for (int i = threadIdx.x; i < nt * kWinTile; i += T) {
        const int64_t c = (int64_t)tiles[(size_t)b * kWinMaxTiles + (i >> kWinTileLog)] * kWinTile + (i & (kWinTile - 1));
        xw[i] = c < n_cols ? x[c] : 0.0;
    }
    __syncthreads();
    // phase 1
    for (int64_t k0 = s4 + 4 * (int64_t)threadIdx.x; k0 < e; k0 += 4 * T * U) {
        if (k0 != s4 + 4 * (int64_t)threadIdx.x) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = k0 + (int64_t)u * 4 * T;
                if (k < e) {
                    lc[u] = *reinterpret_cast<const v4us *>(loc + (k - loc_base));
                    va[u] = *reinterpret_cast<const v2d *>(val + k);
                    vb[u] = *reinterpret_cast<const v2d *>(val + k + 2);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + (int64_t)u * 4 * T;
            if (k < e) {
                // elements before s / after e in the 4-aligned vector belong to a
                // neighbouring block (or the padding): their offsets are not for
                // this window -- clamp, the products are never read
                const int lim = nt * kWinTile - 1;
                va[u].x *= xw[min((int)lc[u].x, lim)];
                va[u].y *= xw[min((int)lc[u].y, lim)];
                vb[u].x *= xw[min((int)lc[u].z, lim)];
                vb[u].y *= xw[min((int)lc[u].w, lim)];
                v2d *dst = reinterpret_cast<v2d *>(prod + (k - s4));
                dst[0] = va[u];
                dst[1] = vb[u];
            }
        }
    }
    __syncthreads();
    // phase 2: one lane per row, left-to-right sum in CRS order
    double dot_acc = 0.0;
    for (int r = my_r; r < r1; r += T) {
        if (r != my_r) { rp_a = row_ptr[r]; rp_z = row_ptr[r + 1]; }
        const int a = (int)((int64_t)rp_a - s4), z = (int)((int64_t)rp_z - s4);
        double acc = 0.0;
        for (int j = a; j < z; ++j) acc += prod[j];
        y[r] = acc;
        if (FUSE_DOT) dot_acc = fma(acc, w[r], dot_acc);
    }
    if (FUSE_DOT) { // one partial per wave (no workgroup barrier): kSpmvWaves per row block
        const double t = wave_sum(dot_acc);
        if ((threadIdx.x & 63) == 0) partials[(size_t)b * (T / 64) + (threadIdx.x >> 6)] = t;
    }
}

} // namespace

void bis_spmv_xwin_drop(bis_mat *A) {
    delete A->xw;
    A->xw = nullptr;
}

bis_status bis_spmv_build_window(bis_ctx *ctx, bis_mat *A) {
    bis_spmv_xwin_drop(A);
    if (!spmv_window_mode() || A->nnz == 0 || A->n_rows == 0) return BIS_OK;
    if ((int64_t)A->chunk_nnz + A->max_row_nnz + 8 > 6144) return BIS_OK; // LDS: products + 16 KiB window <= 64 KiB
    std::unique_ptr<bis_xwin> w(new bis_xwin);
    const int nb = A->n_blocks;
    int64_t ends[2];
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&ends[0], A->blk_nnz, 8, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&ends[1], A->blk_nnz + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    w->loc_base = ends[0] & ~(int64_t)3;
    const size_t n_loc = (size_t)(ends[1] - w->loc_base) + 16;
    BIS_HIP_CHECK(ctx, hipMalloc(&w->loc, sizeof(uint16_t) * n_loc));
    BIS_HIP_CHECK(ctx, hipMalloc(&w->tiles, sizeof(int32_t) * (size_t)nb * kWinMaxTiles));
    BIS_HIP_CHECK(ctx, hipMalloc(&w->tile_cnt, sizeof(int32_t) * (size_t)nb));
    BIS_HIP_CHECK(ctx, hipMemsetAsync(w->loc, 0, sizeof(uint16_t) * n_loc, ctx->stream));
    int *status = bis_slot_ptr(ctx, kSlotXwin);
    BIS_HIP_CHECK(ctx, bis_slot_io(ctx, kSlotXwin, 2));
    if (A->rp64) hipLaunchKernelGGL(window_build_kernel<int64_t>, dim3(nb), dim3(256), 0, ctx->stream, A->col, A->blk_nnz, nb, w->loc_base, w->loc, w->tiles, w->tile_cnt, status);
    else hipLaunchKernelGGL(window_build_kernel<int32_t>, dim3(nb), dim3(256), 0, ctx->stream, A->col, A->blk_nnz, nb, w->loc_base, w->loc, w->tiles, w->tile_cnt, status);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    int h[2] = {0, 0};
    BIS_HIP_CHECK(ctx, bis_slot_io(ctx, kSlotXwin, 2, h));
    if (h[0]) return BIS_OK; // some block touches too many tiles: keep the gather kernel, drop the structure
    w->max_tiles = h[1];
    A->xw = w.release();
    return BIS_OK;
}

void bis_spmv_xwin_launch(const bis_mat *A, const SpmvArgs &a) {
    const bis_xwin *xw = A->xw;
    const int xw_doubles = ((xw->max_tiles * kWinTile) + 1) & ~1;
    const size_t lds_win = a.lds_bytes + sizeof(double) * (size_t)xw_doubles;
#define BIS_WIN_LAUNCH(RP, FUSE)                                                                   \
    hipLaunchKernelGGL((spmv_window_kernel<RP, 256, 2, FUSE>), dim3(a.nb8), dim3(256), lds_win,    \
                       a.stream, (const RP *)A->row_ptr, xw->loc, xw->loc_base, A->val, a.x, a.y,  \
                       A->blk_row, A->blk_nnz, xw->tiles, xw->tile_cnt, A->n_cols, xw_doubles, a.nb, \
                       bis_opts().spmv_xcd_remap > 0 ? a.nb8 : -1, a.w, a.partials)
    if (A->rp64) { if (a.w) BIS_WIN_LAUNCH(int64_t, true); else BIS_WIN_LAUNCH(int64_t, false); }
    else { if (a.w) BIS_WIN_LAUNCH(int32_t, true); else BIS_WIN_LAUNCH(int32_t, false); }
#undef BIS_WIN_LAUNCH
}
