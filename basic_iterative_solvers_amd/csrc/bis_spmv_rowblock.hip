// bis_spmv_rowblock.hip -- CRS SpMV for gfx950 (reference kernels.hpp:22-52): the row-block kernel, its launch tables and
// block map, and the wave-per-row fallback.  Which matrices run it: spmv_resolve (bis_spmv.hip).
//
// HBM-bound: algorithmic traffic 12*nnz + 20*N bytes (val 8 + col 4 per
// non-zero; row_ptr 4, x 8, y 8 per row).  Design ("row-block stream"):
//
//   * rows are grouped into row blocks of ~chunk non-zeros (bis_matrix.hip,
//     blk_row[]); one workgroup streams one block's contiguous val/col range
//     with 16-byte vector loads (4 non-zeros per lane per step) -- perfectly
//     coalesced regardless of row lengths -- gathers x[col] through L1/L2,
//     and parks the products in LDS;
//   * after one barrier each lane owns a row and sums that row's products
//     from LDS left to right (CRS storage order, like the reference's scalar
//     loop), then writes y coalesced;
//   * XCD-aware block map, fine-grained: workgroups are dealt round-robin to
//     the 8 XCDs, so within every window of 64 consecutive row blocks XCD j is
//     given the 8 consecutive blocks [8j, 8j+8) (neighbouring x-lines share one
//     L2) while all XCDs still stream ONE advancing window of val/col.  Giving
//     each XCD its own contiguous SLAB of the matrix -- the textbook map --
//     was measured 9 % slower (HPCG-256, same arrays: 1.109 ms slabs, 1.032
//     plain blockIdx order, 1.012 groups of 8): eight far-apart HBM streams
//     cost more than the x re-fetches they save, which the 256 MiB Infinity
//     Cache absorbs.  Option "spmv_xcd_remap": 0 none, 1 slabs, G>1 groups.
//
// An optional fused epilogue accumulates sum_r y[r]*w[r] (the (Ap,p) of
// cg.hpp:23) into per-wave partials so CG needs no separate dot pass; a third
// epilogue turns the kernel into one triangular-sweep step on a row range.
// Measurements, the PMC analysis of what bounds the kernel (L1->L2 request rate,
// 93 % of the streaming rate in fabric bytes) and the tuning record: DESIGN.md 4.
#include "bis_spmv_forms.hpp"

#include <algorithm>
#include <vector>

namespace {

template <int PK>
__device__ __forceinline__ int pk_decode(unsigned code, const int (&B)[8], int lane_base, int col_max) {
    int base;
    if (PK == 3) { // 32 windows of 2048 columns: window:5 | offset:11, lane j < 32 of every wave holds base j
        base = __builtin_amdgcn_ds_bpermute((int)((code >> (kPk3OffBits - 2)) & 124u), lane_base);
        return min(base + (int)(code & ((1u << kPk3OffBits) - 1)), col_max);
    }
    if (PK == 2) {
        base = __builtin_amdgcn_ds_bpermute((int)((code >> (kPkOffBits - 2)) & 28u), lane_base);
    } else {
        const bool b0 = code & (1u << kPkOffBits), b1 = code & (2u << kPkOffBits), b2 = code & (4u << kPkOffBits);
        const int a0 = b0 ? B[1] : B[0], a1 = b0 ? B[3] : B[2], a2 = b0 ? B[5] : B[4], a3 = b0 ? B[7] : B[6];
        const int c0 = b1 ? a1 : a0, c1 = b1 ? a3 : a2;
        base = b2 ? c1 : c0;
    }
    return min(base + (int)(code & (kPkSpan - 1)), col_max);
}

// T threads; U = 4-non-zero vectors staged per lane before the first use
// (all loads of a stage are in flight together); NT = nontemporal val/col
// loads (streamed once: keep them from evicting x out of L2).
// MODE 0: y = A x.  MODE 1: also partials[b] = sum y[r]*w[r] (CG's (Ap,p)).
// MODE 2: triangular-sweep epilogue for one dependency level given as a row
// range: y[r] = (w[r] - (A x)[r]) / dinv_or_d[r], i.e. x_level = (b - T x)/D
// (kernels.hpp:70,102); y may be the same array as x -- rows of one level do
// not reference each other.
// MODE 3: one Jacobi-Richardson step on a triangle (bis_itrsv.hip): y[r] = (w[r] - (A x)[r]) * dinv[r], the row sum
// exactly MODE 0's, subtraction and multiplication rounded separately; every row reads x, so y must not be x.
//
// PK != 0: the column stream is the packed one (2 B per non-zero): code =
// segment:3 | offset:13, column = seg_base[8*b + segment] + offset.  PK 1 picks
// the base with a select tree over 8 registers, PK 2 with one cross-lane
// permute (lane j < 8 of every wave holds base j).  Codes of the neighbouring
// blocks that share the first/last 4-aligned vector decode against the wrong
// bases: clamped to a valid column, their products are never read.
template <typename RP, int T, int U, int PK, int MODE, bool WIDE = false, int BR = 0>
__global__ __launch_bounds__(T) void spmv_rowblock_kernel(
    const RP *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *x, double *y,
    const int32_t *__restrict__ blk_row, const int64_t *__restrict__ blk_nnz, int n_blocks,
    int n_blocks_pad8, const double *w, double *partials, const uint16_t *__restrict__ pk,
    int64_t pk_base, const int32_t *__restrict__ seg_base, int col_max, const int *stop, int acc_y) {
    constexpr bool FUSE_DOT = MODE == 1;
    if (stop && stop[1]) return; // the solver has stopped: this launch is a no-op
    extern __shared__ __attribute__((aligned(16))) double prod[];
    const int b = n_blocks_pad8 > 0 ? xcd_remap(blockIdx.x, n_blocks_pad8)
                                    : (n_blocks_pad8 < -1 ? xcd_group_remap(blockIdx.x, -n_blocks_pad8) : (int)blockIdx.x);
    if (b >= n_blocks) return;
    // one dependent level only: row range and nnz range come from the block
    // table; the row_ptr entries phase 2 needs are fetched now, under phase 1
    const int r0 = blk_row[b], r1 = blk_row[b + 1];
    const int64_t s = blk_nnz[b], e = blk_nnz[b + 1];
    const int64_t s4 = s & ~(int64_t)3;
    const int my_r = r0 + (int)threadIdx.x;
    RP rp_a = 0, rp_z = 0;
    if (my_r < r1) { rp_a = row_ptr[my_r]; rp_z = row_ptr[my_r + 1]; }
    int segb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int lane_base = 0;
    if (PK == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) segb[i] = seg_base[(size_t)b * 8 + i];
    }
    if (PK == 2) lane_base = seg_base[(size_t)b * 8 + (threadIdx.x & 7)];
    if (PK == 3) lane_base = seg_base[(size_t)b * kPk3Segs + (threadIdx.x & (kPk3Segs - 1))];
    const char *xb = reinterpret_cast<const char *>(x);

    // phase 1: stream val/col, gather x, park products.  Branch-free up to the
    // LDS store: lanes past the block's end re-read its last vector (clamped
    // index), so every load and gather of all U stages is in flight before
    // the first use and the wave stays whole (the lane permute needs that).
    if (BR == 2) {
        // consecutive form: lane t of the workgroup takes non-zeros base + j*T + t, so
        // one gather instruction covers 64 consecutive non-zeros (neighbouring lanes
        // mostly share an x cache line); narrow (8 B / 4 B / 2 B) but fully coalesced
        // stream loads, conflict-free LDS stores.  No alignment slack: prod[k - s4]
        // keeps the index convention of the other forms.
        constexpr int J = 4 * U;
        for (int64_t base = s; base < e; base += (int64_t)J * T) {
            int cc[J];
            double vv[J], xx[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int64_t k = min(base + (int64_t)j * T + threadIdx.x, e - 1);
                if (PK) cc[j] = pk[k - pk_base];
                else cc[j] = col[k];
                vv[j] = val[k];
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (PK) cc[j] = pk_decode<PK>((unsigned)cc[j], segb, lane_base, col_max);
                xx[j] = x_at<WIDE>(xb, cc[j]);
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int64_t k = base + (int64_t)j * T + threadIdx.x;
                double pr = vv[j] * xx[j];
                asm volatile("" : "+v"(pr));
                if (k < e) prod[k - s4] = pr;
            }
        }
    } else if (BR == 1) { // staged, predicated form (each stage waits for its own gathers)
        for (int64_t k0 = s4 + 4 * (int64_t)threadIdx.x; k0 < e; k0 += 4 * T * U) {
            v4i c[U];
            v4us pc[U];
            v2d va[U], vb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = k0 + (int64_t)u * 4 * T;
                if (k < e) {
                    if (PK) pc[u] = *reinterpret_cast<const v4us *>(pk + (k - pk_base));
                    else c[u] = *reinterpret_cast<const v4i *>(col + k);
                    va[u] = *reinterpret_cast<const v2d *>(val + k);
                    vb[u] = *reinterpret_cast<const v2d *>(val + k + 2);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = k0 + (int64_t)u * 4 * T;
                if (k < e) {
                    if (PK) {
                        c[u].x = pk_decode<PK>(pc[u].x, segb, lane_base, col_max);
                        c[u].y = pk_decode<PK>(pc[u].y, segb, lane_base, col_max);
                        c[u].z = pk_decode<PK>(pc[u].z, segb, lane_base, col_max);
                        c[u].w = pk_decode<PK>(pc[u].w, segb, lane_base, col_max);
                    }
                    va[u].x *= x[c[u].x];
                    va[u].y *= x[c[u].y];
                    vb[u].x *= x[c[u].z];
                    vb[u].y *= x[c[u].w];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = k0 + (int64_t)u * 4 * T;
                if (k < e) {
                    v2d *dst = reinterpret_cast<v2d *>(prod + (k - s4));
                    dst[0] = va[u];
                    dst[1] = vb[u];
                }
            }
        }
    } else {
    const int64_t k_last = (e - 1) & ~(int64_t)3;
    for (int64_t base = s4; base < e; base += 4 * T * U) {
        v4i c[U];
        v4us pc[U];
        v2d va[U], vb[U];
        double xv[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = min(base + 4 * (int64_t)threadIdx.x + (int64_t)u * 4 * T, k_last);
            if (PK) pc[u] = *reinterpret_cast<const v4us *>(pk + (k - pk_base));
            else c[u] = *reinterpret_cast<const v4i *>(col + k);
            va[u] = *reinterpret_cast<const v2d *>(val + k);
            vb[u] = *reinterpret_cast<const v2d *>(val + k + 2);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (PK) {
                c[u].x = pk_decode<PK>(pc[u].x, segb, lane_base, col_max);
                c[u].y = pk_decode<PK>(pc[u].y, segb, lane_base, col_max);
                c[u].z = pk_decode<PK>(pc[u].z, segb, lane_base, col_max);
                c[u].w = pk_decode<PK>(pc[u].w, segb, lane_base, col_max);
            }
            xv[u][0] = x_at<WIDE>(xb, c[u].x);
            xv[u][1] = x_at<WIDE>(xb, c[u].y);
            xv[u][2] = x_at<WIDE>(xb, c[u].z);
            xv[u][3] = x_at<WIDE>(xb, c[u].w);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = base + 4 * (int64_t)threadIdx.x + (int64_t)u * 4 * T;
            double p0 = va[u].x * xv[u][0], p1 = va[u].y * xv[u][1];
            double p2 = vb[u].x * xv[u][2], p3 = vb[u].y * xv[u][3];
            // pin the products here: otherwise the val loads sink into the
            // predicated store below and leave the load stage
            asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
            if (k < e) {
                v2d *dst = reinterpret_cast<v2d *>(prod + (k - s4));
                dst[0] = v2d{p0, p1};
                dst[1] = v2d{p2, p3};
            }
        }
    }
    }
    __syncthreads();

    // phase 2: one lane per row, left-to-right sum in CRS order
    double dot_acc = 0.0;
    for (int r = my_r; r < r1; r += T) {
        if (r != my_r) { rp_a = row_ptr[r]; rp_z = row_ptr[r + 1]; }
        const int a = (int)((int64_t)rp_a - s4), z = (int)((int64_t)rp_z - s4);
        // (acc_y: this launch is a later column slab of the matrix -- bis_spmv_slab.hip -- and continues the row's sum where the
        // slab before it left it in y)
        double acc = (MODE < 2 && acc_y) ? y[r] : 0.0;
        for (int j = a; j < z; ++j) acc += prod[j];
        if (MODE == 3) // (b and 1/D are streamed once: non-temporal, like the elementwise kernels' operands)
            y[r] = __dmul_rn(__dsub_rn(__builtin_nontemporal_load(w + r), acc), __builtin_nontemporal_load(partials + r));
        else if (MODE == 2) y[r] = (w[r] - acc) / partials[r];
        else y[r] = acc;
        if (FUSE_DOT) dot_acc = fma(acc, w[r], dot_acc);
    }
    if (FUSE_DOT) { // one partial per wave (no workgroup barrier): kSpmvWaves per row block
        const double t = wave_sum(dot_acc);
        if ((threadIdx.x & 63) == 0) partials[(size_t)b * (T / 64) + (threadIdx.x >> 6)] = t;
    }
}

// Fallback for rows longer than the LDS budget: one wave per row.
template <typename RP>
__global__ __launch_bounds__(256) void spmv_wave_per_row_kernel(
    const RP *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ x, double *__restrict__ y,
    int64_t n_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t r = wave; r < n_rows; r += n_waves) {
        double acc = 0.0;
        for (int64_t k = (int64_t)row_ptr[r] + lane; k < (int64_t)row_ptr[r + 1]; k += 64)
            acc = fma(val[k], x[col[k]], acc);
        acc = wave_sum(acc);
        if (lane == 0) y[r] = acc;
    }
}

template <typename RP, int T, int U, int BR = 0>
void launch_variant(const SpmvArgs &a) {
#define BIS_LV(PK, MODE)                                                                          \
    hipLaunchKernelGGL((spmv_rowblock_kernel<RP, T, U, (PK) < 0 ? 0 : (PK), MODE, (PK) < 0, BR>), dim3(a.grid), dim3(T), a.lds_bytes, \
                       a.stream, (const RP *)a.row_ptr, a.col, a.val, a.x, a.y, a.blk_row, a.blk_nnz, \
                       a.nb, a.remap_arg, a.w, a.partials, a.pk, a.pk_base, a.seg_base, a.col_max, a.stop, a.acc_y)
#define BIS_LVM(PK)                                                                               \
    do {                                                                                          \
        if (a.mode == 3) BIS_LV(PK, 3);                                                           \
        else if (a.mode == 2) BIS_LV(PK, 2);                                                      \
        else if (a.mode == 1) BIS_LV(PK, 1);                                                      \
        else BIS_LV(PK, 0);                                                                       \
    } while (0)
    if (a.wide) BIS_LVM(-1);
    else if (a.pk_mode == 1) BIS_LVM(1);
    else if (a.pk_mode == 2) BIS_LVM(2);
    else if (a.pk_mode == 3) BIS_LVM(3);
    else BIS_LVM(0);
#undef BIS_LVM
#undef BIS_LV
}
// variant id: 10/20/40 = 256 threads with U = 1/2/4 staged vectors per lane
// (tuning knob BIS_SPMV_VARIANT)
template <typename RP>
bool launch_by_id(int id, const SpmvArgs &a) {
    switch (id) {
    case 10: launch_variant<RP, 256, 1>(a); return true;
    case 20: launch_variant<RP, 256, 2>(a); return true;
    case 40: launch_variant<RP, 256, 4>(a); return true;
    case 11: launch_variant<RP, 256, 1, 1>(a); return true;
    case 21: launch_variant<RP, 256, 2, 1>(a); return true;
    case 41: launch_variant<RP, 256, 4, 1>(a); return true;
    case 12: launch_variant<RP, 256, 1, 2>(a); return true;
    case 22: launch_variant<RP, 256, 2, 2>(a); return true;
    default: return false;
    }
}

} // namespace

// Default: the branch-free 2-stage form with the packed stream, the staged 4-deep form with 32-bit columns.  Tuning
// history (tools/spmv_ab.py, same arrays, interleaved rounds, HPCG-256):
// chunk 1024 1.019 ms | 1280 1.026 | 1536 1.047 | 2048 1.084 | 4096 1.100;
// 128-thread blocks 1.10; a lane-per-row "row-major" phase 2 (fma order) 1.23-1.30;
// a persistent, software-pipelined grid 1.23-1.48; 64 consecutive non-zeros per
// gather instruction (8/4-byte loads) 1.23; nontemporal val/col loads +10 %.
int spmv_variant(const SpmvArgs &a) {
    const int v = bis_opts().spmv_variant >= 0 ? bis_opts().spmv_variant : (a.pk_mode ? 20 : 41);
    return (a.pk_mode >= 2 && v % 10 != 0) ? 20 : v; // the lane-permute decodes need the whole wave: branch-free form only
}

// Names bis_mat_spmv_kernel reports: static strings, built once, so that a launch only stores a pointer.
// The row-block kernel's instance as launch_by_id picks it: U staged vectors, PK the column stream (WIDE: 32-bit columns,
// 64-bit x addressing), BR the phase-1 form.  nullptr for an id launch_by_id does not know.
const char *rowblock_name(int id, const SpmvArgs &a) {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (int u : {1, 2, 4})
            for (int pk = 0; pk < 5; ++pk)
                for (int br = 0; br < 3; ++br)
                    v.push_back("spmv_rowblock_kernel U=" + std::to_string(u) + " PK=" + (pk == 4 ? std::string("0 WIDE") : std::to_string(pk)) +
                                " BR=" + std::to_string(br));
        return v;
    }();
    const int u = id / 10 == 1 ? 0 : (id / 10 == 2 ? 1 : 2), br = id % 10;
    static const int known[] = {10, 20, 40, 11, 21, 41, 12, 22}; // (launch_by_id's)
    if (std::find(std::begin(known), std::end(known), id) == std::end(known)) return nullptr;
    const int pk = a.wide ? 4 : a.pk_mode;
    return names[(size_t)(u * 5 + pk) * 3 + br].c_str();
}

bool bis_spmv_rowblock_launch(bool rp64, int id, const SpmvArgs &a) { return rp64 ? launch_by_id<int64_t>(id, a) : launch_by_id<int32_t>(id, a); }

void bis_spmv_longrows_launch(bis_ctx *ctx, const bis_mat *A, const double *x, double *y) {
    const int grid = (int)std::min<int64_t>((A->n_rows + 3) / 4, 8192);
    if (A->rp64) hipLaunchKernelGGL(spmv_wave_per_row_kernel<int64_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int64_t *)A->row_ptr, A->col, A->val, x, y, A->n_rows);
    else hipLaunchKernelGGL(spmv_wave_per_row_kernel<int32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t *)A->row_ptr, A->col, A->val, x, y, A->n_rows);
}

// The block map of nb logical blocks (shared with the forms of bis_spmv_sellwin.hip and bis_spmv_win8.hip).  Kernel argument:
// nb rounded up to 8 = XCD slabs, -1 = blockIdx order, -G = groups of G; default: groups of 8 (HPCG-256: 1.012 ms vs 1.032
// blockIdx order vs 1.109 slabs).  Grid: a whole number of windows so that every logical block id < nb is produced.
int bis_spmv_remap_arg(int nb) {
    const int r = bis_opts().spmv_xcd_remap < 0 ? 8 : bis_opts().spmv_xcd_remap;
    return r == 1 ? (nb + 7) & ~7 : (r > 1 ? -r : -1);
}
int bis_spmv_grid(int nb) {
    const int remap_arg = bis_spmv_remap_arg(nb), w = remap_arg < -1 ? 8 * -remap_arg : 8;
    return (nb + w - 1) / w * w;
}
