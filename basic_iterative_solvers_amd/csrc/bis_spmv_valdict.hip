// bis_spmv_valdict.hip -- the value dictionary (bis_valdict, bis_spmv_forms.hpp), its two kernels and the lane-per-row block build.
#include "bis_spmv_forms.hpp"

#include <algorithm>
#include <vector>

namespace {

// ---------------------------------------------------------------------------
// Value-dictionary variant.  A matrix with at most 256 distinct values (any
// constant-coefficient stencil: HPCG has two) keeps them in a 256-entry table;
// per non-zero the kernel streams a 2-byte column code and a 1-byte value code
// -- 3 instead of CRS's 12 bytes -- and takes the value from an LDS copy of the
// table.  The values are the CRS ones bit for bit, products, their order and
// the row sums are those of spmv_rowblock_kernel: same results to the last bit.
// The CRS arrays stay authoritative (download, split, triangular solves use
// them).  With a quarter of the bytes the kernel is no longer HBM-bound: what
// counts is the number of wave instructions and of L1 tag lookups per non-zero
// (profiles/r02_g_spmv_pmc_*), hence the form below.
// ---------------------------------------------------------------------------

// acc += prod[a] + ... + prod[z - 1], left to right (the reference's summation order), the LDS reads issued eight at a time
__device__ __forceinline__ void acc_row(const double *prod, int a, int z, double &acc) {
    int j = a;
    for (; j + 8 <= z; j += 8) {
        double p[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) p[q] = prod[j + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += p[q];
    }
    for (; j < z; ++j) acc += prod[j];
}

// Consecutive form: lane t of the workgroup takes non-zeros s + j*256 + t, so one gather instruction covers 64
// CONSECUTIVE non-zeros (2-3 rows of a stencil), the narrow stream loads (2 B + 1 B per lane) are fully coalesced, and
// the column window base comes from one cross-lane permute (lane j < 8 of every wave holds base j) instead of the
// select tree: 159 M vector-ALU wave instructions per HPCG-256 launch against 273 M for the 4-non-zeros-per-lane form
// with the select tree (0.62 against 0.70 ms; a persistent, software-pipelined variant of this form: 0.71 ms).
template <typename RP, int MODE>
__global__ __launch_bounds__(256) void spmv_rowblock_vd_kernel(
    const RP *__restrict__ row_ptr, const double *x, double *y, const int32_t *__restrict__ blk_row,
    const int64_t *__restrict__ blk_nnz, int n_blocks, int n_blocks_pad8, const double *w, double *partials,
    const uint16_t *__restrict__ pk, int64_t pk_base, const int32_t *__restrict__ seg_base, int col_max, const int *stop,
    const uint8_t *__restrict__ vcode, int64_t vd_base, const double *__restrict__ vdict) {
    constexpr int T = 256, J = 8;
    constexpr bool FUSE_DOT = MODE == 1;
    if (stop && stop[1]) return;
    extern __shared__ __attribute__((aligned(16))) double prod[];
    __shared__ double dict[256];
    const int b = n_blocks_pad8 > 0 ? xcd_remap(blockIdx.x, n_blocks_pad8)
                                    : (n_blocks_pad8 < -1 ? xcd_group_remap(blockIdx.x, -n_blocks_pad8) : (int)blockIdx.x);
    if (b >= n_blocks) return;
    dict[threadIdx.x] = vdict[threadIdx.x];
    const int r0 = blk_row[b], r1 = blk_row[b + 1];
    const int64_t s = blk_nnz[b], e = blk_nnz[b + 1];
    const int my_r = r0 + (int)threadIdx.x;
    RP rp_a = 0, rp_z = 0;
    if (my_r < r1) { rp_a = row_ptr[my_r]; rp_z = row_ptr[my_r + 1]; }
    const int lane_base = seg_base[(size_t)b * 8 + (threadIdx.x & 7)];
    const char *xb = reinterpret_cast<const char *>(x);
    const uint16_t *pkp = pk + (s - pk_base);
    const uint8_t *vcp = vcode + (s - vd_base);
    const int n = (int)(e - s);
    __syncthreads();
    for (int base = 0; base < n; base += J * T) {
        unsigned cc[J], vc[J];
        double xx[J], vv[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const unsigned idx = (unsigned)min(base + j * T + (int)threadIdx.x, n - 1); // 32-bit offsets: scalar base + vector offset addressing
            cc[j] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(pkp) + (idx << 1));
            vc[j] = *(vcp + idx);
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int wbase = __builtin_amdgcn_ds_bpermute((int)((cc[j] >> (kPkOffBits - 2)) & 28u), lane_base);
            xx[j] = x_at<false>(xb, wbase + (int)(cc[j] & (kPkSpan - 1)));
            vv[j] = dict[vc[j]];
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int idx = base + j * T + (int)threadIdx.x;
            double pr = vv[j] * xx[j];
            asm volatile("" : "+v"(pr));
            if (idx < n) prod[idx] = pr;
        }
    }
    __syncthreads();
    double dot_acc = 0.0;
    for (int r = my_r; r < r1; r += T) {
        if (r != my_r) { rp_a = row_ptr[r]; rp_z = row_ptr[r + 1]; }
        const int a = (int)((int64_t)rp_a - s), z = (int)((int64_t)rp_z - s);
        double acc = 0.0;
        acc_row(prod, a, z, acc);
        if (MODE == 2) y[r] = (w[r] - acc) / partials[r];
        else y[r] = acc;
        if (FUSE_DOT) dot_acc = fma(acc, w[r], dot_acc);
    }
    if (FUSE_DOT) {
        const double t = wave_sum(dot_acc);
        if ((threadIdx.x & 63) == 0) partials[(size_t)b * (T / 64) + (threadIdx.x >> 6)] = t;
    }
}

// Lane-per-row form of the dictionary kernel (same three epilogues): a workgroup takes 256 consecutive
// rows, copies their column and value codes into LDS with 16- and 8-byte vector loads (3 bytes per non-zero), and
// lane t then walks row t in CRS order, eight non-zeros at a time: code from LDS, window base by the cross-lane
// permute, x gathered -- neighbouring lanes are neighbouring rows, so for a stencil the 64 gathers of one instruction
// fall into consecutive x entries -- value from the table, acc += value * x (two roundings, like the product/sum
// passes of the other forms: bit-identical y).  No product round trip through LDS, one gather instruction per 64
// non-zeros as the only vector-memory instruction in the inner loop.
constexpr int kRmRows = 256;
constexpr int kRmMaxRow = 40; // LDS: 256 rows * 40 codes * 3 B = 30 KiB
static_assert(kRmRows == kSwRows, "bis_spmv_partials_bound: the lane-per-row form's blocks are the R = 1 case");

__device__ __forceinline__ int wave_max_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// DIAG: value code 255 stands for the row's own diagonal value vdiag[row] (matrices whose off-diagonal values are few
// but whose diagonal is not: Anderson's random potential).
// W32: the block's columns are coded against 32 windows of 2048 columns (lane j < 32 of every wave holds base j) instead
// of 8 windows of 8192: multi-colour-permuted matrices, whose rows reach into a dozen or more short column runs.
template <typename RP, int MODE, bool DIAG, bool W32>
__global__ __launch_bounds__(256) void spmv_rowmajor_vd_kernel(
    const RP *__restrict__ row_ptr, const double *x, double *y, int64_t n_rows, int n_blocks, int n_blocks_pad8,
    const double *w, double *partials, const uint16_t *__restrict__ pk, int64_t pk_base, const int32_t *__restrict__ seg_base,
    const int *stop, const uint8_t *__restrict__ vcode, int64_t vd_base, const double *__restrict__ vdict, int code_cap,
    const double *__restrict__ vdiag) {
    constexpr bool FUSE_DOT = MODE == 1;
    if (stop && stop[1]) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double dict[256];
    const int b = n_blocks_pad8 > 0 ? xcd_remap(blockIdx.x, n_blocks_pad8)
                                    : (n_blocks_pad8 < -1 ? xcd_group_remap(blockIdx.x, -n_blocks_pad8) : (int)blockIdx.x);
    if (b >= n_blocks) return;
    dict[threadIdx.x] = vdict[threadIdx.x];
    const int64_t r0 = (int64_t)b * kRmRows;
    const int rows = (int)min((int64_t)kRmRows, n_rows - r0);
    const int64_t s = (int64_t)row_ptr[r0], e = (int64_t)row_ptr[r0 + rows];
    const int64_t s8 = s & ~(int64_t)7;
    const int first = (int)(s - s8);  // LDS position of the block's first code
    const int n8 = (int)(e - s8);     // LDS positions [0, n8) get loaded (rounded up to whole vectors of 8)
    uint16_t *lpk = reinterpret_cast<uint16_t *>(lds_raw);
    uint8_t *lvc = lds_raw + 2 * (size_t)code_cap;
    {
        const uint4 *gpk = reinterpret_cast<const uint4 *>(pk + (s8 - pk_base));
        const uint2 *gvc = reinterpret_cast<const uint2 *>(vcode + (s8 - vd_base));
        for (int v = (int)threadIdx.x; v * 8 < n8; v += 256) {
            reinterpret_cast<uint4 *>(lpk)[v] = gpk[v];
            reinterpret_cast<uint2 *>(lvc)[v] = gvc[v];
        }
    }
    const bool mine = (int)threadIdx.x < rows;
    int a = first, len = 0;
    double dval = 0.0;
    if (mine) {
        const int64_t ra = (int64_t)row_ptr[r0 + threadIdx.x];
        a = (int)(ra - s8);
        len = (int)((int64_t)row_ptr[r0 + threadIdx.x + 1] - ra);
        if (DIAG) dval = vdiag[r0 + threadIdx.x];
    }
    constexpr int SEGS = W32 ? kPk3Segs : kPkSegs, OFFBITS = W32 ? kPk3OffBits : kPkOffBits;
    const int lane_base = seg_base[(size_t)b * SEGS + (threadIdx.x & (SEGS - 1))];
    const char *xb = reinterpret_cast<const char *>(x);
    __syncthreads();
    double acc = 0.0;
    const int wmax = __builtin_amdgcn_readfirstlane(wave_max_i(len)), wmin = __builtin_amdgcn_readfirstlane(wave_min_i(len)); // wave-uniform
    // eight entries of every row at a time: codes from LDS, window base, gather, table value ...
    auto issue = [&](int j0, double (&xx)[8], double (&vv)[8]) {
        const bool whole = j0 + 8 <= wmin; // every row of the wave has these eight entries
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            // ragged tail: lanes past their row's end re-read the block's first code; their product is dropped
            const int idx = (whole || j0 + q < len) ? a + j0 + q : first;
            const unsigned code = lpk[idx];
            const int wbase = __builtin_amdgcn_ds_bpermute((int)((code >> (OFFBITS - 2)) & (unsigned)((SEGS - 1) * 4)), lane_base);
            xx[q] = x_at<false>(xb, wbase + (int)(code & ((1u << OFFBITS) - 1)));
            const unsigned vcd = lvc[idx];
            vv[q] = dict[vcd];
            if (DIAG) vv[q] = vcd == 255u ? dval : vv[q];
        }
    };
    // ... and acc += value * x in CRS order
    auto consume = [&](int j0, const double (&xx)[8], const double (&vv)[8]) {
        if (j0 + 8 <= wmin) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                double pr = vv[q] * xx[q];
                asm volatile("" : "+v"(pr));
                acc += pr;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                double pr = vv[q] * xx[q];
                asm volatile("" : "+v"(pr));
                if (j0 + q < len) acc += pr;
            }
        }
    };
    // (issuing the next eight gathers before consuming the current eight -- sixteen in flight per lane -- was measured
    // slower: HPCG-256 0.513 against 0.476 ms, Anderson-256 0.246 against 0.197: the kernel is bound by the gather and
    // LDS instruction rates, not by latency)
    for (int j0 = 0; j0 < wmax; j0 += 8) {
        double xx[8], vv[8];
        issue(j0, xx, vv);
        consume(j0, xx, vv);
    }
    if (mine) y[r0 + threadIdx.x] = MODE == 2 ? (w[r0 + threadIdx.x] - acc) / partials[r0 + threadIdx.x] : acc; // MODE 2: one triangular-sweep level
    if (FUSE_DOT) {
        const double t = wave_sum(mine ? acc * w[r0 + threadIdx.x] : 0.0);
        if ((threadIdx.x & 63) == 0) partials[(size_t)b * 4 + (threadIdx.x >> 6)] = t;
    }
}

// rm_nnz[k] = row_ptr[min(256 k, n_rows)]
template <typename RP>
__global__ __launch_bounds__(256) void rm_blocks_kernel(const RP *__restrict__ row_ptr, int64_t n_rows, int n_blocks, int64_t *__restrict__ rm_nnz) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k <= n_blocks) rm_nnz[k] = (int64_t)row_ptr[min((int64_t)k * kRmRows, n_rows)];
}

// distinct values of val[s, e), one list per wave (a workgroup is one wave): lists[w * 257] = count (257 = more than
// 256, *overflow is raised and every wave stops), then the values' bit patterns
__global__ __launch_bounds__(64) void vd_collect_kernel(const double *__restrict__ val, int64_t s, int64_t e,
                                                        unsigned long long *__restrict__ lists, int *overflow) {
    __shared__ unsigned long long list[256];
    const int lane = threadIdx.x;
    int n = 0;
    for (int64_t k0 = s + (int64_t)blockIdx.x * 64; k0 < e && n <= 256; k0 += (int64_t)gridDim.x * 64) {
        if (__hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { n = 257; break; }
        const int64_t k = k0 + lane;
        const unsigned long long v = k < e ? (unsigned long long)__double_as_longlong(val[k]) : 0ull;
        bool found = k >= e;
        for (int j = 0; j < n && __ballot(!found); ++j) found |= list[j] == v;
        while (const unsigned long long open = __ballot(!found)) {
            const int leader = (int)__builtin_ctzll(open);
            const unsigned long long lv = __shfl(v, leader);
            if (n == 256) { n = 257; break; }
            if (lane == 0) list[n] = lv;
            ++n;
            found |= v == lv;
        }
        __syncthreads(); // one wave: orders the list writes before the next round's reads
    }
    if (n > 256 && lane == 0) atomicExch(overflow, 1);
    if (lane == 0) lists[(size_t)blockIdx.x * 257] = (unsigned long long)n;
    for (int j = lane; j < n && j < 256; j += 64) lists[(size_t)blockIdx.x * 257 + 1 + j] = list[j];
}

// Row-wise variants for the "dictionary + per-row diagonal" encoding: a lane per row, diagonal entries (col == row +
// row0) are left out of the dictionary.  *overflow: 1 = more than 255 distinct off-diagonal values, 2 = a row with more
// than one diagonal entry (its values could differ: not representable).
template <typename RP>
__global__ __launch_bounds__(64) void vd_collect_rows_kernel(const RP *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                             const double *__restrict__ val, int64_t n_rows, int64_t row0,
                                                             unsigned long long *__restrict__ lists, int *overflow) {
    __shared__ unsigned long long list[256];
    const int lane = threadIdx.x;
    int n = 0;
    for (int64_t rb = (int64_t)blockIdx.x * 64; rb < n_rows && n <= 255; rb += (int64_t)gridDim.x * 64) {
        if (__hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { n = 256; break; }
        const int64_t r = rb + lane;
        int64_t k = 0, k1 = 0;
        if (r < n_rows) { k = (int64_t)row_ptr[r]; k1 = (int64_t)row_ptr[r + 1]; }
        int n_diag = 0;
        while (__ballot(k < k1) && n <= 255) {
            bool found = true;
            unsigned long long v = 0;
            if (k < k1) {
                if ((int64_t)col[k] == r + row0) ++n_diag;
                else { v = (unsigned long long)__double_as_longlong(val[k]); found = false; }
                ++k;
            }
            for (int j = 0; j < n && __ballot(!found); ++j) found |= list[j] == v;
            while (const unsigned long long open = __ballot(!found)) {
                const int leader = (int)__builtin_ctzll(open);
                const unsigned long long lv = __shfl(v, leader);
                if (n == 255) { n = 256; break; }
                if (lane == 0) list[n] = lv;
                ++n;
                found |= v == lv;
            }
            __syncthreads();
        }
        if (__ballot(n_diag > 1)) { if (lane == 0) atomicExch(overflow, 2); n = 256; }
    }
    if (n > 255 && lane == 0) atomicCAS(overflow, 0, 1);
    if (lane == 0) lists[(size_t)blockIdx.x * 257] = (unsigned long long)n;
    for (int j = lane; j < n && j < 255; j += 64) lists[(size_t)blockIdx.x * 257 + 1 + j] = list[j];
}

template <typename RP>
__global__ __launch_bounds__(256) void vd_encode_rows_kernel(const RP *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                             const double *__restrict__ val, int64_t n_rows, int64_t row0, int64_t base,
                                                             const double *__restrict__ vdict, int n_dict, uint8_t *__restrict__ vcode,
                                                             double *__restrict__ vdiag) {
    __shared__ unsigned long long dict[256];
    dict[threadIdx.x] = (unsigned long long)__double_as_longlong(vdict[threadIdx.x]);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += stride) {
        double d = 0.0;
        for (int64_t k = (int64_t)row_ptr[r]; k < (int64_t)row_ptr[r + 1]; ++k) {
            if ((int64_t)col[k] == r + row0) { d = val[k]; vcode[k - base] = 255; continue; }
            const unsigned long long v = (unsigned long long)__double_as_longlong(val[k]);
            int lo = 0, hi = n_dict - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (dict[mid] < v) lo = mid + 1; else hi = mid;
            }
            vcode[k - base] = (uint8_t)lo;
        }
        vdiag[r] = d;
    }
}

// vcode[k - base] = index of val[k] in the (ascending) dictionary; four codes per thread, one 32-bit store
__global__ __launch_bounds__(256) void vd_encode_kernel(const double *__restrict__ val, int64_t s, int64_t e, int64_t base,
                                                        const double *__restrict__ vdict, int n_dict, uint8_t *__restrict__ vcode) {
    __shared__ unsigned long long dict[256];
    dict[threadIdx.x] = (unsigned long long)__double_as_longlong(vdict[threadIdx.x]);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    for (int64_t k4 = base + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; k4 < e; k4 += stride) {
        unsigned packed = 0;
        for (int q = 0; q < 4; ++q) {
            const int64_t k = k4 + q;
            if (k < s || k >= e) continue;
            const unsigned long long v = (unsigned long long)__double_as_longlong(val[k]);
            int lo = 0, hi = n_dict - 1; // the value is in the table
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (dict[mid] < v) lo = mid + 1; else hi = mid;
            }
            packed |= (unsigned)lo << (8 * q);
        }
        *reinterpret_cast<unsigned *>(vcode + (k4 - base)) = packed;
    }
}

template <typename RP, int MODE>
void launch_vd(const SpmvArgs &a) {
    hipLaunchKernelGGL((spmv_rowblock_vd_kernel<RP, MODE>), dim3(a.grid), dim3(256), a.lds_bytes, a.stream,
                       (const RP *)a.row_ptr, a.x, a.y, a.blk_row, a.blk_nnz, a.nb, a.remap_arg, a.w, a.partials, a.pk,
                       a.pk_base, a.seg_base, a.col_max, a.stop, a.vcode, a.vd_base, a.vdict);
}

// a dictionary that cannot be used after all: it goes, state -1, with everything a value change drops (bis_mat_values_changed)
void vd_give_up(bis_mat *A) {
    bis_spmv_valdict_drop(A);
    bis_spmv_sellwin_drop(A);
    bis_spmv_win8_drop(A);
    bis_spmv_colslab_drop(A);
    A->vd.state = -1;
}

} // namespace

bis_valdict::~bis_valdict() {
    hipFree(codes); hipFree(table); hipFree(diag_val);
    hipFree(rm_nnz);
    delete rm_pk;
}

void bis_spmv_valdict_drop(bis_mat *A) {
    delete A->vd.p;
    A->vd.p = nullptr;
    A->vd.state = 0;
}

void bis_spmv_valdict_launch_rowblock(const bis_mat *A, const SpmvArgs &a) {
    if (A->rp64) { if (a.mode == 2) launch_vd<int64_t, 2>(a); else if (a.mode == 1) launch_vd<int64_t, 1>(a); else launch_vd<int64_t, 0>(a); }
    else { if (a.mode == 2) launch_vd<int32_t, 2>(a); else if (a.mode == 1) launch_vd<int32_t, 1>(a); else launch_vd<int32_t, 0>(a); }
}

void bis_spmv_valdict_launch_rowmajor(const bis_mat *A, const SpmvArgs &a) {
    const bis_valdict *d = A->vd.p;
    const int code_cap = kRmRows * std::max(A->max_row_nnz, 1) + 16; // positions: a block's codes + the 8-alignment slack on both sides
    const size_t lds = 3 * (size_t)code_cap;
#define BIS_RM_LAUNCH3(RP, MODE, DIAG, W32)                                                                            \
    hipLaunchKernelGGL((spmv_rowmajor_vd_kernel<RP, MODE, DIAG, W32>), dim3(a.grid), dim3(256), lds, a.stream, (const RP *)A->row_ptr, a.x, a.y, \
                       A->n_rows, a.nb, a.remap_arg, a.w, a.partials, d->rm_pk->codes, d->rm_pk->base, d->rm_pk->seg, a.stop, d->codes, d->base, d->table, code_cap, \
                       d->diag_val)
#define BIS_RM_LAUNCH2(RP, MODE, DIAG) do { if (d->rm_pk->kind == 3) BIS_RM_LAUNCH3(RP, MODE, DIAG, true); else BIS_RM_LAUNCH3(RP, MODE, DIAG, false); } while (0)
#define BIS_RM_LAUNCH(RP, MODE) do { if (d->diag) BIS_RM_LAUNCH2(RP, MODE, true); else BIS_RM_LAUNCH2(RP, MODE, false); } while (0)
    if (A->rp64) { if (a.mode == 2) BIS_RM_LAUNCH(int64_t, 2); else if (a.mode == 1) BIS_RM_LAUNCH(int64_t, 1); else BIS_RM_LAUNCH(int64_t, 0); }
    else { if (a.mode == 2) BIS_RM_LAUNCH(int32_t, 2); else if (a.mode == 1) BIS_RM_LAUNCH(int32_t, 1); else BIS_RM_LAUNCH(int32_t, 0); }
#undef BIS_RM_LAUNCH
#undef BIS_RM_LAUNCH2
#undef BIS_RM_LAUNCH3
}

bis_status bis_spmv_valdict_try_rowmajor(bis_ctx *ctx, bis_mat *A) {
    bis_valdict *d = A->vd.state == 1 ? A->vd.p : nullptr;
    if (!d || d->rm_state != 0) return BIS_OK;
    d->rm_state = -1;
    if (A->n_rows == 0 || A->max_row_nnz > kRmMaxRow || A->n_cols >= ((int64_t)1 << 29)) return BIS_OK;
    const int64_t nb64 = (A->n_rows + kRmRows - 1) / kRmRows;
    if (nb64 > (int64_t)1 << 28) return BIS_OK;
    const int nb = (int)nb64;
    BIS_HIP_CHECK(ctx, hipMalloc(&d->rm_nnz, sizeof(int64_t) * (size_t)(nb + 1)));
    if (A->rp64) hipLaunchKernelGGL(rm_blocks_kernel<int64_t>, dim3((unsigned)(nb / 256 + 1)), dim3(256), 0, ctx->stream, (const int64_t *)A->row_ptr, A->n_rows, nb, d->rm_nnz);
    else hipLaunchKernelGGL(rm_blocks_kernel<int32_t>, dim3((unsigned)(nb / 256 + 1)), dim3(256), 0, ctx->stream, (const int32_t *)A->row_ptr, A->n_rows, nb, d->rm_nnz);
    BIS_HIP_CHECK(ctx, hipGetLastError());
    // whole 8-byte vectors of codes; no look before the build, and both window formats
    if (bis_status st = bis_colpack_build(ctx, A, d->rm_nnz, nb, 8, false, true, &d->rm_pk)) return st;
    // some block of 256 rows needs more column windows than either format has: the other kernels stay
    // (a base below the dictionary's: both are the first row's start rounded down, cannot happen)
    if (!d->rm_pk->kind || d->rm_pk->base < d->base) {
        hipFree(d->rm_nnz);
        delete d->rm_pk;
        d->rm_nnz = nullptr; d->rm_pk = nullptr;
        return BIS_OK;
    }
    d->rm_blocks = nb;
    d->rm_state = 1;
    return BIS_OK;
}

// distinct values of the matrix (plain), or of its off-diagonal entries (diag): at most `cap` bit patterns, ascending;
// *ok = false when there are more (or, diag, when a row has several diagonal entries)
static bis_status vd_collect(bis_ctx *ctx, const bis_mat *A, int64_t s, int64_t e, bool diag, std::vector<unsigned long long> *all, bool *ok) {
    *ok = false;
    all->clear();
    const size_t cap = diag ? 255 : 256;
    const int64_t units = diag ? A->n_rows : e - s;
    const int n_waves = (int)std::min<int64_t>((units + 63) / 64, (int64_t)ctx->n_cus * 8);
    unsigned long long *lists = nullptr;
    int *overflow = bis_slot_ptr(ctx, kSlotValdict);
    BIS_HIP_CHECK(ctx, hipMalloc(&lists, sizeof(unsigned long long) * 257 * (size_t)n_waves));
    hipError_t he = bis_slot_io(ctx, kSlotValdict, 1);
    if (he == hipSuccess) {
        if (!diag) hipLaunchKernelGGL(vd_collect_kernel, dim3(n_waves), dim3(64), 0, ctx->stream, A->val, s, e, lists, overflow);
        else if (A->rp64) hipLaunchKernelGGL(vd_collect_rows_kernel<int64_t>, dim3(n_waves), dim3(64), 0, ctx->stream, (const int64_t *)A->row_ptr, A->col, A->val, A->n_rows, A->view_row0, lists, overflow);
        else hipLaunchKernelGGL(vd_collect_rows_kernel<int32_t>, dim3(n_waves), dim3(64), 0, ctx->stream, (const int32_t *)A->row_ptr, A->col, A->val, A->n_rows, A->view_row0, lists, overflow);
        he = hipGetLastError();
    }
    std::vector<unsigned long long> h((size_t)257 * n_waves);
    int h_over = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(h.data(), lists, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess) he = bis_slot_io(ctx, kSlotValdict, 1, &h_over); // (synchronises: the lists have arrived too)
    hipFree(lists);
    BIS_HIP_CHECK(ctx, he);
    if (h_over) return BIS_OK;
    for (int w = 0; w < n_waves; ++w) {
        const size_t n = (size_t)h[(size_t)w * 257];
        if (n > cap) return BIS_OK;
        all->insert(all->end(), h.begin() + (size_t)w * 257 + 1, h.begin() + (size_t)w * 257 + 1 + n);
    }
    std::sort(all->begin(), all->end());
    all->erase(std::unique(all->begin(), all->end()), all->end());
    *ok = all->size() <= cap;
    return BIS_OK;
}

bis_status bis_spmv_try_valdict(bis_ctx *ctx, bis_mat *A, bool consecutive_ok) {
    if (A->vd.state != 0) return BIS_OK;
    A->vd.state = -1;
    if (A->nnz == 0 || A->n_blocks == 0) return BIS_OK;
    int64_t ends[2];
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&ends[0], A->blk_nnz, 8, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&ends[1], A->blk_nnz + A->n_blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t s = ends[0], e = ends[1];
    if (e <= s) return BIS_OK;
    std::vector<unsigned long long> all;
    bool ok = false, diag = false;
    if (bis_status st = vd_collect(ctx, A, s, e, false, &all, &ok)) return st;
    if (ok && all.empty()) ok = false;
    const bool rm_possible = spmv_valdict_mode() >= 2 && A->max_row_nnz <= kRmMaxRow && A->n_cols < ((int64_t)1 << 29);
    if (!consecutive_ok && !rm_possible) return BIS_OK;
    if (!ok && rm_possible) {
        // few values apart from the diagonal?  (served by the lane-per-row form only: a lane knows its row)
        if (bis_status st = vd_collect(ctx, A, s, e, true, &all, &ok)) return st;
        diag = ok;
    }
    if (!ok) return BIS_OK;
    unsigned long long table[256] = {};
    std::copy(all.begin(), all.end(), table);
    bis_valdict *d = A->vd.p = new bis_valdict;
    d->base = s & ~(int64_t)7; // whole 8-byte vectors of codes for the lane-per-row form
    const size_t n_code = (size_t)(e - d->base) + 16;
    hipError_t he = hipMalloc(&d->table, sizeof table);
    if (he == hipSuccess) he = hipMalloc(&d->codes, n_code);
    if (he == hipSuccess && diag) he = hipMalloc(&d->diag_val, sizeof(double) * (size_t)A->n_rows);
    if (he == hipSuccess) he = hipMemsetAsync(d->codes, 0, n_code, ctx->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d->table, table, sizeof table, hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess) {
        if (!diag) {
            const int grid = (int)std::min<int64_t>((e - d->base + 1023) / 1024, (int64_t)ctx->n_cus * 32);
            hipLaunchKernelGGL(vd_encode_kernel, dim3(grid), dim3(256), 0, ctx->stream, A->val, s, e, d->base, d->table, (int)all.size(), d->codes);
        } else {
            const int grid = (int)std::min<int64_t>((A->n_rows + 255) / 256, (int64_t)ctx->n_cus * 32);
            if (A->rp64) hipLaunchKernelGGL(vd_encode_rows_kernel<int64_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int64_t *)A->row_ptr, A->col, A->val, A->n_rows, A->view_row0, d->base, d->table, (int)all.size(), d->codes, d->diag_val);
            else hipLaunchKernelGGL(vd_encode_rows_kernel<int32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t *)A->row_ptr, A->col, A->val, A->n_rows, A->view_row0, d->base, d->table, (int)all.size(), d->codes, d->diag_val);
        }
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream); // table[] lives on this stack frame
    if (he != hipSuccess) {
        vd_give_up(A);
        BIS_HIP_CHECK(ctx, he);
    }
    d->n = (int)all.size();
    d->diag = diag;
    d->rm_only = diag || !consecutive_ok;
    A->vd.state = 1;
    if (d->rm_only) { // only the lane-per-row kernel can use it: does the matrix qualify?
        if (bis_status st = bis_spmv_valdict_try_rowmajor(ctx, A)) return st;
        if (d->rm_state != 1) vd_give_up(A);
    }
    return BIS_OK;
}
