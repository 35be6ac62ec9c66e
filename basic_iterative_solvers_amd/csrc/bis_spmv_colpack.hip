// bis_spmv_colpack.hip -- packed columns: a 16-bit code per non-zero against the column windows of its block (bis_colpack,
// bis_spmv_forms.hpp).  One build for the row-block tables' streams and for the dictionary's lane-per-row blocks.
#include "bis_spmv_forms.hpp"

namespace {

// Packed-column analysis, one workgroup per row block: cover the block's
// columns greedily with windows [base, base + 8192) taken at the smallest
// uncovered column (so the bases come out ascending); more than 8 windows ->
// the matrix keeps the 32-bit column stream.
template <int SEGS, int OFFBITS>
__global__ __launch_bounds__(256) void pk_build_kernel(const int32_t *__restrict__ col,
                                                       const int64_t *__restrict__ blk_nnz, int n_blocks,
                                                       int64_t pk_base, uint16_t *__restrict__ pk,
                                                       int32_t *__restrict__ seg_base, int *__restrict__ status) {
    constexpr int SPAN = 1 << OFFBITS;
    __shared__ int base[SEGS];
    __shared__ int cur;
    const int b = blockIdx.x;
    if (b >= n_blocks) return;
    const int64_t s = blk_nnz[b], e = blk_nnz[b + 1];
    int n_seg = 0;
    for (int sg = 0; sg <= SEGS; ++sg) {
        if (threadIdx.x == 0) cur = INT32_MAX;
        __syncthreads();
        int m = INT32_MAX;
        for (int64_t k = s + threadIdx.x; k < e; k += 256) {
            const int c = col[k];
            bool covered = false;
            for (int i = 0; i < sg; ++i) covered |= (c >= base[i] && c - base[i] < SPAN);
            if (!covered) m = min(m, c);
        }
        if (m != INT32_MAX) atomicMin(&cur, m);
        __syncthreads();
        const int found = cur;
        __syncthreads();
        if (found == INT32_MAX) break;
        if (sg == SEGS) { // one window too many
            if (threadIdx.x == 0) atomicExch(&status[0], 1);
            return;
        }
        if (threadIdx.x == 0) base[sg] = found;
        n_seg = sg + 1;
        __syncthreads();
    }
    if (threadIdx.x < SEGS) seg_base[(size_t)b * SEGS + threadIdx.x] = (int)threadIdx.x < n_seg ? base[threadIdx.x] : 0;
    for (int64_t k = s + threadIdx.x; k < e; k += 256) {
        const int c = col[k];
        int sg = 0;
        for (int i = 1; i < n_seg; ++i) sg += base[i] <= c; // ascending bases: last one not above c
        pk[k - pk_base] = (uint16_t)((sg << OFFBITS) | (c - base[sg]));
    }
}

// A cheap look before pk_build_kernel: a window of SPAN columns overlaps at most two SPAN-aligned buckets, so a block whose
// entries fall into more than 2 * SEGS distinct buckets cannot be covered by SEGS windows.  64 blocks spread over the matrix
// are looked at (one pass each, a bitmap in LDS); if one of them proves the failure, the build -- up to SEGS + 1 passes over
// EVERY block before it gives up -- is skipped: a matrix without locality (`unstr:80,80,80` as generated, its triangles, its
// column slabs: 23 failing builds, 16.5 ms) is told so at once.  The build's own answer is never changed, only anticipated.
template <int SEGS, int OFFBITS>
__global__ __launch_bounds__(256) void pk_probe_kernel(const int32_t *__restrict__ col, const int64_t *__restrict__ blk_nnz, int n_blocks,
                                                       int n_words, int *__restrict__ status) {
    extern __shared__ unsigned bitmap[];
    __shared__ int s_count;
    const int b = (int)(((int64_t)blockIdx.x * n_blocks) / gridDim.x);
    for (int i = threadIdx.x; i < n_words; i += 256) bitmap[i] = 0u;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int64_t s = blk_nnz[b], e = blk_nnz[b + 1];
    for (int64_t k = s + threadIdx.x; k < e; k += 256) {
        const unsigned bucket = min((unsigned)col[k] >> OFFBITS, (unsigned)n_words * 32u - 1u);
        atomicOr(&bitmap[bucket >> 5], 1u << (bucket & 31u));
    }
    __syncthreads();
    int c = 0;
    for (int i = threadIdx.x; i < n_words; i += 256) c += __popc(bitmap[i]);
    if (c) atomicAdd(&s_count, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_count > 2 * SEGS) atomicExch(status, 1);
}

} // namespace

bis_colpack::~bis_colpack() { hipFree(codes); hipFree(seg); }

// *out: the stream, or -- kind 0 -- what is left of a build that found no format: the caller deletes either.  Null after an error.
bis_status bis_colpack_build(bis_ctx *ctx, const bis_mat *A, const int64_t *tab, int nb, int align, bool probe, bool try32, bis_colpack **out) {
    *out = nullptr;
    std::unique_ptr<bis_colpack> p(new bis_colpack);
    int64_t ends[2];
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&ends[0], tab, 8, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipMemcpyAsync(&ends[1], tab + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    BIS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    p->base = ends[0] & ~(int64_t)(align - 1);
    const size_t n_pk = (size_t)(ends[1] - p->base) + 16;
    BIS_HIP_CHECK(ctx, hipMalloc(&p->codes, sizeof(uint16_t) * n_pk));
    BIS_HIP_CHECK(ctx, hipMalloc(&p->seg, sizeof(int32_t) * (size_t)nb * kPk3Segs));
    int *status = bis_slot_ptr(ctx, kSlotColpack);
    // format 1: 8 windows of 8192 columns (select-tree decode); format 3: 32 windows of 2048 columns (lane-permute decode) for
    // matrices whose rows reach into many short column runs, e.g. after a multi-colour reordering
    for (int kind = 1; kind <= (try32 ? 3 : 1); kind += 2) {
        int h = 0;
        BIS_HIP_CHECK(ctx, bis_slot_io(ctx, kSlotColpack, 1));
        if (probe && nb >= 256 && A->n_cols > 0) { // (the look before the build, see pk_probe_kernel)
            const int offbits = kind == 1 ? kPkOffBits : kPk3OffBits;
            const int n_words = (int)((((A->n_cols - 1) >> offbits) + 32) / 32);
            if ((size_t)n_words * 4 <= 48 * 1024) {
                if (kind == 1) hipLaunchKernelGGL((pk_probe_kernel<kPkSegs, kPkOffBits>), dim3(64), dim3(256), (size_t)n_words * 4, ctx->stream, A->col, tab, nb, n_words, status);
                else hipLaunchKernelGGL((pk_probe_kernel<kPk3Segs, kPk3OffBits>), dim3(64), dim3(256), (size_t)n_words * 4, ctx->stream, A->col, tab, nb, n_words, status);
                BIS_HIP_CHECK(ctx, bis_slot_io(ctx, kSlotColpack, 1, &h));
                if (h) continue; // this window format cannot hold the matrix
            }
        }
        BIS_HIP_CHECK(ctx, hipMemsetAsync(p->codes, 0, sizeof(uint16_t) * n_pk, ctx->stream));
        if (kind == 1) hipLaunchKernelGGL((pk_build_kernel<kPkSegs, kPkOffBits>), dim3(nb), dim3(256), 0, ctx->stream, A->col, tab, nb, p->base, p->codes, p->seg, status);
        else hipLaunchKernelGGL((pk_build_kernel<kPk3Segs, kPk3OffBits>), dim3(nb), dim3(256), 0, ctx->stream, A->col, tab, nb, p->base, p->codes, p->seg, status);
        BIS_HIP_CHECK(ctx, hipGetLastError());
        BIS_HIP_CHECK(ctx, bis_slot_io(ctx, kSlotColpack, 1, &h));
        if (!h) { p->kind = kind; break; }
    }
    *out = p.release();
    return BIS_OK;
}

bis_status bis_spmv_try_pack(bis_ctx *ctx, bis_mat *A, int t) {
    auto &s = A->pk[t];
    if (s.state != 0) return BIS_OK;
    s.state = -1;
    if (A->nnz == 0 || A->n_cols >= ((int64_t)1 << 29)) return BIS_OK;
    // (the 32-window format is opt-in here: measured no gain)
    if (bis_status st = bis_colpack_build(ctx, A, t ? A->blkf_nnz : A->blk_nnz, t ? A->n_blocks_f : A->n_blocks, 4, true, bis_opts().spmv_packed32 > 0, &s.p)) return st;
    if (s.p->kind) s.state = 1;
    else { delete s.p; s.p = nullptr; }
    return BIS_OK;
}

void bis_spmv_colpack_drop(bis_mat *A) {
    for (auto &s : A->pk) { delete s.p; s.p = nullptr; s.state = 0; }
}
