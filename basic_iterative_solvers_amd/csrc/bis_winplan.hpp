// bis_winplan.hpp -- what the two window + sliced-ELL forms share: the dictionary forms of bis_spmv_sellwin.hip (sellwin fmt 0-3,
// the row masks) and win8 / win4 of bis_spmv_win8.hip.  gfx950 only.
//
// Both cut the matrix into blocks of kSwRows R rows, copy the x entries a block reads into LDS (its WINDOW) and stream, slice by
// slice (64 rows = one wave), chunks of 4 entries per row whose column codes are slots of that window.  The window is a list of
// RUNS of consecutive 8-column granules (64 bytes of x).  A block's header is two rows of words, one word per run and row (32
// runs per block in the dictionary forms, 64 in win8; unused runs are 0):
//   row 0: the run's first granule;
//   row 1: (rank of that granule in the window) | (granules of the run) << 16, at most kSwRunGran granules per run.
// LDS behind the window's base: 16 bytes whose first 8 hold -0.0 (the padding's slot), then granule `rank` at byte 64 rank.
#pragma once

#include "bis_internal.hpp"

// The plan both forms are built on.  bis_sellwin (bis_spmv_sellwin.hip) and bis_win8 (bis_spmv_win8.hip) add their streams.
struct bis_winplan {
    int n_blocks = 0;
    int64_t n_slices = 0, total_chunks = 0;
    int32_t *hdr = nullptr;          // [n_blocks * 2 * runs]: the blocks' headers (above)
    int64_t *slice_chunk0 = nullptr; // [n_slices + 1]
    int32_t *own_rank = nullptr;     // [n_blocks] rank (in the window) of the granule of the block's first row's OWN column (row + view_row0) when the
                                     // own columns of all the block's rows lie in the window side by side, else -1: the fused dot then takes w from LDS
    int max_gran = 0;                // largest window of a block, in granules
    int R = 1;                       // rows per lane: a block is 256 R rows
};

constexpr int kSwRunGran = 64; // granules per run at most
constexpr int kSwHash = 4096;
constexpr int kSwMaxGran = 940; // window <= (2 + 8 * 940) * 8 = 60176 bytes (list[1024] in the plan kernels, 13-bit slots in the joint codes)

__host__ __device__ inline int win_run_word(int rank, int granules) { return rank | (granules << 16); }
__host__ __device__ inline int win_run_rank(int word) { return word & 0xffff; }
__host__ __device__ inline int win_run_granules(int word) { return word >> 16; }

// The chunk offsets of the slices from their chunk counts: slice_chunk0[0 .. ns] = the exclusive scan of slice_chunks[0 .. ns] as
// 64-bit numbers, *total = slice_chunk0[ns], read back: the stream is synchronized, so earlier asynchronous read-backs on it have
// arrived too.  Frees its own temporary on every path.  (bis_spmv_sellwin.hip)
hipError_t bis_winplan_scan(const int32_t *slice_chunks, int64_t *slice_chunk0, int64_t ns, int64_t *total, hipStream_t stream);

// the logical block of this workgroup under the caller's block map (bis_spmv_remap_arg); >= the number of blocks: nothing to do
__device__ __forceinline__ int win_block(int remap_arg) {
    return remap_arg > 0 ? xcd_remap(blockIdx.x, remap_arg)
                         : (remap_arg < -1 ? xcd_group_remap(blockIdx.x, -remap_arg) : (int)blockIdx.x);
}

// The window copy of the SpMV kernels: runs 0 .. N_RUNS - 1 of the block, whose header words lane k of G_WORD and lane R_LANE0 + k
// of R_WORD hold, from X (N_COLS entries) to WIN = the window's base + 16.  A run has at most 256 pieces of 16 bytes; wave WV
// takes 64 of them and the hardware writes them to LDS behind the wave-uniform base (LDS-DMA: no register staging, nothing
// waited for here); where X is not 16-byte aligned (X_AL16 false) or the piece straddles the end of X, two guarded loads and an
// LDS store.  A macro, not a function: the kernels' code must not depend on where the inliner meets the loop (an inlined
// function came out with the loop's exit test inverted in every kernel).
#define WIN_COPY_RUNS(X, N_COLS, X_AL16, WIN, WV, LANE, N_RUNS, G_WORD, R_WORD, R_LANE0)                                   \
    for (int k = 0; k < (N_RUNS); ++k) {                                                                                   \
        const int g0 = __builtin_amdgcn_readlane(G_WORD, k);                                                               \
        const int w2 = __builtin_amdgcn_readlane(R_WORD, (R_LANE0) + k);                                                   \
        const int rank = w2 & 0xffff, n_pieces = (w2 >> 16) * 4;                                                           \
        const int j = ((WV) + k) & 3;                                                                                      \
        const int p = j * 64 + (LANE);                                                                                     \
        const int64_t c = (int64_t)g0 * 8 + 2 * p;                                                                         \
        unsigned char *dst = (WIN) + (size_t)rank * 64 + (size_t)j * 1024;                                                 \
        if (p < n_pieces) {                                                                                                \
            if ((X_AL16) && c + 1 < (N_COLS)) {                                                                            \
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((X) + c),                \
                                                 (__attribute__((address_space(3))) void *)dst, 16, 0, 0);                 \
            } else {                                                                                                       \
                double2 v;                                                                                                 \
                v.x = c < (N_COLS) ? (X)[c] : 0.0;                                                                         \
                v.y = c + 1 < (N_COLS) ? (X)[c + 1] : 0.0;                                                                 \
                *reinterpret_cast<double2 *>(dst + (LANE) * 16) = v;                                                       \
            }                                                                                                              \
        }                                                                                                                  \
    }

// The granule set of a block, for the plan kernels (256 threads, all of them call): the 8-column granules of col[s .. e) into
// the LDS hash set `table`, compacted into `list` and sorted ascending (bitonic).  Returns their number, or -1 where there are
// more than max_gran (wave-uniform: every thread gets the same answer).  *cnt and *failed are the caller's LDS words.
__device__ inline int win_granule_set(const int32_t *__restrict__ col, int64_t s, int64_t e, int max_gran, int (&table)[kSwHash],
                                      int (&list)[1024], int *cnt, int *failed) {
    const int tid = threadIdx.x;
    for (int i = tid; i < kSwHash; i += 256) table[i] = -1;
    if (tid == 0) { *cnt = 0; *failed = 0; }
    __syncthreads();
    for (int64_t k = s + tid; k < e; k += 256) {
        if (__hip_atomic_load(failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        const int g = col[k] >> 3;
        unsigned h = ((unsigned)g * 2654435761u) >> 20;
        for (;;) {
            const int cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == g) break;
            if (cur == -1) {
                const int old = atomicCAS(&table[h], -1, g);
                if (old == -1) {
                    if (atomicAdd(cnt, 1) >= max_gran) atomicExch(failed, 1);
                    break;
                }
                if (old == g) break;
            }
            h = (h + 1) & (kSwHash - 1);
        }
    }
    __syncthreads();
    const int n = *cnt;
    if (*failed || n > max_gran) return -1;
    __syncthreads();
    if (tid == 0) *cnt = 0;
    __syncthreads();
    for (int i = tid; i < kSwHash; i += 256) {
        const int g = table[i];
        if (g != -1) list[atomicAdd(cnt, 1)] = g;
    }
    int P = 2;
    while (P < n) P <<= 1;
    __syncthreads();
    for (int i = n + tid; i < P; i += 256) list[i] = INT32_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int o = i ^ j;
                if (o > i) {
                    const int a = list[i], c = list[o];
                    if ((a > c) == ((i & k) == 0)) { list[i] = c; list[o] = a; }
                }
            }
            __syncthreads();
        }
    return n;
}
