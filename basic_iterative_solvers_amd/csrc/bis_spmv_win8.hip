// bis_spmv_win8.hip -- CRS SpMV (kernels.hpp:22-42 of the reference), the block's x window in LDS and the values in a
// sliced-ELL stream: "win8", and "win4" with 4-byte values.  gfx950 only.
//
// win8: the SAME window + sliced-ELL plan as the dictionary forms' (bis_spmv_sellwin.hip; what the two share is
// bis_winplan.hpp) for matrices with ARBITRARY values (round 5).  Per non-zero the kernel streams the
// 8-byte CRS value and a 2-byte window slot -- 10 bytes, like the packed row-block kernel of bis_spmv_rowblock.hip -- but x comes
// from the block's LDS window (every entry once per block, by LDS-DMA) instead of one 8-byte gather per non-zero through
// the texture path, a lane owns a row (no product staging in LDS, no row_ptr, no second pass), and the stream is laid out
// in the order the lanes consume it: a chunk = 4 entries of each of the 64 rows of a slice = 2560 contiguous bytes
// [64 x (4 x 16-bit slot)][64 x 2 values][64 x 2 values], read with one 8-byte and two 16-byte non-temporal loads per lane.
// Entry j of a row is entry j of the CRS row; product and sum are rounded separately, in CRS order: y is bit-identical to
// the other kernels'.  Padding: value 1.0 at the slot that holds -0.0.  The CRS arrays stay authoritative (the stream is a
// lossless re-layout of val, built on the device at the first SpMV and dropped when values change).
// Usable by any matrix whose blocks of 256 R rows read at most 64 runs / 60 KB of x (runs a few granules apart are merged: banded /
// stencil orderings, RCM-ordered meshes); the rows of a block are taken in order of their length (w8_plan_kernel), so rows of
// very different lengths do not pad each other (refused beyond 12 % padding).
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>

// (the scan of the slices' slot records.  It stays here, not behind bis_winplan_scan: with rocprim's kernels in the unit the
// compiler keeps __shfl_down's width a variable until it is inlined, and the MODE 1 kernels' wave_sum the code it had in the
// single file -- docs/EXPERIMENTS.md section 36)
#include <rocprim/rocprim.hpp>

#include "bis_winplan.hpp"

struct bis_win8 : bis_winplan {
    // ONE buffer (placement search and swaps move it whole).  Today's layout: [total_chunks + 1] chunks of slots and values.  With
    // implied slots: the values, 256 vb bytes per chunk, then at byte w8_desc the [total_chunks + 1] 8-byte chunk descriptors (4 slot
    // bases of the chunk's entries), then at byte w8_side the [expl_chunks] 512-byte slot records of the chunks of explicit slices;
    // w8_end bytes in all
    unsigned char *stream = nullptr;
    void *own_stream = nullptr;       // the library's own stream while a debugging caller has redirected `stream` (bis_mat_win8_debug_stream)
    size_t w8_desc = 0, w8_side = 0, w8_end = 0;
    uint16_t *row_of = nullptr;       // [n_blocks * 256 R] row (in its block) of every position of the block's length order
    int64_t *slice_rec = nullptr;     // implied slots: [n_slices + 1] slot record of each slice's first chunk (exclusive scan); null: today's layout
    int64_t expl_chunks = 0;          // implied slots: chunks that keep their slots (total_chunks when the layout is today's)
    int64_t win_gran_sum = 0;         // granules of all the blocks' windows (x bytes a launch copies into LDS / 64)
    int tune_trials = 0;              // placement tuning at build time (re-allocations tried), the kernel's time on the first
    double tune_first_ms = 0.0, tune_kept_ms = 0.0; // allocation and on the one kept
    int vb = 8;                       // bytes per streamed value (4: the float stream of a matrix whose values are exact in binary32, "win4")
};

namespace {

constexpr int kW8ChunkBytes = 2560;
constexpr int kW8ValBytes = 2048; // a chunk of the implied-slot layout: its values only
// win4: the same chunks with 4-byte values (VT = float): [64 x 4 slots][64 x 4 floats] = 1536 bytes, 1024 with implied slots
template <typename VT> constexpr int w8_chunk_bytes() { return 512 + 256 * (int)sizeof(VT); }
template <typename VT> constexpr int w8_val_bytes() { return 256 * (int)sizeof(VT); }
static_assert(w8_chunk_bytes<double>() == kW8ChunkBytes && w8_val_bytes<double>() == kW8ValBytes, "the 8-byte stream's chunk sizes");
inline size_t w8_chunk_bytes(int vb) { return 512 + 256 * (size_t)vb; }
inline size_t w8_val_bytes(int vb) { return 256 * (size_t)vb; }

constexpr int kW8Runs = 64;     // runs of the window per block at most (header: 2 x 64 words)
constexpr int kW8GapMerge = 4;  // runs at most this many granules apart become one (the gap's x entries are copied too)

// win8's own plan, one workgroup per block of 256 R rows:
//  * the 8-column granules of x the block reads (LDS hash set, bitonic sort), cut into runs of consecutive granules; runs at most
//    kW8GapMerge granules apart are MERGED (an RCM-ordered mesh reads many short runs with small gaps: 34 raw runs per 1024-row
//    block become 23), runs of more than 64 granules split (a wave copies 64 x 64 bytes per instruction); at most kW8Runs runs
//    and max_gran granules (gaps included), else status[0] = 1;
//  * the block's rows SORTED BY LENGTH, longest first (stable: equal lengths keep their order), 64 sorted positions = one slice:
//    a slice is padded to ITS longest row, so rows of very different lengths no longer pad each other (FEM-like rows of 18-81
//    entries: 19 % padding -> 4 %).  row_of[b * 256 R + position] = row in the block; own_rank[b] >= 0 only where the order is
//    the identity (every row as long as the first, or already descending) and the own columns lie in the window side by side.
template <typename RP>
__global__ __launch_bounds__(256) void w8_plan_kernel(const RP *__restrict__ row_ptr, const int32_t *__restrict__ col, int64_t n_rows, int R,
                                                      int max_gran, int64_t row0, int32_t *__restrict__ hdr, int32_t *__restrict__ slice_chunks,
                                                      int32_t *__restrict__ own_rank, uint16_t *__restrict__ row_of, int *status) {
    __shared__ int table[kSwHash];
    __shared__ int list[1024];
    __shared__ int keys[1024]; // (length << 10 | 1023 - row) of the block's rows: descending order = longest first, equal lengths by row
    __shared__ int cnt, failed, n_out, win_gran, own_s, ident;
    __shared__ int out_g0[kW8Runs], out_rk[kW8Runs];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = (int64_t)b * kSwRows * R;
    const int rows = (int)min((int64_t)kSwRows * R, n_rows - r0);
    const int cap = kSwRows * R; // 256, 512 or 1024
    if (tid == 0) { n_out = 0; win_gran = 0; own_s = -1; ident = 1; }
    __syncthreads();
    // rows by length
    for (int i = tid; i < 1024; i += 256) {
        int len = -1; // (positions past the block's rows sort behind every row)
        if (i < rows) len = (int)((int64_t)row_ptr[r0 + i + 1] - (int64_t)row_ptr[r0 + i]);
        keys[i] = i < cap ? ((min(len, (1 << 20) - 1) + 1) << 10 | (1023 - i)) : -1;
    }
    __syncthreads();
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < 1024; i += 256) {
                const int o = i ^ j;
                if (o > i) {
                    const int a = keys[i], c = keys[o];
                    if ((a < c) == ((i & k) == 0)) { keys[i] = c; keys[o] = a; } // descending
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < cap; i += 256) {
        const int row = 1023 - (keys[i] & 1023);
        row_of[(size_t)b * cap + i] = (uint16_t)row;
        if (row != i) atomicExch(&ident, 0);
        if ((i & 63) == 0) { // first (= longest) row of slice i / 64
            const int len = (keys[i] >> 10) - 1;
            const int ch = len > 0 ? (len + 3) >> 2 : 0;
            slice_chunks[(size_t)b * 4 * R + (i >> 6)] = ch;
            atomicMax(&status[5], ch);
        }
    }
    const int n = win_granule_set(col, (int64_t)row_ptr[r0], (int64_t)row_ptr[r0 + rows], max_gran, table, list, &cnt, &failed);
    if (n < 0) {
        if (tid == 0) atomicExch(&status[0], 1);
        return;
    }
    if (tid == 0) { // one thread walks the sorted granules: merge, split, rank (a setup kernel: ~n steps)
        int m = 0, rank = 0; // runs emitted, granules of the window so far (gaps included)
        int i = 0;
        bool ok = true;
        const int64_t c_first = r0 + row0, c_last = c_first + rows - 1;
        const int g_first = (int)(c_first >> 3), g_last = (int)(c_last >> 3);
        int own = -1;
        while (i < n && ok) {
            const int g0 = list[i];
            int g1 = g0; // last granule of the merged run
            ++i;
            while (i < n && list[i] - g1 <= kW8GapMerge + 1) { g1 = list[i]; ++i; }
            const int len = g1 - g0 + 1;
            if ((c_first & 7) == 0 && g0 <= g_first && g_last <= g1) own = rank + (g_first - g0);
            for (int o = 0; o < len && ok; o += kSwRunGran) {
                if (m >= kW8Runs) { ok = false; break; }
                out_g0[m] = g0 + o;
                out_rk[m] = win_run_word(rank + o, min(kSwRunGran, len - o));
                ++m;
            }
            rank += len;
            if (rank > max_gran) ok = false;
        }
        if (!ok) atomicExch(&failed, 1);
        n_out = m;
        win_gran = rank;
        own_s = own;
    }
    __syncthreads();
    if (failed) {
        if (tid == 0) atomicExch(&status[0], 1);
        return;
    }
    if (tid < 2 * kW8Runs) {
        const int k = tid % kW8Runs;
        int word = 0;
        if (k < n_out) word = tid < kW8Runs ? out_g0[k] : out_rk[k];
        hdr[(size_t)b * 2 * kW8Runs + tid] = word;
    }
    if (tid == 0) {
        own_rank[b] = ident ? own_s : -1;
        atomicMax(&status[1], win_gran);
        atomicAdd(reinterpret_cast<unsigned *>(&status[2]), (unsigned)win_gran);
    }
}

// The stream, one wave per slice.  PHASE 0: today's layout, 2560-byte chunks [64 x 4 slots][64 x 2 values][64 x 2 values].
// PHASE 1: classify the slices (no stream written): slice_rec[s] = 0 where slice s is IMPLICIT -- its 64 positions hold real rows
// of one length, and for every entry j, slot(row, j) - 8 (row - block_row0) (bytes) is the same in all 64 lanes -- else its chunks.
// PHASE 2 (slice_rec = the exclusive scan of PHASE 1): the implied-slot layout, 2048-byte chunks of values only; an implicit slice's
// chunk keeps its 4 slot bases (16 bits each, the lane's 8 (row - block_row0) is added modulo 2^16 by the kernel; 1 = a padding
// entry, slot 0 in every lane) in desc[chunk], an explicit slice's chunk keeps its 512 bytes of slots in side[slice_rec[s] + k].
// VT = float (win4): the values are written as binary32, one 16-byte store of a lane's four -- exact on a matrix that
// bis_mat_round_f32 flagged, the only ones that get this stream; the padding value is 1.0f.
template <typename RP, int PHASE, typename VT = double>
__global__ __launch_bounds__(256) void w8_fill_kernel(const RP *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                      int64_t n_rows, int R, const int32_t *__restrict__ hdr,
                                                      const int64_t *__restrict__ slice_chunk0, const uint16_t *__restrict__ row_of,
                                                      unsigned char *__restrict__ stream, int64_t *__restrict__ slice_rec,
                                                      uint2 *__restrict__ desc, unsigned char *__restrict__ side) {
    __shared__ int g0s[kW8Runs], rk[kW8Runs];
    __shared__ int nr_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < kW8Runs) {
        g0s[tid] = hdr[(size_t)b * 2 * kW8Runs + tid];
        const int w2 = hdr[(size_t)b * 2 * kW8Runs + kW8Runs + tid];
        rk[tid] = w2 & 0xffff;
        const unsigned long long m = __ballot((w2 >> 16) != 0);
        if (tid == 0) nr_s = __popcll(m);
    }
    __syncthreads();
    const int nr = nr_s;
    for (int rr = 0; rr < R; ++rr) {
        const int64_t slice = ((int64_t)b * 4 + wv) * R + rr;
        const int64_t pos = slice * 64 + lane; // position in the block's length order
        const int in_block = row_of[pos];
        const int64_t r = (int64_t)b * kSwRows * R + in_block;
        int64_t rs = 0;
        int len = 0;
        if (r < n_rows) {
            rs = (int64_t)row_ptr[r];
            len = (int)((int64_t)row_ptr[r + 1] - rs);
        }
        const int64_t c0 = slice_chunk0[slice];
        const int nch = (int)(slice_chunk0[slice + 1] - c0);
        bool implicit = false; // (wave-uniform)
        if (PHASE == 1) implicit = __ballot(r < n_rows && len == __builtin_amdgcn_readfirstlane(len)) == ~0ull;
        if (PHASE == 2) implicit = slice_rec[slice + 1] == slice_rec[slice];
        for (int c = 0; c < nch && (PHASE != 1 || implicit); ++c) {
            unsigned cc[4];
            double vv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 4 * c + q;
                cc[q] = 0;      // the -0.0 slot
                vv[q] = 1.0;    // 1.0 * -0.0 = -0.0: acc + -0.0 == acc for every acc
                if (j < len) {
                    const int ci = col[rs + j];
                    const int g = ci >> 3;
                    int lo = 0, hi = nr - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (g0s[mid] <= g) lo = mid; else hi = mid - 1;
                    }
                    cc[q] = (unsigned)(2 + (rk[lo] + (g - g0s[lo])) * 8 + (ci & 7)) * 8u; // byte offset of the slot behind the window's base
                    if (PHASE != 1) vv[q] = val[rs + j];
                }
            }
            unsigned base[4]; // (implicit slices: one length, so an entry is padding in all lanes or in none)
#pragma unroll
            for (int q = 0; q < 4; ++q) base[q] = 4 * c + q < len ? (cc[q] - 8u * (unsigned)in_block) & 0xffffu : 1u;
            if (PHASE == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (__ballot(base[q] != (unsigned)__builtin_amdgcn_readfirstlane((int)base[q])) != 0ull) implicit = false;
            } else if (PHASE == 0) {
                unsigned char *p = stream + (size_t)(c0 + c) * w8_chunk_bytes<VT>();
                *reinterpret_cast<uint2 *>(p + lane * 8) = make_uint2(cc[0] | cc[1] << 16, cc[2] | cc[3] << 16);
                if constexpr (sizeof(VT) == 4) {
                    *reinterpret_cast<float4 *>(p + 512 + lane * 16) = make_float4((float)vv[0], (float)vv[1], (float)vv[2], (float)vv[3]);
                } else {
                    *reinterpret_cast<double2 *>(p + 512 + lane * 16) = make_double2(vv[0], vv[1]);
                    *reinterpret_cast<double2 *>(p + 1536 + lane * 16) = make_double2(vv[2], vv[3]);
                }
            } else {
                unsigned char *p = stream + (size_t)(c0 + c) * w8_val_bytes<VT>();
                if constexpr (sizeof(VT) == 4) {
                    *reinterpret_cast<float4 *>(p + lane * 16) = make_float4((float)vv[0], (float)vv[1], (float)vv[2], (float)vv[3]);
                } else {
                    *reinterpret_cast<double2 *>(p + lane * 16) = make_double2(vv[0], vv[1]);
                    *reinterpret_cast<double2 *>(p + 1024 + lane * 16) = make_double2(vv[2], vv[3]);
                }
                if (!implicit) *reinterpret_cast<uint2 *>(side + (size_t)(slice_rec[slice] + c) * 512 + lane * 8) = make_uint2(cc[0] | cc[1] << 16, cc[2] | cc[3] << 16);
                else if (lane == 0) desc[c0 + c] = make_uint2(base[0] | base[1] << 16, base[2] | base[3] << 16);
            }
        }
        if (PHASE == 1 && lane == 0) slice_rec[slice] = implicit ? 0 : nch;
    }
}

typedef double w8_v2d __attribute__((ext_vector_type(2)));
typedef unsigned w8_v2u __attribute__((ext_vector_type(2)));
typedef float w8_v4f __attribute__((ext_vector_type(4)));
template <typename VT> struct W8Chunk { w8_v2u code; w8_v2d v0, v1; };
template <> struct W8Chunk<float> { w8_v2u code; w8_v4f v; }; // win4: a lane's four values are ONE 16-byte load

// one chunk of the stream for this lane: three non-temporal loads (the stream is read once per product); win4: two
template <typename VT>
__device__ __forceinline__ W8Chunk<VT> w8_load(const unsigned char *__restrict__ stream, int64_t c, int lane) {
    const unsigned char *p = stream + (size_t)c * w8_chunk_bytes<VT>();
    W8Chunk<VT> ch;
    ch.code = __builtin_nontemporal_load(reinterpret_cast<const w8_v2u *>(p + lane * 8));
    if constexpr (sizeof(VT) == 4) {
        ch.v = __builtin_nontemporal_load(reinterpret_cast<const w8_v4f *>(p + 512 + lane * 16));
    } else {
        ch.v0 = __builtin_nontemporal_load(reinterpret_cast<const w8_v2d *>(p + 512 + lane * 16));
        ch.v1 = __builtin_nontemporal_load(reinterpret_cast<const w8_v2d *>(p + 1536 + lane * 16));
    }
    return ch;
}

// the implied-slot layout: a chunk's values (two non-temporal loads per lane, as above; win4: one); its slots are loaded by the kernel
template <typename VT>
__device__ __forceinline__ void w8_load_values(const unsigned char *__restrict__ stream, int64_t c, int lane, W8Chunk<VT> &ch) {
    const unsigned char *p = stream + (size_t)c * w8_val_bytes<VT>();
    if constexpr (sizeof(VT) == 4) {
        ch.v = __builtin_nontemporal_load(reinterpret_cast<const w8_v4f *>(p + lane * 16));
    } else {
        ch.v0 = __builtin_nontemporal_load(reinterpret_cast<const w8_v2d *>(p + lane * 16));
        ch.v1 = __builtin_nontemporal_load(reinterpret_cast<const w8_v2d *>(p + 1024 + lane * 16));
    }
}

// the slots of a chunk of the implied-slot layout: code = 4 x 16-bit bases, off2 = (8 (row - block_row0)) x 0x10001 in an implicit
// slice, 0 in an explicit one (whose code holds the slots themselves); per half: (base + off) mod 2^16, 0 where the base is 1 (padding)
typedef unsigned short w8_v2h __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned w8_imply(unsigned code, unsigned off2) {
    const unsigned pad = (code & 0x10001u) * 0xffffu;
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(w8_v2h, code) + __builtin_bit_cast(w8_v2h, off2)) & ~pad;
}

// acc += v_q * window[slot_q], q = 0..3, products and sums rounded separately (the CRS kernels' arithmetic)
__device__ __forceinline__ void w8_consume(const unsigned char *win, const W8Chunk<double> &ch, double &acc) {
#pragma clang fp contract(off)
    const double x0 = *reinterpret_cast<const double *>(win + (ch.code.x & 0xffffu));
    const double x1 = *reinterpret_cast<const double *>(win + (ch.code.x >> 16));
    const double x2 = *reinterpret_cast<const double *>(win + (ch.code.y & 0xffffu));
    const double x3 = *reinterpret_cast<const double *>(win + (ch.code.y >> 16));
    const double p0 = ch.v0.x * x0, p1 = ch.v0.y * x1, p2 = ch.v1.x * x2, p3 = ch.v1.y * x3;
    acc = acc + p0;
    acc = acc + p1;
    acc = acc + p2;
    acc = acc + p3;
}
// win4: the float is widened first (exact), so each product is the one of the fp64 CRS value the float was made from
__device__ __forceinline__ void w8_consume(const unsigned char *win, const W8Chunk<float> &ch, double &acc) {
#pragma clang fp contract(off)
    const double x0 = *reinterpret_cast<const double *>(win + (ch.code.x & 0xffffu));
    const double x1 = *reinterpret_cast<const double *>(win + (ch.code.x >> 16));
    const double x2 = *reinterpret_cast<const double *>(win + (ch.code.y & 0xffffu));
    const double x3 = *reinterpret_cast<const double *>(win + (ch.code.y >> 16));
    const double p0 = (double)ch.v.x * x0, p1 = (double)ch.v.y * x1, p2 = (double)ch.v.z * x2, p3 = (double)ch.v.w * x3;
    acc = acc + p0;
    acc = acc + p1;
    acc = acc + p2;
    acc = acc + p3;
}

// MODE 0: y = A x.  MODE 1: also partials[4 b + wave] = sum over the wave's rows of y[r] w[r] (CG's (Ap, p)).
// A wave owns the R consecutive slices slice0 .. slice0 + R - 1; their chunks are ONE contiguous range of the stream (the chunk
// offsets are a prefix sum), walked with a ring of D chunks in flight per lane: the chunk D places ahead is requested as soon
// as a ring entry has been consumed, so the stream never waits for the arithmetic, and the first D chunks are requested before
// the window is (they do not need it).  LDS: 16 bytes (the -0.0 slot), then the window.
// IMPL: the implied-slot layout (w8_fill_kernel PHASE 2): a chunk's 8 slot bytes per lane come from desc[chunk] (the same 8 bytes
// for every lane: implicit slice) or from its record in side (explicit slice), chosen per chunk by its slice (wave-uniform).
// VT: the stream's value type, double, or float for win4 (chunks of 1536 / 1024 bytes, everything else the same).
// TWO: the ring has two register sets (see the walk below); false: one set, whose loads the compiler drains once per round.
template <int MODE, int R, int D, bool IMPL, typename VT = double, bool TWO = false>
__global__ __launch_bounds__(256) void spmv_win8_kernel(
    const double *x, double *__restrict__ y, int64_t n_rows, int64_t n_cols, int n_blocks, int remap_arg, const double *w,
    double *__restrict__ partials, const int *stop, const int32_t *__restrict__ hdr, const int64_t *__restrict__ slice_chunk0,
    const unsigned char *__restrict__ stream, int x_al16, const int32_t *__restrict__ own_rank, const uint16_t *__restrict__ row_of,
    const w8_v2u *__restrict__ desc, const unsigned char *__restrict__ side, const int64_t *__restrict__ slice_rec) {
    if (stop && stop[1]) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = win_block(remap_arg);
    if (b >= n_blocks) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hw_g = hdr[(size_t)b * 2 * kW8Runs + lane], hw_r = hdr[(size_t)b * 2 * kW8Runs + kW8Runs + lane]; // run k: first granule / rank | granules << 16
    const int64_t slice0 = ((int64_t)b * 4 + wv) * R;
    const int64_t block_row0 = (int64_t)b * kSwRows * R;
    int64_t rows_of[R]; // the rows this lane owns: position (slice, lane) of the block's length order -> row
#pragma unroll
    for (int r = 0; r < R; ++r) rows_of[r] = block_row0 + row_of[(slice0 + r) * 64 + lane];
    // chunk boundaries of the wave's slices: lane r holds slice_chunk0[slice0 + r], r <= R
    const int64_t my_bnd = slice_chunk0[slice0 + min(lane, R)];
    auto bnd = [&](int r) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)my_bnd, r);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)my_bnd >> 32), r);
        return (int64_t)(((unsigned long long)hi << 32) | lo);
    };
    const int64_t C0 = bnd(0), C1 = bnd(R);
    const int64_t c_last = max(C1 - 1, C0); // (the stream ends with one spare chunk: an empty wave reads it)
    int64_t e[R]; // slice rr of the wave ends at chunk e[rr] (an empty slice: e[rr] == e[rr - 1])
#pragma unroll
    for (int rr = 0; rr < R; ++rr) e[rr] = bnd(rr + 1);
    // IMPL: the slot record of each slice's first chunk (rec[rr + 1] == rec[rr]: slice rr is implicit), and the lane's slot
    // offset per slice (0 in an explicit slice)
    int64_t rec[R + 1];
    unsigned off2[R];
    if (IMPL) {
        const int64_t my_rec = slice_rec[slice0 + min(lane, R)];
#pragma unroll
        for (int r = 0; r <= R; ++r) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)my_rec, r);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)my_rec >> 32), r);
            rec[r] = (int64_t)(((unsigned long long)hi << 32) | lo);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) off2[r] = rec[r + 1] == rec[r] ? (unsigned)(rows_of[r] - block_row0) * 0x80008u : 0u;
    }
    auto load = [&](int64_t cc) {
        if (!IMPL) return w8_load<VT>(stream, cc, lane);
        W8Chunk<VT> ch;
        w8_load_values<VT>(stream, cc, lane, ch);
        int64_t rs = 0, re = 0, cs = 0; // chunk cc lies in the wave's slice rr (cc = C0 of an empty wave: in none)
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
            if (cc >= (rr ? e[rr - 1] : C0) && cc < e[rr]) { rs = rec[rr]; re = rec[rr + 1]; cs = rr ? e[rr - 1] : C0; }
        if (re > rs) ch.code = __builtin_nontemporal_load(reinterpret_cast<const w8_v2u *>(side + (size_t)(rs + cc - cs) * 512 + lane * 8));
        else ch.code = desc[cc];
        return ch;
    };
    W8Chunk<VT> ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ring[d] = load(min(C0 + d, c_last));
    // MODE 1: the dot's operand.  own_rank != nullptr: w is x at the rows' own columns (CG: w = x = p) -- where the block's window
    // holds them side by side (own >= 0) the operand comes from LDS behind the barrier instead of a second global read of p
    double wr[R];
    int own = -1;
    if (MODE == 1 && own_rank) own = own_rank[b];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = rows_of[r];
        wr[r] = (MODE == 1 && own < 0 && row < n_rows) ? w[row] : 0.0;
    }
    if (tid == 0) *reinterpret_cast<double *>(lds) = -0.0;
    {   // window: the runs of 8-column granules, 16-byte pieces by LDS-DMA
        const int n_runs = __popcll(__ballot((hw_r >> 16) != 0));
        unsigned char *win = lds + 16;
        WIN_COPY_RUNS(x, n_cols, x_al16, win, wv, lane, n_runs, hw_g, hw_r, 0)
    }
    __syncthreads();
    if (MODE == 1 && own >= 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) wr[r] = *reinterpret_cast<const double *>(lds + 16 + ((size_t)own * 8 + (wv * R + r) * 64 + lane) * 8);
    }
    double dot_acc = 0.0; // MODE 1: sum over the wave's slices of y[row] w[row] (one partial per WAVE)
    // the walk over [C0, C1): ring[d] holds chunk c whenever (c - C0) % D == d, so the ring index is a compile-time constant in
    // the unrolled round.  All slice indices are compile-time constants too (a run-time index put wr[] into scratch memory):
    // cur_off, the slot offset of the slice being summed, follows `next` where a slice ends.
    int64_t c = C0;
    int next = 0; // the slice being summed (wave-uniform)
    double acc = 0.0;
    unsigned cur_off = IMPL ? off2[0] : 0u;
#define W8_END_SLICES()                                                                    \
    _Pragma("unroll") for (int rr = 0; rr < R; ++rr)                                       \
        if (rr == next && c == e[rr]) {                                                    \
            const int64_t row = rows_of[rr];                                               \
            if (row < n_rows) y[row] = acc;                                                \
            if (MODE == 1) dot_acc += row < n_rows ? acc * wr[rr] : 0.0;                   \
            acc = 0.0;                                                                     \
            ++next;                                                                        \
            if (IMPL) cur_off = off2[rr + 1 < R ? rr + 1 : R - 1];                         \
        }
    W8_END_SLICES()
    // one step of the walk: chunk c is taken from FROM, chunk c + D is requested INTO, chunk c is summed
#define W8_STEP(FROM, INTO)                                                                \
    {                                                                                      \
        W8Chunk<VT> cur = FROM;                                                            \
        INTO = load(min(c + D, c_last));                                                   \
        if (IMPL) {                                                                        \
            cur.code.x = w8_imply(cur.code.x, cur_off);                                    \
            cur.code.y = w8_imply(cur.code.y, cur_off);                                    \
        }                                                                                  \
        w8_consume(lds, cur, acc);                                                         \
        ++c;                                                                               \
        W8_END_SLICES()                                                                    \
    }
    // the last steps of a wave, fewer than D: nothing is left to request
#define W8_TAIL(FROM)                                                                      \
    _Pragma("unroll") for (int d = 0; d < D - 1; ++d)                                      \
        if (c < C1) {                                                                      \
            W8Chunk<VT> cur = FROM[d];                                                     \
            if (IMPL) {                                                                    \
                cur.code.x = w8_imply(cur.code.x, cur_off);                                \
                cur.code.y = w8_imply(cur.code.y, cur_off);                                \
            }                                                                              \
            w8_consume(lds, cur, acc);                                                     \
            ++c;                                                                           \
            W8_END_SLICES()                                                                \
        }
    if constexpr (TWO) {
        // two register sets: a round takes its chunks from one set and requests the chunks of the next round into the OTHER, so no
        // step writes a register that holds a chunk still to be summed, the loop's back edge carries no copy of a loaded value,
        // and the only waits in the loop are counted ones that leave the youngest D chunks' loads in flight
        W8Chunk<VT> ring2[D];
        while (c + 2 * D <= C1) { // (wave-uniform) two whole rounds per trip, no guard inside
#pragma unroll
            for (int d = 0; d < D; ++d) W8_STEP(ring[d], ring2[d])
#pragma unroll
            for (int d = 0; d < D; ++d) W8_STEP(ring2[d], ring[d])
        }
        if (c + D <= C1) { // at most one more whole round, then fewer than D chunks, already requested
#pragma unroll
            for (int d = 0; d < D; ++d) W8_STEP(ring[d], ring2[d])
            W8_TAIL(ring2)
        } else {
            W8_TAIL(ring)
        }
    } else {
        while (c < C1) { // (wave-uniform)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (c < C1) W8_STEP(ring[d], ring[d])
            }
        }
    }
#undef W8_TAIL
#undef W8_STEP
#undef W8_END_SLICES
    if (MODE == 1) {
        const double t = wave_sum(dot_acc);
        if (lane == 0) partials[(size_t)b * 4 + wv] = t;
    }
}

} // namespace

// The 8-byte stream (vb = 8: A->w8[0]) and the 4-byte one (vb = 4, "win4": A->w8[1]) are two instances of one form: every function
// below takes the value width and works on that instance.
static inline bis_win8 *&w8_ptr(bis_mat *A, int vb) { return A->w8[vb == 4].p; }
static inline int &w8_state(bis_mat *A, int vb) { return A->w8[vb == 4].state; }
static inline const bis_win8 *w8_get(const bis_mat *A, int vb) { return A->w8[vb == 4].state == 1 ? A->w8[vb == 4].p : nullptr; } // the usable instance, or null

static void w8_drop_one(bis_mat *A, int vb) {
    if (bis_win8 *&sw = w8_ptr(A, vb)) {
        if (sw->own_stream) sw->stream = static_cast<unsigned char *>(sw->own_stream); // (a redirected stream is the caller's memory: never freed here)
        hipFree(sw->hdr); hipFree(sw->slice_chunk0); hipFree(sw->own_rank); hipFree(sw->stream); hipFree(sw->row_of);
        hipFree(sw->slice_rec);
        delete sw;
        sw = nullptr;
    }
    w8_state(A, vb) = 0;
}

void bis_spmv_win8_drop(bis_mat *A) {
    w8_drop_one(A, 8);
    w8_drop_one(A, 4);
}

// which of the two streams the reports without a context speak of (bis_mat_win8_layout, _tuning, _debug_stream): the 4-byte one
// where it is built and spmv_resolve's conditions on the flag and the options still hold, else the 8-byte one
int bis_spmv_win8_active(const bis_mat *A) {
    return A->f32_exact && w8_get(A, 4) && bis_opts().spmv_win4 != 0 && bis_opts().spmv_win8 != 0 ? 4 : 8;
}

int bis_spmv_win8_blocks(const bis_mat *A, int vb) { const bis_win8 *sw = w8_get(A, vb); return sw ? sw->n_blocks : 0; }
int bis_spmv_win8_rows(const bis_mat *A, int vb) { const bis_win8 *sw = w8_get(A, vb); return sw ? sw->R : 0; }
bool bis_spmv_win8_implied(const bis_mat *A, int vb) { const bis_win8 *sw = w8_get(A, vb); return sw && sw->slice_rec != nullptr; }
// bytes of the form's own arrays one launch reads: the stream (with its padding), block headers, slice offsets.  The implied-slot
// layout: 2048 bytes of values per chunk, 8 bytes of slot bases per chunk of an implicit slice, 512 bytes of slots per chunk of an
// explicit slice, and the slices' slot-record offsets.  win4: 1536 / 1024 bytes per chunk
int64_t bis_spmv_win8_bytes(const bis_mat *A, int vb) {
    const bis_win8 *sw = w8_get(A, vb);
    if (!sw) return 0;
    const int64_t meta = (int64_t)sw->n_blocks * (8 * kW8Runs + 2 * kSwRows * sw->R) + 8 * (sw->n_slices + 1);
    if (!sw->slice_rec) return sw->total_chunks * (int64_t)w8_chunk_bytes(vb) + meta;
    return sw->total_chunks * (int64_t)w8_val_bytes(vb) + 8 * (sw->total_chunks - sw->expl_chunks) + 512 * sw->expl_chunks + meta + 8 * (sw->n_slices + 1);
}

// placement tuning (bis_mat_tune_placement): the stream's size, and an exchange of the buffer the kernel reads (values and slots,
// in either layout)
size_t bis_spmv_win8_stream_bytes(const bis_mat *A, int vb) {
    const bis_win8 *sw = w8_get(A, vb);
    if (!sw) return 0;
    return sw->slice_rec ? sw->w8_end : w8_chunk_bytes(vb) * (size_t)(sw->total_chunks + 1);
}

// the placement searches' test for the fast level of the stream's placement, priced on the bytes a launch moves (the same
// measure for both layouts): the form's own arrays, the x granules copied into the blocks' windows, y.  HPCG-256 moves 5.43 GB
// in today's layout and 4.59 GB with implied slots, where the search times the fused product.  With the two-set chunk ring
// (docs/EXPERIMENTS.md section 32) the first allocations of eight processes gave 0.639-0.655 ms = 7.0-7.2 TB/s (the fast level),
// 0.693 ms = 6.63 TB/s and 0.72-0.79 ms; the explicit layout's plain product 0.755-0.79 ms = 6.9-7.2 TB/s against 0.855-0.89 ms.
// 6.85 TB/s (0.671 ms with implied slots) lies between the fast level and the next one of either.  (The 4-byte stream is held to
// the same rate on its own, smaller, byte count: whether it reaches that rate has not been measured -- docs/EXPERIMENTS.md
// section 23 -- and no other threshold is invented for it.)
double bis_spmv_win8_moved_bytes(const bis_mat *A, int vb) {
    const bis_win8 *sw = w8_get(A, vb);
    if (!sw) return 0.0;
    return (double)bis_spmv_win8_bytes(A, vb) + 64.0 * (double)sw->win_gran_sum + 8.0 * (double)A->n_rows;
}
bool bis_spmv_win8_fast(const bis_mat *A, double ms, int vb) {
    return w8_get(A, vb) && ms > 0.0 && bis_spmv_win8_moved_bytes(A, vb) / (ms * 1e-3) >= 6.85e12;
}
void *bis_spmv_win8_swap_stream(bis_mat *A, void *stream, int vb) {
    bis_win8 *sw = w8_ptr(A, vb);
    void *old = sw->stream;
    sw->stream = static_cast<unsigned char *>(stream);
    return old;
}

#define W8_CHECK(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            (void)hipGetLastError();                                           \
            hipFree(slice_chunks); hipFree(tmp);                               \
            w8_drop_one(A, vb);                                                \
            w8_state(A, vb) = -1;                                              \
            if (e_ == hipErrorOutOfMemory) return BIS_OK; /* the gather kernel stays */ \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);      \
            return BIS_ERR_HIP;                                                \
        }                                                                      \
    } while (0)

// Build the form (its state in A->w8: 1 usable, -1 does not apply).  Rows per lane: option spmv_win8_rows (1, 2, 4), default 2 for
// matrices of at least half a million rows.
// Placement tuning of the stream at build time.  WHERE in HBM the stream lies decides between two levels of the kernel's time,
// 13 % apart (HPCG-256: 0.755 / 0.855 ms; constant over time for an allocation, independent of where x and y lie, and the slow
// level is the common one early in a process: tools/win8_place2.py, tools/win8_timeline.py, profiles/r05_f_win8_placement.log).
// So a stream of 1 GiB or more (counted in today's layout, 2560 bytes per chunk, also where slots are implied) is tried in up to k fresh allocations (option spmv_win8_tune, default 12 -- five slow allocations
// in a row have been seen --; the earlier ones are
// held so that the next one lands elsewhere; bounded by the free memory minus 8 GiB), each a device-to-device copy timed with
// the kernel itself on a zero vector, and the search ends at the first allocation of the fast level.
static bis_status w8_tune_placement(bis_ctx *ctx, bis_mat *A, int vb) {
    bis_win8 *sw = w8_ptr(A, vb);
    const size_t bytes = bis_spmv_win8_stream_bytes(A, vb);
    // (the size test is on today's layout, 2560 bytes per chunk, in both layouts and for the 4-byte stream: the same matrices are searched)
    const int k = bis_opts().spmv_win8_tune >= 0 ? bis_opts().spmv_win8_tune : ((size_t)kW8ChunkBytes * (size_t)(sw->total_chunks + 1) >= ((size_t)1 << 30) ? 12 : 0);
    if (k <= 0) return BIS_OK;
    double *x = nullptr, *y = nullptr, *part = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<void *> losers;
    auto cleanup = [&]() {
        hipStreamSynchronize(ctx->stream);
        for (void *l : losers) hipFree(l);
        hipFree(x); hipFree(y); hipFree(part);
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        (void)hipGetLastError();
    };
    const size_t nx = (size_t)std::max(A->n_cols, A->view_row0 + A->n_rows) + 2; // (x is also the fused dot's w at the rows' own columns)
    if (hipMalloc(&x, sizeof(double) * nx) != hipSuccess || hipMalloc(&y, sizeof(double) * (size_t)A->n_rows) != hipSuccess ||
        hipMalloc(&part, sizeof(double) * 4 * (size_t)sw->n_blocks) != hipSuccess ||
        hipMemsetAsync(x, 0, sizeof(double) * nx, ctx->stream) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { cleanup(); return BIS_OK; } // no room to tune: keep the first allocation
    const int nb = sw->n_blocks, remap_arg = bis_spmv_remap_arg(nb), grid = bis_spmv_grid(nb);
    // the kernel timed: with implied slots the one CG runs (the fused (Ap, p) dot, w = x) -- the plain product's time did not tell
    // its placement level (HPCG-256: 0.635 ms plain on an allocation where the CG loop's fused launches took 0.81 ms)
    const bool implied = bis_spmv_win8_implied(A, vb);
    const int mode = implied ? 1 : 0;
    const double *w = implied ? x + A->view_row0 : nullptr;
    double *partials = implied ? part : nullptr;
    auto measure = [&](double &ms) -> bool {
        for (int i = 0; i < 2; ++i) if (bis_spmv_win8_launch(ctx, A, x, y, mode, w, partials, nullptr, remap_arg, grid, vb) != BIS_OK) return false;
        hipEventRecord(e0, ctx->stream);
        for (int i = 0; i < 5; ++i) if (bis_spmv_win8_launch(ctx, A, x, y, mode, w, partials, nullptr, remap_arg, grid, vb) != BIS_OK) return false;
        hipEventRecord(e1, ctx->stream);
        if (hipEventSynchronize(e1) != hipSuccess) return false;
        float f = 0.f;
        hipEventElapsedTime(&f, e0, e1);
        ms = f / 5.0;
        return true;
    };
    double best = 0.0;
    if (!measure(best)) { cleanup(); ctx->err = "win8 placement tuning: launch failed"; return BIS_ERR_HIP; }
    sw->tune_first_ms = best;
    // the search ends at an allocation of the fast level (bis_spmv_win8_fast), or, in today's layout, one at least 8 % faster than
    // the slowest seen (ragged rows never reach the fast level's rate).  With implied slots the placements spread over more than
    // two levels (HPCG-256: 0.65-0.78 ms) and the 8 % rule stopped at middle ones (0.70-0.72 ms): there only the rate counts
    double slowest = best;
    auto fast_enough = [&](double ms) { return bis_spmv_win8_fast(A, ms, vb) || (!implied && ms <= 0.92 * slowest); };
    int trials = 0;
    for (; trials < k && !fast_enough(best); ++trials) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + ((size_t)8 << 30)) break;
        void *cand = nullptr;
        if (hipMalloc(&cand, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        void *cur = bis_spmv_win8_swap_stream(A, cand, vb);
        hipMemcpyAsync(cand, cur, bytes, hipMemcpyDeviceToDevice, ctx->stream);
        double ms = 0.0;
        if (!measure(ms)) { bis_spmv_win8_swap_stream(A, cur, vb); losers.push_back(cand); cleanup(); ctx->err = "win8 placement tuning: launch failed"; return BIS_ERR_HIP; }
        slowest = std::max(slowest, ms);
        if (ms < best) { best = ms; losers.push_back(cur); }
        else { bis_spmv_win8_swap_stream(A, cur, vb); losers.push_back(cand); }
    }
    sw->tune_trials = trials;
    sw->tune_kept_ms = best;
    if (getenv("BIS_WIN8_STATS")) fprintf(stderr, "win8 placement: %d re-allocation(s) of %zu bytes tried, kernel %.4f ms on the first allocation, %.4f ms on the one kept (%.0f bytes moved: %.2f TB/s)\n", trials, bytes, sw->tune_first_ms, best, bis_spmv_win8_moved_bytes(A, vb), bis_spmv_win8_moved_bytes(A, vb) / (best * 1e9));
    cleanup();
    return BIS_OK;
}

// debugging / tuning aid (tools/win8_offsets.py): the stream's address and size; *set != NULL: read the stream from there from now
// on (the caller owns that memory and has copied the stream into it; the library's own buffer stays allocated)
extern "C" BIS_API bis_status bis_mat_win8_debug_stream(bis_mat *A, void **ptr, size_t *bytes, void *set) {
    const int vb = A ? bis_spmv_win8_active(A) : 8;
    if (!A || !w8_get(A, vb)) return BIS_ERR_INVALID;
    bis_win8 *sw = w8_ptr(A, vb);
    if (ptr) *ptr = sw->own_stream ? sw->own_stream : (void *)sw->stream;
    if (bytes) *bytes = bis_spmv_win8_stream_bytes(A, vb);
    if (set) { if (!sw->own_stream) sw->own_stream = sw->stream; sw->stream = static_cast<unsigned char *>(set); }
    else if (sw->own_stream) { sw->stream = static_cast<unsigned char *>(sw->own_stream); sw->own_stream = nullptr; }
    return BIS_OK;
}

extern "C" BIS_API void bis_mat_win8_layout(const bis_mat *A, int64_t *chunks, int64_t *explicit_chunks, int64_t *slices, int *blocks, int *implied) {
    const bis_win8 *sw = A ? w8_get(A, bis_spmv_win8_active(A)) : nullptr;
    if (chunks) *chunks = sw ? sw->total_chunks : 0;
    if (explicit_chunks) *explicit_chunks = sw ? sw->expl_chunks : 0;
    if (slices) *slices = sw ? sw->n_slices : 0;
    if (blocks) *blocks = sw ? sw->n_blocks : 0;
    if (implied) *implied = sw && sw->slice_rec != nullptr;
}

extern "C" BIS_API void bis_mat_win8_tuning(const bis_mat *A, int *trials, double *first_ms, double *kept_ms) {
    const bis_win8 *sw = A ? w8_get(A, bis_spmv_win8_active(A)) : nullptr;
    if (trials) *trials = sw ? sw->tune_trials : 0;
    if (first_ms) *first_ms = sw ? sw->tune_first_ms : 0.0;
    if (kept_ms) *kept_ms = sw ? sw->tune_kept_ms : 0.0;
}

static bis_status w8_try_rows(bis_ctx *ctx, bis_mat *A, int R, bool *window_too_large, int vb);

bis_status bis_spmv_win8_try(bis_ctx *ctx, bis_mat *A, int vb) {
    if (w8_state(A, vb) != 0) return BIS_OK;
    w8_state(A, vb) = -1;
    if (A->n_rows == 0 || A->nnz == 0 || A->n_cols >= ((int64_t)1 << 31) - 16) return BIS_OK;
    // default 4 rows per lane (blocks of 1024 rows): HPCG-256 0.78 ms against 0.86 with 2 and 1.20 with 1 -- the larger the block, the
    // fewer times an x entry is copied into some block's window (tools/win8_probe.py, profiles/r05_c_win8_probe.log).  Where a
    // block of that size reads more than 64 runs / 60 KB of x the plan is made again with half the rows (an RCM-ordered mesh of
    // 1.5 M rows: not representable with 1024 rows, 43.6 KB windows with 512: 0.193 against 0.237 ms for the row-block kernel).
    int R = bis_opts().spmv_win8_rows > 0 ? std::min(bis_opts().spmv_win8_rows, 4) : 4;
    if (R == 3) R = 2;
    while (R > 1 && A->n_rows < (int64_t)kSwRows * R * 1024) R >>= 1;
    for (;; R >>= 1) {
        bool too_large = false;
        if (bis_status st = w8_try_rows(ctx, A, R, &too_large, vb)) return st;
        if (w8_state(A, vb) == 1 || !too_large || R == 1 || bis_opts().spmv_win8_rows > 0) return BIS_OK;
        w8_state(A, vb) = -1;
    }
}

static bis_status w8_try_rows(bis_ctx *ctx, bis_mat *A, int R, bool *window_too_large, int vb) {
    *window_too_large = false;
    const int64_t nb64 = (A->n_rows + (int64_t)kSwRows * R - 1) / ((int64_t)kSwRows * R);
    if (nb64 > (int64_t)1 << 26) return BIS_OK;
    const int nb = (int)nb64;
    bis_win8 *sw = new bis_win8;
    w8_ptr(A, vb) = sw;
    sw->n_blocks = nb;
    sw->R = R;
    sw->vb = vb;
    sw->n_slices = (int64_t)nb * 4 * R;
    int32_t *slice_chunks = nullptr;
    void *tmp = nullptr;
    int *status = bis_slot_ptr(ctx, kSlotWinplan);
    W8_CHECK(hipMalloc(&sw->hdr, sizeof(int32_t) * 2 * kW8Runs * (size_t)nb));
    W8_CHECK(hipMalloc(&sw->own_rank, sizeof(int32_t) * (size_t)nb));
    W8_CHECK(hipMemsetAsync(sw->own_rank, 0xFF, sizeof(int32_t) * (size_t)nb, ctx->stream)); // (blocks the plan leaves early: -1)
    W8_CHECK(hipMalloc(&sw->row_of, sizeof(uint16_t) * (size_t)nb * kSwRows * (size_t)R));
    W8_CHECK(hipMalloc(&slice_chunks, sizeof(int32_t) * (size_t)(sw->n_slices + 1)));
    W8_CHECK(hipMalloc(&sw->slice_chunk0, sizeof(int64_t) * (size_t)(sw->n_slices + 1)));
    W8_CHECK(bis_slot_io(ctx, kSlotWinplan, 3));
    W8_CHECK(bis_slot_io(ctx, kSlotWinplan + 5, 1));
    W8_CHECK(hipMemsetAsync(slice_chunks, 0, sizeof(int32_t) * (size_t)(sw->n_slices + 1), ctx->stream));
    W8_CHECK(hipMemsetAsync(sw->hdr, 0, sizeof(int32_t) * 2 * kW8Runs * (size_t)nb, ctx->stream));
    if (A->rp64) hipLaunchKernelGGL(w8_plan_kernel<int64_t>, dim3(nb), dim3(256), 0, ctx->stream, (const int64_t *)A->row_ptr, A->col, A->n_rows, R, kSwMaxGran, A->view_row0, sw->hdr, slice_chunks, sw->own_rank, sw->row_of, status);
    else hipLaunchKernelGGL(w8_plan_kernel<int32_t>, dim3(nb), dim3(256), 0, ctx->stream, (const int32_t *)A->row_ptr, A->col, A->n_rows, R, kSwMaxGran, A->view_row0, sw->hdr, slice_chunks, sw->own_rank, sw->row_of, status);
    W8_CHECK(hipGetLastError());
    int h[3] = {0, 0, 0};
    W8_CHECK(hipMemcpyAsync(h, status, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    const int64_t ns1 = sw->n_slices + 1;
    int64_t total = 0;
    W8_CHECK(bis_winplan_scan(slice_chunks, sw->slice_chunk0, sw->n_slices, &total, ctx->stream)); // (and h has arrived)
    hipFree(slice_chunks); slice_chunks = nullptr;
    sw->total_chunks = total;
    sw->max_gran = h[1];
    sw->win_gran_sum = (int64_t)(unsigned)h[2];
    // not representable (more than 64 runs / 60 KiB of window in some block), or more than 12 % of padding (every padded entry costs
    // 10 streamed bytes: Anderson's 7-entry rows in 8 slots, 14 %, run 0.310 ms against 0.297 for the row-block kernel): that kernel stays
    if (h[0] || (double)total * 256.0 > 1.12 * (double)A->nnz + 256.0 * 4 * 64) {
        if (getenv("BIS_WIN8_STATS")) fprintf(stderr, "win8 plan (R = %d): %s, %.1f %% padding: not used\n", R, h[0] ? "window not representable" : "representable", 100.0 * ((double)total * 256.0 / (double)A->nnz - 1.0));
        *window_too_large = h[0] != 0;
        w8_drop_one(A, vb);
        w8_state(A, vb) = -1;
        return BIS_OK;
    }
#define W8_FILL(PHASE, VT, STREAM, DESC, SIDE)                                                                                                    \
    do {                                                                                                                                          \
        if (A->rp64) hipLaunchKernelGGL((w8_fill_kernel<int64_t, PHASE, VT>), dim3(nb), dim3(256), 0, ctx->stream, (const int64_t *)A->row_ptr, A->col, \
                                        A->val, A->n_rows, R, sw->hdr, sw->slice_chunk0, sw->row_of, STREAM, sw->slice_rec, DESC, SIDE);           \
        else hipLaunchKernelGGL((w8_fill_kernel<int32_t, PHASE, VT>), dim3(nb), dim3(256), 0, ctx->stream, (const int32_t *)A->row_ptr, A->col, \
                                A->val, A->n_rows, R, sw->hdr, sw->slice_chunk0, sw->row_of, STREAM, sw->slice_rec, DESC, SIDE);                   \
        W8_CHECK(hipGetLastError());                                                                                                              \
    } while (0)
    // implied slots (option spmv_win8_implicit, default on): classify the slices, count the chunks that keep their slots; the
    // layout is built where at least half of the chunks are implicit (stencils: HPCG-256 93.6 %), today's layout elsewhere
    sw->expl_chunks = total;
    if (bis_opts().spmv_win8_implicit != 0 && total > 0) {
        W8_CHECK(hipMalloc(&sw->slice_rec, sizeof(int64_t) * (size_t)ns1));
        W8_CHECK(hipMemsetAsync(sw->slice_rec, 0, sizeof(int64_t) * (size_t)ns1, ctx->stream));
        W8_FILL(1, double, nullptr, nullptr, nullptr); // (value-free: one instance serves both widths)
        size_t tmp_bytes = 0;
        W8_CHECK(rocprim::exclusive_scan(nullptr, tmp_bytes, sw->slice_rec, sw->slice_rec, (int64_t)0, (size_t)ns1, rocprim::plus<int64_t>(), ctx->stream));
        W8_CHECK(hipMalloc(&tmp, tmp_bytes));
        W8_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, sw->slice_rec, sw->slice_rec, (int64_t)0, (size_t)ns1, rocprim::plus<int64_t>(), ctx->stream));
        int64_t expl = 0;
        W8_CHECK(hipMemcpyAsync(&expl, sw->slice_rec + sw->n_slices, sizeof expl, hipMemcpyDeviceToHost, ctx->stream));
        W8_CHECK(hipStreamSynchronize(ctx->stream));
        hipFree(tmp); tmp = nullptr;
        if (2 * (total - expl) >= total) sw->expl_chunks = expl;
        else { hipFree(sw->slice_rec); sw->slice_rec = nullptr; }
    }
    const size_t chunk_bytes = sw->slice_rec ? w8_val_bytes(vb) : w8_chunk_bytes(vb);
    size_t stream_bytes = chunk_bytes * (size_t)(total + 1);
    if (sw->slice_rec) {
        sw->w8_desc = stream_bytes;
        sw->w8_side = sw->w8_desc + ((8 * (size_t)(total + 1) + 255) & ~(size_t)255);
        sw->w8_end = stream_bytes = sw->w8_side + 512 * (size_t)sw->expl_chunks;
    }
    W8_CHECK(hipMalloc(&sw->stream, stream_bytes));
    unsigned char *stream = sw->stream;
    W8_CHECK(hipMemsetAsync(stream + (size_t)total * chunk_bytes, 0, chunk_bytes, ctx->stream));
    if (sw->slice_rec) {
        W8_CHECK(hipMemsetAsync(stream + sw->w8_desc, 0, sw->w8_side - sw->w8_desc, ctx->stream));
        if (vb == 4) W8_FILL(2, float, stream, reinterpret_cast<uint2 *>(stream + sw->w8_desc), stream + sw->w8_side);
        else W8_FILL(2, double, stream, reinterpret_cast<uint2 *>(stream + sw->w8_desc), stream + sw->w8_side);
    } else {
        if (vb == 4) W8_FILL(0, float, stream, nullptr, nullptr);
        else W8_FILL(0, double, stream, nullptr, nullptr);
    }
#undef W8_FILL
    w8_state(A, vb) = 1;
    if (bis_status tst = w8_tune_placement(ctx, A, vb)) return tst;
    if (getenv("BIS_WIN8_STATS")) fprintf(stderr, "win%d plan (R = %d): %d blocks, window <= %d granules (%zu bytes), %.1f %% padding: used; implied slots: %s, %.1f %% of %lld chunks implicit; stream at %p (%zu bytes), hdr %p\n", vb, R, nb, sw->max_gran, (size_t)(2 + 8 * sw->max_gran) * 8, 100.0 * ((double)total * 256.0 / (double)A->nnz - 1.0), sw->slice_rec ? "built" : "not built", 100.0 * (double)(total - sw->expl_chunks) / (double)std::max<int64_t>(total, 1), (long long)total, (void *)sw->stream, bis_spmv_win8_stream_bytes(A, vb), (void *)sw->hdr);
    return BIS_OK;
}
#undef W8_CHECK

bis_status bis_spmv_win8_launch(bis_ctx *ctx, const bis_mat *A, const double *x, double *y, int mode, const double *w,
                                double *partials, const int *stop, int remap_arg, int grid, int vb) {
    const bis_win8 *sw = A->w8[vb == 4].p;
    const int x_al16 = ((uintptr_t)x & 15) == 0;
    const size_t lds = (size_t)(2 + 8 * sw->max_gran) * 8;
    const unsigned char *stream = sw->stream;
    const int32_t *own = (mode == 1 && w == x + A->view_row0 && x_al16) ? sw->own_rank : nullptr; // the fused dot's w is x itself (CG: p)
    // The chunk ring.  Two register sets (spmv_win8_sets, default 2; depths 1-4): the loop never drains the loads it has issued, so
    // `depth` chunks per lane stay in flight at every wait; one set: the ring is drained once per round.  Chunks requested ahead
    // per lane (spmv_win8_depth), by measurement in the CG loop (docs/EXPERIMENTS.md section 32), two sets: 3 for 512- and
    // 1024-row blocks (HPCG-256 0.673-0.778 ms by placement, one set at its best depth 0.767-0.812; HPCG-512 5.16 against 5.30;
    // fem:80,80,80 0.177 against 0.184; win4 HPCG-256 0.439 against 0.459), 2 for 256-row blocks, whose occupancy the VGPRs bound
    // (HPCG-256 0.758 ms; 3: 0.808; one set 0.826).  One set (spmv_win8_sets = 1) keeps its earlier rule: 1024-row blocks 1 where
    // the slices are uniform, 2 with ragged rows, smaller blocks 3.
    const bool ragged = (double)sw->total_chunks * 256.0 > 1.08 * (double)A->nnz;
    const bool two = bis_opts().spmv_win8_sets > 0 ? bis_opts().spmv_win8_sets >= 2 : true;
    const int depth = bis_opts().spmv_win8_depth > 0 ? bis_opts().spmv_win8_depth
                      : two ? (sw->R == 1 ? 2 : 3) : (sw->R == 4 ? (ragged ? 2 : 1) : 3);
#define W8_L3(MODE, RR, DD) do { if (sw->slice_rec) W8_L5(MODE, RR, DD, true); else W8_L5(MODE, RR, DD, false); } while (0)
#define W8_L5(MODE, RR, DD, IMPL) do { if (vb == 4) W8_L6(MODE, RR, DD, IMPL, float); else W8_L6(MODE, RR, DD, IMPL, double); } while (0)
#define W8_L6(MODE, RR, DD, IMPL, VT) do { if (two && DD <= 4) W8_L4(MODE, RR, DD, IMPL, VT, (DD <= 4)); else W8_L4(MODE, RR, DD, IMPL, VT, false); } while (0)
#define W8_L4(MODE, RR, DD, IMPL, VT, TWO) hipLaunchKernelGGL((spmv_win8_kernel<MODE, RR, DD, IMPL, VT, TWO>), dim3(grid), dim3(256), lds, ctx->stream, x, y, A->n_rows, A->n_cols, \
                                               sw->n_blocks, remap_arg, w, partials, stop, sw->hdr, sw->slice_chunk0, stream, x_al16, own, sw->row_of, \
                                               reinterpret_cast<const w8_v2u *>(stream + sw->w8_desc), stream + sw->w8_side, sw->slice_rec)
#define W8_L2(MODE, RR) do { if (depth <= 1) W8_L3(MODE, RR, 1); else if (depth == 2) W8_L3(MODE, RR, 2); else if (depth == 3) W8_L3(MODE, RR, 3); else if (depth <= 5) W8_L3(MODE, RR, 4); else W8_L3(MODE, RR, 6); } while (0)
#define W8_L1(MODE) do { if (sw->R == 4) W8_L2(MODE, 4); else if (sw->R == 2) W8_L2(MODE, 2); else W8_L2(MODE, 1); } while (0)
    if (mode == 1) W8_L1(1); else W8_L1(0);
#undef W8_L1
#undef W8_L2
#undef W8_L3
#undef W8_L4
#undef W8_L5
#undef W8_L6
    BIS_HIP_CHECK(ctx, hipGetLastError());
    return BIS_OK;
}
