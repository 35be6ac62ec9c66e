// bis_lockstep.hpp -- what the lock-step solvers on n x k interleaved blocks share (bis_mcg.hip, bis_mbicgstab.hip): the
// lane-to-column map's constants and the per-column last-arriver reductions.  A lane of an elementwise pass owns ONE column:
// the first act = (kT / k) k lanes of a workgroup work, lane t on column t % k, on the flat index range.  A column's partial
// sums are folded in lane order, the workgroups' partials are summed by the last arriver in index order: a column's bits
// depend on (n, k, its own data) only.
#pragma once

#include "bis_solver.hpp"

#include <algorithm>

namespace bis_lockstep {

constexpr int kT = kSolverT;
constexpr int kMaxK = 8;
// one last-arriver counter set per reduction; every reducing pass is launched with lockstep_grid, capped at kMaxReduceBlocks
constexpr unsigned kCounterSet = bis_counter_set_words(kMaxReduceBlocks);

// per-column sums of a workgroup: lane t < act holds a partial of column t % k; thread 0 publishes the k (or 2 k) sums and
// takes the ticket.  Returns (in every lane) whether this workgroup arrived last.
template <int NV>
__device__ __forceinline__ bool fold_and_arrive(const double (&v)[NV], int k, int act, double *lds /*[NV][kT]*/, double *partials,
                                                size_t stride, unsigned *counter) {
    __shared__ bool last;
    __shared__ double sums[NV * kMaxK];
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NV; ++q) lds[q * kT + t] = v[q];
    __syncthreads();
    if (t < NV * k) { // lane (q, j): column j's partials in lane order
        const int q = t / k, j = t - q * k;
        double s = 0.0;
        for (int i = j; i < act; i += k) s += lds[q * kT + i];
        sums[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        for (int i = 0; i < NV * k; ++i) publish(partials + (size_t)i * stride + blockIdx.x, sums[i]);
        last = arrive_last_set(counter, blockIdx.x, gridDim.x);
    }
    __syncthreads();
    return last;
}

// the last workgroup: out[i] (valid in thread 0) = sum over the workgroups of value i's partials, in a fixed order: 16 lanes
// per value (NV k <= 16 values), lane l sums the workgroups l, l + 16, ... in index order, thread 0 the 16 lane sums in lane order
template <int NV>
__device__ __forceinline__ void sum_partials(int k, const double *partials, size_t stride, double *lds /*[kT]*/, double (&out)[NV * kMaxK]) {
    const int t = threadIdx.x, v = t >> 4, l = t & 15;
    double a = 0.0;
    if (v < NV * k)
        for (int b = l; b < (int)gridDim.x; b += 16) a += fetch(partials + (size_t)v * stride + b);
    lds[t] = a;
    __syncthreads();
    if (t == 0)
        for (int i = 0; i < NV * k; ++i) {
            double s = 0.0;
            for (int q = 0; q < 16; ++q) s += lds[i * 16 + q];
            out[i] = s;
        }
}

// workgroups of an elementwise pass over an n x k block
inline int lockstep_grid(int64_t n, int k) {
    const int act = (kT / k) * k;
    int64_t g = (n * k + act - 1) / act;
    return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kMaxReduceBlocks);
}

} // namespace bis_lockstep
