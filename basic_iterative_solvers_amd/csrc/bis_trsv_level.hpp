// bis_trsv_level.hpp -- what the level-scheduled sweeps on one vector (bis_sptrsv.hip) and on several (bis_sptrsm.hip)
// share: the hand-off constants ("the data IS the flag": a scratch pre-filled with a NaN sentinel, results published into it),
// the bound of every wait, and the kernels that build the position table of a level-ordered scratch.  Each translation unit
// gets its own copy of the kernels (no relocatable device code); the source is one.
#pragma once
#include "bis_internal.hpp"

namespace {

constexpr unsigned long long kSentinel = 0x7FF85EA71E55C0DEull; // quiet NaN + payload
constexpr unsigned long long kCanonNaN = 0x7FF8000000000000ull;
constexpr unsigned kSpinLimit = 1u << 20; // polls of one row before it gives up and publishes NaN (about a second)
constexpr unsigned kFaultPollMask = 1023u; // a waiting row reads the context's fault word every 1024 polls: once ANY wait of the
                                           // sweep has given up, every other wait ends within a millisecond and later rows do not
                                           // wait at all -- a starved or lost hand-off drains the grid at once instead of row by row
__device__ __forceinline__ bool fault_raised(const unsigned *fault) {
    return __hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
}

__global__ __launch_bounds__(256) void invert_perm_kernel(const int32_t *__restrict__ perm, int64_t n,
                                                          int32_t *__restrict__ inv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) inv[perm[i]] = (int32_t)i;
}

__global__ __launch_bounds__(256) void cols_to_positions_kernel(const int32_t *__restrict__ col,
                                                                const int32_t *__restrict__ inv,
                                                                int64_t nnz, int32_t *__restrict__ pcol) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += stride) pcol[k] = inv[col[k]];
}

} // namespace
