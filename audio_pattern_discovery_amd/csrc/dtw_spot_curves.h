// What the kernels that read a chunk's curves again share (dtw_spot_detect.hip, dtw_spot_quantile.hip): the walk over the columns
// of one SpotCurve record, and the 64-bit forms of the wavefront shuffles.
#pragma once
#include "apd_internal.h"

namespace apd {

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, uint32_t delta)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, delta, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), delta, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// grid: (pairs of the chunk, column blocks), kColumns work-items; the block walks P's columns kColumns at a time, gridDim.y blocks
// apart, coalesced over the two curves.  body(j, live, cost, start, score) for the calling lane's 0-based columns j: live = j < P.m,
// score = spot_score of the column (zeros when not live).  The trip count is the wavefront's -- j0 is the column of its lane 0 --
// so every lane reaches the body and the body's ballots are wave-uniform.
template <uint32_t kColumns, class Body>
__device__ __forceinline__ void spot_curve_walk(const SpotCurve &P, const float *d_cost, const uint32_t *d_start, Body body)
{
    const float *cost = d_cost + P.curve_off;
    const uint32_t *start = d_start + P.curve_off;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.y * kColumns;
    for (uint64_t j0 = (uint64_t)blockIdx.y * kColumns + (threadIdx.x - lane); j0 < P.m; j0 += stride) {
        const uint64_t j = j0 + lane;
        const bool live = j < P.m;
        const float c = live ? cost[j] : 0.0f;
        const uint32_t s = live ? start[j] : 0u;
        body(j, live, c, s, live ? spot_score(c, (uint32_t)j + 1u, s, P.n) : 0.0f);
    }
}

}  // namespace apd
