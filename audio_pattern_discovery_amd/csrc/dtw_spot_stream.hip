// Streaming spotting (gfx950): the kernels of an apd_spot_stream session.  apd_spot's free-start table, entered and left in
// mid-stream: column j of the table depends on column j - 1 and on nothing else, so a session that keeps rows 1 .. n of the last
// pushed column (value and start) in HBM continues the very same table with the next chunk, and the curves of the pushes, one after
// the other, are the bits of apd_spot on the whole stream (include/apd.h, "streaming spotting").
//
// The sweep is spot_sweep (dtw_spot_sweep.h) with CARRY = true -- one text with apd_spot for the lane mapping, the macro-step and
// the arithmetic, under the one kernel template and launcher of that header.  What a push adds around it -- where the pair's chunk,
// carried column and curves lie -- is spot_stream_pair (dtw_spot_stream.h), which the kind SpotStreamSweep shares with the recording
// kind of a session that keeps a history (dtw_spot_stream_rec.hip).
#include <cstdio>
#include <cstdlib>

#include "dtw_spot_stream.h"

namespace apd {

struct SpotStreamSweep {
    using Launch = SpotStreamLaunch;
    static constexpr const char *word = "stream";
    template <int RT, int D>
    static __device__ __forceinline__ void pair(const Launch &S) { spot_stream_pair<RT, D, false>(S, SpotHistory{}); }
};

// A fresh table for the pairs of `channel` (0xFFFFFFFF: every channel): column 0 (+INF / 0) in both halves of the state, best none.
__global__ __launch_bounds__(64) void spot_stream_reset_kernel(const SpotStreamLaunch S, uint32_t channel)
{
    const SpotStreamPair Q = S.d_pairs[blockIdx.x];
    if (channel != 0xFFFFFFFFu && Q.channel != channel) return;
    const uint32_t column = Q.rows * 64u;
    for (uint32_t half = 0; half < 2; ++half) {
        float *v = S.d_state + half * S.state_half + Q.state_off;
        uint32_t *s = reinterpret_cast<uint32_t *>(v + column);
        for (uint32_t e = threadIdx.x; e < column; e += 64) { v[e] = APD_INF; s[e] = 0u; }
    }
    if (threadIdx.x == 0) {
        apd_spot_best b;
        b.end = 0u; b.start = 0u; b.cost = APD_INF; b.score = APD_INF;
        S.d_best[Q.out] = b;
    }
}

hipError_t launch_spot_stream(const SpotStreamLaunch &S, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    return spot_launch<SpotStreamSweep>(S, S.n_pairs, S.src.dim, rt, r_max, stream);
}

hipError_t launch_spot_stream_reset(const SpotStreamLaunch &S, uint32_t channel, hipStream_t stream)
{
    if (S.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(spot_stream_reset_kernel, dim3(S.n_pairs), dim3(64), 0, stream, S, channel);
    return hipGetLastError();
}

}  // namespace apd
