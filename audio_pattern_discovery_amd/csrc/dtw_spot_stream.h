// One pair of a streaming push (gfx950), shared by the kinds SpotStreamSweep (dtw_spot_stream.hip) and SpotStreamRecordSweep
// (dtw_spot_stream_rec.hip): where the pair's chunk, carried column, curves and -- with RING -- rings lie, then spot_sweep
// (dtw_spot_sweep.h).  The query rows come from the templates' batch, the stream columns from the session's staging buffer (the
// chunk in the resident layout), the carried column from one half of the state buffer and the new one goes to the other half (the
// per-channel parity word says which).
#pragma once
#include "dtw_spot_sweep.h"

namespace apd {

template <int RT, int D, bool RING>
__device__ __forceinline__ void spot_stream_pair(const SpotStreamLaunch &S, const SpotHistory &H)
{
    const SpotStreamPair Q = S.d_pairs[blockIdx.x];
    const uint32_t first = S.d_push[Q.channel], m = S.d_push[Q.channel + 1] - first;
    if (m == 0) return;                                                     // nothing pushed on this channel: state, best, parity and rings stay
    const uint32_t base = S.d_push[S.n_channels + 1 + Q.channel];
    const uint32_t parity = S.d_push[2 * S.n_channels + 1 + Q.channel] & 1u;
    const SpotOut O{S.d_cost, S.d_start, S.d_best};
    SpotPair P{};
    P.px = Q.px; P.out = Q.out;
    // pair p = channel n_queries + q owns m entries behind those of the pairs before it
    P.curve_off = (uint64_t)S.n_queries * first + (uint64_t)(Q.out - Q.channel * S.n_queries) * m;
    const uint64_t column = (uint64_t)Q.rows * 64;                          // floats of a pair's values; its starts lie behind them
    float *in = S.d_state + parity * S.state_half + Q.state_off, *out = S.d_state + (parity ^ 1u) * S.state_half + Q.state_off;
    SpotCarry C;
    C.y = S.d_stage + (uint64_t)first * S.src.dpad;
    C.m = m; C.base = base;
    C.in_v = in; C.in_s = reinterpret_cast<const uint32_t *>(in + column);
    C.out_v = out; C.out_s = reinterpret_cast<uint32_t *>(out + column);
    if constexpr (RING) {
        SpotRing G;
        G.dirs = H.d_dirs + (uint64_t)H.d_wpl_before[Q.out] * H.rows * 64;
        G.curve_v = H.d_curve_v + (uint64_t)Q.out * H.rows;
        G.curve_s = H.d_curve_s + (uint64_t)Q.out * H.rows;
        G.rows = H.rows;
        spot_sweep<RT, D, false, true, true>(S.src, O, P, SpotRecord{}, C, G);
    } else {
        spot_sweep<RT, D, false, true>(S.src, O, P, SpotRecord{}, C);
    }
}

}  // namespace apd
