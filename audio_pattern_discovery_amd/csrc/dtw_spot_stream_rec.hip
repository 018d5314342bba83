// Streaming spotting with a history (gfx950): the kernels of a session that keeps its last H columns (include/apd.h,
// apd_spot_stream_keep / apd_spot_stream_paths).  A window [S, end] is walked back only through cells of
// columns S .. end, and the session sweeps those very cells of the very table once, as the chunks arrive: what it keeps of the last
// H columns -- every cell's branch, row n's value and start, the stream frames -- traces every window that still lies inside them,
// bit for bit as apd_spot_paths would on the whole stream.
//
//   the kind SpotStreamRecordSweep: SpotStreamSweep's sweep (spot_stream_pair, dtw_spot_stream.h) with RING: curves, running best and
//      carried column as before, and every live cell's branch goes to the pair's ring, row n's T and S to its curve ring.  Both are
//      indexed by ABSOLUTE macro-step J + lane modulo H (dtw_spot_sweep.h, SpotRing): one coalesced 256-byte store per macro-step
//      and word, each lane overwriting its own column J - H, whatever the chunking and however often a push wraps.
//   spot_stream_frames_kernel: the last min(m, H) staged frames of every channel's chunk go to the channel's frame ring, column J at
//      row J mod H.  Only those: of a push longer than H two frames would meet in one row.
//   dtw_spot_stream_trace: dtw_spot_trace's walk and replay (dtw_spot_trace.h) reading branch rows and frames through the rings'
//      modulus.  A window whose start lies before the channel's first kept column gets found start and score, and no walk.
#include "dtw_spot_stream.h"
#include "dtw_spot_trace.h"

namespace apd {

struct SpotStreamRecordSweep {
    using Launch = SpotStreamRecLaunch;
    static constexpr const char *word = "streamrec";
    template <int RT, int D>
    static __device__ __forceinline__ void pair(const Launch &A) { spot_stream_pair<RT, D, true>(A.S, A.H); }
};

// One workgroup per staged frame g of the push (grid-stride): its channel k is the one whose chunk [d_push[k], d_push[k + 1]) holds g.
__global__ __launch_bounds__(64) void spot_stream_frames_kernel(const SpotStreamRecLaunch A, uint32_t total)
{
    const SpotStreamLaunch &S = A.S;
    const uint32_t rows = A.H.rows, dpad = S.src.dpad, dp4 = dpad / 4;
    for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
        uint32_t lo = 0, hi = S.n_channels;                                 // the last k with d_push[k] <= g
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (S.d_push[mid] <= g) lo = mid; else hi = mid;
        }
        const uint32_t k = lo, first = S.d_push[k], m = S.d_push[k + 1] - first;
        const uint32_t idx = g - first;                                     // < m: chunks of no frames hold no g
        if (m - idx > rows) continue;                                       // older than the last H of this push
        const uint32_t column = S.d_push[S.n_channels + 1 + k] + idx + 1u;  // absolute; < 2^32: kSpotMaxStream
        const float4 *src = reinterpret_cast<const float4 *>(S.d_stage + (uint64_t)g * dpad);
        float4 *dst = reinterpret_cast<float4 *>(A.H.d_frames + ((uint64_t)k * rows + column % rows) * dpad);
        for (uint32_t e = threadIdx.x; e < dp4; e += 64) dst[e] = src[e];
    }
}

// dtw_spot_stream_trace's source (dtw_spot_trace.h): macro-steps are counted absolutely, lane lu's column j in macro-step j + lu,
// and live in ring row (j + lu) mod H; the rows of a staged window are neither contiguous across the wrap nor, when the stage holds
// more macro-steps than the ring has rows, distinct -- each is fetched through the modulus on its own, and the walk reads only rows
// of the window's own columns, which the ring still holds (the host and walks() see to that).
struct SpotRingSource {
    const uint32_t *dirs;      // the pair's ring
    const float *frames;       // the channel's ring
    uint32_t rows, dpad;
    float cost;                // T[n][end]
    uint32_t start_found;      // S[n][end]
    uint32_t first;            // the channel's first kept column
    __device__ __forceinline__ uint32_t found() const { return start_found; }
    __device__ __forceinline__ float end_cost_of() const { return cost; }
    __device__ __forceinline__ bool walks(uint32_t s) const { return s >= first; }
    __device__ __forceinline__ int64_t row(uint32_t j, int lu) const { return (int64_t)j + lu; }
    __device__ __forceinline__ void stage(uint32_t *dst, int64_t lo, int64_t hi, int row_words, int lane) const
    {
        for (int64_t t = lo; t < hi; ++t) {
            const uint32_t *src = dirs + (uint64_t)((uint64_t)t % rows) * row_words;
            uint32_t *to = dst + (int)(t - lo) * row_words;
            for (int e = lane; e < row_words; e += 64) to[e] = src[e];
        }
    }
    __device__ __forceinline__ const float4 *y(uint32_t j) const { return reinterpret_cast<const float4 *>(frames + (uint64_t)(j % rows) * dpad); }
};

__global__ __launch_bounds__(64) void dtw_spot_stream_trace(const SpotRingTraceLaunch L)
{
    const SpotRingWindow W = L.d_windows[blockIdx.x];
    const uint32_t rows = L.H.rows, dpad = L.src.dpad;
    const SpotTraceJob J = spot_trace_job(L, W.px, W.end, W.start, W.step_off);
    const uint32_t R = ((uint32_t)J.n + 63u) / 64u, lane_n = ((uint32_t)J.n - 1u) / R;
    const uint64_t at = (uint64_t)W.pair * rows + (W.end + lane_n) % rows;  // row n's macro-step of column `end`
    SpotRingSource src;
    src.dirs = L.H.d_dirs + (uint64_t)L.H.d_wpl_before[W.pair] * rows * 64;
    src.frames = L.H.d_frames + (uint64_t)W.channel * rows * dpad;
    src.rows = rows; src.dpad = dpad;
    src.cost = L.H.d_curve_v[at]; src.start_found = L.H.d_curve_s[at];
    src.first = W.first;
    spot_trace_window(J, src);
}

hipError_t launch_spot_stream_record(const SpotStreamRecLaunch &A, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    return spot_launch<SpotStreamRecordSweep>(A, A.S.n_pairs, A.S.src.dim, rt, r_max, stream);
}

hipError_t launch_spot_stream_frames(const SpotStreamRecLaunch &A, uint32_t total, hipStream_t stream)
{
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(spot_stream_frames_kernel, dim3(std::min<uint32_t>(total, 1u << 16)), dim3(64), 0, stream, A, total);
    return hipGetLastError();
}

hipError_t launch_spot_stream_trace(const SpotRingTraceLaunch &L, hipStream_t stream)
{
    if (L.n_windows == 0) return hipSuccess;
    hipLaunchKernelGGL(dtw_spot_stream_trace, dim3(L.n_windows), dim3(64), 0, stream, L);
    return hipGetLastError();
}

}  // namespace apd
