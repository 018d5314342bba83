// Streaming spotting with a history (gfx950): the kernels of a session that keeps its last H columns (include/apd.h,
// apd_spot_stream_keep / apd_spot_stream_paths).  A window [S, end] is walked back only through cells of
// columns S .. end, and the session sweeps those very cells of the very table once, as the chunks arrive: what it keeps of the last
// H columns -- every cell's branch, row n's value and start, the stream frames -- traces every window that still lies inside them,
// bit for bit as apd_spot_paths would on the whole stream.
//
//   dtw_spot_stream_record<RT, D>: dtw_spot_stream's sweep (spot_stream_pair, dtw_spot_stream.h) with RING: curves, running best and
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

template <int RT, int D>
__global__ __launch_bounds__(64) void dtw_spot_stream_record(const SpotStreamRecLaunch A)
{
    spot_stream_pair<RT, D, true>(A.S, A.H);
}

// One workgroup per staged frame g of the push (grid-stride): its channel k is the one whose chunk [d_push[k], d_push[k + 1]) holds g.
__global__ __launch_bounds__(64) void spot_stream_frames_kernel(const SpotStreamRecLaunch A, uint32_t total)
{
    const SpotStreamLaunch &S = A.S;
    const uint32_t rows = A.H.rows, dp4 = S.dpad / 4;
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
        const float4 *src = reinterpret_cast<const float4 *>(S.d_stage + (uint64_t)g * S.dpad);
        float4 *dst = reinterpret_cast<float4 *>(A.H.d_frames + ((uint64_t)k * rows + column % rows) * S.dpad);
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
    const uint32_t ox = L.d_seq_off[W.px], rows = L.H.rows;
    SpotTraceJob J;
    J.X = L.d_frames + (uint64_t)ox * L.dpad;
    J.n = (int)(L.d_seq_off[W.px + 1] - ox) - 2;
    J.dim = L.dim; J.dpad = L.dpad;
    J.ins = L.ins; J.del = L.del; J.mat = L.mat;
    J.end = W.end; J.start = W.start;
    J.out = reinterpret_cast<uint4 *>(L.d_steps + W.step_off);
    J.d_len = L.d_len; J.d_found = L.d_found; J.d_scores = L.d_scores;
    J.slot = blockIdx.x;
    const uint32_t R = ((uint32_t)J.n + 63u) / 64u, lane_n = ((uint32_t)J.n - 1u) / R;
    const uint64_t at = (uint64_t)W.pair * rows + (W.end + lane_n) % rows;  // row n's macro-step of column `end`
    SpotRingSource src;
    src.dirs = L.H.d_dirs + (uint64_t)L.H.d_wpl_before[W.pair] * rows * 64;
    src.frames = L.H.d_frames + (uint64_t)W.channel * rows * L.dpad;
    src.rows = rows; src.dpad = L.dpad;
    src.cost = L.H.d_curve_v[at]; src.start_found = L.H.d_curve_s[at];
    src.first = W.first;
    spot_trace_window(J, src);
}

namespace {

template <int RT, int D>
hipError_t launch_stream_record_as(const SpotStreamRecLaunch &A, uint32_t r_max, hipStream_t stream)
{
    const size_t lds_bytes = RT > 0 ? 0 : spot_lds_bytes(r_max);
    spot_debug_line("streamrec", RT, D, A.S.n_pairs, r_max, lds_bytes);
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_spot_stream_record<RT, D>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((dtw_spot_stream_record<RT, D>), dim3(A.S.n_pairs), dim3(64), lds_bytes, stream, A);
    return hipGetLastError();
}

template <int D>
hipError_t launch_stream_record_rows(const SpotStreamRecLaunch &A, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    switch (rt) {
        case 1: return launch_stream_record_as<1, D>(A, r_max, stream);
        case 2: return launch_stream_record_as<2, D>(A, r_max, stream);
        case 3: return launch_stream_record_as<3, D>(A, r_max, stream);
        case 4: return launch_stream_record_as<4, D>(A, r_max, stream);
        default: return launch_stream_record_as<0, D>(A, r_max, stream);
    }
}

}  // namespace

// The pairs of A.S all belong to one class (spot_row_class), as for launch_spot_stream.
hipError_t launch_spot_stream_record(const SpotStreamRecLaunch &A, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    if (A.S.n_pairs == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    const bool typed = with_kernel_dim(A.S.dim, [&](auto d) { e = launch_stream_record_rows<decltype(d)::value>(A, rt, r_max, stream); });
    if (!typed) e = launch_stream_record_as<0, 0>(A, r_max, stream);     // any other dimension: frames re-read per cell, column in LDS
    return e;
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
