// Warping paths of spotted windows (gfx950): apd_spot_paths.  Which query frame was matched to which stream frame inside a window
// [start, end] that apd_spot reported -- read from the very table apd_spot sweeps, not from a table of the window alone: the tie
// rule of alignments.rs:153-159 (an exact DELETE / INSERT tie takes MATCH even when MATCH is larger) makes the cells inside a
// window depend on the columns before it.  The table never exists; two launches on the context's stream, as dtw_path.hip does it.
//
//   1. dtw_spot_record: spot_sweep (dtw_spot_sweep.h) with REC = true, one wavefront per DISTINCT (query, stream) pair of the chunk,
//      however many windows the pair has.  It starts at column 1 -- a cell's value and branch depend on every column before it --
//      and stops after the pair's largest requested end.  The branch of every live cell whose column lies in one of the pair's
//      intervals (the union of its windows, merged on the host) goes to HBM at 2 bits per cell, 64 consecutive words per store;
//      the lane that owns row n leaves T[n][end] and S[n][end] for every requested end.
//   2. dtw_spot_trace: one wavefront per window.  The caller's start is checked against S[n][end], not trusted: a window whose
//      start differs gets no path.  Otherwise the walk goes back from (n, end) through the interval's words -- row i lives on lane
//      (i - 1) / R, its macro-step is tau = j - 1 + lane, and tau never grows along the walk (MATCH: -1 or -2, INSERT: 0 or -1,
//      DELETE: -1), so dtw_path_trace's staging of a window of macro-steps in LDS carries over -- until it reaches row 0, where it
//      emits START.  It stays inside columns start .. end (S is the column in which the alignment left row 0), so inside the
//      interval.  The replay then goes forward, 64 steps at a time, exactly as dtw_path_trace's: a table value IS predecessor +
//      pen * d in these operations, so the replayed costs are the table's bits and the last one is apd_spot's cost at `end`.
#include "dtw_spot_trace.h"

namespace apd {

template <int RT, int D>
__global__ __launch_bounds__(64) void dtw_spot_record(const SpotPathLaunch L)
{
    const SpotRecPair Q = L.d_pairs[blockIdx.x];
    SpotLaunch S{};
    S.d_frames = L.d_frames; S.d_seq_off = L.d_seq_off; S.dim = L.dim; S.dpad = L.dpad;
    S.ins = L.ins; S.del = L.del; S.mat = L.mat;
    const SpotPair P{Q.px, Q.py, 0u, 0u, 0ull};
    const SpotRecord rec{L.d_intervals + Q.iv_first, Q.n_iv, L.d_ends + Q.end_first, Q.n_ends, L.d_end_cost + Q.end_first,
                         L.d_end_start + Q.end_first, L.d_dirs, Q.max_end};
    spot_sweep<RT, D, true>(S, P, rec);
}

// dtw_spot_trace's source (dtw_spot_trace.h): the words of the interval that holds the window, as dtw_spot_record left them, the
// stream resident in the batch, row n's value and start at the pair's requested ends.
struct SpotIntervalSource {
    const uint32_t *dirs;      // the interval's first word
    uint32_t a;                // its first column
    const float *Y;
    uint32_t dpad;
    const float *end_cost;
    const uint32_t *end_start;
    __device__ __forceinline__ uint32_t found() const { return *end_start; }
    __device__ __forceinline__ float end_cost_of() const { return *end_cost; }
    __device__ __forceinline__ bool walks(uint32_t) const { return true; }
    // j >= start >= a: inside the interval's (b - a + 64) macro-steps, counted from the interval's first
    __device__ __forceinline__ int64_t row(uint32_t j, int lu) const { return (int64_t)(j - a) + lu; }
    __device__ __forceinline__ void stage(uint32_t *dst, int64_t lo, int64_t hi, int row_words, int lane) const
    {
        const int words = (int)(hi - lo) * row_words;
        const uint64_t base = (uint64_t)lo * row_words;
        for (int e = lane; e < words; e += 64) dst[e] = dirs[base + e];
    }
    __device__ __forceinline__ const float4 *y(uint32_t j) const { return reinterpret_cast<const float4 *>(Y + (uint64_t)(j - 1) * dpad); }
};

__global__ __launch_bounds__(64) void dtw_spot_trace(const SpotPathLaunch L)
{
    const SpotTraceWindow W = L.d_windows[blockIdx.x];
    const uint32_t ox = L.d_seq_off[W.px], oy = L.d_seq_off[W.py];
    SpotTraceJob J;
    J.X = L.d_frames + (uint64_t)ox * L.dpad;
    J.n = (int)(L.d_seq_off[W.px + 1] - ox) - 2;
    J.dim = L.dim; J.dpad = L.dpad;
    J.ins = L.ins; J.del = L.del; J.mat = L.mat;
    J.end = W.end; J.start = W.start;
    J.out = reinterpret_cast<uint4 *>(L.d_steps + W.step_off);
    J.d_len = L.d_len; J.d_found = L.d_found; J.d_scores = L.d_scores;
    J.slot = blockIdx.x;
    const SpotIntervalSource src{L.d_dirs + W.dir_off, W.a, L.d_frames + (uint64_t)oy * L.dpad, L.dpad, L.d_end_cost + W.end_slot,
                                 L.d_end_start + W.end_slot};
    spot_trace_window(J, src);
}

namespace {

template <int RT, int D>
hipError_t launch_record_as(const SpotPathLaunch &L, uint32_t r_max, hipStream_t stream)
{
    const size_t lds_bytes = RT > 0 ? 0 : spot_lds_bytes(r_max);
    spot_debug_line("record", RT, D, L.n_pairs, r_max, lds_bytes);
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_spot_record<RT, D>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((dtw_spot_record<RT, D>), dim3(L.n_pairs), dim3(64), lds_bytes, stream, L);
    return hipGetLastError();
}

template <int D>
hipError_t launch_record_rows(const SpotPathLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    switch (rt) {
        case 1: return launch_record_as<1, D>(L, r_max, stream);
        case 2: return launch_record_as<2, D>(L, r_max, stream);
        case 3: return launch_record_as<3, D>(L, r_max, stream);
        case 4: return launch_record_as<4, D>(L, r_max, stream);
        default: return launch_record_as<0, D>(L, r_max, stream);
    }
}

}  // namespace

hipError_t launch_spot_record(const SpotPathLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    if (L.n_pairs == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    const bool typed = with_kernel_dim(L.dim, [&](auto d) { e = launch_record_rows<decltype(d)::value>(L, rt, r_max, stream); });
    if (!typed) e = launch_record_as<0, 0>(L, r_max, stream);            // any other dimension: frames re-read per cell, column in LDS
    return e;
}

hipError_t launch_spot_trace(const SpotPathLaunch &L, hipStream_t stream)
{
    if (L.n_windows == 0) return hipSuccess;
    hipLaunchKernelGGL(dtw_spot_trace, dim3(L.n_windows), dim3(64), 0, stream, L);
    return hipGetLastError();
}

}  // namespace apd
