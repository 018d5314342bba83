// Warping paths of spotted windows (gfx950): apd_spot_paths.  Which query frame was matched to which stream frame inside a window
// [start, end] that apd_spot reported -- read from the very table apd_spot sweeps, not from a table of the window alone: the tie
// rule of alignments.rs:153-159 (an exact DELETE / INSERT tie takes MATCH even when MATCH is larger) makes the cells inside a
// window depend on the columns before it.  The table never exists; two launches on the context's stream, as dtw_path.hip does it.
//
//   1. the kind SpotRecordSweep: spot_sweep (dtw_spot_sweep.h) with REC = true, one wavefront per DISTINCT (query, stream) pair of the chunk,
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

// One pair of a recording launch: where its intervals, ends and results lie, then spot_sweep -- as spot_stream_pair is for the
// streaming kinds.  Keep it a function of its own: folded into SpotRecordSweep::pair it measured 1 % slower on
// tools/spot_path_bench.py.
template <int RT, int D>
__device__ __forceinline__ void spot_record_pair(const SpotPathLaunch &L)
{
    const SpotRecPair Q = L.d_pairs[blockIdx.x];
    const SpotPair P{Q.px, Q.py, 0u, 0u, 0ull};
    const SpotRecord rec{L.d_intervals + Q.iv_first, Q.n_iv, L.d_ends + Q.end_first, Q.n_ends, L.d_end_cost + Q.end_first,
                         L.d_end_start + Q.end_first, L.d_dirs, Q.max_end};
    spot_sweep<RT, D, true>(L.src, SpotOut{}, P, rec);
}

struct SpotRecordSweep {
    using Launch = SpotPathLaunch;
    static constexpr const char *word = "record";
    template <int RT, int D>
    static __device__ __forceinline__ void pair(const Launch &L) { spot_record_pair<RT, D>(L); }
};

// dtw_spot_trace's source (dtw_spot_trace.h): the words of the interval that holds the window, as the recording sweep left them, the
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
    const SpotTraceJob J = spot_trace_job(L, W.px, W.end, W.start, W.step_off);
    const uint32_t dpad = L.src.dpad;
    const SpotIntervalSource src{L.d_dirs + W.dir_off, W.a, L.src.d_frames + (uint64_t)L.src.d_seq_off[W.py] * dpad, dpad,
                                 L.d_end_cost + W.end_slot, L.d_end_start + W.end_slot};
    spot_trace_window(J, src);
}

hipError_t launch_spot_record(const SpotPathLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    return spot_launch<SpotRecordSweep>(L, L.n_pairs, L.src.dim, rt, r_max, stream);
}

hipError_t launch_spot_trace(const SpotPathLaunch &L, hipStream_t stream)
{
    if (L.n_windows == 0) return hipSuccess;
    hipLaunchKernelGGL(dtw_spot_trace, dim3(L.n_windows), dim3(64), 0, stream, L);
    return hipGetLastError();
}

}  // namespace apd
