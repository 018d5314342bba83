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
#include "dtw_spot_sweep.h"

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

constexpr int kSpotTraceStageWords = 2048;                      // 8 KB of direction words staged per window of macro-steps
static_assert(kSpotTraceStageWords / 64 >= (int)((kSpotMaxQuery / 64 + 15) / 16), "a window holds at least one macro-step of the longest query");

__global__ __launch_bounds__(64) void dtw_spot_trace(const SpotPathLaunch L)
{
    __shared__ uint32_t stage[kSpotTraceStageWords];
    __shared__ float s_wd[64];
    __shared__ uint32_t s_op[64];
    const int lane = threadIdx.x;
    const SpotTraceWindow W = L.d_windows[blockIdx.x];
    const uint32_t ox = L.d_seq_off[W.px], oy = L.d_seq_off[W.py];
    const int n = (int)(L.d_seq_off[W.px + 1] - ox) - 2;
    const float *X = L.d_frames + (uint64_t)ox * L.dpad;
    const float *Y = L.d_frames + (uint64_t)oy * L.dpad;
    uint4 *out = reinterpret_cast<uint4 *>(L.d_steps + W.step_off);   // {i, j, bits of cost, op}
    const uint32_t bound = (uint32_t)n + (W.end - W.start + 1u);      // apd_spot_path_bound; < 2^32: kSpotMaxStream
    const int R = (n + 63) / 64;
    const int wpl = (R + 15) >> 4;
    const int row_words = wpl * 64;
    const int window = kSpotTraceStageWords / row_words;              // macro-steps per staged window, >= 1
    const uint32_t *dirs = L.d_dirs + W.dir_off;
    const uint32_t found = L.d_end_start[W.end_slot];                 // S[n][end] and T[n][end] as the sweep carried them
    const float end_cost = L.d_end_cost[W.end_slot];

    // ---- walk back (every lane runs the same walk; lane k % 64 keeps step k until the next flush)
    int i = n;
    uint32_t j = W.end;
    int lu = (n - 1) / R, r = (n - 1) - lu * R;                      // row i is row r of lane lu
    bool go = found == W.start;                                      // the caller's start is checked, not trusted
    int64_t lo = 0, hi = 0;                                          // staged macro-steps [lo, hi), counted from the interval's first
    uint32_t k = 0, mi = 0, mj = 0, mop = 0;
    while (go && k < bound) {
        uint32_t op;
        if (i == 0) {
            op = APD_PATH_START;
        } else {
            const int64_t row = (int64_t)(j - W.a) + lu;            // j >= start >= a: inside the interval's (b - a + 64) macro-steps
            if (row < lo || row >= hi) {
                __syncthreads();
                hi = row + 1;
                lo = hi > window ? hi - window : 0;
                const int words = (int)(hi - lo) * row_words;
                const uint64_t base = (uint64_t)lo * row_words;
                for (int e = lane; e < words; e += 64) stage[e] = dirs[base + e];
                __syncthreads();
            }
            const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[((int)(row - lo) * wpl + (r >> 4)) * 64 + lu]);
            op = (word >> (2 * (r & 15))) & 3u;
        }
        if ((int)(k & 63u) == lane) { mi = (uint32_t)i; mj = j; mop = op; }
        ++k;
        if ((k & 63u) == 0u) out[bound - 1 - (k - 64 + lane)] = make_uint4(mi, mj, 0u, mop);
        if (op == APD_PATH_START) break;
        if (op != APD_PATH_DELETE) { --i; if (--r < 0) { r = R - 1; --lu; } }
        if (op != APD_PATH_INSERT) --j;
        if (i >= 1 && j < W.start) go = false;                       // never with a start that matched; keeps every read inside the interval
    }
    const uint32_t len = k;
    if ((k & 63u) != 0u && (uint32_t)lane < (k & 63u)) out[bound - 1 - ((k & ~63u) + lane)] = make_uint4(mi, mj, 0u, mop);
    __threadfence();                                                 // the replay reads the slots other lanes have just written
    __syncthreads();

    // ---- replay forward: slot bound - len + s holds path step s; step s goes to slot s (never ahead of what is still unread)
    const int dp4 = (int)L.dpad / 4, dim = (int)L.dim;
    float carry = APD_INF;
    for (uint32_t s = 0; s < len; s += 64) {
        const uint32_t idx = s + lane;
        const bool live = idx < len;
        uint4 st = make_uint4(0u, 0u, 0u, 0u);
        float wd = 0.0f;
        if (live) {
            st = out[bound - len + idx];
            if (st.w != APD_PATH_START) {
                const float4 *xa = reinterpret_cast<const float4 *>(X + (uint64_t)(st.x - 1) * L.dpad);
                const float4 *yb = reinterpret_cast<const float4 *>(Y + (uint64_t)(st.y - 1) * L.dpad);
                const float d = __builtin_sqrtf(spot_sq_distance_any(xa, yb, dp4, dim));
                const float pen = st.w == APD_PATH_DELETE ? L.del : st.w == APD_PATH_INSERT ? L.ins : L.mat;
                wd = pen * d;                                        // rounded on its own, then added
            }
        }
        s_wd[lane] = wd;
        s_op[lane] = st.w;
        __syncthreads();
        const int count = (int)min(64u, len - s);
        float mine = 0.0f;
        for (int t = 0; t < count; ++t) {
            const float v = s_op[t] == APD_PATH_START ? 0.0f : carry + s_wd[t];   // T[0][j] = 0
            carry = v;
            if (t == lane) mine = v;
        }
        __syncthreads();
        if (live) out[idx] = make_uint4(st.x, st.y, __builtin_bit_cast(uint32_t, mine), st.w);
    }
    __syncthreads();
    for (uint32_t idx = len + lane; idx < bound; idx += 64) out[idx] = make_uint4(0u, 0u, 0u, 0u);   // unused slots read as zeros
    if (lane == 0) {
        L.d_len[blockIdx.x] = len;
        L.d_found[blockIdx.x] = found;
        const uint32_t covered = W.end - found + 1u;                 // frames of y the alignment covers, as dtw_spot counts them
        L.d_scores[blockIdx.x] = end_cost / (float)((uint32_t)n + covered);
    }
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
