// The walk back and the forward replay of a spotted window (gfx950), shared by dtw_spot_trace (dtw_spot_path.hip: the direction words
// of a recording sweep's interval, the stream resident) and dtw_spot_stream_trace (dtw_spot_stream_rec.hip: the rings of a streaming
// session): ONE text for the walk, the staging of macro-steps in LDS and the replay, templated on where a direction word, a stream
// frame and row n's value and start at `end` come from.
//
// A source Src provides
//   found(), end_cost_of():        S[n][end] and T[n][end] as the sweep left them;
//   walks(found):                 false: the window gets no path whatever the start says (the streaming form: its start has aged out);
//   row(j, lu):                   the index of the macro-step that holds lane lu's column j, counted so that a walk's rows never grow
//                                 and never fall below 0;
//   stage(dst, lo, hi, row_words, lane): copies the words of macro-steps [lo, hi) to dst, row_words each;
//   y(j):                         the resident frame of stream column j.
// The walk: row i lives on lane (i - 1) / R, its macro-step is j - 1 + lane, and the macro-step never grows along the walk (MATCH: -1
// or -2, INSERT: 0 or -1, DELETE: -1), so a window of macro-steps staged in LDS serves many steps (dtw_path_trace's scheme).
#pragma once
#include "dtw_spot_sweep.h"

namespace apd {

constexpr int kSpotTraceStageWords = 2048;                      // 8 KB of direction words staged per window of macro-steps
static_assert(kSpotTraceStageWords / 64 >= (int)((kSpotMaxQuery / 64 + 15) / 16), "a window holds at least one macro-step of the longest query");

// What both forms know of their window.  slot: the window's index in d_len / d_found / d_scores.
struct SpotTraceJob {
    SpotSource src;
    const float *X;        // the query's resident frames
    int n;
    uint32_t end, start;
    uint4 *out;            // the window's slots: {i, j, bits of cost, op}
    uint32_t *d_len, *d_found;
    float *d_scores;
    uint32_t slot;
};
// The job of window blockIdx.x of either trace launch L: the query at resident position px, the caller's window [start, end], the
// window's first step slot in L.d_steps.
template <class L>
__device__ __forceinline__ SpotTraceJob spot_trace_job(const L &l, uint32_t px, uint32_t end, uint32_t start, uint64_t step_off)
{
    const uint32_t ox = l.src.d_seq_off[px];
    return {l.src, l.src.d_frames + (uint64_t)ox * l.src.dpad, (int)(l.src.d_seq_off[px + 1] - ox) - 2, end, start,
            reinterpret_cast<uint4 *>(l.d_steps + step_off), l.d_len, l.d_found, l.d_scores, blockIdx.x};
}

template <class Src>
__device__ __forceinline__ void spot_trace_window(const SpotTraceJob W, const Src src)
{
    __shared__ uint32_t stage[kSpotTraceStageWords];
    __shared__ float s_wd[64];
    __shared__ uint32_t s_op[64];
    const int lane = threadIdx.x;
    const int n = W.n;
    const float *X = W.X;
    uint4 *out = W.out;
    const uint32_t bound = (uint32_t)n + (W.end - W.start + 1u);      // apd_spot_path_bound; < 2^32: kSpotMaxStream
    const int R = (n + 63) / 64;
    const int wpl = (R + 15) >> 4;
    const int row_words = wpl * 64;
    const int window = kSpotTraceStageWords / row_words;              // macro-steps per staged window, >= 1
    const uint32_t found = src.found();                               // S[n][end] and T[n][end] as the sweep carried them
    const float end_cost = src.end_cost_of();

    // ---- walk back (every lane runs the same walk; lane k % 64 keeps step k until the next flush)
    int i = n;
    uint32_t j = W.end;
    int lu = (n - 1) / R, r = (n - 1) - lu * R;                      // row i is row r of lane lu
    bool go = found == W.start && src.walks(found);                  // the caller's start is checked, not trusted
    int64_t lo = 0, hi = 0;                                          // staged macro-steps [lo, hi)
    uint32_t k = 0, mi = 0, mj = 0, mop = 0;
    while (go && k < bound) {
        uint32_t op;
        if (i == 0) {
            op = APD_PATH_START;
        } else {
            const int64_t row = src.row(j, lu);
            if (row < lo || row >= hi) {
                __syncthreads();
                hi = row + 1;
                lo = hi > window ? hi - window : 0;
                src.stage(stage, lo, hi, row_words, lane);
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
        if (i >= 1 && j < W.start) go = false;                       // never with a start that matched; keeps every read inside the window's columns
    }
    const uint32_t len = k;
    if ((k & 63u) != 0u && (uint32_t)lane < (k & 63u)) out[bound - 1 - ((k & ~63u) + lane)] = make_uint4(mi, mj, 0u, mop);
    __threadfence();                                                 // the replay reads the slots other lanes have just written
    __syncthreads();

    // ---- replay forward: slot bound - len + s holds path step s; step s goes to slot s (never ahead of what is still unread)
    const int dp4 = (int)W.src.dpad / 4, dim = (int)W.src.dim;
    float carry = APD_INF;
    for (uint32_t s = 0; s < len; s += 64) {
        const uint32_t idx = s + lane;
        const bool live = idx < len;
        uint4 st = make_uint4(0u, 0u, 0u, 0u);
        float wd = 0.0f;
        if (live) {
            st = out[bound - len + idx];
            if (st.w != APD_PATH_START) {
                const float4 *xa = reinterpret_cast<const float4 *>(X + (uint64_t)(st.x - 1) * W.src.dpad);
                const float4 *yb = src.y(st.y);
                const float d = __builtin_sqrtf(spot_sq_distance_any(xa, yb, dp4, dim));
                const float pen = st.w == APD_PATH_DELETE ? W.src.del : st.w == APD_PATH_INSERT ? W.src.ins : W.src.mat;
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
        W.d_len[W.slot] = len;
        W.d_found[W.slot] = found;
        W.d_scores[W.slot] = spot_score(end_cost, W.end, found, (uint32_t)n);   // as the sweep scores its running best
    }
}

}  // namespace apd
