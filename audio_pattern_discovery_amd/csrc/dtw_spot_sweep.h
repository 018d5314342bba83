// The sweep of the free-start table (gfx950), shared by apd_spot (dtw_spot.hip, REC = false) and by the recording sweep of
// apd_spot_paths (dtw_spot_path.hip, REC = true): ONE text for the lane mapping, the macro-step and the arithmetic, so that the
// branches the second records are the branches of the very table the first reports.  What REC adds is compiled out of apd_spot's
// instantiations (`if constexpr`): the same instruction mix, no scratch, registers within 2 of what they were and the same measured
// speed as before this header existed.  The streaming session (dtw_spot_stream.hip, CARRY = true) enters the
// same table behind any column and leaves it for the next chunk; what CARRY adds is compiled out of the other two likewise
// (DESIGN.md section 4.13).  A session that keeps a history (dtw_spot_stream_rec.hip, CARRY and RING) does all of CARRY and stores the
// branches and row n's curve of every column into the pair's rings; what RING adds is compiled out of the other three (section 4.14).
//
// One wavefront per (query, stream) pair.  Rows go on lanes, the stream flows through: lane l owns the R = ceil(n / 64) query rows
// l R + 1 .. l R + R, macro-step tau gives it stream column j = tau - l + 1, and m + (lane of row n) macro-steps cover the pair.
// What a cell needs:
//   DELETE  (i, j-1): the lane's own previous column -- R values and R starts, in registers for R <= 4 (RT = R), else in dynamic LDS
//                     laid out [r][lane] (RT = 0; conflict-free, as the path sweep keeps its row);
//   INSERT  (i-1, j): the row above in the same macro-step; for the lane's first row the lower lane's last row of column j, which
//                     that lane computed one macro-step earlier: one from_lower_lane each for value and start;
//   MATCH (i-1, j-1): the row above one column earlier; for the first row what arrived from the lower lane one macro-step earlier.
// Lane 0 has no lower lane: it reads row 0, value 0 and start j.  Cells of columns outside 1 .. m and of rows beyond n hold +INF
// (start 0) and reach no output.
//
// Arithmetic: numerics.rs:114-120 / alignments.rs:153-159 operation for operation, always (the context's distance mode is not
// read).  D: the resident frame dimension as a compile-time constant (frames in registers), 0 = any dimension (frames re-read per
// cell, as dtw_path.hip does).  The register variants take the square roots of a macro-step with sqrt_rn_finite when every squared
// distance of the wavefront is inside its domain, and with the compiler's general sequence otherwise (identical frames, infinities,
// NaN): the bits are the same either way (dtw_common.h).
#pragma once
#include "dtw_common.h"

namespace apd {

// the select of dtw_path.hip's select_node_branch, carrying the start column of the chosen predecessor beside the branch
struct SpotNode { float value; uint32_t start; uint32_t op; };
template <bool REC>
__device__ __forceinline__ SpotNode spot_select(float del_v, uint32_t del_s, float ins_v, uint32_t ins_s, float m_v, uint32_t m_s, float d,
                                                float del_pen, float ins_pen, float mat_pen)
{
    const bool pick_d = (del_v < m_v) & (del_v < ins_v);
    const bool pick_i = (ins_v < m_v) & (ins_v < del_v);
    float base = pick_i ? ins_v : m_v;
    base = pick_d ? del_v : base;
    float pen = pick_i ? ins_pen : mat_pen;
    pen = pick_d ? del_pen : pen;
    uint32_t s = pick_i ? ins_s : m_s;
    s = pick_d ? del_s : s;
    const float weighted = pen * d;                               // rounded on its own (alignments.rs:154-158)
    uint32_t op = 0u;                                             // the branch: the recording sweep only
    if constexpr (REC) op = pick_d ? (uint32_t)APD_PATH_DELETE : pick_i ? (uint32_t)APD_PATH_INSERT : (uint32_t)APD_PATH_MATCH;
    return {base + weighted, s, op};
}

// numerics.rs:114-120 up to the square root: every difference, square and partial sum rounded on its own
template <int D, int DN>
__device__ __forceinline__ float spot_sq_distance(const float (&x)[DN], const float (&y)[DN])
{
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const float t = x[k] - y[k];
        const float sq = t * t;
        acc = acc + sq;
    }
    return acc;
}
// the same for any dimension, both frames from memory (slots >= dim of a resident frame hold the squared norm / padding)
__device__ __forceinline__ float spot_sq_distance_any(const float4 *xa, const float4 *yb, int dp4, int dim)
{
    float acc = 0.0f;
    for (int q = 0; q < dp4; ++q) {
        const float4 xv = xa[q], yv = yb[q];
        const int k0 = 4 * q;
        float t = xv.x - yv.x, sq = t * t;
        acc = (k0 < dim) ? acc + sq : acc;
        t = xv.y - yv.y; sq = t * t; acc = (k0 + 1 < dim) ? acc + sq : acc;
        t = xv.z - yv.z; sq = t * t; acc = (k0 + 2 < dim) ? acc + sq : acc;
        t = xv.w - yv.w; sq = t * t; acc = (k0 + 3 < dim) ? acc + sq : acc;
    }
    return acc;
}

template <int DN>
__device__ __forceinline__ void spot_load_frame(float (&f)[DN], const float *p)
{
#pragma unroll
    for (int q = 0; q < DN / 4; ++q) {
        const float4 v = reinterpret_cast<const float4 *>(p)[q];
        f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
    }
}

__device__ __forceinline__ uint32_t from_lower_lane_u32(uint32_t v, uint32_t fill)
{
    return __builtin_bit_cast(uint32_t, from_lower_lane(__builtin_bit_cast(float, v), __builtin_bit_cast(float, fill)));
}

// What the recording sweep (REC) is given for its pair; apd_spot passes an empty one that nothing reads.
//   iv[0 .. n_iv): the columns whose branches are wanted, as sorted disjoint intervals [a, b] with the first word of each in dirs.
//     A live cell of column j in interval k belongs to macro-step j - 1 + lane; the lane packs the branches of its R rows at 2 bits
//     each, 16 rows per word, WPL = ceil(R / 16) words, at dirs[off_k + ((j - a_k + lane) * WPL + w) * 64 + lane]: indexed by
//     macro-step, so the 64 lanes of a store are 64 consecutive words; an interval of L columns owns (L + 63) WPL 64 words.
//   ends[0 .. n_ends): the columns, ascending, whose T[n][j] and S[n][j] go to end_cost / end_start at the same index.
//   max_end: the last column swept (the largest of ends).
struct SpotRecord {
    const SpotInterval *iv;
    uint32_t n_iv;
    const uint32_t *ends;
    uint32_t n_ends;
    float *end_cost;
    uint32_t *end_start;
    uint32_t *dirs;
    uint32_t max_end;
};

// What the streaming sweep (CARRY) is given for its pair: the table is entered behind absolute column `base` and left behind column
// base + m.  The stream side is the chunk alone -- m >= 1 frames at y in the resident layout, src's frames and offsets serve the
// query only and P.py is not read -- and the column the table was left in last time comes from in_v / in_s, laid out [r][lane] like
// the LDS column: T[i][base] and S[i][base] of the lane's rows, +INF / 0 for column 0 and for rows beyond n.  Every lane with a
// live row stores its column base + m to out_v / out_s behind the loop.  The session keeps in and out apart (two buffers taking
// turns), so that nothing depends on the order in which the lanes of a wavefront read the old column and write the new one.
// The running best starts from out.d_best[P.out] instead of +INF, and starts and ends are absolute columns.
struct SpotCarry {
    const float *y;
    uint32_t m;
    uint32_t base;
    const float *in_v;
    const uint32_t *in_s;
    float *out_v;
    uint32_t *out_s;
};

// What the recording streaming sweep (RING, on top of CARRY) is given for its pair: rings of H rows indexed by ABSOLUTE macro-step.
// The live cell of lane l at absolute column J belongs to macro-step J + l; its branch words (packed as SpotRecord's) go to
// dirs[(((J + l) mod H) * WPL + w) * 64 + l], so the 64 lanes of a store write 64 consecutive words, and lane l's column J overwrites
// lane l's column J - H and nothing else: every lane holds exactly its last H columns, whatever the chunking.  Row n's lane stores
// T[n][J] and S[n][J] (absolute) at curve_v / curve_s[(J + lane_n) mod H].  The row is one wrapping counter, the same for every lane.
// J + l < 2^32: kSpotMaxStream.  A waiting or drained lane and a lane without live rows store nothing.
struct SpotRing {
    uint32_t *dirs;
    float *curve_v;
    uint32_t *curve_s;
    uint32_t rows;          // H >= 1
};

// Where a sweep that is not REC leaves its results: row n's curves at P.curve_off (both null: best only) and the best at P.out.
struct SpotOut {
    float *d_cost;
    uint32_t *d_start;
    apd_spot_best *d_best;
};

template <int RT, int D, bool REC, bool CARRY = false, bool RING = false>
__device__ __forceinline__ void spot_sweep(const SpotSource src, const SpotOut out, const SpotPair P, const SpotRecord rec,
                                           const SpotCarry carry = SpotCarry{}, const SpotRing ring = SpotRing{})
{
    static_assert(RT == 0 || D > 0, "rows in registers need the frame dimension at compile time");
    static_assert(!(REC && CARRY), "a carried table has no column 1 to record from");
    static_assert(!RING || CARRY, "the rings belong to a carried table: absolute columns, curves and best as CARRY keeps them");
    constexpr bool OPS = REC || RING;                                       // the branch of a cell is wanted
    extern __shared__ __attribute__((aligned(16))) float spot_column[];   // RT == 0: [r][lane] values, then [r][lane] starts
    constexpr int DN = D > 0 ? ((D + 4) & ~3) : 4;                          // floats of a resident frame
    const int lane = threadIdx.x;
    uint32_t ox = src.d_seq_off[P.px], oy = 0u;
    if constexpr (!CARRY) oy = src.d_seq_off[P.py];
    const int n = (int)(src.d_seq_off[P.px + 1] - ox) - 2;                    // <= kSpotMaxQuery
    uint32_t m;
    if constexpr (CARRY) m = carry.m;
    else m = REC ? rec.max_end : src.d_seq_off[P.py + 1] - oy - 2;            // REC: column j depends on columns <= j only
    const float *X = src.d_frames + (uint64_t)ox * src.dpad;
    const float *Y = CARRY ? carry.y : src.d_frames + (uint64_t)oy * src.dpad;
    const float ins = src.ins, del = src.del, mat = src.mat;
    const int R = RT > 0 ? RT : (n + 63) / 64;
    const int row0 = lane * R;                                              // 0-based first query row of the lane
    const int rows_live = min(max(n - row0, 0), R);
    const int lane_n = (n - 1) / R, r_n = (n - 1) - lane_n * R;             // where row n lives
    const bool curves = !REC && out.d_cost != nullptr;
    float *cost = curves ? out.d_cost + P.curve_off : nullptr;
    uint32_t *start = curves ? out.d_start + P.curve_off : nullptr;
    uint32_t *col_start = reinterpret_cast<uint32_t *>(spot_column) + (size_t)R * 64;

    float pv[RT > 0 ? RT : 1];                                              // the lane's previous column
    uint32_t ps[RT > 0 ? RT : 1];
    float xr[RT > 0 ? RT : 1][DN];                                          // the lane's query rows (RT > 0 and D > 0)
    if constexpr (RT > 0) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            pv[r] = CARRY ? carry.in_v[r * 64 + lane] : APD_INF;
            ps[r] = CARRY ? carry.in_s[r * 64 + lane] : 0u;
            spot_load_frame<DN>(xr[r], X + (uint64_t)min(row0 + r, n - 1) * src.dpad);
        }
    } else {
        for (int r = 0; r < R; ++r) {
            spot_column[r * 64 + lane] = CARRY ? carry.in_v[r * 64 + lane] : APD_INF;
            col_start[r * 64 + lane] = CARRY ? carry.in_s[r * 64 + lane] : 0u;
        }
    }

    // REC: the lane's cursor into the intervals (its columns only ascend), and the cursor of row n's lane into the ends
    [[maybe_unused]] const uint64_t row_words = (uint64_t)((R + 15) >> 4) * 64;
    [[maybe_unused]] uint32_t iv_k = 0, iv_a = 1u, iv_b = 0u, end_k = 0, end_next = 0;
    [[maybe_unused]] uint64_t iv_off = 0;
    if constexpr (REC) {
        if (rec.n_iv) { const SpotInterval v = rec.iv[0]; iv_a = v.a; iv_b = v.b; iv_off = v.off; }
        if (rec.n_ends) end_next = rec.ends[0];
    }
    // RING: the ring row of the current macro-step; macro-step tau of this launch is absolute macro-step base + 1 + tau for every lane
    [[maybe_unused]] uint32_t ring_row = 0;
    if constexpr (RING) ring_row = (carry.base + 1u) % ring.rows;

    const int dp4 = (int)src.dpad / 4, dim = (int)src.dim;
    float y_even[DN], y_odd[DN];                                            // column j's frame and the next macro-step's, taking turns (D > 0)
    uint32_t jm1 = 0u - (uint32_t)lane;                                     // j - 1; wraps above m while the lane waits for column 1
    if constexpr (D > 0) spot_load_frame<DN>(y_even, Y + (uint64_t)min(jm1, m - 1) * src.dpad);
    float in_prev = lane == 0 ? 0.0f : APD_INF;                             // T[row0][j-1]: row 0 reads 0, column 0 below it +INF
    uint32_t in_prev_s = 0u;
    float last = APD_INF;
    uint32_t last_s = 0u;
    [[maybe_unused]] uint32_t best_end = 0u, best_start = 0u;
    [[maybe_unused]] float best_cost = APD_INF, best_score = APD_INF;
    if constexpr (CARRY) {
        // what the lane above takes as its MATCH predecessor at its first live step: this lane's last row of the carried column.
        // A waiting lane hands it on unchanged (below); lane 0 never waits, so it starts out with it.
        if constexpr (RT > 0) { last = pv[RT - 1]; last_s = ps[RT - 1]; }
        else { last = spot_column[(R - 1) * 64 + lane]; last_s = col_start[(R - 1) * 64 + lane]; }
        const apd_spot_best b = out.d_best[P.out];
        best_end = b.end; best_start = b.start; best_cost = b.cost; best_score = b.score;
    }
    const uint64_t total = (uint64_t)m + (uint64_t)lane_n;
    // one macro-step: yv holds column j's frame, yn receives the next column's while this one is computed
    auto macro_step = [&](const float (&yv)[DN], float (&yn)[DN]) {
        const uint32_t j = jm1 + 1u;
        const bool column_live = jm1 < m;
        // CARRY: the absolute column.  Outside its columns 1 .. m a lane keeps its column instead of the +INF of a dead cell: while it
        // waits for column 1 (jm1 = -lane .. -1 has wrapped) that is the carried column, once it has drained it is column m, which
        // goes to the state behind the loop.  No live cell reads a drained lane: the lane above takes its INSERT and MATCH
        // predecessors from this lane's live steps only.
        uint32_t ja = j;
        if constexpr (CARRY) ja = carry.base + j;
        if constexpr (D > 0) spot_load_frame<DN>(yn, Y + (uint64_t)min(jm1 + 1u, m - 1) * src.dpad);
        const float4 *yb = reinterpret_cast<const float4 *>(Y + (uint64_t)min(jm1, m - 1) * src.dpad);
        // REC: where this column's branch words go, if it lies in an interval
        [[maybe_unused]] uint32_t *rec_words = nullptr;
        [[maybe_unused]] uint32_t word = 0;
        if constexpr (REC) {
            if (column_live) {
                while (iv_k < rec.n_iv && j > iv_b) {
                    if (++iv_k < rec.n_iv) { const SpotInterval v = rec.iv[iv_k]; iv_a = v.a; iv_b = v.b; iv_off = v.off; }
                }
                if ((rows_live > 0) & (j >= iv_a) & (j <= iv_b)) rec_words = rec.dirs + iv_off + ((uint64_t)(j - iv_a) + lane) * row_words + lane;
            }
        }
        if constexpr (RING) {
            if (column_live & (rows_live > 0)) rec_words = ring.dirs + (uint64_t)ring_row * row_words + lane;
        }
        // T[row0][j] from the lower lane (lane 0: row 0 of the table, value 0, start j)
        float up = from_lower_lane(last, 0.0f);
        uint32_t up_s = from_lower_lane_u32(last_s, 0u);
        up_s = lane == 0 ? ja : up_s;
        const float in_cur = up;
        const uint32_t in_cur_s = up_s;
        float diag = in_prev;
        uint32_t diag_s = lane == 0 ? ja : in_prev_s;
        float cap_v = APD_INF;
        uint32_t cap_s = 0u;
        if constexpr (RT > 0) {
            float d[RT];
            {
                bool in_domain = true;
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    d[r] = spot_sq_distance<D, DN>(xr[r], yv);
                    in_domain &= (d[r] >= 0x1p-96f) & (d[r] < APD_INF);
                }
                if (__builtin_expect(__ballot(!in_domain) != 0ull, 0)) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) d[r] = __builtin_sqrtf(d[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < RT; ++r) d[r] = sqrt_rn_finite(d[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const float left = pv[r];
                const uint32_t left_s = ps[r];
                const SpotNode node = spot_select<OPS>(left, left_s, up, up_s, diag, diag_s, d[r], del, ins, mat);
                const bool live = column_live & (r < rows_live);
                float v = live ? node.value : APD_INF;
                uint32_t s = live ? node.start : 0u;
                if constexpr (CARRY) { v = column_live ? v : left; s = column_live ? s : left_s; }
                diag = left; diag_s = left_s;                               // (i, j-1) is the next row's MATCH predecessor
                pv[r] = v; ps[r] = s;
                up = v; up_s = s;
                if (r == r_n) { cap_v = v; cap_s = s; }
                if constexpr (OPS) word |= node.op << (2 * r);
            }
            if constexpr (OPS) if (rec_words) rec_words[0] = word;
        } else {
            for (int r = 0; r < R; ++r) {
                const float *xrow = X + (uint64_t)min(row0 + r, n - 1) * src.dpad;
                float dist;
                if constexpr (D > 0) {
                    float xf[DN];
                    spot_load_frame<DN>(xf, xrow);
                    dist = __builtin_sqrtf(spot_sq_distance<D, DN>(xf, yv));
                } else {
                    dist = __builtin_sqrtf(spot_sq_distance_any(reinterpret_cast<const float4 *>(xrow), yb, dp4, dim));
                }
                const float left = spot_column[r * 64 + lane];
                const uint32_t left_s = col_start[r * 64 + lane];
                const SpotNode node = spot_select<OPS>(left, left_s, up, up_s, diag, diag_s, dist, del, ins, mat);
                const bool live = column_live & (r < rows_live);
                float v = live ? node.value : APD_INF;
                uint32_t s = live ? node.start : 0u;
                if constexpr (CARRY) { v = column_live ? v : left; s = column_live ? s : left_s; }
                diag = left; diag_s = left_s;
                spot_column[r * 64 + lane] = v;
                col_start[r * 64 + lane] = s;
                up = v; up_s = s;
                if (r == r_n) { cap_v = v; cap_s = s; }
                if constexpr (OPS) {
                    word |= node.op << (2 * (r & 15));
                    if (((r & 15) == 15) | (r == R - 1)) {
                        if (rec_words) rec_words[(r >> 4) * 64] = word;
                        word = 0;
                    }
                }
            }
        }
        in_prev = in_cur; in_prev_s = in_cur_s;
        last = up; last_s = up_s;
        if ((lane == lane_n) & column_live) {                               // row n of column j
            if constexpr (REC) {
                if (end_k < rec.n_ends && j == end_next) {
                    rec.end_cost[end_k] = cap_v;
                    rec.end_start[end_k] = cap_s;
                    if (++end_k < rec.n_ends) end_next = rec.ends[end_k];
                }
            } else {
                if (curves) { cost[jm1] = cap_v; start[jm1] = cap_s; }
                if constexpr (RING) { ring.curve_v[ring_row] = cap_v; ring.curve_s[ring_row] = cap_s; }
                const float score = spot_score(cap_v, ja, cap_s, (uint32_t)n);
                if (score < best_score) { best_end = ja; best_start = cap_s; best_cost = cap_v; best_score = score; }
            }
        }
        ++jm1;
        if constexpr (RING) { if (++ring_row == ring.rows) ring_row = 0u; }
    };
    // two macro-steps per turn, the frame buffers swapping roles; a step beyond `total` computes nothing that is live
    for (uint64_t tau = 0; tau < total; tau += 2) {
        macro_step(y_even, y_odd);
        macro_step(y_odd, y_even);
    }
    if constexpr (CARRY) {
        // every lane with a live row holds column m of its rows now (dead rows: +INF / 0): the state the next chunk enters with.
        // Lanes without a live row never hold anything but the +INF / 0 the reset wrote.
        if (rows_live > 0) {
            if constexpr (RT > 0) {
#pragma unroll
                for (int r = 0; r < RT; ++r) { carry.out_v[r * 64 + lane] = pv[r]; carry.out_s[r * 64 + lane] = ps[r]; }
            } else {
                for (int r = 0; r < R; ++r) {
                    carry.out_v[r * 64 + lane] = spot_column[r * 64 + lane];
                    carry.out_s[r * 64 + lane] = col_start[r * 64 + lane];
                }
            }
        }
    }
    if constexpr (!REC) {
        if (lane == lane_n) {
            apd_spot_best b;
            b.end = best_end; b.start = best_start; b.cost = best_cost; b.score = best_score;
            out.d_best[P.out] = b;
        }
    }
}

// ---- the one kernel and the one launcher of the four sweep kinds.  A kind is a type with
//   Launch:         its launch struct, the kernel's only argument;
//   word:           its name on the APD_DEBUG_PLAN line (spot_debug_line);
//   pair<RT, D>(L): what the wavefront of pair blockIdx.x does -- spot_sweep with the kind's REC / CARRY / RING.
// SpotSweep (dtw_spot.hip), SpotRecordSweep (dtw_spot_path.hip), SpotStreamSweep (dtw_spot_stream.hip) and SpotStreamRecordSweep
// (dtw_spot_stream_rec.hip) are the kinds; each unit instantiates its own kind's kernels through its launch_*.
template <class Kind, int RT, int D>
__global__ __launch_bounds__(64) void spot_kernel(const typename Kind::Launch L)
{
    Kind::template pair<RT, D>(L);
}

template <class Kind, int RT, int D>
hipError_t spot_launch_as(const typename Kind::Launch &L, uint32_t n_pairs, uint32_t r_max, hipStream_t stream)
{
    const size_t lds_bytes = RT > 0 ? 0 : spot_lds_bytes(r_max);
    spot_debug_line(Kind::word, RT, D, n_pairs, r_max, lds_bytes);
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spot_kernel<Kind, RT, D>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((spot_kernel<Kind, RT, D>), dim3(n_pairs), dim3(64), lds_bytes, stream, L);
    return hipGetLastError();
}

// class C of kSpotClasses is kernel <C, D>; an rt that names no class runs as class 0
template <class Kind, int D, size_t... C>
hipError_t spot_launch_class(const typename Kind::Launch &L, uint32_t n_pairs, uint32_t rt, uint32_t r_max, hipStream_t stream,
                             std::index_sequence<C...>)
{
    hipError_t e = hipSuccess;
    const bool named = ((rt == C ? (e = spot_launch_as<Kind, (int)C, D>(L, n_pairs, r_max, stream), true) : false) || ...);
    return named ? e : spot_launch_as<Kind, 0, D>(L, n_pairs, r_max, stream);
}

// The n_pairs pairs of L all belong to one class (spot_row_class): rt = 1 .. kSpotRegisterRows rows per lane in registers, or 0 with
// at most r_max rows in LDS.  dim: the resident dimension of L's source.
template <class Kind>
hipError_t spot_launch(const typename Kind::Launch &L, uint32_t n_pairs, uint32_t dim, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    if (n_pairs == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    const bool typed = with_kernel_dim(dim, [&](auto d) {
        e = spot_launch_class<Kind, decltype(d)::value>(L, n_pairs, rt, r_max, stream, std::make_index_sequence<kSpotClasses>{});
    });
    if (!typed) e = spot_launch_as<Kind, 0, 0>(L, n_pairs, r_max, stream);   // any other dimension: frames re-read per cell, column in LDS
    return e;
}

}  // namespace apd
