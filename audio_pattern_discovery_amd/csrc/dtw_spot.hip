// Subsequence alignment ("spotting", gfx950): apd_spot.  A query x of n frames against every window of a stream y of m frames in ONE
// DP: the recurrence of alignments.rs:153-159 with a free start (row 0 of the table is 0 in every column, column 0 is +INF below
// it), no band, and the column in which each cell's alignment left row 0 carried along with the value.  The results are the last
// row's value and start per stream column (include/apd.h, "subsequence alignment").
//
// The reference has no spotting, so nothing of it is mirrored beyond the recurrence and the arithmetic -- in particular NOT its habit
// of reading the score one row and one column short, at (n-1, m-1) (alignments.rs:120): the curves are row n's, or a one-frame query
// would have no row at all.
//
// One wavefront per (query, stream) pair of the call's list.  Rows go on lanes, the stream flows through: lane l owns the R =
// ceil(n / 64) query rows l R + 1 .. l R + R, macro-step tau gives it stream column j = tau - l + 1, and m + (lane of row n) macro-
// steps cover the pair.  What a cell needs:
//   DELETE  (i, j-1): the lane's own previous column -- R values and R starts, in registers for R <= 4 (RT = R), else in dynamic LDS
//                     laid out [r][lane] (RT = 0; conflict-free, as the path sweep keeps its row);
//   INSERT  (i-1, j): the row above in the same macro-step; for the lane's first row the lower lane's last row of column j, which
//                     that lane computed one macro-step earlier: one from_lower_lane each for value and start;
//   MATCH (i-1, j-1): the row above one column earlier; for the first row what arrived from the lower lane one macro-step earlier.
// Lane 0 has no lower lane: it reads row 0, value 0 and start j.  The lane that owns row n stores the curves (when the caller asked
// for them) and keeps the running best -- the scan over j is serial there already, no atomics, no reduction.
// Cells of columns outside 1 .. m and of rows beyond n hold +INF (start 0) and reach no output.
//
// Arithmetic: numerics.rs:114-120 / alignments.rs:153-159 operation for operation, always (the context's distance mode is not
// read).  D: the resident frame dimension as a compile-time constant (frames in registers), 0 = any dimension (frames re-read per
// cell, as dtw_path.hip does).  The register variants take the square roots of a macro-step with sqrt_rn_finite when every squared
// distance of the wavefront is inside its domain, and with the compiler's general sequence otherwise (identical frames, infinities,
// NaN): the bits are the same either way (dtw_common.h).
#include "dtw_common.h"

namespace apd {

// the select of dtw_path.hip's select_node_branch, carrying the start column of the chosen predecessor instead of the branch
struct SpotNode { float value; uint32_t start; };
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
    return {base + weighted, s};
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

template <int RT, int D>
__global__ __launch_bounds__(64) void dtw_spot(const SpotLaunch L)
{
    static_assert(RT == 0 || D > 0, "rows in registers need the frame dimension at compile time");
    extern __shared__ __attribute__((aligned(16))) float spot_column[];   // RT == 0: [r][lane] values, then [r][lane] starts
    constexpr int DN = D > 0 ? ((D + 4) & ~3) : 4;                          // floats of a resident frame
    const int lane = threadIdx.x;
    const SpotPair P = L.d_pairs[blockIdx.x];
    const uint32_t ox = L.d_seq_off[P.px], oy = L.d_seq_off[P.py];
    const int n = (int)(L.d_seq_off[P.px + 1] - ox) - 2;                    // <= kSpotMaxQuery
    const uint32_t m = L.d_seq_off[P.py + 1] - oy - 2;
    const float *X = L.d_frames + (uint64_t)ox * L.dpad;
    const float *Y = L.d_frames + (uint64_t)oy * L.dpad;
    const float ins = L.ins, del = L.del, mat = L.mat;
    const int R = RT > 0 ? RT : (n + 63) / 64;
    const int row0 = lane * R;                                              // 0-based first query row of the lane
    const int rows_live = min(max(n - row0, 0), R);
    const int lane_n = (n - 1) / R, r_n = (n - 1) - lane_n * R;             // where row n lives
    const bool curves = L.d_cost != nullptr;
    float *cost = curves ? L.d_cost + P.curve_off : nullptr;
    uint32_t *start = curves ? L.d_start + P.curve_off : nullptr;
    uint32_t *col_start = reinterpret_cast<uint32_t *>(spot_column) + (size_t)R * 64;

    float pv[RT > 0 ? RT : 1];                                              // the lane's previous column
    uint32_t ps[RT > 0 ? RT : 1];
    float xr[RT > 0 ? RT : 1][DN];                                          // the lane's query rows (RT > 0 and D > 0)
    if constexpr (RT > 0) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            pv[r] = APD_INF;
            ps[r] = 0u;
            spot_load_frame<DN>(xr[r], X + (uint64_t)min(row0 + r, n - 1) * L.dpad);
        }
    } else {
        for (int r = 0; r < R; ++r) {
            spot_column[r * 64 + lane] = APD_INF;
            col_start[r * 64 + lane] = 0u;
        }
    }

    const int dp4 = (int)L.dpad / 4, dim = (int)L.dim;
    float y_even[DN], y_odd[DN];                                            // column j's frame and the next macro-step's, taking turns (D > 0)
    uint32_t jm1 = 0u - (uint32_t)lane;                                     // j - 1; wraps above m while the lane waits for column 1
    if constexpr (D > 0) spot_load_frame<DN>(y_even, Y + (uint64_t)min(jm1, m - 1) * L.dpad);
    float in_prev = lane == 0 ? 0.0f : APD_INF;                             // T[row0][j-1]: row 0 reads 0, column 0 below it +INF
    uint32_t in_prev_s = 0u;
    float last = APD_INF;
    uint32_t last_s = 0u;
    uint32_t best_end = 0u, best_start = 0u;
    float best_cost = APD_INF, best_score = APD_INF;
    const uint64_t total = (uint64_t)m + (uint64_t)lane_n;
    // one macro-step: yv holds column j's frame, yn receives the next column's while this one is computed
    auto macro_step = [&](const float (&yv)[DN], float (&yn)[DN]) {
        const uint32_t j = jm1 + 1u;
        const bool column_live = jm1 < m;
        if constexpr (D > 0) spot_load_frame<DN>(yn, Y + (uint64_t)min(jm1 + 1u, m - 1) * L.dpad);
        const float4 *yb = reinterpret_cast<const float4 *>(Y + (uint64_t)min(jm1, m - 1) * L.dpad);
        // T[row0][j] from the lower lane (lane 0: row 0 of the table, value 0, start j)
        float up = from_lower_lane(last, 0.0f);
        uint32_t up_s = from_lower_lane_u32(last_s, 0u);
        up_s = lane == 0 ? j : up_s;
        const float in_cur = up;
        const uint32_t in_cur_s = up_s;
        float diag = in_prev;
        uint32_t diag_s = lane == 0 ? j : in_prev_s;
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
                const SpotNode node = spot_select(left, left_s, up, up_s, diag, diag_s, d[r], del, ins, mat);
                const bool live = column_live & (r < rows_live);
                const float v = live ? node.value : APD_INF;
                const uint32_t s = live ? node.start : 0u;
                diag = left; diag_s = left_s;                               // (i, j-1) is the next row's MATCH predecessor
                pv[r] = v; ps[r] = s;
                up = v; up_s = s;
                if (r == r_n) { cap_v = v; cap_s = s; }
            }
        } else {
            for (int r = 0; r < R; ++r) {
                const float *xrow = X + (uint64_t)min(row0 + r, n - 1) * L.dpad;
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
                const SpotNode node = spot_select(left, left_s, up, up_s, diag, diag_s, dist, del, ins, mat);
                const bool live = column_live & (r < rows_live);
                const float v = live ? node.value : APD_INF;
                const uint32_t s = live ? node.start : 0u;
                diag = left; diag_s = left_s;
                spot_column[r * 64 + lane] = v;
                col_start[r * 64 + lane] = s;
                up = v; up_s = s;
                if (r == r_n) { cap_v = v; cap_s = s; }
            }
        }
        in_prev = in_cur; in_prev_s = in_cur_s;
        last = up; last_s = up_s;
        if ((lane == lane_n) & column_live) {                               // row n of column j
            if (curves) { cost[jm1] = cap_v; start[jm1] = cap_s; }
            const uint32_t window = j - cap_s + 1u;                         // frames of y the alignment covers
            const float score = cap_v / (float)((uint32_t)n + window);      // one f32 division (alignments.rs:121 with the window for m); < 2^32: kSpotMaxStream
            if (score < best_score) { best_end = j; best_start = cap_s; best_cost = cap_v; best_score = score; }
        }
        ++jm1;
    };
    // two macro-steps per turn, the frame buffers swapping roles; a step beyond `total` computes nothing that is live
    for (uint64_t tau = 0; tau < total; tau += 2) {
        macro_step(y_even, y_odd);
        macro_step(y_odd, y_even);
    }
    if (lane == lane_n) {
        apd_spot_best b;
        b.end = best_end; b.start = best_start; b.cost = best_cost; b.score = best_score;
        L.d_best[P.out] = b;
    }
}

size_t spot_lds_bytes(uint32_t rows_per_lane) { return (size_t)rows_per_lane * 64 * (sizeof(float) + sizeof(uint32_t)); }

namespace {

template <int RT, int D>
hipError_t launch_spot_as(const SpotLaunch &L, uint32_t r_max, hipStream_t stream)
{
    const size_t lds_bytes = RT > 0 ? 0 : spot_lds_bytes(r_max);
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_spot<RT, D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((dtw_spot<RT, D>), dim3(L.n_pairs), dim3(64), lds_bytes, stream, L);
    return hipGetLastError();
}

template <int D>
hipError_t launch_spot_rows(const SpotLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    switch (rt) {
        case 1: return launch_spot_as<1, D>(L, r_max, stream);
        case 2: return launch_spot_as<2, D>(L, r_max, stream);
        case 3: return launch_spot_as<3, D>(L, r_max, stream);
        case 4: return launch_spot_as<4, D>(L, r_max, stream);
        default: return launch_spot_as<0, D>(L, r_max, stream);
    }
}

}  // namespace

// The pairs of L all belong to one class (spot_row_class): rt = 1 .. 4 rows per lane in registers, or 0 with at most r_max rows in LDS.
hipError_t launch_spot(const SpotLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    if (L.n_pairs == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    const bool typed = with_kernel_dim(L.dim, [&](auto d) { e = launch_spot_rows<decltype(d)::value>(L, rt, r_max, stream); });
    if (!typed) e = launch_spot_as<0, 0>(L, r_max, stream);              // any other dimension: frames re-read per cell, column in LDS
    return e;
}

}  // namespace apd
