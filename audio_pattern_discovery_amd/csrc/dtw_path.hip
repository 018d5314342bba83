// Warping paths for selected ordered pairs (gfx950): apd_align_paths / apd_align_pair_path.
//
// The reference keeps the whole DP table (Alignment.sparse, alignments.rs:99-111,165-180); a caller who wants to know which
// frames were matched to which walks it back from the score cell (n-1, m-1).  Here the table never exists: two launches on the
// context's stream, one wavefront per ordered pair (x, y) each.
//
//   1. dtw_path_sweep: the literal recurrence of generic_pair (dtw_generic.hip) for the ONE ordered pair -- same lane mapping
//      (a lane owns C consecutive band offsets u = j - i + w, macro-step tau handles row i = tau - lane, neighbours through
//      from_lower_lane / from_upper_lane, the previous row in LDS), the arithmetic of numerics.rs:114-120 / alignments.rs:153-159
//      operation for operation whatever the context's distance mode -- whose select also returns WHICH branch won.  The branch of
//      every swept cell goes to HBM at 2 bits per cell: per (macro-step, lane) ceil(C / 16) words, word k holding cells 16k ..
//      16k + 15 of the lane, stored at dirs[(tau * WPL + k) * 64 + lane].  Indexed by macro-step, not by row: the 64 lanes of a
//      store are 64 consecutive words.  Rows 1 .. n-1 only, tau < n + 63: path_dir_words().
//   2. dtw_path_trace: walks back from (n-1, m-1) through those words -- a chain of at most n + m - 2 dependent reads, served from
//      LDS: tau never grows along the walk (MATCH: tau - 1; INSERT / DELETE: tau or tau - 1 as the offset crosses a lane), so a
//      window of kTraceStageWords / (64 WPL) macro-steps (8 KB) is staged at a time.  The walked cells land at the END of the pair's
//      slots (last cell at slot bound - 1).  The replay then goes forward, 64 steps at a time: every lane computes the literal
//      distance of its step and weights it by its branch's penalty (rounded), one chain adds them in path order.  A table value
//      IS predecessor + pen * d in exactly these operations, so the replayed costs are the table's bits.
#include "dtw_common.h"

namespace apd {

// numerics.rs:114-120 operation for operation, over the resident frame layout (slots >= dim hold the squared norm / padding)
__device__ __forceinline__ float path_distance(const float4 *xa, const float4 *yb, int dp4, int dim)
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
    return __builtin_sqrtf(acc);
}

// alignments.rs:153-159 with the branch it took: the sibling of select_node<false> (dtw_common.h).  An exact DELETE / INSERT tie,
// a NaN anywhere (compares false) and an all-INF node take MATCH.
struct NodeBranch { float value; uint32_t op; };
__device__ __forceinline__ NodeBranch select_node_branch(float del_v, float ins_v, float m_v, float d, float del_pen, float ins_pen,
                                                         float mat_pen)
{
    const bool pick_d = (del_v < m_v) & (del_v < ins_v);
    const bool pick_i = (ins_v < m_v) & (ins_v < del_v);
    float base = pick_i ? ins_v : m_v;
    base = pick_d ? del_v : base;
    float pen = pick_i ? ins_pen : mat_pen;
    pen = pick_d ? del_pen : pen;
    const float weighted = pen * d;                               // rounded on its own (alignments.rs:154-158)
    return {base + weighted, pick_d ? (uint32_t)APD_PATH_DELETE : pick_i ? (uint32_t)APD_PATH_INSERT : (uint32_t)APD_PATH_MATCH};
}

struct PathPairInfo { const float *X, *Y; int n, m; };
__device__ __forceinline__ PathPairInfo decode_path_pair(const PathLaunch &L, const PathPair &P)
{
    // x from a frames / offsets pair of its own when the launch has one (apd_barycenters), from the batch otherwise
    const float *x_frames = L.d_x_frames ? L.d_x_frames : L.d_frames;
    const uint32_t *x_off = L.d_x_seq_off ? L.d_x_seq_off : L.d_seq_off;
    const uint32_t ox = x_off[P.px], oy = L.d_seq_off[P.py];
    PathPairInfo r;
    r.n = (int)(x_off[P.px + 1] - ox) - 2;
    r.m = (int)(L.d_seq_off[P.py + 1] - oy) - 2;
    r.X = x_frames + (uint64_t)ox * L.dpad;
    r.Y = L.d_frames + (uint64_t)oy * L.dpad;
    return r;
}

__global__ __launch_bounds__(64) void dtw_path_sweep(const PathLaunch L)
{
    extern __shared__ float prev[];                            // [c][lane]: the previous row's cells of every lane
    const int lane = threadIdx.x;
    const PathPair P = L.d_pairs[blockIdx.x];
    const PathPairInfo I = decode_path_pair(L, P);
    const int n = I.n, m = I.m;
    if (n < 2 || m < 2) return;                                // nothing to sweep: the trace knows these paths without a table
    const int w = pair_w(L.band, n, m);
    const float ins = L.band.ins, del = L.band.del, mat = L.band.mat;
    const int two_w = 2 * w;
    const int C = (int)path_cells_per_lane((uint32_t)w);
    const int wpl = (C + 15) >> 4;
    uint32_t *dirs = L.d_dirs + P.dir_off;
    for (int c = 0; c < C; ++c) prev[c * 64 + lane] = APD_INF;
    const int dp4 = (int)L.dpad / 4, dim = (int)L.dim;
    const int u0 = C * lane;
    const int g_act = (two_w + 1 + C - 1) / C;
    const int total = (n - 1) + g_act;                         // <= n + 63 macro-steps: the rows path_dir_words() provides
    float last = APD_INF;
    for (int tau = 0; tau < total; ++tau) {
        const int i = tau - lane;
        const int jb = i + u0 - w;
        const float4 *xa = reinterpret_cast<const float4 *>(I.X + (uint64_t)(min(max(i, 1), n) - 1) * L.dpad);
        float left = from_lower_lane(last, APD_INF);
        float upr = APD_INF;
        float nxt = prev[lane];
        const bool row_swept = (i >= 1) & (i <= n - 1);
        uint32_t word = 0;
        for (int c = 0; c < C; ++c) {
            const int j = jb + c, u = u0 + c;
            const float4 *yb = reinterpret_cast<const float4 *>(I.Y + (uint64_t)(min(max(j, 1), m) - 1) * L.dpad);
            const float d = path_distance(xa, yb, dp4, dim);
            const float mv = nxt;
            const float up = (c < C - 1) ? prev[(c + 1) * 64 + lane] : upr;
            nxt = up;                                            // prev[c+1] is the next cell's MATCH predecessor
            const NodeBranch r = select_node_branch(left, up, mv, d, del, ins, mat);   // left = DELETE, up = INSERT
            const bool inside = (i >= 1) & (j >= 1) & (u <= two_w - 1);
            const float inv = ((i == 0) & (j == 0)) ? 0.0f : APD_INF;                   // D[0][0] = 0 (alignments.rs:109)
            const float v = inside ? r.value : inv;
            prev[c * 64 + lane] = v;
            left = v;
            if (c == 0) upr = from_upper_lane(v, APD_INF);
            word |= r.op << (2 * (c & 15));
            if (((c & 15) == 15) | (c == C - 1)) {
                if (row_swept) dirs[((uint64_t)tau * wpl + (c >> 4)) * 64 + lane] = word;
                word = 0;
            }
        }
        last = left;
    }
}

constexpr int kTraceStageWords = 2048;                          // 8 KB of direction words staged per window (18 wavefronts per CU)
static_assert(kTraceStageWords / 64 >= (int)((kPathMaxOffsets / 64 + 15) / 16), "a window holds at least one macro-step of the widest band");

__global__ __launch_bounds__(64) void dtw_path_trace(const PathLaunch L)
{
    __shared__ uint32_t stage[kTraceStageWords];
    __shared__ float s_wd[64];
    __shared__ uint32_t s_op[64];
    const int lane = threadIdx.x;
    const PathPair P = L.d_pairs[blockIdx.x];
    const PathPairInfo I = decode_path_pair(L, P);
    const int n = I.n, m = I.m;
    uint4 *out = reinterpret_cast<uint4 *>(L.d_steps + P.step_off);   // {i, j, bits of cost, op}
    const uint32_t bound = (uint32_t)(n + m - 1);
    const int w = pair_w(L.band, n, m);
    const int two_w = 2 * w;
    const int C = (int)path_cells_per_lane((uint32_t)w);
    const int wpl = (C + 15) >> 4;
    const int row_words = wpl * 64;
    const int window = kTraceStageWords / row_words;              // macro-steps per staged window, >= 1
    const uint32_t *dirs = L.d_dirs + P.dir_off;

    // ---- walk back (every lane runs the same walk; lane k % 64 keeps step k until the next flush)
    int i = n - 1, j = m - 1;
    bool go = (n == 1) == (m == 1);                             // exactly one length 1: the score cell is absent, the path empty
    int u = j - i + w, lu = u / C, c = u - lu * C;
    int lo = 0, hi = 0;                                         // staged macro-steps [lo, hi)
    uint32_t k = 0, mi = 0, mj = 0, mop = 0;
    while (go && k < bound) {
        uint32_t op;
        if (i == 0 && j == 0) {
            op = APD_PATH_START;
            go = false;
        } else {
            const int tau = i + lu;
            if (tau < lo || tau >= hi) {
                __syncthreads();
                hi = tau + 1;
                lo = max(hi - window, 0);
                const int words = (hi - lo) * row_words;
                const uint64_t base = (uint64_t)lo * row_words;
                for (int e = lane; e < words; e += 64) stage[e] = dirs[base + e];   // hi <= n + 63: inside the pair's words
                __syncthreads();
            }
            const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[((tau - lo) * wpl + (c >> 4)) * 64 + lu]);
            op = (word >> (2 * (c & 15))) & 3u;
        }
        if ((int)(k & 63u) == lane) { mi = (uint32_t)i; mj = (uint32_t)j; mop = op; }
        ++k;
        if ((k & 63u) == 0u) out[bound - 1 - (k - 64 + lane)] = make_uint4(mi, mj, 0u, mop);
        if (op == APD_PATH_START) break;
        if (op == APD_PATH_MATCH) { --i; --j; }
        else if (op == APD_PATH_INSERT) { --i; ++u; if (++c == C) { c = 0; ++lu; } }
        else { --j; --u; if (--c < 0) { c = C - 1; --lu; } }
        // an absent predecessor ends the walk: row 0 / column 0 other than the origin, or outside the band
        if (!(i == 0 && j == 0) && (i < 1 || j < 1 || u < 0 || u > two_w - 1)) go = false;
    }
    const uint32_t len = k;
    if ((k & 63u) != 0u && (uint32_t)lane < (k & 63u)) out[bound - 1 - ((k & ~63u) + lane)] = make_uint4(mi, mj, 0u, mop);
    __threadfence();                                            // the replay reads the slots other lanes have just written
    __syncthreads();

    // ---- replay forward: slot bound - len + s holds path step s; step s goes to slot s (never ahead of what is still unread)
    const int dp4 = (int)L.dpad / 4, dim = (int)L.dim;
    float carry = APD_INF;                                      // an absent predecessor reads as +INF
    for (uint32_t s = 0; s < len; s += 64) {
        const uint32_t idx = s + lane;
        const bool live = idx < len;
        uint4 st = make_uint4(0u, 0u, 0u, 0u);
        float wd = 0.0f;
        if (live) {
            st = out[bound - len + idx];
            if (st.w != APD_PATH_START) {
                const float4 *xa = reinterpret_cast<const float4 *>(I.X + (uint64_t)(st.x - 1) * L.dpad);
                const float4 *yb = reinterpret_cast<const float4 *>(I.Y + (uint64_t)(st.y - 1) * L.dpad);
                const float d = path_distance(xa, yb, dp4, dim);
                const float pen = st.w == APD_PATH_DELETE ? L.band.del : st.w == APD_PATH_INSERT ? L.band.ins : L.band.mat;
                wd = pen * d;                                   // rounded on its own, then added
            }
        }
        s_wd[lane] = wd;
        s_op[lane] = st.w;
        __syncthreads();
        const int count = (int)min(64u, len - s);
        float mine = 0.0f;
        for (int t = 0; t < count; ++t) {
            const float v = s_op[t] == APD_PATH_START ? 0.0f : carry + s_wd[t];   // sparse[(0,0)] = 0
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
        L.d_scores[blockIdx.x] = len ? carry / (float)(n + m) : APD_INF;          // alignments.rs:116-125
    }
}

size_t path_sweep_lds_bytes(uint32_t c_max) { return (size_t)c_max * 64 * sizeof(float); }

hipError_t launch_path_sweep(const PathLaunch &L, uint32_t c_max, hipStream_t stream)
{
    if (L.n_pairs == 0) return hipSuccess;
    const size_t lds_bytes = path_sweep_lds_bytes(c_max);
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_path_sweep), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dtw_path_sweep, dim3(L.n_pairs), dim3(64), lds_bytes, stream, L);
    return hipGetLastError();
}

hipError_t launch_path_trace(const PathLaunch &L, hipStream_t stream)
{
    if (L.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(dtw_path_trace, dim3(L.n_pairs), dim3(64), 0, stream, L);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// DTW barycenters (apd_barycenters).  An iteration is the sweep and the trace above with the barycenters as the x side, then these
// kernels over the steps the trace left on the device.  Every sum is a serial f32 chain in the contract's order (members ascending,
// steps in path order), owned by ONE lane from the first chunk of an iteration to the last: no atomics, and the chunking cannot
// show in the result.
// ------------------------------------------------------------------------------------------------

// the set that owns padded barycenter frame f: largest k with d_bary_off[k] <= f
__device__ __forceinline__ uint32_t bary_set_of(const BaryLaunch &L, uint32_t f)
{
    uint32_t lo = 0, hi = L.n_sets;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (L.d_bary_off[mid] <= f) lo = mid; else hi = mid; }
    return lo;
}

// One lane per float of d_bary: the frames of init[k] (all dpad slots), zeros in the two padding frames.
__global__ __launch_bounds__(256) void bary_init_kernel(const BaryLaunch L, const uint32_t *__restrict__ init_pos)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)L.n_padded * L.dpad) return;
    const uint32_t f = (uint32_t)(e / L.dpad), q = (uint32_t)(e - (uint64_t)f * L.dpad);
    const uint32_t k = bary_set_of(L, f);
    const uint32_t t = f - L.d_bary_off[k], T = L.d_bary_off[k + 1] - L.d_bary_off[k] - 2;
    L.d_bary[e] = t < T ? L.d_frames[(uint64_t)(L.d_seq_off[init_pos[k]] + t) * L.dpad + q] : 0.0f;
}

// One lane per set: which of the chunk's paths contribute (non-empty, first step START), and the chain of their scores.
__global__ __launch_bounds__(64) void bary_scores_kernel(const BaryLaunch L)
{
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= L.n_sets) return;
    const uint2 range = L.d_set_pairs[k];
    if (range.x >= range.y) return;
    float sum = L.d_score_sum[k];
    uint32_t used = L.d_used[k];
    for (uint32_t p = range.x; p < range.y; ++p) {
        const bool contributes = L.d_len[p] > 0 && L.d_steps[L.d_pairs[p].step_off].op == APD_PATH_START;
        L.d_contrib[p] = contributes ? 1u : 0u;
        if (contributes) { sum = sum + L.d_scores[p]; ++used; }
    }
    L.d_score_sum[k] = sum;
    L.d_used[k] = used;
}

// One lane per (set, table row t, frame slot): over the chunk's contributing paths of its set in order, the steps with i == t -- a
// contiguous range, the steps are monotone in i: a binary search finds its start -- add frame j - 1 of the member, serially, onto
// the running sum the earlier chunks left.  Slot 0's lane keeps the row's count.
__global__ __launch_bounds__(256) void bary_accumulate_kernel(const BaryLaunch L)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)L.n_padded * L.dpad) return;
    const uint32_t f = (uint32_t)(e / L.dpad), q = (uint32_t)(e - (uint64_t)f * L.dpad);
    const uint32_t k = bary_set_of(L, f);
    const uint32_t t = f - L.d_bary_off[k] + 1, T = L.d_bary_off[k + 1] - L.d_bary_off[k] - 2;
    const uint2 range = L.d_set_pairs[k];
    if (t > T || q >= L.dim || range.x >= range.y) return;
    float sum = L.d_sum[e];
    uint32_t cnt = L.d_cnt[f];
    for (uint32_t p = range.x; p < range.y; ++p) {
        if (!L.d_contrib[p]) continue;
        const PathPair P = L.d_pairs[p];
        const apd_path_step *steps = L.d_steps + P.step_off;
        const uint32_t len = L.d_len[p];
        const float *y = L.d_frames + (uint64_t)L.d_seq_off[P.py] * L.dpad + q;
        uint32_t lo = 0, hi = len;                                   // first step with i >= t
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (steps[mid].i < t) lo = mid + 1; else hi = mid; }
        for (; lo < len && steps[lo].i == t; ++lo) {                 // t >= 1: never the START step
            sum = sum + y[(uint64_t)(steps[lo].j - 1) * L.dpad];
            ++cnt;
        }
    }
    L.d_sum[e] = sum;
    if (q == 0) L.d_cnt[f] = cnt;
}

// One lane per (set, row, slot): the mean, or the old frame where nothing warped onto the row; lane (row 1, slot 0) of a set also
// writes the set's inertia and count.
__global__ __launch_bounds__(256) void bary_finalize_kernel(const BaryLaunch L, float *__restrict__ inertia, uint32_t *__restrict__ used_out)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)L.n_padded * L.dpad) return;
    const uint32_t f = (uint32_t)(e / L.dpad), q = (uint32_t)(e - (uint64_t)f * L.dpad);
    const uint32_t k = bary_set_of(L, f);
    const uint32_t t = f - L.d_bary_off[k] + 1, T = L.d_bary_off[k + 1] - L.d_bary_off[k] - 2;
    if (t == T + 1 && q == 0) {                                      // the first padding frame: one lane per set, empty sets too
        const uint32_t used = L.d_used[k];
        inertia[k] = used ? L.d_score_sum[k] / (float)used : APD_INF;
        used_out[k] = used;
    }
    if (t > T || q >= L.dim) return;
    const uint32_t cnt = L.d_cnt[f];
    if (cnt > 0) L.d_bary[e] = L.d_sum[e] / (float)cnt;
}

// One lane per (set, frame, component of the caller's dimension): the caller's packing, frame_off[k] = d_bary_off[k] - 2 k.
__global__ __launch_bounds__(256) void bary_pack_kernel(const BaryLaunch L, float *__restrict__ out)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)L.n_padded * L.dpad) return;
    const uint32_t f = (uint32_t)(e / L.dpad), q = (uint32_t)(e - (uint64_t)f * L.dpad);
    const uint32_t k = bary_set_of(L, f);
    const uint32_t t = f - L.d_bary_off[k], T = L.d_bary_off[k + 1] - L.d_bary_off[k] - 2;
    if (t >= T || q >= L.src_dim) return;
    out[(uint64_t)(f - 2 * k) * L.src_dim + q] = L.d_bary[e];
}

static uint32_t bary_blocks(const BaryLaunch &L) { return (uint32_t)(((uint64_t)L.n_padded * L.dpad + 255) / 256); }

hipError_t launch_bary_init(const BaryLaunch &L, const uint32_t *d_init_pos, hipStream_t stream)
{
    if (L.n_sets == 0) return hipSuccess;
    hipLaunchKernelGGL(bary_init_kernel, dim3(bary_blocks(L)), dim3(256), 0, stream, L, d_init_pos);
    return hipGetLastError();
}

hipError_t launch_bary_accumulate(const BaryLaunch &L, hipStream_t stream)
{
    if (L.n_sets == 0) return hipSuccess;
    hipLaunchKernelGGL(bary_scores_kernel, dim3((L.n_sets + 63) / 64), dim3(64), 0, stream, L);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(bary_accumulate_kernel, dim3(bary_blocks(L)), dim3(256), 0, stream, L);
    return hipGetLastError();
}

hipError_t launch_bary_finalize(const BaryLaunch &L, float *d_inertia, uint32_t *d_used_out, hipStream_t stream)
{
    if (L.n_sets == 0) return hipSuccess;
    hipLaunchKernelGGL(bary_finalize_kernel, dim3(bary_blocks(L)), dim3(256), 0, stream, L, d_inertia, d_used_out);
    return hipGetLastError();
}

hipError_t launch_bary_pack(const BaryLaunch &L, float *d_out, hipStream_t stream)
{
    if (L.n_sets == 0) return hipSuccess;
    hipLaunchKernelGGL(bary_pack_kernel, dim3(bary_blocks(L)), dim3(256), 0, stream, L, d_out);
    return hipGetLastError();
}

}  // namespace apd
