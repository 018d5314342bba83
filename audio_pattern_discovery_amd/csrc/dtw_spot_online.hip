// Online spot detection (gfx950): the hold-off machine of an armed streaming session (include/apd.h, "streaming spotting, online
// detection").  A push's sweeps (the kinds SpotStreamSweep / SpotStreamRecordSweep) leave the chunk's curves in
// the session's buffer; spot_online_scan, launched behind them on the same stream, turns them into hits without the curves ever
// leaving the device.
//
//   spot_online_scan   one workgroup of 16 wavefronts per group.  It walks the chunk in tiles of 16 x 64 columns.  Wavefront w takes
//                      the tile's w-th block of 64 columns, lanes as columns: the score (spot_score, the sweep's own: one IEEE
//                      division), the strict threshold test, and per channel the smallest (spot_score_key(score), pair) key over the
//                      channel's pairs -- a lane loop over the pairs, every load coalesced (a pair's chunk entries are contiguous,
//                      a channel's pairs adjacent).  A column belongs to ONE lane, which sees all of the group's pairs, so there
//                      is no order of partial results for the outcome to depend on.  The block's candidates and their ballot go
//                      to LDS; behind a barrier wavefront 0 walks the 16 ballots in ascending order with a wave-uniform loop over
//                      their set bits and applies the machine's steps with the state in registers.  The timer is looked at where
//                      a candidate stands and at the chunk's last column: between two candidates nothing else can change the
//                      state, so this emits what the per-column wording emits.
//   spot_online_touch  one lane per group: flush (emit the pending window) or reset (drop it, move the floor).
//
// A hit goes to the session's queue through one atomic on its counter; the order of the queue therefore depends on scheduling, and
// nothing reads it: a record carries (pair, rank), and the drain orders by (group, rank) on the host.  The host has sized the queue
// for the most a launch can emit (chunk columns + 1 per group; one per group for a flush) before the launch.
#include "apd_internal.h"

namespace apd {

namespace {

// every lane holds the same state; lane 0 writes the record
__device__ __forceinline__ void online_emit(const SpotOnlineLaunch &L, SpotOnlineState &st, bool writer)
{
    if (writer) {
        const unsigned long long at = atomicAdd(L.d_count, 1ull);
        if (at < L.queue_cap) {                                               // always true: the host sized the queue for the bound
            apd_spot_hit h;
            h.pair = st.pair; h.end = st.end; h.start = st.start; h.cost = st.cost; h.score = st.score; h.rank = st.rank;
            L.d_queue[at] = h;
        }
    }
    st.floor = st.end;
    st.end = 0u;
    ++st.rank;
}

constexpr uint32_t kScanWaves = 16;                                          // wavefronts of a scan workgroup at most: a tile is 1024 columns

// grid: the session's groups; 64 * waves threads, waves <= kScanWaves, as many as the longest chunk has blocks of 64 columns
__global__ __launch_bounds__(64 * kScanWaves) void spot_online_scan(const SpotOnlineLaunch L)
{
    __shared__ uint32_t s_pair[64 * kScanWaves], s_start[64 * kScanWaves];
    __shared__ float s_cost[64 * kScanWaves], s_score[64 * kScanWaves];
    __shared__ unsigned long long s_vote[kScanWaves];
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockDim.x;
    const uint32_t members = L.per_stream ? L.n_queries : 1u;
    const uint32_t p0 = L.per_stream ? g * L.n_queries : g;                   // the group's first pair
    const uint32_t k = p0 / L.n_queries;
    const uint32_t first = L.d_push[k], m = L.d_push[k + 1] - first;
    if (m == 0) return;                                                       // nothing pushed on this channel: no column passes (the whole workgroup leaves)
    const uint32_t base = L.d_push[L.n_channels + 1 + k];                     // chunk entry i is absolute column base + 1 + i
    // pair p0 + q owns entries [off0 + q m, off0 + (q + 1) m) (spot_stream_pair, dtw_spot_stream.h)
    const uint64_t off0 = (uint64_t)L.n_queries * first + (uint64_t)(p0 - k * L.n_queries) * m;
    SpotOnlineState st = L.d_state[g];                                        // wavefront 0's copy is the one that lives
    for (uint32_t t0 = 0; t0 < m; t0 += tile) {                               // the trip count is the workgroup's: every thread reaches the barriers
        const uint32_t i = t0 + tid;
        bool cand = false;
        if (i < m) {
            const uint32_t end = base + 1u + i;
            unsigned long long c_key = ~0ull;
            uint32_t c_start = 0;
            float c_cost = 0.0f, c_score = 0.0f;
#pragma unroll 8
            for (uint32_t q = 0; q < members; ++q) {
                const SpotOnlinePair Q = L.d_pairs[p0 + q];
                const uint64_t e = off0 + (uint64_t)q * m + i;
                const float c = L.d_cost[e];
                const uint32_t s = L.d_start[e];
                const float score = spot_score(c, end, s, Q.n);
                if (s != 0u && score < Q.threshold) {                         // strict; a NaN on either side compares false
                    const unsigned long long key = ((unsigned long long)spot_score_key(score) << 32) | (p0 + q);
                    if (key < c_key) { c_key = key; cand = true; c_start = s; c_cost = c; c_score = score; }
                }
            }
            if (cand) { s_pair[tid] = (uint32_t)c_key; s_start[tid] = c_start; s_cost[tid] = c_cost; s_score[tid] = c_score; }
        }
        const unsigned long long mine = __ballot(cand);
        if (lane == 0) s_vote[wave] = mine;
        __syncthreads();
        if (wave == 0) {
            const uint32_t blocks = tile >> 6;
            for (uint32_t w = 0; w < blocks; ++w) {
                unsigned long long vote = s_vote[w];
                while (vote) {                                                // wave-uniform: every lane walks the same bits
                    const uint32_t at = w * 64u + (uint32_t)(__ffsll((long long)vote) - 1);
                    vote &= vote - 1ull;
                    const uint32_t j = base + 1u + t0 + at;
                    const uint32_t pair = s_pair[at], start = s_start[at];
                    const float cost = s_cost[at], score = s_score[at];
                    if (st.end != 0u && j - st.end > L.holdoff) online_emit(L, st, lane == 0);   // 1: the timer (never with 0xFFFFFFFF)
                    if (start <= st.floor) continue;                          // 3: shares a column with an emitted hit
                    bool take = true;
                    if (st.end != 0u) {
                        if (start <= st.end) take = score < st.score;         // 5: overlap; an equal score keeps the earlier end
                        else online_emit(L, st, lane == 0);                   // 6: disjoint
                    }
                    if (take) { st.pair = pair; st.end = j; st.start = start; st.cost = cost; st.score = score; }   // 4, 5, 6
                }
            }
        }
        __syncthreads();                                                      // the next tile overwrites the candidates
    }
    if (wave != 0) return;
    if (st.end != 0u && (base + m) - st.end > L.holdoff) online_emit(L, st, lane == 0);   // the timer at the chunk's last column
    if (lane == 0) L.d_state[g] = st;
}

// grid: 64 groups per workgroup
__global__ __launch_bounds__(64) void spot_online_touch(const SpotOnlineLaunch L, uint32_t channel, bool flush, uint32_t first_column)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= L.n_groups) return;
    const uint32_t k = L.per_stream ? g : g / L.n_queries;
    if (channel != 0xFFFFFFFFu && k != channel) return;
    SpotOnlineState st = L.d_state[g];
    if (flush) {
        if (st.end == 0u) return;
        online_emit(L, st, true);
    } else {
        st.end = 0u;
        st.floor = first_column;
    }
    L.d_state[g] = st;
}

}  // namespace

hipError_t launch_spot_online_scan(const SpotOnlineLaunch &L, uint64_t m_max, hipStream_t stream)
{
    if (L.n_groups == 0 || m_max == 0) return hipSuccess;
    // one wavefront per 64 columns of the longest chunk, kScanWaves at most, and no more than fill the chip once (256 CUs x 32
    // wavefronts): with a thousand groups a wavefront each walks several tiles rather than wait for a second round of workgroups.
    // The hits do not depend on it: a column belongs to one lane whatever the tile's width.
    const uint64_t fill = std::max<uint64_t>(8192 / L.n_groups, 1);
    const uint32_t waves = (uint32_t)std::min<uint64_t>(std::min<uint64_t>((m_max + 63) / 64, kScanWaves), fill);
    hipLaunchKernelGGL(spot_online_scan, dim3(L.n_groups), dim3(64 * waves), 0, stream, L);
    return hipGetLastError();
}

hipError_t launch_spot_online_touch(const SpotOnlineLaunch &L, uint32_t channel, bool flush, uint32_t first_column, hipStream_t stream)
{
    if (L.n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(spot_online_touch, dim3((L.n_groups + 63u) / 64u), dim3(64), 0, stream, L, channel, flush, first_column);
    return hipGetLastError();
}

}  // namespace apd
