// Nearest neighbours: for every queried row (or column) of a distance matrix in HBM its k smallest entries, ascending by (value,
// index) -- apd_neighbors (include/apd.h), DESIGN.md section 4.22.
//
//   neighbors_select_kernel   one workgroup per query: the k-th key by four 8-bit digit passes over order_key (histogram in LDS,
//                             prefix and rank in registers, as vat_select_kernel), every entry below it plus the lowest-indexed
//                             ties at it into an LDS buffer of (key << 32 | j) words through ballot prefixes, a bitonic sort of that
//                             buffer, the store.  <true>: the row stays in LDS after the first pass, HBM is read once; <false>: the
//                             row is re-read per pass (rows beyond kResidentColumns).
//   neighbors_gather_kernel   the column form: queried columns into a [panel][rows] workspace, 64 x 64 tiles through LDS, both sides
//                             coalesced (adjacent columns without a query list); the select then runs on the workspace's rows.
//
// The answer is a function of the entries alone: every slot of the buffer is named by a prefix count over the row in index order and
// the sort's keys are unique, so neither the workgroup's size, nor the schedule, nor the panel cut can move a bit.  The histogram's
// LDS atomics only count.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "apd_internal.h"

using namespace apd;

namespace {

constexpr uint32_t kResidentColumns = 32768;      // rows of up to this many entries stay in LDS: 128 of the CU's 160 KiB
constexpr size_t kWorkspaceBytes = (size_t)256 << 20;   // the column form's panel
constexpr uint32_t kLongestRow = 0x7FFFFFF0u;     // 4 * (groups + U * blockDim) stays below 2^32 (sweep)
constexpr uint32_t kSweepAhead = 4;               // 16-byte loads a work-item has in flight (vat.hip: one per step waits on HBM)
constexpr uint32_t kHistWords = 272;              // 256 digits, [256] the NaNs; a multiple of 4 (what follows stays 16-byte aligned)
constexpr uint32_t kPadIndex = 0xFFFFFFFFu, kPadBits = 0x7FC00000u;

struct SelectParams {
    const float *src;          // row 0
    uint64_t stride;           // entries from a row to the next
    uint32_t n;                // entries of a row
    const uint32_t *queries;   // device: the whole call's query list; null: slot s is query s
    uint32_t q_first;          // output slot of workgroup 0
    uint32_t from_panel;       // 1: row b of src is the query of workgroup b (column form); 0: the query names its row
    uint32_t k, kcap;          // kcap: a power of two >= max(2, min(k, n)), the buffer's words
    uint32_t skip_self;
    uint32_t *index;           // [Q][k]
    uint32_t *distance;        // [Q][k] the matrix's bits
    uint32_t *count, *nans;    // [Q]; nans may be null
};

// Every entry e of x[0 .. n) once, in no particular order, by the whole workgroup: f(e, x[e], live) is called by all work-items of a
// wavefront together (f ballots), `live` false on the lanes without an entry.  Loads are 16 bytes wherever the address allows: `a` is
// x rounded down to 16 bytes and sh = x - a (0 .. 3), so group g = entries a[4g .. 4g + 3]; the groups cut by either end of the row
// load entry by entry.  keep (LDS, or null): a copy of the groups as loaded, entry e at keep[e + sh].
template <class F>
__device__ __forceinline__ void sweep(const float *a, uint32_t sh, uint32_t n, float *keep, F f)
{
    const uint32_t end = sh + n, groups = (end + 3) >> 2;
    for (uint32_t g0 = 0; g0 < groups; g0 += kSweepAhead * blockDim.x) {
        float4 v[kSweepAhead];
#pragma unroll
        for (uint32_t u = 0; u < kSweepAhead; ++u) {
            const uint32_t g = g0 + u * blockDim.x + threadIdx.x, i = 4 * g;
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (g < groups) {
                if (i >= sh && i + 4 <= end) {
                    v[u] = *reinterpret_cast<const float4 *>(a + i);
                } else {
                    if (i + 0 >= sh && i + 0 < end) v[u].x = a[i + 0];
                    if (i + 1 >= sh && i + 1 < end) v[u].y = a[i + 1];
                    if (i + 2 >= sh && i + 2 < end) v[u].z = a[i + 2];
                    if (i + 3 >= sh && i + 3 < end) v[u].w = a[i + 3];
                }
                if (keep) *reinterpret_cast<float4 *>(keep + i) = v[u];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kSweepAhead; ++u) {
            if (g0 + u * blockDim.x >= groups) break;                  // uniform: f sees whole wavefronts
            const uint32_t i = 4 * (g0 + u * blockDim.x + threadIdx.x);   // i + c < end implies g < groups
            f(i + 0 - sh, v[u].x, i + 0 >= sh && i + 0 < end);
            f(i + 1 - sh, v[u].y, i + 1 >= sh && i + 1 < end);
            f(i + 2 - sh, v[u].z, i + 2 >= sh && i + 2 < end);
            f(i + 3 - sh, v[u].w, i + 3 >= sh && i + 3 < end);
        }
    }
}

// hist[d] += 1 for the lanes that want it.  Equal digits are the rule (distances of one scale share their leading digit): the
// first wanting lane's digit is added once per wavefront, as vat_select_kernel does.
__device__ __forceinline__ void hist_add(uint32_t *hist, bool want, uint32_t d, uint32_t lane)
{
    const unsigned long long m = __ballot(want);
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t ld = __shfl(d, leader);
        const unsigned long long same = __ballot(want && d == ld);
        if ((int)lane == leader) atomicAdd(&hist[ld], (uint32_t)__popcll(same));
        else if (want && d != ld) atomicAdd(&hist[d], 1u);
    }
}

template <bool RESIDENT>
__global__ __launch_bounds__(1024) void neighbors_select_kernel(const SelectParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(lds);           // [kcap] (key << 32 | j)
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds + (size_t)P.kcap * 8);          // [kHistWords]
    uint32_t *s_cnt = hist + kHistWords;                                              // [2 parities][16 wavefronts], zeroed with hist
    uint32_t *s_next = s_cnt + 32;                                                    // [8] what wavefront 0 decides after a pass
    float *row = reinterpret_cast<float *>(s_next + 8);                               // RESIDENT: entry e at row[e + sh]

    const uint32_t slot = P.q_first + blockIdx.x;
    const uint32_t id = P.queries ? P.queries[slot] : slot;
    const float *x = P.src + (uint64_t)(P.from_panel ? blockIdx.x : id) * P.stride;
    const uint32_t n = P.n, k = P.k, self = P.skip_self ? id : 0xFFFFFFFFu;          // an entry's number is below 2^31
    const uint32_t sh = (uint32_t)(((uintptr_t)x >> 2) & 3u);
    const float *a = x - sh;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

    // ---- the k-th key among the candidates, or "all of them" when there are no more than k
    uint32_t prefix = 0, mask = 0, rank = k - 1, nan = 0, total = 0;
    bool all = false;
    for (int pass = 0; pass < 4 && !all; ++pass) {
        const int shift = 24 - 8 * pass;
        for (uint32_t h = threadIdx.x; h < kHistWords + 32; h += blockDim.x) hist[h] = 0;
        __syncthreads();
        auto digit = [&](uint32_t e, float v, bool live) {
            const bool is_nan = v != v;
            const uint32_t key = order_key(v + 0.0f);                                 // -0.0 and +0.0 tie
            const bool want = live && e != self && (is_nan ? pass == 0 : (key & mask) == prefix);
            hist_add(hist, want, is_nan ? 256u : (key >> shift) & 0xFFu, lane);
        };
        if (RESIDENT && pass > 0) sweep(row, sh, n, nullptr, digit);
        else sweep(a, sh, n, RESIDENT ? row : nullptr, digit);
        __syncthreads();
        if (wave == 0) {                                                              // lane l: digits 4l .. 4l + 3
            const uint4 h = *reinterpret_cast<const uint4 *>(hist + 4 * lane);
            const uint32_t sum = h.x + h.y + h.z + h.w;
            uint32_t incl = sum;
            for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
            const uint32_t found = __shfl(incl, 63);
            const bool take_all = pass == 0 && found <= k;
            const unsigned long long hit = __ballot(rank < incl);                     // not empty unless take_all: rank < found
            if (lane == 0) { s_next[2] = take_all; s_next[3] = hist[256]; s_next[4] = found; }
            if (hit && (int)lane == __ffsll((long long)hit) - 1) {
                uint32_t r = rank - (incl - sum), d = 4 * lane;
                if (r >= h.x) { r -= h.x; ++d; if (r >= h.y) { r -= h.y; ++d; if (r >= h.z) { r -= h.z; ++d; } } }
                s_next[0] = d << shift; s_next[1] = r;
            }
        }
        __syncthreads();
        if (pass == 0) { all = s_next[2] != 0; nan = s_next[3]; total = s_next[4]; }
        if (!all) { prefix |= s_next[0]; rank = s_next[1]; mask |= 0xFFu << shift; }
    }
    // all: every candidate is kept.  Otherwise the k-th candidate has key `prefix` and `rank` equal keys in front of it: the
    // entries below the key fill slots [0, n_below), the first `need` ties in index order the slots behind them.
    const uint32_t count = all ? total : k, need = all ? 0u : rank + 1, n_below = count - need;

    // ---- ordered compaction: blockDim entries per step, a slot is a prefix count over wavefronts (LDS) and lanes (ballot)
    const unsigned long long below_me = (1ull << lane) - 1;
    uint32_t below_done = 0, tie_done = 0, parity = 0;
    for (uint32_t e0 = 0; e0 < n; e0 += blockDim.x, parity ^= 1) {
        const uint32_t e = e0 + threadIdx.x;
        const bool live = e < n;
        const float v = live ? (RESIDENT ? row[e + sh] : x[e]) : 0.0f;
        const uint32_t key = order_key(v + 0.0f);
        const bool cand = live && e != self && v == v;
        const bool below = cand && (all || key < prefix), tie = cand && !all && key == prefix;
        const unsigned long long B = __ballot(below), T = __ballot(tie);
        uint32_t *cnt = s_cnt + parity * 16;                                          // per wavefront: below | ties << 16 (each <= 64)
        if (lane == 0) cnt[wave] = (uint32_t)__popcll(B) | ((uint32_t)__popcll(T) << 16);
        __syncthreads();
        uint32_t before = 0, whole = 0;                                               // sums of at most 16 x 64 per half: no carry
#pragma unroll
        for (uint32_t w4 = 0; w4 < 4; ++w4) {                                         // words of wavefronts that do not exist stay 0
            const uint4 c = reinterpret_cast<const uint4 *>(cnt)[w4];
            before += (4 * w4 + 0 < wave ? c.x : 0u) + (4 * w4 + 1 < wave ? c.y : 0u) + (4 * w4 + 2 < wave ? c.z : 0u) + (4 * w4 + 3 < wave ? c.w : 0u);
            whole += c.x + c.y + c.z + c.w;
        }
        const uint32_t b_at = below_done + (before & 0xFFFFu) + (uint32_t)__popcll(B & below_me);
        const uint32_t t_at = tie_done + (before >> 16) + (uint32_t)__popcll(T & below_me);
        below_done += whole & 0xFFFFu; tie_done += whole >> 16;
        const unsigned long long word = ((unsigned long long)key << 32) | e;
        if (below && b_at < n_below) buf[b_at] = word;                                // b_at < n_below by construction
        if (tie && t_at < need) buf[n_below + t_at] = word;
    }
    __syncthreads();

    // ---- ascending by (key, j): bitonic network over the next power of two, unused words at the top
    uint32_t width = 1;
    while (width < count) width <<= 1;                                                // <= kcap
    for (uint32_t s = count + threadIdx.x; s < width; s += blockDim.x) buf[s] = ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= width; size <<= 1) {
        for (uint32_t step = size >> 1; step > 0; step >>= 1) {
            for (uint32_t t = threadIdx.x; t < width / 2; t += blockDim.x) {
                const uint32_t i = ((t & ~(step - 1)) << 1) | (t & (step - 1)), j = i | step;
                const unsigned long long lo = buf[i], hi = buf[j];
                if ((lo > hi) == ((i & size) == 0)) { buf[i] = hi; buf[j] = lo; }
            }
            __syncthreads();
        }
    }

    // ---- the store: the matrix's own bits (a -0.0 stays -0.0), padding behind the candidates
    for (uint32_t s = threadIdx.x; s < k; s += blockDim.x) {
        uint32_t j = kPadIndex, bits = kPadBits;
        if (s < count) {
            j = (uint32_t)buf[s];                                                     // every word below `count` was written: j < n
            if (j < n) bits = __builtin_bit_cast(uint32_t, RESIDENT ? row[j + sh] : x[j]);
        }
        P.index[(uint64_t)slot * k + s] = j;
        P.distance[(uint64_t)slot * k + s] = bits;
    }
    if (threadIdx.x == 0) {
        P.count[slot] = count;
        if (P.nans) P.nans[slot] = nan;
    }
}

// panel[s][y] = d[y][column of slot q_first + s], s < n_slots: 64 x 64 tiles through LDS.  A wavefront reads 64 columns of one
// row (256 contiguous bytes when the columns are adjacent) and writes 64 rows of one column's panel row.
__global__ __launch_bounds__(256) void neighbors_gather_kernel(const float *__restrict__ d, uint32_t rows, uint32_t cols,
                                                               const uint32_t *__restrict__ queries, uint32_t q_first, uint32_t n_slots,
                                                               float *__restrict__ panel, uint64_t stride)
{
    __shared__ float tile[64][65];
    const uint32_t tiles_y = (rows + 63) / 64, tiles_x = (n_slots + 63) / 64, lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < (uint64_t)tiles_y * tiles_x; t += gridDim.x) {
        const uint32_t ty = (uint32_t)(t / tiles_x), tx = (uint32_t)(t % tiles_x);
        const uint32_t s = tx * 64 + lx;
        const uint32_t col = s < n_slots ? (queries ? queries[q_first + s] : q_first + s) : 0u;
        for (uint32_t r = ly; r < 64; r += 4) {
            const uint32_t y = ty * 64 + r;
            tile[r][lx] = (y < rows && s < n_slots) ? d[(uint64_t)y * cols + col] : 0.0f;
        }
        __syncthreads();
        for (uint32_t r = ly; r < 64; r += 4) {
            const uint32_t to = tx * 64 + r, y = ty * 64 + lx;
            if (to < n_slots && y < rows) panel[(uint64_t)to * stride + y] = tile[lx][r];
        }
        __syncthreads();
    }
}

size_t env_bytes(const char *name, size_t fallback)
{
    const char *text = std::getenv(name);
    if (!text || !*text) return fallback;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(text, &end, 10);
    return end && *end == 0 ? (size_t)v : fallback;
}

// The select of n_q queries whose output slots start at S.q_first.
int launch_select(apd_context *ctx, SelectParams S, uint32_t n_q, uint32_t resident_columns)
{
    const bool resident = S.n <= resident_columns;
    const size_t lds_bytes = (size_t)S.kcap * 8 + (kHistWords + 32 + 8) * sizeof(uint32_t) +
                             (resident ? (size_t)((S.n + 3 + 3) / 4) * 16 : 0);       // the row's groups: sh <= 3 entries in front
    const void *fn = resident ? reinterpret_cast<const void *>(neighbors_select_kernel<true>)
                              : reinterpret_cast<const void *>(neighbors_select_kernel<false>);
    if (lds_bytes > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    // 256 work-items where a row is short (more rows per compute unit); beyond 8192 entries 512 while two resident rows fit a compute
    // unit's LDS (measured at 16384 entries: 1.61 ms against 2.11 with 1024 and 2.46 with 256), 1024 otherwise; the answer is the same
    unsigned wg = S.n <= 8192 ? 256 : (resident && 2 * lds_bytes <= 160 * 1024 ? 512 : 1024);
    const size_t asked = env_bytes("APD_NEIGHBORS_WORKGROUP", 0);                     // tests and measurement only
    if (asked >= 64 && asked <= 1024 && asked % 64 == 0) wg = (unsigned)asked;
    for (uint32_t done = 0; done < n_q;) {
        const uint32_t part = std::min<uint32_t>(n_q - done, 1u << 30);
        SelectParams L = S;
        L.q_first = S.q_first + done;
        if (S.from_panel) L.src = S.src + (uint64_t)done * S.stride;
        if (resident) hipLaunchKernelGGL(neighbors_select_kernel<true>, dim3(part), dim3(wg), lds_bytes, ctx->stream, L);
        else hipLaunchKernelGGL(neighbors_select_kernel<false>, dim3(part), dim3(wg), lds_bytes, ctx->stream, L);
        HIP_TRY(ctx, hipGetLastError());
        done += part;
    }
    return APD_OK;
}

}  // namespace

// The gather's launch, shared with the column form of apd_silhouette (silhouette.hip).  n_slots, rows > 0.
hipError_t apd::launch_column_gather(const float *d, uint32_t rows, uint32_t cols, const uint32_t *d_queries, uint32_t q_first,
                                     uint32_t n_slots, float *panel, uint64_t stride, hipStream_t stream)
{
    const uint64_t tiles = (uint64_t)((rows + 63) / 64) * ((n_slots + 63) / 64);
    hipLaunchKernelGGL(neighbors_gather_kernel, dim3((unsigned)std::min<uint64_t>(tiles, 65536)), dim3(256), 0, stream, d, rows, cols, d_queries,
                       q_first, n_slots, panel, stride);
    return hipGetLastError();
}

// Workspaces, both owned by the context so that the device form only enqueues: ws_misc [query list | host form: matrix | index |
// distance | count | nans], ws_neighbors the column form's panel.
extern "C" int apd_neighbors(apd_context *ctx, const float *distances, int on_device, uint32_t rows, uint32_t cols, int axis,
                             const uint32_t *queries, uint32_t n_queries, uint32_t k, int skip_self, uint32_t *index, float *distance,
                             uint32_t *count, uint32_t *nans)
{
    if (!ctx || k == 0 || k > APD_NEIGHBORS_MAX_K || (axis != APD_NEIGHBORS_ROWS && axis != APD_NEIGHBORS_COLUMNS)) return APD_ERR_INVALID_ARG;
    const bool by_rows = axis == APD_NEIGHBORS_ROWS;
    const uint32_t named = by_rows ? rows : cols, n = by_rows ? cols : rows;          // a query names one of `named`, ranks n entries
    const uint32_t n_q = queries ? n_queries : named;
    for (uint32_t q = 0; queries && q < n_q; ++q) if (queries[q] >= named) return APD_ERR_INVALID_ARG;
    if (n_q == 0) return APD_OK;
    if (!index || !distance || !count || (rows && cols && !distances)) return APD_ERR_INVALID_ARG;
    if (n > kLongestRow) { ctx->last_error = "apd_neighbors: 2^31 entries or more to rank per query"; return APD_ERR_UNSUPPORTED; }
    HIP_TRY(ctx, bind_device(ctx));
    // tests only; read at every call, and the answer does not depend on either
    const uint32_t resident_columns = (uint32_t)std::min<size_t>(env_bytes("APD_NEIGHBORS_LDS_COLUMNS", kResidentColumns), kResidentColumns);
    const size_t panel_bytes = env_bytes("APD_NEIGHBORS_WORKSPACE_BYTES", kWorkspaceBytes);

    auto round = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t mat_bytes = (size_t)rows * cols * sizeof(float), out_words = (size_t)n_q * k;
    const size_t o_mat = round(queries ? (size_t)n_q * 4 : 0), o_index = o_mat + (on_device ? 0 : round(mat_bytes));
    const size_t o_distance = o_index + round(out_words * 4), o_count = o_distance + round(out_words * 4), o_nans = o_count + round((size_t)n_q * 4);
    if (const int rc = reserve_ws(ctx, ctx->ws_misc, std::max<size_t>(on_device ? o_mat : o_nans + round((size_t)n_q * 4), 256))) return rc;
    char *ws = ctx->ws_misc.as<char>();
    const uint64_t panel_stride = std::max<uint64_t>(((uint64_t)n + 3) & ~3ull, 4);  // every panel row starts on 16 bytes
    uint32_t panel_cols = 0;
    if (!by_rows) {
        const uint64_t fit = std::max<uint64_t>(panel_bytes / (panel_stride * sizeof(float)), 1);
        panel_cols = (uint32_t)std::min<uint64_t>(fit >= 64 ? fit & ~63ull : fit, n_q);
        if (const int rc = reserve_ws(ctx, ctx->ws_neighbors, (size_t)panel_cols * panel_stride * sizeof(float))) return rc;
    }
    APD_AFFINITY(ctx, "neighbours launch");
    const uint32_t *d_queries = queries ? reinterpret_cast<const uint32_t *>(ws) : nullptr;
    if (queries) HIP_TRY(ctx, hipMemcpyAsync(ws, queries, (size_t)n_q * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!on_device && mat_bytes) HIP_TRY(ctx, hipMemcpyAsync(ws + o_mat, distances, mat_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (queries && on_device) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));        // the caller's list has left the host

    SelectParams S{};
    S.n = n; S.queries = d_queries; S.k = k; S.skip_self = skip_self != 0;
    S.kcap = 2;
    while (S.kcap < std::min(k, n)) S.kcap <<= 1;
    S.index = on_device ? index : reinterpret_cast<uint32_t *>(ws + o_index);
    S.distance = on_device ? reinterpret_cast<uint32_t *>(distance) : reinterpret_cast<uint32_t *>(ws + o_distance);
    S.count = on_device ? count : reinterpret_cast<uint32_t *>(ws + o_count);
    S.nans = on_device ? nans : (nans ? reinterpret_cast<uint32_t *>(ws + o_nans) : nullptr);
    const float *d_mat = on_device ? distances : reinterpret_cast<const float *>(ws + o_mat);
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (by_rows) {
        S.src = d_mat; S.stride = cols; S.from_panel = 0; S.q_first = 0;
        if (const int rc = launch_select(ctx, S, n_q, resident_columns)) return rc;
    } else {
        float *panel = ctx->ws_neighbors.as<float>();
        S.src = panel; S.stride = panel_stride; S.from_panel = 1;
        for (uint64_t at = 0; at < n_q; at += panel_cols) {                           // the stream orders a panel's select before its refill
            const uint32_t first = (uint32_t)at, part = std::min(panel_cols, n_q - first);
            if (n) HIP_TRY(ctx, launch_column_gather(d_mat, rows, cols, d_queries, first, part, panel, panel_stride, ctx->stream));
            S.q_first = first;
            if (const int rc = launch_select(ctx, S, part, resident_columns)) return rc;
        }
    }
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    if (on_device) return APD_OK;
    HIP_TRY(ctx, hipMemcpyAsync(index, S.index, out_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(distance, S.distance, out_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(count, S.count, (size_t)n_q * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (nans) HIP_TRY(ctx, hipMemcpyAsync(nans, S.nans, (size_t)n_q * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}
