// Density clustering (DBSCAN with a fixed border rule) over a distance matrix in HBM, up to APD_DENSITY_MAX_SETTINGS (eps, min_pts)
// settings per call -- apd_density_clusters (include/apd.h), DESIGN.md section 4.24.
//
//   density_adjacency_kernel   the one pass over the f32 matrix: a workgroup takes the tiles (I, J) and (J, I), I <= J, 64 x 64 each,
//                              through LDS (rows padded to 65), evaluates d <= eps for every setting on an entry and its mirror, and
//                              turns each wavefront's 64 answers into one word of the bit matrix bits[s][i][J] / bits[s][j][I] with a
//                              ballot.  Entries outside the matrix and the diagonal enter as NaN (never near), so their bits are 0.
//                              NaN entries off the diagonal: one integer atomic per workgroup.
//   density_degree_kernel      degree = popcount of a bit row, the core mask (a word per 64 rows), label[i] = i.
//   density_propagate_kernel   a wavefront per core row: the minimum label over its core neighbours; lowers label[i] and the label of
//                              i's old label (hooking) with atomicMin, then label[i] to label[label[i]] (pointer jumping); sets the
//                              setting's "changed" word whenever it lowered a value.  The host enqueues rounds until a batch of them
//                              left the word 0.
//   density_border_kernel      after convergence: a non-core row takes the minimum label over its core neighbours (border) or keeps
//                              its own number (noise); kind and the four counts.
//
// Everything behind the comparison is integer and every combination is a minimum, a popcount or a sum of counts, so the answer is a
// function of the matrix and the settings alone.  Labels only ever decrease, and only to numbers of core points of the same
// component; a round that lowered nothing read a stable array in which no core point has a core neighbour with a smaller label, so
// every component holds one value, and that value is its smallest member (label[i] <= i throughout).  DESIGN.md has the argument.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "apd_internal.h"

using namespace apd;

namespace {

constexpr size_t kWorkspaceBytes = (size_t)256 << 20;   // the bit planes of the settings processed together
constexpr uint32_t kLargest = 1u << 21;                 // tile pairs stay below 2^31 and a plane's words below 2^37
constexpr uint32_t kRoundsPerSync = 4;                  // rounds enqueued between two reads of the changed words
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t S_MAX = APD_DENSITY_MAX_SETTINGS;

struct EpsList { float v[S_MAX]; };
struct MinPtsList { uint32_t v[S_MAX]; };

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// vec: n is a multiple of 4 and the matrix starts on 16 bytes, so four entries of a tile row are one aligned 16-byte load and are
// inside or outside the matrix together.
template <bool BOTH>
__global__ __launch_bounds__(256) void density_adjacency_kernel(const float *__restrict__ d, uint32_t n, uint32_t words, int vec,
                                                                const EpsList eps, uint32_t n_set, unsigned long long *__restrict__ bits,
                                                                uint64_t plane_words, unsigned long long *nan_count)
{
    __shared__ float ta[64][65], tb[64][65];
    __shared__ uint32_t s_nan[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tile pair p = J (J + 1) / 2 + I, I <= J
    const uint64_t p = blockIdx.x;
    uint32_t J = (uint32_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((uint64_t)J * (J + 1) / 2 > p) --J;
    while ((uint64_t)(J + 1) * (J + 2) / 2 <= p) ++J;
    const uint32_t I = (uint32_t)(p - (uint64_t)J * (J + 1) / 2);
    const bool mirror = I != J;
    const float quiet = __builtin_nanf("");
    uint32_t nan = 0;

    if (vec) {
        const uint32_t q = tid & 15, r0 = tid >> 4;                                   // 16 rows of 16 x 16 bytes per step
        float4 va[4], vb[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t r = r0 + 16 * k;
            const uint32_t ya = I * 64 + r, xa = J * 64 + 4 * q, yb = J * 64 + r, xb = I * 64 + 4 * q;
            va[k] = vb[k] = make_float4(quiet, quiet, quiet, quiet);
            if (ya < n && xa < n) va[k] = *reinterpret_cast<const float4 *>(d + (uint64_t)ya * n + xa);
            if (mirror && yb < n && xb < n) vb[k] = *reinterpret_cast<const float4 *>(d + (uint64_t)yb * n + xb);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t r = r0 + 16 * k;
            const uint32_t ya = I * 64 + r, xa = J * 64 + 4 * q, yb = J * 64 + r, xb = I * 64 + 4 * q;
            const float a4[4] = {va[k].x, va[k].y, va[k].z, va[k].w}, b4[4] = {vb[k].x, vb[k].y, vb[k].z, vb[k].w};
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                const bool in_a = ya < n && xa < n && ya != xa + e;                   // the diagonal's value enters nothing
                nan += (in_a && a4[e] != a4[e]) ? 1u : 0u;
                ta[r][4 * q + e] = in_a ? a4[e] : quiet;
                if (mirror) {
                    const bool in_b = yb < n && xb < n;                               // (no diagonal in an off-diagonal tile)
                    nan += (in_b && b4[e] != b4[e]) ? 1u : 0u;
                    tb[r][4 * q + e] = in_b ? b4[e] : quiet;
                }
            }
        }
    } else {
        for (uint32_t r = wave; r < 64; r += 4) {
            const uint32_t ya = I * 64 + r, xa = J * 64 + lane, yb = J * 64 + r, xb = I * 64 + lane;
            float a = quiet, b = quiet;
            if (ya < n && xa < n && ya != xa) { a = d[(uint64_t)ya * n + xa]; nan += a != a ? 1u : 0u; }
            if (mirror && yb < n && xb < n) { b = d[(uint64_t)yb * n + xb]; nan += b != b ? 1u : 0u; }
            ta[r][lane] = a;
            if (mirror) tb[r][lane] = b;
        }
    }
    nan = wave_sum(nan);
    if (lane == 0) s_nan[wave] = nan;
    __syncthreads();
    if (nan_count && tid == 0) {
        const uint32_t total = s_nan[0] + s_nan[1] + s_nan[2] + s_nan[3];
        if (total) atomicAdd(nan_count, (unsigned long long)total);
    }

    // wavefront `wave`: rows 16 wave .. 16 wave + 15 of both tiles; lane k keeps the words of row 16 wave + k
    const float (*B)[65] = mirror ? tb : ta;
    unsigned long long up[S_MAX], low[S_MAX];
#pragma unroll
    for (uint32_t s = 0; s < S_MAX; ++s) up[s] = low[s] = 0;
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t r = wave * 16 + k;
        const float a = ta[r][lane], bt = B[lane][r];                                 // d[i][j] and d[j][i]: i = 64 I + r, j = 64 J + lane
        const float b = B[r][lane], at = ta[lane][r];                                 // d[j][i] and d[i][j]: j = 64 J + r, i = 64 I + lane
#pragma unroll
        for (uint32_t s = 0; s < S_MAX; ++s) {
            if (s < n_set) {
                const float e = eps.v[s];
                const bool na = a <= e, nbt = bt <= e, nb = b <= e, nat = at <= e;     // (no short circuits: the row loop stays branch-free)
                const unsigned long long w1 = __ballot(BOTH ? (na & nbt) : (na | nbt));
                const unsigned long long w2 = __ballot(BOTH ? (nb & nat) : (nb | nat));
                up[s] = lane == k ? w1 : up[s];
                low[s] = lane == k ? w2 : low[s];
            }
        }
    }
    if (lane < 16) {
        const uint32_t r = wave * 16 + lane, i = I * 64 + r, j = J * 64 + r;
#pragma unroll
        for (uint32_t s = 0; s < S_MAX; ++s) {
            if (s < n_set) {
                if (i < n) bits[s * plane_words + (uint64_t)i * words + J] = up[s];
                if (mirror && j < n) bits[s * plane_words + (uint64_t)j * words + I] = low[s];
            }
        }
    }
}

// grid (ceil(n / 64), settings): 64 rows per workgroup, 16 per wavefront.
__global__ __launch_bounds__(256) void density_degree_kernel(const unsigned long long *__restrict__ bits, uint64_t plane_words, uint32_t n,
                                                             uint32_t words, const MinPtsList min_pts, uint32_t *__restrict__ degree,
                                                             unsigned long long *__restrict__ core, uint32_t *__restrict__ label)
{
    __shared__ uint32_t s_core[64];
    const uint32_t s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t need = 0;
#pragma unroll
    for (uint32_t t = 0; t < S_MAX; ++t) if (t == s) need = min_pts.v[t];
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t r = wave * 16 + k, i = blockIdx.x * 64 + r;
        uint32_t c = 0;
        if (i < n) {
            const unsigned long long *row = bits + s * plane_words + (uint64_t)i * words;
            for (uint32_t w = lane; w < words; w += 64) c += (uint32_t)__popcll(row[w]);
        }
        c = wave_sum(c);
        if (lane == 0) {
            s_core[r] = (i < n && (uint64_t)c + 1 >= need) ? 1u : 0u;
            if (i < n) {
                if (degree) degree[(uint64_t)s * n + i] = c;
                label[(uint64_t)s * n + i] = i;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        const unsigned long long w = __ballot(s_core[lane] != 0);
        if (lane == 0) core[(uint64_t)s * words + blockIdx.x] = w;
    }
}

// The smallest label among the core neighbours of row i (kNone: it has none), by the whole wavefront.
__device__ __forceinline__ uint32_t least_core_label(const unsigned long long *row, const unsigned long long *core, const uint32_t *lab,
                                                     uint32_t words, uint32_t lane)
{
    uint32_t m = kNone;
    for (uint32_t w = lane; w < words; w += 64) {
        unsigned long long x = row[w] & core[w];
        while (x) {
            const uint32_t j = w * 64 + (uint32_t)__builtin_ctzll(x);                 // j < n: tail bits are 0
            x &= x - 1;
            const uint32_t l = lab[j];
            m = l < m ? l : m;
        }
    }
    return wave_min(m);
}

// grid (ceil(n / wavefronts of a workgroup), settings); a wavefront per row.  active: the settings still changing.
__global__ __launch_bounds__(1024) void density_propagate_kernel(const unsigned long long *__restrict__ bits, uint64_t plane_words, uint32_t n,
                                                                 uint32_t words, const unsigned long long *__restrict__ core, uint32_t *label,
                                                                 uint32_t *changed, uint32_t active)
{
    const uint32_t s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!((active >> s) & 1u)) return;
    const uint64_t at = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (at >= n) return;
    const uint32_t i = (uint32_t)at;
    const unsigned long long *cm = core + (uint64_t)s * words;
    if (!((cm[i >> 6] >> (i & 63)) & 1ull)) return;
    uint32_t *lab = label + (uint64_t)s * n;
    const uint32_t m = least_core_label(bits + s * plane_words + (uint64_t)i * words, cm, lab, words, lane);
    if (lane == 0) {
        uint32_t cur = lab[i];
        bool lowered = false;
        if (m < cur) {
            atomicMin(&lab[i], m);
            atomicMin(&lab[cur], m);                                                  // hooking: what i pointed at follows
            cur = m;
            lowered = true;
        }
        const uint32_t above = lab[cur];                                              // pointer jumping
        if (above < cur) { atomicMin(&lab[i], above); lowered = true; }
        if (lowered) changed[s] = 1u;
    }
}

// grid as the propagate kernel.  counts[s]: clusters, core, border, noise.
__global__ __launch_bounds__(1024) void density_border_kernel(const unsigned long long *__restrict__ bits, uint64_t plane_words, uint32_t n,
                                                              uint32_t words, const unsigned long long *__restrict__ core, uint32_t *label,
                                                              uint8_t *__restrict__ kind, uint32_t *counts)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t at = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (at < n) {
        const uint32_t i = (uint32_t)at;
        const unsigned long long *cm = core + (uint64_t)s * words;
        uint32_t *lab = label + (uint64_t)s * n;
        const bool is_core = ((cm[i >> 6] >> (i & 63)) & 1ull) != 0;
        uint32_t role = APD_DENSITY_CORE, m = kNone;
        if (!is_core) {
            m = least_core_label(bits + s * plane_words + (uint64_t)i * words, cm, lab, words, lane);
            role = m != kNone ? APD_DENSITY_BORDER : APD_DENSITY_NOISE;
        }
        if (lane == 0) {
            if (is_core) { if (lab[i] == i) atomicAdd(&s_cnt[0], 1u); }               // a cluster is named by its smallest core point
            else lab[i] = m != kNone ? m : i;                                         // only core labels are read by the others
            if (kind) kind[(uint64_t)s * n + i] = (uint8_t)role;
            atomicAdd(&s_cnt[role == APD_DENSITY_CORE ? 1 : (role == APD_DENSITY_BORDER ? 2 : 3)], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counts[s * 4 + threadIdx.x], s_cnt[threadIdx.x]);
}

size_t env_number(const char *name, size_t fallback)
{
    const char *text = std::getenv(name);
    if (!text || !*text) return fallback;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(text, &end, 10);
    return end && *end == 0 ? (size_t)v : fallback;
}

}  // namespace

// Workspaces: ws_density [bit planes of a group of settings | their core masks | changed words | NaN count], ws_misc the host form's
// [matrix | labels | degree | counts | nans | kind].
extern "C" int apd_density_clusters(apd_context *ctx, const float *distances, int on_device, uint32_t n, int link, const float *eps,
                                    const uint32_t *min_pts, uint32_t n_settings, uint32_t *labels, uint8_t *kind, uint32_t *degree,
                                    uint32_t *counts, uint64_t *nans)
{
    if (!ctx || (link != APD_DENSITY_EITHER && link != APD_DENSITY_BOTH) || n_settings == 0 || n_settings > S_MAX || !eps || !min_pts ||
        !labels || !counts || (n && !distances))
        return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_settings; ++s) if (min_pts[s] == 0) return APD_ERR_INVALID_ARG;
    if (n > kLargest) { ctx->last_error = "apd_density_clusters: more than 2^21 instances"; return APD_ERR_UNSUPPORTED; }
    HIP_TRY(ctx, bind_device(ctx));
    const uint32_t S = n_settings;
    ctx->density_rounds = 0;
    for (float &ms : ctx->density_phase_ms) ms = 0.0f;
    if (n == 0) {
        if (on_device) {
            HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)S * 16, ctx->stream));
            if (nans) HIP_TRY(ctx, hipMemsetAsync(nans, 0, 8, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        } else {
            std::memset(counts, 0, (size_t)S * 16);
            if (nans) *nans = 0;
        }
        return APD_OK;
    }
    // tests and measurement only; read at every call, and the answer does not depend on any of them
    const size_t plane_budget = env_number("APD_DENSITY_WORKSPACE_BYTES", kWorkspaceBytes);
    const uint32_t rounds_per_sync = (uint32_t)std::min<size_t>(std::max<size_t>(env_number("APD_DENSITY_ROUNDS_PER_SYNC", kRoundsPerSync), 1), 1024);
    unsigned wg = 256;
    const size_t asked = env_number("APD_DENSITY_WORKGROUP", 0);
    if (asked >= 64 && asked <= 1024 && asked % 64 == 0) wg = (unsigned)asked;

    auto round = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const uint32_t words = (n + 63) / 64;
    const uint64_t plane_words = (uint64_t)n * words;
    const size_t plane_bytes = (size_t)plane_words * 8;
    const uint32_t group = (uint32_t)std::min<size_t>(std::max<size_t>(plane_budget / plane_bytes, 1), S);   // at least one plane is taken
    const size_t o_core = round((size_t)group * plane_bytes), o_changed = o_core + round((size_t)group * words * 8);
    const size_t o_nan = o_changed + 256, total = o_nan + 256;
    if (const int rc = reserve_ws(ctx, ctx->ws_density, total)) return rc;
    char *ws = ctx->ws_density.as<char>();
    unsigned long long *d_bits = reinterpret_cast<unsigned long long *>(ws);
    unsigned long long *d_core = reinterpret_cast<unsigned long long *>(ws + o_core);
    uint32_t *d_changed = reinterpret_cast<uint32_t *>(ws + o_changed);
    unsigned long long *d_nan = reinterpret_cast<unsigned long long *>(ws + o_nan);

    const size_t mat_bytes = (size_t)n * n * sizeof(float), per_sample = (size_t)S * n * 4;
    const size_t h_labels = round(mat_bytes), h_degree = h_labels + round(per_sample), h_counts = h_degree + (degree ? round(per_sample) : 0);
    const size_t h_kind = h_counts + 256, h_total = h_kind + (kind ? round((size_t)S * n) : 0);
    const float *d_mat = distances;
    uint32_t *d_labels = labels, *d_degree = degree, *d_counts = counts;
    uint8_t *d_kind = kind;
    if (!on_device) {
        if (const int rc = reserve_ws(ctx, ctx->ws_misc, h_total)) return rc;
        char *hs = ctx->ws_misc.as<char>();
        d_mat = reinterpret_cast<const float *>(hs);
        d_labels = reinterpret_cast<uint32_t *>(hs + h_labels);
        d_degree = degree ? reinterpret_cast<uint32_t *>(hs + h_degree) : nullptr;
        d_counts = reinterpret_cast<uint32_t *>(hs + h_counts);
        d_kind = kind ? reinterpret_cast<uint8_t *>(hs + h_kind) : nullptr;
    }
    APD_AFFINITY(ctx, "density launch");
    hipEvent_t phase[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EventGuard { hipEvent_t *e; ~EventGuard() { for (int k = 0; k < 5; ++k) if (e[k]) hipEventDestroy(e[k]); } } guard{phase};
    if (ctx->timing) for (hipEvent_t &e : phase) HIP_TRY(ctx, hipEventCreate(&e));
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_misc.ptr, distances, mat_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)S * 16, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_nan, 0, 8, ctx->stream));

    const uint64_t tiles = words, pairs = tiles * (tiles + 1) / 2;                    // < 2^31 for n <= kLargest
    const int vec = (n % 4 == 0 && (reinterpret_cast<uintptr_t>(d_mat) & 15u) == 0) ? 1 : 0;
    const unsigned waves = wg / 64, row_blocks = (unsigned)(((uint64_t)n + waves - 1) / waves);
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (uint32_t s0 = 0; s0 < S; s0 += group) {
        const uint32_t g = std::min(group, S - s0);
        EpsList E{};
        MinPtsList M{};
        for (uint32_t s = 0; s < g; ++s) { E.v[s] = eps[s0 + s]; M.v[s] = min_pts[s0 + s]; }
        uint32_t *g_labels = d_labels + (size_t)s0 * n, *g_degree = d_degree ? d_degree + (size_t)s0 * n : nullptr;
        uint8_t *g_kind = d_kind ? d_kind + (size_t)s0 * n : nullptr;
        if (ctx->timing) HIP_TRY(ctx, hipEventRecord(phase[0], ctx->stream));
        unsigned long long *g_nan = s0 == 0 ? d_nan : nullptr;                        // a later group re-reads the matrix: NaNs are counted once
        if (link == APD_DENSITY_BOTH)
            hipLaunchKernelGGL(density_adjacency_kernel<true>, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, d_mat, n, words, vec, E, g, d_bits,
                               plane_words, g_nan);
        else
            hipLaunchKernelGGL(density_adjacency_kernel<false>, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, d_mat, n, words, vec, E, g, d_bits,
                               plane_words, g_nan);
        HIP_TRY(ctx, hipGetLastError());
        if (ctx->timing) HIP_TRY(ctx, hipEventRecord(phase[1], ctx->stream));
        hipLaunchKernelGGL(density_degree_kernel, dim3(words, g), dim3(256), 0, ctx->stream, d_bits, plane_words, n, words, M, g_degree, d_core,
                           g_labels);
        HIP_TRY(ctx, hipGetLastError());
        if (ctx->timing) HIP_TRY(ctx, hipEventRecord(phase[2], ctx->stream));
        // the component search: rounds until a batch of them lowered nothing.  A round moves every label at least one step along a
        // shortest path towards its component's minimum, so n rounds always suffice.
        uint32_t active = (1u << g) - 1u;
        uint64_t rounds = 0;
        while (active) {
            HIP_TRY(ctx, hipMemsetAsync(d_changed, 0, S_MAX * 4, ctx->stream));
            for (uint32_t r = 0; r < rounds_per_sync; ++r) {
                hipLaunchKernelGGL(density_propagate_kernel, dim3(row_blocks, g), dim3(wg), 0, ctx->stream, d_bits, plane_words, n, words, d_core,
                                   g_labels, d_changed, active);
                HIP_TRY(ctx, hipGetLastError());
            }
            rounds += rounds_per_sync;
            uint32_t h_changed[S_MAX];
            HIP_TRY(ctx, hipMemcpyAsync(h_changed, d_changed, S_MAX * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            active = 0;
            for (uint32_t s = 0; s < g; ++s) if (h_changed[s]) active |= 1u << s;
            if (active && rounds > (uint64_t)n + rounds_per_sync) {
                ctx->last_error = "apd_density_clusters: the component search did not settle within n rounds";
                return APD_ERR_HIP;
            }
        }
        ctx->density_rounds += (uint32_t)rounds;
        if (ctx->timing) HIP_TRY(ctx, hipEventRecord(phase[3], ctx->stream));
        hipLaunchKernelGGL(density_border_kernel, dim3(row_blocks, g), dim3(wg), 0, ctx->stream, d_bits, plane_words, n, words, d_core, g_labels,
                           g_kind, d_counts + (size_t)s0 * 4);
        HIP_TRY(ctx, hipGetLastError());
        if (ctx->timing) {
            HIP_TRY(ctx, hipEventRecord(phase[4], ctx->stream));
            HIP_TRY(ctx, hipEventSynchronize(phase[4]));
            for (int k = 0; k < 4; ++k) {
                float ms = 0.0f;
                HIP_TRY(ctx, hipEventElapsedTime(&ms, phase[k], phase[k + 1]));
                ctx->density_phase_ms[k] += ms;
            }
        }
    }
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    if (on_device) {
        if (nans) HIP_TRY(ctx, hipMemcpyAsync(nans, d_nan, 8, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(labels, d_labels, per_sample, hipMemcpyDeviceToHost, ctx->stream));
        if (degree) HIP_TRY(ctx, hipMemcpyAsync(degree, d_degree, per_sample, hipMemcpyDeviceToHost, ctx->stream));
        if (kind) HIP_TRY(ctx, hipMemcpyAsync(kind, d_kind, (size_t)S * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, (size_t)S * 16, hipMemcpyDeviceToHost, ctx->stream));
        if (nans) HIP_TRY(ctx, hipMemcpyAsync(nans, d_nan, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

extern "C" int apd_density_last_profile(apd_context *ctx, float *phase_ms, uint32_t *rounds)
{
    if (!ctx || !phase_ms || !rounds) return APD_ERR_INVALID_ARG;
    for (int k = 0; k < 4; ++k) phase_ms[k] = ctx->density_phase_ms[k];
    *rounds = ctx->density_rounds;
    return APD_OK;
}
