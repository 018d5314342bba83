// The density hierarchy of a distance matrix in HBM: core distances and the minimum spanning forest of the mutual-reachability graph
// -- apd_density_tree and the host-only apd_density_tree_cut / apd_density_tree_operations (include/apd.h), DESIGN.md section 4.25.
//
//   tree_init_kernel      comp[v] = v, and the core key of every vertex when it needs no select (min_pts = 1: -INF; min_pts > n: missing).
//   tree_core_kernel      a workgroup per row i: key(sym(i, j)) from the row and its mirror column (a row of the [panel][n] gather of
//                         neighbors.hip), and an 8-bit radix select of the (min_pts - 1)-th smallest key, the histogram in LDS.  The keys
//                         are formed again in each of the four digit passes: the row and the panel row are 8 n bytes that the pass
//                         before left in L2.
//   tree_scan_kernel      one Boruvka round's pass over the matrix, in density_adjacency_kernel's access pattern: a workgroup takes the
//                         tiles (I, J) and (J, I), I <= J, through LDS; a work-item per row of either tile walks half of the row's 64
//                         mutual-reachability keys and keeps the smallest (key, other) whose other end lies in another component; the
//                         two halves meet in LDS and one 64-bit atomic minimum per row reaches best[row] -- none when the row's word
//                         is already below the candidate.  A tile pair whose 128 vertices share one component is left without
//                         reading the matrix.  The first round also counts the NaN entries.
//   tree_reduce_kernel    rows to components on the full (key, lo, hi): a minimum of (key, lo) per component, then, among the rows that
//                         hold it, a minimum of hi (two launches: 32 + 21 + 21 bits do not fit one word).
//   tree_hook_kernel      every root with an edge hooks onto the root at the edge's other end and appends the edge -- unless that root
//                         chose the same edge and has the larger number: then it stays a root and appends nothing.
//   tree_jump_kernel      comp[v] = the root above comp[v] (the parent words of a round are stable while it runs).
//   tree_sort_*           bitonic sort of the appended edges by (key, i, j): steps below 1024 elements in LDS, the others in HBM.
//   tree_finish_kernel    keys back to floats: core[n], the edges, the padding behind them.
//
// Every combination is a minimum of unique integer words or a sort of unique words, so the answer is a function of the matrix, the
// link and min_pts alone.  DESIGN.md has the arguments for uniqueness and for the hooking rule.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "apd_internal.h"

using namespace apd;

namespace {

constexpr size_t kPanelBytes = (size_t)256 << 20;       // the gathered mirror columns of a group of rows
constexpr uint32_t kLargest = 1u << 21;                 // tile pairs stay below 2^31
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMissing = 0xFFFFFFFFu;              // the key of NaN: behind +INF (0xFF800000)
constexpr uint32_t kMinusInf = 0x007FFFFFu;             // key(-INF)
constexpr unsigned long long kNoEdge = ~0ull;
constexpr uint32_t kSortChunk = 1024;                   // elements a workgroup of the local sort holds in LDS

// The order of the contract: NaN is missing and last, the two zeros are one value, everything else in IEEE order.
__host__ __device__ __forceinline__ uint32_t tree_key(float v)
{
    if (v != v) return kMissing;
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float tree_value(uint32_t key)
{
    const uint32_t u = key == kMissing ? 0x7FC00000u : ((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
    float v;
    memcpy(&v, &u, 4);
    return v;
}
template <bool BOTH>
__device__ __forceinline__ uint32_t sym_key(float a, float b)
{
    const uint32_t ka = tree_key(a), kb = tree_key(b);
    return BOTH ? (ka > kb ? ka : kb) : (ka < kb ? ka : kb);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void tree_init_kernel(uint32_t n, uint32_t core_key, uint32_t *__restrict__ comp, uint32_t *__restrict__ ck)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) { comp[v] = (uint32_t)v; ck[v] = core_key; }
}

// grid: the rows first .. first + gridDim.x - 1; panel row b is column first + b of the matrix.  rank < n - 1: the 0-based rank of the
// selected key among the n - 1 keys of the row.
template <bool BOTH>
__global__ __launch_bounds__(1024) void tree_core_kernel(const float *__restrict__ d, const float *__restrict__ panel, uint64_t stride,
                                                         uint32_t n, uint32_t first, uint32_t rank, uint32_t *__restrict__ ck)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_rank;
    const uint32_t tid = threadIdx.x, lane = tid & 63, i = first + blockIdx.x;
    const float *row = d + (uint64_t)i * n, *col = panel + (uint64_t)blockIdx.x * stride;
    uint32_t prefix = 0, mask = 0, r = rank;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t b = tid; b < 256; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        for (uint32_t j = tid; j < n; j += blockDim.x) {
            if (j == i) continue;
            const uint32_t k = sym_key<BOTH>(row[j], col[j]);
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                                               // lane l: bins 4 l .. 4 l + 3
            const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const uint32_t own = h0 + h1 + h2 + h3;
            uint32_t incl = own;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if ((int)lane >= o) incl += t; }
            const uint32_t excl = incl - own;
            if (excl <= r && r < incl) {                                              // one lane: the keys under the prefix number more than r
                uint32_t c = excl, b = 4 * lane;
                if (r >= c + h0) { c += h0; ++b; if (r >= c + h1) { c += h1; ++b; if (r >= c + h2) { c += h2; ++b; } } }
                s_prefix = prefix | (b << shift);
                s_rank = r - c;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        r = s_rank;
        mask |= 255u << shift;
    }
    if (tid == 0) ck[i] = prefix;
}

// vec: as density_adjacency_kernel's.  nan_count: the first round only.
template <bool BOTH>
__global__ __launch_bounds__(256) void tree_scan_kernel(const float *__restrict__ d, uint32_t n, int vec, const uint32_t *__restrict__ ck,
                                                        const uint32_t *__restrict__ comp, unsigned long long *best,
                                                        unsigned long long *nan_count)
{
    __shared__ float ta[64][65], tb[64][65];
    __shared__ uint32_t s_comp[2][64], s_ck[2][64];
    __shared__ unsigned long long s_best[2][64];
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

    int differs = 0;
    if (tid < 128) {                                                                  // side 0: the vertices of I, side 1: of J
        const uint32_t v = (wave ? J : I) * 64 + lane;
        const uint32_t c = v < n ? comp[v] : kNone;
        s_comp[wave][lane] = c;
        s_ck[wave][lane] = v < n ? ck[v] : kMissing;
        s_best[wave][lane] = kNoEdge;
        differs = v < n && c != comp[I * 64];
    }
    differs = __syncthreads_or(differs);
    if (!differs && !nan_count) return;                                               // one component: no edge of these tiles leaves it

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

    // wavefronts 0, 1: the rows of tile (I, J) against the vertices of J; 2, 3: the rows of tile (J, I) against the vertices of I.
    // Lane r owns row r and walks 32 of its entries; entries outside the matrix and the diagonal are NaN, so their key is missing.
    const uint32_t side = wave >> 1, half = wave & 1;
    if (side == 0 || mirror) {
        const float (*B)[65] = mirror ? tb : ta;
        const uint32_t mine = s_comp[side][lane], my_core = s_ck[side][lane], other_base = (side ? I : J) * 64;
        unsigned long long low = kNoEdge;
        for (uint32_t c = half * 32; c < half * 32 + 32; ++c) {
            const float a = side ? B[lane][c] : ta[lane][c], b = side ? ta[c][lane] : B[c][lane];   // the entry and its mirror
            uint32_t mr = sym_key<BOTH>(a, b);
            const uint32_t oc = s_ck[side ^ 1][c];
            mr = mr > my_core ? mr : my_core;
            mr = mr > oc ? mr : oc;
            const unsigned long long cand = ((unsigned long long)mr << 32) | (other_base + c);
            if (mr != kMissing && s_comp[side ^ 1][c] != mine && cand < low) low = cand;
        }
        if (low != kNoEdge) atomicMin(&s_best[side][lane], low);
    }
    __syncthreads();
    if (tid < 128) {
        const uint32_t v = (wave ? J : I) * 64 + lane;
        const unsigned long long low = s_best[wave][lane];
        if (low != kNoEdge && v < n && (wave == 0 || mirror) &&
            low < __hip_atomic_load(&best[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))   // the word only ever falls
            atomicMin(&best[v], low);
    }
}

// step 0: cbest[c] = min (key, lo); step 1: chi[c] = min hi over the rows whose (key, lo) is cbest[c].
__global__ void tree_reduce_kernel(uint32_t n, int step, const uint32_t *__restrict__ comp, const unsigned long long *__restrict__ best,
                                   unsigned long long *cbest, uint32_t *chi)
{
    const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n) return;
    const uint32_t v = (uint32_t)at;
    const unsigned long long b = best[v];
    if (b == kNoEdge) return;
    const uint32_t o = (uint32_t)b, lo = v < o ? v : o, hi = v < o ? o : v, c = comp[v];
    const unsigned long long word = (b & 0xFFFFFFFF00000000ull) | lo;
    if (step == 0) atomicMin(&cbest[c], word);
    else if (cbest[c] == word) atomicMin(&chi[c], hi);
}

// sort_hi / sort_lo: `capacity` slots; a forest never fills more.
__global__ void tree_hook_kernel(uint32_t n, const uint32_t *__restrict__ comp, const unsigned long long *__restrict__ cbest,
                                 const uint32_t *__restrict__ chi, uint32_t *__restrict__ parent, uint32_t *count,
                                 unsigned long long *__restrict__ sort_hi, uint32_t *__restrict__ sort_lo, uint32_t capacity)
{
    const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n) return;
    const uint32_t v = (uint32_t)at;
    if (comp[v] != v) return;                                                         // roots only
    const unsigned long long e = cbest[v];
    if (e == kNoEdge) { parent[v] = v; return; }
    const uint32_t lo = (uint32_t)e, hi = chi[v];
    if (lo >= n || hi >= n) { parent[v] = v; return; }                                // (never: a row of v's component holds the edge)
    const uint32_t c_lo = comp[lo], other = c_lo == v ? comp[hi] : c_lo;
    if (cbest[other] == e && chi[other] == hi && v < other) { parent[v] = v; return; }   // both chose this edge: the smaller number stays
    parent[v] = other;
    const uint32_t slot = atomicAdd(count, 1u);
    if (slot < capacity) { sort_hi[slot] = e; sort_lo[slot] = hi; }
}

__global__ void tree_jump_kernel(uint32_t n, uint32_t *comp, const uint32_t *__restrict__ parent)
{
    const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n) return;
    uint32_t r = comp[at];
    for (uint32_t step = 0; step < n; ++step) {                                       // (the hooks form a forest: the walk ends at a root)
        const uint32_t above = parent[r];
        if (above == r) break;
        r = above;
    }
    comp[at] = r;
}

__device__ __forceinline__ bool edge_above(unsigned long long a_hi, uint32_t a_lo, unsigned long long b_hi, uint32_t b_lo)
{
    return a_hi > b_hi || (a_hi == b_hi && a_lo > b_lo);
}

// One compare-exchange step (k, j) of the bitonic network over `count` (a power of two) elements; a work-item per pair.
__global__ void tree_sort_global_kernel(unsigned long long *hi, uint32_t *lo, uint32_t count, uint32_t k, uint32_t j)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count / 2) return;
    const uint32_t x = (uint32_t)(((t & ~(uint64_t)(j - 1)) << 1) | (t & (j - 1))), y = x | j;
    const unsigned long long xh = hi[x], yh = hi[y];
    const uint32_t xl = lo[x], yl = lo[y];
    if (edge_above(xh, xl, yh, yl) == ((x & k) == 0)) { hi[x] = yh; lo[x] = yl; hi[y] = xh; lo[y] = xl; }
}

// The steps of the stages k_from .. k_to whose distance is below kSortChunk, a chunk of kSortChunk elements per workgroup in LDS.
__global__ __launch_bounds__(kSortChunk / 2) void tree_sort_local_kernel(unsigned long long *hi, uint32_t *lo, uint32_t count, uint32_t k_from,
                                                                         uint32_t k_to)
{
    __shared__ unsigned long long s_hi[kSortChunk];
    __shared__ uint32_t s_lo[kSortChunk];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * kSortChunk;
    for (uint32_t e = tid; e < kSortChunk; e += kSortChunk / 2) {
        const bool in = base + e < count;
        s_hi[e] = in ? hi[base + e] : kNoEdge;
        s_lo[e] = in ? lo[base + e] : kNone;
    }
    __syncthreads();
    for (uint32_t k = k_from; k <= k_to; k <<= 1) {
        for (uint32_t j = (k >> 1) < kSortChunk / 2 ? (k >> 1) : kSortChunk / 2; j > 0; j >>= 1) {
            const uint32_t x = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), y = x | j;
            const unsigned long long xh = s_hi[x], yh = s_hi[y];
            const uint32_t xl = s_lo[x], yl = s_lo[y];
            if (edge_above(xh, xl, yh, yl) == (((base + x) & k) == 0)) { s_hi[x] = yh; s_lo[x] = yl; s_hi[y] = xh; s_lo[y] = xl; }
            __syncthreads();
        }
    }
    for (uint32_t e = tid; e < kSortChunk; e += kSortChunk / 2)
        if (base + e < count) { hi[base + e] = s_hi[e]; lo[base + e] = s_lo[e]; }
}

// core[n]; the n - 1 edge slots: the first n_edges from the sorted words, the padding behind them.
__global__ void tree_finish_kernel(uint32_t n, uint32_t n_edges, const uint32_t *__restrict__ ck, const unsigned long long *__restrict__ sort_hi,
                                   const uint32_t *__restrict__ sort_lo, float *__restrict__ core, uint32_t *__restrict__ edge_i,
                                   uint32_t *__restrict__ edge_j, float *__restrict__ weight)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    core[t] = tree_value(ck[t]);
    if (t + 1 >= n) return;
    const bool edge = t < n_edges;
    const unsigned long long e = edge ? sort_hi[t] : kNoEdge;
    edge_i[t] = (uint32_t)e;
    edge_j[t] = edge ? sort_lo[t] : kNone;
    weight[t] = tree_value((uint32_t)(e >> 32));
}

size_t env_number(const char *name, size_t fallback)
{
    const char *text = std::getenv(name);
    if (!text || !*text) return fallback;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(text, &end, 10);
    return end && *end == 0 ? (size_t)v : fallback;
}

// Union-find over the vertices of an edge list (host entry points).
struct Forest {
    std::vector<uint32_t> up;
    explicit Forest(uint32_t n) : up(n) { for (uint32_t v = 0; v < n; ++v) up[v] = v; }
    uint32_t find(uint32_t v)
    {
        while (up[v] != v) { up[v] = up[up[v]]; v = up[v]; }
        return v;
    }
    bool join(uint32_t a, uint32_t b)                                                 // false: already joined
    {
        a = find(a);
        b = find(b);
        if (a == b) return false;
        if (a < b) up[b] = a; else up[a] = b;                                         // the root is the smallest vertex
        return true;
    }
};

bool is_forest(uint32_t n, const uint32_t *edge_i, const uint32_t *edge_j, uint32_t n_edges)
{
    if (n_edges && (!edge_i || !edge_j || n_edges >= n)) return false;
    Forest f(n);
    for (uint32_t t = 0; t < n_edges; ++t)
        if (edge_j[t] >= n || edge_i[t] >= edge_j[t] || !f.join(edge_i[t], edge_j[t])) return false;
    return true;
}

}  // namespace

// Workspaces: ws_density_tree [core keys | comp | parent | best | cbest | chi | sort hi | sort lo | edge count | NaN count],
// ws_neighbors the panel of mirror columns, ws_misc the host form's [matrix | core | edge_i | edge_j | weight].
extern "C" int apd_density_tree(apd_context *ctx, const float *distances, int on_device, uint32_t n, int link, uint32_t min_pts, float *core,
                                uint32_t *edge_i, uint32_t *edge_j, float *weight, uint32_t *n_edges, uint64_t *nans)
{
    if (!ctx || (link != APD_DENSITY_EITHER && link != APD_DENSITY_BOTH) || min_pts == 0 || !n_edges || !nans || (n && (!distances || !core)) ||
        (n > 1 && (!edge_i || !edge_j || !weight)))
        return APD_ERR_INVALID_ARG;
    if (n > kLargest) { ctx->last_error = "apd_density_tree: more than 2^21 instances"; return APD_ERR_UNSUPPORTED; }
    HIP_TRY(ctx, bind_device(ctx));
    ctx->density_tree_rounds = 0;
    for (float &ms : ctx->density_tree_phase_ms) ms = 0.0f;
    if (n == 0) { *n_edges = 0; *nans = 0; return APD_OK; }
    // tests and measurement only; read at every call, and the answer does not depend on either
    const size_t panel_budget = env_number("APD_DENSITY_TREE_WORKSPACE_BYTES", kPanelBytes);
    unsigned wg = 256;
    const size_t asked = env_number("APD_DENSITY_TREE_WORKGROUP", 0);
    if (asked >= 64 && asked <= 1024 && asked % 64 == 0) wg = (unsigned)asked;

    auto round = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const bool select = min_pts >= 2 && min_pts <= n;                                 // otherwise every core distance is -INF or missing
    const uint32_t capacity = n - 1;
    uint32_t sort_slots = 1;
    while (sort_slots < capacity) sort_slots <<= 1;
    const size_t o_comp = round((size_t)n * 4), o_parent = o_comp + round((size_t)n * 4), o_best = o_parent + round((size_t)n * 4);
    const size_t o_cbest = o_best + round((size_t)n * 8), o_chi = o_cbest + round((size_t)n * 8), o_sort_hi = o_chi + round((size_t)n * 4);
    const size_t o_sort_lo = o_sort_hi + round((size_t)sort_slots * 8), o_count = o_sort_lo + round((size_t)sort_slots * 4);
    const size_t o_nan = o_count + 256, total = o_nan + 256;
    if (const int rc = reserve_ws(ctx, ctx->ws_density_tree, total)) return rc;
    char *ws = ctx->ws_density_tree.as<char>();
    uint32_t *d_ck = reinterpret_cast<uint32_t *>(ws), *d_comp = reinterpret_cast<uint32_t *>(ws + o_comp);
    uint32_t *d_parent = reinterpret_cast<uint32_t *>(ws + o_parent), *d_chi = reinterpret_cast<uint32_t *>(ws + o_chi);
    unsigned long long *d_best = reinterpret_cast<unsigned long long *>(ws + o_best), *d_cbest = reinterpret_cast<unsigned long long *>(ws + o_cbest);
    unsigned long long *d_sort_hi = reinterpret_cast<unsigned long long *>(ws + o_sort_hi), *d_nan = reinterpret_cast<unsigned long long *>(ws + o_nan);
    uint32_t *d_sort_lo = reinterpret_cast<uint32_t *>(ws + o_sort_lo), *d_count = reinterpret_cast<uint32_t *>(ws + o_count);

    const uint64_t panel_stride = std::max<uint64_t>(((uint64_t)n + 3) & ~3ull, 4);
    uint32_t panel_rows = 0;
    if (select) {
        const uint64_t fit = std::max<uint64_t>(panel_budget / (panel_stride * sizeof(float)), 1);   // at least one column is taken
        panel_rows = (uint32_t)std::min<uint64_t>(fit >= 64 ? fit & ~63ull : fit, n);
        if (const int rc = reserve_ws(ctx, ctx->ws_neighbors, (size_t)panel_rows * panel_stride * sizeof(float))) return rc;
    }
    const size_t mat_bytes = (size_t)n * n * sizeof(float), vertex_bytes = (size_t)n * 4, edge_bytes = (size_t)capacity * 4;
    const size_t h_core = round(mat_bytes), h_edge_i = h_core + round(vertex_bytes), h_edge_j = h_edge_i + round(edge_bytes);
    const size_t h_weight = h_edge_j + round(edge_bytes), h_total = h_weight + round(edge_bytes);
    const float *d_mat = distances;
    float *d_core = core, *d_weight = weight;
    uint32_t *d_edge_i = edge_i, *d_edge_j = edge_j;
    if (!on_device) {
        if (const int rc = reserve_ws(ctx, ctx->ws_misc, h_total)) return rc;
        char *hs = ctx->ws_misc.as<char>();
        d_mat = reinterpret_cast<const float *>(hs);
        d_core = reinterpret_cast<float *>(hs + h_core);
        d_edge_i = reinterpret_cast<uint32_t *>(hs + h_edge_i);
        d_edge_j = reinterpret_cast<uint32_t *>(hs + h_edge_j);
        d_weight = reinterpret_cast<float *>(hs + h_weight);
    }
    APD_AFFINITY(ctx, "density tree launch");
    hipEvent_t phase[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EventGuard { hipEvent_t *e; ~EventGuard() { for (int k = 0; k < 4; ++k) if (e[k]) hipEventDestroy(e[k]); } } guard{phase};
    if (ctx->timing) for (hipEvent_t &e : phase) HIP_TRY(ctx, hipEventCreate(&e));
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws_misc.ptr, distances, mat_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ws + o_sort_hi, 0xFF, o_count - o_sort_hi, ctx->stream));   // unused sort slots rank behind every edge
    HIP_TRY(ctx, hipMemsetAsync(ws + o_count, 0, total - o_count, ctx->stream));

    const unsigned vertex_blocks = (unsigned)(((uint64_t)n + wg - 1) / wg);
    const bool both = link == APD_DENSITY_BOTH;
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream)); HIP_TRY(ctx, hipEventRecord(phase[0], ctx->stream)); }
    hipLaunchKernelGGL(tree_init_kernel, dim3(vertex_blocks), dim3(wg), 0, ctx->stream, n, min_pts == 1 ? kMinusInf : kMissing, d_comp, d_ck);
    HIP_TRY(ctx, hipGetLastError());
    if (select) {
        float *panel = ctx->ws_neighbors.as<float>();
        for (uint64_t at = 0; at < n; at += panel_rows) {                             // the stream orders a panel's rows before its refill
            const uint32_t first = (uint32_t)at, part = std::min(panel_rows, n - first);
            HIP_TRY(ctx, launch_column_gather(d_mat, n, n, nullptr, first, part, panel, panel_stride, ctx->stream));
            if (both) hipLaunchKernelGGL(tree_core_kernel<true>, dim3(part), dim3(wg), 0, ctx->stream, d_mat, panel, panel_stride, n, first, min_pts - 2, d_ck);
            else hipLaunchKernelGGL(tree_core_kernel<false>, dim3(part), dim3(wg), 0, ctx->stream, d_mat, panel, panel_stride, n, first, min_pts - 2, d_ck);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(phase[1], ctx->stream));

    // Boruvka: every round at least halves the components that still have an edge, so floor(log2 n) rounds append and one more finds
    // nothing (it is not run once n - 1 edges are there).
    const uint64_t tiles = ((uint64_t)n + 63) / 64, pairs = tiles * (tiles + 1) / 2;   // < 2^31 for n <= kLargest
    const int vec = (n % 4 == 0 && (reinterpret_cast<uintptr_t>(d_mat) & 15u) == 0) ? 1 : 0;
    uint32_t most_rounds = 1;
    while ((1ull << (most_rounds - 1)) < n) ++most_rounds;                            // ceil(log2 n) + 1
    uint32_t edges = 0, rounds = 0;
    while (n >= 2 && edges < capacity) {
        if (rounds == most_rounds) {
            ctx->last_error = "apd_density_tree: the forest did not settle within ceil(log2 n) + 1 rounds";
            return APD_ERR_HIP;
        }
        HIP_TRY(ctx, hipMemsetAsync(ws + o_best, 0xFF, o_sort_hi - o_best, ctx->stream));   // best, cbest, chi: nothing found yet
        unsigned long long *g_nan = rounds == 0 ? d_nan : nullptr;
        if (both) hipLaunchKernelGGL(tree_scan_kernel<true>, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, d_mat, n, vec, d_ck, d_comp, d_best, g_nan);
        else hipLaunchKernelGGL(tree_scan_kernel<false>, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, d_mat, n, vec, d_ck, d_comp, d_best, g_nan);
        HIP_TRY(ctx, hipGetLastError());
        for (int step = 0; step < 2; ++step) {
            hipLaunchKernelGGL(tree_reduce_kernel, dim3(vertex_blocks), dim3(wg), 0, ctx->stream, n, step, d_comp, d_best, d_cbest, d_chi);
            HIP_TRY(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(tree_hook_kernel, dim3(vertex_blocks), dim3(wg), 0, ctx->stream, n, d_comp, d_cbest, d_chi, d_parent, d_count, d_sort_hi,
                           d_sort_lo, capacity);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(tree_jump_kernel, dim3(vertex_blocks), dim3(wg), 0, ctx->stream, n, d_comp, d_parent);
        HIP_TRY(ctx, hipGetLastError());
        ++rounds;
        uint32_t now = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&now, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (now > capacity) { ctx->last_error = "apd_density_tree: more than n - 1 edges appended"; return APD_ERR_HIP; }
        if (now == edges) break;                                                      // no component found an edge
        edges = now;
    }
    ctx->density_tree_rounds = rounds;
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(phase[2], ctx->stream));

    uint32_t count = 1;
    while (count < edges) count <<= 1;
    if (edges > 1) {
        const unsigned chunks = (count + kSortChunk - 1) / kSortChunk, pair_blocks = (count / 2 + 255) / 256;
        hipLaunchKernelGGL(tree_sort_local_kernel, dim3(chunks), dim3(kSortChunk / 2), 0, ctx->stream, d_sort_hi, d_sort_lo, count, 2u,
                           std::min(count, kSortChunk));
        HIP_TRY(ctx, hipGetLastError());
        for (uint32_t k = 2 * kSortChunk; k <= count; k <<= 1) {
            for (uint32_t j = k >> 1; j >= kSortChunk; j >>= 1) {
                hipLaunchKernelGGL(tree_sort_global_kernel, dim3(pair_blocks), dim3(256), 0, ctx->stream, d_sort_hi, d_sort_lo, count, k, j);
                HIP_TRY(ctx, hipGetLastError());
            }
            hipLaunchKernelGGL(tree_sort_local_kernel, dim3(chunks), dim3(kSortChunk / 2), 0, ctx->stream, d_sort_hi, d_sort_lo, count, k, k);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    hipLaunchKernelGGL(tree_finish_kernel, dim3(vertex_blocks), dim3(wg), 0, ctx->stream, n, edges, d_ck, d_sort_hi, d_sort_lo, d_core, d_edge_i,
                       d_edge_j, d_weight);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->timing) {
        HIP_TRY(ctx, hipEventRecord(phase[3], ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->timed = true;
        HIP_TRY(ctx, hipEventSynchronize(phase[3]));
        for (int k = 0; k < 3; ++k) HIP_TRY(ctx, hipEventElapsedTime(&ctx->density_tree_phase_ms[k], phase[k], phase[k + 1]));
    }
    unsigned long long h_nan = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&h_nan, d_nan, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(core, d_core, vertex_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (capacity) {
            HIP_TRY(ctx, hipMemcpyAsync(edge_i, d_edge_i, edge_bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(edge_j, d_edge_j, edge_bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(weight, d_weight, edge_bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_edges = edges;
    *nans = h_nan;
    return APD_OK;
}

extern "C" int apd_density_tree_last_profile(apd_context *ctx, float *phase_ms, uint32_t *rounds)
{
    if (!ctx || !phase_ms || !rounds) return APD_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) phase_ms[k] = ctx->density_tree_phase_ms[k];
    *rounds = ctx->density_tree_rounds;
    return APD_OK;
}

extern "C" int apd_density_tree_cut(uint32_t n, const float *core, const uint32_t *edge_i, const uint32_t *edge_j, const float *weight,
                                    uint32_t n_edges, const float *eps, uint32_t n_eps, uint32_t *labels, uint8_t *kind, uint32_t *counts)
{
    if ((n && !core) || (n_edges && !weight) || (n_eps && (!eps || !counts || (n && !labels)))) return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_eps; ++s) if (eps[s] != eps[s]) return APD_ERR_INVALID_ARG;
    if (!is_forest(n, edge_i, edge_j, n_edges)) return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_eps; ++s) {
        Forest f(n);
        for (uint32_t t = 0; t < n_edges; ++t) if (weight[t] <= eps[s]) f.join(edge_i[t], edge_j[t]);
        uint32_t clusters = 0, cores = 0;
        for (uint32_t v = 0; v < n; ++v) {
            const bool is_core = core[v] <= eps[s];                                   // a missing core distance never is
            const uint32_t root = is_core ? f.find(v) : v;                            // the smallest vertex of the component
            labels[(size_t)s * n + v] = root;
            if (kind) kind[(size_t)s * n + v] = is_core ? APD_DENSITY_CORE : APD_DENSITY_NOISE;
            cores += is_core;
            clusters += is_core && root == v;
        }
        counts[4 * s] = clusters; counts[4 * s + 1] = cores; counts[4 * s + 2] = 0; counts[4 * s + 3] = n - cores;
    }
    return APD_OK;
}

extern "C" int apd_density_tree_operations(uint32_t n, const uint32_t *edge_i, const uint32_t *edge_j, const float *weight, uint32_t n_edges,
                                           apd_cluster_op *ops)
{
    if (n_edges && (!weight || !ops)) return APD_ERR_INVALID_ARG;
    if (!is_forest(n, edge_i, edge_j, n_edges)) return APD_ERR_INVALID_ARG;
    Forest f(n);
    std::vector<uint32_t> id(n);                                                      // the cluster a root stands for
    for (uint32_t v = 0; v < n; ++v) id[v] = v;
    for (uint32_t t = 0; t < n_edges; ++t) {
        const uint32_t p = id[f.find(edge_i[t])], q = id[f.find(edge_j[t])];
        f.join(edge_i[t], edge_j[t]);
        id[f.find(edge_i[t])] = n + t;
        // clustering.rs:193-201
        const uint32_t op = (p < n && q < n) ? APD_SEQUENCE2SEQUENCE : (p >= n && q >= n) ? APD_CLUSTER2CLUSTER
                            : (p >= n) ? APD_CLUSTER2SEQUENCE : APD_SEQUENCE2CLUSTER;
        ops[t] = apd_cluster_op{p, q, n + t, weight[t], op};
    }
    return APD_OK;
}
