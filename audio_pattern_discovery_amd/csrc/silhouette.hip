// Silhouette of cluster assignments over a distance matrix in HBM, any number of assignments ("cuts") per call -- apd_silhouette
// (include/apd.h), DESIGN.md section 4.23.
//
//   silhouette_row_kernel     one workgroup per instance i.  The host has sorted every cut's instances by (label, index) and flattened
//                             all (cut, cluster) pairs into one item table, dealt to the work-items longest first; a work-item walks
//                             whole items: the contract's serial f32 chain over the cluster's members ascending, out of the row staged
//                             in LDS (<true>) or out of HBM (<false>, rows beyond kResidentColumns).  The own cluster's chain gives
//                             a(i); the others' means meet per cut in a 64-bit minimum (ordered mean bits, -0 folded to +0 | the
//                             cluster's rank by label | "the mean is -0"), which is b(i) and nearest(i).  Then a, b, s, nearest.
//   silhouette_score_kernel   one wavefront per cut: the sequential mean of the non-NaN s(i), the NaN count, the cluster count.
//
// The column form gathers the instances' columns into a bounded [panel][n] workspace through the tiled transpose of neighbors.hip
// (launch_column_gather) and runs the same row kernel on the panel's rows.
//
// The answer is a function of the matrix and the labels alone: every chain is walked by one work-item in member order, a minimum does
// not depend on the order of its operands, and its keys are unique per cut (the rank).  How the items are dealt, the workgroup's
// size, the residency limit and the panel cut only move work.
#include <algorithm>
#include <cstdlib>
#include <queue>

#include "apd_internal.h"

using namespace apd;

namespace {

constexpr uint32_t kResidentColumns = 32768;      // rows of up to this many entries stay in LDS: 128 of the CU's 160 KiB
constexpr size_t kWorkspaceBytes = (size_t)256 << 20;   // the column form's panel
constexpr uint32_t kCutsPerLaunch = 1024;         // 16 bytes of LDS per cut beside the row
constexpr uint32_t kLongestRow = 0x7FFFFFF0u;     // a rank and its flag share 32 bits
constexpr uint32_t kNoItem = 0xFFFFFFFFu, kNoLabel = 0xFFFFFFFFu, kNanBits = 0x7FC00000u;
constexpr uint32_t kItemOverhead = 8;             // what an item costs beside its members, in members (the division, the key)

struct RowParams {
    const float *src;          // row 0
    uint64_t stride;           // entries from a row to the next
    uint32_t n;                // instances = entries of a row
    uint32_t first;            // instance of workgroup 0
    uint32_t from_panel;       // 1: row b of src is the instance of workgroup b (column form); 0: the instance names its row
    uint32_t n_cuts;           // of this launch, <= kCutsPerLaunch
    const uint32_t *members;   // [n_cuts][n] instances by (label, index)
    const uint32_t *own_rank;  // [n_cuts][n] rank of the instance's cluster among the cut's labels ascending; top bit: a singleton
    const uint32_t *cut_off;   // [n_cuts + 1] first entry of a cut in cluster_label
    const uint32_t *cluster_label;
    const uint4 *items;        // [steps][work-items] (cut, rank, t0, t1): members[t0 .. t1); cut == kNoItem: none
    uint32_t steps;
    float *s, *a, *b;          // [n_cuts][n]; a, b may be null
    uint32_t *nearest;         // may be null
};

template <bool RESIDENT>
__global__ __launch_bounds__(1024) void silhouette_row_kernel(const RowParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t n = P.n, n_cuts = P.n_cuts, cuts4 = (n_cuts + 3) & ~3u;
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(lds);          // [cuts4]
    float *s_a = reinterpret_cast<float *>(s_key + cuts4);                            // [cuts4] sum / cnt of the own cluster
    uint32_t *s_own = reinterpret_cast<uint32_t *>(s_a + cuts4);                      // [cuts4] own_rank of instance i
    float *row = reinterpret_cast<float *>(s_own + cuts4);                            // RESIDENT: [n]

    const uint32_t i = P.first + blockIdx.x;
    const float *x = P.src + (uint64_t)(P.from_panel ? blockIdx.x : i) * P.stride;
    for (uint32_t c = threadIdx.x; c < n_cuts; c += blockDim.x) {
        s_key[c] = ~0ull;
        s_own[c] = P.own_rank[(uint64_t)c * n + i];
    }
    if (RESIDENT) for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) row[e] = x[e];
    __syncthreads();

    auto entry = [&](uint32_t y) { return RESIDENT ? row[y] : x[y]; };
    // means of one cut arrive in a row (the host orders a work-item's items of equal length by cut): one LDS minimum per stretch
    unsigned long long best = ~0ull;
    uint32_t best_cut = kNoItem;
    for (uint32_t step = 0; step < P.steps; ++step) {
        const uint4 it = P.items[(uint64_t)step * blockDim.x + threadIdx.x];
        if (it.x == kNoItem) continue;
        const uint32_t cut = it.x, rank = it.y, t1 = it.w;
        uint32_t t = it.z;
        float sum = 0.0f;
        auto add = [&](uint32_t y) { if (y != i) sum += entry(y); };                  // the diagonal entry is skipped, not added
        for (; t < t1 && (t & 3u); ++t) add(P.members[t]);
        // A long chain is one work-item's, and nothing hides its latencies for it: 16 members per step, the next step's members
        // loaded before this step's entries are read and added (the adds stay in member order).
        if (t + 16 <= t1) {
            const uint4 *mp = reinterpret_cast<const uint4 *>(P.members + t);
            uint4 m[4] = {mp[0], mp[1], mp[2], mp[3]};
            for (; t + 16 <= t1; t += 16) {
                uint4 nx[4] = {m[0], m[1], m[2], m[3]};
                if (t + 32 <= t1) {
                    mp = reinterpret_cast<const uint4 *>(P.members + t + 16);
                    nx[0] = mp[0]; nx[1] = mp[1]; nx[2] = mp[2]; nx[3] = mp[3];
                }
                uint32_t y[16];
                float v[16];
#pragma unroll
                for (int k = 0; k < 4; ++k) { y[4 * k] = m[k].x; y[4 * k + 1] = m[k].y; y[4 * k + 2] = m[k].z; y[4 * k + 3] = m[k].w; }
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = entry(y[k]);                      // y < n, the diagonal's entry included
#pragma unroll
                for (int k = 0; k < 16; ++k) if (y[k] != i) sum += v[k];
#pragma unroll
                for (int k = 0; k < 4; ++k) m[k] = nx[k];
            }
        }
        for (; t + 4 <= t1; t += 4) {                                                 // the member table starts on 16 bytes
            const uint4 m = *reinterpret_cast<const uint4 *>(P.members + t);
            add(m.x); add(m.y); add(m.z); add(m.w);
        }
        for (; t < t1; ++t) add(P.members[t]);
        const bool own = rank == (s_own[cut] & 0x7FFFFFFFu);
        const uint32_t cnt = it.w - it.z - (own ? 1u : 0u);                           // 0: the own cluster of a singleton
        const float mean = sum / (float)cnt;
        if (own) {
            s_a[cut] = cnt ? mean : 0.0f;                                             // one item per cut is the own one
        } else if (mean < __builtin_inff()) {                                         // strictly below +INF; NaN never is
            const uint32_t bits = __builtin_bit_cast(uint32_t, mean);
            const unsigned long long key = ((unsigned long long)order_key(mean + 0.0f) << 32) | (rank << 1) | (bits == 0x80000000u ? 1u : 0u);
            if (cut != best_cut) {
                if (best != ~0ull) atomicMin(&s_key[best_cut], best);
                best_cut = cut; best = key;
            } else if (key < best) best = key;
        }
    }
    if (best != ~0ull) atomicMin(&s_key[best_cut], best);
    __syncthreads();

    for (uint32_t c = threadIdx.x; c < n_cuts; c += blockDim.x) {
        const unsigned long long key = s_key[c];
        float b = __builtin_inff();
        uint32_t nearest = kNoLabel;
        if (key != ~0ull) {
            const uint32_t o = (uint32_t)(key >> 32), low = (uint32_t)key;
            b = (low & 1u) ? -0.0f : __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
            nearest = P.cluster_label[P.cut_off[c] + (low >> 1)];
        }
        const bool single = (s_own[c] & 0x80000000u) != 0;                            // the host's mark: the own chain is empty
        const float a = s_a[c];
        const float m = (a < b) ? b : a;
        const float s = single ? 0.0f : (b - a) / m;
        const uint64_t at = (uint64_t)c * n + i;
        P.s[at] = s;
        if (P.a) P.a[at] = a;
        if (P.b) P.b[at] = b;
        if (P.nearest) P.nearest[at] = nearest;
    }
}

// score[c] = (((0 + s(i1)) + s(i2)) + ...) / kept over the non-NaN s(i), i ascending: every lane of the wavefront holds the same chain
// (the values go round by readlane), the loads are 64 wide and one step ahead.
__global__ __launch_bounds__(64) void silhouette_score_kernel(const float *__restrict__ s, uint32_t n, const uint32_t *__restrict__ cut_off,
                                                              float *__restrict__ score, uint32_t *__restrict__ clusters,
                                                              uint32_t *__restrict__ nans)
{
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const float *v = s + (uint64_t)c * n;
    float sum = 0.0f;
    uint32_t kept = 0, nan = 0;
    float next = lane < n ? v[lane] : 0.0f;
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
        const float cur = next;
        const uint32_t j1 = j0 + 64;                                                  // n < 2^31
        next = (j1 < n && j1 + lane < n) ? v[j1 + lane] : 0.0f;
        const uint32_t live = n - j0 < 64u ? n - j0 : 64u;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) {
            const float w = __shfl(cur, (int)k);
            if (k < live) {
                if (w == w) { sum += w; ++kept; }
                else ++nan;
            }
        }
    }
    if (lane == 0) {
        score[c] = kept ? sum / (float)kept : __builtin_bit_cast(float, kNanBits);
        clusters[c] = cut_off[c + 1] - cut_off[c];
        nans[c] = nan;
    }
}

size_t env_number(const char *name, size_t fallback)
{
    const char *text = std::getenv(name);
    if (!text || !*text) return fallback;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(text, &end, 10);
    return end && *end == 0 ? (size_t)v : fallback;
}

// What a launch of up to kCutsPerLaunch cuts reads: one upload, every table on a 256-byte boundary.
struct CutPlan {
    uint32_t c0 = 0, cuts = 0, steps = 0;
    size_t o_members = 0, o_rank = 0, o_cut_off = 0, o_label = 0, o_items = 0;       // words into `blob`
    std::vector<uint32_t> blob;
    size_t at = 0;                                                                    // bytes into the call's upload
};

// labels: the cuts [c0, c0 + cuts) of the caller's table.  wg: work-items the items are dealt to.
void plan_cuts(const uint32_t *labels, uint32_t n, uint32_t c0, uint32_t cuts, uint32_t wg, CutPlan &plan)
{
    plan.c0 = c0; plan.cuts = cuts;
    struct Item { uint32_t cut, rank, t0, t1; };
    std::vector<Item> items;
    std::vector<uint32_t> members((size_t)cuts * n), own((size_t)cuts * n), cut_off(cuts + 1, 0), cluster_label;
    std::vector<uint32_t> order(n);
    for (uint32_t c = 0; c < cuts; ++c) {
        const uint32_t *lab = labels + (size_t)(c0 + c) * n;
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [lab](uint32_t p, uint32_t q) { return lab[p] < lab[q]; });   // by (label, index)
        const size_t base = (size_t)c * n;
        for (uint32_t t = 0; t < n;) {
            uint32_t t1 = t;
            while (t1 < n && lab[order[t1]] == lab[order[t]]) ++t1;
            const uint32_t rank = (uint32_t)cluster_label.size() - cut_off[c];
            cluster_label.push_back(lab[order[t]]);
            items.push_back({c, rank, (uint32_t)(base + t), (uint32_t)(base + t1)});
            for (uint32_t u = t; u < t1; ++u) {
                members[base + u] = order[u];
                own[base + order[u]] = rank | (t1 - t == 1 ? 0x80000000u : 0u);       // top bit: a singleton (no a, s = 0)
            }
            t = t1;
        }
        cut_off[c + 1] = (uint32_t)cluster_label.size();
    }
    // longest first, equal lengths cut by cut; each item to the work-item with the least work so far (the lowest one among equals)
    std::stable_sort(items.begin(), items.end(), [](const Item &p, const Item &q) { return p.t1 - p.t0 > q.t1 - q.t0; });
    using Load = std::pair<uint64_t, uint32_t>;
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> lanes;
    for (uint32_t l = 0; l < wg; ++l) lanes.push({0, l});
    std::vector<std::vector<uint32_t>> dealt(wg);
    for (uint32_t k = 0; k < (uint32_t)items.size(); ++k) {
        Load least = lanes.top();
        lanes.pop();
        dealt[least.second].push_back(k);
        least.first += (uint64_t)(items[k].t1 - items[k].t0) + kItemOverhead;
        lanes.push(least);
    }
    size_t steps = 0;
    for (const auto &list : dealt) steps = std::max(steps, list.size());
    plan.steps = (uint32_t)steps;

    auto round = [](size_t words) { return (words + 63) & ~(size_t)63; };
    plan.o_members = 0;
    plan.o_rank = plan.o_members + round(members.size());
    plan.o_cut_off = plan.o_rank + round(own.size());
    plan.o_label = plan.o_cut_off + round(cut_off.size());
    plan.o_items = plan.o_label + round(cluster_label.size());
    plan.blob.assign(plan.o_items + round(steps * wg * 4), kNoItem);                  // an item slot nobody was dealt: cut == kNoItem
    std::copy(members.begin(), members.end(), plan.blob.begin() + plan.o_members);
    std::copy(own.begin(), own.end(), plan.blob.begin() + plan.o_rank);
    std::copy(cut_off.begin(), cut_off.end(), plan.blob.begin() + plan.o_cut_off);
    std::copy(cluster_label.begin(), cluster_label.end(), plan.blob.begin() + plan.o_label);
    for (uint32_t l = 0; l < wg; ++l)
        for (size_t st = 0; st < dealt[l].size(); ++st) {
            const Item &it = items[dealt[l][st]];
            uint32_t *w = plan.blob.data() + plan.o_items + (st * wg + l) * 4;
            w[0] = it.cut; w[1] = it.rank; w[2] = it.t0; w[3] = it.t1;
        }
}

size_t row_lds_bytes(uint32_t cuts, uint32_t n, bool resident)
{
    return (size_t)((cuts + 3) & ~3u) * 16 + (resident ? ((size_t)n * 4 + 15) & ~(size_t)15 : 0);
}

}  // namespace

// Workspaces, owned by the context so that the device form only enqueues: ws_misc [the cuts' tables | s when the caller wants none |
// host form: matrix | s | a | b | nearest | score | clusters | nans], ws_neighbors the column form's panel.
extern "C" int apd_silhouette(apd_context *ctx, const float *distances, int on_device, uint32_t n, int axis, const uint32_t *labels,
                              uint32_t n_cuts, float *score, uint32_t *clusters, uint32_t *nans, float *s, float *a, float *b,
                              uint32_t *nearest)
{
    if (!ctx || n_cuts == 0 || (axis != APD_NEIGHBORS_ROWS && axis != APD_NEIGHBORS_COLUMNS) || !labels || !score || !clusters || !nans ||
        (n && !distances))
        return APD_ERR_INVALID_ARG;
    if (n > kLongestRow) { ctx->last_error = "apd_silhouette: 2^31 instances or more"; return APD_ERR_UNSUPPORTED; }
    HIP_TRY(ctx, bind_device(ctx));
    const bool by_rows = axis == APD_NEIGHBORS_ROWS;
    // tests only; read at every call, and the answer does not depend on any of them
    const uint32_t resident_columns = (uint32_t)std::min<size_t>(env_number("APD_SILHOUETTE_LDS_COLUMNS", kResidentColumns), kResidentColumns);
    const size_t panel_bytes = env_number("APD_SILHOUETTE_WORKSPACE_BYTES", kWorkspaceBytes);
    const bool resident = n <= resident_columns;
    // cuts of one launch: their LDS words beside the row, and a member's place in the launch's table is 32 bits
    const uint32_t per_launch = (uint32_t)std::min<uint64_t>(kCutsPerLaunch, 0xFFFFFFFFull / std::max(n, 1u));
    // as the select of neighbors.hip: 256 work-items where a row is short, 512 while two resident rows fit a compute unit's LDS
    unsigned wg = n <= 8192 ? 256 : (resident && 2 * row_lds_bytes(std::min(n_cuts, per_launch), n, true) <= 160 * 1024 ? 512 : 1024);
    const size_t asked = env_number("APD_SILHOUETTE_WORKGROUP", 0);
    if (asked >= 64 && asked <= 1024 && asked % 64 == 0) wg = (unsigned)asked;

    auto round = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    std::vector<CutPlan> plans((n_cuts + per_launch - 1) / per_launch);
    size_t tables = 0;
    for (size_t p = 0; p < plans.size(); ++p) {
        const uint32_t c0 = (uint32_t)p * per_launch;
        plan_cuts(labels, n, c0, std::min(per_launch, n_cuts - c0), wg, plans[p]);
        plans[p].at = tables;
        tables += round(plans[p].blob.size() * 4);
    }
    const size_t per_sample = round((size_t)n_cuts * n * 4), per_cut = round((size_t)n_cuts * 4);
    const size_t mat_bytes = (size_t)n * n * sizeof(float);
    const bool own_s = !on_device || !s;
    const size_t o_s = tables, o_mat = o_s + (own_s ? per_sample : 0), o_a = o_mat + (on_device ? 0 : round(mat_bytes));
    const size_t o_b = o_a + (!on_device && a ? per_sample : 0), o_nearest = o_b + (!on_device && b ? per_sample : 0);
    const size_t o_score = o_nearest + (!on_device && nearest ? per_sample : 0), o_clusters = o_score + (on_device ? 0 : per_cut);
    const size_t o_nans = o_clusters + (on_device ? 0 : per_cut), total = o_nans + (on_device ? 0 : per_cut);
    if (const int rc = reserve_ws(ctx, ctx->ws_misc, std::max<size_t>(total, 256))) return rc;
    char *ws = ctx->ws_misc.as<char>();
    const uint64_t panel_stride = std::max<uint64_t>(((uint64_t)n + 3) & ~3ull, 4);
    uint32_t panel_cols = 0;
    if (!by_rows && n) {
        const uint64_t fit = std::max<uint64_t>(panel_bytes / (panel_stride * sizeof(float)), 1);
        panel_cols = (uint32_t)std::min<uint64_t>(fit >= 64 ? fit & ~63ull : fit, n);
        if (const int rc = reserve_ws(ctx, ctx->ws_neighbors, (size_t)panel_cols * panel_stride * sizeof(float))) return rc;
    }
    const size_t lds_most = row_lds_bytes(std::min(n_cuts, per_launch), n, resident);
    if (lds_most > 64 * 1024) {
        const void *fn = resident ? reinterpret_cast<const void *>(silhouette_row_kernel<true>)
                                  : reinterpret_cast<const void *>(silhouette_row_kernel<false>);
        HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_most));
    }
    APD_AFFINITY(ctx, "silhouette launch");
    for (const CutPlan &plan : plans)
        HIP_TRY(ctx, hipMemcpyAsync(ws + plan.at, plan.blob.data(), plan.blob.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!on_device && mat_bytes) HIP_TRY(ctx, hipMemcpyAsync(ws + o_mat, distances, mat_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (on_device) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                   // the tables have left the host

    const float *d_mat = on_device ? distances : reinterpret_cast<const float *>(ws + o_mat);
    float *d_s = own_s ? reinterpret_cast<float *>(ws + o_s) : s;
    float *d_a = on_device ? a : (a ? reinterpret_cast<float *>(ws + o_a) : nullptr);
    float *d_b = on_device ? b : (b ? reinterpret_cast<float *>(ws + o_b) : nullptr);
    uint32_t *d_nearest = on_device ? nearest : (nearest ? reinterpret_cast<uint32_t *>(ws + o_nearest) : nullptr);
    float *d_score = on_device ? score : reinterpret_cast<float *>(ws + o_score);
    uint32_t *d_clusters = on_device ? clusters : reinterpret_cast<uint32_t *>(ws + o_clusters);
    uint32_t *d_nans = on_device ? nans : reinterpret_cast<uint32_t *>(ws + o_nans);

    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (const CutPlan &plan : plans) {
        const uint32_t *tab = reinterpret_cast<const uint32_t *>(ws + plan.at);
        const size_t out = (size_t)plan.c0 * n;
        RowParams R{};
        R.n = n; R.n_cuts = plan.cuts; R.steps = plan.steps;
        R.members = tab + plan.o_members; R.own_rank = tab + plan.o_rank; R.cut_off = tab + plan.o_cut_off;
        R.cluster_label = tab + plan.o_label; R.items = reinterpret_cast<const uint4 *>(tab + plan.o_items);
        R.s = d_s + out; R.a = d_a ? d_a + out : nullptr; R.b = d_b ? d_b + out : nullptr; R.nearest = d_nearest ? d_nearest + out : nullptr;
        const size_t lds = row_lds_bytes(plan.cuts, n, resident);
        auto rows_of = [&](uint32_t first, uint32_t count) {
            for (uint32_t done = 0; done < count;) {                                  // (a grid holds 2^31 - 1 workgroups)
                const uint32_t part = std::min<uint32_t>(count - done, 1u << 30);
                RowParams L = R;
                L.first = first + done;
                if (R.from_panel) L.src = R.src + (uint64_t)done * R.stride;
                if (resident) hipLaunchKernelGGL(silhouette_row_kernel<true>, dim3(part), dim3(wg), lds, ctx->stream, L);
                else hipLaunchKernelGGL(silhouette_row_kernel<false>, dim3(part), dim3(wg), lds, ctx->stream, L);
                if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
                done += part;
            }
            return hipSuccess;
        };
        if (by_rows) {
            R.src = d_mat; R.stride = n; R.from_panel = 0;
            if (n) HIP_TRY(ctx, rows_of(0, n));
        } else {
            float *panel = ctx->ws_neighbors.as<float>();
            R.src = panel; R.stride = panel_stride; R.from_panel = 1;
            for (uint64_t at = 0; at < n; at += panel_cols) {                         // the stream orders a panel's rows before its refill
                const uint32_t first = (uint32_t)at, part = std::min(panel_cols, n - first);
                HIP_TRY(ctx, launch_column_gather(d_mat, n, n, nullptr, first, part, panel, panel_stride, ctx->stream));
                HIP_TRY(ctx, rows_of(first, part));
            }
        }
        hipLaunchKernelGGL(silhouette_score_kernel, dim3(plan.cuts), dim3(64), 0, ctx->stream, R.s, n, R.cut_off, d_score + plan.c0,
                           d_clusters + plan.c0, d_nans + plan.c0);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    if (on_device) return APD_OK;
    const size_t sample_bytes = (size_t)n_cuts * n * 4, cut_bytes = (size_t)n_cuts * 4;
    if (s && sample_bytes) HIP_TRY(ctx, hipMemcpyAsync(s, d_s, sample_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (a && sample_bytes) HIP_TRY(ctx, hipMemcpyAsync(a, d_a, sample_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (b && sample_bytes) HIP_TRY(ctx, hipMemcpyAsync(b, d_b, sample_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (nearest && sample_bytes) HIP_TRY(ctx, hipMemcpyAsync(nearest, d_nearest, sample_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(score, d_score, cut_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(clusters, d_clusters, cut_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(nans, d_nans, cut_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}
