// C ABI of libapd_hip.so (include/apd.h): subsequence alignment over pair lists -- curves and bests, detection, the warping paths
// of spotted windows.  The host side around dtw_spot.hip, dtw_spot_detect.hip and dtw_spot_path.hip.
#include <cstring>
#include <map>
#include <new>
#include <tuple>

#include "apd_host.h"

using namespace apd;

extern "C" int apd_spot(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                        float *cost, uint32_t *start, uint64_t capacity, uint64_t *curve_off, apd_spot_best *best)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !curve_off || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if ((cost == nullptr) != (start == nullptr)) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    const ResidentIndex idx(batch);
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    curve_off[0] = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) curve_off[p + 1] = curve_off[p] + idx.len(pairs[2 * p + 1]);
    const bool curves = cost != nullptr;
    if (!curves && !best) return APD_OK;                                  // sizes only
    if (curves && capacity < curve_off[n_pairs]) return APD_ERR_INVALID_ARG;
    if (n_pairs == 0) return APD_OK;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if ((rc = spot_check_lengths(ctx, "apd_spot", idx.len(pairs[2 * p]), idx.len(pairs[2 * p + 1])))) return rc;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot launch");
    ChunkBudget budget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch};
    std::vector<apd_spot_best> best_sink;
    if (!best) best_sink.resize(n_pairs);
    apd_spot_best *h_best = best ? best : best_sink.data();
    std::vector<SpotPair> desc;
    for (uint64_t first = 0; first < n_pairs;) {
        // the chunk [first, last): at least one pair, then as many as keep the curves under the cap (best only: nothing is stored)
        uint64_t last = first;
        budget.reset();
        while (last < n_pairs && budget.admit(curves ? (curve_off[last + 1] - curve_off[last]) * (sizeof(float) + sizeof(uint32_t)) : 0)) ++last;
        const uint64_t np = last - first;
        // the chunk's descriptors, grouped by kernel class (one launch each); `out` keeps the input order
        SpotClasses classes;
        for (uint64_t p = first; p < last; ++p) classes.add(batch->dim, idx.len(pairs[2 * p]));
        classes.close();
        desc.resize(np);
        for (uint64_t p = first; p < last; ++p)
            desc[classes.slot(spot_row_class(batch->dim, idx.len(pairs[2 * p])))] =
                SpotPair{idx.pos[pairs[2 * p]], idx.pos[pairs[2 * p + 1]], (uint32_t)(p - first), 0, curve_off[p] - curve_off[first]};
        const size_t curve_floats = curves ? (size_t)(curve_off[last] - curve_off[first]) : 0;
        Carve ws;
        const size_t o_cost = ws.take<float>(curve_floats), o_start = ws.take<uint32_t>(curve_floats);
        const size_t o_desc = ws.take<SpotPair>(np), o_best = ws.take<apd_spot_best>(np);
        rc = reserve_ws(ctx, ctx->ws_spot, ws.size);
        if (rc) return rc;
        char *base = ctx->ws_spot.as<char>();
        SpotLaunch L{};
        L.src = spot_source(batch, cfg->insertion_penalty, cfg->deletion_penalty, cfg->match_penalty);
        L.d_cost = curves ? (float *)(base + o_cost) : nullptr;
        L.d_start = curves ? (uint32_t *)(base + o_start) : nullptr;
        const SpotPair *d_desc = (const SpotPair *)(base + o_desc);
        L.d_best = (apd_spot_best *)(base + o_best);
        HIP_TRY(ctx, hipMemcpyAsync((void *)d_desc, desc.data(), (size_t)np * sizeof(SpotPair), hipMemcpyHostToDevice, ctx->stream));
        if (ctx->timing && first == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (uint32_t c = 0; c < kSpotClasses; ++c) {
            L.d_pairs = d_desc + classes.first[c];
            L.n_pairs = (uint32_t)classes.n[c];
            HIP_TRY(ctx, launch_spot(L, c, classes.r_max, ctx->stream));
        }
        if (ctx->timing && last == n_pairs) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (curve_floats) {
            HIP_TRY(ctx, hipMemcpyAsync(cost + curve_off[first], L.d_cost, curve_floats * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(start + curve_off[first], L.d_start, curve_floats * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpyAsync(h_best + first, L.d_best, (size_t)np * sizeof(apd_spot_best), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `desc`)
        first = last;
    }
    return APD_OK;
}

// score(j) of the spotting contract: one f32 division, the window's length in place of m (alignments.rs:121)
static float spot_score(float cost, uint64_t j, uint32_t start, uint64_t n)
{
    return cost / (float)(n + (j - start + 1));
}

extern "C" int apd_spot_hits(const float *cost, const uint32_t *start, uint64_t m, uint64_t n, float threshold, apd_spot_best *hits,
                             uint64_t capacity, uint64_t *n_hits)
{
    if (!n_hits || n == 0 || (m && (!cost || !start)) || (capacity && !hits)) return APD_ERR_INVALID_ARG;
    *n_hits = 0;
    try {
        std::vector<std::pair<float, uint64_t>> cand;                     // (score, end), ends ascending
        for (uint64_t j = 1; j <= m; ++j) {
            if (start[j - 1] > j) return APD_ERR_INVALID_ARG;             // not a curve of apd_spot
            const float s = spot_score(cost[j - 1], j, start[j - 1], n);
            if (s < threshold) cand.emplace_back(s, j);                   // strict; NaN compares false
        }
        std::stable_sort(cand.begin(), cand.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        std::map<uint64_t, uint64_t> taken;                               // accepted windows, first column -> last column (disjoint)
        for (const auto &c : cand) {
            const uint64_t hi = c.second, lo = start[hi - 1];
            auto next = taken.upper_bound(hi);                            // the first accepted window that begins after `hi`
            if (next != taken.begin() && std::prev(next)->second >= lo) continue;   // the one before it reaches into [lo, hi]
            taken.emplace(lo, hi);
            if (*n_hits < capacity) {
                apd_spot_best &h = hits[*n_hits];
                h.end = (uint32_t)hi; h.start = (uint32_t)lo; h.cost = cost[hi - 1]; h.score = c.first;
            }
            ++*n_hits;
        }
    } catch (const std::bad_alloc &) {
        return APD_ERR_OOM;
    }
    return APD_OK;
}

// ----------------------------------------------------------------------------------------- spot detection

// apd_spot's sweep into the workspace, then candidates, greedy picking and the packed hits on the device (kernels:
// dtw_spot_detect.hip).  A chunk is a run of whole groups; its pairs are numbered group by group.  ws_spot_hits: the chunk's packed
// hits, sized once its hit counts are known.
extern "C" int apd_spot_detect(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                               const float *thresholds, int compete, apd_spot_hit *hits, uint64_t capacity, uint64_t *hit_off,
                               uint64_t *n_groups, uint64_t *n_hits)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if ((compete != APD_DETECT_PER_PAIR && compete != APD_DETECT_PER_STREAM) || (n_pairs && !thresholds) || !hit_off || !n_groups || !n_hits ||
        (capacity && !hits))
        return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    const ResidentIndex idx(batch);
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    *n_groups = 0;
    *n_hits = 0;
    hit_off[0] = 0;
    if (n_pairs == 0) return APD_OK;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if ((rc = spot_check_lengths(ctx, "apd_spot_detect", idx.len(pairs[2 * p]), idx.len(pairs[2 * p + 1])))) return rc;
    // groups in order of first appearance; members[member_first[g] .. member_first[g + 1]): the group's pairs, ascending
    std::vector<uint64_t> group_of(n_pairs);
    uint64_t ng = n_pairs;
    if (compete == APD_DETECT_PER_PAIR)
        for (uint64_t p = 0; p < n_pairs; ++p) group_of[p] = p;
    else
        ng = number_by_first_appearance(pairs + 1, 2, n_pairs, n_seq, group_of);
    GroupMembers groups;
    if (!groups.build(group_of, ng, kMaxPairsPerLaunch)) {
        ctx->last_error = "apd_spot_detect: a group of more than 2^24 pairs";
        return APD_ERR_UNSUPPORTED;
    }
    const std::vector<uint64_t> &member_first = groups.first, &members = groups.members;
    auto stream_len = [&](uint64_t g) { return (uint64_t)idx.len(pairs[2 * members[member_first[g]] + 1]); };
    auto group_pairs = [&](uint64_t g) { return groups.size(g); };
    *n_groups = ng;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot detect launch");
    ChunkBudget budget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch};
    constexpr uint64_t kEntryBytes = sizeof(float) + sizeof(uint32_t) + sizeof(ulonglong2), kStageBytes = sizeof(uint2);
    std::vector<char> upload;
    std::vector<uint32_t> counts;
    for (uint64_t g0 = 0; g0 < ng;) {
        // the chunk of groups [g0, g1): at least one, then as many as keep the curves, the candidates and the windows under the cap
        uint64_t g1 = g0, entries = 0, stage_slots = 0;
        budget.reset();
        while (g1 < ng && budget.admit(group_pairs(g1) * stream_len(g1) * kEntryBytes + stream_len(g1) * kStageBytes, 0, group_pairs(g1))) {
            entries += group_pairs(g1) * stream_len(g1); stage_slots += stream_len(g1);
            ++g1;
        }
        const uint64_t ngc = g1 - g0, np = budget.items;
        // ws_spot: the curves, the candidates and the accepted windows; what is uploaded -- the sweep's pairs by kernel class, the
        // detector's pairs and groups --; the bests; what is zeroed -- candidate and hit counts --; the hit bases
        Carve ws;
        const size_t o_cost = ws.take<float>(entries), o_start = ws.take<uint32_t>(entries);
        const size_t o_cand = ws.take<ulonglong2>(entries), o_stage = ws.take<uint2>(stage_slots);
        const size_t o_desc = ws.take<SpotPair>(np), o_dp = ws.take<SpotDetectPair>(np), o_grp = ws.take<SpotDetectGroup>(ngc);
        const size_t o_best = ws.take<apd_spot_best>(np);
        const size_t o_cc = ws.take<unsigned long long>(ngc), o_hc = ws.take<uint32_t>(ngc), o_hb = ws.take<unsigned long long>(ngc + 1);
        upload.assign(o_best - o_desc, 0);
        SpotPair *desc = (SpotPair *)upload.data();
        SpotDetectPair *dp = (SpotDetectPair *)(upload.data() + (o_dp - o_desc));
        SpotDetectGroup *grp = (SpotDetectGroup *)(upload.data() + (o_grp - o_desc));
        SpotClasses classes;
        uint32_t m_max = 1;
        uint64_t k = 0, off = 0, stage_off = 0;
        for (uint64_t g = g0; g < g1; ++g) {
            SpotDetectGroup &G = grp[g - g0];
            const uint32_t m = (uint32_t)stream_len(g);
            G.cand_off = off; G.cand_cap = group_pairs(g) * m; G.stage_off = stage_off; G.stage_cap = m;
            stage_off += m;
            m_max = std::max(m_max, m);
            for (uint64_t t = member_first[g]; t < member_first[g + 1]; ++t, ++k) {
                const uint64_t p = members[t];
                SpotDetectPair &d = dp[k];
                d.curve_off = off; d.m = m; d.n = idx.len(pairs[2 * p]); d.threshold = thresholds[p];
                d.group = (uint32_t)(g - g0); d.pair = (uint32_t)p;
                off += m;
                classes.add(batch->dim, d.n);
            }
        }
        classes.close();
        for (k = 0; k < np; ++k) {
            const uint64_t p = dp[k].pair;
            desc[classes.slot(spot_row_class(batch->dim, dp[k].n))] = SpotPair{idx.pos[pairs[2 * p]], idx.pos[pairs[2 * p + 1]], (uint32_t)k, 0, dp[k].curve_off};
        }
        rc = reserve_ws(ctx, ctx->ws_spot, ws.size);
        if (rc) return rc;
        char *base = ctx->ws_spot.as<char>();
        SpotLaunch L{};
        L.src = spot_source(batch, cfg->insertion_penalty, cfg->deletion_penalty, cfg->match_penalty);
        L.d_cost = (float *)(base + o_cost);
        L.d_start = (uint32_t *)(base + o_start);
        const SpotPair *d_desc = (const SpotPair *)(base + o_desc);
        L.d_best = (apd_spot_best *)(base + o_best);
        SpotDetectLaunch D{};
        D.d_cost = L.d_cost; D.d_start = L.d_start;
        D.d_pairs = (const SpotDetectPair *)(base + o_dp); D.n_pairs = (uint32_t)np;
        D.d_groups = (const SpotDetectGroup *)(base + o_grp); D.n_groups = (uint32_t)ngc;
        D.d_cand = (ulonglong2 *)(base + o_cand);
        D.d_stage = (uint2 *)(base + o_stage);
        D.d_cand_count = (unsigned long long *)(base + o_cc);
        D.d_hit_count = (uint32_t *)(base + o_hc);
        D.d_hit_base = (unsigned long long *)(base + o_hb);
        HIP_TRY(ctx, hipMemcpyAsync(base + o_desc, upload.data(), upload.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(base + o_cc, 0, o_hb - o_cc, ctx->stream));
        if (ctx->timing && g0 == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (uint32_t c = 0; c < kSpotClasses; ++c) {
            L.d_pairs = d_desc + classes.first[c];
            L.n_pairs = (uint32_t)classes.n[c];
            HIP_TRY(ctx, launch_spot(L, c, classes.r_max, ctx->stream));
        }
        HIP_TRY(ctx, launch_spot_detect(D, m_max, ctx->stream));
        counts.resize(ngc);
        HIP_TRY(ctx, hipMemcpyAsync(counts.data(), D.d_hit_count, (size_t)ngc * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the packed buffer is sized by the counts
        const uint64_t chunk_first = hit_off[g0];
        for (uint64_t g = g0; g < g1; ++g) hit_off[g + 1] = hit_off[g] + counts[g - g0];
        const uint64_t chunk_hits = hit_off[g1] - chunk_first;
        const uint64_t n_write = capacity > chunk_first ? std::min(chunk_hits, capacity - chunk_first) : 0;
        if (n_write) {
            rc = reserve_ws(ctx, ctx->ws_spot_hits, (size_t)n_write * sizeof(apd_spot_hit));
            if (rc) return rc;
            HIP_TRY(ctx, launch_spot_detect_emit(D, ctx->ws_spot_hits.as<apd_spot_hit>(), n_write, ctx->stream));
        }
        if (ctx->timing && g1 == ng) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (n_write) {
            HIP_TRY(ctx, hipMemcpyAsync(hits + chunk_first, ctx->ws_spot_hits.ptr, (size_t)n_write * sizeof(apd_spot_hit), hipMemcpyDeviceToHost,
                                        ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `upload`)
        g0 = g1;
    }
    *n_hits = hit_off[ng];
    return APD_OK;
}

// ----------------------------------------------------------------------------------- spot score quantiles

// apd_spot's sweep into the workspace, then the radix select of every (group, quantile) on the device (kernels:
// dtw_spot_quantile.hip).  A chunk is a run of whole groups; its pairs are numbered group by group.  The rank k of every (group,
// quantile) is worked out here from the group's entries and uploaded with its state record.
extern "C" int apd_spot_quantiles(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                                  int grouping, const float *perc, uint32_t n_perc, float *values, int32_t *status, uint64_t *group_of_out,
                                  uint64_t *entries_out, uint64_t *nans_out, uint64_t *n_groups)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if (grouping < APD_QUANTILES_PER_PAIR || grouping > APD_QUANTILES_ALL || n_perc == 0 || n_perc > APD_SPOT_QUANTILES_MAX || !perc || !values ||
        !n_groups)
        return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    const ResidentIndex idx(batch);
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    if (n_pairs == 0) { *n_groups = 0; return APD_OK; }
    for (uint64_t p = 0; p < n_pairs; ++p)
        if ((rc = spot_check_lengths(ctx, "apd_spot_quantiles", idx.len(pairs[2 * p]), idx.len(pairs[2 * p + 1])))) return rc;
    // groups in order of first appearance; members[member_first[g] .. member_first[g + 1]): the group's pairs, ascending
    std::vector<uint64_t> group_of(n_pairs, 0);                           // APD_QUANTILES_ALL: every pair in group 0
    uint64_t ng = 1;
    if (grouping == APD_QUANTILES_PER_PAIR) {
        ng = n_pairs;
        for (uint64_t p = 0; p < n_pairs; ++p) group_of[p] = p;
    } else if (grouping == APD_QUANTILES_PER_QUERY) {
        ng = number_by_first_appearance(pairs, 2, n_pairs, n_seq, group_of);
    }
    GroupMembers groups;
    if (!groups.build(group_of, ng, kMaxPairsPerLaunch)) {
        ctx->last_error = "apd_spot_quantiles: a group of more than 2^24 pairs";
        return APD_ERR_UNSUPPORTED;
    }
    const std::vector<uint64_t> &member_first = groups.first, &members = groups.members;
    std::vector<uint64_t> group_entries(ng, 0);
    for (uint64_t p = 0; p < n_pairs; ++p) group_entries[group_of[p]] += idx.len(pairs[2 * p + 1]);
    auto group_pairs = [&](uint64_t g) { return groups.size(g); };
    *n_groups = ng;
    if (group_of_out) std::copy(group_of.begin(), group_of.end(), group_of_out);
    if (entries_out) std::copy(group_entries.begin(), group_entries.end(), entries_out);
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot quantiles launch");
    ChunkBudget budget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch};
    constexpr uint64_t kEntryBytes = sizeof(float) + sizeof(uint32_t);
    constexpr uint64_t kPairBytes = sizeof(SpotPair) + sizeof(SpotQuantilePair) + sizeof(apd_spot_best);
    const uint64_t group_bytes = (uint64_t)n_perc * (kSpotQuantileBins * sizeof(unsigned long long) + sizeof(SpotQuantileState) + 8);
    std::vector<char> upload, results;
    std::vector<uint64_t> slot_pair;                                      // the caller's pair of every pair of the chunk
    for (uint64_t g0 = 0; g0 < ng;) {
        // the chunk of groups [g0, g1): at least one, then as many as keep the curves, the pairs' records and the histograms under the cap
        uint64_t g1 = g0, entries = 0;
        budget.reset();
        while (g1 < ng && budget.admit(group_entries[g1] * kEntryBytes + group_pairs(g1) * kPairBytes + group_bytes, 0, group_pairs(g1))) entries += group_entries[g1++];
        const uint64_t ngc = g1 - g0, np = budget.items, nq = n_perc;
        // ws_spot: the curves; what is uploaded -- the sweep's pairs by kernel class, the select's pairs, the states --; the bests; what
        // is zeroed -- the histograms --; what is read back -- values, statuses, NaN counts
        Carve ws;
        const size_t o_cost = ws.take<float>(entries), o_start = ws.take<uint32_t>(entries);
        const size_t o_desc = ws.take<SpotPair>(np), o_qp = ws.take<SpotQuantilePair>(np), o_state = ws.take<SpotQuantileState>(ngc * nq);
        const size_t o_best = ws.take<apd_spot_best>(np);
        const size_t o_hist = ws.take<unsigned long long>(ngc * nq * kSpotQuantileBins);
        const size_t o_values = ws.take<float>(ngc * nq), o_status = ws.take<int32_t>(ngc * nq), o_nans = ws.take<unsigned long long>(ngc);
        upload.assign(o_best - o_desc, 0);
        SpotPair *desc = (SpotPair *)upload.data();
        SpotQuantilePair *qp = (SpotQuantilePair *)(upload.data() + (o_qp - o_desc));
        SpotQuantileState *state = (SpotQuantileState *)(upload.data() + (o_state - o_desc));
        slot_pair.resize(np);
        SpotClasses classes;
        uint32_t m_max = 1;
        uint64_t k = 0, off = 0;
        for (uint64_t g = g0; g < g1; ++g) {
            for (uint32_t q = 0; q < n_perc; ++q) state[(g - g0) * nq + q].rank = percentile_index(group_entries[g], perc[q]);
            for (uint64_t t = member_first[g]; t < member_first[g + 1]; ++t, ++k) {
                const uint64_t p = members[t];
                SpotQuantilePair &d = qp[k];
                d.curve_off = off; d.m = idx.len(pairs[2 * p + 1]); d.n = idx.len(pairs[2 * p]); d.group = (uint32_t)(g - g0);
                slot_pair[k] = p;
                off += d.m;
                m_max = std::max(m_max, d.m);
                classes.add(batch->dim, d.n);
            }
        }
        classes.close();
        for (k = 0; k < np; ++k) {
            const uint64_t p = slot_pair[k];
            desc[classes.slot(spot_row_class(batch->dim, qp[k].n))] = SpotPair{idx.pos[pairs[2 * p]], idx.pos[pairs[2 * p + 1]], (uint32_t)k, 0, qp[k].curve_off};
        }
        rc = reserve_ws(ctx, ctx->ws_spot, ws.size);
        if (rc) return rc;
        char *base = ctx->ws_spot.as<char>();
        SpotLaunch L{};
        L.src = spot_source(batch, cfg->insertion_penalty, cfg->deletion_penalty, cfg->match_penalty);
        L.d_cost = (float *)(base + o_cost);
        L.d_start = (uint32_t *)(base + o_start);
        const SpotPair *d_desc = (const SpotPair *)(base + o_desc);
        L.d_best = (apd_spot_best *)(base + o_best);
        SpotQuantileLaunch Q{};
        Q.d_cost = L.d_cost; Q.d_start = L.d_start;
        Q.d_pairs = (const SpotQuantilePair *)(base + o_qp); Q.n_pairs = (uint32_t)np;
        Q.n_groups = (uint32_t)ngc; Q.n_perc = n_perc;
        Q.d_state = (SpotQuantileState *)(base + o_state);
        Q.d_hist = (unsigned long long *)(base + o_hist);
        Q.d_values = (float *)(base + o_values);
        Q.d_status = (int32_t *)(base + o_status);
        Q.d_nans = (unsigned long long *)(base + o_nans);
        HIP_TRY(ctx, hipMemcpyAsync(base + o_desc, upload.data(), upload.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(base + o_hist, 0, o_values - o_hist, ctx->stream));
        if (ctx->timing && g0 == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (uint32_t c = 0; c < kSpotClasses; ++c) {
            L.d_pairs = d_desc + classes.first[c];
            L.n_pairs = (uint32_t)classes.n[c];
            HIP_TRY(ctx, launch_spot(L, c, classes.r_max, ctx->stream));
        }
        HIP_TRY(ctx, launch_spot_quantiles(Q, m_max, ctx->stream));
        if (ctx->timing && g1 == ng) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        results.resize(ws.size - o_values);
        HIP_TRY(ctx, hipMemcpyAsync(results.data(), base + o_values, results.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `upload`)
        std::memcpy(values + g0 * nq, results.data(), (size_t)(ngc * nq) * sizeof(float));
        if (status) std::memcpy(status + g0 * nq, results.data() + (o_status - o_values), (size_t)(ngc * nq) * sizeof(int32_t));
        if (nans_out) std::memcpy(nans_out + g0, results.data() + (o_nans - o_values), (size_t)ngc * sizeof(uint64_t));
        g0 = g1;
    }
    return APD_OK;
}

// ------------------------------------------------------------------- warping paths of spotted windows

extern "C" uint64_t apd_spot_path_bound(uint64_t n, uint64_t end, uint64_t start)
{
    return (n == 0 || start == 0 || start > end) ? 0 : n + (end - start + 1);
}

// The windows are taken in input order, a chunk at a time: as many as keep the direction words (counted per window, before the
// merge makes them fewer) and the steps under the workspace cap, at least one.  Inside a chunk the windows are grouped by (query,
// stream) pair: one sweep per pair over the union of its windows' columns, one trace per window (kernels: dtw_spot_path.hip).
extern "C" int apd_spot_paths(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const apd_spot_window *windows,
                              uint64_t n_windows, apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len,
                              uint32_t *found_start, float *scores)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !step_off || (n_windows && !windows)) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    const ResidentIndex idx(batch);
    for (uint64_t p = 0; p < n_windows; ++p)
        if (windows[p].x >= n_seq || windows[p].y >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    for (uint64_t p = 0; p < n_windows; ++p) {
        const apd_spot_window &w = windows[p];
        if (w.end > idx.len(w.y) || (w.end && w.start > w.end)) return APD_ERR_INVALID_ARG;
    }
    step_off[0] = 0;
    for (uint64_t p = 0; p < n_windows; ++p)
        step_off[p + 1] = step_off[p] + apd_spot_path_bound(idx.len(windows[p].x), windows[p].end, windows[p].start);
    if (!steps) return APD_OK;                                            // sizes only
    if (capacity < step_off[n_windows] || (n_windows && !path_len)) return APD_ERR_INVALID_ARG;
    if (n_windows == 0) return APD_OK;
    for (uint64_t p = 0; p < n_windows; ++p)
        if ((rc = spot_check_lengths(ctx, "apd_spot_paths", idx.len(windows[p].x), idx.len(windows[p].y)))) return rc;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot path launch");
    ChunkBudget budget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch};
    WindowResults results{path_len, found_start, scores};
    std::vector<uint64_t> &live = results.live;                           // the chunk's windows that own slots, input order
    std::vector<uint64_t> by_pair;                                        // the same, grouped by pair, starts ascending
    std::vector<SpotRecPair> rec_pairs;                                   // in by_pair's order, and each one's kernel class
    std::vector<uint32_t> rec_class;
    std::vector<SpotInterval> intervals;
    std::vector<uint32_t> ends;
    std::vector<SpotTraceWindow> trace;
    std::vector<char> upload;
    bool first_launch = true;
    for (uint64_t first = 0; first < n_windows;) {
        uint64_t last = first;
        budget.reset();
        for (; last < n_windows; ++last) {
            const apd_spot_window &w = windows[last];
            const uint64_t slots = step_off[last + 1] - step_off[last];
            const uint64_t est_words = slots ? spot_dir_words(idx.len(w.x), (uint64_t)w.end - w.start + 1) : 0;
            if (!budget.admit(est_words * sizeof(uint32_t), slots * sizeof(apd_path_step))) break;
        }
        live.clear();
        for (uint64_t p = first; p < last; ++p) {
            if (step_off[p + 1] > step_off[p]) live.push_back(p);
            else results.dead(p);                                         // no window: nothing to sweep
        }
        if (live.empty()) { first = last; continue; }
        // ---- the plan: per pair its merged intervals and its distinct ends; per window its interval and its end's slot
        by_pair = live;
        std::sort(by_pair.begin(), by_pair.end(), [&](uint64_t a, uint64_t b) {
            const apd_spot_window &u = windows[a], &v = windows[b];
            return std::make_tuple(u.x, u.y, u.start, u.end, a) < std::make_tuple(v.x, v.y, v.start, v.end, b);
        });
        rec_pairs.clear(); rec_class.clear();
        intervals.clear(); ends.clear();
        trace.assign(live.size(), SpotTraceWindow{});
        SpotClasses classes;
        uint64_t words = 0;
        for (size_t g = 0; g < by_pair.size();) {
            size_t g_end = g;
            const apd_spot_window &head = windows[by_pair[g]];
            while (g_end < by_pair.size() && windows[by_pair[g_end]].x == head.x && windows[by_pair[g_end]].y == head.y) ++g_end;
            const uint32_t n = idx.len(head.x);
            SpotRecPair rp{};
            rp.px = idx.pos[head.x]; rp.py = idx.pos[head.y];
            rp.iv_first = (uint32_t)intervals.size(); rp.end_first = (uint32_t)ends.size();
            for (size_t t = g; t < g_end; ++t) {
                const apd_spot_window &w = windows[by_pair[t]];
                if (intervals.size() > rp.iv_first && (uint64_t)w.start <= (uint64_t)intervals.back().b + 1)
                    intervals.back().b = std::max(intervals.back().b, w.end);   // overlapping or touching: one interval
                else
                    intervals.push_back(SpotInterval{w.start, w.end, 0});
                ends.push_back(w.end);
                rp.max_end = std::max(rp.max_end, w.end);
            }
            std::sort(ends.begin() + rp.end_first, ends.end());
            ends.erase(std::unique(ends.begin() + rp.end_first, ends.end()), ends.end());
            rp.n_iv = (uint32_t)intervals.size() - rp.iv_first; rp.n_ends = (uint32_t)ends.size() - rp.end_first;
            for (uint32_t k = rp.iv_first; k < intervals.size(); ++k) {
                intervals[k].off = words;
                words += spot_dir_words(n, (uint64_t)intervals[k].b - intervals[k].a + 1);
            }
            for (size_t t = g; t < g_end; ++t) {
                const uint64_t p = by_pair[t];
                const apd_spot_window &w = windows[p];
                SpotTraceWindow &tw = trace[std::lower_bound(live.begin(), live.end(), p) - live.begin()];
                uint32_t k = rp.iv_first;
                while (intervals[k].b < w.end) ++k;                       // the interval that holds [start, end]
                tw.px = rp.px; tw.py = rp.py; tw.end = w.end; tw.start = w.start;
                tw.a = intervals[k].a; tw.dir_off = intervals[k].off;
                tw.end_slot = (uint32_t)(std::lower_bound(ends.begin() + rp.end_first, ends.end(), w.end) - ends.begin());
                tw.step_off = step_off[p] - step_off[first];
            }
            rec_pairs.push_back(rp);
            rec_class.push_back(classes.add(batch->dim, n));
            g = g_end;
        }
        classes.close();
        // ---- ws_spot_steps: the steps; what is uploaded -- the sweep's pairs by kernel class, intervals, windows, ends --; what the
        // sweep leaves at the ends; the windows' results.  ws_spot_dirs: the intervals' words
        const size_t np = rec_pairs.size(), ne = ends.size();
        const uint64_t slots = step_off[last] - step_off[first];
        Carve ws;
        const size_t o_steps = ws.take<apd_path_step>(slots);
        const size_t o_pairs = ws.take<SpotRecPair>(np), o_iv = ws.take<SpotInterval>(intervals.size());
        const size_t o_win = ws.take<SpotTraceWindow>(trace.size()), o_ends = ws.take<uint32_t>(ne);
        const size_t o_end_cost = ws.take<float>(ne), o_end_start = ws.take<uint32_t>(ne);
        results.carve(ws);
        rc = reserve_ws(ctx, ctx->ws_spot_dirs, std::max<size_t>((size_t)words * sizeof(uint32_t), 16));
        if (rc) return rc;
        rc = reserve_ws(ctx, ctx->ws_spot_steps, ws.size);
        if (rc) return rc;
        upload.assign(o_end_cost - o_pairs, 0);
        SpotRecPair *h_pairs = (SpotRecPair *)upload.data();
        for (size_t k = 0; k < np; ++k) h_pairs[classes.slot(rec_class[k])] = rec_pairs[k];
        std::memcpy(upload.data() + (o_iv - o_pairs), intervals.data(), intervals.size() * sizeof(SpotInterval));
        std::memcpy(upload.data() + (o_win - o_pairs), trace.data(), trace.size() * sizeof(SpotTraceWindow));
        std::memcpy(upload.data() + (o_ends - o_pairs), ends.data(), ne * 4);
        char *base = ctx->ws_spot_steps.as<char>();
        SpotPathLaunch L{};
        L.src = spot_source(batch, cfg->insertion_penalty, cfg->deletion_penalty, cfg->match_penalty);
        L.d_intervals = (const SpotInterval *)(base + o_iv);
        L.d_ends = (const uint32_t *)(base + o_ends);
        L.d_end_cost = (float *)(base + o_end_cost); L.d_end_start = (uint32_t *)(base + o_end_start);
        L.d_dirs = ctx->ws_spot_dirs.as<uint32_t>();
        L.d_windows = (const SpotTraceWindow *)(base + o_win);
        L.d_steps = (apd_path_step *)(base + o_steps);
        results.bind(L, base);
        HIP_TRY(ctx, hipMemcpyAsync(base + o_pairs, upload.data(), upload.size(), hipMemcpyHostToDevice, ctx->stream));
        if (ctx->timing && first_launch) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        first_launch = false;
        for (uint32_t c = 0; c < kSpotClasses; ++c) {
            L.d_pairs = (const SpotRecPair *)(base + o_pairs) + classes.first[c];
            L.n_pairs = (uint32_t)classes.n[c];
            HIP_TRY(ctx, launch_spot_record(L, c, classes.r_max, ctx->stream));
        }
        HIP_TRY(ctx, launch_spot_trace(L, ctx->stream));
        if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }   // the last chunk's record stands
        HIP_TRY(ctx, hipMemcpyAsync(steps + step_off[first], L.d_steps, (size_t)slots * sizeof(apd_path_step), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = results.read_back(ctx, L))) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspaces (and `upload`)
        results.scatter();
        first = last;
    }
    return APD_OK;
}
