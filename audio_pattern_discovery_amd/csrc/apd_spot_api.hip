// C ABI of libapd_hip.so (include/apd.h): subsequence alignment over pair lists -- curves and bests, detection, score quantiles, the
// warping paths of spotted windows.  The host side around dtw_spot.hip, dtw_spot_detect.hip, dtw_spot_quantile.hip and
// dtw_spot_path.hip.  apd_spot, apd_spot_detect and apd_spot_quantiles are one plan and one sweep -- GroupChunkPlan (apd_plan.h) cuts
// the list into chunks of whole groups and numbers a chunk's pairs, CurveSweep (apd_host.h) lays out, uploads and launches
// launch_spot -- and then each its own stage on the curves: the read-back, the detector, the select.
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
    const ResidentIndex idx(batch);
    int rc = check_pair_list(batch, pairs, n_pairs);
    if (rc) return rc;
    CurveSweep sweep{ctx, batch, cfg, idx, pairs};
    curve_off[0] = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) curve_off[p + 1] = curve_off[p] + sweep.stream_len(p);
    const bool curves = cost != nullptr;
    if (!curves && !best) return APD_OK;                                  // sizes only
    if (curves && capacity < curve_off[n_pairs]) return APD_ERR_INVALID_ARG;
    if (n_pairs == 0) return APD_OK;
    if ((rc = spot_check_pairs(ctx, "apd_spot", idx, pairs, n_pairs))) return rc;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot launch");
    // every pair its own group; a chunk: as many as keep the curves under the cap (best only: nothing is stored)
    constexpr uint64_t kEntryBytes = sizeof(float) + sizeof(uint32_t);
    GroupChunkPlan plan(n_pairs, ChunkBudget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch});
    while (sweep.next(plan, [&](uint64_t p) { return curves ? sweep.stream_len(p) * kEntryBytes : 0; })) {
        sweep.carve(plan, curves);
        sweep.place(plan);
        if ((rc = sweep.run(plan))) return rc;
        if (ctx->timing && plan.g1 == n_pairs) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (curves) {
            HIP_TRY(ctx, hipMemcpyAsync(cost + curve_off[plan.g0], sweep.L.d_cost, (size_t)plan.entries * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(start + curve_off[plan.g0], sweep.L.d_start, (size_t)plan.entries * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (best) HIP_TRY(ctx, hipMemcpyAsync(best + plan.g0, sweep.L.d_best, plan.np() * sizeof(apd_spot_best), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace
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

// CurveSweep, then candidates, greedy picking and the packed hits on the device (kernels: dtw_spot_detect.hip).  ws_spot_hits: the
// chunk's packed hits, sized once its hit counts are known.
extern "C" int apd_spot_detect(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                               const float *thresholds, int compete, apd_spot_hit *hits, uint64_t capacity, uint64_t *hit_off,
                               uint64_t *n_groups, uint64_t *n_hits)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if ((compete != APD_DETECT_PER_PAIR && compete != APD_DETECT_PER_STREAM) || (n_pairs && !thresholds) || !hit_off || !n_groups || !n_hits ||
        (capacity && !hits))
        return APD_ERR_INVALID_ARG;
    const ResidentIndex idx(batch);
    int rc = check_pair_list(batch, pairs, n_pairs);
    if (rc) return rc;
    *n_groups = 0;
    *n_hits = 0;
    hit_off[0] = 0;
    if (n_pairs == 0) return APD_OK;
    if ((rc = spot_check_pairs(ctx, "apd_spot_detect", idx, pairs, n_pairs))) return rc;
    // groups in order of first appearance: every pair its own, or the pairs of a stream
    std::vector<uint64_t> group_of(n_pairs);
    uint64_t ng = n_pairs;
    if (compete == APD_DETECT_PER_PAIR)
        for (uint64_t p = 0; p < n_pairs; ++p) group_of[p] = p;
    else
        ng = number_by_first_appearance(pairs + 1, 2, n_pairs, batch->n_seq, group_of);
    GroupMembers groups;
    if (!groups.build(group_of, ng, kMaxPairsPerLaunch)) {
        ctx->last_error = "apd_spot_detect: a group of more than 2^24 pairs";
        return APD_ERR_UNSUPPORTED;
    }
    *n_groups = ng;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot detect launch");
    CurveSweep sweep{ctx, batch, cfg, idx, pairs};
    // a group weighs its curves and candidates, and the accepted windows of its stream
    constexpr uint64_t kEntryBytes = sizeof(float) + sizeof(uint32_t) + sizeof(ulonglong2), kStageBytes = sizeof(uint2);
    auto group_bytes = [&](uint64_t g) {
        const uint64_t m = sweep.stream_len(groups.members[groups.first[g]]);
        return groups.size(g) * m * kEntryBytes + m * kStageBytes;
    };
    GroupChunkPlan plan(groups, ChunkBudget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch});
    std::vector<uint32_t> counts;
    while (sweep.next(plan, group_bytes)) {
        const uint64_t g0 = plan.g0, g1 = plan.g1, ngc = g1 - g0, np = plan.np();
        // ws_spot behind the sweep's regions: what is uploaded with its descriptors -- the detector's pairs and groups --; what is
        // zeroed -- candidate and hit counts --; the hit bases; the candidates and the accepted windows
        Carve &ws = sweep.ws;
        sweep.carve(plan);
        const size_t o_dp = ws.take<SpotDetectPair>(np), o_grp = ws.take<SpotDetectGroup>(ngc);
        sweep.place(plan);
        const size_t o_cc = ws.take<unsigned long long>(ngc), o_hc = ws.take<uint32_t>(ngc), o_hb = ws.take<unsigned long long>(ngc + 1);
        const size_t o_cand = ws.take<ulonglong2>(plan.entries);
        uint64_t stage_slots = 0;
        SpotDetectPair *dp = sweep.record<SpotDetectPair>(o_dp);
        SpotDetectGroup *grp = sweep.record<SpotDetectGroup>(o_grp);
        for (uint64_t k = 0; k < np; ++k) {
            const GroupChunkPlan::Slot &s = plan.slots[k];
            dp[k] = SpotDetectPair{sweep.curve(s), thresholds[s.item], 0};
            SpotDetectGroup &G = grp[s.group];
            if (k == 0 || plan.slots[k - 1].group != s.group) {
                G.cand_off = s.off; G.stage_off = stage_slots; G.stage_cap = s.len;
                stage_slots += s.len;
            }
            G.cand_cap += s.len;
        }
        const size_t o_stage = ws.take<uint2>(stage_slots);
        if ((rc = sweep.run(plan, o_cc, o_hb - o_cc))) return rc;
        SpotDetectLaunch D{};
        D.d_cost = sweep.L.d_cost; D.d_start = sweep.L.d_start;
        D.d_pairs = sweep.device<SpotDetectPair>(o_dp); D.n_pairs = (uint32_t)np;
        D.d_groups = sweep.device<SpotDetectGroup>(o_grp); D.n_groups = (uint32_t)ngc;
        D.d_cand = sweep.device<ulonglong2>(o_cand);
        D.d_stage = sweep.device<uint2>(o_stage);
        D.d_cand_count = sweep.device<unsigned long long>(o_cc);
        D.d_hit_count = sweep.device<uint32_t>(o_hc);
        D.d_hit_base = sweep.device<unsigned long long>(o_hb);
        HIP_TRY(ctx, launch_spot_detect(D, plan.max_len, ctx->stream));
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
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace
    }
    *n_hits = hit_off[ng];
    return APD_OK;
}

// ----------------------------------------------------------------------------------- spot score quantiles

// CurveSweep, then the radix select of every (group, quantile) on the device (kernels: dtw_spot_quantile.hip).  The rank k of every
// (group, quantile) is worked out here from the group's entries and uploaded with its state record.
extern "C" int apd_spot_quantiles(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                                  int grouping, const float *perc, uint32_t n_perc, float *values, int32_t *status, uint64_t *group_of_out,
                                  uint64_t *entries_out, uint64_t *nans_out, uint64_t *n_groups)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if (grouping < APD_QUANTILES_PER_PAIR || grouping > APD_QUANTILES_ALL || n_perc == 0 || n_perc > APD_SPOT_QUANTILES_MAX || !perc || !values ||
        !n_groups)
        return APD_ERR_INVALID_ARG;
    const ResidentIndex idx(batch);
    int rc = check_pair_list(batch, pairs, n_pairs);
    if (rc) return rc;
    if (n_pairs == 0) { *n_groups = 0; return APD_OK; }
    if ((rc = spot_check_pairs(ctx, "apd_spot_quantiles", idx, pairs, n_pairs))) return rc;
    // groups in order of first appearance: every pair its own, the pairs of a query, or all
    std::vector<uint64_t> group_of(n_pairs, 0);                           // APD_QUANTILES_ALL: every pair in group 0
    uint64_t ng = 1;
    if (grouping == APD_QUANTILES_PER_PAIR) {
        ng = n_pairs;
        for (uint64_t p = 0; p < n_pairs; ++p) group_of[p] = p;
    } else if (grouping == APD_QUANTILES_PER_QUERY) {
        ng = number_by_first_appearance(pairs, 2, n_pairs, batch->n_seq, group_of);
    }
    GroupMembers groups;
    if (!groups.build(group_of, ng, kMaxPairsPerLaunch)) {
        ctx->last_error = "apd_spot_quantiles: a group of more than 2^24 pairs";
        return APD_ERR_UNSUPPORTED;
    }
    CurveSweep sweep{ctx, batch, cfg, idx, pairs};
    std::vector<uint64_t> group_entries(ng, 0);
    for (uint64_t p = 0; p < n_pairs; ++p) group_entries[group_of[p]] += sweep.stream_len(p);
    *n_groups = ng;
    if (group_of_out) std::copy(group_of.begin(), group_of.end(), group_of_out);
    if (entries_out) std::copy(group_entries.begin(), group_entries.end(), entries_out);
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot quantiles launch");
    // a group weighs its curves, its pairs' records and the histograms and states of its quantiles
    constexpr uint64_t kEntryBytes = sizeof(float) + sizeof(uint32_t);
    constexpr uint64_t kPairBytes = sizeof(SpotPair) + sizeof(SpotCurve) + sizeof(apd_spot_best);
    const uint64_t quantile_bytes = (uint64_t)n_perc * (kSpotQuantileBins * sizeof(unsigned long long) + sizeof(SpotQuantileState) + 8);
    auto group_bytes = [&](uint64_t g) { return group_entries[g] * kEntryBytes + groups.size(g) * kPairBytes + quantile_bytes; };
    GroupChunkPlan plan(groups, ChunkBudget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch});
    std::vector<char> results;
    while (sweep.next(plan, group_bytes)) {
        const uint64_t g0 = plan.g0, ngc = plan.g1 - g0, np = plan.np(), nq = n_perc;
        // ws_spot behind the sweep's regions: what is uploaded with its descriptors -- the select's pairs, the states --; what is
        // zeroed -- the histograms --; what is read back -- values, statuses, NaN counts
        Carve &ws = sweep.ws;
        sweep.carve(plan);
        const size_t o_qp = ws.take<SpotCurve>(np), o_state = ws.take<SpotQuantileState>(ngc * nq);
        sweep.place(plan);
        const size_t o_hist = ws.take<unsigned long long>(ngc * nq * kSpotQuantileBins);
        const size_t o_values = ws.take<float>(ngc * nq), o_status = ws.take<int32_t>(ngc * nq), o_nans = ws.take<unsigned long long>(ngc);
        SpotCurve *qp = sweep.record<SpotCurve>(o_qp);
        SpotQuantileState *state = sweep.record<SpotQuantileState>(o_state);
        for (uint64_t k = 0; k < np; ++k) qp[k] = sweep.curve(plan.slots[k]);
        for (uint64_t g = g0; g < plan.g1; ++g)
            for (uint32_t q = 0; q < n_perc; ++q) state[(g - g0) * nq + q].rank = percentile_index(group_entries[g], perc[q]);
        if ((rc = sweep.run(plan, o_hist, o_values - o_hist))) return rc;
        SpotQuantileLaunch Q{};
        Q.d_cost = sweep.L.d_cost; Q.d_start = sweep.L.d_start;
        Q.d_pairs = sweep.device<SpotCurve>(o_qp); Q.n_pairs = (uint32_t)np;
        Q.n_groups = (uint32_t)ngc; Q.n_perc = n_perc;
        Q.d_state = sweep.device<SpotQuantileState>(o_state);
        Q.d_hist = sweep.device<unsigned long long>(o_hist);
        Q.d_values = sweep.device<float>(o_values);
        Q.d_status = sweep.device<int32_t>(o_status);
        Q.d_nans = sweep.device<unsigned long long>(o_nans);
        HIP_TRY(ctx, launch_spot_quantiles(Q, plan.max_len, ctx->stream));
        if (ctx->timing && plan.g1 == ng) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        results.resize(ws.size - o_values);
        HIP_TRY(ctx, hipMemcpyAsync(results.data(), sweep.device<char>(o_values), results.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace
        std::memcpy(values + g0 * nq, results.data(), (size_t)(ngc * nq) * sizeof(float));
        if (status) std::memcpy(status + g0 * nq, results.data() + (o_status - o_values), (size_t)(ngc * nq) * sizeof(int32_t));
        if (nans_out) std::memcpy(nans_out + g0, results.data() + (o_nans - o_values), (size_t)ngc * sizeof(uint64_t));
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
