// The grouping helpers of csrc/apd_plan.h (number_by_first_appearance, GroupMembers) and the chunk plan over them (GroupChunkPlan)
// against their definitions, on seeded random inputs.  Plain C++17, no GPU; tests/test_spot_group_plan.py builds it under
// AddressSanitizer + UBSan and runs it.
//   group_check <rounds> <seed>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../audio_pattern_discovery_amd/csrc/apd_plan.h"

using namespace apd;

#define REQUIRE(cond)                                                                 \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "round %ld: %s\n", round, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    const long rounds = argc > 1 ? std::atol(argv[1]) : 1000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    for (long round = 0; round < rounds; ++round) {
        const uint32_t n_keys = 1 + (uint32_t)(rng() % 12);
        const uint64_t n = rng() % 40;
        std::vector<uint32_t> pairs(2 * n + 1);
        for (auto &v : pairs) v = (uint32_t)(rng() % n_keys);
        const size_t column = rng() % 2;                                  // key = the pair's x or its y
        std::vector<uint64_t> group_of;
        const uint64_t ng = number_by_first_appearance(pairs.data() + column, 2, n, n_keys, group_of);
        // definition: equal keys share a group, and the groups are numbered as their first items stand in the list
        REQUIRE(group_of.size() == n);
        uint64_t next = 0;
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t first = i;
            for (uint64_t j = 0; j < i; ++j)
                if (pairs[2 * j + column] == pairs[2 * i + column]) { first = j; break; }
            if (first == i) REQUIRE(group_of[i] == next++);
            else REQUIRE(group_of[i] == group_of[first]);
        }
        REQUIRE(ng == next);
        // definition of the member lists: every item once, in its group's stretch, ascending inside it
        std::vector<uint64_t> sizes(ng, 0);
        for (uint64_t g : group_of) ++sizes[g];
        uint64_t largest = 0;
        for (uint64_t s : sizes) largest = s > largest ? s : largest;
        GroupMembers groups;
        if (largest > 0) REQUIRE(!groups.build(group_of, ng, largest - 1));   // one item too many for some group: refused
        REQUIRE(groups.build(group_of, ng, largest));
        REQUIRE(groups.first.size() == ng + 1 && groups.first[0] == 0 && groups.first[ng] == n && groups.members.size() == n);
        for (uint64_t g = 0; g < ng; ++g) {
            REQUIRE(groups.size(g) == sizes[g] && sizes[g] >= 1);
            for (uint64_t t = groups.first[g]; t < groups.first[g + 1]; ++t) {
                REQUIRE(groups.members[t] < n && group_of[groups.members[t]] == g);
                if (t > groups.first[g]) REQUIRE(groups.members[t - 1] < groups.members[t]);
            }
        }
        // the chunk plan over these groups (half the rounds: n groups of one, both forms) under a random weight per group and length
        // per item.  Caps: below every group, a few groups, everything; in a quarter of the rounds the item limit binds instead.
        const bool singles = round % 2 == 1;
        GroupMembers identity;
        if (singles) {
            std::vector<uint64_t> own(n);
            for (uint64_t i = 0; i < n; ++i) own[i] = i;
            REQUIRE(identity.build(own, n, 1));
        }
        const GroupMembers &gm = singles ? identity : groups;
        const uint64_t n_groups = gm.first.size() - 1;
        std::vector<uint32_t> len(n);
        for (auto &v : len) v = 1 + (uint32_t)(rng() % 300);
        std::vector<uint64_t> weight(n_groups);
        uint64_t total = 0;
        for (auto &w : weight) total += w = rng() % 4 == 0 ? 0 : 1 + rng() % 1000;
        const uint64_t caps[3] = {0, 1 + rng() % 2500, total};
        const uint64_t cap = caps[rng() % 3];
        const uint64_t max_items = round % 4 < 2 ? ~0ull : (singles ? 1 : largest) + rng() % 4;
        const uint64_t cap_used = round % 4 < 2 ? cap : ~0ull >> 1;
        auto weigh = [&](uint64_t g) { return weight[g]; };
        auto length = [&](uint64_t i) { return len[i]; };
        GroupChunkPlan plan(gm, ChunkBudget{cap_used, max_items});
        GroupChunkPlan ones(n, ChunkBudget{cap_used, max_items});
        uint64_t expect_g0 = 0;
        while (plan.next(weigh, length)) {
            REQUIRE(plan.g0 == expect_g0 && plan.g1 > plan.g0 && plan.g1 <= n_groups);   // in order, never empty
            // the greedy rule: what the chunk holds beyond its first group fits, and the next group would not
            uint64_t bytes = 0, items = 0;
            for (uint64_t g = plan.g0; g < plan.g1; ++g) { bytes += weight[g]; items += gm.size(g); }
            if (plan.g1 - plan.g0 > 1) REQUIRE(bytes <= cap_used && items <= max_items);
            if (plan.g1 < n_groups) REQUIRE(bytes + weight[plan.g1] > cap_used || items + gm.size(plan.g1) > max_items);
            // slots: group by group, members ascending, offsets the prefix sums of the lengths
            REQUIRE(plan.np() == items && plan.slots.size() == items);
            uint64_t k = 0, off = 0;
            uint32_t longest = 0;
            for (uint64_t g = plan.g0; g < plan.g1; ++g)
                for (uint64_t t = gm.first[g]; t < gm.first[g + 1]; ++t, ++k) {
                    const GroupChunkPlan::Slot &s = plan.slots[k];
                    REQUIRE(s.item == gm.members[t] && s.group == g - plan.g0 && s.len == len[s.item] && s.off == off);
                    off += s.len;
                    longest = s.len > longest ? s.len : longest;
                }
            REQUIRE(plan.entries == off && plan.max_len == longest);
            if (singles) {                                                // "n groups of one" is the identity grouping
                REQUIRE(ones.next(weigh, length) && ones.g0 == plan.g0 && ones.g1 == plan.g1 && ones.np() == plan.np());
                REQUIRE(ones.entries == plan.entries && ones.max_len == plan.max_len);
                for (k = 0; k < plan.np(); ++k) {
                    const GroupChunkPlan::Slot &a = ones.slots[k], &b = plan.slots[k];
                    REQUIRE(a.item == b.item && a.off == b.off && a.group == b.group && a.len == b.len);
                }
            }
            expect_g0 = plan.g1;
        }
        REQUIRE(expect_g0 == n_groups);                                   // the chunks partition the groups
        REQUIRE(!plan.next(weigh, length) && plan.g0 == n_groups);        // and the end stays the end
        if (singles) REQUIRE(!ones.next(weigh, length));
    }
    std::printf("groups ok: %ld rounds, no sanitizer report\n", rounds);
    return 0;
}
