// The grouping helpers of csrc/apd_plan.h (number_by_first_appearance, GroupMembers) against their definitions, on seeded random
// inputs.  Plain C++17, no GPU; tests/test_spot_group_plan.py builds it under AddressSanitizer + UBSan and runs it.
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
    }
    std::printf("groups ok: %ld rounds, no sanitizer report\n", rounds);
    return 0;
}
