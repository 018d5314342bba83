// Planning arithmetic of the host drivers (apd_path_api.hip, apd_spot_api.hip, apd_spot_stream_api.hip): where the regions of a
// workspace lie, where a chunk of a work list ends, where the descriptors of a kernel class go, how a grouped pair list is cut
// into chunks of whole groups and numbered inside them.  Plain C++17 and no project types: tests/cpp/plan_check.cpp and
// tests/cpp/group_check.cpp check every piece against its definition on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#pragma GCC visibility push(hidden)   // internal to libapd_hip.so: nothing here joins its exported symbols
namespace apd {

// The layout of one workspace: regions in the order of the take() calls, each on an `align`-byte boundary (16: the widest device
// type, ulonglong2; hipMalloc's own alignment is coarser).  `size` is what the workspace must hold; a region of no elements is legal
// and shares its offset with the next one.
struct Carve {
    size_t size = 0, align;
    explicit Carve(size_t align_bytes = 16) : align(align_bytes) {}
    template <class T> size_t take(size_t count)
    {
        const size_t off = (size + align - 1) / align * align;
        size = off + count * sizeof(T);
        return off;
    }
};

// The greedy cut of a work list into chunks: a chunk takes its first item whatever it weighs, then every further one that keeps both
// running byte totals within cap_bytes and the item count within max_items.  reset() opens the next chunk.
struct ChunkBudget {
    uint64_t cap_bytes, max_items;
    uint64_t bytes_a = 0, bytes_b = 0, items = 0;
    bool open = false;
    bool admit(uint64_t a, uint64_t b = 0, uint64_t n = 1)
    {
        if (open && (bytes_a + a > cap_bytes || bytes_b + b > cap_bytes || items + n > max_items)) return false;
        bytes_a += a; bytes_b += b; items += n;
        return open = true;
    }
    void reset() { bytes_a = bytes_b = items = 0; open = false; }
};

// A counting sort into K classes: count() every item, close(), then slot() hands every item its place -- classes in ascending order,
// items of a class in the order they ask.  Class c owns slots first[c] .. first[c] + n[c].
template <uint32_t K>
struct ClassBuckets {
    uint64_t n[K] = {}, first[K] = {}, next[K] = {};
    void count(uint32_t c, uint64_t items = 1) { n[c] += items; }
    void close()
    {
        for (uint32_t c = 1; c < K; ++c) first[c] = first[c - 1] + n[c - 1];
        for (uint32_t c = 0; c < K; ++c) next[c] = first[c];
    }
    uint64_t slot(uint32_t c) { return next[c]++; }
};

// The groups of a pair list (apd_spot_detect, apd_spot_quantiles).  number_by_first_appearance: item i of `n` has key keys[i * stride]
// (< n_keys); group_of[i] = the rank of its key among the distinct keys in order of first appearance; returns their number.
inline uint64_t number_by_first_appearance(const uint32_t *keys, size_t stride, uint64_t n, uint32_t n_keys, std::vector<uint64_t> &group_of)
{
    std::vector<uint64_t> group_of_key(n_keys, ~0ull);
    uint64_t ng = 0;
    group_of.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t &g = group_of_key[keys[i * stride]];
        if (g == ~0ull) g = ng++;
        group_of[i] = g;
    }
    return ng;
}
// members[first[g] .. first[g + 1]): the items of group g, ascending (a counting sort of group_of).
struct GroupMembers {
    std::vector<uint64_t> first, members;
    // false, with nothing usable built: some group holds more than max_items items
    bool build(const std::vector<uint64_t> &group_of, uint64_t n_groups, uint64_t max_items)
    {
        first.assign(n_groups + 1, 0);
        for (uint64_t g : group_of) ++first[g + 1];
        for (uint64_t g = 0; g < n_groups; ++g) {
            if (first[g + 1] > max_items) return false;
            first[g + 1] += first[g];
        }
        std::vector<uint64_t> fill(first.begin(), first.end() - 1);
        members.resize(group_of.size());
        for (uint64_t i = 0; i < group_of.size(); ++i) members[fill[group_of[i]]++] = i;
        return true;
    }
    uint64_t size(uint64_t g) const { return first[g + 1] - first[g]; }
};

// The cut of a grouped list into chunks of whole groups, and the numbering inside a chunk: what apd_spot, apd_spot_detect and
// apd_spot_quantiles plan before they sweep (CurveSweep, apd_host.h).  next() moves to the chunk of groups [g0, g1) -- the first
// group whatever weight(g) bytes it weighs, then every further one that keeps the bytes and the items within the budget -- and
// numbers its items group by group, members ascending: slot k holds the caller's item, its group of the chunk (g - g0), its length
// length(item) and its offset, the sum of the lengths before it.  entries: the sum of all; max_len: the longest.
struct GroupChunkPlan {
    struct Slot {
        uint64_t item, off;
        uint32_t group, len;
    };
    const GroupMembers *groups;       // null: n_groups groups of one, group g = item g
    uint64_t n_groups;
    ChunkBudget budget;
    uint64_t g0 = 0, g1 = 0, entries = 0;
    uint32_t max_len = 0;
    std::vector<Slot> slots;

    GroupChunkPlan(const GroupMembers &members, ChunkBudget b) : groups(&members), n_groups(members.first.size() - 1), budget(b) {}
    GroupChunkPlan(uint64_t n_singletons, ChunkBudget b) : groups(nullptr), n_groups(n_singletons), budget(b) {}
    uint64_t np() const { return slots.size(); }
    // false: the list is used up
    template <class Weight, class Length> bool next(Weight weight, Length length)
    {
        g0 = g1;
        if (g0 == n_groups) return false;
        budget.reset();
        slots.clear();
        entries = 0;
        max_len = 0;
        while (g1 < n_groups && budget.admit(weight(g1), 0, groups ? groups->size(g1) : 1)) {
            const uint64_t t0 = groups ? groups->first[g1] : g1, t1 = groups ? groups->first[g1 + 1] : g1 + 1;
            for (uint64_t t = t0; t < t1; ++t) {
                const uint64_t item = groups ? groups->members[t] : t;
                const uint32_t len = length(item);
                slots.push_back(Slot{item, entries, (uint32_t)(g1 - g0), len});
                entries += len;
                max_len = len > max_len ? len : max_len;
            }
            ++g1;
        }
        return true;
    }
};

// Cap of a chunk's device workspace in bytes: the environment variable (APD_PATH_WORKSPACE_BYTES, APD_SPOT_WORKSPACE_BYTES) when it
// holds a positive number, 1 GiB otherwise.
inline uint64_t workspace_cap(const char *env_name)
{
    if (const char *v = std::getenv(env_name)) {
        const unsigned long long b = std::strtoull(v, nullptr, 10);
        if (b > 0) return b;
    }
    return 1ull << 30;
}

}  // namespace apd
#pragma GCC visibility pop
