// Planning arithmetic of the host drivers (apd_path_api.hip, apd_spot_api.hip, apd_spot_stream_api.hip): where the regions of a
// workspace lie, where a chunk of a work list ends, where the descriptors of a kernel class go.  Plain C++17 and no project types:
// tests/cpp/plan_check.cpp checks every piece against its definition on the host.
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
