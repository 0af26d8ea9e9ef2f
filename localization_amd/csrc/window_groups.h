// The TOPOLOGY KEY of a forest window (option "forest_groups"; DESIGN.md §2, "Forest groups"), stated once for the host and the device in
// window_admit.h's way: plain C++ over ONE window's counts and index rows — no HIP types, no allocation, no library call.
// window_structure.cpp's topology_key is a loop over topology_key_word; window_groups_kernel.hip (loc_window_upload_dev under option
// "upload_dev_forest_groups") reads the same words lane-parallel; tests/host/upload_dev_forest_groups_driver.cpp holds both to each other.
//
// The key of a window with counts (nv, nr, np, ns), as int32 words in this order:
//   [0, 4)                     the four counts
//   [4, 4 + 2 nr)              the used r_idx rows, (v0, v1), every fixed endpoint (v1 < 0: an anchor code) collapsed to -1
//   [.., + np)                 the used p_idx rows
//   [.., + 2 ns)               columns 0 - 1 of the used s_idx rows
// Anchor numbers and robust flags (s_idx columns 2 - 3) are not part of it: the grouped kernels read them from the window's own rows.  No row
// at or beyond a count is read.  Two windows are of one group iff their keys are equal word for word.
//
// The DEVICE's candidate hash of a key (window_groups_kernel.hip).  It finds candidates only: the groups are defined by key equality and first
// appearance, and nothing observable depends on the hash (the host's own pass 1 keeps its FNV-1a).  Lane l of 64 folds the words l, l + 64,
// l + 128, ... into a partial (topology_key_lane_hash); the 64 partials are added up modulo 2^64 — in any order and grouping, so a butterfly
// over the lanes and the serial loop below give the same bits — and finished (topology_key_hash_finish).  groups_hash_masked applies the test
// seam (option "upload_dev_groups_hash_bits": the low `bits` bits are kept) and reserves the value 0, which marks an empty slot of the pass's table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "slide_admit.h"

namespace locamd {

LOCAMD_SLIDE_HD inline long long topology_key_words(const int32_t* counts) { return 4 + 2 * (long long)counts[1] + counts[2] + 2 * (long long)counts[3]; }

// word k of the key, 0 <= k < topology_key_words(counts); r_idx [nr][2], p_idx [np], s_idx [ns][4]: the window's own rows
LOCAMD_SLIDE_HD inline int32_t topology_key_word(const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, const int32_t* s_idx, long long k) {
    if (k < 4) return counts[k];
    k -= 4;
    const long long nr2 = 2 * (long long)counts[1];
    if (k < nr2) {
        const int32_t v = r_idx[k];
        return (k & 1) != 0 && v < 0 ? -1 : v;
    }
    k -= nr2;
    if (k < counts[2]) return p_idx[k];
    k -= counts[2];
    return s_idx[(k >> 1) * 4 + (k & 1)];
}

LOCAMD_SLIDE_HD inline bool topology_key_equal(const int32_t* ca, const int32_t* ra, const int32_t* pa, const int32_t* sa, const int32_t* cb, const int32_t* rb, const int32_t* pb,
                                               const int32_t* sb) {
    if (ca[0] != cb[0] || ca[1] != cb[1] || ca[2] != cb[2] || ca[3] != cb[3]) return false;
    const long long nw = topology_key_words(ca);
    for (long long k = 4; k < nw; ++k)
        if (topology_key_word(ca, ra, pa, sa, k) != topology_key_word(cb, rb, pb, sb, k)) return false;
    return true;
}

LOCAMD_SLIDE_HD inline uint64_t groups_mix64(uint64_t x) {   // (splitmix64's finisher)
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// lane `lane`'s partial over the words lane, lane + 64, ... of a key of nw words
LOCAMD_SLIDE_HD inline uint64_t topology_key_lane_hash(const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, const int32_t* s_idx, long long nw, int lane) {
    uint64_t h = 0x9e3779b97f4a7c15ull * (uint64_t)(lane + 1);
    for (long long k = lane; k < nw; k += 64) h = (h ^ (uint32_t)topology_key_word(counts, r_idx, p_idx, s_idx, k)) * 1099511628211ull;
    return groups_mix64(h);
}
LOCAMD_SLIDE_HD inline uint64_t topology_key_hash_finish(uint64_t lane_sum, long long nw) { return groups_mix64(lane_sum + (uint64_t)nw); }
// the whole hash, serially (the device adds the partials with a butterfly)
LOCAMD_SLIDE_HD inline uint64_t topology_key_hash(const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, const int32_t* s_idx) {
    const long long nw = topology_key_words(counts);
    uint64_t sum = 0;
    for (int lane = 0; lane < 64; ++lane) sum += topology_key_lane_hash(counts, r_idx, p_idx, s_idx, nw, lane);
    return topology_key_hash_finish(sum, nw);
}
// bits in [0, 64]: the low bits kept; never 0
LOCAMD_SLIDE_HD inline uint64_t groups_hash_masked(uint64_t h, int bits) {
    const uint64_t m = bits >= 64 ? h : bits <= 0 ? 0 : h & ((1ull << bits) - 1);
    return m != 0 ? m : 1;
}
// where a hash starts probing a table of `cap` slots (a power of two)
LOCAMD_SLIDE_HD inline uint64_t groups_hash_slot(uint64_t masked, uint64_t cap) { return groups_mix64(masked) & (cap - 1); }
// the table's size for n windows: the power of two >= 2 n (at least 64)
LOCAMD_SLIDE_HD inline uint64_t groups_table_slots(long long n) {
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)(n > 0 ? n : 0)) cap <<= 1;
    return cap;
}

// ---- what window_groups_kernel.hip leaves of a batch: OR and sum, in any order and grouping ---------------------------------------------------
enum WindowGroupsBit : uint32_t {
    kGroupsBadNv = 1u,       // a window with nv outside [2, 64] (or a count outside its capacity: an admitted batch has none)
    kGroupsCollision = 2u,   // a window whose key differs from the key of the lowest window of its hash: the host groups the batch itself
    kGroupsOverflow = 4u     // a probe of the pass's table ran out (or met a slot no insert left): likewise
};
struct WindowGroupsRecord {
    uint32_t or_bits;
    int32_t n_groups;        // windows that are the lowest of their hash; the number of groups when no bit is set
};
LOCAMD_SLIDE_HD inline void groups_record_merge(WindowGroupsRecord& r, const WindowGroupsRecord& o) { r.or_bits |= o.or_bits; r.n_groups += o.n_groups; }

}  // namespace locamd
