// Stand-alone driver of the two passes localization_amd/csrc/window_structure.cpp adds for joint covariance calls — check_pairs, the
// host-side check that stands between a caller's pair tables and the kernels, and envelope_blocks_max_joint, the pair-aware envelope count —
// for tests/test_joint_covariance_cpu.py: host code only, built with plain g++ under AddressSanitizer + UBSan.  It links against
// window_structure.cpp and nothing else of the product.
//
//   joint_pairs_driver <in>      prints one line per batch of <in>: "<check_pairs> <envelope_blocks_max_joint> <envelope_blocks_max>"
//
// <in>: one or more batches back to back.  One batch =
//   int32[4]  nv_max nr_max ns_max npair_max
//   int64     n (>= 1)
//   counts int32 [n][4], r_idx int32 [n][nr_max][2], s_idx int32 [n][ns_max][4], pair_counts int32 [n], pairs int32 [n][npair_max][2]
// check_pairs runs on every batch (its contract asks for valid counts[.][0] only); the envelope counts are documented to run on tables
// nobody has validated.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "window_structure.h"

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc != 2) { std::fprintf(stderr, "usage: %s <in>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int index = 0;; ++index) {
        int32_t head[4];
        const size_t got = std::fread(head, 4, 4, in);
        if (got == 0) break;   // the end of the input
        int64_t n = 0;
        if (got != 4 || std::fread(&n, 8, 1, in) != 1 || n < 1 || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0) {
            std::fprintf(stderr, "batch %d: bad header\n", index);
            return 2;
        }
        const WindowCaps c{head[0], head[1], 0, head[2], head[0]};
        const int32_t npm = head[3];
        const size_t N = (size_t)n;
        std::vector<int32_t> counts, r_idx, s_idx, pair_counts, pairs;
        if (!read_vec(in, counts, N * 4) || !read_vec(in, r_idx, N * c.nr_max * 2) || !read_vec(in, s_idx, N * c.ns_max * 4) ||
            !read_vec(in, pair_counts, N) || !read_vec(in, pairs, N * (size_t)npm * 2)) {
            std::fprintf(stderr, "batch %d: short tables\n", index);
            return 2;
        }
        const HostBatch b{n, nullptr, counts.data(), nullptr, nullptr, nullptr, r_idx.data(), nullptr, s_idx.data()};
        const PairTables pt{npm, pair_counts.data(), pairs.data()};
        std::printf("%d %lld %lld\n", check_pairs(n, counts.data(), pt), envelope_blocks_max_joint(c, b, pt), envelope_blocks_max(c, b));
    }
    std::fclose(in);
    return 0;
}
