// Stand-alone driver of the host half of loc_window_slide_resident (localization_amd/csrc/window_structure.cpp: slide_indices,
// slide_rows_translation_only) for tests/test_resident_slide_cpu.py: host code only, built with plain g++ under AddressSanitizer + UBSan.
// It links against window_structure.cpp and nothing else of the product.
//
//   slide_indices_driver <in>      prints per batch "<bad> <new rows translation-only>"; where bad = 0 the rule is then applied to the
//                                  mirror and "<largest anchor code>" and one line per window follow: "nv nr np : v0 v1 ... : p ..." (used rows)
//
// <in>: one or more batches back to back.  One batch =
//   int32[8]  nv_max nr_max np_max bw_max n_anchors nr_new_max np_new_max has_drop
//   int64     n (>= 1)
//   int32     counts [n][4], r_idx [n][nr_max][2], p_idx [n][np_max]                 the mirror
//   int32     drop [n] (has_drop), r_counts [n], new r_idx [n][nr_new_max][2] (nr_new_max > 0), p_counts [n] (np_new_max > 0)
//   double    new_pose [n][12], new r_val [n][nr_new_max][5], new p_val [n][np_new_max][18]
// Every table is allocated at exactly its size, so that a read or write past a table's end is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "window_structure.h"

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    v.shrink_to_fit();
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc != 2) { std::fprintf(stderr, "usage: %s <in>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int index = 0;; ++index) {
        int32_t head[8];
        const size_t got = std::fread(head, 4, 8, in);
        if (got == 0) break;
        int64_t n = 0;
        if (got != 8 || std::fread(&n, 8, 1, in) != 1 || n < 1) { std::fprintf(stderr, "batch %d: bad header\n", index); return 2; }
        const WindowCaps c{head[0], head[1], head[2], 0, head[3]};
        const int n_anchors = head[4], nrn = head[5], npn = head[6];
        const bool has_drop = head[7] != 0;
        std::vector<int32_t> counts, r_idx, p_idx, drop, r_counts, new_r_idx, p_counts;
        std::vector<double> new_pose, r_val, p_val;
        const size_t N = (size_t)n;
        if (!read_vec(in, counts, N * 4) || !read_vec(in, r_idx, N * c.nr_max * 2) || !read_vec(in, p_idx, N * c.np_max) || !read_vec(in, drop, has_drop ? N : 0) ||
            !read_vec(in, r_counts, nrn > 0 ? N : 0) || !read_vec(in, new_r_idx, N * nrn * 2) || !read_vec(in, p_counts, npn > 0 ? N : 0) ||
            !read_vec(in, new_pose, N * 12) || !read_vec(in, r_val, N * nrn * 5) || !read_vec(in, p_val, N * npn * 18)) {
            std::fprintf(stderr, "batch %d: short tables\n", index);
            return 2;
        }
        const SlideRows rows{has_drop ? drop.data() : nullptr, nrn, r_counts.data(), new_r_idx.data(), npn, p_counts.data()};
        const std::vector<int32_t> before_c = counts, before_r = r_idx, before_p = p_idx;
        const int bad = slide_indices(c, n_anchors, n, counts.data(), r_idx.data(), p_idx.data(), rows, false).bad;
        if (counts != before_c || r_idx != before_r || p_idx != before_p) { std::fprintf(stderr, "batch %d: the check wrote to the mirror\n", index); return 3; }
        std::printf("%d %d\n", bad, slide_rows_translation_only(n, rows, new_pose.data(), r_val.data(), p_val.data()) ? 1 : 0);
        if (bad) continue;
        const SlideVerdict v = slide_indices(c, n_anchors, n, counts.data(), r_idx.data(), p_idx.data(), rows, true);
        std::printf("%d\n", v.max_anchor);
        for (size_t i = 0; i < N; ++i) {
            const int32_t* cn = counts.data() + i * 4;
            std::printf("%d %d %d :", cn[0], cn[1], cn[2]);
            for (int e = 0; e < cn[1] * 2; ++e) std::printf(" %d", r_idx[i * c.nr_max * 2 + e]);
            std::printf(" :");
            for (int e = 0; e < cn[2]; ++e) std::printf(" %d", p_idx[i * c.np_max + e]);
            std::printf("\n");
        }
    }
    std::fclose(in);
    return 0;
}
