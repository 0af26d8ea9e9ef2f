// Stand-alone driver of the host check of loc_window_marginal_prior_host (localization_amd/csrc/window_structure.cpp: check_marginal_drop,
// translation_only with a full-matrix table, prior_information_translation_only) for tests/test_marginal_prior_cpu.py: host code only,
// built with plain g++ under AddressSanitizer + UBSan.  It links against window_structure.cpp and nothing else of the product.
//
//   marginal_drop_driver <in>      prints one line per batch: "<check_instances> <check_marginal_drop> <translation_only> <pinfo translation-only>"
//                                  (-1 where a pass was not run: only a validated batch reaches the drop check, as in capi_window.cpp)
//
// <in>: one or more batches back to back.  One batch =
//   int32[8]  nv_max nr_max np_max ns_max bw_max n_anchors has_pinfo 0
//   int64     n (>= 1)
//   the eight tables in window_tables.h's order and window_kernel.h's layout: poses counts r_val p_val s_val r_idx p_idx s_idx
//   int32[n]  drop
//   has_pinfo: double[n][np_max][36]
// Every table is allocated at exactly its size, so that a read past a table's end is an AddressSanitizer report.
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
        const WindowCaps c{head[0], head[1], head[2], head[3], head[4]};
        const int n_anchors = head[5];
        const bool has_pinfo = head[6] != 0;
        std::vector<double> poses, r_val, p_val, s_val, pinfo;
        std::vector<int32_t> counts, r_idx, p_idx, s_idx, drop;
        const size_t N = (size_t)n;
        if (!read_vec(in, poses, N * c.nv_max * 12) || !read_vec(in, counts, N * 4) || !read_vec(in, r_val, N * c.nr_max * 5) ||
            !read_vec(in, p_val, N * c.np_max * 18) || !read_vec(in, s_val, N * c.ns_max * 48) || !read_vec(in, r_idx, N * c.nr_max * 2) ||
            !read_vec(in, p_idx, N * c.np_max) || !read_vec(in, s_idx, N * c.ns_max * 4) || !read_vec(in, drop, N) ||
            (has_pinfo && !read_vec(in, pinfo, N * c.np_max * 36))) {
            std::fprintf(stderr, "batch %d: short tables\n", index);
            return 2;
        }
        const HostBatch b{n, poses.data(), counts.data(), r_val.data(), p_val.data(), s_val.data(), r_idx.data(), p_idx.data(), s_idx.data()};
        const int code = check_instances(c, n_anchors, b);
        int drop_code = -1, translation = -1, pinfo_ok = -1;
        if (code == 0) {
            drop_code = check_marginal_drop(c, b, drop.data());
            translation = translation_only(c, n_anchors, b, has_pinfo) ? 1 : 0;
            if (has_pinfo) pinfo_ok = prior_information_translation_only(N * c.np_max, pinfo.data()) ? 1 : 0;
        }
        std::printf("%d %d %d %d\n", code, drop_code, translation, pinfo_ok);
    }
    std::fclose(in);
    return 0;
}
