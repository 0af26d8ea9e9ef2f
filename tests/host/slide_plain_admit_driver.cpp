// Stand-alone driver of the plain-drop slide's per-window admission rule (localization_amd/csrc/slide_plain_admit.h: slide_plain_admit, the one
// statement the device prologue of window_slide_plain_kernel.hip restates) for tests/test_resident_slide_plain_cpu.py: host code only, built
// with plain g++ under AddressSanitizer + UBSan.
//
//   slide_plain_admit_driver <in>      prints one line per window: slide_plain_admit's code
//
// <in>: one or more batches back to back.  One batch =
//   int32[12] nv_max nr_max np_max ns_max bw_max n_anchors pair_rule nr_new_max np_new_max ns_new_max has_drop 0
//   int64     n (>= 1)
//   int32     counts [n][4], r_idx [n][nr_max][2], p_idx [n][np_max], s_idx [n][ns_max][4]
//   int32     drop [n] (has_drop), r_counts [n], p_counts [n], s_counts [n], new r_idx [n][nr_new_max][2], new s_idx [n][ns_new_max][4]
// (a count under a capacity of 0 is in the file and not read, as by the kernel).  Every window's tables are handed over as copies of exactly
// the rows its counts name (no row where a new count is out of range), so that a read past a count is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_plain_admit.h"

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    v.shrink_to_fit();
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}
// rows [first, first + rows) of `width` values each, as a vector of exactly that size
template <class T>
static std::vector<T> rows_of(const std::vector<T>& v, size_t first, size_t rows, size_t width) {
    std::vector<T> out(v.begin() + first * width, v.begin() + (first + rows) * width);
    out.shrink_to_fit();
    return out;
}

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc != 2) { std::fprintf(stderr, "usage: %s <in>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int index = 0;; ++index) {
        int32_t head[12];
        const size_t got = std::fread(head, 4, 12, in);
        if (got == 0) break;
        int64_t n = 0;
        if (got != 12 || std::fread(&n, 8, 1, in) != 1 || n < 1) { std::fprintf(stderr, "batch %d: bad header\n", index); return 2; }
        const int nv_max = head[0], nr_max = head[1], np_max = head[2], ns_max = head[3], bw_max = head[4], n_anchors = head[5], pair_rule = head[6];
        const int nrn = head[7], npn = head[8], nsn = head[9];
        const bool has_drop = head[10] != 0;
        std::vector<int32_t> counts, r_idx, p_idx, s_idx, drop, r_counts, p_counts, s_counts, new_r_idx, new_s_idx;
        const size_t N = (size_t)n;
        if (!read_vec(in, counts, N * 4) || !read_vec(in, r_idx, N * nr_max * 2) || !read_vec(in, p_idx, N * np_max) || !read_vec(in, s_idx, N * ns_max * 4) ||
            !read_vec(in, drop, has_drop ? N : 0) || !read_vec(in, r_counts, N) || !read_vec(in, p_counts, N) || !read_vec(in, s_counts, N) ||
            !read_vec(in, new_r_idx, N * nrn * 2) || !read_vec(in, new_s_idx, N * nsn * 4)) {
            std::fprintf(stderr, "batch %d: short tables\n", index);
            return 2;
        }
        for (size_t i = 0; i < N; ++i) {
            const int nv = counts[i * 4], nr = counts[i * 4 + 1], np = counts[i * 4 + 2], ns = counts[i * 4 + 3];
            if (nr < 0 || nr > nr_max || np < 0 || np > np_max || ns < 0 || ns > ns_max) { std::fprintf(stderr, "batch %d window %zu: counts beyond the capacities\n", index, i); return 2; }
            const int32_t rc = nrn > 0 ? r_counts[i] : 0, pc = npn > 0 ? p_counts[i] : 0, sc = nsn > 0 ? s_counts[i] : 0;
            const bool counts_ok = rc >= 0 && rc <= nrn && pc >= 0 && pc <= npn && sc >= 0 && sc <= nsn;   // (no new row is handed over otherwise)
            const std::vector<int32_t> ri = rows_of(r_idx, i * nr_max, (size_t)nr, 2), pi = rows_of(p_idx, i * np_max, (size_t)np, 1), si = rows_of(s_idx, i * ns_max, (size_t)ns, 4);
            const std::vector<int32_t> xr = rows_of(new_r_idx, i * nrn, counts_ok ? (size_t)rc : 0, 2), xs = rows_of(new_s_idx, i * nsn, counts_ok ? (size_t)sc : 0, 4);
            const SlidePlainWindow sw{nv_max, nr_max, np_max, ns_max, bw_max, n_anchors, pair_rule, nv, nr, np, ns, ri.data(), pi.data(), si.data(),
                                      !has_drop || drop[i] != 0, nrn, rc, xr.data(), npn, pc, nsn, sc, xs.data()};
            std::printf("%d\n", slide_plain_admit(sw));
        }
    }
    std::fclose(in);
    return 0;
}
