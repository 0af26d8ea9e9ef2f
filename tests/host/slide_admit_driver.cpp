// Stand-alone driver of the resident slide's per-window admission rule (localization_amd/csrc/slide_admit.h: slide_admit, the one statement
// the device prologue of window_slide_kernel.hip restates) for tests/test_resident_slide_dev_cpu.py: host code only, built with plain g++ under
// AddressSanitizer + UBSan.  It holds the shared function to the batch-wide rule of loc_window_slide_resident (window_structure.cpp:
// slide_indices with apply = false, and slide_rows_translation_only), asked about ONE window at a time.
//
//   slide_admit_driver <in>      prints one line per window: "<slide_admit's code> <slide_indices' bad> <new rows translation-only>"
//
// <in>: one or more batches back to back, in slide_indices_driver.cpp's format.  One batch =
//   int32[8]  nv_max nr_max np_max bw_max n_anchors nr_new_max np_new_max has_drop
//   int64     n (>= 1)
//   int32     counts [n][4], r_idx [n][nr_max][2], p_idx [n][np_max]
//   int32     drop [n] (has_drop), r_counts [n], new r_idx [n][nr_new_max][2] (nr_new_max > 0), p_counts [n] (np_new_max > 0)
//   double    new_pose [n][12], new r_val [n][nr_new_max][5], new p_val [n][np_new_max][18]
// Every window's tables are handed over as copies of exactly the rows its counts name (no row where a new count is out of range), so that a
// read past a count is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_admit.h"
#include "window_structure.h"

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
        for (size_t i = 0; i < N; ++i) {
            std::vector<int32_t> cn = rows_of(counts, i, 1, 4);
            const int nv = cn[0], nr = cn[1], np = cn[2];
            if (nr < 0 || nr > c.nr_max || np < 0 || np > c.np_max) { std::fprintf(stderr, "batch %d window %zu: counts beyond the capacities\n", index, i); return 2; }
            const int32_t rc = nrn > 0 ? r_counts[i] : 0, pc = npn > 0 ? p_counts[i] : 0;
            const size_t r_rows = rc >= 0 && rc <= nrn ? (size_t)rc : 0, p_rows = pc >= 0 && pc <= npn ? (size_t)pc : 0;
            std::vector<int32_t> ri = rows_of(r_idx, i * c.nr_max, (size_t)nr, 2), pi = rows_of(p_idx, i * c.np_max, (size_t)np, 1);
            const std::vector<int32_t> xi = rows_of(new_r_idx, i * nrn, r_rows, 2);
            const std::vector<double> xv = rows_of(r_val, i * nrn, r_rows, 5), pv = rows_of(p_val, i * npn, p_rows, 18), pose = rows_of(new_pose, i, 1, 12);
            const bool drops = !has_drop || drop[i] != 0;
            const SlideWindow sw{c.nv_max, c.nr_max, c.np_max, c.bw_max, n_anchors, nv, nr, np, ri.data(), pi.data(), drops,
                                 nrn, rc, xi.data(), xv.data(), npn, pc, pv.data(), pose.data()};
            const int code = slide_admit(sw);
            // the batch-wide rule on this window alone (a batch of one: its row 0 is this window's)
            const int32_t one_drop = drops ? 1 : 0;
            const SlideRows rows{&one_drop, nrn, &rc, xi.data(), npn, &pc};
            const std::vector<int32_t> before_c = cn, before_r = ri, before_p = pi;
            const int bad = slide_indices(c, n_anchors, 1, cn.data(), ri.data(), pi.data(), rows, false).bad;
            if (cn != before_c || ri != before_r || pi != before_p) { std::fprintf(stderr, "batch %d window %zu: the check wrote to the mirror\n", index, i); return 3; }
            const bool translation = slide_rows_translation_only(1, rows, pose.data(), xv.data(), pv.data());
            std::printf("%d %d %d\n", code, bad, translation ? 1 : 0);
        }
    }
    std::fclose(in);
    return 0;
}
