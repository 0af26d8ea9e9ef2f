// Stand-alone driver of the block layouts of localization_amd/csrc/window_tables.h and of window_structure.cpp's anchor scan for
// tests/test_window_blocks_cpu.py: host code only, built with plain g++ under AddressSanitizer + UBSan.  It links against
// window_structure.cpp and nothing else of the product.
//
//   window_blocks_driver <in> <out>
//
// <in>: one or more tables back to back, each behind int64[3] {rule set, rows, columns}.  <out>: int64, row-major.
//   rule set 1, the layouts.  rows x 8 int64: N nv_max nr_max np_max ns_max npair_max nr_new_max np_new_max.  Per row 50 results:
//     covariance_layout(caps, N, npair_max)                 pre[0..5] tab[0..7] end   (npair_max = 0: the plain call, pre[3..5] = 0)
//     marginal_prior_layout(caps, N)                        pre[0..6] tab[0..7] end
//     resident_pairs_layout(N, npair_max)                   pre[0..1] end
//     slide_inputs_layout(N, nr_new_max, np_new_max)        pre[0..6] end
//     slide_marginal_layout(N)                              pre[kMDrop .. kMShift] end
//   rule set 2, the anchor scan of one batch.  rows = n, columns = nr_max; then int32 counts [n][4] and int32 r_idx [n][nr_max][2], each in an
//     allocation of exactly its size.  One result: max_anchor_referenced.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_structure.h"
#include "window_tables.h"

static void put(std::vector<int64_t>& res, const locamd::BlockLayout& L, int n_pre, bool tables) {
    for (int k = 0; k < n_pre; ++k) res.push_back((int64_t)L.pre[k]);
    for (int t = 0; t < locamd::kWindowTables && tables; ++t) res.push_back((int64_t)L.tab[t]);
    res.push_back((int64_t)L.end);
}

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (;;) {
        int64_t head[3];
        const size_t got = std::fread(head, 8, 3, in);
        if (got == 0) break;   // the end of the input
        const int64_t rule = head[0], rows = head[1], cols = head[2];
        if (got != 3 || rows < 0 || cols < 0 || !((rule == 1 && cols == 8) || rule == 2)) { std::fprintf(stderr, "bad table header\n"); return 2; }
        std::vector<int64_t> res;
        if (rule == 1) {
            std::vector<int64_t> t((size_t)(rows * cols));
            if (!t.empty() && std::fread(t.data(), 8, t.size(), in) != t.size()) { std::fprintf(stderr, "short table\n"); return 2; }
            for (int64_t i = 0; i < rows; ++i) {
                const int64_t* r = t.data() + i * cols;
                const size_t N = (size_t)r[0];
                const WindowCaps c{(int)r[1], (int)r[2], (int)r[3], (int)r[4], 0};
                put(res, covariance_layout(c, N, (size_t)r[5]), 6, true);
                put(res, marginal_prior_layout(c, N), 7, true);
                put(res, resident_pairs_layout(N, (size_t)r[5]), 2, false);
                put(res, slide_inputs_layout(N, (size_t)r[6], (size_t)r[7]), 7, false);
                const BlockLayout M = slide_marginal_layout(N);
                for (int k : {kMDrop, kMSlot, kMRank, kMStatus, kMPrior, kMGrad, kMShift}) res.push_back((int64_t)M.pre[k]);
                res.push_back((int64_t)M.end);
            }
        } else {
            std::vector<int32_t> counts((size_t)rows * 4), r_idx((size_t)(rows * cols) * 2);
            if ((!counts.empty() && std::fread(counts.data(), 4, counts.size(), in) != counts.size()) ||
                (!r_idx.empty() && std::fread(r_idx.data(), 4, r_idx.size(), in) != r_idx.size())) { std::fprintf(stderr, "short batch\n"); return 2; }
            const WindowCaps c{1, (int)cols, 0, 0, 0};
            res.push_back(max_anchor_referenced(c, rows, counts.data(), r_idx.data()));
        }
        if (!res.empty() && std::fwrite(res.data(), 8, res.size(), out) != res.size()) { std::fprintf(stderr, "write failed\n"); return 2; }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) { std::fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
