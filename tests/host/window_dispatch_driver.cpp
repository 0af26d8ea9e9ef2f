// Stand-alone driver of localization_amd/csrc/window_dispatch.cpp for tests/test_window_dispatch_cpu.py: host code only, built with plain
// g++ under AddressSanitizer + UBSan.  It links against window_dispatch.cpp and window_structure.cpp and nothing else of the product.
//
//   window_dispatch_driver <in> <out> [<texts>]
//
// <in>: one or more tables back to back.  One table = int64[3] {rule set, rows, columns}, then rows x columns int64 (row-major).
// <out>: per table rows x (results of the rule set) int64, row-major.
//   rule set 1, the solve kernel.  Columns: topology n chain_min env_chain_min_set env_chain_min has_off1 natural_order wave3 wave6 chain3
//     tree wave3_fits.  Results: pick_kernel, effective_chain_min, tree_min_batch.
//   rule set 2, the resident batch's covariance pass.  Columns: kind (CovKind's value) has_off1 nv_max n tree arrow3 cov_general
//     arrow_fits.  Results: cov_admitted, cov_stale with env_switches = cov_switches(), the same with env_switches = cov_switches() + 1,
//     cov_switches, arrow3_wanted.
//   rule set 3, what a resident entry refuses.  Columns: entry (ResidentEntry's value) handle resident mirror_valid solved pinfo_short topology
//     has_off1 has_pinfo pinfo_translation msg_set arg_failed.  Results: resident_refusal's code; its words go to <texts>, one line per row
//     (an empty line: go on).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_dispatch.h"

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s <in> <out> [<texts>]\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    FILE* texts = argc == 4 ? std::fopen(argv[3], "wb") : nullptr;
    if (argc == 4 && !texts) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    for (;;) {
        int64_t head[3];
        const size_t got = std::fread(head, 8, 3, in);
        if (got == 0) break;   // the end of the input
        const int64_t rule = head[0], rows = head[1], cols = head[2];
        if (got != 3 || rows < 0 || !((rule == 1 && cols == 12) || (rule == 2 && cols == 8) || (rule == 3 && cols == 12 && texts))) { std::fprintf(stderr, "bad table header\n"); return 2; }
        std::vector<int64_t> t((size_t)(rows * cols)), res;
        if (!t.empty() && std::fread(t.data(), 8, t.size(), in) != t.size()) { std::fprintf(stderr, "short table\n"); return 2; }
        for (int64_t i = 0; i < rows; ++i) {
            const int64_t* r = t.data() + i * cols;
            DispatchOpts o;
            DispatchFits f;
            if (rule == 1) {
                o.chain_min = r[2]; o.env_chain_min_set = r[3] != 0; o.env_chain_min = r[4]; o.has_off1 = r[5] != 0; o.natural_order = r[6] != 0;
                o.wave3 = r[7] != 0; o.wave6 = r[8] != 0; o.chain3 = r[9] != 0; o.tree = (int)r[10];
                f.wave3 = r[11] != 0; f.nv_max = 64;
                res.insert(res.end(), {(int64_t)pick_kernel(o, f, r[1], (int)r[0]), (int64_t)effective_chain_min(o), (int64_t)tree_min_batch(o)});
            } else if (rule == 3) {
                ResidentFacts x;
                x.handle = r[1] != 0; x.resident = r[2] != 0; x.mirror_valid = r[3] != 0; x.solved = r[4] != 0; x.pinfo_short = r[5] != 0; x.topology = (int)r[6];
                x.has_off1 = r[7] != 0; x.has_pinfo = r[8] != 0; x.pinfo_translation = r[9] != 0; x.msg_set = r[10] != 0;
                if (r[0] < 0 || r[0] >= kResidentEntries) { std::fprintf(stderr, "bad entry\n"); return 2; }
                const Refusal no = resident_refusal((ResidentEntry)r[0], x, (int)r[11]);
                res.push_back(no.code);
                std::fprintf(texts, "%s\n", no.text ? no.text : "");
            } else {
                const CovKind kind = (CovKind)r[0];
                o.has_off1 = r[1] != 0; f.nv_max = (int)r[2]; o.tree = (int)r[4]; o.arrow3 = (int)r[5]; o.cov_general = r[6] != 0; f.cov_arrow = r[7] != 0;
                const long long sw = cov_switches(o);
                res.insert(res.end(), {(int64_t)cov_admitted(o, f, r[3], kind), (int64_t)cov_stale(o, f, r[3], kind, sw), (int64_t)cov_stale(o, f, r[3], kind, sw + 1),
                                       (int64_t)sw, (int64_t)arrow3_wanted(o, f)});
            }
        }
        if (!res.empty() && std::fwrite(res.data(), 8, res.size(), out) != res.size()) { std::fprintf(stderr, "write failed\n"); return 2; }
    }
    std::fclose(in);
    if (std::fclose(out) != 0 || (texts && std::fclose(texts) != 0)) { std::fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
