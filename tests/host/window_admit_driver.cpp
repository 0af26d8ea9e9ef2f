// Stand-alone driver of the per-window admission and structure rule of loc_window_upload_dev (localization_amd/csrc/window_admit.h: window_admit
// and window_structure_flags, the two functions window_admit_kernel.hip restates lane-parallel) for tests/test_window_admit_cpu.py: host code
// only, built with plain g++ under AddressSanitizer + UBSan together with window_structure.cpp and window_dispatch.cpp.
//
//   window_admit_driver <in>
//
// <in>: one or more batches back to back, in the format of tests/_window_structure_model.Batch.write:
//   int32[8] nv_max nr_max np_max ns_max bw_max n_anchors has_off1 0;  int64 n (>= 1);
//   poses [n][nv_max][12] f64, counts [n][4] i32, r_val [n][nr_max][5], p_val [n][np_max][18], s_val [n][ns_max][48] f64,
//   r_idx [n][nr_max][2], p_idx [n][np_max], s_idx [n][ns_max][4] i32
// Per batch the two functions run window by window — every window's tables handed over as copies of EXACTLY the rows its counts name (none
// where a count is out of range), so that a read past a count is an AddressSanitizer report — and are reduced with window_record_add.  The
// result is held to window_structure.cpp's batch passes on the same tables, here: check_instances (the code of the lowest refused window),
// and for an admitted batch chain_scan(ordered = true) (the pair verdicts where the batch is a chain), translation_only with both values of
// skip_prior_diagonal and max_anchor_referenced; and topology_from_flags to batch_topology for every combination of the wave6 fit, the wave6_se3
// fit and structured_pinfo, options "tree" and "arrow3" at 0.  A difference is printed to stderr and the exit status is 1.
// stdout, one line per batch: first_bad code and_bits or_bits max_anchor | the eight verdicts (an admitted batch; index = wave6 + 2 wave6_se3
// + 4 structured) | every window's code
#include <cstdint>
#include <cstdio>
#include <vector>

#include "window_admit.h"
#include "window_dispatch.h"
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
    int differences = 0;
    for (int index = 0;; ++index) {
        int32_t head[8];
        const size_t got = std::fread(head, 4, 8, in);
        if (got == 0) break;
        int64_t n = 0;
        if (got != 8 || std::fread(&n, 8, 1, in) != 1 || n < 1) { std::fprintf(stderr, "batch %d: bad header\n", index); return 2; }
        const WindowCaps c{head[0], head[1], head[2], head[3], head[4]};
        const int n_anchors = head[5];
        const size_t N = (size_t)n;
        std::vector<double> poses, r_val, p_val, s_val;
        std::vector<int32_t> counts, r_idx, p_idx, s_idx;
        if (!read_vec(in, poses, N * c.nv_max * 12) || !read_vec(in, counts, N * 4) || !read_vec(in, r_val, N * c.nr_max * 5) || !read_vec(in, p_val, N * c.np_max * 18) ||
            !read_vec(in, s_val, N * c.ns_max * 48) || !read_vec(in, r_idx, N * c.nr_max * 2) || !read_vec(in, p_idx, N * c.np_max) || !read_vec(in, s_idx, N * c.ns_max * 4)) {
            std::fprintf(stderr, "batch %d: short tables\n", index);
            return 2;
        }
        const WindowAdmitCaps ac{c.nv_max, c.nr_max, c.np_max, c.ns_max, c.bw_max, n_anchors};
        WindowAdmitRecord rec = window_record_empty();
        std::vector<int> codes(N);
        for (size_t i = 0; i < N; ++i) {
            const int32_t* cn = counts.data() + i * 4;
            const bool in_range = cn[0] >= 0 && cn[0] <= c.nv_max && cn[1] >= 0 && cn[1] <= c.nr_max && cn[2] >= 0 && cn[2] <= c.np_max && cn[3] >= 0 && cn[3] <= c.ns_max;
            const size_t nv = in_range ? cn[0] : 0, nr = in_range ? cn[1] : 0, np = in_range ? cn[2] : 0, ns = in_range ? cn[3] : 0;   // (no row is handed over otherwise)
            const std::vector<int32_t> cw = rows_of(counts, i, 1, 4), ri = rows_of(r_idx, i * c.nr_max, nr, 2), pi = rows_of(p_idx, i * c.np_max, np, 1),
                                       si = rows_of(s_idx, i * c.ns_max, ns, 4);
            const int code = window_admit(ac, cw.data(), ri.data(), pi.data(), si.data());
            uint64_t word = 0;
            if (code == kWinAdmitOk) {
                const std::vector<double> X = rows_of(poses, i * c.nv_max, nv, 12), rv = rows_of(r_val, i * c.nr_max, nr, 5), pv = rows_of(p_val, i * c.np_max, np, 18);
                word = window_structure_flags(ac, cw.data(), ri.data(), pi.data(), si.data(), X.data(), rv.data(), pv.data());
            }
            codes[i] = code;
            window_record_add(rec, (long long)i, code, word);
        }
        // ---- window_structure.cpp on the same batch ----
        const HostBatch b{n, poses.data(), counts.data(), r_val.data(), p_val.data(), s_val.data(), r_idx.data(), p_idx.data(), s_idx.data()};
        const int host_code = check_instances(c, n_anchors, b);
        const bool admitted = rec.first_bad == kWinNoneRefused;
        if (host_code != rec.code || admitted != (host_code == 0)) {
            std::fprintf(stderr, "batch %d: check_instances %d, window_admit %d (window %lld)\n", index, host_code, rec.code, rec.first_bad);
            ++differences;
        }
        int verdicts[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
        if (admitted && host_code == 0) {
            const WindowBatchFlags f = window_batch_flags(rec);
            bool chain = false, single_pairs = false, se3_pairs = false;
            chain_scan(c, b, true, chain, single_pairs, se3_pairs);
            const bool t0 = translation_only(c, n_anchors, b, false), t1 = translation_only(c, n_anchors, b, true);
            const int max_anchor = max_anchor_referenced(c, n, counts.data(), r_idx.data());
            if (chain != f.chain || (chain && (single_pairs != f.single_pairs || se3_pairs != f.se3_pairs)) || t0 != f.translation_only || t1 != f.translation_only_skip ||
                max_anchor != rec.max_anchor) {
                std::fprintf(stderr, "batch %d: host chain %d single %d se3 %d translation %d / %d anchor %d; flags %d %d %d %d / %d anchor %d\n", index, chain, single_pairs, se3_pairs,
                             t0, t1, max_anchor, f.chain, f.single_pairs, f.se3_pairs, f.translation_only, f.translation_only_skip, rec.max_anchor);
                ++differences;
            }
            for (int k = 0; k < 8; ++k) {
                DispatchOpts o;
                o.tree = 0; o.arrow3 = 0;   // (batch_topology cannot answer TREE or ARROW3)
                if (k & 4) { o.pinfo_structured = true; o.has_pinfo = true; o.pinfo_translation = true; }
                DispatchFits fits = dispatch_fits(c);
                fits.wave6 = (k & 1) != 0; fits.wave6_se3 = (k & 2) != 0;
                WinAux aux;
                const int host_kind = batch_topology(c, o, fits, n_anchors, b, aux, nullptr).kind;
                verdicts[k] = topology_from_flags(o, fits, f);
                if (structured_pinfo(o) != ((k & 4) != 0) || host_kind != verdicts[k]) {
                    std::fprintf(stderr, "batch %d, combination %d: batch_topology %d, topology_from_flags %d\n", index, k, host_kind, verdicts[k]);
                    ++differences;
                }
            }
        }
        std::printf("%lld %d %u %u %d |", admitted ? -1ll : rec.first_bad, rec.code, rec.and_bits, rec.or_bits, rec.max_anchor);
        for (int k = 0; k < 8; ++k) std::printf(" %d", verdicts[k]);
        std::printf(" |");
        for (size_t i = 0; i < N; ++i) std::printf(" %d", codes[i]);
        std::printf("\n");
    }
    std::fclose(in);
    return differences ? 1 : 0;
}
