// Stand-alone driver of localization_amd/csrc/arrow_pack.h for tests/test_arrow_pack_cpu.py: host code only, built with plain g++ under
// AddressSanitizer + UBSan.  It links against window_structure.cpp and nothing else of the product.
//
//   arrow_pack_driver --info     prints "gap <arrow_range_owner's refusal for a chain-chain range between rows that are no neighbours>"
//   arrow_pack_driver <in>       one line per batch of <in> (tests/host/window_structure_driver.cpp's input format)
//
// Per batch: arrow_window_structure and arrow_window_pack run WINDOW BY WINDOW, every table of a window in a heap block of exactly the size
// its counts name (a read or a write beyond a count trips the sanitizer), and their merged result is held to build_arrow_aux on the whole
// batch: the verdict with and without structure_only, h_ahdr, h_arslot (its slots from nv on: 0), h_arec, h_aprec byte for byte, arrow_nb_max,
// arrow_jmax, arrow_jpmax, arrow_jch, arrow_jpch, arrow_list_cap.  The line: "<verdict> <index of the first refused window, -1: none>
// <its ArrowRefusal> <batch-level refusal: 0 none, 1 arrow_batch_refused, 2 arrow3_fits> <nb_max> <jmax> <jpmax> <list_cap>".
// Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "arrow_pack.h"
#include "window_layouts.h"
#include "window_structure.h"

namespace {

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
std::vector<T> exact(const T* p, size_t count) { return std::vector<T>(p, p + count); }

int differ(int index, const char* what) {
    std::fprintf(stderr, "batch %d: %s differs from build_arrow_aux\n", index, what);
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc == 2 && std::string(argv[1]) == "--info") {
        const ArrowShape s = arrow_shape(10, 2);
        std::printf("gap %d\n", arrow_range_owner(s, 0, 3).refusal);
        return 0;
    }
    if (argc != 2) { std::fprintf(stderr, "usage: %s --info | <in>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int32_t index = 0;; ++index) {
        int32_t head[8];
        const size_t got = std::fread(head, 4, 8, in);
        if (got == 0) break;
        int64_t n = 0;
        if (got != 8 || std::fread(&n, 8, 1, in) != 1 || n < 1) { std::fprintf(stderr, "batch %d: bad header\n", index); return 2; }
        const WindowCaps c{head[0], head[1], head[2], head[3], head[4]};
        std::vector<double> poses, r_val, p_val, s_val;
        std::vector<int32_t> counts, r_idx, p_idx, s_idx;
        const size_t N = (size_t)n;
        if (!read_vec(in, poses, N * c.nv_max * 12) || !read_vec(in, counts, N * 4) || !read_vec(in, r_val, N * c.nr_max * 5) ||
            !read_vec(in, p_val, N * c.np_max * 18) || !read_vec(in, s_val, N * c.ns_max * 48) || !read_vec(in, r_idx, N * c.nr_max * 2) ||
            !read_vec(in, p_idx, N * c.np_max) || !read_vec(in, s_idx, N * c.ns_max * 4)) {
            std::fprintf(stderr, "batch %d: short tables\n", index);
            return 2;
        }
        const HostBatch b{n, poses.data(), counts.data(), r_val.data(), p_val.data(), s_val.data(), r_idx.data(), p_idx.data(), s_idx.data()};
        WinAux A, S;
        const bool want = build_arrow_aux(c, b, A, false), want_only = build_arrow_aux(c, b, S, true);

        // (a) window by window
        struct Window { std::vector<int32_t> cn, ri, pi, hdr, rslot; std::vector<double> rv, pv; };
        std::vector<Window> win(N);
        ArrowMaxima m = arrow_maxima_empty();
        long long first_bad = -1;
        int first_code = 0;
        for (size_t i = 0; i < N; ++i) {
            Window& x = win[i];
            x.cn = exact(counts.data() + i * 4, 4);
            const size_t nv = (size_t)x.cn[0], nr = (size_t)x.cn[1], np = (size_t)x.cn[2];
            x.ri = exact(r_idx.data() + i * c.nr_max * 2, nr * 2); x.rv = exact(r_val.data() + i * c.nr_max * 5, nr * 5);
            x.pi = exact(p_idx.data() + i * c.np_max, np); x.pv = exact(p_val.data() + i * c.np_max * 18, np * 18);
            x.hdr.assign(8, -77); x.rslot.assign(nv, -77);
            std::vector<int32_t> work(3 * nv, -77);
            const int code = arrow_window_structure(x.cn.data(), x.ri.data(), x.pi.data(), x.hdr.data(), x.rslot.data(), work.data(), m);
            if (code != kArrowOk) { first_bad = (long long)i; first_code = code; break; }   // (build_arrow_aux stops here as well)
        }
        int batch_refusal = 0;
        if (first_bad < 0) batch_refusal = arrow_batch_refused(m) ? 1 : !arrow3_fits(c, m.nb_max) ? 2 : 0;
        const bool got_verdict = first_bad < 0 && batch_refusal == 0;
        if (got_verdict != want || got_verdict != want_only) return differ(index, "the verdict");
        if (got_verdict) {
            if (A.arrow_nb_max != m.nb_max || A.arrow_jmax != m.jmax || A.arrow_jpmax != m.jpmax || A.arrow_list_cap != m.list_cap || S.arrow_list_cap != m.list_cap ||
                std::memcmp(A.arrow_jch, m.jch, sizeof(m.jch)) != 0 || std::memcmp(A.arrow_jpch, m.jpch, sizeof(m.jpch)) != 0) return differ(index, "a size");
            // (b) window by window, at the batch's sizes
            const int nchunk = (c.nv_max + 63) / 64;
            const size_t rec_per = arrow_rec_doubles(nchunk, m.jmax), prec_per = arrow_prec_doubles(nchunk, m.jpmax);
            if (A.h_arec.size() != N * rec_per || A.h_aprec.size() != N * prec_per || A.h_ahdr.size() != N * 8 || A.h_arslot.size() != N * c.nv_max) return differ(index, "a table's length");
            for (size_t i = 0; i < N; ++i) {
                const Window& x = win[i];
                const size_t nv = (size_t)x.cn[0];
                if (std::memcmp(x.hdr.data(), A.h_ahdr.data() + i * 8, 8 * sizeof(int32_t)) != 0 || std::memcmp(x.hdr.data(), S.h_ahdr.data() + i * 8, 8 * sizeof(int32_t)) != 0)
                    return differ(index, "hdr");
                if (nv && std::memcmp(x.rslot.data(), A.h_arslot.data() + i * c.nv_max, nv * sizeof(int32_t)) != 0) return differ(index, "rslot");
                for (size_t r = nv; r < (size_t)c.nv_max; ++r) if (A.h_arslot[i * c.nv_max + r] != 0) return differ(index, "rslot's tail");
                std::vector<double> rec(rec_per, 7.0), prec(prec_per, 7.0);
                std::vector<int32_t> work(2 * nv, -77);
                arrow_window_pack(x.cn.data(), x.hdr.data(), x.ri.data(), x.rv.data(), x.pi.data(), x.pv.data(), nchunk, m.jmax, m.jpmax, rec.data(), prec.data(), work.data());
                if (std::memcmp(rec.data(), A.h_arec.data() + i * rec_per, rec_per * sizeof(double)) != 0) return differ(index, "rec");
                if (std::memcmp(prec.data(), A.h_aprec.data() + i * prec_per, prec_per * sizeof(double)) != 0) return differ(index, "prec");
            }
        }
        std::printf("%d %lld %d %d %d %d %d %d\n", got_verdict ? 1 : 0, first_bad, first_code, batch_refusal, m.nb_max, m.jmax, m.jpmax, m.list_cap);
    }
    std::fclose(in);
    return 0;
}
