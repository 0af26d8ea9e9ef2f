// Stand-alone driver of localization_amd/csrc/window_structure.cpp for tests/test_window_structure_cpu.py: host code only, built with
// plain g++ under AddressSanitizer + UBSan and under ThreadSanitizer.  It links against window_structure.cpp and nothing else of the product.
//
//   window_structure_driver --info                 prints "hw <std::thread::hardware_concurrency()>" and "lds <arrow3_lds_layout(100, 7).bytes>"
//   window_structure_driver <in> <out>             runs every pass of window_structure.h on each batch of <in>
//
// <in>: one or more batches back to back (several only to spare process starts: each batch is analysed on its own).  One batch =
//   int32[8]  nv_max nr_max np_max ns_max bw_max n_anchors has_off1 0
//   int64     n (>= 1)
//   the eight tables in window_tables.h's order and window_kernel.h's layout: poses counts r_val p_val s_val r_idx p_idx s_idx
// <out>: a list of sections, each  char name[16], int32 type (0: int32, 1: double, 2: int64), int64 count, data.  Per batch: "batch"
// {index, hw}, "check", "envelope"; when the counts fit the capacities "hash" {has_off1 as given, flipped}; and for a batch
// check_instances accepts the rest (only a validated batch may reach those passes, capi_window.cpp: validate_instances comes first).
// "tsched_bind": where bind_tree_sched puts TreeSched's 23 pointers in "tsched" (offsets in int32s), and the table length it returns.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "window_layouts.h"
#include "window_structure.h"

namespace {

struct Out {
    FILE* f;
    bool ok = true;
    void raw(const char* name, int32_t type, const void* p, size_t elem, int64_t count) {
        char nm[16] = {0};
        std::strncpy(nm, name, 15);
        ok = ok && std::fwrite(nm, 1, 16, f) == 16 && std::fwrite(&type, 4, 1, f) == 1 && std::fwrite(&count, 8, 1, f) == 1;
        if (count) ok = ok && std::fwrite(p, elem, (size_t)count, f) == (size_t)count;
    }
    void i32(const char* name, const std::vector<int32_t>& v) { raw(name, 0, v.data(), 4, (int64_t)v.size()); }
    void f64(const char* name, const std::vector<double>& v) { raw(name, 1, v.data(), 8, (int64_t)v.size()); }
    void i64(const char* name, const std::vector<int64_t>& v) { raw(name, 2, v.data(), 8, (int64_t)v.size()); }
};

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

void arrow_sizes(Out& out, const char* name, bool ok, const locamd::WinAux& A) {
    std::vector<int32_t> v{ok ? 1 : 0, A.arrow_list_cap, A.arrow_nb_max, A.arrow_jmax, A.arrow_jpmax};
    for (int k = 0; k < 16; ++k) v.push_back(A.arrow_jch[k]);
    for (int k = 0; k < 16; ++k) v.push_back(A.arrow_jpch[k]);
    out.i32(name, v);
}

}  // namespace

int main(int argc, char** argv) {
    using namespace locamd;
    const int hw = (int)std::thread::hardware_concurrency();
    if (argc == 2 && std::string(argv[1]) == "--info") {
        const WindowCaps c{100, 0, 0, 0, 0};
        std::printf("hw %d\nlds %zu\n", hw, arrow3_lds_layout(c.nv_max, 7).bytes);
        return 0;
    }
    if (argc != 3) { std::fprintf(stderr, "usage: %s --info | <in> <out>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Out out{std::fopen(argv[2], "wb")};
    if (!out.f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int32_t index = 0;; ++index) {
        int32_t head[8];
        const size_t got = std::fread(head, 4, 8, in);
        if (got == 0) break;   // the end of the input
        int64_t n = 0;
        if (got != 8 || std::fread(&n, 8, 1, in) != 1 || n < 1) { std::fprintf(stderr, "batch %d: bad header\n", index); return 2; }
        const WindowCaps c{head[0], head[1], head[2], head[3], head[4]};
        const int n_anchors = head[5];
        const bool has_off1 = head[6] != 0;
        if (c.nv_max < 0 || c.nr_max < 0 || c.np_max < 0 || c.ns_max < 0) { std::fprintf(stderr, "batch %d: bad capacities\n", index); return 2; }
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
        out.i32("batch", {index, hw});
        const int code = check_instances(c, n_anchors, b);
        out.i32("check", {code});
        out.i64("envelope", {(int64_t)envelope_blocks_max(c, b)});   // (documented to run on tables nobody has validated)
        bool counts_fit = true;
        for (size_t i = 0; i < N; ++i)
            counts_fit = counts_fit && counts[4 * i] >= 0 && counts[4 * i] <= c.nv_max && counts[4 * i + 1] >= 0 && counts[4 * i + 1] <= c.nr_max &&
                         counts[4 * i + 2] >= 0 && counts[4 * i + 2] <= c.np_max && counts[4 * i + 3] >= 0 && counts[4 * i + 3] <= c.ns_max;
        if (counts_fit) out.i64("hash", {(int64_t)hash_structure(c, has_off1, b), (int64_t)hash_structure(c, !has_off1, b)});
        if (code != 0) continue;
        out.i32("translation", {translation_only(c, n_anchors, b) ? 1 : 0});
        std::vector<int32_t> scan;
        for (int ordered = 1; ordered >= 0; --ordered) {
            bool chain = false, single_pairs = false, se3_pairs = false;
            chain_scan(c, b, ordered != 0, chain, single_pairs, se3_pairs);
            scan.push_back(chain); scan.push_back(single_pairs); scan.push_back(se3_pairs);
        }
        out.i32("chain_scan", scan);   // ordered {chain, single_pairs, se3_pairs}, then any order
        {
            WinAux A;
            const bool ok = build_tree_sched(c, has_off1, b, A);
            const TreeSched& t = A.tsched;
            out.i32("tree_ok", {ok ? 1 : 0});
            if (ok) {
                out.i32("tree_sizes", {t.nv, t.nr, t.np, t.ns, t.depth, t.nroots, t.nlev, t.max_se3_per_node, t.nu, t.max_r_per_node});
                out.i32("tsched", A.h_tsched);
                // bind_tree_sched on the host table: every pointer's offset from the base in TreeSched's order, then the length it reports
                TreeSched bound = t;
                const int32_t* base = A.h_tsched.data();
                const int64_t len = (int64_t)bind_tree_sched(bound, base);
                std::vector<int64_t> at;
                for (const int32_t* p : {bound.node, bound.par, bound.r_off, bound.r_list, bound.p_off, bound.p_list, bound.s_off, bound.s_list, bound.r_idx, bound.s_idx,
                                         bound.w_par, bound.w_height, bound.w_koff, bound.w_klist, bound.w_roff, bound.w_rlist, bound.w_poff, bound.w_plist, bound.w_soff,
                                         bound.w_slist, bound.w_kleaf, bound.w_ulist, bound.w_kpos}) at.push_back((int64_t)(p - base));
                at.push_back(len);
                out.i64("tsched_bind", at);
            }
        }
        {
            WinAux A;
            const bool ok = build_arrow_aux(c, b, A, false);
            arrow_sizes(out, "arrow", ok, A);
            if (ok) { out.i32("ahdr", A.h_ahdr); out.i32("arslot", A.h_arslot); out.f64("arec", A.h_arec); out.f64("aprec", A.h_aprec); }
            WinAux S;
            const bool ok_s = build_arrow_aux(c, b, S, true);
            arrow_sizes(out, "arrow_only", ok_s, S);
            out.i64("arrow_only_len", {(int64_t)S.h_arec.size(), (int64_t)S.h_aprec.size()});
        }
    }
    std::fclose(in);
    if (std::fclose(out.f) != 0 || !out.ok) { std::fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
