// Stand-alone driver of build_tree_groups (localization_amd/csrc/window_structure.cpp, option "forest_groups") for
// tests/test_forest_groups_cpu.py: host code only, built with plain g++ under AddressSanitizer + UBSan and under ThreadSanitizer.  It
// links against window_structure.cpp and nothing else of the product.
//
//   forest_groups_driver <in> <out>     groups each batch of <in> and writes what the kernel would be handed
//
// <in>: batches back to back in tests/host/window_structure_driver.cpp's format (int32[8] nv_max nr_max np_max ns_max bw_max n_anchors
//   has_off1 0, int64 n, the eight tables).  <out>: sections  char name[16], int32 type (0: int32, 2: int64), int64 count, data.  Per batch:
//   "batch" {index, hw}, "check" (check_instances: only a validated batch goes on), "tree_ok" (build_tree_sched on the whole batch) with
//   "tree_sizes" / "tsched" when it holds, "groups_ok", and for a grouped batch:
//   "n_groups"; "at" {sched_of's start, the tables' start, the block's length}; "block" (h_groups as a whole); "bind": per group the 23
//   offsets tree_sched_bind gives TreeSched's pointers inside the group's table, then the length it returns; "rep_sizes" / "rep_tables" /
//   "rep_len": build_tree_sched on a batch of the group's FIRST window alone — its ten sizes, its table, the table's length — which the
//   group's header and table must repeat int for int.
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    void i64(const char* name, const std::vector<int64_t>& v) { raw(name, 2, v.data(), 8, (int64_t)v.size()); }
};

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

std::vector<int32_t> sizes_of(const locamd::TreeSched& t) { return {t.nv, t.nr, t.np, t.ns, t.depth, t.nroots, t.nlev, t.max_se3_per_node, t.nu, t.max_r_per_node}; }

}  // namespace

int main(int argc, char** argv) {
    using namespace locamd;
    const int hw = (int)std::thread::hardware_concurrency();
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
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
        if (code != 0) continue;
        {
            WinAux A;
            const bool ok = build_tree_sched(c, has_off1, b, A);
            out.i32("tree_ok", {ok ? 1 : 0});
            if (ok) { out.i32("tree_sizes", sizes_of(A.tsched)); out.i32("tsched", A.h_tsched); }
        }
        WinAux A;
        A.h_groups.assign(7, 12345);   // (a refusal leaves no stale block behind)
        A.n_groups = 3;
        const bool ok = build_tree_groups(c, has_off1, b, A);
        out.i32("groups_ok", {ok ? 1 : 0});
        out.i32("n_groups", {A.n_groups});
        if (!ok) { out.i64("at", {0, 0, (int64_t)A.h_groups.size()}); continue; }
        out.i64("at", {(int64_t)A.groups_of_at, (int64_t)A.groups_tab_at, (int64_t)A.h_groups.size()});
        out.i32("block", A.h_groups);
        std::vector<int64_t> bind, rep_len;
        std::vector<int32_t> rep_sizes, rep_tables;
        std::vector<char> seen((size_t)A.n_groups, 0);
        const int32_t* of = A.h_groups.data() + A.groups_of_at;
        for (int g = 0; g < A.n_groups; ++g) {
            const int32_t* h = A.h_groups.data() + (size_t)g * kTreeGroupHdr;
            TreeSched ts{};
            tree_group_sizes(ts, h);
            // (offsets a test has not yet held to the block's length are not walked: the Python side checks `hdr` first on the block itself)
            if (h[10] < 0 || A.groups_tab_at + (size_t)h[10] + (size_t)(h[11] < 0 ? 0 : h[11]) > A.h_groups.size()) { std::fprintf(stderr, "batch %d: group %d lies outside the block\n", index, g); return 2; }
            const int32_t* base = A.h_groups.data() + A.groups_tab_at + h[10];
            const int64_t len = (int64_t)tree_sched_bind(ts, base);
            for (const int32_t* p : {ts.node, ts.par, ts.r_off, ts.r_list, ts.p_off, ts.p_list, ts.s_off, ts.s_list, ts.r_idx, ts.s_idx, ts.w_par, ts.w_height, ts.w_koff,
                                     ts.w_klist, ts.w_roff, ts.w_rlist, ts.w_poff, ts.w_plist, ts.w_soff, ts.w_slist, ts.w_kleaf, ts.w_ulist, ts.w_kpos}) bind.push_back((int64_t)(p - base));
            bind.push_back(len);
        }
        for (int64_t i = 0; i < n; ++i) {   // every group's first window, alone, through build_tree_sched
            const int g = of[i];
            if (g < 0 || g >= A.n_groups) { std::fprintf(stderr, "batch %d: sched_of[%lld] = %d\n", index, (long long)i, g); return 2; }
            if (seen[(size_t)g]) continue;
            seen[(size_t)g] = 1;
            const HostBatch one{1, poses.data() + (size_t)i * c.nv_max * 12, counts.data() + i * 4, r_val.data() + (size_t)i * c.nr_max * 5, p_val.data() + (size_t)i * c.np_max * 18,
                                s_val.data() + (size_t)i * c.ns_max * 48, r_idx.data() + (size_t)i * c.nr_max * 2, p_idx.data() + (size_t)i * c.np_max, s_idx.data() + (size_t)i * c.ns_max * 4};
            WinAux R;
            if (!build_tree_sched(c, has_off1, one, R)) { std::fprintf(stderr, "batch %d: build_tree_sched refuses the first window of group %d\n", index, g); return 2; }
            const std::vector<int32_t> s = sizes_of(R.tsched);
            rep_sizes.insert(rep_sizes.end(), s.begin(), s.end());
            rep_tables.insert(rep_tables.end(), R.h_tsched.begin(), R.h_tsched.end());
            rep_len.push_back((int64_t)R.h_tsched.size());
        }
        out.i64("bind", bind);
        out.i32("rep_sizes", rep_sizes);
        out.i32("rep_tables", rep_tables);
        out.i64("rep_len", rep_len);
    }
    std::fclose(in);
    if (std::fclose(out.f) != 0 || !out.ok) { std::fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
