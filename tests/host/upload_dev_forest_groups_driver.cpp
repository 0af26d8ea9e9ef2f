// Stand-alone driver of the host half of option "upload_dev_forest_groups" for tests/test_upload_dev_forest_groups_cpu.py: host code only, built
// with plain g++ under AddressSanitizer + UBSan.  It links against window_structure.cpp and nothing else of the product.
//
//   upload_dev_forest_groups_driver <in> <out> <bits> [<bits> ...]
//
// <in>: batches back to back in tests/host/window_structure_driver.cpp's format.  <out>: sections as tests/host/forest_groups_driver.cpp
// writes them.  Per batch:
//   "batch" {index}; "check" (check_instances: only a validated batch goes on);
//   "key_at" (n + 1 offsets) / "keys": every window's topology key, word by word from window_groups.h's topology_key_word;
//   "equal" [n][n]: topology_key_equal of every pair of windows (batches of at most 80 windows);
//   "a_ok" / "a_of" / "a_rep": part (a), group_windows;
//   per <bits>, a SERIAL model of window_groups_kernel.hip's rule on window_groups.h's hash — masked hash per window, the open-addressed table
//   with its bounded probe, the lowest window per hash, the verification against that window's key, the numbering by first appearance:
//   "m_flags_<bits>" {bits, bad_nv, collision, overflow, G} and "m_of_<bits>" / "m_rep_<bits>";
//   "full" {ok, n_groups, of_at, tab_at} + "full_block": build_tree_groups on the batch;
//   "part_b" {ok, n_groups, of_at, tab_at} + "part_b_block": build_tree_groups_block from the COMPACT batch of the representatives (their counts
//   and used rows alone, everything else poisoned) and of[] — the grouping taken from the 64-bit model, which groups whatever nv is;
//   "chain" {chain_scan(ordered = false) on the batch, on the compact batch of the representatives}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "window_groups.h"
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

struct Tables {
    locamd::WindowCaps c;
    const int32_t *counts, *r_idx, *p_idx, *s_idx;
    const int32_t* cn(int64_t i) const { return counts + i * 4; }
    const int32_t* r(int64_t i) const { return r_idx + (size_t)i * c.nr_max * 2; }
    const int32_t* p(int64_t i) const { return p_idx + (size_t)i * c.np_max; }
    const int32_t* s(int64_t i) const { return s_idx + (size_t)i * c.ns_max * 4; }
    bool equal(int64_t i, int64_t j) const { return locamd::topology_key_equal(cn(i), r(i), p(i), s(i), cn(j), r(j), p(j), s(j)); }
};

// the device's rule, one window after the other
struct Model { bool bad_nv = false, collision = false, overflow = false; int32_t G = 0; std::vector<int32_t> of, rep; };
Model model(const Tables& t, int64_t n, int bits) {
    using namespace locamd;
    Model m;
    const uint64_t slots = groups_table_slots(n), mask = slots - 1;
    std::vector<uint64_t> hash((size_t)n, 0), tab_key((size_t)slots, 0);
    std::vector<uint32_t> tab_inv((size_t)slots, 0);
    for (int64_t b = 0; b < n; ++b) {   // hash and insert
        const int32_t nv = t.cn(b)[0];
        if (nv < 2 || nv > 64) m.bad_nv = true;   // (the kernel does not hash such a window; the model does, to be able to group a refused batch)
        const uint64_t key = groups_hash_masked(topology_key_hash(t.cn(b), t.r(b), t.p(b), t.s(b)), bits);
        hash[(size_t)b] = key;
        uint64_t slot = groups_hash_slot(key, slots);
        for (uint64_t i = 0; i < slots; ++i) {
            if (tab_key[slot] == 0) tab_key[slot] = key;
            if (tab_key[slot] == key) { if (~(uint32_t)b > tab_inv[slot]) tab_inv[slot] = ~(uint32_t)b; break; }
            slot = (slot + 1) & mask;
        }
    }
    std::vector<int64_t> rep0((size_t)n);
    for (int64_t b = 0; b < n; ++b) {   // look up and verify
        const uint64_t key = hash[(size_t)b];
        uint64_t slot = groups_hash_slot(key, slots);
        bool found = false;
        for (uint64_t i = 0; i < slots; ++i) {
            if (tab_key[slot] == key) { found = true; break; }
            if (tab_key[slot] == 0) break;
            slot = (slot + 1) & mask;
        }
        int64_t r = b;
        if (found && (uint64_t)(uint32_t)~tab_inv[slot] <= (uint64_t)b) r = (int64_t)(uint32_t)~tab_inv[slot];
        else m.overflow = true;
        if (r != b && !t.equal(b, r)) m.collision = true;
        rep0[(size_t)b] = r;
        if (r == b) ++m.G;
    }
    m.of.assign((size_t)n, 0);   // number
    for (int64_t b = 0; b < n; ++b) if (rep0[(size_t)b] == b) { m.of[(size_t)b] = (int32_t)m.rep.size(); m.rep.push_back((int32_t)b); }
    for (int64_t b = 0; b < n; ++b) if (rep0[(size_t)b] != b) m.of[(size_t)b] = m.of[(size_t)rep0[(size_t)b]];
    return m;
}

}  // namespace

int main(int argc, char** argv) {
    using namespace locamd;
    if (argc < 4) { std::fprintf(stderr, "usage: %s <in> <out> <bits> [<bits> ...]\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Out out{std::fopen(argv[2], "wb")};
    if (!out.f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<int> all_bits;
    for (int k = 3; k < argc; ++k) all_bits.push_back(std::atoi(argv[k]));
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
        // (the value tables are not handed on: nothing here may read them)
        const HostBatch b{n, nullptr, counts.data(), nullptr, nullptr, nullptr, r_idx.data(), p_idx.data(), s_idx.data()};
        const Tables t{c, counts.data(), r_idx.data(), p_idx.data(), s_idx.data()};
        out.i32("batch", {index});
        const int code = check_instances(c, n_anchors, b);
        out.i32("check", {code});
        if (code != 0) continue;
        {   // the key, word by word
            std::vector<int64_t> at{0};
            std::vector<int32_t> keys;
            for (int64_t i = 0; i < n; ++i) {
                const long long nw = topology_key_words(t.cn(i));
                for (long long k = 0; k < nw; ++k) keys.push_back(topology_key_word(t.cn(i), t.r(i), t.p(i), t.s(i), k));
                at.push_back((int64_t)keys.size());
            }
            out.i64("key_at", at);
            out.i32("keys", keys);
            if (n <= 80) {
                std::vector<int32_t> eq(N * N);
                for (int64_t i = 0; i < n; ++i) for (int64_t j = 0; j < n; ++j) eq[(size_t)(i * n + j)] = t.equal(i, j) ? 1 : 0;
                out.i32("equal", eq);
            }
        }
        {   // part (a)
            std::vector<int32_t> of;
            std::vector<int64_t> rep;
            const bool ok = group_windows(c, b, of, rep);
            out.i32("a_ok", {ok ? 1 : 0});
            if (ok) { out.i32("a_of", of); out.i64("a_rep", rep); }
        }
        for (int bits : all_bits) {
            const Model m = model(t, n, bits);
            char name[16];
            std::snprintf(name, sizeof(name), "m_flags_%d", bits);
            out.i32(name, {bits, m.bad_nv ? 1 : 0, m.collision ? 1 : 0, m.overflow ? 1 : 0, m.G});
            std::snprintf(name, sizeof(name), "m_of_%d", bits);
            out.i32(name, m.of);
            std::snprintf(name, sizeof(name), "m_rep_%d", bits);
            out.i32(name, m.rep);
        }
        WinAux F;
        const bool full_ok = build_tree_groups(c, has_off1, b, F);
        out.i64("full", {full_ok ? 1 : 0, F.n_groups, (int64_t)F.groups_of_at, (int64_t)F.groups_tab_at});
        out.i32("full_block", F.h_groups);
        // the compact batch of the representatives: counts and used rows, everything else poisoned
        const Model m = model(t, n, 64);
        if (m.collision || m.overflow) { std::fprintf(stderr, "batch %d: the 64-bit model reports a collision or an overflow\n", index); return 2; }
        const size_t G = m.rep.size();
        std::vector<int32_t> cc(G * 4), cr(G * c.nr_max * 2, INT32_MIN), cp(G * c.np_max, INT32_MAX), cs(G * c.ns_max * 4, INT32_MIN);
        for (size_t g = 0; g < G; ++g) {
            const int64_t i = m.rep[g];
            std::memcpy(cc.data() + g * 4, t.cn(i), 4 * sizeof(int32_t));
            if (t.cn(i)[1]) std::memcpy(cr.data() + g * c.nr_max * 2, t.r(i), (size_t)t.cn(i)[1] * 2 * sizeof(int32_t));
            if (t.cn(i)[2]) std::memcpy(cp.data() + g * c.np_max, t.p(i), (size_t)t.cn(i)[2] * sizeof(int32_t));
            if (t.cn(i)[3]) std::memcpy(cs.data() + g * c.ns_max * 4, t.s(i), (size_t)t.cn(i)[3] * 4 * sizeof(int32_t));
        }
        const HostBatch reps{(int64_t)G, nullptr, cc.data(), nullptr, nullptr, nullptr, cr.data(), cp.data(), cs.data()};
        WinAux P;
        P.h_groups.assign(7, 12345);   // (a refusal leaves no stale block behind)
        P.n_groups = 3;
        const bool part_ok = build_tree_groups_block(c, has_off1, reps, n, m.of.data(), P);
        out.i64("part_b", {part_ok ? 1 : 0, P.n_groups, (int64_t)P.groups_of_at, (int64_t)P.groups_tab_at});
        out.i32("part_b_block", P.h_groups);
        bool chain_full = false, chain_reps = false, sp = false, se = false;
        chain_scan(c, b, false, chain_full, sp, se);
        chain_scan(c, reps, false, chain_reps, sp, se);
        out.i32("chain", {chain_full ? 1 : 0, chain_reps ? 1 : 0});
    }
    std::fclose(in);
    if (std::fclose(out.f) != 0 || !out.ok) { std::fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
