// Stand-alone driver of the dispatch rules behind option "forest_groups_covariance" (localization_amd/csrc/window_dispatch.cpp, the launcher's
// header bounds in window_layouts.h) for tests/test_forest_groups_covariance_cpu.py: host code only, built with plain g++ under
// AddressSanitizer + UBSan.  It links against window_dispatch.cpp and window_structure.cpp and nothing else of the product.
//
//   forest_groups_covariance_driver <section>      section: verdicts | admission | keyed | bounds
//
// The driver builds its batches itself (key-frame stars with one anchor range per pose), states what it expects next to every call, prints
// "<section>: <n> checks" and exits 0; the first expectation that fails is reported on stderr with its line, exit status 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/localization_amd.h"
#include "window_dispatch.h"
#include "window_layouts.h"

namespace {

using namespace locamd;

long g_checks = 0;
#define EXPECT(cond) do { ++g_checks; if (!(cond)) { std::fprintf(stderr, "line %d: expected %s\n", __LINE__, #cond); return 1; } } while (0)

struct Batch {
    WindowCaps c;
    int64_t n;
    std::vector<double> poses, r_val, p_val, s_val;
    std::vector<int32_t> counts, r_idx, p_idx, s_idx;
    Batch(int64_t n_, WindowCaps c_) : c(c_), n(n_) {
        const size_t N = (size_t)n;
        poses.assign(N * c.nv_max * 12, 0.0); r_val.assign(N * c.nr_max * 5, 0.0); p_val.assign(N * c.np_max * 18, 0.0); s_val.assign(N * c.ns_max * 48, 0.0);
        counts.assign(N * 4, 0); r_idx.assign(N * c.nr_max * 2, INT32_MIN); p_idx.assign(N * c.np_max, INT32_MIN); s_idx.assign(N * c.ns_max * 4, INT32_MIN);
        for (size_t k = 0; k < N * c.nv_max; ++k) poses[k * 12] = poses[k * 12 + 4] = poses[k * 12 + 8] = 1.0;
    }
    void add_range(int64_t i, int v0, int v1) { int32_t& e = counts[i * 4 + 1]; int32_t* r = r_idx.data() + ((size_t)i * c.nr_max + e) * 2; r[0] = v0; r[1] = v1; r_val[((size_t)i * c.nr_max + e) * 5 + 1] = 1.0; ++e; }
    void add_se3(int64_t i, int vi, int vj, int robust = 1) { int32_t& e = counts[i * 4 + 3]; int32_t* s = s_idx.data() + ((size_t)i * c.ns_max + e) * 4; s[0] = vi; s[1] = vj; s[2] = robust; s[3] = 0; ++e; }
    // a key-frame star: pose k hangs on the last key before it (every `every`-th pose is a key) by an EdgeSE3 and ranges one anchor
    void star(int64_t i, int nv, int every, int anchor) {
        counts[i * 4] = nv;
        for (int k = 1; k < nv; ++k) add_se3(i, k, (k - 1) / every * every);
        for (int k = 0; k < nv; ++k) add_range(i, k, -1 - (anchor + k) % 4);
    }
    // a chain: pose k hangs on pose k - 1
    void chain(int64_t i, int nv) { star(i, nv, 1, 0); }
    HostBatch host() const { return HostBatch{n, poses.data(), counts.data(), r_val.data(), p_val.data(), s_val.data(), r_idx.data(), p_idx.data(), s_idx.data()}; }
};

const WindowCaps kCaps{64, 70, 2, 64, 63};
const PairTables kNoPairs{0, nullptr, nullptr};

// six windows of two topologies (9 and 8 poses), every window ranging other anchors
Batch mixed_batch() {
    Batch b(6, kCaps);
    for (int i = 0; i < 6; ++i) b.star(i, i % 2 ? 8 : 9, 4, i);
    return b;
}
Batch one_topology_batch() {
    Batch b(6, kCaps);
    for (int i = 0; i < 6; ++i) b.star(i, 9, 4, 0);
    return b;
}

DispatchOpts options(bool groups, bool groups_cov, bool general, int tree = -1, long long chain_min = 1, bool pinfo = false) {
    DispatchOpts o;
    o.forest_groups = groups; o.forest_groups_cov = groups_cov; o.cov_general = general; o.tree = tree; o.chain_min = chain_min; o.has_pinfo = pinfo;
    return o;
}

int verdicts() {
    const DispatchFits f = dispatch_fits(kCaps);
    EXPECT(f.cov_envelope && f.cov_chain);
    const Batch mixed = mixed_batch(), one = one_topology_batch();
    Batch cyc = mixed_batch(), dbl = mixed_batch(), tiny = mixed_batch(), chains(6, kCaps);
    cyc.add_range(2, 1, 2);              // 1 and 2 both hang on 0: a triangle in one window
    dbl.add_se3(3, 0, 1);                // a second EdgeSE3 on the pair (1, 0)
    tiny.counts[5 * 4] = 1; tiny.counts[5 * 4 + 1] = 1; tiny.counts[5 * 4 + 3] = 0;   // a window of one pose
    for (int i = 0; i < 6; ++i) chains.chain(i, 5 + i);
    for (int groups = 0; groups < 2; ++groups)
        for (int gcov = 0; gcov < 2; ++gcov)
            for (int general = 0; general < 2; ++general)
                for (int tree : {-1, 0, 2})
                    for (long long chain_min : {1ll, 7ll})
                        for (int pinfo = 0; pinfo < 2; ++pinfo) {
                            const DispatchOpts o = options(groups, gcov, general, tree, chain_min, pinfo);
                            const CovKind rest = general ? CovKind::Envelope : CovKind::None;
                            const bool forest = tree != 0 && chain_min == 1 && !pinfo;
                            const bool served = groups && gcov && forest && tree != 2;
                            WinAux own;
                            CovVerdict v = covariance_kind(kCaps, o, f, 4, mixed.host(), kNoPairs, own, nullptr);
                            EXPECT(v.kind == (served ? CovKind::ForestGroupsOwn : rest));
                            EXPECT(v.need_upload == served && (!served || (own.n_groups == 2 && !own.h_groups.empty())));
                            EXPECT(v.kind != CovKind::Envelope || v.env_blocks > 0);
                            // what build_tree_groups refuses stays with the envelope pass or the refusal
                            for (const Batch* bad : {&cyc, &dbl, &tiny}) {
                                WinAux a;
                                v = covariance_kind(kCaps, o, f, 4, bad->host(), kNoPairs, a, nullptr);
                                EXPECT(v.kind == rest && !v.need_upload);
                            }
                            // a one-topology batch and a chain batch keep their pass
                            WinAux a, c;
                            v = covariance_kind(kCaps, o, f, 4, one.host(), kNoPairs, a, nullptr);
                            EXPECT(v.kind == (forest ? CovKind::ForestOwn : rest) && v.need_upload == forest);
                            v = covariance_kind(kCaps, o, f, 4, chains.host(), kNoPairs, c, nullptr);
                            EXPECT(v.kind == (pinfo ? rest : CovKind::Chain6) && !v.need_upload);
                            // the solve's rule, stated once: batch_topology groups the batch exactly when the covariance would (but for its own option)
                            WinAux s;
                            const int topology = batch_topology(kCaps, o, f, 4, mixed.host(), s, nullptr).kind;
                            EXPECT((topology == LOC_WINDOW_KERNEL_TREE_GROUPS) == (groups && forest && tree != 2));
                            EXPECT(forest_groups_wanted(o, kCaps, mixed.n) == (groups && forest && tree != 2));
                        }
    // a handle of longer windows: never grouped
    WindowCaps wide = kCaps; wide.nv_max = 65;
    EXPECT(!forest_groups_wanted(options(true, true, false), wide, 6));
    return 0;
}

int admission() {
    const CovKind news[2] = {CovKind::ForestGroups, CovKind::ForestGroupsOwn};
    long long seen_off = -1;
    for (int groups = 0; groups < 2; ++groups)
        for (int gcov = 0; gcov < 2; ++gcov)
            for (int general = 0; general < 2; ++general)
                for (int tree : {-1, 0, 2})
                    for (int64_t n : {255, 256})
                        for (int off1 = 0; off1 < 2; ++off1)
                            for (int pinfo = 0; pinfo < 2; ++pinfo)
                                for (int nv_max : {64, 65})
                                    for (int arrow3 : {-1, 1}) {
                                        DispatchOpts o = options(groups, gcov, general, tree, -1, pinfo);   // (the default threshold: forests from 256 windows on)
                                        o.has_off1 = off1; o.arrow3 = arrow3;
                                        DispatchFits f; f.nv_max = nv_max; f.cov_arrow = true;
                                        const bool want = groups && gcov && tree == -1 && n >= 256 && !off1 && !pinfo && nv_max <= 64;
                                        for (CovKind k : news) {
                                            EXPECT(cov_admitted(o, f, n, k) == want);
                                            EXPECT(cov_stale(o, f, n, k, cov_switches(o)) == (general && !off1 && !want));
                                        }
                                        EXPECT(resident_groups_covariance(o, f, n, true) == (want ? CovKind::ForestGroups : CovKind::Unclassified));
                                        EXPECT(resident_groups_covariance(o, f, n, false) == CovKind::Unclassified);
                                        // the old kinds and the switch word: as with both options off, but for the one new bit
                                        DispatchOpts base = o; base.forest_groups = false; base.forest_groups_cov = false;
                                        for (int k = -1; k <= 6; ++k) {
                                            EXPECT(cov_admitted(o, f, n, (CovKind)k) == cov_admitted(base, f, n, (CovKind)k));
                                            EXPECT(cov_stale(o, f, n, (CovKind)k, cov_switches(o)) == cov_stale(base, f, n, (CovKind)k, cov_switches(base)));
                                        }
                                        const long long bit = cov_switches(o) ^ cov_switches(base);
                                        EXPECT(bit == (groups && gcov ? 1ll << 57 : 0) && (cov_switches(base) & (1ll << 57)) == 0);
                                        // an Envelope verdict taken before the option was switched on is out of date afterwards, and only then
                                        EXPECT(cov_stale(o, f, n, CovKind::Envelope, cov_switches(base)) == (groups && gcov));
                                        if (groups && gcov) seen_off = cov_switches(base);
                                    }
    EXPECT(seen_off >= 0);
    EXPECT((int)CovKind::Envelope == 6 && (int)CovKind::ForestGroups == 7 && (int)CovKind::ForestGroupsOwn == 8);   // appended: the recorded grid's values stay
    EXPECT(cov_public_kind(CovKind::ForestGroups) == LOC_WINDOW_COV_FOREST_GROUPS && cov_public_kind(CovKind::ForestGroupsOwn) == LOC_WINDOW_COV_FOREST_GROUPS);
    EXPECT(cov_public_kind(CovKind::Forest) == LOC_WINDOW_COV_FOREST && cov_public_kind(CovKind::ForestOwn) == LOC_WINDOW_COV_FOREST);
    EXPECT(cov_public_kind(CovKind::Chain3) == LOC_WINDOW_COV_CHAIN3 && cov_public_kind(CovKind::Chain6) == LOC_WINDOW_COV_CHAIN6 && cov_public_kind(CovKind::Arrow) == LOC_WINDOW_COV_ARROW);
    EXPECT(cov_public_kind(CovKind::Envelope) == LOC_WINDOW_COV_ENVELOPE && cov_public_kind(CovKind::None) == LOC_WINDOW_COV_NONE && cov_public_kind(CovKind::Unclassified) == LOC_WINDOW_COV_NONE);
    return 0;
}

int keyed() {
    const DispatchFits f = dispatch_fits(kCaps);
    const Batch mixed = mixed_batch(), one = one_topology_batch();
    const DispatchOpts on = options(true, true, false), off = options(true, false, false), off_general = options(true, false, true), lane = options(true, true, false, 2);
    WinAux own;
    SchedKey key;
    auto call = [&](const DispatchOpts& o, const Batch& b) {
        const CovVerdict v = covariance_kind(kCaps, o, f, 4, b.host(), kNoPairs, own, &key);
        if (v.need_upload) key.valid = true;   // (the caller's part: the tables have gone to the device)
        return v;
    };
    // a refusal is no entry: the key is noted, nothing is valid
    CovVerdict v = call(off, mixed);
    EXPECT(v.kind == CovKind::None && !v.need_upload && !key.valid && key.kind == CovKind::None);
    const unsigned long long k_mixed = key.key;
    // the same key, now under both options: built and sent
    v = call(on, mixed);
    EXPECT(v.kind == CovKind::ForestGroupsOwn && v.need_upload && key.valid && key.key == k_mixed && key.kind == CovKind::ForestGroupsOwn && own.n_groups == 2);
    const std::vector<int32_t> block = own.h_groups;
    own.h_groups.assign(own.h_groups.size(), 777);   // (a hit must not rebuild: the device copy is what counts)
    v = call(on, mixed);
    EXPECT(v.kind == CovKind::ForestGroupsOwn && !v.need_upload && own.h_groups[0] == 777 && own.n_groups == 2);
    // the key holds a groups block, the options no longer ask for one: no stale verdict, and the entry survives for the next call that does
    v = call(off, mixed);
    EXPECT(v.kind == CovKind::None && !v.need_upload);
    v = call(off_general, mixed);
    EXPECT(v.kind == CovKind::Envelope && !v.need_upload);
    v = call(lane, mixed);
    EXPECT(v.kind == CovKind::None && !v.need_upload);
    v = call(on, mixed);
    EXPECT(v.kind == CovKind::ForestGroupsOwn && !v.need_upload && key.valid);
    // another structure takes the entry over: a one-topology schedule, whatever the grouped options say
    v = call(on, one);
    EXPECT(v.kind == CovKind::ForestOwn && v.need_upload && key.kind == CovKind::ForestOwn && key.key != k_mixed);
    v = call(off, one);
    EXPECT(v.kind == CovKind::ForestOwn && !v.need_upload);
    v = call(lane, one);
    EXPECT(v.kind == CovKind::ForestOwn && !v.need_upload);
    // ... and the mixed batch again: its block is rebuilt, the one-topology verdict of the entry does not leak
    v = call(on, mixed);
    EXPECT(v.kind == CovKind::ForestGroupsOwn && v.need_upload && key.key == k_mixed && own.h_groups == block);
    v = call(on, one);
    EXPECT(v.kind == CovKind::ForestOwn && v.need_upload);
    // a change of what only the general kernel evaluates changes the key: nothing of the entry is reused
    DispatchOpts pinfo = on; pinfo.has_pinfo = true; pinfo.cov_general = true;
    v = call(pinfo, mixed);
    EXPECT(v.kind == CovKind::Envelope && !v.need_upload);
    return 0;
}

int bounds() {
    const Batch mixed = mixed_batch();
    WinAux A;
    EXPECT(build_tree_groups(kCaps, false, mixed.host(), A) && A.n_groups == 2);
    const std::vector<int32_t> hdr(A.h_groups.begin(), A.h_groups.begin() + 2 * kTreeGroupHdr);
    const size_t want = forest_cov_layout(9, false, true).bytes;
    EXPECT(forest_cov_layout(8, false, true).bytes < want);
    EXPECT(forest_cov_groups_lds_bytes(hdr.data(), 2, kCaps) == want);
    EXPECT(forest_cov_groups_lds_bytes(hdr.data(), 1, kCaps) == want && forest_cov_groups_lds_bytes(hdr.data() + kTreeGroupHdr, 1, kCaps) == forest_cov_layout(8, false, true).bytes);
    EXPECT(forest_cov_groups_lds_bytes(nullptr, 2, kCaps) == 0 && forest_cov_groups_lds_bytes(hdr.data(), 0, kCaps) == 0 && forest_cov_groups_lds_bytes(hdr.data(), -1, kCaps) == 0);
    // one bad header refuses the launch, whichever group it is: slot (0 nv, 1 nr, 2 np, 3 ns, 10 the table's offset) and value
    const int bad[][2] = {{0, 1}, {0, 0}, {0, 65}, {0, -3}, {1, 71}, {1, -1}, {2, 3}, {2, -1}, {3, 65}, {3, -1}, {10, -4}};
    for (const auto& m : bad)
        for (int g = 0; g < 2; ++g) {
            std::vector<int32_t> h = hdr;
            h[(size_t)g * kTreeGroupHdr + m[0]] = m[1];
            EXPECT(forest_cov_groups_lds_bytes(h.data(), 2, kCaps) == 0);
        }
    // within 64 poses but beyond the handle's capacity
    WindowCaps small = kCaps; small.nv_max = 8;
    EXPECT(forest_cov_groups_lds_bytes(hdr.data(), 2, small) == 0 && forest_cov_groups_lds_bytes(hdr.data() + kTreeGroupHdr, 1, small) > 0);
    // the largest group sets the launch's LDS: a 64-pose group with priors and EdgeSE3 is the 60 KB of the one-topology pass, within the limit
    std::vector<int32_t> h = hdr;
    h[0] = 64; h[1] = 70; h[2] = 2; h[3] = 63;
    EXPECT(forest_cov_groups_lds_bytes(h.data(), 2, kCaps) == forest_cov_layout(64, true, true).bytes && forest_cov_layout(64, true, true).bytes <= kCovMaxLds);
    // forest_cov_sizes_ok is the one-topology launcher's rule
    for (int nv = -1; nv <= 66; ++nv)
        for (int nr : {0, 70, 71})
            for (int np : {0, 2, 3})
                for (int ns : {0, 64, 65}) {
                    TreeSched ts{};
                    ts.nv = nv; ts.nr = nr; ts.np = np; ts.ns = ns;
                    const bool rule = !(nv < 2 || nv > 64 || nv > kCaps.nv_max || nr > kCaps.nr_max || np > kCaps.np_max || ns > kCaps.ns_max) && cov_forest_fits(nv, np > 0, ns > 0);
                    EXPECT(forest_cov_sizes_ok(ts, kCaps) == rule);
                }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s verdicts|admission|keyed|bounds\n", argv[0]); return 2; }
    const std::string s(argv[1]);
    int rc = 2;
    if (s == "verdicts") rc = verdicts();
    else if (s == "admission") rc = admission();
    else if (s == "keyed") rc = keyed();
    else if (s == "bounds") rc = bounds();
    else std::fprintf(stderr, "unknown section %s\n", argv[1]);
    if (rc == 0) std::printf("%s: %ld checks\n", argv[1], g_checks);
    return rc;
}
