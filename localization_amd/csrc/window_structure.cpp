// Structure analysis of a batch of windows.  Host code only: no HIP runtime call in this file.
#include "window_structure.h"
#include "window_layouts.h"
#include "arrow_pack.h"
#include "window_groups.h"

#include <cstring>
#include <algorithm>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>

namespace locamd {

// The host passes over a batch (validation, structure hash, chain / translation-only scans) are O(instances x edges) and run in front of a
// kernel of a millisecond or two: batches of >= 4 096 instances are split over up to eight threads (f(lo, hi) on disjoint instance ranges).
template <class F>
static void parallel_chunks(int64_t n, F&& f) {
    const unsigned hw = std::thread::hardware_concurrency();
    const int nt = n >= 4096 ? (int)std::min<unsigned>(8u, hw ? hw : 1u) : 1;
    if (nt <= 1) { f((int64_t)0, n, 0); return; }
    const int64_t per = (n + nt - 1) / nt;
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back([&f, t, per, n] { f(std::min(n, t * per), std::min(n, (t + 1) * per), t); });
    f((int64_t)0, std::min(n, per), 0);
    for (auto& x : th) x.join();
}

// Host-side shape check of every instance: 0, or WHICH check failed first (the caller words the error: capi_window.cpp, validate_instances)
int check_instances(const WindowCaps& c, int n_anchors, const HostBatch& b) {
    std::atomic<int> first_bad{0};
    parallel_chunks(b.n, [&](int64_t lo, int64_t hi, int) {
        auto check = [&](int64_t i) -> int {
            const int32_t* cn = b.counts + i * 4;
            if (cn[0] < 0 || cn[0] > c.nv_max || cn[1] < 0 || cn[1] > c.nr_max || cn[2] < 0 || cn[2] > c.np_max || cn[3] < 0 || cn[3] > c.ns_max) return 1;
            for (int e = 0; e < cn[1]; ++e) {
                const int32_t* ix = b.r_idx + ((size_t)i * c.nr_max + e) * 2;
                if (ix[0] < 0 || ix[0] >= cn[0] || ix[1] >= cn[0] || ix[1] < -n_anchors || ix[0] == ix[1]) return 2;
                if (ix[1] >= 0 && (ix[0] - ix[1] > c.bw_max || ix[1] - ix[0] > c.bw_max)) return 3;
            }
            for (int e = 0; e < cn[2]; ++e) {
                const int32_t v = b.p_idx[(size_t)i * c.np_max + e];
                if (v < 0 || v >= cn[0]) return 4;
            }
            for (int e = 0; e < cn[3]; ++e) {
                const int32_t* ix = b.s_idx + ((size_t)i * c.ns_max + e) * 4;
                if (ix[0] < 0 || ix[0] >= cn[0] || ix[1] < 0 || ix[1] >= cn[0] || ix[0] == ix[1]) return 5;
                if (ix[0] - ix[1] > c.bw_max || ix[1] - ix[0] > c.bw_max) return 6;
            }
            return 0;
        };
        for (int64_t i = lo; i < hi && first_bad.load(std::memory_order_relaxed) == 0; ++i) {
            const int bad = check(i);
            if (bad) { int zero = 0; first_bad.compare_exchange_strong(zero, bad); return; }
        }
    });
    return first_bad.load();
}

// what loc_window_set_anchors may not shrink the anchor table below while the batch is resident
int max_anchor_referenced(const WindowCaps& c, int64_t n, const int32_t* counts, const int32_t* r_idx) {
    int max_anchor = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int e = 0; e < counts[i * 4 + 1]; ++e) {
            const int32_t v1 = r_idx[((size_t)i * c.nr_max + e) * 2 + 1];
            if (v1 < 0 && -v1 > max_anchor) max_anchor = -v1;
        }
    return max_anchor;
}

// Host-side check of the pair tables of a joint covariance call: the kernels index LDS and the workspace with these slots
int check_pairs(int64_t n, const int32_t* counts, const PairTables& pt) {
    if (pt.npair_max <= 0) return 0;
    std::atomic<int> first_bad{0};
    parallel_chunks(n, [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi && first_bad.load(std::memory_order_relaxed) == 0; ++i) {
            const int32_t nv = counts[i * 4], np = pt.counts[i];
            int bad = np < 0 || np > pt.npair_max ? 1 : 0;
            for (int p = 0; p < np && !bad; ++p) {
                const int32_t* ix = pt.pairs + ((size_t)i * pt.npair_max + p) * 2;
                if (ix[0] < 0 || ix[0] >= nv || ix[1] < 0 || ix[1] >= nv) bad = 2;
            }
            if (bad) { int zero = 0; first_bad.compare_exchange_strong(zero, bad); return; }
        }
    });
    return first_bad.load();
}

// translation-only (the exact 3-DoF reduction, chain3_kernel.hip / arrow3_kernel.hip): no EdgeSE3, every lever arm zero, every
// rotation the identity, priors with an identity measurement rotation and no rotation information
bool translation_only(const WindowCaps& c, int n_anchors, const HostBatch& b, bool skip_prior_diagonal) {
    static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (n_anchors > 500000) return false;   // (the packed endpoint word of chain3 holds 2^19 anchors)
    std::atomic<bool> all{true};
    parallel_chunks(b.n, [&](int64_t lo, int64_t hi, int) {
        auto one = [&](int64_t i) {
            const int32_t* cn = b.counts + i * 4;
            if (cn[3] != 0 || cn[0] > 1048575) return false;
            for (int e = 0; e < cn[1]; ++e) {
                const double* v = b.r_val + ((size_t)i * c.nr_max + e) * 5;
                if (v[2] != 0.0 || v[3] != 0.0 || v[4] != 0.0) return false;
            }
            for (int p = 0; p < cn[0]; ++p)
                if (std::memcmp(b.poses + ((size_t)i * c.nv_max + p) * 12, I9, sizeof(I9)) != 0) return false;
            for (int e = 0; e < cn[2]; ++e) {
                const double* v = b.p_val + ((size_t)i * c.np_max + e) * 18;
                if (std::memcmp(v, I9, sizeof(I9)) != 0 || (!skip_prior_diagonal && (v[15] != 0.0 || v[16] != 0.0 || v[17] != 0.0))) return false;
            }
            return true;
        };
        for (int64_t i = lo; i < hi && all.load(std::memory_order_relaxed); ++i)
            if (!one(i)) { all.store(false); return; }
    });
    return all.load();
}

bool prior_information_translation_only(size_t n_rows, const double* pinfo) {
    for (size_t e = 0; e < n_rows; ++e) {
        const double* W = pinfo + e * 36;
        for (int i = 0; i < 6; ++i)
            for (int j = (i < 3 ? 3 : 0); j < 6; ++j)
                if (W[i * 6 + j] != 0.0) return false;
    }
    return true;
}

// Host-side check of the drop slots of a marginal-prior call: the kernel indexes the pose table with them, and takes the one neighbour it finds
int check_marginal_drop(const WindowCaps& c, const HostBatch& b, const int32_t* drop) {
    for (int64_t i = 0; i < b.n; ++i)   // (every slot first: an invalid call is invalid whatever else is wrong with it)
        if (drop[i] < 0 || drop[i] >= b.counts[i * 4]) return 1;
    std::atomic<int> first_bad{0};
    parallel_chunks(b.n, [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi && first_bad.load(std::memory_order_relaxed) == 0; ++i) {
            const int32_t* cn = b.counts + i * 4;
            const int32_t d = drop[i];
            int bad = 0, m = -1;
            for (int e = 0; e < cn[1] && !bad; ++e) {
                const int32_t* ix = b.r_idx + ((size_t)i * c.nr_max + e) * 2;
                if (ix[1] < 0 || (ix[0] != d && ix[1] != d)) continue;
                const int other = ix[0] == d ? ix[1] : ix[0];
                if (m >= 0 && other != m) bad = 2;
                m = other;
            }
            for (int e = 0; e < cn[3] && !bad; ++e) {   // (a translation-only batch has none: the caller's scan comes first; counted all the same)
                const int32_t* ix = b.s_idx + ((size_t)i * c.ns_max + e) * 4;
                if (ix[0] != d && ix[1] != d) continue;
                const int other = ix[0] == d ? ix[1] : ix[0];
                if (m >= 0 && other != m) bad = 2;
                m = other;
            }
            if (bad) { int zero = 0; first_bad.compare_exchange_strong(zero, bad); return; }
        }
    });
    return first_bad.load();
}

// The resident slide's index rule on the host mirror (window_structure.h; window_slide_kernel.hip applies the same rule to the device tables)
SlideVerdict slide_indices(const WindowCaps& c, int n_anchors, int64_t n, int32_t* counts, int32_t* r_idx, int32_t* p_idx, const SlideRows& s, bool apply) {
    std::atomic<int> first_bad{0};
    int max_part[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // one per thread's window range
    parallel_chunks(n, [&](int64_t lo, int64_t hi, int t) {
        int max_anchor = 0;
        for (int64_t i = lo; i < hi && first_bad.load(std::memory_order_relaxed) == 0; ++i) {
            int32_t* cn = counts + i * 4;
            int32_t* ri = r_idx + (size_t)i * c.nr_max * 2;
            int32_t* pi = p_idx + (size_t)i * c.np_max;
            const int nv = cn[0], nr = cn[1], np = cn[2];
            const bool drop = !s.drop || s.drop[i] != 0;
            const int nrn = s.nr_new_max > 0 ? s.r_counts[i] : 0, npn = s.np_new_max > 0 ? s.p_counts[i] : 0;
            const int32_t* nri = s.r_idx + (size_t)i * (s.nr_new_max > 0 ? s.nr_new_max : 0) * 2;
            // what the drop leaves: the kept rows, and whether a pose-to-pose range joined slot 0 to another pose (the marginal's slot >= 0)
            int r_kept = nr, p_kept = np, carried = 0;
            if (drop) {
                r_kept = 0; p_kept = 0;
                for (int e = 0; e < nr; ++e) {
                    const int32_t v0 = ri[e * 2], v1 = ri[e * 2 + 1];
                    if (v0 != 0 && v1 != 0) ++r_kept;
                    else if (v1 >= 0) carried = 1;
                }
                for (int e = 0; e < np; ++e) p_kept += pi[e] != 0;
            }
            const int nv2 = nv - (drop ? 1 : 0) + 1, sl = nv2 - 1;   // the slid window's poses, its new slot
            if (!apply) {
                int bad = 0;
                if (nv <= 0) bad = 1;
                else if (nrn < 0 || nrn > s.nr_new_max || npn < 0 || npn > s.np_new_max) bad = 2;
                bool named = false;   // a row so far names the new slot
                for (int e = 0; e < nrn && !bad; ++e) {
                    const int32_t v0 = nri[e * 2], v1 = nri[e * 2 + 1];
                    const bool ok0 = v0 == sl || (v0 == sl - 1 && v0 >= 0);
                    const bool ok1 = v1 < 0 ? v1 >= -n_anchors : ((v1 == sl || v1 == sl - 1) && v1 != v0 && c.bw_max >= 1);
                    const bool names = v0 == sl || v1 == sl;
                    if (!ok0 || !ok1 || (named && !names)) bad = 3;
                    named = named || names;
                }
                if (!bad && nv2 > c.nv_max) bad = 4;
                if (!bad && r_kept + nrn > c.nr_max) bad = 5;
                if (!bad && carried + p_kept + npn > c.np_max) bad = 6;
                if (bad) { int zero = 0; first_bad.compare_exchange_strong(zero, bad); return; }
                continue;
            }
            if (drop) {   // destinations never pass sources: in place
                int k = 0;
                for (int e = 0; e < nr; ++e) {
                    const int32_t v0 = ri[e * 2], v1 = ri[e * 2 + 1];
                    if (v0 == 0 || v1 == 0) continue;
                    ri[k * 2] = v0 - 1; ri[k * 2 + 1] = v1 > 0 ? v1 - 1 : v1;
                    ++k;
                }
                k = 0;
                for (int e = 0; e < np; ++e)
                    if (pi[e] != 0) pi[k++] = pi[e] - 1;
                if (carried) {   // the one-row shift, from the top down
                    for (int e = p_kept; e > 0; --e) pi[e] = pi[e - 1];
                    pi[0] = 0;
                }
            }
            for (int e = 0; e < nrn; ++e) { ri[(r_kept + e) * 2] = nri[e * 2]; ri[(r_kept + e) * 2 + 1] = nri[e * 2 + 1]; }
            for (int e = 0; e < npn; ++e) pi[carried + p_kept + e] = sl;
            cn[0] = nv2; cn[1] = r_kept + nrn; cn[2] = carried + p_kept + npn;
            for (int e = 0; e < cn[1]; ++e)
                if (ri[e * 2 + 1] < 0 && -ri[e * 2 + 1] > max_anchor) max_anchor = -ri[e * 2 + 1];
        }
        max_part[t] = max_anchor;
    });
    int max_anchor = 0;
    for (int v : max_part) max_anchor = std::max(max_anchor, v);
    return SlideVerdict{first_bad.load(), max_anchor};
}

bool slide_rows_translation_only(int64_t n, const SlideRows& s, const double* new_pose, const double* r_val, const double* p_val) {
    static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::atomic<bool> all{true};
    parallel_chunks(n, [&](int64_t lo, int64_t hi, int) {
        auto one = [&](int64_t i) {
            if (std::memcmp(new_pose + (size_t)i * 12, I9, sizeof(I9)) != 0) return false;
            const int nrn = s.nr_new_max > 0 ? s.r_counts[i] : 0, npn = s.np_new_max > 0 ? s.p_counts[i] : 0;
            for (int e = 0; e < nrn && nrn <= s.nr_new_max; ++e) {
                const double* v = r_val + ((size_t)i * s.nr_new_max + e) * 5;
                if (v[2] != 0.0 || v[3] != 0.0 || v[4] != 0.0) return false;
            }
            for (int e = 0; e < npn && npn <= s.np_new_max; ++e) {
                const double* v = p_val + ((size_t)i * s.np_new_max + e) * 18;
                if (std::memcmp(v, I9, sizeof(I9)) != 0 || v[15] != 0.0 || v[16] != 0.0 || v[17] != 0.0) return false;
            }
            return true;
        };
        for (int64_t i = lo; i < hi && all.load(std::memory_order_relaxed); ++i)
            if (!one(i)) { all.store(false); return; }
    });
    return all.load();
}

// The chain scan: every pose-to-pose edge (range or SE3) of every window joins consecutive pose slots.  ordered: edges are also listed
// in the order of their later pose and priors in pose order (what the lane-per-window and wave-per-window solve kernels walk); the
// covariance pass takes any order.  single_pairs / se3_pairs: batch_topology's pair counts (only meaningful for chain batches, where
// every range was scanned).
void chain_scan(const WindowCaps& c, const HostBatch& b, bool ordered, bool& chain, bool& single_pairs, bool& se3_pairs) {
    std::atomic<bool> a_chain{true}, a_single{true}, a_single_r{true}, a_single_s{true}, a_any_s{false};
    parallel_chunks(b.n, [&](int64_t lo, int64_t hi, int) {
        bool chain_l = true, single_l = true, single_r = true, single_s = true, any_s = false;
        for (int64_t i = lo; i < hi && chain_l && a_chain.load(std::memory_order_relaxed); ++i) {
            const int32_t* cn = b.counts + i * 4;
            if (cn[3] != 0) { single_l = false; any_s = true; }
            int last = 0;
            for (int e = 0; e < cn[3]; ++e) {   // EdgeSE3 factors: between consecutive poses, ordered by their later pose (addTwistEdge)
                const int32_t* ix = b.s_idx + ((size_t)i * c.ns_max + e) * 4;
                const int key2 = ix[1] > ix[0] ? ix[1] : ix[0];
                if ((ordered && key2 < last) || (ix[0] - ix[1] != 1 && ix[1] - ix[0] != 1)) { chain_l = false; break; }
                if (key2 == last) single_s = false;   // (a second EdgeSE3 on the same pair; poses are numbered from 0, so `last` = 0 is no pair)
                last = key2;
            }
            last = 0;
            int last_pair = -1;
            for (int e = 0; e < cn[1] && chain_l; ++e) {
                const int32_t* ix = b.r_idx + ((size_t)i * c.nr_max + e) * 2;
                const int key2 = ix[1] > ix[0] ? ix[1] : ix[0];
                if (ordered && key2 < last) chain_l = false;
                if (ix[1] >= 0) { if (key2 == last_pair) { single_l = false; single_r = false; } last_pair = key2; }
                last = key2;
                if (ix[1] >= 0 && ix[0] - ix[1] != 1 && ix[1] - ix[0] != 1) chain_l = false;
            }
            last = 0;
            for (int e = 0; e < cn[2] && chain_l && ordered; ++e) {
                const int32_t v = b.p_idx[(size_t)i * c.np_max + e];
                if (v < last) chain_l = false;
                last = v;
            }
        }
        if (!chain_l) a_chain.store(false);
        if (!single_l) a_single.store(false);
        if (!single_r) a_single_r.store(false);
        if (!single_s) a_single_s.store(false);
        if (any_s) a_any_s.store(true);
    });
    chain = a_chain.load();
    single_pairs = a_single.load();
    se3_pairs = a_any_s.load() && a_single_r.load() && a_single_s.load();
}

// 64-bit hash of a batch's STRUCTURE: n, the counts and the used entries of the index tables (never the measurements)
unsigned long long hash_structure(const WindowCaps& c, bool has_off1, const HostBatch& b) {
    unsigned long long part[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // one hash per thread's instance range, combined in range order
    parallel_chunks(b.n, [&](int64_t lo, int64_t hi, int t) {
        unsigned long long h = 0x9e3779b97f4a7c15ull + (unsigned long long)t;
        auto mix = [&h](const int32_t* p, size_t cnt) {
            size_t i = 0;
            for (; i + 2 <= cnt; i += 2) {
                unsigned long long v;
                std::memcpy(&v, p + i, 8);
                h = (h ^ v) * 0xff51afd7ed558ccdull;
                h ^= h >> 32;
            }
            if (i < cnt) { h = (h ^ (unsigned long long)(uint32_t)p[i]) * 0xc4ceb9fe1a85ec53ull; h ^= h >> 29; }
        };
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t* cn = b.counts + i * 4;
            mix(cn, 4);
            if (cn[1]) mix(b.r_idx + (size_t)i * c.nr_max * 2, (size_t)cn[1] * 2);
            if (cn[2]) mix(b.p_idx + (size_t)i * c.np_max, (size_t)cn[2]);
            if (cn[3]) mix(b.s_idx + (size_t)i * c.ns_max * 4, (size_t)cn[3] * 4);
        }
        part[t & 7] = h;
    });
    unsigned long long h = 0x9e3779b97f4a7c15ull ^ (unsigned long long)b.n ^ (has_off1 ? 0x51ull << 56 : 0);
    for (int t = 0; t < 8; ++t) { h = (h ^ part[t]) * 0xff51afd7ed558ccdull; h ^= h >> 32; }
    return h;
}

// The envelope (skyline) of every instance's block matrix in the caller's pose order, as envelope_covariance_kernel.hip lays it out: row i
// holds the blocks (i, first[i]) .. (i, i).  Returns the largest block count of the batch, -1 when a count or an index is out of range
// (loc_window_covariance_plan calls this on tables no handle has validated).
long long envelope_blocks_max(const WindowCaps& c, const HostBatch& b) { return envelope_blocks_max_joint(c, b, PairTables{0, nullptr, nullptr}); }

// Pairs count as edges: a pair count or a slot out of range is -1 as well.
long long envelope_blocks_max_joint(const WindowCaps& c, const HostBatch& b, const PairTables& pt) {
    std::atomic<long long> most{0};
    std::atomic<bool> bad{false};
    parallel_chunks(b.n, [&](int64_t lo, int64_t hi, int) {
        std::vector<int32_t> first;
        long long most_l = 0;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t* cn = b.counts + i * 4;
            const int nv = cn[0], nr = cn[1], ns = cn[3];
            if (nv < 0 || nv > c.nv_max || nr < 0 || nr > c.nr_max || ns < 0 || ns > c.ns_max) { bad.store(true); return; }
            first.resize((size_t)nv);
            for (int v = 0; v < nv; ++v) first[(size_t)v] = v;
            auto join = [&](int v0, int v1) {
                if (v0 < 0 || v0 >= nv || v1 >= nv) return false;
                if (v1 < 0) return true;   // a fixed endpoint
                const int up = v0 > v1 ? v0 : v1, dn = v0 > v1 ? v1 : v0;
                if (dn < first[(size_t)up]) first[(size_t)up] = dn;
                return true;
            };
            for (int e = 0; e < nr; ++e) {
                const int32_t* ix = b.r_idx + ((size_t)i * c.nr_max + e) * 2;
                if (!join(ix[0], ix[1])) { bad.store(true); return; }
            }
            for (int e = 0; e < ns; ++e) {
                const int32_t* ix = b.s_idx + ((size_t)i * c.ns_max + e) * 4;
                if (ix[1] < 0 || !join(ix[0], ix[1])) { bad.store(true); return; }
            }
            if (pt.npair_max > 0) {
                const int32_t np = pt.counts[i];
                if (np < 0 || np > pt.npair_max) { bad.store(true); return; }
                for (int p = 0; p < np; ++p) {
                    const int32_t* ix = pt.pairs + ((size_t)i * pt.npair_max + p) * 2;
                    if (ix[1] < 0 || !join(ix[0], ix[1])) { bad.store(true); return; }
                }
            }
            long long blocks = 0;
            for (int v = 0; v < nv; ++v) blocks += v - first[(size_t)v] + 1;
            if (blocks > most_l) most_l = blocks;
        }
        long long seen = most.load();
        while (most_l > seen && !most.compare_exchange_weak(seen, most_l)) {}
    });
    return bad.load() ? -1 : most.load();
}

// CHAIN + BORDER ("arrowhead": BASELINE config 4, anchor self-calibration — a tag trajectory whose poses range to a few nodes that
// are unknowns themselves, localization.cpp:94-98).  The border of an instance = its last nb0 pose slots, nb0 = the smallest number
// such that every pose-to-pose edge between NON-consecutive slots has an endpoint there; the other poses form the chain (one edge
// per consecutive pair at most).  The chain is cut into up to four segments at separator poses, which join the border (one level of
// nested dissection: arrow3_lm_kernel sweeps the segments with one wave each).  Rows = chain rows segment by segment, then border
// rows (separators first, then the original border in slot order).  A chain row owns its edges to anchors, to border poses and
// to the previous chain row; a border row those to lower-index border poses and to anchors.  Every row's edges (creation order)
// and priors are packed as records [chunk of 64 rows][slot][lane].
// A.arrow_list_cap: the most edges and priors any pose in front of the nb0 border slots has (arrow_covariance_kernel.hip's list size).
// structure_only: the test alone, for the covariance pass — A is a table set of the covariance's own and nothing is packed.
// The rule for one window — structure, owners, refusals, records — is arrow_pack.h's; this is the loop over the batch and its batch-level refusals.
bool build_arrow_aux(const WindowCaps& c, const HostBatch& b, WinAux& A, bool structure_only) {
    static_assert(kArrowPackAnchors == kArrowMaxAnchors && kArrowSegments == ARROW_NW, "arrow_pack.h states arrow3_lm_kernel's limits");
    const int nchunk = (c.nv_max + 63) / 64;
    A.h_ahdr.assign((size_t)b.n * 8, 0);
    A.h_arslot.assign((size_t)b.n * c.nv_max, 0);
    std::vector<int32_t> work((size_t)3 * c.nv_max);
    // pass 1 (arrow_pack.h, (a)): structure, record counts
    ArrowMaxima m = arrow_maxima_empty();
    for (int64_t i = 0; i < b.n; ++i)
        if (arrow_window_structure(b.counts + i * 4, b.r_idx + (size_t)i * c.nr_max * 2, b.p_idx + (size_t)i * c.np_max, A.h_ahdr.data() + (size_t)i * 8,
                                   A.h_arslot.data() + (size_t)i * c.nv_max, work.data(), m) != kArrowOk) return false;
    if (arrow_batch_refused(m)) return false;
    if (!arrow3_fits(c, m.nb_max)) return false;
    A.arrow_list_cap = m.list_cap;
    if (structure_only) return true;
    // pass 2 (arrow_pack.h, (b)): the records
    const size_t rec_per = arrow_rec_doubles(nchunk, m.jmax), prec_per = arrow_prec_doubles(nchunk, m.jpmax);
    A.h_arec.resize((size_t)b.n * rec_per);
    A.h_aprec.resize((size_t)b.n * prec_per);
    for (int64_t i = 0; i < b.n; ++i)
        arrow_window_pack(b.counts + i * 4, A.h_ahdr.data() + (size_t)i * 8, b.r_idx + (size_t)i * c.nr_max * 2, b.r_val + (size_t)i * c.nr_max * 5,
                          b.p_idx + (size_t)i * c.np_max, b.p_val + (size_t)i * c.np_max * 18, nchunk, m.jmax, m.jpmax, A.h_arec.data() + (size_t)i * rec_per,
                          A.h_aprec.data() + (size_t)i * prec_per, work.data());
    A.arrow_nb_max = m.nb_max; A.arrow_jmax = m.jmax; A.arrow_jpmax = m.jpmax;
    for (int k = 0; k < 16; ++k) { A.arrow_jch[k] = m.jch[k]; A.arrow_jpch[k] = m.jpch[k]; }
    return true;
}

// One topology's schedule: everything build_tree_sched does behind its "one topology" loop — the forest test, centres, post-order, by-slot
// lists — on ONE window's counts and used index rows.  t receives the table (cleared first), ts the ten sizes.  false: nv outside [2, 64], or a cycle.
static bool tree_sched_one(const int32_t* counts, const int32_t* r_idx, const int32_t* p_idx, const int32_t* s_idx, std::vector<int32_t>& t, TreeSched& ts) {
    const int nv = counts[0], nr = counts[1], np = counts[2], ns = counts[3];
    if (nv < 2 || nv > 64) return false;
    // adjacency (pairs joined by at least one edge); a forest has no cycle: union-find on the distinct pairs
    std::vector<int> uf((size_t)nv);
    for (int v = 0; v < nv; ++v) uf[(size_t)v] = v;
    auto find = [&](int v) { while (uf[(size_t)v] != v) { uf[(size_t)v] = uf[(size_t)uf[(size_t)v]]; v = uf[(size_t)v]; } return v; };
    std::vector<std::vector<int>> adj((size_t)nv);
    auto join = [&](int u, int v) -> bool {
        for (int x : adj[(size_t)u]) if (x == v) return true;   // a second edge on the same pair
        const int ra = find(u), rb = find(v);
        if (ra == rb) return false;                             // a cycle
        uf[(size_t)ra] = rb;
        adj[(size_t)u].push_back(v); adj[(size_t)v].push_back(u);
        return true;
    };
    for (int e = 0; e < nr; ++e) if (r_idx[2 * e + 1] >= 0 && !join(r_idx[2 * e], r_idx[2 * e + 1])) return false;
    for (int e = 0; e < ns; ++e) if (!join(s_idx[4 * e], s_idx[4 * e + 1])) return false;
    // root of every component = its CENTRE (the middle of a longest path: two breadth-first searches), so that the elimination by
    // height takes half as many steps as from an end (config 5's chain of eight keys: 6 levels instead of 9); parents towards the
    // root; subtree sizes; post-order, heavy child first
    std::vector<int> parent((size_t)nv, -2), size((size_t)nv, 1), order, stack, depth((size_t)nv, 0);
    int nroots = 0, maxdepth = 0;
    std::vector<int> bfs;
    std::vector<int> seen((size_t)nv, 0), dist((size_t)nv, 0), from((size_t)nv, -1), centre_of;
    auto far_from = [&](int start) {   // the farthest node from `start` inside its component (dist / from filled)
        std::vector<int> q2{start};
        std::vector<int> mark((size_t)nv, 0);
        mark[(size_t)start] = 1; dist[(size_t)start] = 0; from[(size_t)start] = -1;
        int last = start;
        for (size_t h = 0; h < q2.size(); ++h) {
            const int v = q2[h];
            last = v;
            for (int x : adj[(size_t)v]) if (!mark[(size_t)x]) { mark[(size_t)x] = 1; dist[(size_t)x] = dist[(size_t)v] + 1; from[(size_t)x] = v; q2.push_back(x); }
        }
        for (int v : q2) seen[(size_t)v] = 1;
        return last;
    };
    for (int v0 = 0; v0 < nv; ++v0) {
        if (seen[(size_t)v0]) continue;
        const int a1 = far_from(v0);
        const int b1 = far_from(a1);        // a1 .. b1: a longest path of this tree
        int c1 = b1;
        for (int step = dist[(size_t)b1] / 2; step > 0; --step) c1 = from[(size_t)c1];
        centre_of.push_back(c1);
    }
    for (int root : centre_of) {
        if (parent[(size_t)root] != -2) continue;
        parent[(size_t)root] = -1; ++nroots;
        const size_t b0 = bfs.size();
        bfs.push_back(root);
        for (size_t h = b0; h < bfs.size(); ++h) {
            const int v = bfs[h];
            for (int x : adj[(size_t)v]) if (parent[(size_t)x] == -2) { parent[(size_t)x] = v; depth[(size_t)x] = depth[(size_t)v] + 1; if (depth[(size_t)x] > maxdepth) maxdepth = depth[(size_t)x]; bfs.push_back(x); }
        }
        for (size_t h = bfs.size(); h-- > b0 + 1;) size[(size_t)parent[(size_t)bfs[h]]] += size[(size_t)bfs[h]];
    }
    std::vector<std::vector<int>> kids((size_t)nv);
    for (int v = 0; v < nv; ++v) if (parent[(size_t)v] >= 0) kids[(size_t)parent[(size_t)v]].push_back(v);
    for (auto& k : kids) std::stable_sort(k.begin(), k.end(), [&](int a2, int b2) { return size[(size_t)a2] > size[(size_t)b2]; });
    // iterative post-order
    for (int root = 0; root < nv; ++root) {
        if (parent[(size_t)root] != -1) continue;
        std::vector<std::pair<int, size_t>> st;
        st.push_back({root, 0});
        while (!st.empty()) {
            auto& top = st.back();
            if (top.second < kids[(size_t)top.first].size()) { const int ch = kids[(size_t)top.first][top.second++]; st.push_back({ch, 0}); }
            else { order.push_back(top.first); st.pop_back(); }
        }
    }
    if ((int)order.size() != nv) return false;
    std::vector<int> pos((size_t)nv);
    for (int k = 0; k < nv; ++k) pos[(size_t)order[(size_t)k]] = k;
    // edges by node: a unary edge belongs to its pose; an edge between a node and its parent to the node (the child)
    std::vector<std::vector<int>> re((size_t)nv), pe((size_t)nv), se((size_t)nv);
    for (int e = 0; e < nr; ++e) {
        const int v0 = r_idx[2 * e], v1 = r_idx[2 * e + 1];
        if (v1 < 0) re[(size_t)pos[(size_t)v0]].push_back(e);
        else re[(size_t)pos[(size_t)(parent[(size_t)v0] == v1 ? v0 : v1)]].push_back(e);
    }
    for (int e = 0; e < np; ++e) pe[(size_t)pos[(size_t)p_idx[e]]].push_back(e);
    for (int e = 0; e < ns; ++e) {
        const int vi = s_idx[4 * e], vj = s_idx[4 * e + 1];
        se[(size_t)pos[(size_t)(parent[(size_t)vi] == vj ? vi : vj)]].push_back(e);
    }
    t.clear();
    for (int k = 0; k < nv; ++k) t.push_back(order[(size_t)k]);
    for (int k = 0; k < nv; ++k) { const int p = parent[(size_t)order[(size_t)k]]; t.push_back(p < 0 ? -1 : pos[(size_t)p]); }
    auto lists = [&](const std::vector<std::vector<int>>& L) {
        int acc = 0;
        for (int k = 0; k < nv; ++k) { t.push_back(acc); acc += (int)L[(size_t)k].size(); }
        t.push_back(acc);
        for (int k = 0; k < nv; ++k) for (int e : L[(size_t)k]) t.push_back(e);
    };
    lists(re); lists(pe); lists(se);
    for (int i = 0; i < 2 * nr; ++i) t.push_back(r_idx[i]);
    for (int i = 0; i < 4 * ns; ++i) t.push_back(s_idx[i]);
    // by pose slot (tree_wave_kernel): parent, height, children, edges
    std::vector<int> height((size_t)nv, 0);
    int hmax = 0;
    for (int k = 0; k < nv; ++k) {   // (post-order: children before their parent)
        const int v = order[(size_t)k], p = parent[(size_t)v];
        if (p >= 0 && height[(size_t)p] < height[(size_t)v] + 1) height[(size_t)p] = height[(size_t)v] + 1;
        if (height[(size_t)v] > hmax) hmax = height[(size_t)v];
    }
    for (int v = 0; v < nv; ++v) t.push_back(parent[(size_t)v]);
    for (int v = 0; v < nv; ++v) t.push_back(height[(size_t)v]);
    auto by_slot = [&](const std::vector<std::vector<int>>& L, bool positions) {   // L indexed by slot, or by schedule position
        int acc = 0;
        for (int v = 0; v < nv; ++v) { t.push_back(acc); acc += (int)L[(size_t)(positions ? pos[(size_t)v] : v)].size(); }
        t.push_back(acc);
        for (int v = 0; v < nv; ++v) for (int e : L[(size_t)(positions ? pos[(size_t)v] : v)]) t.push_back(e);
    };
    // (tree_wave_kernel wants a node's LEAF children first: their sums are taken in one parallel pass right after the leaves' level)
    std::vector<std::vector<int>> kids_lf((size_t)nv);
    std::vector<int> nleafkids((size_t)nv, 0);
    for (int v = 0; v < nv; ++v) {
        for (int ch : kids[(size_t)v]) if (height[(size_t)ch] == 0) { kids_lf[(size_t)v].push_back(ch); ++nleafkids[(size_t)v]; }
        for (int ch : kids[(size_t)v]) if (height[(size_t)ch] != 0) kids_lf[(size_t)v].push_back(ch);
    }
    by_slot(kids_lf, false); by_slot(re, true); by_slot(pe, true); by_slot(se, true);
    for (int v = 0; v < nv; ++v) t.push_back(nleafkids[(size_t)v]);
    // the inner nodes, parents first (tree_wave_kernel sums over children with lane = entry, one inner node after the other)
    int nu = 0;
    for (int h = hmax; h >= 1; --h)
        for (int v = 0; v < nv; ++v) if (height[(size_t)v] == h) { t.push_back(v); ++nu; }
    ts.nu = nu;
    {   // a pose's position in the children list just emitted (by_slot(kids_lf)): parents in slot order, a parent's leaf children first
        std::vector<int> kpos((size_t)nv, -1);
        int at = 0;
        for (int v = 0; v < nv; ++v) for (int ch : kids_lf[(size_t)v]) kpos[(size_t)ch] = at++;
        for (int v = 0; v < nv; ++v) if (kpos[(size_t)v] < 0) kpos[(size_t)v] = at++;   // roots
        for (int v = 0; v < nv; ++v) t.push_back(kpos[(size_t)v]);
    }
    ts.nlev = hmax + 1;
    ts.max_se3_per_node = 0;
    ts.max_r_per_node = 0;
    for (int k = 0; k < nv; ++k) if ((int)se[(size_t)k].size() > ts.max_se3_per_node) ts.max_se3_per_node = (int)se[(size_t)k].size();
    for (int k = 0; k < nv; ++k) if ((int)re[(size_t)k].size() > ts.max_r_per_node) ts.max_r_per_node = (int)re[(size_t)k].size();
    ts.nv = nv; ts.nr = nr; ts.np = np; ts.ns = ns; ts.depth = maxdepth + 1; ts.nroots = nroots;
    return true;
}

// FOREST windows of ONE shared topology (BASELINE config 5: the key-frame star of addPoseEdge, localization.cpp:254-290, replayed
// with different measurements in every instance): every instance has the same counts and index tables, and the pose-to-pose
// edges form a forest.  Builds the elimination schedule tree_lm_kernel walks: nodes in post-order (children before their parent,
// a node's children heavy subtree first so that the leaves of one parent are consecutive), per node its parent and its edges.
// Layout of the int table: tree_sched_bind (window_layouts.h), which walks it in the order tree_sched_one above emits it from "t.clear()" on.
bool build_tree_sched(const WindowCaps& c, bool has_off1, const HostBatch& b, WinAux& A) {
    const int nv = b.counts[0], nr = b.counts[1], np = b.counts[2], ns = b.counts[3];
    if (nv < 2 || nv > 64 || has_off1) return false;
    for (int64_t i = 1; i < b.n; ++i) {   // one topology
        if (std::memcmp(b.counts + i * 4, b.counts, 4 * sizeof(int32_t)) != 0) return false;
        if (nr && std::memcmp(b.r_idx + (size_t)i * c.nr_max * 2, b.r_idx, (size_t)nr * 2 * sizeof(int32_t)) != 0) return false;
        if (np && std::memcmp(b.p_idx + (size_t)i * c.np_max, b.p_idx, (size_t)np * sizeof(int32_t)) != 0) return false;
        if (ns && std::memcmp(b.s_idx + (size_t)i * c.ns_max * 4, b.s_idx, (size_t)ns * 4 * sizeof(int32_t)) != 0) return false;
    }
    return tree_sched_one(b.counts, b.r_idx, b.p_idx, b.s_idx, A.h_tsched, A.tsched);   // (the one-group case of build_tree_groups below)
}

// ts's pointers into a copy of the table build_tree_sched wrote (A.h_tsched, or its device copy) that starts at base; ts's sizes are those
// build_tree_sched set.  The table's length: the int32s from base to the end of w_kpos.
size_t bind_tree_sched(TreeSched& ts, const int32_t* base) { return tree_sched_bind(ts, base); }   // (window_layouts.h: the one statement)

// ---- forest windows of DIFFERING topologies (option "forest_groups"; DESIGN.md §2, "Forest groups") -------------------------------------------
// Key-frame windows cut from different robots, or at different phases of one robot's key cadence (Localization::addPoseEdge,
// localization.cpp:254-290), have different parents and lengths and range different anchors.  A window's TOPOLOGY KEY: its four counts, its
// used r_idx rows with every fixed endpoint (v1 < 0) collapsed to -1, its used p_idx rows, columns 0 - 1 of its used s_idx rows.  Anchor
// numbers and robust flags are not part of it: tree_wave_groups_kernel reads them from the window's own rows.
static void topology_key(const WindowCaps& c, const HostBatch& b, int64_t i, std::vector<int32_t>& k) {   // (window_groups.h: the one statement)
    const int32_t* cn = b.counts + i * 4;
    const int32_t *r = b.r_idx + (size_t)i * c.nr_max * 2, *p = b.p_idx + (size_t)i * c.np_max, *s = b.s_idx + (size_t)i * c.ns_max * 4;
    const long long nw = topology_key_words(cn);
    k.resize((size_t)nw);
    for (long long j = 0; j < nw; ++j) k[(size_t)j] = topology_key_word(cn, r, p, s, j);
}

// Part (a), the grouping: of[b] = window b's group, ids in order of first appearance; rep[g] = group g's first window.  A hash finds the
// candidates, a memcmp of the keys decides.  false: a window with nv outside [2, 64] (of and rep are then worth nothing).
bool group_windows(const WindowCaps& c, const HostBatch& b, std::vector<int32_t>& of, std::vector<int64_t>& rep) {
    const int64_t n = b.n;
    of.assign((size_t)(n > 0 ? n : 0), 0);
    rep.clear();
    if (n <= 0) return false;
    // pass 1, split over the windows: a 64-bit FNV-1a of every key
    std::vector<uint64_t> hash((size_t)n);
    std::atomic<bool> bad{false};
    parallel_chunks(n, [&](int64_t lo, int64_t hi, int) {
        std::vector<int32_t> k;
        for (int64_t i = lo; i < hi && !bad.load(std::memory_order_relaxed); ++i) {
            const int32_t nv = b.counts[i * 4];
            if (nv < 2 || nv > 64) { bad.store(true); return; }
            topology_key(c, b, i, k);
            uint64_t h = 1469598103934665603ull;
            for (int32_t x : k) { h ^= (uint32_t)x; h *= 1099511628211ull; }
            hash[(size_t)i] = h;
        }
    });
    if (bad.load()) return false;
    // pass 2, in window order: a window joins the first group of its hash whose representative's key equals its own
    std::vector<int32_t> k;
    std::vector<std::pair<uint64_t, int64_t>> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[(size_t)i] = {hash[(size_t)i], i};
    std::sort(order.begin(), order.end());   // (equal hashes in window order: a group's representative is its first window)
    std::vector<int32_t> local((size_t)n, -1);   // per window: index of its group among the groups found in hash order
    std::vector<int64_t> lrep;
    std::vector<std::vector<int32_t>> lkey;
    for (size_t a0 = 0; a0 < order.size();) {
        size_t a1 = a0;
        while (a1 < order.size() && order[a1].first == order[a0].first) ++a1;
        const size_t g0 = lrep.size();
        for (size_t q = a0; q < a1; ++q) {
            const int64_t i = order[q].second;
            topology_key(c, b, i, k);
            size_t g = g0;
            for (; g < lrep.size(); ++g)
                if (lkey[g].size() == k.size() && std::memcmp(lkey[g].data(), k.data(), k.size() * sizeof(int32_t)) == 0) break;
            if (g == lrep.size()) { lrep.push_back(i); lkey.push_back(k); }
            local[(size_t)i] = (int32_t)g;
        }
        a0 = a1;
    }
    // group ids in order of first appearance
    std::vector<int32_t> id(lrep.size(), -1);
    for (int64_t i = 0; i < n; ++i) {
        int32_t& g = id[(size_t)local[(size_t)i]];
        if (g < 0) { g = (int32_t)rep.size(); rep.push_back(i); }
        of[(size_t)i] = g;
    }
    return true;
}

// Part (b), representatives -> block: group g's representative is window rep[g] of b (rep == nullptr: window g — b is then the compact batch
// of the G representatives, each with its counts and used index rows at the capacities c).  Runs every representative through
// tree_sched_one, applies the refusals and writes A.h_groups = [hdr | sched_of | pad | tables] for the n windows of of[].
static bool groups_block(const WindowCaps& c, const HostBatch& b, const int64_t* rep, int64_t G, int64_t n, const int32_t* of, WinAux& A) {
    A.n_groups = 0;
    A.h_groups.clear();
    if (G <= 0 || n < G) return false;
    for (int64_t i = 0; i < n; ++i) if (of[i] < 0 || of[i] >= G) return false;   // (the kernels index the headers by sched_of unchecked)
    // every group's schedule, split over the groups
    std::atomic<bool> bad{false};
    std::vector<std::vector<int32_t>> tab((size_t)G);
    std::vector<TreeSched> sizes((size_t)G);
    parallel_chunks(G, [&](int64_t lo, int64_t hi, int) {
        for (int64_t g = lo; g < hi && !bad.load(std::memory_order_relaxed); ++g) {
            const int64_t i = rep ? rep[g] : g;
            TreeSched& ts = sizes[(size_t)g];
            ts = TreeSched{};
            if (!tree_sched_one(b.counts + i * 4, b.r_idx + (size_t)i * c.nr_max * 2, b.p_idx + (size_t)i * c.np_max, b.s_idx + (size_t)i * c.ns_max * 4, tab[(size_t)g], ts) ||
                ts.max_se3_per_node > 1 || !tree_wave_sizes_ok(ts)) { bad.store(true); return; }
        }
    });
    if (bad.load()) return false;
    // [hdr | sched_of | pad | tables]: every table starts at a multiple of 4 int32s; the slots no table owns are poisoned
    std::vector<int32_t>& t = A.h_groups;
    const size_t of_at = (size_t)G * kTreeGroupHdr, tab_at = (of_at + (size_t)n + 3) / 4 * 4;
    size_t total = 0;
    for (const auto& x : tab) total += (x.size() + 3) / 4 * 4;
    if (total > (size_t)INT32_MAX) return false;   // (a header holds its table's offset as an int32)
    t.assign(tab_at + total, kTreeGroupPoison);
    std::memcpy(t.data() + of_at, of, (size_t)n * sizeof(int32_t));
    size_t at = 0;
    for (int64_t g = 0; g < G; ++g) {
        const TreeSched& ts = sizes[(size_t)g];
        const int32_t h[kTreeGroupHdr] = {ts.nv, ts.nr, ts.np, ts.ns, ts.depth, ts.nroots, ts.nlev, ts.max_se3_per_node, ts.nu, ts.max_r_per_node, (int32_t)at, (int32_t)tab[(size_t)g].size()};
        std::memcpy(t.data() + (size_t)g * kTreeGroupHdr, h, sizeof(h));
        std::memcpy(t.data() + tab_at + at, tab[(size_t)g].data(), tab[(size_t)g].size() * sizeof(int32_t));
        at += (tab[(size_t)g].size() + 3) / 4 * 4;
    }
    A.n_groups = (int)G;
    A.groups_of_at = of_at;
    A.groups_tab_at = tab_at;
    return true;
}

// Part (b) for a caller that has grouped the batch elsewhere (loc_window_upload_dev under option "upload_dev_forest_groups": on the device):
// reps = the compact batch of the G = reps.n representatives in group order, of [n] = every window's group.  The block and the refusals are
// build_tree_groups' for the batch those representatives were taken from (a window's nv is part of its key: the representatives' suffice).
bool build_tree_groups_block(const WindowCaps& c, bool has_off1, const HostBatch& reps, int64_t n, const int32_t* of, WinAux& A) {
    A.n_groups = 0;
    A.h_groups.clear();
    if (has_off1 || c.nv_max > 64 || n <= 0 || !of) return false;
    return groups_block(c, reps, nullptr, reps.n, n, of, A);
}

// Groups the windows by topology key (group_windows), runs every group's first window through tree_sched_one and writes
// A.h_groups = [hdr | sched_of | pad | tables] (window_kernel.h: TreeGroups).
// The batch is refused as a whole — false, A.n_groups = 0 — when any window has nv outside [2, 64], any group has a cycle or more than one
// EdgeSE3 on a node's edge to its parent (tree_lm_kernel, which takes those, has no twin), under has_off1, or when the handle's nv_max > 64.
bool build_tree_groups(const WindowCaps& c, bool has_off1, const HostBatch& b, WinAux& A) {
    A.n_groups = 0;
    A.h_groups.clear();
    if (has_off1 || c.nv_max > 64 || b.n <= 0) return false;
    std::vector<int32_t> of;
    std::vector<int64_t> rep;
    if (!group_windows(c, b, of, rep)) return false;
    return groups_block(c, b, rep.data(), (int64_t)rep.size(), b.n, of.data(), A);
}

}  // namespace locamd
