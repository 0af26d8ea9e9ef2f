// Stand-alone check of option "prior_information_structured" in localization_amd/csrc/window_dispatch.cpp for
// tests/test_structured_prior_dispatch_cpu.py: host code only, built with plain g++ under AddressSanitizer + UBSan.  It links against
// window_dispatch.cpp and window_structure.cpp and nothing else of the product.
//
//   structured_prior_dispatch_driver      exit status 0 and one summary line, or the first rule that failed on stderr and exit status 1
//
// What it holds the rules to, over the product of option x has_pinfo x table translation-only x has_off1 x topology x n x the wave3 / chain3 /
// threshold / ordering switches x the LDS-fit flags:
//   1. with option 0 every verdict is the verdict of a handle whose table is handled as before the option existed: the general kernel /
//      no structured covariance pass whenever a table (or endpoint-1 lever arms) is set, and the table-less rule otherwise — whatever the
//      translation-only flag and the twin's fit flag say;
//   2. with option 1, LOC_WINDOW_KERNEL_WAVE3 / CovKind::Chain3 appear under a table exactly when: the table is translation-only, there
//      are no endpoint-1 lever arms, the batch is a translation-only chain with the priors' diagonals skipped (they hold NaN here), the
//      table-less rule would pick WAVE3 for a CHAIN3 topology / the chain pass fits and nv_max <= 64, and the twin's LDS fits — and every
//      other verdict is the one of option 0;
//   3. cov_switches differs between two settings whenever the option or the table's translation-only verdict differs under a table.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/localization_amd.h"
#include "window_dispatch.h"

using namespace locamd;

static long long g_checks = 0;
#define HOLD(cond, ...) do { ++g_checks; if (!(cond)) { std::fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static DispatchOpts without_table(DispatchOpts o) { o.has_pinfo = false; o.pinfo_translation = false; o.pinfo_structured = false; return o; }

// ---- a small batch: n windows of nv poses, each pose ranged to three anchors and joined to the previous one; one prior on pose 0 whose
// diagonal in p_val is NaN (not read under a table).  star: the pose-to-pose edges all go to pose 0 (no chain); rotated: one pose is not the identity
struct Batch {
    WindowCaps c;
    std::vector<int32_t> counts, ridx, pidx, sidx;
    std::vector<double> poses, rval, pval, sval;
    HostBatch host(int64_t n) const { return HostBatch{n, poses.data(), counts.data(), rval.data(), pval.data(), sval.data(), ridx.data(), pidx.data(), sidx.data()}; }
};
static Batch make_batch(int nv_max, int nv, int64_t n, bool star, bool rotated, bool nan_diagonal) {
    Batch b;
    b.c = WindowCaps{nv_max, 4 * nv_max, 1, 0, nv_max - 1};
    const size_t N = (size_t)n;
    b.counts.assign(N * 4, 0); b.ridx.assign(N * b.c.nr_max * 2, 0); b.pidx.assign(N, 0); b.sidx.assign(4, 0);
    b.poses.assign(N * nv_max * 12, 0.0); b.rval.assign(N * b.c.nr_max * 5, 0.0); b.pval.assign(N * 18, 0.0); b.sval.assign(48, 0.0);
    for (size_t i = 0; i < N; ++i) {
        int e = 0;
        for (int p = 0; p < nv; ++p) {
            double* X = &b.poses[(i * nv_max + p) * 12];
            X[0] = X[4] = X[8] = 1.0; X[9] = 0.1 * p; X[10] = 0.2; X[11] = 1.0;
            for (int a = 0; a < 3; ++a, ++e) {
                b.ridx[(i * b.c.nr_max + e) * 2] = p; b.ridx[(i * b.c.nr_max + e) * 2 + 1] = -1 - a;
                b.rval[(i * b.c.nr_max + e) * 5] = 2.0; b.rval[(i * b.c.nr_max + e) * 5 + 1] = 100.0;
            }
            if (p) {
                b.ridx[(i * b.c.nr_max + e) * 2] = star ? 0 : p - 1; b.ridx[(i * b.c.nr_max + e) * 2 + 1] = p;
                b.rval[(i * b.c.nr_max + e) * 5 + 1] = 10.0;
                ++e;
            }
        }
        if (rotated && i == N - 1) { double* X = &b.poses[(i * nv_max + nv - 1) * 12]; X[0] = X[4] = 0.0; X[1] = -1.0; X[3] = 1.0; }
        double* P = &b.pval[i * 18];
        P[0] = P[4] = P[8] = 1.0;
        for (int k = 12; k < 18; ++k) P[k] = nan_diagonal ? std::nan("") : (k < 15 ? 5.0 : 0.0);
        b.counts[i * 4] = nv; b.counts[i * 4 + 1] = e; b.counts[i * 4 + 2] = 1;
    }
    return b;
}

int main() {
    long long wave3_seen = 0, chain3_seen = 0;
    // ---- pick_kernel -----------------------------------------------------------------------------------------------------------------------
    const int64_t ns[] = {1, 8, 4095, 4096, 12287, 12288, 65536};
    const long long chain_mins[] = {-1, 0, 100, 5000};
    for (int topology = 0; topology < 9; ++topology)
    for (int64_t n : ns)
    for (long long chain_min : chain_mins)
    for (int env_set = 0; env_set < 2; ++env_set)
    for (int bits = 0; bits < (1 << 10); ++bits) {
        DispatchOpts o;
        DispatchFits f;
        o.chain_min = chain_min; o.env_chain_min_set = env_set != 0; o.env_chain_min = env_set ? 4096 : 12288;
        o.pinfo_structured = bits & 1; o.has_pinfo = bits & 2; o.pinfo_translation = bits & 4; o.has_off1 = bits & 8;
        o.wave3 = bits & 16; o.chain3 = bits & 32; o.natural_order = bits & 64;
        f.wave3 = bits & 128; f.wave3_pinfo = bits & 256; o.wave6 = bits & 512;
        f.nv_max = 64;
        const int got = pick_kernel(o, f, n, topology);
        // the rule of a handle without the option: a table or lever arms -> the general kernel, else the table-less rule
        const int before = (o.has_off1 || o.has_pinfo) ? (int)LOC_WINDOW_KERNEL_GENERAL : pick_kernel(without_table(o), f, n, topology);
        if (!o.pinfo_structured) { HOLD(got == before, "option 0: topology %d n %lld bits %d: %d, before %d", topology, (long long)n, bits, got, before); continue; }
        DispatchFits twin = f;
        twin.wave3 = true;   // (the twin's own fit flag stands in for wave3's)
        const bool expect = o.has_pinfo && o.pinfo_translation && !o.has_off1 && topology == LOC_WINDOW_KERNEL_CHAIN3 && f.wave3_pinfo &&
                            pick_kernel(without_table(o), twin, n, topology) == LOC_WINDOW_KERNEL_WAVE3;
        HOLD(got == (expect ? (int)LOC_WINDOW_KERNEL_WAVE3 : before), "option 1: topology %d n %lld bits %d: %d, expected %d", topology, (long long)n, bits, got,
             expect ? (int)LOC_WINDOW_KERNEL_WAVE3 : before);
        if (expect) {
            ++wave3_seen;
            HOLD(o.wave3 && o.chain3 && !o.natural_order && effective_chain_min(o) > 0, "WAVE3 under a switch that forbids it: bits %d", bits);
        }
        HOLD(structured_pinfo(o) == (o.has_pinfo && o.pinfo_translation && !o.has_off1), "structured_pinfo: bits %d", bits);
    }
    HOLD(wave3_seen > 0, "no row of the grid reached WAVE3");

    // ---- cov_admitted, cov_stale, cov_switches -------------------------------------------------------------------------------------------------
    for (int kind = -1; kind <= (int)CovKind::Envelope; ++kind)
    for (int nv_max = 64; nv_max <= 65; ++nv_max)
    for (int64_t n : {255, 256})
    for (int bits = 0; bits < (1 << 7); ++bits) {
        DispatchOpts o;
        DispatchFits f;
        o.pinfo_structured = bits & 1; o.has_pinfo = bits & 2; o.pinfo_translation = bits & 4; o.has_off1 = bits & 8; o.cov_general = bits & 16;
        o.tree = bits & 32 ? 0 : -1; o.arrow3 = bits & 64 ? 1 : -1;
        f.nv_max = nv_max; f.cov_arrow = true; f.cov_chain = true; f.cov_envelope = true;
        const CovKind k = (CovKind)kind;
        const bool got = cov_admitted(o, f, n, k);
        const bool plain = cov_admitted(without_table(o), f, n, k);
        const bool before = o.has_pinfo ? plain && k == CovKind::Envelope : plain;
        const bool expect = o.pinfo_structured && o.has_pinfo && o.pinfo_translation && !o.has_off1 && k == CovKind::Chain3 ? plain : before;
        HOLD(got == expect, "cov_admitted: kind %d nv_max %d bits %d: %d, expected %d", kind, nv_max, bits, (int)got, (int)expect);
        if (!o.pinfo_structured) HOLD(got == before, "cov_admitted, option 0: kind %d bits %d", kind, bits);
        if (got && o.has_pinfo && k == CovKind::Chain3) ++chain3_seen;
        // a batch the envelope pass holds is classified again when the option or the table's verdict has changed since
        const long long sw = cov_switches(o);
        HOLD(!cov_stale(o, f, n, CovKind::Envelope, sw), "cov_stale with its own switches: bits %d", bits);
        if (o.has_pinfo) {
            DispatchOpts p = o;
            p.pinfo_structured = !o.pinfo_structured;
            HOLD(cov_switches(p) != sw && cov_stale(p, f, n, CovKind::Envelope, sw), "cov_switches does not carry the option: bits %d", bits);
            p = o;
            p.pinfo_translation = !o.pinfo_translation;
            HOLD(cov_switches(p) != sw && cov_stale(p, f, n, CovKind::Envelope, sw), "cov_switches does not carry the table's translation-only verdict: bits %d", bits);
        }
        {
            DispatchOpts p = o;
            p.has_pinfo = !o.has_pinfo;
            if (!p.has_pinfo) p.pinfo_translation = false;   // (the setter clears it with the table)
            HOLD(cov_switches(p) != sw, "cov_switches does not carry has_pinfo: bits %d", bits);
        }
        // with the new fields at their defaults the word is the one of a handle without them
        if (!o.pinfo_structured && !o.has_pinfo) HOLD((sw >> 58) == 0, "cov_switches: bits above 57 without a table: bits %d", bits);
    }
    HOLD(chain3_seen > 0, "no row of the grid admitted Chain3 under a table");

    // ---- batch_topology's clause and covariance_kind on batches ------------------------------------------------------------------------------------
    long long topo_chain3 = 0, kind_chain3 = 0;
    for (int shape = 0; shape < 4; ++shape)          // 0 translation-only chain, 1 star, 2 a rotated pose, 3 a chain on a handle of 65 pose slots
    for (int nan_diag = 0; nan_diag < 2; ++nan_diag)
    for (int bits = 0; bits < (1 << 6); ++bits) {
        const int nv_max = shape == 3 ? 65 : 8;
        const Batch B = make_batch(nv_max, 6, 5, shape == 1, shape == 2, nan_diag != 0);
        const HostBatch hb = B.host(5);
        DispatchOpts o;
        DispatchFits f;
        o.arrow3 = 0; o.tree = 0;
        o.pinfo_structured = bits & 1; o.has_pinfo = bits & 2; o.pinfo_translation = bits & 4; o.has_off1 = bits & 8; o.cov_general = bits & 16;
        f.cov_chain = bits & 32; f.cov_envelope = true; f.nv_max = nv_max; f.wave3 = f.wave3_pinfo = nv_max <= 64; f.wave6 = true;
        HOLD(check_instances(B.c, 3, hb) == 0, "the driver's own batch is invalid");
        const bool structured = o.pinfo_structured && o.has_pinfo && o.pinfo_translation && !o.has_off1;
        const bool chain = shape != 1, translation = shape != 2 && (structured || !nan_diag);   // (NaN diagonals: translation-only only when they are skipped)
        WinAux aux;
        TopoCache tc;
        for (int pass = 0; pass < 2; ++pass) {   // (the second pass answers from the topology cache)
            const Topology t = batch_topology(B.c, o, f, 3, hb, aux, &tc);
            HOLD(t.cached == (pass == 1), "topology cache: shape %d bits %d pass %d", shape, bits, pass);
            HOLD((t.kind == LOC_WINDOW_KERNEL_CHAIN3) == (chain && translation), "batch_topology: shape %d nan %d bits %d: %d", shape, nan_diag, bits, t.kind);
            const int k = pick_kernel(o, f, hb.n, t.kind);
            const bool wave3 = chain && translation && nv_max <= 64 && !o.has_off1 && (!o.has_pinfo || structured);
            HOLD((k == LOC_WINDOW_KERNEL_WAVE3) == wave3, "solve kernel: shape %d nan %d bits %d: %d", shape, nan_diag, bits, k);
            if (o.has_pinfo && k == LOC_WINDOW_KERNEL_WAVE3) ++topo_chain3;
            if ((o.has_pinfo || o.has_off1) && !wave3) HOLD(k == LOC_WINDOW_KERNEL_GENERAL, "a table outside the rule must take the general kernel: shape %d bits %d: %d", shape, bits, k);
        }
        WinAux own;
        const CovVerdict v = covariance_kind(B.c, o, f, 3, hb, PairTables{0, nullptr, nullptr}, own, nullptr);
        CovKind expect;
        if (o.has_off1) expect = CovKind::None;
        else if (o.has_pinfo && !structured) expect = o.cov_general ? CovKind::Envelope : CovKind::None;
        else if (chain && nv_max <= 64 && f.cov_chain && (translation || !o.has_pinfo)) expect = translation ? CovKind::Chain3 : CovKind::Chain6;
        else expect = o.cov_general ? CovKind::Envelope : CovKind::None;   // (a structured table on anything else: the envelope pass, as with option 0)
        HOLD(v.kind == expect, "covariance_kind: shape %d nan %d bits %d: %d, expected %d", shape, nan_diag, bits, (int)v.kind, (int)expect);
        HOLD(v.kind == CovKind::None || cov_admitted(o, f, hb.n, v.kind), "a verdict that is not admitted: shape %d bits %d", shape, bits);
        if (o.has_pinfo && v.kind == CovKind::Chain3) ++kind_chain3;
    }
    HOLD(topo_chain3 > 0 && kind_chain3 > 0, "no batch reached the structured verdicts");
    std::printf("structured prior dispatch: %lld checks hold; WAVE3 under a table in %lld rows, Chain3 admitted in %lld, batches: %lld solves / %lld covariance verdicts\n",
                g_checks, wave3_seen, chain3_seen, topo_chain3, kind_chain3);
    return 0;
}
