// gfx950 (MI355X / CDNA4): the resident PLAIN-DROP slide of 6-DoF chain windows (loc_window_slide_plain_resident_dev; DESIGN.md §2, "The plain
// drop for 6-DoF chain windows"): what Robot::new_vertex does with its oldest pose (robot.cpp:92-98) — slot 0 of every uploaded window goes
// with every factor on it, NOTHING is carried, the newest pose and its factors are appended — in the device tables the batch lives in.  One
// launch: there is no marginal pass, no inserted prior row, no table of full information matrices.
//
// Mapping: one wave per window.  Each wave first admits its own window (slide_plain_admit.h's rule, rows over lanes, "any row" as a ballot)
// and leaves a refused window untouched.  Then every table (r_idx / r_val, p_idx / p_val, s_idx / s_val) is re-packed IN PLACE by
// window_slide_kernel.hip's ballot scheme, 64 rows per step in ascending order: the keep-mask is a ballot over the step's index rows, a kept
// row's destination the number of kept rows before it.  Both safety arguments of that kernel carry over unchanged:
//   (1) a step loads all of its rows (indices AND values) into registers, then wave_sync() (all loads have returned), then stores;
//   (2) destinations never pass sources (dst <= src for every kept row), so a step stores only to rows that this or an earlier step has
//       already loaded, and never to a row a later step still has to load.
// Nothing shifts up here (no carried row), so there is no descending loop.  No atomics and no dependence on the window's position in the
// batch: the same bits wherever the window sits.  Plain vector loads and stores only.
//
// It reads and writes nothing outside the handle's allocations and the caller's arrays — by induction over the calls on one resident batch:
//   * loc_window_upload validated counts[b] = (nv, nr, np, ns) against (nv_max, nr_max, np_max, ns_max); this kernel is the only writer of
//     counts next to window_slide_kernel (which never runs on a batch this one admits), and it writes (s + 1, r_kept + nrn, p_kept + npn,
//     s_kept + nsn) only after codes 4, 5, 6 and 8 have held each of them to its capacity.  So every loop over [0, count) below stays inside
//     window b's slice of r_idx / r_val, p_idx / p_val and s_idx / s_val — 2 / 5, 1 / 18 and 4 / 48 entries per row.
//   * a compaction step stores row dst <= src < count; the appended rows go to [kept, kept + new) with kept + new <= capacity (the same codes).
//   * the caller's new_r_* / new_p_* / new_s_* rows are read at e < nrn <= nr_new_max (..) only after code 2 has placed all three counts in range;
//     a count under a capacity of 0 is never read (its array may be NULL).
//   * poses: the kept poses move from [drop, nv) to [0, nv - drop), the new one goes to slot s <= nv_max - 1 (code 4); poses_in likewise.
// The VALUES the new rows carry (rotations, lever arms, information) are the caller's and are not looked at: every solve kernel of these
// verdicts evaluates them.
#include "slide_plain_admit.h"
#include "window_device.h"

namespace locamd {

namespace {

// The admission of ONE window by its wave: slide_plain_admit.h's rule.  Every lane returns the same code.
__device__ __forceinline__ int slide_plain_admit_wave(const SlidePlainArgs& s, long long b, int lane, int nv, int nr, int np, int ns, bool drop, int nrn, int npn, int nsn) {
    const WindowCaps& cp = s.caps;
    if (nv <= 0) return kSlideAdmitNoPoses;
    if (nrn < 0 || nrn > s.nr_new_max || npn < 0 || npn > s.np_new_max || nsn < 0 || nsn > s.ns_new_max) return kSlideAdmitCount;
    const int sl = nv - (drop ? 1 : 0);   // the new slot
    const u64 below = (1ull << lane) - 1;
    bool named = false, bad = false;      // a row of an earlier step names the new slot; a row so far breaks the index rule
    int pairs = 0;                        // new pose-to-pose range rows
    for (int e0 = 0; e0 < nrn; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < nrn;
        int v0 = 0, v1 = 0;
        if (in) { const int32_t* xi = s.new_r_idx + ((size_t)b * s.nr_new_max + e) * 2; v0 = xi[0]; v1 = xi[1]; }
        const bool ok0 = v0 == sl || (v0 == sl - 1 && v0 >= 0);
        const bool ok1 = v1 < 0 ? v1 >= -s.n_anchors : ((v1 == sl || v1 == sl - 1) && v1 != v0 && cp.bw_max >= 1);
        const bool names = in && (v0 == sl || v1 == sl);
        const u64 mn = __ballot(names);
        const bool after = named || (mn & below) != 0;   // a row before this one names s: this one has to as well
        bad = bad || __ballot(in && (!ok0 || !ok1 || (after && !names))) != 0;
        named = named || mn != 0;
        pairs += __popcll(__ballot(in && v1 >= 0));
    }
    for (int e0 = 0; e0 < nsn; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < nsn;
        int vi = 0, vj = 0;
        if (in) { const int32_t* xi = s.new_s_idx + ((size_t)b * s.ns_new_max + e) * 4; vi = xi[0]; vj = xi[1]; }
        const bool joins = (vi == sl - 1 && vj == sl) || (vi == sl && vj == sl - 1);
        bad = bad || __ballot(in && (!joins || sl < 1 || cp.bw_max < 1)) != 0;
    }
    if (bad) return kSlideAdmitIndex;
    // what the drop leaves
    int r_kept = nr, p_kept = np, s_kept = ns;
    if (drop) {
        r_kept = 0; p_kept = 0; s_kept = 0;
        const int32_t* ri = s.r_idx + (size_t)b * cp.nr_max * 2;
        const int32_t* pi = s.p_idx + (size_t)b * cp.np_max;
        const int32_t* si = s.s_idx + (size_t)b * cp.ns_max * 4;
        for (int e0 = 0; e0 < nr; e0 += 64) {
            const int e = e0 + lane;
            r_kept += __popcll(__ballot(e < nr && ri[e * 2] != 0 && ri[e * 2 + 1] != 0));
        }
        for (int e0 = 0; e0 < np; e0 += 64) {
            const int e = e0 + lane;
            p_kept += __popcll(__ballot(e < np && pi[e] != 0));
        }
        for (int e0 = 0; e0 < ns; e0 += 64) {
            const int e = e0 + lane;
            s_kept += __popcll(__ballot(e < ns && si[e * 4] != 0 && si[e * 4 + 1] != 0));
        }
    }
    if (sl + 1 > cp.nv_max) return kSlideAdmitNvMax;
    if (r_kept + nrn > cp.nr_max) return kSlideAdmitNrMax;
    if (p_kept + npn > cp.np_max) return kSlideAdmitNpMax;
    if (s_kept + nsn > cp.ns_max) return kSlideAdmitNsMax;
    if (s.pair_rule == kSlidePairsWave6 && (nsn > 0 || pairs > 1)) return kSlideAdmitPairs;
    if (s.pair_rule == kSlidePairsWave6S && (nsn > 1 || pairs > 1)) return kSlideAdmitPairs;
    return kSlideAdmitOk;
}

// The rows of a table pair (WI ints at ti, WV doubles at tv per row) without the rows on slot 0, compacted in place in ascending order;
// pose slots among the first NS ints of a row decrease by 1 (a negative entry is an anchor code and stays), the other ints travel as they
// are.  Returns how many rows are kept.
template <int WI, int NS, int WV>
__device__ __forceinline__ int slide_plain_compact(int32_t* ti, double* tv, int n, int lane) {
    int kept = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        int ix[WI];
        bool k = e < n;
#pragma unroll
        for (int j = 0; j < WI; ++j) ix[j] = e < n ? ti[(size_t)e * WI + j] : 0;
#pragma unroll
        for (int j = 0; j < NS; ++j) k = k && ix[j] != 0;
        double v[WV];
#pragma unroll
        for (int j = 0; j < WV; ++j) v[j] = k ? tv[(size_t)e * WV + j] : 0.0;
        const u64 m = __ballot(k);
        const int dst = kept + __popcll(m & ((1ull << lane) - 1));   // dst <= e: destinations never pass sources
        wave_sync();                                                 // every row of the step is in registers before any is stored
        if (k) {
#pragma unroll
            for (int j = 0; j < WI; ++j) ti[(size_t)dst * WI + j] = (j < NS && ix[j] > 0) ? ix[j] - 1 : ix[j];
#pragma unroll
            for (int j = 0; j < WV; ++j) tv[(size_t)dst * WV + j] = v[j];
        }
        kept += __popcll(m);
    }
    return kept;
}

__global__ void __launch_bounds__(64) window_slide_plain_kernel(const SlidePlainArgs s) {
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const WindowCaps& cp = s.caps;
    const int nv = s.counts[b * 4], nr = s.counts[b * 4 + 1], np = s.counts[b * 4 + 2], ns = s.counts[b * 4 + 3];
    const bool drop = s.drop == nullptr || s.drop[b] != 0;
    const int nrn = s.nr_new_max > 0 ? s.new_r_counts[b] : 0, npn = s.np_new_max > 0 ? s.new_p_counts[b] : 0, nsn = s.ns_new_max > 0 ? s.new_s_counts[b] : 0;
    const int code = slide_plain_admit_wave(s, b, lane, nv, nr, np, ns, drop, nrn, npn, nsn);
    if (lane == 0) {
        if (s.admit) s.admit[b] = code;
        if (s.status) s.status[b] = code == kSlideAdmitOk ? 0 : (code == kSlideAdmitPairs ? -5 : -1);   // LOC_OK / LOC_ERR_UNSUPPORTED / LOC_ERR_INVALID
    }
    if (code != kSlideAdmitOk) return;   // (the same code in every lane: the whole wave leaves, the window stays as it was)

    int32_t* ri = s.r_idx + (size_t)b * cp.nr_max * 2;
    double* rv = s.r_val + (size_t)b * cp.nr_max * 5;
    int32_t* pi = s.p_idx + (size_t)b * cp.np_max;
    double* pv = s.p_val + (size_t)b * cp.np_max * 18;
    int32_t* si = s.s_idx + (size_t)b * cp.ns_max * 4;
    double* sv = s.s_val + (size_t)b * cp.ns_max * 48;
    int nr_kept = nr, np_kept = np, ns_kept = ns;
    if (drop) {   // the rows with slot 0 as an endpoint go (a prior's one pose, both of a range's or an EdgeSE3's; s_idx[.][2..3] travel as they are)
        nr_kept = slide_plain_compact<2, 2, 5>(ri, rv, nr, lane);
        np_kept = slide_plain_compact<1, 1, 18>(pi, pv, np, lane);
        ns_kept = slide_plain_compact<4, 2, 48>(si, sv, ns, lane);
    }

    // ---- poses: x's kept poses (all 12 doubles) become slots 0 .. in the output array AND in the next solve's input estimates; then the new pose ----
    double* X = s.poses + (size_t)b * cp.nv_max * 12;
    double* Xin = s.poses_in + (size_t)b * cp.nv_max * 12;
    const int nv_kept = nv - (drop ? 1 : 0), from = drop ? 12 : 0;
    for (int i0 = 0; i0 < nv_kept * 12; i0 += 64) {   // (a step loads [i0 + from, i0 + from + 64) and stores [i0, i0 + 64): the same argument)
        const int i = i0 + lane;
        const bool k = i < nv_kept * 12;
        const double v = k ? X[i + from] : 0.0;
        wave_sync();
        if (k) { X[i] = v; Xin[i] = v; }
    }
    if (lane < 12) {
        const double v = s.new_pose[(size_t)b * 12 + lane];
        X[nv_kept * 12 + lane] = v; Xin[nv_kept * 12 + lane] = v;
    }

    // ---- the new rows, last ----------------------------------------------------------------------------------------------------------------------
    for (int j = lane; j < nrn; j += 64) {
        const int32_t* xi = s.new_r_idx + ((size_t)b * s.nr_new_max + j) * 2;
        const double* xv = s.new_r_val + ((size_t)b * s.nr_new_max + j) * 5;
        ri[(nr_kept + j) * 2] = xi[0]; ri[(nr_kept + j) * 2 + 1] = xi[1];
#pragma unroll
        for (int k = 0; k < 5; ++k) rv[(size_t)(nr_kept + j) * 5 + k] = xv[k];
    }
    for (int j = lane; j < npn; j += 64) {
        const double* xv = s.new_p_val + ((size_t)b * s.np_new_max + j) * 18;
        pi[np_kept + j] = nv_kept;   // the new slot
#pragma unroll
        for (int k = 0; k < 18; ++k) pv[(size_t)(np_kept + j) * 18 + k] = xv[k];
    }
    for (int j = lane; j < nsn; j += 64) {
        const int32_t* xi = s.new_s_idx + ((size_t)b * s.ns_new_max + j) * 4;
        const double* xv = s.new_s_val + ((size_t)b * s.ns_new_max + j) * 48;
#pragma unroll
        for (int k = 0; k < 4; ++k) si[(size_t)(ns_kept + j) * 4 + k] = xi[k];
#pragma unroll
        for (int k = 0; k < 48; ++k) sv[(size_t)(ns_kept + j) * 48 + k] = xv[k];
    }
    if (lane == 0) {
        s.counts[b * 4] = nv_kept + 1; s.counts[b * 4 + 1] = nr_kept + nrn; s.counts[b * 4 + 2] = np_kept + npn; s.counts[b * 4 + 3] = ns_kept + nsn;
    }
}

}  // namespace

hipError_t launch_window_slide_plain(const SlidePlainArgs& s, hipStream_t stream) {
    if (s.B <= 0) return hipSuccess;
    if (!s.counts || !s.poses || !s.poses_in || !s.new_pose) return hipErrorInvalidValue;
    if ((s.nr_new_max > 0 && (!s.new_r_counts || !s.new_r_idx || !s.new_r_val)) || (s.np_new_max > 0 && (!s.new_p_counts || !s.new_p_val)) ||
        (s.ns_new_max > 0 && (!s.new_s_counts || !s.new_s_idx || !s.new_s_val)))
        return hipErrorInvalidValue;
    if ((s.caps.nr_max > 0 && (!s.r_idx || !s.r_val)) || (s.caps.np_max > 0 && (!s.p_idx || !s.p_val)) || (s.caps.ns_max > 0 && (!s.s_idx || !s.s_val))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_slide_plain_kernel, dim3((unsigned)s.B), dim3(64), 0, stream, s);
    return hipGetLastError();
}

}  // namespace locamd
