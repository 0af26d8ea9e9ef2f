// gfx950 (MI355X / CDNA4): the resident fixed-lag slide (loc_window_slide_resident; DESIGN.md §2, "The resident slide"): drop slot 0 of every
// uploaded window, put the marginal prior it leaves in front of the kept priors, append the newest pose and its factors — in the device
// tables the batch lives in.  window_structure.cpp's slide_indices applies the same integer rule to the host's mirror and has admitted
// every count and index before this runs — or, behind loc_window_slide_resident_dev, nobody has: the ARGS = SlideDevArgs twin reads the
// caller's device arrays and each wave admits its own window first (slide_admit.h's rule), leaving a refused window untouched.
//
// Two launches.  The marginal of slot 0 is marginal_prior_kernel ITSELF (launch_window_marginal_prior with a drop table of zeros, into a
// scratch block of the handle): the one statement of that arithmetic, so loc_window_marginal_prior_host and the slide return the same bits,
// and that kernel's code and resource report stay what they were.  Folding it into this kernel would save one launch and a round trip of
// 60 doubles per window through HBM (3 % of what the slide moves) at the price of a second instantiation of the arithmetic.
//
// Mapping: one wave per window, as marginal_prior_kernel.  Every table is re-packed IN PLACE, 64 rows per step in ascending order: the
// keep-mask is a ballot, a kept row's destination the number of kept rows before it.  The safety argument of every loop below:
//   (1) a step loads all of its rows into registers, then wave_sync() (all loads have returned), then stores;
//   (2) destinations never pass sources (dst <= src for every kept row), so a step stores only to rows that this or an earlier step has
//       already loaded, and never to a row a later step still has to load.
// The carried prior needs the kept prior rows one row UP (dst = src + 1): that shift runs as a second loop from the top down, where the same
// argument holds mirrored (a step stores to rows above the ones the later, lower steps load).
// No atomics and no dependence on the window's position in the batch: the same bits wherever the window sits.  Plain vector loads and
// stores only.
#include <type_traits>

#include "slide_admit.h"
#include "window_device.h"

namespace locamd {

namespace {

// the rows keep(e) selects of the n rows of W doubles at t, compacted in place in ascending order; returns how many
template <int W, class Keep>
__device__ __forceinline__ int slide_compact(double* t, int n, int lane, Keep keep) {
    int kept = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        const bool k = e < n && keep(e);
        double v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = k ? t[(size_t)e * W + j] : 0.0;
        const u64 m = __ballot(k);
        const int dst = kept + __popcll(m & ((1ull << lane) - 1));   // dst <= e: destinations never pass sources
        wave_sync();                                                 // every row of the step is in registers before any is stored
        if (k) {
#pragma unroll
            for (int j = 0; j < W; ++j) t[(size_t)dst * W + j] = v[j];
        }
        kept += __popcll(m);
    }
    return kept;
}
// rows [0, n) of W doubles one row up, from the top down (row n must be free)
template <int W>
__device__ __forceinline__ void slide_shift_up(double* t, int n, int lane) {
    for (int hi = n; hi > 0; hi -= 64) {
        const int e = hi - 64 + lane;   // this step's rows: [max(hi - 64, 0), hi)
        const bool k = e >= 0;
        double v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = k ? t[(size_t)e * W + j] : 0.0;
        wave_sync();
        if (k) {
#pragma unroll
            for (int j = 0; j < W; ++j) t[(size_t)(e + 1) * W + j] = v[j];   // rows (hi - 64, hi]: above everything the later steps load
        }
    }
}

// the twin's arguments: the re-pack's, and what the admission needs on top (all of s's input arrays are then the CALLER's device memory)
struct SlideDevArgs : SlideArgs {
    int n_anchors;    // the anchor table's size at call time: new anchor codes are admitted against it
    int32_t* admit;   // [B] the admission code of every window, may be nullptr
};

// The admission of ONE window by its wave (loc_window_slide_resident_dev): slide_admit.h's rule, rows over lanes, "any row" as a ballot.  Every
// lane returns the same code.  Reads the window's own index tables (valid by induction: the upload validated them and every slide either
// admits a window or leaves it alone) and the caller's new rows — never a row beyond a count, and no row before both counts are in range.
__device__ __forceinline__ int slide_admit_wave(const SlideArgs& s, int n_anchors, long long b, int lane, int nv, int nr, int np, bool drop, int nrn, int npn) {
    const WindowCaps& cp = s.caps;
    if (nv <= 0) return kSlideAdmitNoPoses;
    if (nrn < 0 || nrn > s.nr_new_max || npn < 0 || npn > s.np_new_max) return kSlideAdmitCount;
    const int sl = nv - (drop ? 1 : 0);   // the new slot
    const u64 below = (1ull << lane) - 1;
    bool named = false, bad = false;      // a row of an earlier step names the new slot; a row so far breaks rule 3
    for (int e0 = 0; e0 < nrn; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < nrn;
        int v0 = 0, v1 = 0;
        if (in) { const int32_t* xi = s.new_r_idx + ((size_t)b * s.nr_new_max + e) * 2; v0 = xi[0]; v1 = xi[1]; }
        const bool ok0 = v0 == sl || (v0 == sl - 1 && v0 >= 0);
        const bool ok1 = v1 < 0 ? v1 >= -n_anchors : ((v1 == sl || v1 == sl - 1) && v1 != v0 && cp.bw_max >= 1);
        const bool names = in && (v0 == sl || v1 == sl);
        const u64 mn = __ballot(names);
        const bool after = named || (mn & below) != 0;   // a row before this one names s: this one has to as well
        bad = bad || __ballot(in && (!ok0 || !ok1 || (after && !names))) != 0;
        named = named || mn != 0;
    }
    if (bad) return kSlideAdmitIndex;
    // what the drop leaves: the kept rows, and whether a pose-to-pose range joined slot 0 to another pose (the marginal's slot >= 0)
    int r_kept = nr, p_kept = np, carried = 0;
    if (drop) {
        r_kept = 0; p_kept = 0;
        const int32_t* ri = s.r_idx + (size_t)b * cp.nr_max * 2;
        const int32_t* pi = s.p_idx + (size_t)b * cp.np_max;
        for (int e0 = 0; e0 < nr; e0 += 64) {
            const int e = e0 + lane;
            int v0 = 1, v1 = 1;
            if (e < nr) { v0 = ri[e * 2]; v1 = ri[e * 2 + 1]; }
            const bool gone = v0 == 0 || v1 == 0;
            r_kept += __popcll(__ballot(e < nr && !gone));
            if (__ballot(gone && v1 >= 0) != 0) carried = 1;
        }
        for (int e0 = 0; e0 < np; e0 += 64) {
            const int e = e0 + lane;
            p_kept += __popcll(__ballot(e < np && pi[e] != 0));
        }
    }
    if (sl + 1 > cp.nv_max) return kSlideAdmitNvMax;
    if (r_kept + nrn > cp.nr_max) return kSlideAdmitNrMax;
    if (carried + p_kept + npn > cp.np_max) return kSlideAdmitNpMax;
    // the value half: identity rotations by their bit pattern, no lever arm, no rotation information
    bool other = false;
    if (lane < 9) other = (u64)__double_as_longlong(s.new_pose[(size_t)b * 12 + lane]) != (lane % 4 == 0 ? 0x3FF0000000000000ull : 0ull);
    for (int j = lane; j < nrn; j += 64) {
        const double* v = s.new_r_val + ((size_t)b * s.nr_new_max + j) * 5;
        other = other || v[2] != 0.0 || v[3] != 0.0 || v[4] != 0.0;
    }
    for (int j = lane; j < npn; j += 64) {
        const double* v = s.new_p_val + ((size_t)b * s.np_new_max + j) * 18;
        other = other || !slide_identity_bits(v) || v[15] != 0.0 || v[16] != 0.0 || v[17] != 0.0;
    }
    if (__ballot(other) != 0) return kSlideAdmitNotTranslation;
    return kSlideAdmitOk;
}

// DENSIFY: the handle had no table of full information matrices so far — p_info is new, and every row it gets is diag(p_val[12..17]) but
// the carried one.  ARGS = SlideDevArgs (ADMIT, loc_window_slide_resident_dev): the host has admitted nothing — the wave first admits its window, then either
// re-packs it exactly as below or writes the refusal's outputs and leaves every table row, pose and count as it was; s.drop may be nullptr
// (every window drops).  Without ADMIT the host has admitted every window and the code is what it was before the parameter existed.
template <bool DENSIFY, class ARGS>
__global__ void __launch_bounds__(64) window_slide_kernel(const ARGS s) {
    constexpr bool ADMIT = std::is_same<ARGS, SlideDevArgs>::value;
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const WindowCaps& cp = s.caps;
    const int nv = s.counts[b * 4], nr = s.counts[b * 4 + 1], np = s.counts[b * 4 + 2];
    const bool drop = ADMIT ? (s.drop == nullptr || s.drop[b] != 0) : s.drop[b] != 0;
    int nrn_in = 0, npn_in = 0;
    if constexpr (ADMIT) {
        nrn_in = s.nr_new_max > 0 ? s.new_r_counts[b] : 0; npn_in = s.np_new_max > 0 ? s.new_p_counts[b] : 0;
        const int code = slide_admit_wave(s, s.n_anchors, b, lane, nv, nr, np, drop, nrn_in, npn_in);
        if (lane == 0 && s.admit) s.admit[b] = code;
        if (code != kSlideAdmitOk) {   // (the same code in every lane: the whole wave leaves)
            if (s.prior && lane < 48) s.prior[(size_t)b * 48 + lane] = 0.0;
            if (lane == 0) {
                if (s.slot) s.slot[b] = -1;
                if (s.rank) s.rank[b] = 0;
                if (s.status) s.status[b] = code == kSlideAdmitNotTranslation ? -5 : -1;   // LOC_ERR_UNSUPPORTED / LOC_ERR_INVALID
            }
            if (DENSIFY) {   // the handle has a table from now on, for this window as well: its rows are the diagonals p_val holds
                const double* pv = s.p_val + (size_t)b * cp.np_max * 18;
                double* pw = s.p_info + (size_t)b * cp.np_max * 36;
                for (int e = lane; e < np; e += 64) {
#pragma unroll
                    for (int k = 0; k < 36; ++k) pw[(size_t)e * 36 + k] = (k % 7 == 0) ? pv[(size_t)e * 18 + 12 + k / 7] : 0.0;
                }
            }
            return;
        }
    }
    const int mslot = drop ? s.m_slot[b] : -1;     // the marginal's neighbour: slot 1 of an ordered chain, or none
    const int ins = mslot >= 0 ? 1 : 0;            // the carried prior takes row 0
    // lanes 0 .. 47: the marginal's row (a window that only grows reports zeros)
    const double prow = (drop && lane < 48) ? s.m_prior[(size_t)b * 48 + lane] : 0.0;
    if (s.prior && lane < 48) s.prior[(size_t)b * 48 + lane] = prow;
    if (lane == 0) {
        if (s.slot) s.slot[b] = mslot;
        if (s.rank) s.rank[b] = drop ? s.m_rank[b] : 0;
        if (s.status) s.status[b] = drop ? s.m_status[b] : 0;
    }

    // ---- ranges: the rows with slot 0 as an endpoint go, moving slots decrease by 1 (anchor codes -1 - a are < 0 and stay) ---------------------
    int32_t* ri = s.r_idx + (size_t)b * cp.nr_max * 2;
    double* rv = s.r_val + (size_t)b * cp.nr_max * 5;
    int nr_kept = nr;
    if (drop) {
        nr_kept = 0;
        for (int e0 = 0; e0 < nr; e0 += 64) {
            const int e = e0 + lane;
            int v0 = 0, v1 = 0;
            if (e < nr) { v0 = ri[e * 2]; v1 = ri[e * 2 + 1]; }
            const bool k = e < nr && v0 != 0 && v1 != 0;
            double v[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) v[j] = k ? rv[(size_t)e * 5 + j] : 0.0;
            const u64 m = __ballot(k);
            const int dst = nr_kept + __popcll(m & ((1ull << lane) - 1));   // dst <= e: destinations never pass sources
            wave_sync();                                                    // every row of the step is in registers before any is stored
            if (k) {
                ri[dst * 2] = v0 - 1; ri[dst * 2 + 1] = v1 > 0 ? v1 - 1 : v1;
#pragma unroll
                for (int j = 0; j < 5; ++j) rv[(size_t)dst * 5 + j] = v[j];
            }
            nr_kept += __popcll(m);
        }
    }

    // ---- poses: x's kept poses become slots 0 .. in the output array AND in the next solve's input estimates; then the new pose ------------------
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

    // ---- priors: the rows on slot 0 go (p_val, the table, p_idx last: it is the keep rule of all three); the kept rows one up for the carried one ----
    int32_t* pi = s.p_idx + (size_t)b * cp.np_max;
    double* pv = s.p_val + (size_t)b * cp.np_max * 18;
    double* pw = s.p_info + (size_t)b * cp.np_max * 36;
    int np_kept = np;
    if (drop) {
        const auto keep = [&](int e) { return pi[e] != 0; };
        np_kept = slide_compact<18>(pv, np, lane, keep);
        if (!DENSIFY) slide_compact<36>(pw, np, lane, keep);
        int kept = 0;
        for (int e0 = 0; e0 < np; e0 += 64) {
            const int e = e0 + lane;
            const int v = e < np ? pi[e] : 0;
            const bool k = v != 0;
            const u64 m = __ballot(k);
            const int dst = kept + __popcll(m & ((1ull << lane) - 1));
            wave_sync();
            if (k) pi[dst] = v - 1;
            kept += __popcll(m);
        }
        if (ins) {
            slide_shift_up<18>(pv, np_kept, lane);
            if (!DENSIFY) slide_shift_up<36>(pw, np_kept, lane);
            for (int hi = np_kept; hi > 0; hi -= 64) {
                const int e = hi - 64 + lane;
                const int v = e >= 0 ? pi[e] : 0;
                wave_sync();
                if (e >= 0) pi[e + 1] = v;
            }
            // row 0 on slot 0: p_val[0..11] = prior[0..11], p_val[12..17] = the information's diagonal, table row = the information
            if (lane < 12) pv[lane] = prow;
            if (lane >= 12 && lane < 48) {
                pw[lane - 12] = prow;
                if ((lane - 12) % 7 == 0) pv[12 + (lane - 12) / 7] = prow;
            }
            if (lane == 0) pi[0] = mslot - 1;
        }
    }

    // ---- the new rows, last ----------------------------------------------------------------------------------------------------------------------
    const int nrn = ADMIT ? nrn_in : (s.nr_new_max > 0 ? s.new_r_counts[b] : 0), npn = ADMIT ? npn_in : (s.np_new_max > 0 ? s.new_p_counts[b] : 0);
    for (int j = lane; j < nrn; j += 64) {
        const int32_t* xi = s.new_r_idx + ((size_t)b * s.nr_new_max + j) * 2;
        const double* xv = s.new_r_val + ((size_t)b * s.nr_new_max + j) * 5;
        ri[(nr_kept + j) * 2] = xi[0]; ri[(nr_kept + j) * 2 + 1] = xi[1];
#pragma unroll
        for (int k = 0; k < 5; ++k) rv[(size_t)(nr_kept + j) * 5 + k] = xv[k];
    }
    const int np0 = np_kept + ins;
    for (int j = lane; j < npn; j += 64) {
        const double* xv = s.new_p_val + ((size_t)b * s.np_new_max + j) * 18;
        pi[np0 + j] = nv_kept;   // the new slot
#pragma unroll
        for (int k = 0; k < 18; ++k) pv[(size_t)(np0 + j) * 18 + k] = xv[k];
        if (!DENSIFY) {
#pragma unroll
            for (int k = 0; k < 36; ++k) pw[(size_t)(np0 + j) * 36 + k] = (k % 7 == 0) ? xv[12 + k / 7] : 0.0;
        }
    }
    if (DENSIFY) {   // the new table: every row but the carried one is the diagonal p_val holds (rows other lanes have just stored among them)
        wave_sync();
        for (int e = ins + lane; e < np0 + npn; e += 64) {
#pragma unroll
            for (int k = 0; k < 36; ++k) pw[(size_t)e * 36 + k] = (k % 7 == 0) ? pv[(size_t)e * 18 + 12 + k / 7] : 0.0;
        }
    }
    if (lane == 0) {
        s.counts[b * 4] = nv_kept + 1; s.counts[b * 4 + 1] = nr_kept + nrn; s.counts[b * 4 + 2] = np0 + npn;
    }
}

}  // namespace

hipError_t launch_window_slide(const SlideArgs& s, bool densify, hipStream_t stream) {
    if (s.B <= 0) return hipSuccess;
    if (!s.counts || !s.poses || !s.poses_in || !s.drop || !s.new_pose || !s.m_slot || !s.m_prior || !s.m_rank || !s.m_status) return hipErrorInvalidValue;
    if (densify) hipLaunchKernelGGL((window_slide_kernel<true, SlideArgs>), dim3((unsigned)s.B), dim3(64), 0, stream, s);
    else hipLaunchKernelGGL((window_slide_kernel<false, SlideArgs>), dim3((unsigned)s.B), dim3(64), 0, stream, s);
    return hipGetLastError();
}

hipError_t launch_window_slide_dev(const SlideArgs& s, int n_anchors, int32_t* admit, bool densify, hipStream_t stream) {
    if (s.B <= 0) return hipSuccess;
    if (!s.counts || !s.poses || !s.poses_in || !s.new_pose || !s.m_slot || !s.m_prior || !s.m_rank || !s.m_status) return hipErrorInvalidValue;
    if ((s.nr_new_max > 0 && (!s.new_r_counts || !s.new_r_idx || !s.new_r_val)) || (s.np_new_max > 0 && (!s.new_p_counts || !s.new_p_val))) return hipErrorInvalidValue;
    if ((s.caps.nr_max > 0 && (!s.r_idx || !s.r_val)) || (s.caps.np_max > 0 && (!s.p_idx || !s.p_val || !s.p_info))) return hipErrorInvalidValue;
    SlideDevArgs d;
    static_cast<SlideArgs&>(d) = s; d.n_anchors = n_anchors; d.admit = admit;
    if (densify) hipLaunchKernelGGL((window_slide_kernel<true, SlideDevArgs>), dim3((unsigned)s.B), dim3(64), 0, stream, d);
    else hipLaunchKernelGGL((window_slide_kernel<false, SlideDevArgs>), dim3((unsigned)s.B), dim3(64), 0, stream, d);
    return hipGetLastError();
}

}  // namespace locamd
