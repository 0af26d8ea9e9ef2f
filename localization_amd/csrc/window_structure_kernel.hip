// gfx950 (MI355X / CDNA4): the forest and arrowhead verdicts of a batch that arrived in the caller's DEVICE arrays, and arrow3_lm_kernel's
// row order and packed records (loc_window_upload_dev under option "upload_dev_structures"; DESIGN.md §2, "Upload from device arrays"): what
// build_arrow_aux and the first loop of build_tree_sched (window_structure.cpp) do on the host for loc_window_upload.  arrow_pack.h states the
// arrowhead rule for ONE window as two functions; this file restates both lane-parallel.
//
// Mapping: one wave per window, the windows dealt round-robin to the waves of the launch (four waves per workgroup, at most kStructMaxWaves),
// as the admit pass deals them.  Rows over lanes in steps of 64; "any row" is a ballot, a maximum over rows a butterfly.
// window_structure_kernel: (arrow) nb0 is a maximum over the range rows; the shape that follows from (nv, nb0) is closed-form (arrow_shape,
//   arrow_row), so hdr and rslot are written without a table; the records a row owns, the priors on it, the ranges on a consecutive chain pair
//   and the degree of a pose slot are counted with LDS atomics in four counter arrays of the wave's own (order is free: they are counts), and
//   the maxima are taken chunk by chunk of 64 rows, lane = row.  (forest) the window's four counts and the USED rows of r_idx, p_idx and s_idx
//   — window 0's counts of them, never a row at or beyond a count — are compared with window 0's, element-wise over lanes.
//   Each wave writes ONE partial record (arrow_pack.h: WindowStructRecord); window_structure_reduce_kernel, one wave, merges them.  AND and
//   maximum are associative and commutative: the batch record is the same bits whatever the launch geometry.
// arrow_pack_kernel: lanes over the range (prior) rows in table order, 64 a step.  A row's k-th record is its k-th row in table order: within
//   a step the lanes that share an owner row are found by a ballot (one round per distinct owner of the step) and take the slots
//   base + (their rank among those lanes, in lane order), base = the owner's running count in LDS from the steps before — order-preserving
//   without atomics.  Afterwards lane = row of a chunk fills the slots from the row's count on with -1.0 / 0.0 (rows from nv on: all of them),
//   so every double of rec / prec is written exactly once.
//
// It reads nothing outside the batch's tables and writes nothing outside hdr / rslot / partial / record / rec / prec:
//   * the batch has passed window_admit_kernel.hip and the tables are the handle's own copies: 0 <= count <= capacity, every v0 and prior
//     pose in [0, nv), every v1 in [-n_anchors, nv), v0 != v1.  Window b's slices as in window_admit_kernel.hip, offsets in size_t; loads are at
//     rows below the window's count (forest: below window 0's count, after the counts were found equal).
//   * NO value read from a table becomes an address before it has been range-checked here again: a row whose indices are outside [0, nv) /
//     above nv refuses the window (arrow) or is skipped (pack) before arrow_row turns it into a row in [0, nv); LDS counters are indexed by
//     that row or that slot alone, the arrays hold nvp = 64 ceil(nv_max / 64) >= nv entries each.
//   * rslot[b nv_max + r], r in [0, nv_max): arrow_row is a permutation of [0, nv), the slots from nv on are zeroed; hdr[8 b ..].
//   * rec / prec: row < nv <= nv_max gives a chunk < nchunk; a slot is stored only when it is < jmax / jpmax, the sizes the tables were
//     allocated with (the structure pass counted the same rows, so it always is).
//   * partial[wave] with wave < waves of the launch <= kStructMaxWaves, the size the entry allocates.
#include "arrow_pack.h"
#include "window_device.h"

namespace locamd {

namespace {

__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { const int o = __shfl_xor(v, s); v = o > v ? o : v; }
    return v;
}

// arrow_window_structure for window b by its wave: the same verdict and maxima in every lane.  cnt: 4 nvp LDS ints of the wave's own
__device__ __forceinline__ bool arrow_structure_wave(const WindowStructArgs& a, size_t b, int lane, int nv, int nr, int np, int nvp, int32_t* cnt, ArrowMaxima& m) {
    const WindowCaps& cp = a.caps;
    const int32_t* ri = a.r_idx + b * cp.nr_max * 2;
    const int32_t* pi = a.p_idx + b * cp.np_max;
    bool bad = false;
    int nb0 = 0;
    for (int e0 = 0; e0 < nr; e0 += 64) {
        const int e = e0 + lane;
        if (e < nr) {
            const int v0 = ri[2 * (size_t)e], v1 = ri[2 * (size_t)e + 1];
            if (v0 < 0 || v0 >= nv || v1 >= nv || v1 == v0) bad = true;                   // (admitted: cannot happen)
            else if (v1 < 0) bad = bad || -1 - (long long)v1 >= kArrowPackAnchors;
            else {
                const int hi = v0 > v1 ? v0 : v1, lo = v0 > v1 ? v1 : v0;
                if (hi - lo != 1 && nv - hi > nb0) nb0 = nv - hi;
            }
        }
    }
    for (int e0 = 0; e0 < np; e0 += 64) {
        const int e = e0 + lane;
        if (e < np) { const int v = pi[e]; bad = bad || v < 0 || v >= nv; }              // (admitted: cannot happen)
    }
    if (__ballot(bad) != 0) return false;
    nb0 = wave_imax(nb0);
    if (nb0 < 1 || nb0 > kArrowBorderMax || nv - nb0 < 2) return false;
    const ArrowShape s = arrow_shape(nv, nb0);
    if (lane == 0) {
        int32_t h[8];
        arrow_header(s, h);
#pragma unroll
        for (int k = 0; k < 8; ++k) a.hdr[b * 8 + k] = h[k];
    }
    int32_t* rs = a.rslot + b * cp.nv_max;
    for (int v = lane; v < cp.nv_max; v += 64) {
        if (v < nv) rs[arrow_row(s, v)] = v;
        else rs[v] = 0;
    }
    int32_t *nedge = cnt, *nprior = cnt + nvp, *pairs = cnt + 2 * nvp, *deg = cnt + 3 * nvp;
    for (int i = lane; i < 4 * nvp; i += 64) cnt[i] = 0;
    wave_sync();
    for (int e0 = 0; e0 < nr; e0 += 64) {
        const int e = e0 + lane;
        if (e < nr) {
            const int v0 = ri[2 * (size_t)e], v1 = ri[2 * (size_t)e + 1];   // (checked above)
            const ArrowOwner o = arrow_range_owner(s, v0, v1);
            if (o.refusal != kArrowOk) bad = true;
            else {
                atomicAdd(&nedge[o.row], 1);
                if (o.chain_pair) atomicAdd(&pairs[o.row], 1);
                atomicAdd(&deg[v0], 1);
                if (v1 >= 0) atomicAdd(&deg[v1], 1);
            }
        }
    }
    for (int e0 = 0; e0 < np; e0 += 64) {
        const int e = e0 + lane;
        if (e < np) {
            const int v = pi[e];
            atomicAdd(&nprior[arrow_row(s, v)], 1);
            atomicAdd(&deg[v], 1);
        }
    }
    wave_sync();
    ArrowMaxima w = arrow_maxima_empty();
    const int nchunk = nvp / 64;
#pragma unroll
    for (int ch = 0; ch < kArrowChunks; ++ch) {
        if (ch < nchunk) {   // (rows from nv on hold 0)
            const int r = ch * 64 + lane;
            const int je = wave_imax(nedge[r]), jp = wave_imax(nprior[r]);
            bad = bad || pairs[r] > 1;
            w.jch[ch] = je > 1 ? je : 1; w.jpch[ch] = jp > 1 ? jp : 1;
            w.jmax = je > w.jmax ? je : w.jmax; w.jpmax = jp > w.jpmax ? jp : w.jpmax;
        }
    }
    for (int ch = kArrowChunks; ch < nchunk; ++ch) {
        const int r = ch * 64 + lane;
        const int je = wave_imax(nedge[r]), jp = wave_imax(nprior[r]);
        bad = bad || pairs[r] > 1;
        w.jmax = je > w.jmax ? je : w.jmax; w.jpmax = jp > w.jpmax ? jp : w.jpmax;
    }
    int cap = 1;
    for (int v = lane; v < s.n0; v += 64) cap = deg[v] > cap ? deg[v] : cap;
    w.list_cap = wave_imax(cap);
    w.nb_max = s.nb;
    wave_sync();   // (the counters are zeroed again for the wave's next window)
    if (__ballot(bad) != 0) return false;
    arrow_maxima_merge(m, w);
    return true;
}

// build_tree_sched's "one topology": window b's counts and used index rows against window 0's
__device__ __forceinline__ bool equals_window0(const WindowStructArgs& a, size_t b, int lane, const int32_t* cn) {
    const WindowCaps& cp = a.caps;
    const int nv = a.counts[0], nr = a.counts[1], np = a.counts[2], ns = a.counts[3];
    if (cn[0] != nv || cn[1] != nr || cn[2] != np || cn[3] != ns) return false;
    bool diff = false;
    const int32_t *r0 = a.r_idx, *rb = a.r_idx + b * cp.nr_max * 2;
    for (int i = lane; i < 2 * nr; i += 64) diff = diff || r0[i] != rb[i];
    const int32_t *p0 = a.p_idx, *pb = a.p_idx + b * cp.np_max;
    for (int i = lane; i < np; i += 64) diff = diff || p0[i] != pb[i];
    const int32_t *s0 = a.s_idx, *sb = a.s_idx + b * cp.ns_max * 4;
    for (int i = lane; i < 4 * ns; i += 64) diff = diff || s0[i] != sb[i];
    return __ballot(diff) == 0;
}

__global__ void __launch_bounds__(256) window_structure_kernel(const WindowStructArgs a) {
    extern __shared__ int32_t lds[];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wave = (int)blockIdx.x * 4 + wib;
    const int nwaves = (int)gridDim.x * 4;
    const int nvp = (a.caps.nv_max + 63) / 64 * 64;
    int32_t* cnt = lds + (size_t)wib * 4 * nvp;
    WindowStructRecord r = struct_record_empty();
    if (!a.arrow) r.and_bits &= ~(uint32_t)kStructArrow;
    if (!a.forest) r.and_bits &= ~(uint32_t)kStructEqual0;
    for (long long b = wave; b < a.B; b += nwaves) {
        const int32_t* cn = a.counts + (size_t)b * 4;
        const int nv = cn[0], nr = cn[1], np = cn[2];
        if (a.arrow && !arrow_structure_wave(a, (size_t)b, lane, nv, nr, np, nvp, cnt, r.arrow)) r.and_bits &= ~(uint32_t)kStructArrow;
        if (a.forest && !equals_window0(a, (size_t)b, lane, cn)) r.and_bits &= ~(uint32_t)kStructEqual0;
    }
    if (lane == 0) a.partial[wave] = r;
}

// one wave: the partial records of the first launch, lanes over records, then a butterfly over the lanes
__global__ void __launch_bounds__(64) window_structure_reduce_kernel(const WindowStructRecord* partial, int n_partial, WindowStructRecord* record) {
    const int lane = threadIdx.x;
    WindowStructRecord r = struct_record_empty();
    for (int j = lane; j < n_partial; j += 64) struct_record_merge(r, partial[j]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        WindowStructRecord o = r;
        o.and_bits = (uint32_t)__shfl_xor((int)r.and_bits, s);
        o.arrow.nb_max = __shfl_xor(r.arrow.nb_max, s); o.arrow.jmax = __shfl_xor(r.arrow.jmax, s);
        o.arrow.jpmax = __shfl_xor(r.arrow.jpmax, s); o.arrow.list_cap = __shfl_xor(r.arrow.list_cap, s);
#pragma unroll
        for (int k = 0; k < kArrowChunks; ++k) { o.arrow.jch[k] = __shfl_xor(r.arrow.jch[k], s); o.arrow.jpch[k] = __shfl_xor(r.arrow.jpch[k], s); }
        struct_record_merge(r, o);
    }
    if (lane == 0) *record = r;
}

// The slots of one step's rows: row = the lane's owner row (< 0: the lane holds no row).  Lanes that share an owner take base + rank in lane
// order, base = run[row] as the steps before left it; run[row] is advanced by their number.  One round per distinct owner of the step.
__device__ __forceinline__ int step_slots(int row, int lane, int32_t* run) {
    const u64 below = (1ull << lane) - 1;
    u64 todo = __ballot(row >= 0);
    int slot = 0;
    while (todo != 0) {
        const int leader = __builtin_ctzll(todo);
        const int lr = __shfl(row, leader);
        const u64 same = __ballot(row == lr);
        const int base = run[lr];
        if (row == lr) slot = base + __popcll(same & below);
        wave_sync();
        if (lane == leader) run[lr] = base + __popcll(same);
        wave_sync();
        todo &= ~same;
    }
    return slot;
}

__global__ void __launch_bounds__(256) arrow_pack_kernel(const ArrowPackArgs a) {
    extern __shared__ int32_t lds[];
    const WindowCaps& cp = a.caps;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wave = (int)blockIdx.x * 4 + wib;
    const int nwaves = (int)gridDim.x * 4;
    const int nvp = a.nchunk * 64;
    int32_t *nedge = lds + (size_t)wib * 2 * nvp, *nprior = nedge + nvp;
    const size_t rec_per = arrow_rec_doubles(a.nchunk, a.jmax), prec_per = arrow_prec_doubles(a.nchunk, a.jpmax);
    for (long long bb = wave; bb < a.B; bb += nwaves) {
        const size_t b = (size_t)bb;
        const int32_t* cn = a.counts + b * 4;
        const int nv = cn[0], nr = cn[1], np = cn[2];
        const int32_t* hdr = a.hdr + b * 8;
        const int32_t h0 = hdr[0], h1 = hdr[1], h2 = hdr[2];
        const int32_t h[3] = {h0, h1, h2};
        const ArrowShape s = arrow_shape_of(h);
        double* rec = a.rec + b * rec_per;
        double* prec = a.prec + b * prec_per;
        for (int i = lane; i < 2 * nvp; i += 64) nedge[i] = 0;
        wave_sync();
        const bool shaped = s.nv == nv && s.nb0 >= 1 && s.n0 >= 2;   // (the structure pass took the window: always)
        const int32_t* ri = a.r_idx + b * cp.nr_max * 2;
        const double* rv = a.r_val + b * cp.nr_max * 5;
        for (int e0 = 0; e0 < nr && shaped; e0 += 64) {
            const int e = e0 + lane;
            int row = -1, code = 0;
            double meas = 0.0, info = 0.0;
            if (e < nr) {
                const int v0 = ri[2 * (size_t)e], v1 = ri[2 * (size_t)e + 1];
                meas = rv[5 * (size_t)e]; info = rv[5 * (size_t)e + 1];
                if (v0 >= 0 && v0 < nv && v1 < nv && v1 != v0) {
                    const ArrowOwner o = arrow_range_owner(s, v0, v1);
                    if (o.refusal == kArrowOk) { row = o.row; code = o.code; }
                }
            }
            const int slot = step_slots(row, lane, nedge);
            if (row >= 0 && slot < a.jmax) {
                double* q = rec + arrow_rec_at(a.jmax, row, slot);
                q[0] = (double)code; q[1] = meas; q[2] = info;
            }
        }
        const int32_t* pi = a.p_idx + b * cp.np_max;
        const double* pv = a.p_val + b * cp.np_max * 18;
        for (int e0 = 0; e0 < np && shaped; e0 += 64) {
            const int e = e0 + lane;
            int row = -1;
            double six[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (e < np) {
                const int v = pi[e];
#pragma unroll
                for (int k = 0; k < 6; ++k) six[k] = pv[18 * (size_t)e + 9 + k];
                if (v >= 0 && v < nv) row = arrow_row(s, v);
            }
            const int slot = step_slots(row, lane, nprior);
            if (row >= 0 && slot < a.jpmax) {
                double* q = prec + arrow_prec_at(a.jpmax, row, slot);
                q[0] = 1.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) q[1 + k] = six[k];
            }
        }
        // the fill: every slot no record took (lane = row of the chunk)
        for (int ch = 0; ch < a.nchunk; ++ch) {
            const int r = ch * 64 + lane;
            for (int k = nedge[r]; k < a.jmax; ++k) {
                double* q = rec + arrow_rec_at(a.jmax, r, k);
                q[0] = -1.0; q[1] = -1.0; q[2] = -1.0;
            }
            for (int k = nprior[r]; k < a.jpmax; ++k) {
                double* q = prec + arrow_prec_at(a.jpmax, r, k);
#pragma unroll
                for (int j = 0; j < 7; ++j) q[j] = 0.0;
            }
        }
        wave_sync();   // (the counters are zeroed again for the wave's next window)
    }
}

int structure_waves(long long B) {
    const long long blocks = (B + 3) / 4;
    return (int)(blocks < kStructMaxWaves / 4 ? blocks : kStructMaxWaves / 4) * 4;
}

}  // namespace

size_t window_structure_lds_bytes(const WindowCaps& c) { return (size_t)4 * 4 * ((c.nv_max + 63) / 64 * 64) * sizeof(int32_t); }

hipError_t launch_window_structure(const WindowStructArgs& a, hipStream_t stream) {
    if (a.B <= 0 || !a.counts || !a.partial || !a.record || (!a.arrow && !a.forest)) return hipErrorInvalidValue;
    if ((a.caps.nr_max > 0 && !a.r_idx) || (a.caps.np_max > 0 && !a.p_idx) || (a.caps.ns_max > 0 && !a.s_idx) || (a.arrow && (!a.hdr || !a.rslot))) return hipErrorInvalidValue;
    const size_t lds = a.arrow ? window_structure_lds_bytes(a.caps) : 0;
    if (lds > 64 * 1024) return hipErrorInvalidValue;   // (arrow3_fits bounds nv_max far below: the caller asks it first)
    const int waves = structure_waves(a.B);
    hipLaunchKernelGGL(window_structure_kernel, dim3((unsigned)(waves / 4)), dim3(256), lds, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(window_structure_reduce_kernel, dim3(1), dim3(64), 0, stream, a.partial, waves, a.record);
    return hipGetLastError();
}

hipError_t launch_window_arrow_pack(const ArrowPackArgs& a, hipStream_t stream) {
    if (a.B <= 0 || !a.counts || !a.hdr || !a.rec || !a.prec || a.jmax < 1 || a.jmax > 64 || a.jpmax < 1 || a.jpmax > 16 || a.nchunk != (a.caps.nv_max + 63) / 64) return hipErrorInvalidValue;
    if ((a.caps.nr_max > 0 && (!a.r_idx || !a.r_val)) || (a.caps.np_max > 0 && (!a.p_idx || !a.p_val))) return hipErrorInvalidValue;
    const size_t lds = (size_t)4 * 2 * a.nchunk * 64 * sizeof(int32_t);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const int waves = structure_waves(a.B);
    hipLaunchKernelGGL(arrow_pack_kernel, dim3((unsigned)(waves / 4)), dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace locamd
