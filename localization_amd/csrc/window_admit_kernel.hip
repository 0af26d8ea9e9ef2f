// gfx950 (MI355X / CDNA4): the admission and the chain-family structure scan of a batch that arrives in the caller's DEVICE arrays
// (loc_window_upload_dev; DESIGN.md §2, "Upload from device arrays"): what check_instances, chain_scan(ordered), translation_only and
// max_anchor_referenced (window_structure.cpp) do on CPU threads for loc_window_upload, before anything of the batch is copied or launched.
// window_admit.h states the rule for ONE window as two functions; this file restates both lane-parallel, in ONE pass over each index table.
//
// Mapping: one wave per window, the windows of the batch dealt round-robin to the waves of the launch (four waves per workgroup, at most
// kAdmitMaxWaves waves).  Rows over lanes in steps of 64; "any row" is a ballot; "the first failing row" is the lowest set bit of a ballot.
// A step first admits its rows (window_admit's checks, a refusal leaves at once) and then adds them to the structure scan
// (window_structure_flags' state), so the scan only ever sees admitted rows and a refused window's scan is simply dropped.  The tables are
// taken in check_instances' order — ranges, priors, EdgeSE3 rows — so the FIRST failing check is reported; the scan's accumulators are
// independent of each other, so their order is free.  The first 64 rows of all three tables are loaded together, before any of them is
// looked at: the counts are known to be in range by then, and that is all a load needs (the window is a chain of dependent round trips to
// memory, and most windows have no more rows than that).
// The ordered scans (key2 < last, key2 == last, last_pair) carry their state across the steps: inside a step a lane compares with its lower
// neighbour (last_pair: with the nearest lower lane that holds a pose-to-pose row — a ballot, a count of leading zeros and one lane read),
// lane 0 with what the previous step left.  The value columns translation_only reads (r_val[.][2..4], poses[.][0..8], p_val[.][0..8] and
// [15..17]) are walked element-wise over lanes, four independent loads per lane and step, contiguous but for the columns it skips, and only
// while a translation-only verdict is open; s_val is never read.
// No LDS, no scratch, no atomics, plain vector loads and stores.  Each wave writes admit[b] and flags[b] of its windows and ONE partial
// record (window_admit.h: WindowAdmitRecord); window_admit_reduce_kernel, one wave, merges the partial records.  AND, OR, minimum and maximum
// are associative and commutative, so the batch record is the same bits wherever a window sits and whatever the launch geometry.
//
// It reads nothing outside the caller's arrays and writes nothing outside admit / flags / partial / record:
//   * window b < B <= the handle's batch capacity; every array is [B][capacity] by the entry's contract, so window b's slices are
//     counts[4 b ..], r_idx[(b nr_max + e) 2 ..], p_idx[b np_max + e], s_idx[(b ns_max + e) 4 ..], poses[(b nv_max + p) 12 ..], r_val[(b nr_max
//     + e) 5 ..], p_val[(b np_max + e) 18 ..], all offsets in size_t.
//   * the four counts are read first and code 1 returns before any row is read: every load below is at a row e < count (or an element
//     i < count * width) with 0 <= count <= capacity, so it stays inside window b's slice.  A table under a capacity of 0 has count 0 and is
//     never dereferenced (it may be NULL).
//   * NO value read from a table ever becomes an index or an address: indices are compared (with counts, with each other, with their lower
//     neighbour) and nothing else; the only data-dependent lane read (last_pair) takes its source lane from a ballot, 0 .. 63.
//   * a step's rows enter the structure scan only after the step has admitted them; its differences v0 - v1 are then between pose slots
//     and anchor codes of the table and cannot overflow.  The admission itself compares widths in 64 bits.
//   * partial[wave] with wave < waves of the launch <= kAdmitMaxWaves, the size the entry allocates.
#include "window_admit.h"
#include "window_device.h"

namespace locamd {

namespace {

// the value of lane - 1 (lane 0: `carry`, what the previous step left)
__device__ __forceinline__ int from_lower(int v, int lane, int carry) {
    const int up = __shfl_up(v, 1);
    return lane == 0 ? carry : up;
}

// the bit pattern of the 3 x 3 identity's entry k (slide_admit.h: slide_identity_bits)
__device__ __forceinline__ bool identity_bits(double v, int k) { return (u64)__double_as_longlong(v) == (k % 4 == 0 ? 0x3FF0000000000000ull : 0ull); }

// window_admit and, for an admitted window, window_structure_flags for window b by its wave; every lane gets the same code and word
__device__ __forceinline__ int window_admit_wave(const WindowAdmitArgs& a, size_t b, int lane, int nv, int nr, int np, int ns, uint64_t& word_out) {
    const WindowCaps& cp = a.caps;
    word_out = 0;
    if (nv < 0 || nv > cp.nv_max || nr < 0 || nr > cp.nr_max || np < 0 || np > cp.np_max || ns < 0 || ns > cp.ns_max) return kWinAdmitCounts;
    const long long bw = cp.bw_max;
    const u64 below = (1ull << lane) - 1;
    // the first step of every table, in flight together
    int r0a = 0, r0b = -1, p0 = 0, s0a = 0, s0b = 1;
    if (lane < nr) { const int32_t* xi = a.r_idx + (b * cp.nr_max + lane) * 2; r0a = xi[0]; r0b = xi[1]; }
    if (lane < np) p0 = a.p_idx[b * cp.np_max + lane];
    if (lane < ns) { const int32_t* xi = a.s_idx + (b * cp.ns_max + lane) * 4; s0a = xi[0]; s0b = xi[1]; }

    bool broken = false, dup_r = false, dup_s = false;   // the chain scan: an order or adjacency rule fails; a second range / EdgeSE3 row on a pair
    int carry = 0, carry_pair = -1, max_anchor = 0;
    for (int e0 = 0; e0 < nr; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < nr;
        int v0 = r0a, v1 = r0b;
        if (e0 != 0) {
            v0 = 0; v1 = -1;
            if (in) { const int32_t* xi = a.r_idx + (b * cp.nr_max + e) * 2; v0 = xi[0]; v1 = xi[1]; }
        }
        const bool f2 = in && (v0 < 0 || v0 >= nv || v1 >= nv || v1 < -a.n_anchors || v0 == v1);
        const long long d = (long long)v0 - v1;
        const bool f3 = in && !f2 && v1 >= 0 && (d > bw || -d > bw);
        const u64 m2 = __ballot(f2), m3 = __ballot(f3);
        if ((m2 | m3) != 0) {   // the lowest failing row decides (a row's 2 comes before its 3: f3 excludes f2)
            const u64 low = (m2 | m3) & (0 - (m2 | m3));
            return (m2 & low) != 0 ? kWinAdmitRangeIndex : kWinAdmitRangeWidth;
        }
        const int key2 = v1 > v0 ? v1 : v0;
        const int last = from_lower(key2, lane, carry);
        const bool pair = in && v1 >= 0;
        const u64 pm = __ballot(pair);
        const u64 lower = pm & below;
        const int from_pair = __shfl(key2, lower != 0 ? 63 - __clzll((long long)lower) : 0);   // the nearest lower lane with a pose-to-pose row
        const int last_pair = lower != 0 ? from_pair : carry_pair;
        broken = broken || __ballot(in && key2 < last) != 0 || __ballot(pair && v0 - v1 != 1 && v1 - v0 != 1) != 0;
        dup_r = dup_r || __ballot(pair && key2 == last_pair) != 0;
        const int top = __shfl(key2, pm != 0 ? 63 - __clzll((long long)pm) : 0);
        if (pm != 0) carry_pair = top;
        carry = __shfl(key2, 63);   // (read only by a further step, and then lane 63 held a row)
        int am = in && v1 < 0 ? -v1 : 0;   // (admitted: v1 >= -n_anchors)
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) { const int o = __shfl_xor(am, s); am = o > am ? o : am; }
        max_anchor = am > max_anchor ? am : max_anchor;
    }
    carry = 0;
    for (int e0 = 0; e0 < np; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < np;
        int v = p0;
        if (e0 != 0) { v = 0; if (in) v = a.p_idx[b * cp.np_max + e]; }
        if (__ballot(in && (v < 0 || v >= nv)) != 0) return kWinAdmitPriorIndex;
        const int last = from_lower(v, lane, carry);
        broken = broken || __ballot(in && v < last) != 0;
        carry = __shfl(v, 63);
    }
    carry = 0;
    for (int e0 = 0; e0 < ns; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < ns;
        int vi = s0a, vj = s0b;
        if (e0 != 0) {
            vi = 0; vj = 1;
            if (in) { const int32_t* xi = a.s_idx + (b * cp.ns_max + e) * 4; vi = xi[0]; vj = xi[1]; }
        }
        const bool f5 = in && (vi < 0 || vi >= nv || vj < 0 || vj >= nv || vi == vj);
        const long long d = (long long)vi - vj;
        const bool f6 = in && !f5 && (d > bw || -d > bw);
        const u64 m5 = __ballot(f5), m6 = __ballot(f6);
        if ((m5 | m6) != 0) {
            const u64 low = (m5 | m6) & (0 - (m5 | m6));
            return (m5 & low) != 0 ? kWinAdmitSe3Index : kWinAdmitSe3Width;
        }
        const int key2 = vj > vi ? vj : vi;
        const int last = from_lower(key2, lane, carry);
        broken = broken || __ballot(in && (key2 < last || (vi - vj != 1 && vj - vi != 1))) != 0;
        dup_s = dup_s || __ballot(in && key2 == last) != 0;
        carry = __shfl(key2, 63);
    }
    uint32_t word = ns != 0 ? kWinAnyS : 0u;
    if (!broken) word |= kWinChain | (ns == 0 && !dup_r ? kWinSingleL : 0u) | (!dup_r ? kWinSingleR : 0u) | (!dup_s ? kWinSingleS : 0u);

    // translation_only: what both values of skip_prior_diagonal share, then the priors' rotation information (read while `shared` holds)
    bool shared = ns == 0 && nv <= 1048575 && a.n_anchors <= 500000, diagonal = true;
    if (shared) {
        const double* rv = a.r_val + b * cp.nr_max * 5;
        const double* X = a.poses + b * cp.nv_max * 12;
        const double* pv = a.p_val + b * cp.np_max * 18;
        bool bad = false, rot = false;
        for (int i0 = 0; i0 < nr * 5; i0 += 256) {   // a lever arm: by value
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = i0 + u * 64 + lane; v[u] = i < nr * 5 && i % 5 >= 2 ? rv[i] : 0.0; }
#pragma unroll
            for (int u = 0; u < 4; ++u) bad = bad || v[u] != 0.0;
        }
        for (int i0 = 0; i0 < nv * 12; i0 += 256) {   // a pose's rotation: the identity's bit pattern
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = i0 + u * 64 + lane; v[u] = i < nv * 12 && i % 12 < 9 ? X[i] : (i % 12 % 4 == 0 ? 1.0 : 0.0); }
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int k = (i0 + u * 64 + lane) % 12; bad = bad || (k < 9 && !identity_bits(v[u], k)); }
        }
        for (int i0 = 0; i0 < np * 18; i0 += 256) {   // a prior's measurement rotation by bits, its rotation information by value
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int i = i0 + u * 64 + lane, k = i % 18; v[u] = i < np * 18 && (k < 9 || k >= 15) ? pv[i] : (k < 9 && k % 4 == 0 ? 1.0 : 0.0); }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = (i0 + u * 64 + lane) % 18;
                bad = bad || (k < 9 && !identity_bits(v[u], k));
                rot = rot || (k >= 15 && v[u] != 0.0);
            }
        }
        shared = __ballot(bad) == 0;
        diagonal = __ballot(rot) == 0;
    }
    if (shared) word |= kWinTransOnlySkip | (diagonal ? kWinTransOnly : 0u);
    word_out = (uint64_t)word | ((uint64_t)(uint32_t)max_anchor << 32);
    return kWinAdmitOk;
}

__global__ void __launch_bounds__(256) window_admit_kernel(const WindowAdmitArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nwaves = (int)gridDim.x * 4;
    WindowAdmitRecord r = window_record_empty();
    for (long long b = wave; b < a.B; b += nwaves) {
        const int32_t* cn = a.counts + (size_t)b * 4;
        const int nv = cn[0], nr = cn[1], np = cn[2], ns = cn[3];
        uint64_t word;
        const int code = window_admit_wave(a, (size_t)b, lane, nv, nr, np, ns, word);   // (the same code and word in every lane; a refused window's word is 0)
        if (lane == 0) {
            if (a.admit) a.admit[b] = code;
            a.flags[b] = word;
        }
        window_record_add(r, b, code, word);
    }
    if (lane == 0) a.partial[wave] = r;
}

// one wave: the partial records of the first launch, lanes over records, then a butterfly over the lanes
__global__ void __launch_bounds__(64) window_admit_reduce_kernel(const WindowAdmitRecord* partial, int n_partial, WindowAdmitRecord* record) {
    const int lane = threadIdx.x;
    WindowAdmitRecord r = window_record_empty();
#pragma unroll 4
    for (int j = lane; j < n_partial; j += 64) window_record_merge(r, partial[j]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        WindowAdmitRecord o = r;
        o.first_bad = __shfl_xor(r.first_bad, s); o.code = __shfl_xor(r.code, s);
        o.and_bits = (uint32_t)__shfl_xor((int)r.and_bits, s); o.or_bits = (uint32_t)__shfl_xor((int)r.or_bits, s); o.max_anchor = __shfl_xor(r.max_anchor, s);
        window_record_merge(r, o);
    }
    if (lane == 0) *record = r;
}

}  // namespace

int window_admit_waves(long long B) {
    const long long blocks = (B + 3) / 4;
    return (int)(blocks < kAdmitMaxWaves / 4 ? blocks : kAdmitMaxWaves / 4) * 4;
}

hipError_t launch_window_admit(const WindowAdmitArgs& a, hipStream_t stream) {
    if (a.B <= 0 || !a.counts || !a.poses || !a.flags || !a.partial || !a.record) return hipErrorInvalidValue;
    if ((a.caps.nr_max > 0 && (!a.r_idx || !a.r_val)) || (a.caps.np_max > 0 && (!a.p_idx || !a.p_val)) || (a.caps.ns_max > 0 && !a.s_idx)) return hipErrorInvalidValue;
    const int waves = window_admit_waves(a.B);
    hipLaunchKernelGGL(window_admit_kernel, dim3((unsigned)(waves / 4)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(window_admit_reduce_kernel, dim3(1), dim3(64), 0, stream, a.partial, waves, a.record);
    return hipGetLastError();
}

}  // namespace locamd
