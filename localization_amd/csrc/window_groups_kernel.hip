// gfx950 (MI355X / CDNA4): the grouping of a batch of forest windows of DIFFERING topologies that arrived in the caller's DEVICE arrays
// (loc_window_upload_dev under option "upload_dev_forest_groups"; DESIGN.md §2, "Upload from device arrays"): what passes 1 and 2 of
// build_tree_groups (window_structure.cpp: group_windows) do on the host for loc_window_upload.  window_groups.h states the topology key and
// the candidate hash; this file reads the same words lane-parallel.  Integer-only and latency-bound, as the admit and structure passes are.
//
// Mapping: one wave per window, the windows dealt round-robin to the waves of the launch (four waves per workgroup, at most kGroupsMaxWaves),
// as the admit and structure passes deal them.  Key words over lanes in steps of 64; "any word differs" is a ballot.
// window_groups_hash_kernel: the wave's 64 partial hashes are added with a butterfly (addition modulo 2^64: any order gives the same bits),
//   finished and masked (window_groups.h); lane 0 claims the hash's slot of the open-addressed table with a 64-bit compare-and-swap and takes
//   the maximum of ~b there — the slot ends with the LOWEST window index of that hash whatever the order of the inserts, so rep0 does not
//   depend on the launch geometry.  A window with nv outside [2, 64] or a count outside its capacity is not hashed: hash[b] = 0.
// window_groups_verify_kernel: finds the hash's slot again, rep0[b] = its lowest window, and compares b's key with rep0[b]'s word for word —
//   counts first, then the rows below the equal counts.  One partial record per wave (window_groups.h: WindowGroupsRecord: OR of the bits, the
//   number of windows with rep0[b] == b); window_groups_reduce_kernel, one wave, merges them.  OR and sum are associative and commutative.
// window_groups_number_kernel: ONE workgroup scans rep0[b] == b over the windows in tiles of 256: a representative's group id is the number
//   of representatives below it (first appearance); sched_of[b] = id[rep0[b]], rep[id] = b.
// window_groups_gather_kernel: one wave per group copies its representative's four counts and used r_idx / p_idx / s_idx rows into the
//   compact tables.
//
// Every loop's trip count is bounded by a value checked here: a probe by the table's size (a probe that runs out sets kGroupsOverflow and
// does not spin), a row loop by a count that was held to its capacity first.
//
// It reads the batch's counts and index tables and its own block, and writes nothing outside that block (hash, the table, rep0, sched_of, rep,
// partial, record) and the compact tables:
//   * the batch has passed window_admit_kernel.hip and the tables are the handle's own copies: 0 <= count <= capacity.  The counts are held
//     to the capacities here AGAIN before any row is addressed (hash, verify, gather); window b's slices as in window_admit_kernel.hip, offsets
//     in size_t; no row at or beyond a count is read.
//   * table indices are masked to the table's size (`slots`, a power of two: launch_window_groups checks it), in the insert and in the lookup.
//   * rep0[b] comes out of the table as ~tab_inv[slot]: it is used as a window index only after it was found <= b (< B); a slot that holds
//     anything else is an overflow and rep0[b] = b.  The number pass checks rep0[b] < B again before it addresses sched_of with it, the gather
//     pass rep[g] < B before it addresses a row.
//   * hash[b], rep0[b], sched_of[b]: b < B.  rep[id]: id counts representatives, at most B of them.  partial[wave] with wave < waves of the
//     launch <= kGroupsMaxWaves, the size the entry allocates.  Compact tables: group g < G, rows below the clamped counts.
#include "window_groups.h"
#include "window_device.h"

namespace locamd {

namespace {

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (u64)__shfl_xor((unsigned long long)v, s);
    return v;
}

__device__ __forceinline__ bool counts_in_range(const WindowCaps& cp, int nv, int nr, int np, int ns) {
    return nv >= 2 && nv <= 64 && nv <= cp.nv_max && nr >= 0 && nr <= cp.nr_max && np >= 0 && np <= cp.np_max && ns >= 0 && ns <= cp.ns_max;
}

__global__ void __launch_bounds__(256) window_groups_hash_kernel(const WindowGroupsArgs a) {
    const WindowCaps& cp = a.caps;
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int nwaves = (int)gridDim.x * 4;
    const u64 mask = a.slots - 1;
    for (long long bb = wave; bb < a.B; bb += nwaves) {
        const size_t b = (size_t)bb;
        const int32_t* cn = a.counts + b * 4;
        const int nv = cn[0], nr = cn[1], np = cn[2], ns = cn[3];
        u64 key = 0;
        if (counts_in_range(cp, nv, nr, np, ns)) {
            const int32_t c4[4] = {nv, nr, np, ns};
            const long long nw = topology_key_words(c4);
            const u64 part = topology_key_lane_hash(c4, a.r_idx + b * cp.nr_max * 2, a.p_idx + b * cp.np_max, a.s_idx + b * cp.ns_max * 4, nw, lane);
            key = groups_hash_masked(topology_key_hash_finish(wave_sum_u64(part), nw), a.hash_bits);
            if (lane == 0) {
                u64 slot = groups_hash_slot(key, a.slots);
                for (u64 i = 0; i < a.slots; ++i) {   // (a probe that runs out leaves the hash out of the table: the verify pass reports it)
                    const u64 old = atomicCAS((unsigned long long*)&a.tab_key[slot], 0ull, (unsigned long long)key);
                    if (old == 0 || old == key) { atomicMax(&a.tab_inv[slot], ~(uint32_t)b); break; }
                    slot = (slot + 1) & mask;
                }
            }
        }
        if (lane == 0) a.hash[b] = key;
    }
}

__global__ void __launch_bounds__(256) window_groups_verify_kernel(const WindowGroupsArgs a) {
    const WindowCaps& cp = a.caps;
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int nwaves = (int)gridDim.x * 4;
    const u64 mask = a.slots - 1;
    WindowGroupsRecord rec{0u, 0};
    for (long long bb = wave; bb < a.B; bb += nwaves) {
        const size_t b = (size_t)bb;
        const u64 key = a.hash[b];
        const int32_t* cn = a.counts + b * 4;
        const int nv = cn[0], nr = cn[1], np = cn[2], ns = cn[3];
        size_t r = b;
        if (key == 0 || !counts_in_range(cp, nv, nr, np, ns)) rec.or_bits |= kGroupsBadNv;
        else {
            // the hash's slot (the same in every lane of the wave)
            u64 slot = groups_hash_slot(key, a.slots);
            bool found = false;
            for (u64 i = 0; i < a.slots; ++i) {
                const u64 k = a.tab_key[slot];
                if (k == key) { found = true; break; }
                if (k == 0) break;
                slot = (slot + 1) & mask;
            }
            if (found) {
                const uint32_t low = ~a.tab_inv[slot];
                if ((u64)low <= (u64)b) r = (size_t)low;   // (the lowest window of the hash: never above b, which carries it)
                else found = false;
            }
            if (!found) rec.or_bits |= kGroupsOverflow;
            else if (r != b) {
                const int32_t* cr = a.counts + r * 4;
                const int32_t c4[4] = {nv, nr, np, ns};
                bool diff = cr[0] != nv || cr[1] != nr || cr[2] != np || cr[3] != ns;
                if (!diff) {   // (the counts are equal: r's rows below b's counts are r's used rows)
                    const int32_t *rb = a.r_idx + b * cp.nr_max * 2, *pb = a.p_idx + b * cp.np_max, *sb = a.s_idx + b * cp.ns_max * 4;
                    const int32_t *rr = a.r_idx + r * cp.nr_max * 2, *pr = a.p_idx + r * cp.np_max, *sr = a.s_idx + r * cp.ns_max * 4;
                    const long long nw = topology_key_words(c4);
                    for (long long k = 4 + lane; k < nw; k += 64) diff = diff || topology_key_word(c4, rb, pb, sb, k) != topology_key_word(c4, rr, pr, sr, k);
                }
                if (__ballot(diff) != 0) rec.or_bits |= kGroupsCollision;
            }
        }
        if (lane == 0) a.rep0[b] = (int32_t)r;
        if (r == b) rec.n_groups += 1;
    }
    if (lane == 0) a.partial[wave] = rec;
}

// one wave: the partial records of the verify launch, lanes over records, then a butterfly over the lanes
__global__ void __launch_bounds__(64) window_groups_reduce_kernel(const WindowGroupsRecord* partial, int n_partial, WindowGroupsRecord* record) {
    const int lane = threadIdx.x;
    WindowGroupsRecord r{0u, 0};
    for (int j = lane; j < n_partial; j += 64) groups_record_merge(r, partial[j]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        WindowGroupsRecord o;
        o.or_bits = (uint32_t)__shfl_xor((int)r.or_bits, s);
        o.n_groups = __shfl_xor(r.n_groups, s);
        groups_record_merge(r, o);
    }
    if (lane == 0) *record = r;
}

// ONE workgroup of four waves: group ids by first appearance
__global__ void __launch_bounds__(256) window_groups_number_kernel(const WindowGroupsArgs a) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const u64 below = (1ull << lane) - 1;
    int base = 0;
    for (long long t0 = 0; t0 < a.B; t0 += 256) {
        const long long b = t0 + tid;
        const bool flag = b < a.B && a.rep0[b] == (int32_t)b;
        const u64 m = __ballot(flag);
        if (lane == 0) wsum[wib] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int s = wsum[k]; off += k < wib ? s : 0; tot += s; }
        if (flag) {
            const int id = base + off + __popcll(m & below);   // (< the number of windows up to b: inside rep)
            a.sched_of[b] = id;
            a.rep[id] = (int32_t)b;
        }
        base += tot;
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    for (long long b = tid; b < a.B; b += 256) {
        const int32_t r = a.rep0[b];
        if (r == (int32_t)b) continue;
        // (a representative's own slot was written above; anything else — only on a batch the host groups itself — reads no slot)
        a.sched_of[b] = r >= 0 && r < a.B && a.rep0[r] == r ? a.sched_of[r] : 0;
    }
}

__global__ void __launch_bounds__(256) window_groups_gather_kernel(const WindowGroupsGatherArgs a) {
    const WindowCaps& cp = a.caps;
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int nwaves = (int)gridDim.x * 4;
    for (long long gg = wave; gg < a.G; gg += nwaves) {
        const size_t g = (size_t)gg;
        const int32_t rb = a.rep[g];
        const bool ok = rb >= 0 && rb < a.B;
        const size_t b = ok ? (size_t)rb : 0;
        const int32_t* cn = a.counts + b * 4;
        int nv = cn[0], nr = cn[1], np = cn[2], ns = cn[3];
        if (!ok || !counts_in_range(cp, nv, nr, np, ns)) { nv = 0; nr = 0; np = 0; ns = 0; }   // (a window no schedule is built for: the host refuses nv = 0)
        if (lane < 4) a.c_counts[g * 4 + lane] = lane == 0 ? nv : lane == 1 ? nr : lane == 2 ? np : ns;
        const int32_t* ri = a.r_idx + b * cp.nr_max * 2;
        int32_t* ro = a.c_r_idx + g * cp.nr_max * 2;
        for (int i = lane; i < 2 * nr; i += 64) ro[i] = ri[i];
        const int32_t* pi = a.p_idx + b * cp.np_max;
        int32_t* po = a.c_p_idx + g * cp.np_max;
        for (int i = lane; i < np; i += 64) po[i] = pi[i];
        const int32_t* si = a.s_idx + b * cp.ns_max * 4;
        int32_t* so = a.c_s_idx + g * cp.ns_max * 4;
        for (int i = lane; i < 4 * ns; i += 64) so[i] = si[i];
    }
}

int groups_waves(long long B) {
    const long long blocks = (B + 3) / 4;
    return (int)(blocks < kGroupsMaxWaves / 4 ? blocks : kGroupsMaxWaves / 4) * 4;
}

}  // namespace

hipError_t launch_window_groups(const WindowGroupsArgs& a, hipStream_t stream) {
    if (a.B <= 0 || a.B > 0x7ffffffell || !a.counts || !a.hash || !a.tab_key || !a.tab_inv || !a.rep0 || !a.sched_of || !a.rep || !a.partial || !a.record) return hipErrorInvalidValue;
    if ((a.caps.nr_max > 0 && !a.r_idx) || (a.caps.np_max > 0 && !a.p_idx) || (a.caps.ns_max > 0 && !a.s_idx)) return hipErrorInvalidValue;
    if (a.slots < 2 * (uint64_t)a.B || (a.slots & (a.slots - 1)) != 0 || a.hash_bits < 0 || a.hash_bits > 64) return hipErrorInvalidValue;
    if ((const char*)a.tab_inv != (const char*)(a.tab_key + a.slots)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.tab_key, 0, a.slots * (sizeof(uint64_t) + sizeof(uint32_t)), stream);
    if (e != hipSuccess) return e;
    const int waves = groups_waves(a.B);
    hipLaunchKernelGGL(window_groups_hash_kernel, dim3((unsigned)(waves / 4)), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(window_groups_verify_kernel, dim3((unsigned)(waves / 4)), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(window_groups_reduce_kernel, dim3(1), dim3(64), 0, stream, a.partial, waves, a.record);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(window_groups_number_kernel, dim3(1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_window_groups_gather(const WindowGroupsGatherArgs& a, hipStream_t stream) {
    if (a.G <= 0 || a.G > a.B || !a.counts || !a.rep || !a.c_counts) return hipErrorInvalidValue;
    if ((a.caps.nr_max > 0 && (!a.r_idx || !a.c_r_idx)) || (a.caps.np_max > 0 && (!a.p_idx || !a.c_p_idx)) || (a.caps.ns_max > 0 && (!a.s_idx || !a.c_s_idx))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_groups_gather_kernel, dim3((unsigned)(groups_waves(a.G) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace locamd
