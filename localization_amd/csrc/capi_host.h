// Host-side plumbing shared by the C ABI files (capi*.cpp, frontend.cpp): error reporting, grow-on-demand device buffers and staging pairs, the
// per-launch HIP-event timer and the chunked three-stream pipeline of the snapshot and fusion solvers' host paths.  Never included by device code.
#pragma once
#include "../../include/localization_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

// set loc_last_error() and return the code (defined in capi.cpp)
int locamd_fail(int code, const char* what);
int locamd_fail_hip(hipError_t e, const char* where);
#define LOC_HIP(expr)                                              \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return locamd_fail_hip(_e, #expr);   \
    } while (0)

namespace locamd {

// ---- grow-on-demand device buffers ------------------------------------------------------------------------------------
// One buffer of a group that shares a capacity: the handle's pointer and the bytes it needs at the new capacity.
struct Want {
    void** p;
    size_t bytes;
    template <class T> Want(T*& ptr, size_t n) : p((void**)&ptr), bytes(n) {}
};
// No-op while need <= cap (in the caller's unit: epochs, bytes, doubles).  Otherwise every buffer is freed and nulled and the capacity
// zeroed, then they are allocated in order and the capacity recorded: a failed allocation leaves its pointer null and the capacity 0.
inline hipError_t grow_buffers(size_t& cap, size_t need, std::initializer_list<Want> bufs) {
    if (need <= cap) return hipSuccess;
    for (const Want& b : bufs) {
        if (*b.p) (void)hipFree(*b.p);
        *b.p = nullptr;
    }
    cap = 0;
    for (const Want& b : bufs)
        if (hipError_t e = hipMalloc(b.p, b.bytes); e != hipSuccess) return e;
    cap = need;
    return hipSuccess;
}

// ---- a page-locked block and its device twin, grown on demand ------------------------------------------------------------------------------
// How a call's small host arrays reach a kernel on the caller's stream: into the page-locked half before the call returns, from there to
// the device half in stream order.
struct StagingPair {
    char *h = nullptr, *d = nullptr;
    size_t cap = 0;
    hipEvent_t copied = nullptr;   // the device half has the page-locked half's content
    bool inflight = false;

    // Both halves for `bytes`; no-op while they fit.  The caller has waited for whatever may still read the device half.
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (h) (void)hipHostFree(h);
        h = nullptr; cap = 0; inflight = false;   // (capacity 0: grow_buffers replaces the device half with the host half, and a failure leaves none)
        if (hipError_t e = hipHostMalloc((void**)&h, bytes, hipHostMallocDefault); e != hipSuccess) return e;
        return grow_buffers(cap, bytes, {{d, bytes}});
    }
    // the page-locked half, once the previous send() has left it
    hipError_t host(char*& out) {
        hipError_t e = copied ? hipSuccess : hipEventCreateWithFlags(&copied, hipEventDisableTiming);
        if (e == hipSuccess && inflight && (e = hipEventSynchronize(copied)) == hipSuccess) inflight = false;
        out = h;
        return e;
    }
    // the first `bytes` of it to the device half, on st
    hipError_t send(size_t bytes, hipStream_t st) {
        hipError_t e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && (e = hipEventRecord(copied, st)) == hipSuccess) inflight = true;
        return e;
    }
    void destroy() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        if (copied) (void)hipEventDestroy(copied);
    }
};

// ---- HIP-event timing of launches (loc_*_timing_begin / _end) -----------------------------------------------------------
struct LaunchTimer {
    std::vector<hipEvent_t> ev;   // one pair per launch
    int used = 0;
    bool on = false, open = false;   // open: start() recorded, stop() completes the pair

    int begin(int device, int32_t max_launches) {
        if (max_launches <= 0) return locamd_fail(LOC_ERR_INVALID, "timing_begin");
        LOC_HIP(hipSetDevice(device));
        while ((int)ev.size() < 2 * max_launches) {
            hipEvent_t e;
            LOC_HIP(hipEventCreate(&e));
            ev.push_back(e);
        }
        used = 0;
        on = true;
        return LOC_OK;
    }
    int end(int device, int32_t* n_launches, double* total_ms, double* avg_ms) {
        LOC_HIP(hipSetDevice(device));
        on = false;
        double tot = 0;
        const int n = used / 2;
        for (int i = 0; i < n; ++i) {
            LOC_HIP(hipEventSynchronize(ev[2 * i + 1]));
            float ms = 0;
            LOC_HIP(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            tot += ms;
        }
        if (n_launches) *n_launches = n;
        if (total_ms) *total_ms = tot;
        if (avg_ms) *avg_ms = n ? tot / n : 0.0;
        used = 0;
        return LOC_OK;
    }
    // around one launch on st; a launch is recorded only while a free pair remains
    hipError_t start(hipStream_t st) {
        open = on && (size_t)(used + 2) <= ev.size();
        return open ? hipEventRecord(ev[used], st) : hipSuccess;
    }
    hipError_t stop(hipStream_t st) {
        if (!open) return hipSuccess;
        open = false;
        const hipError_t e = hipEventRecord(ev[used + 1], st);
        if (e == hipSuccess) used += 2;
        return e;
    }
    void destroy() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
    }
};

// ---- the pipelined host path (loc_snapshot_solve_host_kmb, loc_fusion_solve_host_kmb and their _cov forms) -----------------
// One array that travels with the epochs: bytes per epoch on both sides.  host == nullptr: skipped.
struct PipeIn { const void* host; void* dev; size_t bytes; };
struct PipeOut { void* host; const void* dev; size_t bytes; bool pin_test = true; };   // pin_test false: copied out, but not looked at by the pinned test

struct HostPipeline {
    float *d_raw_dist = nullptr, *d_raw_err = nullptr;   // the ranges as the caller holds them, [K][M][B]; the solve stream packs them into tiles
    size_t raw_epochs = 0;
    double* d_cov = nullptr;                             // covariance outputs, allocated by the first call that asks for them
    int32_t *d_cov_mask = nullptr, *d_cov_status = nullptr;
    size_t cov_epochs = 0;
    hipStream_t in_stream = nullptr, out_stream = nullptr;
    std::vector<hipEvent_t> ev;                          // two per chunk: copied in, solved

    // device buffers for `epochs` epochs of B tags with M ranges each, and cov_terms covariance entries per tag (0: no covariances); the copy streams
    int prepare(size_t epochs, size_t B, size_t M, size_t cov_terms) {
        const size_t raw = sizeof(float) * M * B * epochs, flags = sizeof(int32_t) * B * epochs;
        LOC_HIP(grow_buffers(raw_epochs, epochs, {{d_raw_dist, raw}, {d_raw_err, raw}}));
        if (cov_terms) LOC_HIP(grow_buffers(cov_epochs, epochs, {{d_cov, sizeof(double) * cov_terms * B * epochs}, {d_cov_mask, flags}, {d_cov_status, flags}}));
        if (!in_stream) LOC_HIP(hipStreamCreateWithFlags(&in_stream, hipStreamNonBlocking));
        if (!out_stream) LOC_HIP(hipStreamCreateWithFlags(&out_stream, hipStreamNonBlocking));
        return LOC_OK;
    }

    // Chunks of ~8 MB of input `sizing`: small enough that copy-in, solve and copy-out of neighbouring chunks overlap, large enough that a
    // chunk's launch fills the GPU (the epochs of one chunk stay sequential per tag inside the kernel).  Pageable buffers cannot overlap
    // anyway — the runtime stages them synchronously — so they go as one chunk.
    // chunk(k0, kc) packs and launches epochs [k0, k0 + kc) on `solve` and returns a LOC_* code.  Blocks until the outputs are on the host.
    template <class Chunk>
    int run(hipStream_t solve, int epochs, int sizing, std::initializer_list<PipeIn> ins, std::initializer_list<PipeOut> outs, Chunk&& chunk) {
        auto pinned = [](const void* p) {
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
            return at.type == hipMemoryTypeHost;
        };
        bool overlap = true;
        for (const PipeIn& i : ins) overlap = overlap && (!i.host || pinned(i.host));
        for (const PipeOut& o : outs) overlap = overlap && (!o.host || !o.pin_test || pinned(o.host));
        const int ce = overlap ? (int)std::max<size_t>(1, (8u << 20) / ins.begin()[sizing].bytes) : epochs;
        const int nchunks = (epochs + ce - 1) / ce;
        while ((int)ev.size() < 2 * nchunks) {
            hipEvent_t e;
            LOC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ev.push_back(e);
        }
        auto issue = [&]() -> int {
            for (int c = 0; c < nchunks; ++c) {
                const int k0 = c * ce, kc = std::min(ce, epochs - k0);
                for (const PipeIn& i : ins)
                    if (i.host) LOC_HIP(hipMemcpyAsync((char*)i.dev + k0 * i.bytes, (const char*)i.host + k0 * i.bytes, kc * i.bytes, hipMemcpyHostToDevice, in_stream));
                LOC_HIP(hipEventRecord(ev[2 * c], in_stream));
                LOC_HIP(hipStreamWaitEvent(solve, ev[2 * c], 0));
                if (int rc = chunk(k0, kc)) return rc;
                LOC_HIP(hipEventRecord(ev[2 * c + 1], solve));
                LOC_HIP(hipStreamWaitEvent(out_stream, ev[2 * c + 1], 0));
                for (const PipeOut& o : outs)
                    if (o.host) LOC_HIP(hipMemcpyAsync((char*)o.host + k0 * o.bytes, (const char*)o.dev + k0 * o.bytes, kc * o.bytes, hipMemcpyDeviceToHost, out_stream));
            }
            LOC_HIP(hipStreamSynchronize(out_stream));
            LOC_HIP(hipStreamSynchronize(solve));
            return LOC_OK;
        };
        const int rc = issue();
        if (rc != LOC_OK) {   // no copy may still be reading or writing the caller's buffers when the error is returned
            (void)hipStreamSynchronize(in_stream);
            (void)hipStreamSynchronize(solve);
            (void)hipStreamSynchronize(out_stream);
        }
        return rc;
    }

    void destroy() {
        void* bufs[] = {d_raw_dist, d_raw_err, d_cov, d_cov_mask, d_cov_status};
        for (void* p : bufs) if (p) (void)hipFree(p);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (in_stream) (void)hipStreamDestroy(in_stream);
        if (out_stream) (void)hipStreamDestroy(out_stream);
    }
};

}  // namespace locamd
