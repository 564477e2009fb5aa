// handle_host.h -- the host skeleton every module's handle shares: device and stream, the events that time a call, the tail of a
// create, the frame of a destroy, and the zeroing of a handle's buffers.  Host code only; include after common.h.
//
//   create:   argument checks, new, host-side set-up, then  handle_open -> timer.create -> the module's allocations and
//             handle_zero / handle_fill -> handle_created  (the one wait for the handle's stream; on failure the handle goes)
//   destroy:  handle_close: set the device, wait for the own stream (and the last foreign one), free_own(), destroy the stream
//
// Zero on the OWN stream, one wait in the tail.  hipMemset returns before the device has written, on the null stream, and the
// null stream does not order a hipStreamNonBlocking stream: whatever the caller does next on the handle's stream (a load_state
// directly after create, the first call after a reset) could be zeroed again behind its back.  So a create zeroes with
// handle_zero and handle_created waits once; a reset / load / set entry point that zeroes waits for its stream before it returns.
#pragma once

#include "common.h"

namespace rtmodt {

struct HandleBase {
    int device = 0;
    hipStream_t stream = nullptr;
};

inline int handle_open(HandleBase *b) {
    RT_HIP(hipSetDevice(b->device));
    RT_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    return RTMODT_OK;
}

// free_own: releases what the module holds, once nothing is in flight any more.  `last`: the foreign stream (a tracker's) the
// handle's last call ran on, if it keeps one.  Every member may still be null (a create that failed half way).
template <typename F> void handle_close(HandleBase *b, F free_own, hipStream_t last = nullptr) {
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    if (last && last != b->stream) hipStreamSynchronize(last);
    free_own();
    if (b->stream) hipStreamDestroy(b->stream);
    b->stream = nullptr;
}

// N events around the launches of a call; `timed` says that the last call recorded them
template <int N> struct EventTimer {
    hipEvent_t ev[N] = {};
    bool timed = false;
    int create() {
        for (hipEvent_t &e : ev)
            if (!e) RT_HIP(hipEventCreate(&e));
        return RTMODT_OK;
    }
    void destroy() {
        for (hipEvent_t &e : ev) {
            if (e) hipEventDestroy(e);
            e = nullptr;
        }
    }
    int record(int i, hipStream_t q) {
        RT_HIP(hipEventRecord(ev[i], q));
        return RTMODT_OK;
    }
    // milliseconds from event i to event j of the last call, after waiting for j (a call fed from a detector does not end with a
    // wait of its own); `not_yet`: the module's words for "nothing was recorded"
    int elapsed(int device, int i, int j, float *ms, const char *not_yet) const {
        RT_CHECK(timed, RTMODT_E_INVALID, "%s", not_yet);
        RT_HIP(hipSetDevice(device));
        RT_HIP(hipEventSynchronize(ev[j]));
        RT_HIP(hipEventElapsedTime(ms, ev[i], ev[j]));
        return RTMODT_OK;
    }
};

// a buffer of the handle filled on the handle's own stream q (see the rule above)
inline hipError_t handle_fill(void *d, int byte, size_t bytes, hipStream_t q) { return hipMemsetAsync(d, byte, bytes, q); }
inline hipError_t handle_zero(void *d, size_t bytes, hipStream_t q) { return handle_fill(d, 0, bytes, q); }

inline int handle_wait(hipStream_t q) {
    RT_HIP(hipStreamSynchronize(q));
    return RTMODT_OK;
}

// the tail of a create: waits once for what the create queued on the handle's stream; on failure the handle goes, the error text
// stays and *out is not written
template <typename T> int handle_created(int rc, T *p, void (*destroy)(T *), T **out) {
    if (rc == RTMODT_OK && p->stream) rc = handle_wait(p->stream);
    if (rc != RTMODT_OK) {
        std::string keep = last_error();
        destroy(p);
        last_error() = keep;
        return rc;
    }
    *out = p;
    return RTMODT_OK;
}

}  // namespace rtmodt
