// track_host.h -- what the four tracker handles (tracker_api.hip: ByteTrack, deepsort.hip, ocsort.hip, botsort.hip) share on top of
// handle_host.h: the event that orders them behind a detector, the meta rows, the detection staging, and the calls every one of
// them makes around its own launches.  A tracker create ends in handle_created like every other.
#pragma once

#include "handle_host.h"
#include "kernels.h"
#include "track_layout.h"

namespace rtmodt {

struct TrackHandleBase : HandleBase {
    // An update fed from a detector runs on THAT detector's post-processing stream (ordered behind its NMS, no host hop).
    // The tracker never keeps the foreign stream handle: it records `foreign_done` there, and everything it later does on
    // its own stream (host-fed updates, state read-back, reset, destroy) waits for that event first.
    hipEvent_t foreign_done = nullptr;
    bool foreign_pending = false;
    int S = 1, Mc = 0, Nc = 0;
    int64_t *d_meta = nullptr, *h_meta = nullptr;          // [S][8]; h_* are pinned
    float4 *d_box = nullptr; float *d_conf = nullptr; int32_t *d_cls = nullptr, *d_n = nullptr, *h_n = nullptr;   // staging [S][Nc], counts [S]
};

static const int64_t track_init_meta[8] = {0, 0, 0, 0, 1, 0, 0, 0};   // cur, n_tracks, err, n_active / n_returned, next_id (tracker.py:55)

inline int track_open(TrackHandleBase *t) {
    RT_TRY(handle_open(t));
    RT_HIP(hipEventCreateWithFlags(&t->foreign_done, hipEventDisableTiming));
    RT_HIP(hipMalloc((void **)&t->d_meta, sizeof(int64_t) * 8 * t->S));
    RT_HIP(hipHostMalloc((void **)&t->h_meta, sizeof(int64_t) * 8 * t->S, hipHostMallocDefault));
    RT_HIP(hipHostMalloc((void **)&t->h_n, sizeof(int32_t) * t->S, hipHostMallocDefault));
    for (int s = 0; s < t->S; ++s) memcpy(t->h_meta + 8 * s, track_init_meta, sizeof(track_init_meta));
    RT_HIP(hipMemcpy(t->d_meta, t->h_meta, sizeof(int64_t) * 8 * t->S, hipMemcpyHostToDevice));
    const size_t SN = (size_t)t->S * t->Nc;
    RT_HIP(hipMalloc((void **)&t->d_box, SN * 16)); RT_HIP(hipMalloc((void **)&t->d_conf, SN * 4)); RT_HIP(hipMalloc((void **)&t->d_cls, SN * 4));
    RT_HIP(hipMalloc((void **)&t->d_n, (size_t)t->S * 4)); RT_HIP(handle_zero(t->d_n, (size_t)t->S * 4, t->stream));
    return RTMODT_OK;
}

// free_own: releases what the tracker holds beyond this struct, once nothing is in flight any more
template <typename F> void track_close(TrackHandleBase *t, F free_own) {
    hipSetDevice(t->device);
    if (t->foreign_done) hipEventSynchronize(t->foreign_done);      // an update may still be queued on a detector's stream
    handle_close(t, [&] {
        if (t->foreign_done) hipEventDestroy(t->foreign_done);
        free_own();
        hipFree(t->d_meta); hipFree(t->d_box); hipFree(t->d_conf); hipFree(t->d_cls); hipFree(t->d_n);
        hipHostFree(t->h_meta); hipHostFree(t->h_n);
    });
}

// make the tracker's own stream wait for the last update that ran on a detector's stream
inline int track_join(TrackHandleBase *t) {
    if (t->foreign_pending) {
        RT_HIP(hipStreamWaitEvent(t->stream, t->foreign_done, 0));
        t->foreign_pending = false;
    }
    return RTMODT_OK;
}

// the common part of a device view; the caller's work on t->stream is ordered behind every update
inline int track_view(TrackHandleBase *t, TrackViewBase *out) {
    *out = TrackViewBase{t->d_meta, t->S, t->Mc, t->device, t->stream};
    return track_join(t);
}

// the sticky error of a stream's meta row; `what` names the solver: "lapjv assignment" (ByteTrack) or "assignment"
inline int track_check_sticky(const TrackHandleBase *t, int s, int64_t err, const char *what) {
    RT_CHECK(err != 1, RTMODT_E_CAPACITY, "stream %d: more than max_tracks=%d live tracks", s, t->Mc);
    RT_CHECK(err != 2, RTMODT_E_CAPACITY, "stream %d: %s too dense (more than 256 contested rows/columns or 2048 contested pairs)", s, what);
    RT_CHECK(err == 0, RTMODT_E_INVALID, "stream %d: tracker error %lld", s, (long long)err);
    return RTMODT_OK;
}

// stream's meta row (every row when stream < 0) back to its initial value, after everything on the device has finished
inline int track_reset_meta(TrackHandleBase *t, int stream) {
    RT_CHECK(t && stream < t->S, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(t->device));
    RT_HIP(hipDeviceSynchronize());
    t->foreign_pending = false;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? t->S : stream + 1;
    for (int s = s0; s < s1; ++s) RT_HIP(hipMemcpy(t->d_meta + 8 * s, track_init_meta, sizeof(track_init_meta), hipMemcpyHostToDevice));
    return RTMODT_OK;
}

// update_batch: the counts and pointers of a host-fed batch ...
inline int track_batch_check(const TrackHandleBase *t, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n, bool *any_out) {
    RT_CHECK(t && n, RTMODT_E_INVALID, "null argument");
    bool any = false;
    for (int s = 0; s < t->S; ++s) {
        RT_CHECK(n[s] >= 0, RTMODT_E_INVALID, "stream %d: %d detections", s, n[s]);
        RT_CHECK(n[s] <= t->Nc, RTMODT_E_CAPACITY, "stream %d: %d detections > max_dets %d", s, n[s], t->Nc);
        any |= n[s] > 0;
    }
    RT_CHECK(!any || (xyxy && conf && cls), RTMODT_E_INVALID, "null detections");
    *any_out = any;
    return RTMODT_OK;
}
// ... and its copies into the staging buffers on the tracker's stream (the arrays only when a stream has a detection)
inline int track_batch_stage(TrackHandleBase *t, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n, bool any) {
    const size_t SN = (size_t)t->S * t->Nc;
    for (int s = 0; s < t->S; ++s) t->h_n[s] = n[s];
    if (any) {
        RT_HIP(hipMemcpyAsync(t->d_box, xyxy, SN * 16, hipMemcpyHostToDevice, t->stream));
        RT_HIP(hipMemcpyAsync(t->d_conf, conf, SN * 4, hipMemcpyHostToDevice, t->stream));
        RT_HIP(hipMemcpyAsync(t->d_cls, cls, SN * 4, hipMemcpyHostToDevice, t->stream));
    }
    RT_HIP(hipMemcpyAsync(t->d_n, t->h_n, (size_t)t->S * 4, hipMemcpyHostToDevice, t->stream));
    return RTMODT_OK;
}

// update_from_detector: the detector's device-resident outputs, on the tracker's device ...
inline int track_detector_outputs(const TrackHandleBase *t, rtmodt_detector *det, DetOutputs *o) {
    RT_TRY(detector_outputs(det, o));
    RT_CHECK(o->device == t->device, RTMODT_E_INVALID, "tracker on device %d, detector on device %d", t->device, o->device);
    return RTMODT_OK;
}
// ... `count` of its frames fit the handle ...
inline int track_detector_fits(const TrackHandleBase *t, const DetOutputs &o, int count) {
    RT_CHECK(count >= 1 && count <= t->S, RTMODT_E_INVALID, "%d frames > tracker streams %d", count, t->S);
    RT_CHECK(o.stride <= t->Nc, RTMODT_E_CAPACITY, "detector max_det %d > tracker max_dets %d", o.stride, t->Nc);
    RT_HIP(hipSetDevice(t->device));
    return RTMODT_OK;
}
// ... and after the launches on the detector's stream q: everything later on the tracker's own stream waits for them
inline int track_detector_done(TrackHandleBase *t, hipStream_t q) {
    RT_HIP(hipEventRecord(t->foreign_done, q));
    t->foreign_pending = true;
    return RTMODT_OK;
}

}  // namespace rtmodt
