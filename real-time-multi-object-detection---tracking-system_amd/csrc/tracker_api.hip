// tracker_api.hip -- the tracker half of include/rtmodt.h: handle lifetime, staging, and
// the three ways a frame's detections reach the kernel in tracker.hip (host arrays for one
// stream, host arrays for all streams, or the detector's device-resident outputs).
// Mirrors _ByteTrackCore's constructor and update() (/root/reference/src/tracking/tracker.py:46-141).
#include <cstring>
#include <vector>

#include "track_host.h"

using namespace rtmodt;

struct rtmodt_tracker : TrackHandleBase {
    bool kalman = false;                  // opt-in motion model (rtmodt_tracker_enable_kalman)
    char *kf_pool = nullptr;
    float track_thresh = 0.5f, match_thresh = 0.8f;
    int track_buffer = 30;
    int assign_mode = RTMODT_ASSIGN_GREEDY;
    double cost_limit = 0.2;
    char *pool = nullptr;                 // all state arrays (track_layout.h: carve_bytetrack)
    TrackerState *d_states = nullptr;
    std::vector<TrackerState> h_states;
    char *h_state = nullptr;              // pinned: one stream's state arrays (rtmodt_tracker_state): 40 bytes per track
};

namespace rtmodt {
int tracker_device_view(rtmodt_tracker *t, TrackerDeviceView *out) {
    RT_CHECK(t && out, RTMODT_E_INVALID, "null argument");
    out->states = t->d_states;
    return track_view(t, out);
}
int tracker_device_view_mut(rtmodt_tracker *t, TrackerDeviceViewMut *out) {
    RT_CHECK(t && out, RTMODT_E_INVALID, "null argument");
    out->states = t->d_states;
    return track_view(t, out);
}
}  // namespace rtmodt

extern "C" {

void rtmodt_tracker_destroy(rtmodt_tracker *t) {
    if (!t) return;
    track_close(t, [t] { hipFree(t->kf_pool); hipFree(t->pool); hipFree(t->d_states); hipHostFree(t->h_state); });
    delete t;
}

static int tracker_create_impl(rtmodt_tracker *t) {
    RT_TRY(track_open(t));
    t->h_states.assign(t->S, TrackerState{});
    const size_t total = carve_bytetrack(t->h_states.data(), t->S, t->Mc, nullptr);
    RT_HIP(hipMalloc((void **)&t->pool, total));
    RT_HIP(handle_zero(t->pool, total, t->stream));
    carve_bytetrack(t->h_states.data(), t->S, t->Mc, t->pool);
    RT_HIP(hipMalloc((void **)&t->d_states, sizeof(TrackerState) * t->S));
    RT_HIP(hipMemcpy(t->d_states, t->h_states.data(), sizeof(TrackerState) * t->S, hipMemcpyHostToDevice));
    RT_HIP(hipHostMalloc((void **)&t->h_state, (size_t)t->Mc * 40, hipHostMallocDefault));
    return RTMODT_OK;
}

int rtmodt_tracker_create(int device, float track_thresh, int track_buffer, float match_thresh, int assign_mode, int max_tracks,
                          int max_dets, int n_streams, rtmodt_tracker **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(assign_mode == RTMODT_ASSIGN_GREEDY || assign_mode == RTMODT_ASSIGN_LAPJV, RTMODT_E_UNSUPPORTED,
             "assign_mode %d: 0 (greedy, tracker.py:182-194) or 1 (lapjv, tracker.py:168-181)", assign_mode);
    RT_CHECK(max_tracks >= 1 && max_tracks <= 4096 && max_dets >= 1 && max_dets <= 4096 && n_streams >= 1 && n_streams <= 4096,
             RTMODT_E_INVALID, "max_tracks %d / max_dets %d / n_streams %d out of range", max_tracks, max_dets, n_streams);
    rtmodt_tracker *t = new rtmodt_tracker();
    t->device = device; t->S = n_streams; t->Mc = max_tracks; t->Nc = max_dets;
    t->track_thresh = track_thresh; t->match_thresh = match_thresh; t->track_buffer = track_buffer;
    t->assign_mode = assign_mode; t->cost_limit = 1.0 - (double)match_thresh;
    return handle_created(tracker_create_impl(t), t, rtmodt_tracker_destroy, out);
}

int rtmodt_tracker_set_cost_limit(rtmodt_tracker *t, double cost_limit) {
    RT_CHECK(t && cost_limit == cost_limit, RTMODT_E_INVALID, "bad argument");
    t->cost_limit = cost_limit;
    return RTMODT_OK;
}

static TrackerArgs make_args(rtmodt_tracker *t) {
    TrackerArgs a{};
    a.n_streams = t->S; a.stream_base = 0; a.max_tracks = t->Mc; a.max_dets = t->Nc;
    a.track_thresh = t->track_thresh; a.match_thresh = t->match_thresh; a.track_buffer = t->track_buffer;
    a.assign_mode = t->assign_mode; a.cost_limit = t->cost_limit; a.kalman = t->kalman ? 1 : 0;
    a.states = t->d_states; a.meta = t->d_meta;
    a.det_box = t->d_box; a.det_conf = t->d_conf; a.det_cls = t->d_cls; a.det_n = t->d_n; a.det_stride = t->Nc;
    return a;
}

static int check_sticky(rtmodt_tracker *t, int s, int64_t err) { return track_check_sticky(t, s, err, "lapjv assignment"); }

// reads back meta rows [s0, s0+cnt) after the launch; raises the sticky capacity error
static int finish(rtmodt_tracker *t, int s0, int cnt, int32_t *n_active_out) {
    RT_HIP(hipMemcpyAsync(t->h_meta + 8 * s0, t->d_meta + 8 * s0, sizeof(int64_t) * 8 * cnt, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(hipStreamSynchronize(t->stream));
    for (int s = s0; s < s0 + cnt; ++s) {
        if (n_active_out) n_active_out[s - s0] = (int32_t)t->h_meta[8 * s + 3];
        RT_TRY(check_sticky(t, s, t->h_meta[8 * s + 2]));
    }
    return RTMODT_OK;
}

int rtmodt_tracker_update(rtmodt_tracker *t, int stream, const float *xyxy, const float *conf, const int32_t *cls, int n,
                          int32_t *n_active_out) {
    RT_CHECK(t && stream >= 0 && stream < t->S && n >= 0, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n == 0 || (xyxy && conf && cls), RTMODT_E_INVALID, "null detections");
    RT_CHECK(n <= t->Nc, RTMODT_E_CAPACITY, "%d detections > max_dets %d", n, t->Nc);
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    t->h_n[stream] = n;
    if (n) {
        RT_HIP(hipMemcpyAsync(t->d_box + (size_t)stream * t->Nc, xyxy, (size_t)n * 16, hipMemcpyHostToDevice, t->stream));
        RT_HIP(hipMemcpyAsync(t->d_conf + (size_t)stream * t->Nc, conf, (size_t)n * 4, hipMemcpyHostToDevice, t->stream));
        RT_HIP(hipMemcpyAsync(t->d_cls + (size_t)stream * t->Nc, cls, (size_t)n * 4, hipMemcpyHostToDevice, t->stream));
    }
    RT_HIP(hipMemcpyAsync(t->d_n + stream, t->h_n + stream, 4, hipMemcpyHostToDevice, t->stream));
    TrackerArgs a = make_args(t);
    a.n_streams = 1; a.stream_base = stream;
    RT_TRY(launch_tracker_update(a, t->stream));
    return finish(t, stream, 1, n_active_out);
}

int rtmodt_tracker_update_batch(rtmodt_tracker *t, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                                int32_t *n_active_out) {
    RT_CHECK(t && n, RTMODT_E_INVALID, "null argument");
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    for (int s = 0; s < t->S; ++s)
        RT_CHECK(n[s] >= 0 && n[s] <= t->Nc, RTMODT_E_CAPACITY, "stream %d: %d detections > max_dets %d", s, n[s], t->Nc);
    RT_TRY(track_batch_stage(t, xyxy, conf, cls, n, true));      // (this call has always copied the arrays, detections or not)
    RT_TRY(launch_tracker_update(make_args(t), t->stream));
    return finish(t, 0, t->S, n_active_out);
}

// frames [first, first + count * frames) of device-resident detections `o` (a detector's, or a slicer's merged ones), on o.stream
static int update_from_outputs(rtmodt_tracker *t, const DetOutputs &o, int first, int count, int frames) {
    if (count < 0) count = o.count - first;
    RT_CHECK(frames >= 1, RTMODT_E_INVALID, "n_frames %d", frames);
    RT_CHECK(first >= 0 && count >= 1 && (long)first + (long)count * frames <= o.count, RTMODT_E_INVALID, "frames [%d, %ld) outside the detector's batch of %d", first,
             (long)first + (long)count * frames, o.count);
    RT_TRY(track_detector_fits(t, o, count));
    TrackerArgs a = make_args(t);
    a.n_streams = count;
    a.det_box = o.box + (size_t)first * o.stride; a.det_conf = o.conf + (size_t)first * o.stride; a.det_cls = o.cls + (size_t)first * o.stride;
    a.det_n = o.n + first; a.det_stride = o.stride;
    a.n_frames = frames; a.frame_step = count;
    // (host-fed updates are synchronous -- finish() waits for them -- so the detector's stream needs no event from ours)
    RT_TRY(launch_tracker_update(a, o.stream));          // same HIP stream as the detector's NMS: ordered, no host sync
    return track_detector_done(t, o.stream);
}

static int update_from_detector_slice(rtmodt_tracker *t, rtmodt_detector *det, int first, int count, int frames = 1) {
    RT_CHECK(t && det, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(track_detector_outputs(t, det, &o));
    return update_from_outputs(t, o, first, count, frames);
}

int rtmodt_tracker_update_from_slicer(rtmodt_tracker *t, rtmodt_slicer *s) {
    RT_CHECK(t && s, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(slicer_outputs(s, &o));
    RT_CHECK(o.device == t->device, RTMODT_E_INVALID, "tracker on device %d, slicer on device %d", t->device, o.device);
    return update_from_outputs(t, o, 0, -1, 1);
}

int rtmodt_tracker_update_from_detector(rtmodt_tracker *t, rtmodt_detector *det) { return update_from_detector_slice(t, det, 0, -1); }

int rtmodt_tracker_update_from_detector_frames(rtmodt_tracker *t, rtmodt_detector *det, int first_frame, int n_frames) {
    RT_CHECK(n_frames >= 1, RTMODT_E_INVALID, "n_frames %d", n_frames);
    return update_from_detector_slice(t, det, first_frame, n_frames);
}

int rtmodt_tracker_update_from_detector_batch(rtmodt_tracker *t, rtmodt_detector *det, int first_frame, int n_streams, int n_frames) {
    RT_CHECK(n_streams >= 1 && n_frames >= 1, RTMODT_E_INVALID, "n_streams %d, n_frames %d", n_streams, n_frames);
    return update_from_detector_slice(t, det, first_frame, n_streams, n_frames);
}

int rtmodt_tracker_state(rtmodt_tracker *t, int stream, int64_t *ids, float *xyxy, float *conf, int32_t *cls, int32_t *age,
                         int32_t *tsu, int32_t *n, int64_t *next_id) {
    RT_CHECK(t && stream >= 0 && stream < t->S, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(t->device));
    // ordered behind the most recent update (own stream, or -- through its event -- a detector's): meta first, then the arrays
    // of the buffer it names, all through pinned memory -- two stream syncs instead of a device sync and seven blocking copies
    RT_TRY(track_join(t));
    hipStream_t q = t->stream;
    int64_t *m = t->h_meta + 8 * stream;
    RT_HIP(hipMemcpyAsync(m, t->d_meta + 8 * stream, sizeof(int64_t) * 8, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    RT_TRY(check_sticky(t, stream, m[2]));
    const int cur = (int)m[0], cnt = (int)m[1];
    const TrackerState &st = t->h_states[stream];
    if (n) *n = cnt;
    if (next_id) *next_id = m[4];
    if (cnt) {
        char *h = t->h_state;
        const size_t M = (size_t)t->Mc;
        char *h_ids = h, *h_box = h + M * 8, *h_conf = h + M * 24, *h_cls = h + M * 28, *h_age = h + M * 32, *h_tsu = h + M * 36;
        if (ids) RT_HIP(hipMemcpyAsync(h_ids, st.ids[cur], (size_t)cnt * 8, hipMemcpyDeviceToHost, q));
        if (xyxy) RT_HIP(hipMemcpyAsync(h_box, st.box[cur], (size_t)cnt * 16, hipMemcpyDeviceToHost, q));
        if (conf) RT_HIP(hipMemcpyAsync(h_conf, st.conf[cur], (size_t)cnt * 4, hipMemcpyDeviceToHost, q));
        if (cls) RT_HIP(hipMemcpyAsync(h_cls, st.cls[cur], (size_t)cnt * 4, hipMemcpyDeviceToHost, q));
        if (age) RT_HIP(hipMemcpyAsync(h_age, st.age[cur], (size_t)cnt * 4, hipMemcpyDeviceToHost, q));
        if (tsu) RT_HIP(hipMemcpyAsync(h_tsu, st.tsu[cur], (size_t)cnt * 4, hipMemcpyDeviceToHost, q));
        RT_HIP(hipStreamSynchronize(q));
        if (ids) memcpy(ids, h_ids, (size_t)cnt * 8);
        if (xyxy) memcpy(xyxy, h_box, (size_t)cnt * 16);
        if (conf) memcpy(conf, h_conf, (size_t)cnt * 4);
        if (cls) memcpy(cls, h_cls, (size_t)cnt * 4);
        if (age) memcpy(age, h_age, (size_t)cnt * 4);
        if (tsu) memcpy(tsu, h_tsu, (size_t)cnt * 4);
    }
    return RTMODT_OK;
}

int rtmodt_tracker_enable_kalman(rtmodt_tracker *t) {
    RT_CHECK(t, RTMODT_E_INVALID, "null argument");
    if (t->kalman) return RTMODT_OK;
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    RT_HIP(hipMemcpyAsync(t->h_meta, t->d_meta, sizeof(int64_t) * 8 * t->S, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(hipStreamSynchronize(t->stream));
    for (int s = 0; s < t->S; ++s)
        RT_CHECK(t->h_meta[8 * s + 1] == 0, RTMODT_E_INVALID, "stream %d already holds tracks: enable the Kalman model before the first update (or after reset)", s);
    const size_t total = carve_bytetrack_kf(t->h_states.data(), t->S, t->Mc, nullptr);
    RT_HIP(hipMalloc((void **)&t->kf_pool, total));
    RT_HIP(handle_zero(t->kf_pool, total, t->stream));
    carve_bytetrack_kf(t->h_states.data(), t->S, t->Mc, t->kf_pool);
    RT_HIP(hipMemcpy(t->d_states, t->h_states.data(), sizeof(TrackerState) * t->S, hipMemcpyHostToDevice));
    RT_TRY(handle_wait(t->stream));
    t->kalman = true;
    return RTMODT_OK;
}

int rtmodt_tracker_kalman_state(rtmodt_tracker *t, int stream, float *mean, float *cov, int32_t *n) {
    RT_CHECK(t && stream >= 0 && stream < t->S && n, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(t->kalman, RTMODT_E_INVALID, "the Kalman model is not enabled on this tracker");
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    int64_t *m = t->h_meta + 8 * stream;
    RT_HIP(hipMemcpyAsync(m, t->d_meta + 8 * stream, sizeof(int64_t) * 8, hipMemcpyDeviceToHost, t->stream));
    RT_HIP(hipStreamSynchronize(t->stream));
    RT_TRY(check_sticky(t, stream, m[2]));
    const int cur = (int)m[0], cnt = (int)m[1];
    *n = cnt;
    if (!cnt) return RTMODT_OK;
    std::vector<float4> buf((size_t)5 * t->Mc);
    RT_HIP(hipMemcpy(buf.data(), t->h_states[stream].kf[cur], buf.size() * sizeof(float4), hipMemcpyDeviceToHost));
    kalman_unpack(&buf[0].x, t->Mc, cnt, mean, cov);
    return RTMODT_OK;
}

int rtmodt_tracker_reset(rtmodt_tracker *t, int stream) { return track_reset_meta(t, stream); }

int rtmodt_iou_matrix(int device, const float *a, int m, const float *b, int n, float *out) {
    RT_CHECK(m >= 0 && n >= 0 && (m * (long)n == 0 || (a && b && out)), RTMODT_E_INVALID, "bad argument");
    if ((long)m * n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(device));
    float4 *da = nullptr, *db = nullptr; float *dout = nullptr;
    int rc = RTMODT_OK;
    auto body = [&]() -> int {
        RT_HIP(hipMalloc((void **)&da, (size_t)m * 16)); RT_HIP(hipMalloc((void **)&db, (size_t)n * 16));
        RT_HIP(hipMalloc((void **)&dout, (size_t)m * n * 4));
        RT_HIP(hipMemcpy(da, a, (size_t)m * 16, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(db, b, (size_t)n * 16, hipMemcpyHostToDevice));
        RT_TRY(launch_iou_matrix(da, m, db, n, dout, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(out, dout, (size_t)m * n * 4, hipMemcpyDeviceToHost));
        return RTMODT_OK;
    };
    rc = body();
    hipFree(da); hipFree(db); hipFree(dout);
    return rc;
}

int rtmodt_assign_greedy(int device, const float *iou, int m, int n, float thresh, int32_t *row_to_col, int32_t *col_used) {
    RT_CHECK(m >= 1 && n >= 1 && iou && row_to_col && col_used, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(device));
    float *di = nullptr; int32_t *dr = nullptr, *dc = nullptr;
    auto body = [&]() -> int {
        RT_HIP(hipMalloc((void **)&di, (size_t)m * n * 4)); RT_HIP(hipMalloc((void **)&dr, (size_t)m * 4));
        RT_HIP(hipMalloc((void **)&dc, (size_t)n * 4));
        RT_HIP(hipMemcpy(di, iou, (size_t)m * n * 4, hipMemcpyHostToDevice));
        RT_TRY(launch_assign_greedy(di, m, n, thresh, dr, dc, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(row_to_col, dr, (size_t)m * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(col_used, dc, (size_t)n * 4, hipMemcpyDeviceToHost));
        return RTMODT_OK;
    };
    int rc = body();
    hipFree(di); hipFree(dr); hipFree(dc);
    return rc;
}

int rtmodt_assign_lapjv(int device, const float *iou, int m, int n, double cost_limit, int32_t *row_to_col, int32_t *col_used) {
    RT_CHECK(m >= 1 && n >= 1 && m <= 4096 && n <= 4096 && iou && row_to_col && col_used && cost_limit == cost_limit, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(device));
    float *di = nullptr; int32_t *dr = nullptr, *dc = nullptr, *de = nullptr;
    int32_t err = 0;
    auto body = [&]() -> int {
        RT_HIP(hipMalloc((void **)&di, (size_t)m * n * 4)); RT_HIP(hipMalloc((void **)&dr, (size_t)m * 4));
        RT_HIP(hipMalloc((void **)&dc, (size_t)n * 4)); RT_HIP(hipMalloc((void **)&de, 4));
        RT_HIP(hipMemcpy(di, iou, (size_t)m * n * 4, hipMemcpyHostToDevice));
        RT_TRY(launch_assign_lapjv(di, m, n, cost_limit, dr, dc, de, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(row_to_col, dr, (size_t)m * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(col_used, dc, (size_t)n * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(&err, de, 4, hipMemcpyDeviceToHost));
        RT_CHECK(err == 0, RTMODT_E_CAPACITY, "assign_lapjv: too dense (more than 256 contested rows/columns or 2048 contested pairs)");
        return RTMODT_OK;
    };
    int rc = body();
    hipFree(di); hipFree(dr); hipFree(dc); hipFree(de);
    return rc;
}

}  // extern "C"
