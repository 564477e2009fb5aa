// track_select_dev.h -- which tracks of a tracker's device-resident state a per-frame consumer reads, and with which box: one
// function per source, and select_tracks, the one switch over a TrackSrc (kernels.h).  Shared by zones.hip, crossing.hip, speed.hip,
// snapshot.hip, privacy.hip, heatmap.hip, leftobj.hip and crosscam.hip.  Include inside namespace rtmodt, after kernels.h.
//   ByteTrack  time_since_update == report_tsu (1 = matched or spawned this frame), the track's box;
//   DeepSORT   confirmed (flag 2) and time_since_update == report_tsu (0 = matched this frame), the matched detection's box;
//   OC-SORT    returned: time_since_update == 0 and (hit_streak >= min_hits or frame_count <= min_hits), the last observation;
//   BoT-SORT   tracked (flag 2) and matched this frame (time_since_update == 0), the matched detection's box.
// `tm` is the stream's meta row (TrackViewBase::meta + 8 * stream): {cur, n_tracks, err, ..., frame_count at [5]}.
#pragma once

struct TrackSel {
    const int64_t *ids = nullptr; const float4 *box = nullptr; const int32_t *cls = nullptr;
    const float *conf = nullptr;                                           // null: a host list without confidences (snapshot.hip reads it)
    const int32_t *tsu = nullptr, *flag = nullptr, *streak = nullptr;      // null: the field does not take part
    int n = 0, want_tsu = 0, min_hits = 0;
    bool early = false;                                                    // OC-SORT: the first min_hits frames return every matched track
};

__device__ __forceinline__ TrackSel select_list(const int64_t *ids, const float4 *box, const int32_t *cls, int n) {
    TrackSel s;
    s.ids = ids; s.box = box; s.cls = cls; s.n = n;
    return s;
}
__device__ __forceinline__ TrackSel select_bytetrack(const TrackerState *st, const int64_t *tm, int report_tsu) {
    const int c = (int)tm[0] & 1;
    TrackSel s;
    s.ids = st->ids[c]; s.box = st->box[c]; s.cls = st->cls[c]; s.conf = st->conf[c]; s.tsu = st->tsu[c]; s.n = (int)tm[1]; s.want_tsu = report_tsu;
    return s;
}
__device__ __forceinline__ TrackSel select_deepsort(const DsState *st, const int64_t *tm, int report_tsu) {
    const int c = (int)tm[0] & 1;
    TrackSel s;
    s.ids = st->ids[c]; s.box = st->dbox[c]; s.cls = st->cls[c]; s.conf = st->conf[c]; s.tsu = st->tsu[c]; s.flag = st->flag[c]; s.n = (int)tm[1]; s.want_tsu = report_tsu;
    return s;
}
__device__ __forceinline__ TrackSel select_ocsort(const OcState *st, const int64_t *tm, int min_hits) {
    const int c = (int)tm[0] & 1;
    TrackSel s;
    s.ids = st->ids[c]; s.box = st->obox[c]; s.cls = st->cls[c]; s.conf = st->conf[c]; s.tsu = st->tsu[c]; s.streak = st->streak[c]; s.n = (int)tm[1];
    s.min_hits = min_hits; s.early = tm[5] <= (int64_t)min_hits;
    return s;
}
__device__ __forceinline__ TrackSel select_botsort(const BotState *st, const int64_t *tm) {
    const int c = (int)tm[0] & 1;
    TrackSel s;
    s.ids = st->ids[c]; s.box = st->dbox[c]; s.cls = st->cls[c]; s.conf = st->conf[c]; s.tsu = st->tsu[c]; s.flag = st->flag[c]; s.n = (int)tm[1];
    return s;
}
// the list of stream `stream` of a tracker source (a consumer with a list of its own asks select_list instead)
__device__ __forceinline__ TrackSel select_tracks(const TrackSrc &t, int stream) {
    const int64_t *tm = t.meta + (size_t)stream * 8;
    if (t.bytetrack) return select_bytetrack(t.bytetrack + stream, tm, t.report_tsu);
    if (t.deepsort) return select_deepsort(t.deepsort + stream, tm, t.report_tsu);
    if (t.ocsort) return select_ocsort(t.ocsort + stream, tm, t.min_hits);
    return select_botsort(t.botsort + stream, tm);
}
// is entry i of the list selected?  (a host list selects every entry)
__device__ __forceinline__ bool selected(const TrackSel &s, int i) {
    return (!s.tsu || s.tsu[i] == s.want_tsu) && (!s.flag || s.flag[i] == 2) && (!s.streak || s.early || s.streak[i] >= s.min_hits);
}
