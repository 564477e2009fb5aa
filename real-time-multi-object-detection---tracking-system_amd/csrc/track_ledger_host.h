// track_ledger_host.h -- the host side every ledger module repeats (zones.hip, crossing.hip, speed.hip, snapshot.hip): lists staged in
// id order, the sticky error decoded, a tracker's view checked against the handle.  Include at file scope.
#pragma once

#include <vector>

#include "kernels.h"
#include "track_ledger.h"

namespace rtmodt {

// a module's staging arrays: one row of `stride` entries per stream, sorted by id; order = the caller's index of a sorted entry, inv =
// its inverse (null: the module stages none)
struct LedgerStaging { int64_t *ids; float4 *box; int32_t *cls, *order, *inv, *n; int stride; };

// the lists of streams [s0, s0 + cnt), rows of in_stride entries -> the staging arrays, copied on q and waited for (the vectors are
// pageable and about to go away).  A list that holds an id twice is refused; name_stream: the message names the stream
inline int ledger_stage_lists(const LedgerStaging &d, int s0, int cnt, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n,
                              int in_stride, bool name_stream, hipStream_t q) {
    const size_t R = d.stride, m = (size_t)cnt * R;
    std::vector<int32_t> perm(m), inv(d.inv ? m : 0), kc(m);
    std::vector<int64_t> ids(m);
    std::vector<float4> box(m);
    for (int s = 0; s < cnt; ++s) {
        const int64_t *ti = track_ids + (size_t)s * in_stride;
        const float *tb = xyxy + (size_t)s * in_stride * 4;
        const int32_t *tc = cls + (size_t)s * in_stride;
        int32_t *pm = perm.data() + s * R;
        const int dup = tl_sort_list(ti, n[s], pm, d.inv ? inv.data() + s * R : nullptr);
        if (dup >= 0 && name_stream) return fail(RTMODT_E_INVALID, "stream %d: track id %lld appears twice", s0 + s, (long long)ti[pm[dup]]);
        if (dup >= 0) return fail(RTMODT_E_INVALID, "track id %lld appears twice", (long long)ti[pm[dup]]);
        for (int i = 0; i < n[s]; ++i) {
            const int p = pm[i];
            ids[s * R + i] = ti[p]; kc[s * R + i] = tc[p];
            box[s * R + i] = make_float4(tb[4 * p], tb[4 * p + 1], tb[4 * p + 2], tb[4 * p + 3]);
        }
    }
    const size_t o = (size_t)s0 * R, len = cnt == 1 ? (size_t)n[0] : m;      // one list: its entries; several: whole rows
    if (len) {
        RT_HIP(hipMemcpyAsync(d.ids + o, ids.data(), len * 8, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(d.box + o, box.data(), len * 16, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(d.cls + o, kc.data(), len * 4, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(d.order + o, perm.data(), len * 4, hipMemcpyHostToDevice, q));
        if (d.inv) RT_HIP(hipMemcpyAsync(d.inv + o, inv.data(), len * 4, hipMemcpyHostToDevice, q));
    }
    RT_HIP(hipMemcpyAsync(d.n + s0, n, (size_t)cnt * 4, hipMemcpyHostToDevice, q));
    RT_HIP(hipStreamSynchronize(q));
    return RTMODT_OK;
}

// a stream's sticky error (meta[2]): 1 = the ledger overflowed; `hint` says what the caller can change
inline int ledger_check_sticky(const char *module, int stream, long long err, int cap, const char *hint) {
    RT_CHECK(err != 1, RTMODT_E_CAPACITY, "%s stream %d: ledger full (%d rows): %s", module, stream, cap, hint);
    RT_CHECK(err == 0, RTMODT_E_INVALID, "%s stream %d: error %lld", module, stream, err);
    return RTMODT_OK;
}

// a tracker's view against a handle on `device` with S streams: at most max_tracks tracks (shown: the figure the message quotes)
inline int ledger_check_view(const TrackViewBase &v, int device, int S, int max_tracks, int shown, const char *handle, const char *module) {
    RT_CHECK(v.device == device, RTMODT_E_INVALID, "%s on device %d, tracker on device %d", handle, device, v.device);
    RT_CHECK(v.n_streams <= S && v.max_tracks <= max_tracks, RTMODT_E_INVALID, "tracker (%d streams, %d tracks) larger than the %s (%d, %d)", v.n_streams,
             v.max_tracks, module, S, shown);
    return RTMODT_OK;
}

}  // namespace rtmodt
