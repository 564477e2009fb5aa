// track_layout.h -- the pure host pieces the trackers and their consumers share: the pool carver, the state layouts of the four
// trackers, and the read-back of a Kalman block.  No HIP header: a plain C++ compiler builds it (tests/native/track_layout_check.cpp).
//
// A pool is laid out by ONE function that is run twice -- base == nullptr measures, a real base assigns -- so a size can never
// disagree with the layout it was computed for.  Every array starts on a 16-byte boundary whatever max_tracks is.  The layouts are
// templates over the state struct (kernels.h: TrackerState, DsState, OcState, BotState): an array's element type is its field's.
#pragma once

#include <cstddef>

namespace rtmodt {

struct Carver {
    char *base; size_t off = 0;
    template <typename T> T *take(size_t count) {
        off = (off + 15) / 16 * 16;
        T *p = base ? (T *)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    template <typename T> void take(T *&field, size_t count) { field = take<T>(count); }
    size_t size() const { return (off + 15) / 16 * 16; }
};

// ByteTrack (tracker_api.hip): states[S]; M = max_tracks
template <typename St> size_t carve_bytetrack(St *states, size_t S, size_t M, char *base) {
    Carver c{base};
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            St &st = states[s];
            c.take(st.ids[b], M); c.take(st.box[b], M); c.take(st.conf[b], M); c.take(st.cls[b], M); c.take(st.age[b], M); c.take(st.tsu[b], M);
        }
    return c.size();
}
// its opt-in Kalman blocks, a pool of their own (rtmodt_tracker_enable_kalman)
template <typename St> size_t carve_bytetrack_kf(St *states, size_t S, size_t M, char *base) {
    Carver c{base};
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) c.take(states[s].kf[b], 5 * M);
    return c.size();
}
// DeepSORT (deepsort.hip)
template <typename St> size_t carve_deepsort(St *states, size_t S, size_t M, char *base) {
    Carver c{base};
    for (size_t s = 0; s < S; ++s) {
        St &st = states[s];
        for (int b = 0; b < 2; ++b) {
            c.take(st.kf[b], 5 * M); c.take(st.dbox[b], M); c.take(st.ids[b], M); c.take(st.conf[b], M);
            c.take(st.cls[b], M); c.take(st.flag[b], M); c.take(st.hits[b], M); c.take(st.age[b], M); c.take(st.tsu[b], M);
            c.take(st.slot[b], M); c.take(st.gcount[b], M);
        }
        c.take(st.slot_used, M);
    }
    return c.size();
}
// OC-SORT (ocsort.hip); R = OC_RING
template <typename St> size_t carve_ocsort(St *states, size_t S, size_t M, size_t R, char *base) {
    Carver c{base};
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            St &st = states[s];
            c.take(st.kf[b], 5 * M); c.take(st.saved[b], 5 * M); c.take(st.ring[b], R * M); c.take(st.ring_age[b], R * M);
            c.take(st.obox[b], M); c.take(st.ids[b], M); c.take(st.dir[b], M); c.take(st.conf[b], M);
            c.take(st.cls[b], M); c.take(st.hits[b], M); c.take(st.streak[b], M); c.take(st.age[b], M); c.take(st.tsu[b], M);
        }
    return c.size();
}

// BoT-SORT (botsort.hip)
template <typename St> size_t carve_botsort(St *states, size_t S, size_t M, char *base) {
    Carver c{base};
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            St &st = states[s];
            c.take(st.kf[b], 7 * M); c.take(st.dbox[b], M); c.take(st.ids[b], M); c.take(st.conf[b], M); c.take(st.cls[b], M);
            c.take(st.flag[b], M); c.take(st.age[b], M); c.take(st.tsu[b], M); c.take(st.start[b], M); c.take(st.last[b], M);
        }
    return c.size();
}

// A Kalman block ([5][Mc] float4 = mean, velocities, and the a / b / c entries of the four 2x2 covariance blocks; here as 4 floats
// each) -> mean[cnt][8] = (mean, velocities) and cov[cnt][12] = per coordinate (a, b, c) of [[a, b], [b, c]].  Either may be null.
inline void kalman_unpack(const float *block, size_t Mc, int cnt, float *mean, float *cov) {
    for (size_t i = 0; i < (size_t)cnt; ++i) {
        const float *pos = block + 4 * i, *vel = pos + 4 * Mc, *pa = vel + 4 * Mc, *pb = pa + 4 * Mc, *pc = pb + 4 * Mc;
        for (int k = 0; k < 4; ++k) {
            if (mean) { mean[8 * i + k] = pos[k]; mean[8 * i + 4 + k] = vel[k]; }
            if (cov) { cov[12 * i + 3 * k] = pa[k]; cov[12 * i + 3 * k + 1] = pb[k]; cov[12 * i + 3 * k + 2] = pc[k]; }
        }
    }
}

// BoT-SORT's block ([7][Mc] float4 = mean, velocities, 5 x 4 covariance entries) -> mean[cnt][8] and cov[cnt][20] = the upper triangles,
// row-major, of the (cx, cy, vx, vy) block and of the (w, h, vw, vh) block.  Either may be null.
inline void botsort_unpack(const float *block, size_t Mc, int cnt, float *mean, float *cov) {
    for (size_t i = 0; i < (size_t)cnt; ++i)
        for (int q = 0; q < 7; ++q)
            for (int k = 0; k < 4; ++k) {
                const float v = block[4 * (q * Mc + i) + k];
                if (q < 2) { if (mean) mean[8 * i + 4 * q + k] = v; }
                else if (cov) cov[20 * i + 4 * (q - 2) + k] = v;
            }
}

}  // namespace rtmodt
