// leftobj_rule.h -- the one statement of the left / removed object detector's rules (csrc/leftobj.hip runs them per frame; its
// header states the mask, the regions, the matching and the launches).  Plain C++, no HIP: the kernels of leftobj.hip, the
// host-only entry point rtmodt_leftobj_cell and tests/native/leftobj_rule_check.cpp (built under the address and UB sanitizers) all
// take them from here, and tests/leftobj_ref.py restates them in NumPy / plain Python.  Everything is integer arithmetic.
//   Grid, cell luma Yc and pixel boxes: motion_model.h, unchanged.
//   Cell.   8 bytes, one load and one store: bg | cand << 16 (unsigned 8.8 fixed point) | age << 32 (16 bits) | miss << 48 (8 bits) |
//           flags << 56 (bit 0: ignore).  With t = Yc << 8:
//             frames_seen == 0:      bg = cand = t, age = miss = 0 (the flags stay).
//             frames_seen < warmup:  bg += (t - bg) >> warm_shift; nothing is foreground.
//             otherwise              fg = |t - bg| > threshold << 8.
//               not fg:              bg += (t - bg) >> learn_shift; if age > 0, miss += 1, and a miss above `occlusion` sets age = miss = 0.
//               fg, |t - cand| <= stable << 8:   cand += (t - cand) >> cand_shift, age = min(age + 1, 65535), miss = 0.
//               fg, not stable:      age > 0 and miss < occlusion: miss += 1 (someone walks in front: cand and age are kept);
//                                    else cand = t, age = 1, miss = 0.
//           Foreground never updates bg.  Every shift is an arithmetic shift of the signed difference, as in mo_cell.
//           static = age >= static_frames && !ignore.
//   Kind.   At a region, cur = the sum over its mask cells c and their 4-neighbours n inside the grid and outside the mask of
//           |(cand[c] >> 8) - Y[n]|, bgc = the same sum of |(bg[c] >> 8) - (bg[n] >> 8)| (the model after this frame's update):
//           ABANDONED if cur > bgc (the edge is in the picture), REMOVED if bgc > cur (the edge is in the model), else UNKNOWN.
//   Status. WARMUP if frames_seen < warmup at entry, else SCENE_CHANGE if 1000 * n_fg >= scene_pm * cells (the model restarts:
//           frames_seen = 0, every ledger entry retires with RESET), else STATIC with a region, else CLEAR.
//   Tracks. A track's box is rounded once: x0, y0 = floor, x1, y1 = ceil of the float32 value clamped to -2^20 .. 2^20; a box with a
//           coordinate that is not finite, or empty after rounding, takes no part.
//             covered:   1000 * area(track box ∩ region box) >= covered_pm * area(region box), pixels;
//             attended:  the track's class is an owner class and its box grown by attend_margin overlaps the region box.
//   Match.  Stored regions in raster order; each takes the still-free entry whose cell box (inclusive) shares most cells with its
//           own, the lowest oid on a tie; no shared cell is no match.
//   Timers. On a call that matches (or bears) an entry: attended -> idle = 0 and the owner is remembered (the largest attending id);
//           else idle += 1 unless the region is covered and no covering track is of a report class.  Until the alarm, kind is the region's, or
//           TRACKED_STATIC when a track of a report class covers it.  idle >= alarm_frames for the first time: one event, latched.
//           Then, frame_id - first_frame >= absorb_frames (0: never): the entry retires ABSORBED and the region's cells take
//           bg = cand, age = miss = 0.  An entry no region matched gains unmatched += 1 and retires CLEARED above miss_frames.
#pragma once

#include <cstdint>

#include "motion_model.h"

namespace rtmodt {

constexpr int LO_WARMUP = 0, LO_CLEAR = 1, LO_STATIC = 2, LO_SCENE_CHANGE = 3;
constexpr int LO_UNKNOWN = 0, LO_ABANDONED = 1, LO_REMOVED = 2, LO_TRACKED_STATIC = 3;
constexpr int LO_CLEARED = 1, LO_ABSORBED = 2, LO_RESET = 3;
constexpr int LO_MAX_REGIONS = 256, LO_MAX_OBJECTS = 256, LO_MAX_TRACKS = 4096, LO_MAX_CLASSES = 8, LO_BOX_LIMIT = 1 << 20;

struct LoRule { int32_t warmup, warm_shift, learn_shift, threshold, stable, cand_shift, occlusion, static_frames; };
struct LoCell { uint32_t bg, cand, age, miss, flags; };

MO_HD inline bool lo_rule_ok(const LoRule &r) {
    return r.warmup >= 1 && r.warmup <= 255 && r.warm_shift >= 1 && r.warm_shift <= 8 && r.learn_shift >= 1 && r.learn_shift <= 12 &&
           r.threshold >= 1 && r.threshold <= 255 && r.stable >= 1 && r.stable <= 255 && r.cand_shift >= 1 && r.cand_shift <= 8 &&
           r.occlusion >= 0 && r.occlusion <= 254 && r.static_frames >= 1 && r.static_frames <= 65535;
}

MO_HD inline uint64_t lo_pack(const LoCell &c) {
    return (uint64_t)c.bg | (uint64_t)c.cand << 16 | (uint64_t)c.age << 32 | (uint64_t)c.miss << 48 | (uint64_t)c.flags << 56;
}
MO_HD inline LoCell lo_unpack(uint64_t v) {
    return LoCell{(uint32_t)(v & 0xffffu), (uint32_t)(v >> 16 & 0xffffu), (uint32_t)(v >> 32 & 0xffffu), (uint32_t)(v >> 48 & 0xffu), (uint32_t)(v >> 56)};
}

// one cell of one frame: updates the cell and returns whether it is foreground
MO_HD inline bool lo_cell(const LoRule &r, uint32_t yc, int32_t frames_seen, LoCell &c) {
    const int32_t t = (int32_t)(yc << 8);
    if (frames_seen == 0) {
        c.bg = c.cand = (uint32_t)t; c.age = c.miss = 0;
        return false;
    }
    const int32_t d = t - (int32_t)c.bg, ad = d < 0 ? -d : d;
    if (frames_seen < r.warmup) {
        c.bg = (uint32_t)((int32_t)c.bg + (d >> r.warm_shift));
        return false;
    }
    if (ad <= r.threshold << 8) {
        c.bg = (uint32_t)((int32_t)c.bg + (d >> r.learn_shift));
        if (c.age > 0 && ++c.miss > (uint32_t)r.occlusion) c.age = c.miss = 0;
        return false;
    }
    const int32_t e = t - (int32_t)c.cand, ae = e < 0 ? -e : e;
    if (ae <= r.stable << 8) {
        c.cand = (uint32_t)((int32_t)c.cand + (e >> r.cand_shift));
        c.age = c.age < 65535u ? c.age + 1 : 65535u;
        c.miss = 0;
    } else if (c.age > 0 && c.miss < (uint32_t)r.occlusion) {
        ++c.miss;
    } else {
        c.cand = (uint32_t)t; c.age = 1; c.miss = 0;
    }
    return true;
}
MO_HD inline bool lo_static(const LoRule &r, const LoCell &c) { return c.age >= (uint32_t)r.static_frames && !(c.flags & 1u); }

MO_HD inline int32_t lo_absdiff(int32_t a, int32_t b) { return a < b ? b - a : a - b; }
MO_HD inline int32_t lo_kind(uint64_t cur, uint64_t bgc) { return cur > bgc ? LO_ABANDONED : (bgc > cur ? LO_REMOVED : LO_UNKNOWN); }

MO_HD inline int32_t lo_status(int32_t frames_seen, int32_t warmup, uint32_t n_fg, int32_t scene_pm, int64_t cells, uint32_t n_regions_total) {
    if (frames_seen < warmup) return LO_WARMUP;
    if (1000LL * (int64_t)n_fg >= (int64_t)scene_pm * cells) return LO_SCENE_CHANGE;
    return n_regions_total >= 1 ? LO_STATIC : LO_CLEAR;
}
MO_HD inline int32_t lo_next_seen(int32_t frames_seen, int32_t status) {
    return status == LO_SCENE_CHANGE ? 0 : (frames_seen + 1 < MO_MAX_SEEN ? frames_seen + 1 : MO_MAX_SEEN);
}

// ---- tracks against a region's pixel box (x1, y1 exclusive) ------------------------------------------------------------
MO_HD inline bool lo_finite(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}
// floor (up == false) or ceil of a finite value clamped to +-LO_BOX_LIMIT
MO_HD inline int32_t lo_round(float v, bool up) {
    const float lim = (float)LO_BOX_LIMIT;
    v = v < -lim ? -lim : (v > lim ? lim : v);
    const int32_t i = (int32_t)v;                           // towards zero
    if (up) return (float)i < v ? i + 1 : i;
    return (float)i > v ? i - 1 : i;
}
MO_HD inline bool lo_track_box(float x0, float y0, float x1, float y1, int32_t *out) {
    if (!lo_finite(x0) || !lo_finite(y0) || !lo_finite(x1) || !lo_finite(y1)) return false;
    out[0] = lo_round(x0, false); out[1] = lo_round(y0, false); out[2] = lo_round(x1, true); out[3] = lo_round(y1, true);
    return out[0] < out[2] && out[1] < out[3];
}
MO_HD inline int64_t lo_overlap(const int32_t *a, const int32_t *b) {            // both exclusive at x1, y1
    const int32_t x0 = a[0] > b[0] ? a[0] : b[0], y0 = a[1] > b[1] ? a[1] : b[1];
    const int32_t x1 = a[2] < b[2] ? a[2] : b[2], y1 = a[3] < b[3] ? a[3] : b[3];
    return x0 < x1 && y0 < y1 ? (int64_t)(x1 - x0) * (y1 - y0) : 0;
}
MO_HD inline bool lo_covered(const int32_t *track, const int32_t *region, int32_t covered_pm) {
    const int64_t area = (int64_t)(region[2] - region[0]) * (region[3] - region[1]);
    return 1000 * lo_overlap(track, region) >= (int64_t)covered_pm * area;
}
MO_HD inline bool lo_attended(const int32_t *track, const int32_t *region, int32_t margin) {
    const int32_t g[4] = {track[0] - margin, track[1] - margin, track[2] + margin, track[3] + margin};
    return lo_overlap(g, region) > 0;
}
// shared cells of two inclusive cell boxes
MO_HD inline int64_t lo_shared_cells(const int32_t *a, const int32_t *b) {
    const int32_t x0 = a[0] > b[0] ? a[0] : b[0], y0 = a[1] > b[1] ? a[1] : b[1];
    const int32_t x1 = a[2] < b[2] ? a[2] : b[2], y1 = a[3] < b[3] ? a[3] : b[3];
    return x0 <= x1 && y0 <= y1 ? (int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) : 0;
}

// ---- one ledger entry on a call that matched (or bore) it --------------------------------------------------------------
struct LoTimer { int32_t idle, kind, alarmed; int64_t owner; };
// covered: by any selected track; covered_report: by one whose class a report class lists.  Returns true when the alarm fires on
// this call.
MO_HD inline bool lo_timer(LoTimer &e, int32_t region_kind, bool attended, int64_t owner, bool covered, bool covered_report, int32_t alarm_frames) {
    if (attended) { e.idle = 0; e.owner = owner; }
    else if (!covered || covered_report) e.idle = e.idle < MO_MAX_SEEN ? e.idle + 1 : e.idle;
    if (!e.alarmed) e.kind = covered_report ? LO_TRACKED_STATIC : region_kind;
    if (!e.alarmed && e.idle >= alarm_frames) { e.alarmed = 1; return true; }
    return false;
}
MO_HD inline bool lo_absorbs(int64_t frame_id, int64_t first_frame, int32_t absorb_frames) {
    return absorb_frames > 0 && frame_id - first_frame >= (int64_t)absorb_frames;
}

}  // namespace rtmodt
