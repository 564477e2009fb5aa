// snapshot_rule.h -- the one statement of the snapshot gallery's per-box arithmetic: which rectangle of the frame a box's thumbnail
// is cut from, how that crop is fitted into the thumbnail slot, the weights of the exact area average that shrinks it, the score
// of a shot and when a better shot replaces the one kept (csrc/snapshot.hip keeps the ledger and runs the resampler; its header
// states the ledger rules).  Plain C++, no HIP: the kernels of snapshot.hip, the host-only entry point rtmodt_snapshot_plan and
// tests/native/snapshot_rule_check.cpp (built under the address and UB sanitizers) all take it from here, and
// tests/snapshot_ref.py restates it in NumPy.  Integer arithmetic throughout, but for ONE float32 multiply (the confidence).
//   1. corners: privacy_regions.h's rule (pv_coord: truncation of the float32 box clamped to +-2^20); this is the RAW rectangle,
//      inclusive; x1 < x0 or y1 < y0, a non-finite coordinate, or a class outside the filter: not sampled;
//   2. margin: the raw rectangle grows by floor(W * margin_pm / 1000) columns left and right and floor(H * margin_pm / 1000) rows
//      above and below, W x H its own size;
//   3. the grown rectangle clipped to the frame is the CROP, Sw x Sh; fewer than min_side pixels on either side: not sampled;
//      the raw rectangle clipped to the frame is the BOX (it may be empty when only the margin reaches into the frame);
//   4. THE FIT, never enlarging: Sw <= Tw and Sh <= Th: Dw x Dh = Sw x Sh (a 1:1 copy).  Otherwise the axis that is relatively
//      longer fills the slot and the other is rounded to nearest, at least 1: if Sw * Th >= Sh * Tw then Dw = Tw,
//      Dh = max(1, (Sh * Tw + Sw / 2) / Sw), else Dh = Th, Dw = max(1, (Sw * Th + Sh / 2) / Sh).  The image stands at
//      ox = (Tw - Dw) / 2, oy = (Th - Dh) / 2 of the slot; every other pixel of the slot is pad_bgr;
//   5. resample, per axis with S source and D <= S destination pixels: in units that give a source pixel the length D,
//      destination pixel j covers [j S, (j + 1) S); the weight of source pixel i is the overlap of that with [i D, (i + 1) D), so
//      the weights of j sum to S.  A pixel is (sum(wy wx p) + tot / 2) / tot, tot = Sw * Sh, in 64 bits: one rounding;
//   6. score = conf_milli * min(area of the BOX, area_cap), halved once when the shot is CUT (the raw rectangle reaches the frame
//      border) and once when it is OCCLUDED (another sampled BOX of the list with inter * 1000 > occl_iou_pm * union);
//   7. a kept shot is replaced iff score * 1000 > best_score * (1000 + min_gain_pm).
#pragma once

#include <cstdint>

#include "privacy_regions.h"

#ifndef SN_HD
#define SN_HD PV_HD
#endif

namespace rtmodt {

constexpr int SN_MIN_THUMB = 8, SN_MAX_THUMB = 512, SN_MAX_CLASSES = 256, SN_MAX_DIM = 16384;
constexpr int SN_F_NEW = 1, SN_F_REWRITTEN = 2, SN_F_CUT = 4, SN_F_OCCLUDED = 8;

struct SnRuleCfg {
    int32_t thumb_h, thumb_w, margin_pm, min_side, area_cap, occl_iou_pm, min_gain_pm;
    const int32_t *classes; int32_t n_classes;      // classes == nullptr: every class
};

struct SnPlan {
    PvRect raw;                // 1. inclusive, neither grown nor clipped
    PvRect box;                // 3. raw clipped to the frame; empty when box.x1 < box.x0 or box.y1 < box.y0
    PvRect crop;               // 3. grown and clipped, never empty
    int32_t sw, sh;            // the crop's size
    int32_t dw, dh, ox, oy;    // 4. the image inside the slot
    int32_t cut, area;         // 6. raw reaches the frame border; min(area of box, area_cap)
};

SN_HD inline bool sn_rule_cfg_ok(const SnRuleCfg &c) {
    return c.thumb_h >= SN_MIN_THUMB && c.thumb_h <= SN_MAX_THUMB && c.thumb_w >= SN_MIN_THUMB && c.thumb_w <= SN_MAX_THUMB && c.margin_pm >= 0 &&
           c.margin_pm <= 1000 && c.min_side >= 1 && c.area_cap >= 1 && c.area_cap <= (1 << 28) && c.occl_iou_pm >= 0 && c.occl_iou_pm <= 1000 &&
           c.min_gain_pm >= 0 && c.min_gain_pm <= 10000 && (!c.classes || (c.n_classes >= 0 && c.n_classes <= SN_MAX_CLASSES));
}

SN_HD inline bool sn_class_listed(const SnRuleCfg &c, int32_t cls) {
    if (!c.classes) return true;
    for (int i = 0; i < c.n_classes; ++i)
        if (c.classes[i] == cls) return true;
    return false;
}

SN_HD inline int32_t sn_lo(int32_t v) { return v < 0 ? 0 : v; }
SN_HD inline int32_t sn_hi(int32_t v, int32_t m) { return v > m ? m : v; }

// one box in an h x w frame -> its plan; false: not sampled (nothing of `out` is meaningful then)
SN_HD inline bool sn_plan(const SnRuleCfg &c, float bx0, float by0, float bx1, float by1, int32_t cls, int h, int w, SnPlan &out) {
    if (!sn_class_listed(c, cls)) return false;
    if (!(pv_finite(bx0) && pv_finite(by0) && pv_finite(bx1) && pv_finite(by1))) return false;
    const int32_t x0 = pv_coord(bx0), y0 = pv_coord(by0), x1 = pv_coord(bx1), y1 = pv_coord(by1);
    if (x1 < x0 || y1 < y0) return false;
    const int64_t W = (int64_t)x1 - x0 + 1, H = (int64_t)y1 - y0 + 1;
    const int32_t mx = (int32_t)(W * c.margin_pm / 1000), my = (int32_t)(H * c.margin_pm / 1000);
    out.raw = PvRect{x0, y0, x1, y1};
    out.box = PvRect{sn_lo(x0), sn_lo(y0), sn_hi(x1, w - 1), sn_hi(y1, h - 1)};
    out.crop = PvRect{sn_lo(x0 - mx), sn_lo(y0 - my), sn_hi(x1 + mx, w - 1), sn_hi(y1 + my, h - 1)};
    if (out.crop.x1 < out.crop.x0 || out.crop.y1 < out.crop.y0) return false;
    const int32_t sw = out.crop.x1 - out.crop.x0 + 1, sh = out.crop.y1 - out.crop.y0 + 1;
    if (sw < c.min_side || sh < c.min_side) return false;
    const int32_t tw = c.thumb_w, th = c.thumb_h;
    int32_t dw = sw, dh = sh;
    if (sw > tw || sh > th) {
        if ((int64_t)sw * th >= (int64_t)sh * tw) {
            dw = tw;
            dh = (int32_t)(((int64_t)sh * tw + sw / 2) / sw);
            if (dh < 1) dh = 1;
        } else {
            dh = th;
            dw = (int32_t)(((int64_t)sw * th + sh / 2) / sh);
            if (dw < 1) dw = 1;
        }
    }
    out.sw = sw; out.sh = sh; out.dw = dw; out.dh = dh; out.ox = (tw - dw) / 2; out.oy = (th - dh) / 2;
    out.cut = x0 <= 0 || y0 <= 0 || x1 >= w - 1 || y1 >= h - 1 ? 1 : 0;
    int64_t area = 0;
    if (out.box.x1 >= out.box.x0 && out.box.y1 >= out.box.y0) area = (int64_t)(out.box.x1 - out.box.x0 + 1) * (out.box.y1 - out.box.y0 + 1);
    out.area = (int32_t)(area > c.area_cap ? c.area_cap : area);
    return true;
}

// 5. the source pixels i0 .. i1 that destination pixel j of an axis (S source, D <= S destination pixels) covers
SN_HD inline void sn_span(int32_t S, int32_t D, int32_t j, int32_t &i0, int32_t &i1) {
    i0 = (int32_t)((int64_t)j * S / D);
    i1 = (int32_t)((((int64_t)j + 1) * S - 1) / D);
}
// ... and the weight of source pixel i of that span
SN_HD inline int32_t sn_weight(int32_t S, int32_t D, int32_t j, int32_t i) {
    const int64_t a0 = (int64_t)j * S, a1 = a0 + S, b0 = (int64_t)i * D, b1 = b0 + D;
    return (int32_t)((a1 < b1 ? a1 : b1) - (a0 > b0 ? a0 : b0));
}

// 6. the confidence in thousandths: ONE float32 multiply, truncated, NaN -> 0, clamped to 0..1000
SN_HD inline int32_t sn_conf_milli(float conf) {
    const float m = conf * 1000.0f;
    if (!(m > 0.0f)) return 0;                      // NaN, zero and negatives
    if (m >= 1000.0f) return 1000;
    return (int32_t)m;
}

// do two BOXes occlude one another?  (empty rectangles never do; pm == 0: the test is off)
SN_HD inline bool sn_occludes(const PvRect &a, const PvRect &b, int32_t occl_iou_pm) {
    if (occl_iou_pm <= 0) return false;
    if (a.x1 < a.x0 || a.y1 < a.y0 || b.x1 < b.x0 || b.y1 < b.y0) return false;
    const int32_t ix0 = a.x0 > b.x0 ? a.x0 : b.x0, iy0 = a.y0 > b.y0 ? a.y0 : b.y0;
    const int32_t ix1 = a.x1 < b.x1 ? a.x1 : b.x1, iy1 = a.y1 < b.y1 ? a.y1 : b.y1;
    if (ix1 < ix0 || iy1 < iy0) return false;
    const int64_t inter = (int64_t)(ix1 - ix0 + 1) * (iy1 - iy0 + 1);
    const int64_t uni = (int64_t)(a.x1 - a.x0 + 1) * (a.y1 - a.y0 + 1) + (int64_t)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1) - inter;
    return inter * 1000 > (int64_t)occl_iou_pm * uni;
}

SN_HD inline int64_t sn_score(int32_t conf_milli, int32_t area, bool cut, bool occluded) {
    int64_t s = (int64_t)conf_milli * area;
    if (cut) s >>= 1;
    if (occluded) s >>= 1;
    return s;
}

// 7.
SN_HD inline bool sn_replaces(int64_t score, int64_t best_score, int32_t min_gain_pm) { return score * 1000 > best_score * (1000 + (int64_t)min_gain_pm); }

// one pixel channel of the image: destination (dx, dy) of a dw x dh image cut from the sw x sh crop whose first byte is `src`
// (rows `pitch` bytes apart, BGR24); the reference form of the average (the kernel sums the same terms in another order)
SN_HD inline uint8_t sn_pixel(const uint8_t *src, int64_t pitch, int32_t sw, int32_t sh, int32_t dw, int32_t dh, int32_t dx, int32_t dy, int32_t ch) {
    int32_t x0, x1, y0, y1;
    sn_span(sw, dw, dx, x0, x1);
    sn_span(sh, dh, dy, y0, y1);
    int64_t acc = 0;
    for (int32_t y = y0; y <= y1; ++y) {
        int64_t row = 0;
        for (int32_t x = x0; x <= x1; ++x) row += (int64_t)sn_weight(sw, dw, dx, x) * src[y * pitch + 3 * (int64_t)x + ch];
        acc += row * sn_weight(sh, dh, dy, y);
    }
    const int64_t tot = (int64_t)sw * sh;
    return (uint8_t)((acc + tot / 2) / tot);
}

}  // namespace rtmodt
