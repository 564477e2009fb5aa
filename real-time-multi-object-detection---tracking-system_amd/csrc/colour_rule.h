// colour_rule.h -- the one statement of the colour attributes' arithmetic: the name of a pixel, which rectangle of the frame a box is
// sampled in and on which grid, which part of the box a row belongs to, which other boxes of the list hide it, how a frame's
// counts enter a track's row, how a row ages and how a part's label is read off its counts (csrc/colour.hip keeps the ledger and
// runs the sampler; its header states the ledger rules).  Plain C++, no HIP: the kernels of colour.hip, the host-only entry points
// rtmodt_colour_name / rtmodt_colour_plan and tests/native/colour_rule_check.cpp (built under the address and UB sanitizers) all
// take it from here, and tests/colour_ref.py restates it in NumPy.  Integer arithmetic throughout, after the corners.
//   1. NAME of (b, g, r): mx = max, mn = min, c = mx - mn, y = mo_luma(b, g, r) (motion_model.h).  In this order:
//        mx < black_max                                                                  BLACK
//        c < chroma_min, or c * 1000 <= sat * mx (sat = sat_hi_pm for mx >= sat_split, else sat_lo_pm)     achromatic:
//                                                        y < y_black BLACK, y >= y_white WHITE, else GREY
//        hue on a 1536-step hexcone; the first channel equal to mx, asked in the order r, g, b, decides:
//        r: floor((g - b) * 256 / c), g: 512 + floor((b - r) * 256 / c), b: 1024 + floor((r - g) * 256 / c), mod 1536 (a TRUE
//        floor: cl_floor_div).  Then, with h[0..7] = the eight hue bounds (64 192 299 725 853 1109 1344 1472):
//        h < h[0] or h >= h[7]   PINK when 2 c < mx and mx >= pink_mx; else BROWN when mx < red_brown_mx; else RED
//        h[0] <= h < h[1]        BROWN when mx < orange_brown_mx, else ORANGE
//        h[1] <= h < h[2]        BROWN when mx < yellow_brown_mx, else YELLOW
//        .. h[3] GREEN, .. h[4] CYAN, .. h[5] BLUE, .. h[6] PURPLE, .. h[7] PINK
//   2. RECTANGLE: corners by privacy_regions.h's rule (pv_coord), the inclusive RAW rectangle, W x H; a non-finite coordinate,
//      x1 < x0 or y1 < y0, or a class outside the filter: not sampled (no row).  Columns x0 + W inset_x_pm / 1000 ..
//      x1 - W inset_x_pm / 1000, rows y0 + H top_pm / 1000 .. y0 + H bottom_pm / 1000 - 1, the split row ys = y0 + H split_pm / 1000:
//      rows < ys are UPPER, the rest LOWER (int64, floor).  Then clipped to the frame; empty: zero samples, no error.
//   3. GRID over the clipped Sw x Sh: sx = max(1, ceil(Sw / max_side)), sy likewise; samples at (cx0 + i sx, cy0 + j sy).
//   4. OCCLUDERS of entry i: the other sampled entries k of the list with (y1_k, id_k) > (y1_i, id_i) (raw bottom edge, then id)
//      whose frame-clipped RAW rectangle meets i's clipped sampled rectangle; the first CL_MAX_OCCLUDERS in list order are used,
//      more set CL_F_MANY_OCCLUDERS.  A sample inside a used occluder's clipped RAW rectangle is skipped.
//   5. ROW: a frame's counts are added when they hold at least min_samples samples over both parts (else CL_F_THIN); after the add
//      a part whose total exceeds CL_AGE_LIMIT = 2^24 has every bin halved (floor).
//   6. LABEL of a part: the largest bin (ties: the lower index), share_pm = count * 1000 / total; the second likewise among the
//      other bins (-1 when its count is 0); total == 0: name -1.  WHOLE is the bin-wise sum of UPPER and LOWER.
#pragma once

#include <cstdint>

#include "privacy_regions.h"

#ifndef MO_HD
#define MO_HD PV_HD
#endif
#include "motion_model.h"

#ifndef CL_HD
#define CL_HD PV_HD
#endif

namespace rtmodt {

constexpr int CL_NAMES = 12, CL_PARTS = 2, CL_BINS = CL_PARTS * CL_NAMES, CL_MAX_OCCLUDERS = 8, CL_MAX_SIDE = 256, CL_MAX_CLASSES = 256, CL_MAX_DIM = 16384;
constexpr int CL_HUE_STEPS = 1536, CL_HUE_BOUNDS = 8;
constexpr uint32_t CL_AGE_LIMIT = 1u << 24;
constexpr int CL_BLACK = 0, CL_GREY = 1, CL_WHITE = 2, CL_RED = 3, CL_ORANGE = 4, CL_YELLOW = 5, CL_GREEN = 6, CL_CYAN = 7, CL_BLUE = 8, CL_PURPLE = 9,
              CL_PINK = 10, CL_BROWN = 11;
constexpr int CL_UPPER = 0, CL_LOWER = 1, CL_WHOLE = 2;
constexpr int CL_F_NEW = 1, CL_F_MANY_OCCLUDERS = 2, CL_F_THIN = 4;

struct ClRuleCfg {
    int32_t black_max, chroma_min, sat_split, sat_hi_pm, sat_lo_pm, y_black, y_white;
    int32_t hue[CL_HUE_BOUNDS];
    int32_t pink_mx, red_brown_mx, orange_brown_mx, yellow_brown_mx;
    int32_t inset_x_pm, top_pm, split_pm, bottom_pm, max_side, skip_occluded, min_samples;
    const int32_t *classes; int32_t n_classes;      // classes == nullptr: every class
};

struct ClPlan {
    PvRect raw;                // 2. inclusive, not clipped
    PvRect box;                // raw clipped to the frame; empty when box.x1 < box.x0 or box.y1 < box.y0
    PvRect rect;               // the clipped sampled rectangle; empty likewise
    int32_t ys;                // the split row (of the unclipped rectangle)
    int32_t sx, sy, nx, ny;    // 3. strides and sample counts; nx = ny = 0 when rect is empty
};

struct ClLabel { int32_t name, share_pm, second, second_pm, samples; };

CL_HD inline bool cl_rule_cfg_ok(const ClRuleCfg &c) {
    bool ok = c.black_max >= 0 && c.black_max <= 256 && c.chroma_min >= 0 && c.chroma_min <= 256 && c.sat_split >= 0 && c.sat_split <= 256 &&
              c.sat_hi_pm >= 0 && c.sat_hi_pm <= 1000 && c.sat_lo_pm >= 0 && c.sat_lo_pm <= 1000 && c.y_black >= 0 && c.y_black <= c.y_white && c.y_white <= 256;
    for (int k = 0; k < CL_HUE_BOUNDS; ++k) ok = ok && c.hue[k] >= (k ? c.hue[k - 1] : 0) && c.hue[k] <= CL_HUE_STEPS;
    ok = ok && c.pink_mx >= 0 && c.pink_mx <= 256 && c.red_brown_mx >= 0 && c.red_brown_mx <= 256 && c.orange_brown_mx >= 0 && c.orange_brown_mx <= 256 &&
         c.yellow_brown_mx >= 0 && c.yellow_brown_mx <= 256;
    ok = ok && c.inset_x_pm >= 0 && c.inset_x_pm <= 499 && c.top_pm >= 0 && c.top_pm < c.split_pm && c.split_pm < c.bottom_pm && c.bottom_pm <= 1000;
    ok = ok && c.max_side >= 1 && c.max_side <= CL_MAX_SIDE && (c.skip_occluded == 0 || c.skip_occluded == 1) && c.min_samples >= 0 &&
         c.min_samples <= CL_MAX_SIDE * CL_MAX_SIDE;
    return ok && (!c.classes || (c.n_classes >= 0 && c.n_classes <= CL_MAX_CLASSES));
}

// floor(a / b) for b > 0 (C++'s `/` truncates toward zero)
CL_HD inline int32_t cl_floor_div(int32_t a, int32_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// 1. the hue of a chromatic pixel (c = mx - mn > 0), 0 .. 1535
CL_HD inline int32_t cl_hue(int32_t b, int32_t g, int32_t r, int32_t mx, int32_t c) {
    int32_t h;
    if (r == mx) h = cl_floor_div((g - b) * 256, c);
    else if (g == mx) h = 512 + cl_floor_div((b - r) * 256, c);
    else h = 1024 + cl_floor_div((r - g) * 256, c);
    h %= CL_HUE_STEPS;
    return h < 0 ? h + CL_HUE_STEPS : h;
}

CL_HD inline int32_t cl_name(const ClRuleCfg &k, uint32_t b, uint32_t g, uint32_t r) {
    const int32_t ib = (int32_t)b, ig = (int32_t)g, ir = (int32_t)r;
    const int32_t mx = ib > ig ? (ib > ir ? ib : ir) : (ig > ir ? ig : ir), mn = ib < ig ? (ib < ir ? ib : ir) : (ig < ir ? ig : ir), c = mx - mn;
    if (mx < k.black_max) return CL_BLACK;
    const int32_t sat = mx >= k.sat_split ? k.sat_hi_pm : k.sat_lo_pm;
    if (c < k.chroma_min || c * 1000 <= sat * mx) {
        const int32_t y = (int32_t)mo_luma(b, g, r);
        return y < k.y_black ? CL_BLACK : (y >= k.y_white ? CL_WHITE : CL_GREY);
    }
    if (c <= 0) return CL_GREY;                      // (chroma_min == 0 and sat == 0 with a grey pixel: no hue to speak of)
    const int32_t h = cl_hue(ib, ig, ir, mx, c);
    if (h < k.hue[0] || h >= k.hue[7]) return 2 * c < mx && mx >= k.pink_mx ? CL_PINK : (mx < k.red_brown_mx ? CL_BROWN : CL_RED);
    if (h < k.hue[1]) return mx < k.orange_brown_mx ? CL_BROWN : CL_ORANGE;
    if (h < k.hue[2]) return mx < k.yellow_brown_mx ? CL_BROWN : CL_YELLOW;
    if (h < k.hue[3]) return CL_GREEN;
    if (h < k.hue[4]) return CL_CYAN;
    if (h < k.hue[5]) return CL_BLUE;
    if (h < k.hue[6]) return CL_PURPLE;
    return CL_PINK;
}

CL_HD inline bool cl_class_listed(const ClRuleCfg &c, int32_t cls) {
    if (!c.classes) return true;
    for (int i = 0; i < c.n_classes; ++i)
        if (c.classes[i] == cls) return true;
    return false;
}

CL_HD inline bool cl_empty(const PvRect &r) { return r.x1 < r.x0 || r.y1 < r.y0; }
CL_HD inline bool cl_meet(const PvRect &a, const PvRect &b) {
    return !cl_empty(a) && !cl_empty(b) && a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1;
}
CL_HD inline bool cl_inside(const PvRect &r, int32_t x, int32_t y) { return x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1; }
CL_HD inline int32_t cl_max(int32_t a, int32_t b) { return a > b ? a : b; }
CL_HD inline int32_t cl_min(int32_t a, int32_t b) { return a < b ? a : b; }

// 2. + 3. one box in an h x w frame -> its plan; false: not sampled (the entry takes no row; nothing of `out` is meaningful)
CL_HD inline bool cl_plan(const ClRuleCfg &c, float bx0, float by0, float bx1, float by1, int32_t cls, int h, int w, ClPlan &out) {
    if (!cl_class_listed(c, cls)) return false;
    if (!(pv_finite(bx0) && pv_finite(by0) && pv_finite(bx1) && pv_finite(by1))) return false;
    const int32_t x0 = pv_coord(bx0), y0 = pv_coord(by0), x1 = pv_coord(bx1), y1 = pv_coord(by1);
    if (x1 < x0 || y1 < y0) return false;
    const int64_t W = (int64_t)x1 - x0 + 1, H = (int64_t)y1 - y0 + 1;
    const int32_t in = (int32_t)(W * c.inset_x_pm / 1000);
    const int32_t ra = y0 + (int32_t)(H * c.top_pm / 1000), rb = y0 + (int32_t)(H * c.bottom_pm / 1000) - 1;
    out.raw = PvRect{x0, y0, x1, y1};
    out.box = PvRect{cl_max(x0, 0), cl_max(y0, 0), cl_min(x1, w - 1), cl_min(y1, h - 1)};
    out.rect = PvRect{cl_max(x0 + in, 0), cl_max(ra, 0), cl_min(x1 - in, w - 1), cl_min(rb, h - 1)};
    out.ys = y0 + (int32_t)(H * c.split_pm / 1000);
    out.sx = out.sy = 1; out.nx = out.ny = 0;
    if (cl_empty(out.rect)) return true;
    const int32_t sw = out.rect.x1 - out.rect.x0 + 1, sh = out.rect.y1 - out.rect.y0 + 1;
    out.sx = cl_max(1, (sw + c.max_side - 1) / c.max_side);
    out.sy = cl_max(1, (sh + c.max_side - 1) / c.max_side);
    out.nx = (sw + out.sx - 1) / out.sx;
    out.ny = (sh + out.sy - 1) / out.sy;
    return true;
}

CL_HD inline int32_t cl_part(const ClPlan &p, int32_t y) { return y < p.ys ? CL_UPPER : CL_LOWER; }

// 4. does entry k (raw bottom edge y1_k, id_k, clipped RAW rectangle box_k) hide part of entry i's sampled rectangle?
CL_HD inline bool cl_occludes(const ClPlan &mine, int64_t my_id, const PvRect &raw_k, const PvRect &box_k, int64_t id_k) {
    const bool nearer = raw_k.y1 > mine.raw.y1 || (raw_k.y1 == mine.raw.y1 && id_k > my_id);
    return nearer && cl_meet(box_k, mine.rect);
}

// 5. a frame's counts into a row's; returns whether they were added
CL_HD inline bool cl_accumulate(uint32_t *row, const uint32_t *frame, int32_t min_samples) {
    uint32_t n = 0;
    for (int k = 0; k < CL_BINS; ++k) n += frame[k];
    if (n < (uint32_t)min_samples) return false;
    for (int p = 0; p < CL_PARTS; ++p) {
        uint32_t tot = 0;
        for (int k = 0; k < CL_NAMES; ++k) { row[p * CL_NAMES + k] += frame[p * CL_NAMES + k]; tot += row[p * CL_NAMES + k]; }
        if (tot > CL_AGE_LIMIT)
            for (int k = 0; k < CL_NAMES; ++k) row[p * CL_NAMES + k] >>= 1;
    }
    return true;
}

// 6. the label of part `part` (CL_UPPER, CL_LOWER, CL_WHOLE) of a row
CL_HD inline ClLabel cl_label(const uint32_t *row, int part) {
    uint64_t v[CL_NAMES], tot = 0;
    for (int k = 0; k < CL_NAMES; ++k) {
        v[k] = part == CL_WHOLE ? (uint64_t)row[k] + row[CL_NAMES + k] : row[part * CL_NAMES + k];
        tot += v[k];
    }
    ClLabel L{-1, 0, -1, 0, (int32_t)tot};
    if (tot == 0) return L;
    int a = 0, s = -1;                               // (no array is indexed by a value found at run time: the loops unroll into registers)
    uint64_t va = v[0], vs = 0;
    for (int k = 1; k < CL_NAMES; ++k)
        if (v[k] > va) { va = v[k]; a = k; }
    for (int k = 0; k < CL_NAMES; ++k)
        if (k != a && v[k] > vs) { vs = v[k]; s = k; }
    L.name = a; L.share_pm = (int32_t)(va * 1000 / tot);
    if (s >= 0) { L.second = s; L.second_pm = (int32_t)(vs * 1000 / tot); }
    return L;
}

}  // namespace rtmodt
