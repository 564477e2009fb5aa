// heatmap_stamp.h -- the one statement of the occupancy heatmap's footprint rule: which cells of the grid one float32 box stamps
// (csrc/heatmap.hip accumulates those footprints; its header states the accumulate, overlay and zone-sum rules).  Plain C++, no
// HIP: the host packer and the device gather of heatmap.hip, the host-only entry point rtmodt_heatmap_footprint and
// tests/native/heatmap_stamp_check.cpp (built under the address and UB sanitizers) all take it from here, and
// tests/heatmap_ref.py restates it in NumPy.  The corners and the class filter are those of privacy_regions.h (pv_coord,
// pv_class_listed).  The grid has ceil(h / cell) x ceil(w / cell) cells, cell in {1, 2, 4, 8, 16}; cell (cx, cy) covers the pixels
// cx * cell .. min(cx * cell + cell - 1, w - 1), likewise in y.  A box becomes a stamp in four steps:
//   1. class filter, then X0, Y0, X1, Y1 = pv_coord of the box; X1 < X0 or Y1 < Y0: no footprint;
//   2. the candidate pixels: BOX and DISC the rectangle, FOOT the square [cxp - r, cxp + r] x [Y1 - r, Y1 + r] with
//      cxp = floor((X0 + X1) / 2), r = foot_radius (0..256); clipped to the frame; empty: no footprint.  The candidate cells are
//      those holding a candidate pixel: x0 / cell .. x1 / cell by y0 / cell .. y1 / cell;
//   3. the distance test, int64 on doubled coordinates, the centre of cell cx at ux = 2 cx cell + cell - 1 (uy likewise): a
//      candidate cell is covered when (ux - sx)^2 + (uy - sy)^2 <= d^2 with
//        DISC (Ultralytics' circular stamp): (sx, sy) = (X0 + X1, Y0 + Y1), d = min(X1 - X0, Y1 - Y0) + 1;
//        FOOT (the ground-contact point):    (sx, sy) = (X0 + X1, 2 Y1),    d = 2 r + 1;
//        BOX: no test, every candidate cell is covered;
//   4. the centre pixel: DISC (floor((X0 + X1) / 2), floor((Y0 + Y1) / 2)), FOOT (cxp, Y1); if it lies in the frame its cell is
//      covered whatever the distance test says (a box smaller than a cell still leaves its mark).  It is a candidate pixel, so
//      its cell lies in the candidate range.
// A footprint covers a cell at most once.  Non-finite coordinates are the caller's business (the host forms refuse them, the
// device forms skip the box).
#pragma once

#include "privacy_regions.h"

namespace rtmodt {

constexpr int HM_BOX = 0, HM_DISC = 1, HM_FOOT = 2;
constexpr int HM_MAX_FOOT_RADIUS = 256, HM_MAX_DIM = 32768;

// the candidate cells cx0..cx1 x cy0..cy1 (inclusive), the doubled centre, d (< 0: no distance test), the centre pixel's cell (-1: none)
struct HmStamp { int32_t cx0, cy0, cx1, cy1, sx, sy, d, pcx, pcy, pad; };
struct HmStampCfg { int32_t kind, foot_radius, cell; const int32_t *classes; int32_t n_classes; };

PV_HD inline bool hm_cell_ok(int32_t cell) { return cell == 1 || cell == 2 || cell == 4 || cell == 8 || cell == 16; }

PV_HD inline bool hm_stamp_cfg_ok(const HmStampCfg &c) {
    return (c.kind == HM_BOX || c.kind == HM_DISC || c.kind == HM_FOOT) && c.foot_radius >= 0 && c.foot_radius <= HM_MAX_FOOT_RADIUS &&
           hm_cell_ok(c.cell) && (!c.classes || (c.n_classes >= 0 && c.n_classes <= PV_MAX_CLASSES));
}

PV_HD inline int32_t hm_floor_half(int32_t v) { return (v - (v < 0 ? 1 : 0)) / 2; }

// one box (finite) -> its stamp on the grid of an h x w frame; false: no footprint
PV_HD inline bool hm_stamp(const HmStampCfg &c, float bx0, float by0, float bx1, float by1, int32_t cls, int h, int w, HmStamp &out) {
    if (!pv_class_listed(PvRegionCfg{PV_REGION_BOX, 1000, 0, c.classes, c.n_classes}, cls)) return false;
    const int32_t X0 = pv_coord(bx0), Y0 = pv_coord(by0), X1 = pv_coord(bx1), Y1 = pv_coord(by1);
    if (X1 < X0 || Y1 < Y0) return false;
    int32_t x0 = X0, y0 = Y0, x1 = X1, y1 = Y1, px = -1, py = -1;
    out.sx = out.sy = 0;
    out.d = -1;
    if (c.kind == HM_DISC) {
        out.sx = X0 + X1; out.sy = Y0 + Y1;
        out.d = (X1 - X0 < Y1 - Y0 ? X1 - X0 : Y1 - Y0) + 1;
        px = hm_floor_half(X0 + X1); py = hm_floor_half(Y0 + Y1);
    } else if (c.kind == HM_FOOT) {
        const int32_t r = c.foot_radius;
        px = hm_floor_half(X0 + X1); py = Y1;
        x0 = px - r; x1 = px + r; y0 = py - r; y1 = py + r;
        out.sx = X0 + X1; out.sy = 2 * Y1;
        out.d = 2 * r + 1;
    }
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > w - 1) x1 = w - 1;
    if (y1 > h - 1) y1 = h - 1;
    if (x1 < x0 || y1 < y0) return false;
    out.cx0 = x0 / c.cell; out.cy0 = y0 / c.cell; out.cx1 = x1 / c.cell; out.cy1 = y1 / c.cell;
    out.pcx = out.pcy = -1;
    if (c.kind != HM_BOX && px >= 0 && px < w && py >= 0 && py < h) { out.pcx = px / c.cell; out.pcy = py / c.cell; }
    out.pad = 0;
    return true;
}

// does the stamp cover cell (cx, cy) of a grid of `cell`-pixel cells?
PV_HD inline bool hm_covers(const HmStamp &s, int32_t cell, int32_t cx, int32_t cy) {
    if (cx < s.cx0 || cx > s.cx1 || cy < s.cy0 || cy > s.cy1) return false;
    if (s.d < 0 || (cx == s.pcx && cy == s.pcy)) return true;
    const int64_t dx = 2 * (int64_t)cx * cell + cell - 1 - s.sx, dy = 2 * (int64_t)cy * cell + cell - 1 - s.sy;
    return dx * dx + dy * dy <= (int64_t)s.d * s.d;
}

}  // namespace rtmodt
