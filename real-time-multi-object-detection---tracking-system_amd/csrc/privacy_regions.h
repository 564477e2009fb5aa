// privacy_regions.h -- the one statement of the privacy masker's region arithmetic: how one float32 box becomes one inclusive
// integer rectangle of the frame (csrc/privacy.hip paints those rectangles; its header states the paint rules).  Plain C++, no
// HIP: the host packer and the device gather of privacy.hip, the host-only entry point rtmodt_privacy_regions and
// tests/native/privacy_regions_check.cpp (built under the address and UB sanitizers) all take it from here, and
// tests/privacy_ref.py restates it in NumPy.  A box becomes a rectangle in five steps:
//   1. corners: int(v), i.e. truncation, of the float32 box clamped to +-2^20 (as the renderer's); x1 < x0 or y1 < y0 after
//      the truncation: no region (skipped, not an error);
//   2. kind: BOX is the whole rectangle; HEAD keeps its top rows y0 .. y0 + max(1, (H * head_pm + 999) / 1000) - 1 with
//      H = y1 - y0 + 1, head_pm 1..1000 per mille, int64 arithmetic;
//   3. expansion: expand_px (0..256) on all four sides;
//   4. clipping to the frame; empty after the clip: no region;
//   5. class filter: an optional list of at most 256 class ids (null: every class); a box whose class is not listed: no region.
// Non-finite coordinates are the caller's business (the host forms refuse them, the device forms skip the box).
#pragma once

#include <cmath>
#include <cstdint>

#ifndef PV_HD
#define PV_HD
#endif

namespace rtmodt {

constexpr int PV_COORD_MAX = 1 << 20, PV_MAX_CLASSES = 256, PV_MAX_EXPAND = 256;
constexpr int PV_REGION_BOX = 0, PV_REGION_HEAD = 1;

struct PvRect { int32_t x0, y0, x1, y1; };              // inclusive
struct PvRegionCfg { int32_t kind, head_pm, expand_px; const int32_t *classes; int32_t n_classes; };

PV_HD inline bool pv_region_cfg_ok(const PvRegionCfg &c) {
    return (c.kind == PV_REGION_BOX || c.kind == PV_REGION_HEAD) && c.head_pm >= 1 && c.head_pm <= 1000 && c.expand_px >= 0 &&
           c.expand_px <= PV_MAX_EXPAND && (!c.classes || (c.n_classes >= 0 && c.n_classes <= PV_MAX_CLASSES));
}

PV_HD inline bool pv_finite(float v) { return v - v == 0.0f; }

PV_HD inline int32_t pv_coord(float v) {
    const float lim = (float)PV_COORD_MAX;
    const float c = v < -lim ? -lim : (v > lim ? lim : v);
    return (int32_t)c;                                   // truncation toward zero
}

PV_HD inline bool pv_class_listed(const PvRegionCfg &c, int32_t cls) {
    if (!c.classes) return true;
    for (int i = 0; i < c.n_classes; ++i)
        if (c.classes[i] == cls) return true;
    return false;
}

// one box (finite) -> its rectangle in an h x w frame; false: no region
PV_HD inline bool pv_region(const PvRegionCfg &c, float bx0, float by0, float bx1, float by1, int32_t cls, int h, int w, PvRect &out) {
    if (!pv_class_listed(c, cls)) return false;
    int32_t x0 = pv_coord(bx0), y0 = pv_coord(by0), x1 = pv_coord(bx1), y1 = pv_coord(by1);
    if (x1 < x0 || y1 < y0) return false;
    if (c.kind == PV_REGION_HEAD) {
        const int64_t H = (int64_t)y1 - y0 + 1;
        int64_t rows = (H * c.head_pm + 999) / 1000;
        if (rows < 1) rows = 1;
        y1 = (int32_t)(y0 + rows - 1);
    }
    x0 -= c.expand_px; y0 -= c.expand_px; x1 += c.expand_px; y1 += c.expand_px;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > w - 1) x1 = w - 1;
    if (y1 > h - 1) y1 = h - 1;
    if (x1 < x0 || y1 < y0) return false;
    out.x0 = x0; out.y0 = y0; out.x1 = x1; out.y1 = y1;
    return true;
}

}  // namespace rtmodt
