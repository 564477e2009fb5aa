// motion_model.h -- the one statement of the motion detector's per-cell rules (csrc/motion.hip runs them per frame; its header
// states the mask, the regions and the status).  Plain C++, no HIP: the kernels of motion.hip, the host-only entry point
// rtmodt_motion_cell and tests/native/motion_model_check.cpp (built under the address and UB sanitizers) all take them from here, and
// tests/motion_ref.py restates them in NumPy.  Everything is integer arithmetic.
//   Grid.   gw = ceil(w / scale), gh = ceil(h / scale), scale in {1, 2, 4, 8}; cell (cx, cy) covers the pixels cx * scale ..
//           min(cx * scale + scale, w) - 1, likewise in y: edge cells are partial.
//   Luma.   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 per pixel (jpeg.hip's and gmc.hip's Y); a cell's luma is
//           Yc = (sum + cnt / 2) / cnt over its cnt pixels inside the frame.
//   Model.  A cell holds bg and dev, unsigned 8.8 fixed point in 16 bits each; a stream holds frames_seen.
//           frames_seen == 0: bg = Yc << 8, dev = 0, the cell is not raw foreground.  Otherwise d = (Yc << 8) - bg, ad = |d|,
//           raw = frames_seen >= warmup && ad > (threshold << 8) + dev_gain * dev, and
//             bg += d >> s (arithmetic shift of the signed value), s = learn_shift_fg for raw cells (0: no update), else learn_shift;
//             dev += (ad - dev) >> learn_shift for the cells that are not raw.
//           bg stays within 0 .. 255 << 8 and dev within 0 .. 65535: both move towards a value in that range and never past it.
//   Boxes.  Cells cx0..cx1 x cy0..cy1 (inclusive) are the pixels x0 = cx0 * scale .. x1 = min(w, (cx1 + 1) * scale), x1 exclusive.
//   Status. WARMUP if frames_seen < warmup at entry, else SCENE_CHANGE if 1000 * n_raw >= scene_pm * gw * gh, else MOTION if there
//           is a region, else STILL; frames_seen becomes 0 after a SCENE_CHANGE, else min(frames_seen + 1, 2^30).
#pragma once

#include <cstdint>

#ifndef MO_HD
#define MO_HD
#endif

namespace rtmodt {

constexpr int MO_WARMUP = 0, MO_STILL = 1, MO_MOTION = 2, MO_SCENE_CHANGE = 3;
constexpr int MO_MAX_SEEN = 1 << 30, MO_MAX_DIM = 32768, MO_MAX_REGIONS = 256;
constexpr long long MO_MAX_CELLS = 1LL << 24;

struct MoRule { int32_t learn_shift, learn_shift_fg, threshold, dev_gain, warmup; };

MO_HD inline bool mo_scale_ok(int32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }
MO_HD inline bool mo_block_ok(int32_t b) { return b == 4 || b == 8 || b == 16 || b == 32; }
MO_HD inline bool mo_rule_ok(const MoRule &r) {
    return r.learn_shift >= 1 && r.learn_shift <= 8 && (r.learn_shift_fg == 0 || (r.learn_shift_fg >= r.learn_shift && r.learn_shift_fg <= 12)) &&
           r.threshold >= 1 && r.threshold <= 255 && r.dev_gain >= 0 && r.dev_gain <= 8 && r.warmup >= 1 && r.warmup <= 255;
}

MO_HD inline int32_t mo_grid(int32_t px, int32_t scale) { return (px + scale - 1) / scale; }
MO_HD inline uint32_t mo_luma(uint32_t b, uint32_t g, uint32_t r) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }
// the pixels of cell c along one axis of `px` pixels (0 for a cell outside the grid)
MO_HD inline int32_t mo_cell_span(int32_t c, int32_t scale, int32_t px) {
    const int32_t left = px - c * scale;
    return left <= 0 ? 0 : (left < scale ? left : scale);
}
MO_HD inline uint32_t mo_cell_mean(uint32_t sum, uint32_t cnt) { return (sum + cnt / 2) / cnt; }

// one cell of one frame: updates bg / dev (8.8 fixed point, 0..65535) and returns whether the cell is raw foreground
MO_HD inline bool mo_cell(const MoRule &r, uint32_t yc, int32_t frames_seen, uint32_t &bg, uint32_t &dev) {
    const int32_t t = (int32_t)(yc << 8);
    if (frames_seen == 0) {
        bg = (uint32_t)t; dev = 0;
        return false;
    }
    const int32_t d = t - (int32_t)bg, ad = d < 0 ? -d : d;
    const bool raw = frames_seen >= r.warmup && ad > (r.threshold << 8) + r.dev_gain * (int32_t)dev;
    if (!raw) {
        bg = (uint32_t)((int32_t)bg + (d >> r.learn_shift));
        dev = (uint32_t)((int32_t)dev + ((ad - (int32_t)dev) >> r.learn_shift));
    } else if (r.learn_shift_fg) {
        bg = (uint32_t)((int32_t)bg + (d >> r.learn_shift_fg));
    }
    return raw;
}

// cells cx0..cx1 x cy0..cy1 (inclusive) -> the pixel box x0, y0, x1, y1 (x1 and y1 exclusive)
MO_HD inline void mo_px_box(int32_t cx0, int32_t cy0, int32_t cx1, int32_t cy1, int32_t scale, int32_t w, int32_t h, int32_t *out) {
    const int32_t x1 = (cx1 + 1) * scale, y1 = (cy1 + 1) * scale;
    out[0] = cx0 * scale; out[1] = cy0 * scale;
    out[2] = x1 < w ? x1 : w; out[3] = y1 < h ? y1 : h;
}

MO_HD inline int32_t mo_status(int32_t frames_seen, int32_t warmup, uint32_t n_raw, int32_t scene_pm, int64_t cells, uint32_t n_regions_total) {
    if (frames_seen < warmup) return MO_WARMUP;
    if (1000LL * (int64_t)n_raw >= (int64_t)scene_pm * cells) return MO_SCENE_CHANGE;
    return n_regions_total >= 1 ? MO_MOTION : MO_STILL;
}
MO_HD inline int32_t mo_next_seen(int32_t frames_seen, int32_t status) {
    return status == MO_SCENE_CHANGE ? 0 : (frames_seen + 1 < MO_MAX_SEEN ? frames_seen + 1 : MO_MAX_SEEN);
}

}  // namespace rtmodt
