// enhance_rule.h -- the one statement of the frame enhancer's rules (csrc/enhance.hip runs them per frame): contrast-limited adaptive
// histogram equalisation of the luma, with the tone curves held per stream and moved by an integer EMA.  Plain C++, no HIP: the
// kernels of enhance.hip, the host-only entry points rtmodt_enhance_curve / rtmodt_enhance_axis and
// tests/native/enhance_rule_check.cpp (built under the address and UB sanitizers) all take them from here, and tests/enhance_ref.py
// restates them in NumPy.  Everything is integer arithmetic.
//   Tiles.   ty x tx tiles, 1..16 each way and no more than the pixels; tile column k covers the pixels [k * w / tx, (k + 1) * w / tx)
//            (floor), rows likewise: tiles are not padded, differ in size by at most one, and a tile's area n is its own.
//   Luma.    mo_luma of motion_model.h, read by cell_grid.h's reader.  A tile's histogram: 256 counts of the luma of its pixels.
//   Curve.   clip_q8 > 0: clip = max(1, (clip_q8 * n) >> 16); excess = sum(max(0, hist - clip)); hist = min(hist, clip); every bin
//            gains excess / 256, and with res = excess % 256, step = max(256 / res, 1), bin i gains 1 more exactly when
//            i % step == 0 && i / step < res (OpenCV's serial residual loop in closed form: res bins, the total stays n).
//            curve[v] = (cdf[v] * 255 + n / 2) / n over the inclusive prefix sum, in 64 bits.  cdf[255] == n, curve[255] == 255.
//   State.   s, unsigned 8.8 in 16 bits per (stream, tile, level), and frames_seen per stream.  frames_seen == 0: s = curve << 8.
//            Else d = (curve << 8) - s and s += d >= 0 ? d >> shift : -((-d) >> shift).  lut8 = min(255, (s + 128) >> 8), after.
//   Axis.    c2[k] = b[k] + b[k + 1] - 1 is twice the centre of tile k.  Pixel x, p = 2x: one tile or p <= c2[0] -> (0, 0);
//            p >= c2[t - 1] -> (t - 1, 0); else k is the last tile with c2[k] <= p and f = ((p - c2[k]) * 256 + den / 2) / den,
//            den = c2[k + 1] - c2[k], so 0 <= f <= 256.  The neighbour is min(k + 1, t - 1).
//   Pixel.   Y1 = ((256 - fy) * ((256 - fx) * A + fx * B) + fy * ((256 - fx) * C + fx * D) + 32768) >> 16 over the lut8[Y] of the four
//            tiles; Y2 = Y + floor(((Y1 - Y) * eff + 128) / 256); SHIFT: c + (Y2 - Y) clamped; GAIN: Y == 0 -> c + Y2 clamped, else
//            min(255, (c * Y2 + Y / 2) / Y).  eff == 0 gives Y2 == Y and the input bytes under both colour rules.
//   Strength. auto_hi > auto_lo: m = sum(v * count) / (h * w) (floor) and eff = strength * clamp(auto_hi - m, 0, auto_hi - auto_lo) /
//            (auto_hi - auto_lo); else eff = strength.
#pragma once

#include "cell_grid.h"

namespace rtmodt {

constexpr int EN_MAX_DIM = 16384, EN_MAX_TILES = 16, EN_LEVELS = 256, EN_MAX_SHIFT = 7, EN_MAX_STRENGTH = 256, EN_MAX_CLIP_Q8 = 1 << 16;
constexpr int EN_SHIFT = 0, EN_GAIN = 1, EN_MAX_SEEN = 1 << 30;
constexpr uint32_t EN_MAX_S = 255u << 8, EN_MAX_AREA = 1u << 28;

struct EnRule { int32_t clip_q8, strength, smooth_shift, auto_lo, auto_hi, colour; };

MO_HD inline bool en_tiles_ok(int32_t t, int32_t px) { return t >= 1 && t <= EN_MAX_TILES && t <= px; }
MO_HD inline bool en_rule_ok(const EnRule &r) {
    return r.clip_q8 >= 0 && r.clip_q8 <= EN_MAX_CLIP_Q8 && r.strength >= 0 && r.strength <= EN_MAX_STRENGTH && r.smooth_shift >= 0 &&
           r.smooth_shift <= EN_MAX_SHIFT && r.auto_lo >= 0 && r.auto_hi >= r.auto_lo && r.auto_hi <= 255 && (r.colour == EN_SHIFT || r.colour == EN_GAIN);
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------------
MO_HD inline int32_t en_bound(int32_t k, int32_t px, int32_t t) { return (int32_t)((int64_t)k * px / t); }
// the tile that holds pixel x: the last k with en_bound(k) <= x
MO_HD inline int32_t en_tile_of(int32_t x, int32_t px, int32_t t) { return (int32_t)((((int64_t)x + 1) * t - 1) / px); }

// One run of up to 4 pixels of a pixel row, read by cell_grid.h's reader at scale 1 (WIDE: three dwords for a full run whose address
// is a multiple of 4), into the histograms of the row's tiles: add(k * 256 + luma, count) once per stretch of equal neighbours.
// bx[t + 1] are the tile bounds of the axis; k is the tile of x0 or one left of it, and leaves as the tile of the run's last pixel.
template <bool WIDE, typename Add> MO_HD inline void en_hist_run(const uint8_t *p, long long pitch, int32_t x0, int32_t npx, const int32_t *bx, int32_t &k, Add &&add) {
    int32_t next = bx[k + 1];                               // x0 + i < px = bx[t]: k stays below t
    uint32_t prev = 0, cnt = 0, sum[CgRun<1>::CPT];
    cg_read_run<1, WIDE>(p, pitch, npx, 1, sum, [&](int, int i, uint32_t yv) {
        while (x0 + i >= next) next = bx[++k + 1];
        const uint32_t at = (uint32_t)k * 256u + yv;
        if (cnt && at == prev) {
            ++cnt;
        } else {
            if (cnt) add(prev, cnt);
            prev = at; cnt = 1;
        }
    });
    if (cnt) add(prev, cnt);
}

// ---- the curve of a tile, one level at a time (the kernel) and whole (the host) -------------------------------------------------
MO_HD inline uint32_t en_clip(int32_t clip_q8, uint32_t n) {        // 0: no clipping
    if (clip_q8 <= 0) return 0;
    const uint64_t c = ((uint64_t)clip_q8 * n) >> 16;
    return c < 1 ? 1u : (uint32_t)c;
}
MO_HD inline uint32_t en_excess_of(uint32_t hist, uint32_t clip) { return clip && hist > clip ? hist - clip : 0u; }
// bin i after the clip and the redistribution of the tile's whole excess
MO_HD inline uint32_t en_bin(uint32_t hist, int32_t i, uint32_t clip, uint32_t excess) {
    if (!clip) return hist;
    uint32_t v = (hist < clip ? hist : clip) + excess / 256;
    const uint32_t res = excess % 256;
    if (res) {
        const uint32_t step = 256 / res < 1 ? 1 : 256 / res;
        if ((uint32_t)i % step == 0 && (uint32_t)i / step < res) ++v;
    }
    return v;
}
MO_HD inline uint32_t en_level(uint32_t cdf, uint32_t n) { return (uint32_t)(((uint64_t)cdf * 255 + n / 2) / n); }

// hist[256] with sum n -> curve[256]; returns the excess
inline uint32_t en_curve_of(const uint32_t *hist, uint32_t n, int32_t clip_q8, uint32_t *curve) {
    const uint32_t clip = en_clip(clip_q8, n);
    uint32_t excess = 0, cdf = 0;
    for (int i = 0; i < EN_LEVELS; ++i) excess += en_excess_of(hist[i], clip);
    for (int i = 0; i < EN_LEVELS; ++i) {
        cdf += en_bin(hist[i], i, clip, excess);
        curve[i] = en_level(cdf, n);
    }
    return excess;
}

// ---- the state ------------------------------------------------------------------------------------------------------------------
MO_HD inline uint32_t en_ema(uint32_t s, uint32_t curve, int32_t frames_seen, int32_t shift) {
    const int32_t t = (int32_t)(curve << 8);
    if (frames_seen == 0) return (uint32_t)t;
    const int32_t d = t - (int32_t)s;
    return (uint32_t)((int32_t)s + (d >= 0 ? d >> shift : -((-d) >> shift)));
}
MO_HD inline uint32_t en_lut8(uint32_t s) {
    const uint32_t v = (s + 128) >> 8;
    return v > 255 ? 255u : v;
}
MO_HD inline int32_t en_next_seen(int32_t frames_seen) { return frames_seen < EN_MAX_SEEN ? frames_seen + 1 : EN_MAX_SEEN; }

// ---- where a pixel sits along one axis of px pixels and t tiles ------------------------------------------------------------------
MO_HD inline void en_axis(int32_t x, int32_t px, int32_t t, int32_t &k, int32_t &f) {
    const int32_t p = 2 * x;
    k = 0; f = 0;
    if (t == 1 || p <= en_bound(0, px, t) + en_bound(1, px, t) - 1) return;
    if (p >= en_bound(t - 1, px, t) + en_bound(t, px, t) - 1) { k = t - 1; return; }
    k = en_tile_of(x, px, t);                               // the centre of x's own tile is at or right of x, or left of it
    int32_t c = en_bound(k, px, t) + en_bound(k + 1, px, t) - 1;
    if (c > p) { --k; c = en_bound(k, px, t) + en_bound(k + 1, px, t) - 1; }
    const int32_t den = en_bound(k + 1, px, t) + en_bound(k + 2, px, t) - 1 - c;
    f = ((p - c) * 256 + den / 2) / den;
}
// the table entry of a pixel: k << 9 | f
MO_HD inline uint32_t en_axis_pack(int32_t k, int32_t f) { return (uint32_t)k << 9 | (uint32_t)f; }
MO_HD inline int32_t en_neighbour(int32_t k, int32_t t) { return k + 1 < t ? k + 1 : t - 1; }

// ---- a pixel --------------------------------------------------------------------------------------------------------------------
MO_HD inline uint32_t en_interp(uint32_t A, uint32_t B, uint32_t C, uint32_t D, uint32_t fx, uint32_t fy) {
    return ((256u - fy) * ((256u - fx) * A + fx * B) + fy * ((256u - fx) * C + fx * D) + 32768u) >> 16;
}
MO_HD inline uint32_t en_eff(const EnRule &r, uint64_t luma_sum, uint64_t pixels) {
    if (r.auto_hi <= r.auto_lo) return (uint32_t)r.strength;
    const int32_t m = (int32_t)(luma_sum / pixels), span = r.auto_hi - r.auto_lo;
    int32_t a = r.auto_hi - m;
    a = a < 0 ? 0 : (a > span ? span : a);
    return (uint32_t)(r.strength * a / span);
}
MO_HD inline int32_t en_y2(int32_t y, int32_t y1, int32_t eff) { return y + (((y1 - y) * eff + 128) >> 8); }      // (>> of a negative value: floor)
MO_HD inline uint32_t en_channel(int32_t colour, int32_t c, int32_t y, int32_t y2) {
    int32_t v;
    if (colour == EN_GAIN && y != 0) v = (c * y2 + y / 2) / y;
    else v = colour == EN_GAIN ? c + y2 : c + (y2 - y);
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace rtmodt
