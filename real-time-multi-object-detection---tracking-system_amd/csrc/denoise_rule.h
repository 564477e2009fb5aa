// denoise_rule.h -- the one statement of the frame denoiser's rules (csrc/denoise.hip runs them per frame): a motion-adaptive temporal
// filter with a sigma filter of the current frame taken in where the temporal filter lets go.  Plain C++, no HIP: the kernel of
// denoise.hip, the host-only entry point rtmodt_denoise_pixel and tests/native/denoise_rule_check.cpp (built under the address and UB
// sanitizers) all take them from here, and tests/denoise_ref.py restates them in NumPy.  Everything is integer arithmetic.
//   State.    acc, unsigned 8.8 in 16 bits per (stream, pixel, channel), and frames_seen per stream.  prev = min(255, (acc + 128) >> 8).
//   Luma.     mo_luma of motion_model.h, Y(.) below.
//   Motion.   D = |sum over the 3 x 3 neighbourhood of (Y(x_q) - Y(prev_q))|, neighbour coordinates clamped to the frame: nine terms
//             always, and the absolute value of the SUM -- zero-mean noise cancels, a real change does not.  a = 0 for D <= motion_lo,
//             256 for D >= motion_hi, else (D - motion_lo) * 256 / (motion_hi - motion_lo) (floor).  frames_seen == 0: a = 256.
//   Spatial.  Among the up to nine neighbours INSIDE the frame (centre included) q counts when |Y(x_q) - Y(x_p)| <= spatial_thr; per
//             channel s = (sum + n / 2) / n over the n >= 1 that count and xs = x + (((s - x) * a * spatial + 32768) >> 16).
//   Temporal. wmin = 256 >> temporal_shift (0: w = 256, no temporal filtering), w = wmin + (((256 - wmin) * a + 128) >> 8),
//             acc' = acc + ((((xs << 8) - acc) * w + 128) >> 8) with acc counting as xs << 8 when frames_seen == 0, and
//             out = min(255, (acc' + 128) >> 8).
//   Ranges.   Every product fits int32: |s - x| <= 255, a <= 256 and spatial <= 256 give at most 255 * 256 * 256 < 2^24 before the
//             rounding term, and |(xs << 8) - acc| <= 65 280 with w <= 256 gives at most 65 280 * 256 < 2^24.  The shifts of negative
//             values are arithmetic (floor).  s lies between the least and the largest neighbour, so xs stays in 0..255 (a * spatial
//             <= 65 536: xs moves from x towards s and never past it); w <= 256, so acc' lies between acc and xs << 8 and needs no
//             clamp: it stays in 0 .. 255 << 8.
//   Results.  Per call and stream: frames_seen after the call (capped at 2^30), n_static (a == 0), n_moving (a == 256) and
//             absdiff_static, the sum of |Y(x) - Y(prev)| over the a == 0 pixels: 256 * absdiff_static / n_static is the noise figure.
#pragma once

#include "motion_model.h"

namespace rtmodt {

constexpr int DN_MAX_DIM = 16384, DN_MAX_SHIFT = 6, DN_MAX_SPATIAL = 256, DN_MAX_THRESHOLD = 9 * 255, DN_MAX_SEEN = 1 << 30;
constexpr uint32_t DN_MAX_ACC = 255u << 8;
constexpr int DN_RUN = 4;                                   // a lane's run of pixels: 12 frame bytes, 24 bytes of acc

struct DnRule { int32_t motion_lo, motion_hi, temporal_shift, spatial, spatial_thr; };

MO_HD inline bool dn_rule_ok(const DnRule &r) {
    return r.motion_lo >= 0 && r.motion_hi > r.motion_lo && r.motion_hi <= DN_MAX_THRESHOLD && r.temporal_shift >= 0 && r.temporal_shift <= DN_MAX_SHIFT &&
           r.spatial >= 0 && r.spatial <= DN_MAX_SPATIAL && r.spatial_thr >= 0 && r.spatial_thr <= 255;
}

// ---- a run of up to 4 pixels of a row: px[i] = b | g << 8 | r << 16 --------------------------------------------------------------
// WIDE: three dwords for a full run whose address is a multiple of 4; a partial run goes byte by byte and touches no byte behind it
struct __attribute__((aligned(4))) DnRun { uint32_t a, b, c; };
template <bool WIDE> MO_HD inline void dn_load_run(const uint8_t *p, int32_t npx, uint32_t *px) {
    if (WIDE && npx == DN_RUN) {
        const DnRun v = *(const DnRun *)p;
        px[0] = v.a & 0xffffffu; px[1] = v.a >> 24 | (v.b & 0xffffu) << 8; px[2] = v.b >> 16 | (v.c & 0xffu) << 16; px[3] = v.c >> 8;
    } else {
        for (int i = 0; i < DN_RUN; ++i) px[i] = i < npx ? (uint32_t)p[3 * i] | (uint32_t)p[3 * i + 1] << 8 | (uint32_t)p[3 * i + 2] << 16 : 0u;
    }
}
template <bool WIDE> MO_HD inline void dn_store_run(uint8_t *p, int32_t npx, const uint32_t *px) {
    if (WIDE && npx == DN_RUN) {
        DnRun v;
        v.a = px[0] | px[1] << 24; v.b = px[1] >> 8 | px[2] << 16; v.c = px[2] >> 16 | px[3] << 8;
        *(DnRun *)p = v;
    } else {
        for (int i = 0; i < DN_RUN; ++i)
            if (i < npx) {
                p[3 * i] = (uint8_t)px[i]; p[3 * i + 1] = (uint8_t)(px[i] >> 8); p[3 * i + 2] = (uint8_t)(px[i] >> 16);
            }
    }
}
MO_HD inline uint32_t dn_luma_of(uint32_t px) { return mo_luma(px & 255u, px >> 8 & 255u, px >> 16 & 255u); }

// ---- the steps -------------------------------------------------------------------------------------------------------------------
MO_HD inline uint32_t dn_prev(uint32_t acc) {
    const uint32_t v = (acc + 128) >> 8;
    return v > 255 ? 255u : v;
}
// the pixel prev of three acc values, packed like a frame pixel
MO_HD inline uint32_t dn_prev_px(uint32_t acc_b, uint32_t acc_g, uint32_t acc_r) { return dn_prev(acc_b) | dn_prev(acc_g) << 8 | dn_prev(acc_r) << 16; }
MO_HD inline int32_t dn_alpha(const DnRule &r, int32_t D, int32_t frames_seen) {
    if (frames_seen == 0 || D >= r.motion_hi) return 256;
    if (D <= r.motion_lo) return 0;
    return (D - r.motion_lo) * 256 / (r.motion_hi - r.motion_lo);
}
MO_HD inline int32_t dn_mean(int32_t sum, int32_t n) { return (sum + n / 2) / n; }
MO_HD inline int32_t dn_spatial(int32_t x, int32_t s, int32_t a, int32_t spatial) { return x + (((s - x) * a * spatial + 32768) >> 16); }
MO_HD inline int32_t dn_weight(const DnRule &r, int32_t a) {
    const int32_t wmin = 256 >> r.temporal_shift;
    return wmin + (((256 - wmin) * a + 128) >> 8);
}
MO_HD inline uint32_t dn_acc(uint32_t acc, int32_t xs, int32_t w, int32_t frames_seen) {
    const int32_t t = xs << 8, old = frames_seen == 0 ? t : (int32_t)acc;
    return (uint32_t)(old + (((t - old) * w + 128) >> 8));
}
MO_HD inline int32_t dn_next_seen(int32_t frames_seen) { return frames_seen < DN_MAX_SEEN ? frames_seen + 1 : DN_MAX_SEEN; }

// ---- one pixel from its two 3 x 3 neighbourhoods ----------------------------------------------------------------------------------
// px[9]: the frame's pixels, packed, b | g << 8 | r << 16 | Y << 24, row by row, coordinates clamped to the frame; dy[9]: Y(x) - Y(prev)
// of the same nine; inside: bit q set when neighbour q lies inside the frame (bit 4, the centre, always); acc[3]: the centre's state,
// replaced.  Returns the output pixel, packed with its luma in bits 24..31 (the next call's Y(prev)); a and D for the counters.
struct DnPixel { uint32_t out; int32_t a, D; };
MO_HD inline DnPixel dn_pixel(const DnRule &r, const uint32_t *px, const int32_t *dy, uint32_t inside, int32_t frames_seen, uint32_t *acc) {
    int32_t D = 0;
    for (int q = 0; q < 9; ++q) D += dy[q];
    D = D < 0 ? -D : D;
    const int32_t a = dn_alpha(r, D, frames_seen), yc = (int32_t)(px[4] >> 24);
    int32_t n = 0, sum[3] = {0, 0, 0};
    for (int q = 0; q < 9; ++q) {
        const int32_t d = (int32_t)(px[q] >> 24) - yc;
        if ((inside >> q & 1u) && (d < 0 ? -d : d) <= r.spatial_thr) {
            ++n;
            sum[0] += (int32_t)(px[q] & 255u); sum[1] += (int32_t)(px[q] >> 8 & 255u); sum[2] += (int32_t)(px[q] >> 16 & 255u);
        }
    }
    const int32_t w = dn_weight(r, a);
    uint32_t out = 0;
    for (int k = 0; k < 3; ++k) {
        const int32_t x = (int32_t)(px[4] >> (8 * k) & 255u);
        acc[k] = dn_acc(acc[k], dn_spatial(x, dn_mean(sum[k], n), a, r.spatial), w, frames_seen);
        out |= dn_prev(acc[k]) << (8 * k);
    }
    return DnPixel{out | dn_luma_of(out) << 24, a, D};
}

}  // namespace rtmodt
