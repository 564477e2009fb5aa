// compose_rule.h -- the one statement of the compositor's per-cell and per-pixel arithmetic: which part of a source a cell shows, where
// the picture stands inside the cell's rectangle, the taps and weights of each axis, the one-rounding pixel and the forward BT.601
// conversion of the 4:2:0 outputs (csrc/compose.hip keeps the layout, cuts the outputs into tiles and runs the kernel).  Plain C++,
// no HIP: the kernel of compose.hip, the host-only entry point rtmodt_compose_plan and tests/native/compose_rule_check.cpp (built
// under the address and UB sanitizers) all take it from here, and tests/compose_ref.py restates it in NumPy.  Integer arithmetic
// throughout, but for the weights of an enlarging axis, which letterbox.h's resize_table builds on the host in float32.
//   1. the CROP: the cell's source rectangle (x, y, w, h), inside the source; 0, 0, 0, 0 is the whole source.  Sw x Sh its size;
//   2. THE FIT of the crop into the cell's rectangle Rw x Rh of the output (cp_fit is snapshot_rule.h's rule 4 without its "never
//      enlarging" clause: the axis that is relatively longer fills, the other is rounded to nearest, at least 1):
//        STRETCH  the INNER picture is the whole rectangle, the crop is kept;
//        FIT      the inner picture is cp_fit(crop into rectangle), at ox = (Rw - Dw) / 2, oy = (Rh - Dh) / 2 of the rectangle
//                 (floored); every other pixel of the rectangle is the cell's pad colour;
//        FILL     the inner picture is the whole rectangle; the crop is cut to cp_fit(rectangle into crop), Cw x Ch, and moved by
//                 (Sw - Cw) / 2, (Sh - Ch) / 2 (floored): cut centrally, no bars;
//   3. on a 4:2:0 output (its rectangles are even already) the inner picture of FIT becomes even: Dw and Dh are rounded UP to the next
//      even number (never past the rectangle, which is even and at least as large), then ox and oy are computed as above and rounded
//      DOWN to even.  Chroma blocks therefore never straddle a cell's picture and its bars;
//   4. each AXIS maps S source pixels (of the effective crop) onto D destination pixels (of the inner picture) and is of one kind:
//        SHRINK   S > D: destination j covers sn_span(S, D, j) with sn_weight (snapshot_rule.h rule 5), total T = S;
//        COPY     S == D: the one tap j, weight 1, T = 1;
//        ENLARGE  S < D: resize_table(D, S) (letterbox.h): taps ofs[j] and min(ofs[j] + 1, S - 1) with the 11-bit weights c0[j], c1[j],
//                 T = 2048 (the second tap of the last pixels has weight 0);
//   5. a channel of a pixel is (sum_y wy (sum_x wx p) + Tx Ty / 2) / (Tx Ty) in 64 bits: ONE rounding for both axes, whatever their
//      kinds.  Two shrinking axes: sn_pixel exactly.  Two enlarging axes: NOT letterbox_dev.h's pixel, which rounds between its passes;
//   6. pixels are painted in cell order, a later cell on top: the value of the last cell whose rectangle holds the pixel, else the
//      output's background.  A cell whose source is absent in a run shows its offline colour on its whole rectangle;
//   7. 4:2:0: the forward form of the conversion preprocess.hip inverts (BT.601 limited range, 20-bit shift):
//        Y = ( 269484 R + 528482 G + 102760 B + 2^19 +  16 * 2^20) >> 20                  per pixel
//        U = (-155188 R - 305135 G + 460324 B + 2^19 + 128 * 2^20) >> 20                  of the 2 x 2 block's per-channel mean
//        V = ( 460324 R - 385875 G -  74448 B + 2^19 + 128 * 2^20) >> 20                  (b00 + b01 + b10 + b11 + 2) >> 2
//      (every sum is positive and below 2^28: int32 is exact).
#pragma once

#include <cstdint>

#include "letterbox.h"
#include "snapshot_rule.h"

#ifndef CP_HD
#define CP_HD SN_HD
#endif

namespace rtmodt {

constexpr int CP_MAX_SOURCES = 64, CP_MAX_OUTPUTS = 16, CP_MAX_CELLS = 64, CP_MAX_DIM = 16384;
constexpr int CP_STRETCH = 0, CP_FIT = 1, CP_FILL = 2;
constexpr int CP_SHRINK = 0, CP_COPY = 1, CP_ENLARGE = 2;
constexpr int CP_ENLARGE_TOTAL = 2048;

struct CpRect { int32_t x, y, w, h; };

struct CpPlan {
    CpRect crop;               // 2. the effective crop inside the source
    CpRect inner;              // 2. / 3. the inner picture, in OUTPUT coordinates
    int32_t kind_x, kind_y;    // 4.
};

CP_HD inline bool cp_rect_inside(const CpRect &r, int32_t h, int32_t w) {
    return r.w >= 1 && r.h >= 1 && r.x >= 0 && r.y >= 0 && (int64_t)r.x + r.w <= w && (int64_t)r.y + r.h <= h;
}

// 2. sw x sh fitted into tw x th, aspect kept
CP_HD inline void cp_fit(int32_t sw, int32_t sh, int32_t tw, int32_t th, int32_t &dw, int32_t &dh) {
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

CP_HD inline int32_t cp_kind(int32_t S, int32_t D) { return S > D ? CP_SHRINK : S == D ? CP_COPY : CP_ENLARGE; }
CP_HD inline int32_t cp_total(int32_t kind, int32_t S) { return kind == CP_SHRINK ? S : kind == CP_COPY ? 1 : CP_ENLARGE_TOTAL; }

// 1. - 4. one cell: `crop` as the caller gave it (all zero: the whole src_h x src_w source; else it must lie inside the source),
// `rect` inside the output, `yuv420`: the output is NV12 / I420
CP_HD inline void cp_plan(int32_t src_h, int32_t src_w, CpRect crop, const CpRect &rect, int32_t fit, bool yuv420, CpPlan &out) {
    if (crop.x == 0 && crop.y == 0 && crop.w == 0 && crop.h == 0) crop = CpRect{0, 0, src_w, src_h};
    CpRect in = rect;
    if (fit == CP_FIT) {
        int32_t dw, dh;
        cp_fit(crop.w, crop.h, rect.w, rect.h, dw, dh);
        if (yuv420) { dw += dw & 1; dh += dh & 1; }
        int32_t ox = (rect.w - dw) / 2, oy = (rect.h - dh) / 2;
        if (yuv420) { ox &= ~1; oy &= ~1; }
        in = CpRect{rect.x + ox, rect.y + oy, dw, dh};
    } else if (fit == CP_FILL) {
        int32_t cw, ch;
        cp_fit(rect.w, rect.h, crop.w, crop.h, cw, ch);
        crop = CpRect{crop.x + (crop.w - cw) / 2, crop.y + (crop.h - ch) / 2, cw, ch};
    }
    out.crop = crop;
    out.inner = in;
    out.kind_x = cp_kind(crop.w, in.w);
    out.kind_y = cp_kind(crop.h, in.h);
}

// 4. the taps i0 .. i1 of destination pixel j of an axis; `tab`: resize_table(D, S)'s ofs | c0 | c1 (D entries each), ENLARGE only
CP_HD inline void cp_span(int32_t kind, int32_t S, int32_t D, int32_t j, const int32_t *tab, int32_t &i0, int32_t &i1) {
    if (kind == CP_SHRINK) sn_span(S, D, j, i0, i1);
    else if (kind == CP_COPY) i0 = i1 = j;
    else {
        i0 = tab[j];
        i1 = i0 + 1 < S ? i0 + 1 : S - 1;
    }
}
// ... and the weight of tap i of that span
CP_HD inline int32_t cp_weight(int32_t kind, int32_t S, int32_t D, int32_t j, int32_t i, const int32_t *tab) {
    if (kind == CP_SHRINK) return sn_weight(S, D, j, i);
    if (kind == CP_COPY) return 1;
    return i == tab[j] ? tab[D + j] : tab[2 * D + j];
}

// 5. the one rounding
CP_HD inline uint8_t cp_round(int64_t acc, int64_t tot) { return (uint8_t)((acc + tot / 2) / tot); }

// one channel of the inner picture: destination (dx, dy) of the plan's inner picture, `src` the first byte of the SOURCE (rows `pitch`
// bytes apart, BGR24); the reference form (the kernel sums the same terms from staged rows)
CP_HD inline uint8_t cp_pixel(const uint8_t *src, int64_t pitch, const CpPlan &p, const int32_t *tab_x, const int32_t *tab_y, int32_t dx, int32_t dy,
                              int32_t ch) {
    const int32_t Sw = p.crop.w, Sh = p.crop.h, Dw = p.inner.w, Dh = p.inner.h;
    int32_t x0, x1, y0, y1;
    cp_span(p.kind_x, Sw, Dw, dx, tab_x, x0, x1);
    cp_span(p.kind_y, Sh, Dh, dy, tab_y, y0, y1);
    int64_t acc = 0;
    for (int32_t y = y0; y <= y1; ++y) {
        int64_t row = 0;
        for (int32_t x = x0; x <= x1; ++x)
            row += (int64_t)cp_weight(p.kind_x, Sw, Dw, dx, x, tab_x) * src[(int64_t)(p.crop.y + y) * pitch + 3 * (int64_t)(p.crop.x + x) + ch];
        acc += row * cp_weight(p.kind_y, Sh, Dh, dy, y, tab_y);
    }
    return cp_round(acc, (int64_t)cp_total(p.kind_x, Sw) * cp_total(p.kind_y, Sh));
}

// 7.
CP_HD inline int32_t cp_yuv_y(int32_t b, int32_t g, int32_t r) { return (269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20; }
CP_HD inline int32_t cp_yuv_u(int32_t b, int32_t g, int32_t r) { return (-155188 * r - 305135 * g + 460324 * b + (1 << 19) + (128 << 20)) >> 20; }
CP_HD inline int32_t cp_yuv_v(int32_t b, int32_t g, int32_t r) { return (460324 * r - 385875 * g - 74448 * b + (1 << 19) + (128 << 20)) >> 20; }
CP_HD inline int32_t cp_block_mean(int32_t a, int32_t b, int32_t c, int32_t d) { return (a + b + c + d + 2) >> 2; }

}  // namespace rtmodt
