// letterbox.h -- the one statement of the letterbox's host arithmetic: where a frame lands in the network's rectangle (ultralytics
// LetterBox, oracle/yolo_oracle.py: letterbox_params), how boxes travel back (scale_boxes' gain and pads) and cv::resize's
// INTER_LINEAR 8-bit tables (oracle/yolo_oracle.py: _resize_coeffs).  The detector (engine.hip) and the overview image of sliced
// inference (slice.hip) both take it from here; the pixel that goes with it is letterbox_dev.h.  Plain C++, no HIP:
// tests/native/letterbox_check.cpp and slice_grid_check.cpp compile it on the host under the address and UB sanitizers, and
// tests/test_letterbox_cpu.py compares it with the oracle over a sweep of geometries.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace rtmodt {

// What the kernels take by value.  A frame of src_h x src_w becomes new_h x new_w at (top, left) of the canvas; resize == 0: a copy.
struct LetterboxGeom { int src_h, src_w, new_w, new_h, top, left, resize; };
struct ResizeTables {          // device arrays, cv::resize INTER_LINEAR fixed-point tables
    const int32_t *xofs, *xa0, *xa1, *yofs, *yb0, *yb1;
};

// ... and the way back for boxes (scale_boxes, App. B.4): pad and gain in double, handed to the kernels as float32
struct Letterbox { LetterboxGeom g; double gain; int pad_x, pad_y; };

inline int round_half_even(double v) { return (int)std::nearbyint(v); }   // == Python round()

// An h x w frame into in_h x in_w (App. B.1).  rect: LetterBox(auto=True) -- new_shape is the SQUARE S x S (S = the longer side of
// the rectangle the engine was built for), the pads are whatever is left of the rectangle (== the square's pads mod 32)
inline Letterbox letterbox_geometry(int h, int w, int in_h, int in_w, bool rect = false) {
    Letterbox lb;
    LetterboxGeom &g = lb.g;
    g.src_h = h; g.src_w = w;
    const int S = std::max(in_h, in_w);
    double r = rect ? std::min((double)S / h, (double)S / w) : std::min((double)in_h / h, (double)in_w / w);
    g.new_w = round_half_even(w * r); g.new_h = round_half_even(h * r);
    double dw = (in_w - g.new_w) / 2.0, dh = (in_h - g.new_h) / 2.0;
    g.top = round_half_even(dh - 0.1); g.left = round_half_even(dw - 0.1);
    g.resize = (g.new_w != w) || (g.new_h != h);
    lb.gain = std::min((double)in_h / h, (double)in_w / w);
    lb.pad_x = round_half_even((in_w - w * lb.gain) / 2 - 0.1);
    lb.pad_y = round_half_even((in_h - h * lb.gain) / 2 - 0.1);
    return lb;
}

// The tables of one axis: source index and the two 11-bit weights per destination position
inline void resize_table(int dst, int src, int32_t *ofs, int32_t *c0, int32_t *c1) {
    const double scale = 1.0 / ((double)dst / src);
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f = f - (float)s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        ofs[d] = s;
        c0[d] = (int)std::nearbyint((1.0f - f) * 2048.0f);
        c1[d] = (int)std::nearbyint(f * 2048.0f);
    }
}

// Both axes in one array, in ResizeTables' member order: xofs | xa0 | xa1 (new_w each) | yofs | yb0 | yb1 (new_h each) ...
inline std::vector<int32_t> resize_tables(const LetterboxGeom &g) {
    std::vector<int32_t> t((size_t)3 * (g.new_w + g.new_h));
    int32_t *x = t.data(), *y = x + 3 * g.new_w;
    resize_table(g.new_w, g.src_w, x, x + g.new_w, x + 2 * g.new_w);
    resize_table(g.new_h, g.src_h, y, y + g.new_h, y + 2 * g.new_h);
    return t;
}
// ... and that array as seen from `base`, the address a copy of it lives at
inline ResizeTables resize_tables_at(const int32_t *base, const LetterboxGeom &g) {
    const int32_t *x = base, *y = x + 3 * g.new_w;
    return ResizeTables{x, x + g.new_w, x + 2 * g.new_w, y, y + g.new_h, y + 2 * g.new_h};
}

}  // namespace rtmodt
