// slice_grid.h -- the host arithmetic of sliced inference (slice.hip): where the tiles of a frame lie, how the overview image is
// letterboxed, how its boxes travel back.  Plain C++, no HIP: tests/native/slice_grid_check.cpp compiles it on the host under the
// address and UB sanitizers, and tests/slice_ref.py restates it.
//
// The grid (SAHI's get_slice_bboxes with the last tile shifted inward): along an axis of length L with tile t and overlap o,
// 0 <= o < t:  te = min(t, L);  step = te - o (one position, 0, when step <= 0);  p_k = min(k * step, L - te) for k = 0, 1, ...
// up to and including the first with p_k + te >= L.  Every tile is te long and lies inside [0, L).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace rtmodt {

constexpr int SLICE_MAX_TILES = 64;         // tiles per frame
constexpr int SLICE_MAX_IMAGES = 65;        // ... plus the overview
constexpr int SLICE_MAX_CAND = 8192;        // candidates per frame the merge sorts in LDS (the NMS kernel's sort size)

struct SliceAxis { int te = 0; std::vector<int> pos; };

// false: a bad argument (L < 1, t < 1, o outside [0, t))
inline bool slice_axis(int L, int t, int o, SliceAxis *out) {
    if (L < 1 || t < 1 || o < 0 || o >= t) return false;
    out->te = std::min(t, L);
    out->pos.clear();
    const int te = out->te, step = te - o;
    if (step <= 0) { out->pos.push_back(0); return true; }
    for (long k = 0;; ++k) {
        const long p = std::min(k * (long)step, (long)(L - te));
        out->pos.push_back((int)p);
        if (p + te >= L) break;
    }
    return true;
}

struct SliceGrid {
    int te_w = 0, te_h = 0;
    std::vector<int> x, y;                  // per tile, row-major (y outer, x inner)
    int tiles() const { return (int)x.size(); }
};

// 0 ok, 1 bad argument, 2 more than SLICE_MAX_TILES tiles
inline int slice_grid(int W, int H, int tw, int th, int ow, int oh, SliceGrid *g) {
    SliceAxis ax, ay;
    if (!slice_axis(W, tw, ow, &ax) || !slice_axis(H, th, oh, &ay)) return 1;
    if ((long)ax.pos.size() * (long)ay.pos.size() > SLICE_MAX_TILES) return 2;
    g->te_w = ax.te; g->te_h = ay.te;
    g->x.clear(); g->y.clear();
    for (int py : ay.pos)
        for (int px : ax.pos) { g->x.push_back(px); g->y.push_back(py); }
    return 0;
}

// The overview: the whole h x w frame letterboxed into in_h x in_w (ultralytics LetterBox, oracle/yolo_oracle.py:295-308) and the way
// back for its boxes (scale_boxes, oracle/yolo_oracle.py:457-468: pad and gain in double, handed to the kernel as float32)
struct SliceLetterbox { int new_w, new_h, top, left, resize; float gain, pad_x, pad_y; };

inline int slice_round_half_even(double v) { return (int)std::nearbyint(v); }      // == Python round()

inline SliceLetterbox slice_letterbox(int h, int w, int in_h, int in_w) {
    SliceLetterbox g;
    const double r = std::min((double)in_h / h, (double)in_w / w);
    g.new_w = slice_round_half_even(w * r); g.new_h = slice_round_half_even(h * r);
    const double dw = (in_w - g.new_w) / 2.0, dh = (in_h - g.new_h) / 2.0;
    g.top = slice_round_half_even(dh - 0.1); g.left = slice_round_half_even(dw - 0.1);
    g.resize = (g.new_w != w) || (g.new_h != h);
    g.gain = (float)r;
    g.pad_x = (float)slice_round_half_even((in_w - w * r) / 2 - 0.1);
    g.pad_y = (float)slice_round_half_even((in_h - h * r) / 2 - 0.1);
    return g;
}

// cv::resize INTER_LINEAR 8-bit tables for one axis (oracle/yolo_oracle.py:311-330, _resize_coeffs): source index and the two
// 11-bit weights per destination position
inline void slice_resize_table(int dst, int src, int32_t *ofs, int32_t *c0, int32_t *c1) {
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

}  // namespace rtmodt
