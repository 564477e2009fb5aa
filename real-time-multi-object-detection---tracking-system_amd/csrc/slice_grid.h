// slice_grid.h -- the host arithmetic of sliced inference (slice.hip): where the tiles of a frame lie.  How the overview image is
// letterboxed and how its boxes travel back is the detector's own letterbox (letterbox.h, included here for slice.hip and the
// native check).  Plain C++, no HIP: tests/native/slice_grid_check.cpp compiles it on the host under the address and UB
// sanitizers, and tests/slice_ref.py restates it.
//
// The grid (SAHI's get_slice_bboxes with the last tile shifted inward): along an axis of length L with tile t and overlap o,
// 0 <= o < t:  te = min(t, L);  step = te - o (one position, 0, when step <= 0);  p_k = min(k * step, L - te) for k = 0, 1, ...
// up to and including the first with p_k + te >= L.  Every tile is te long and lies inside [0, L).
#pragma once

#include <algorithm>
#include <vector>

#include "letterbox.h"

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

}  // namespace rtmodt
