// letterbox_dev.h -- the letterboxed pixel, once, for every kernel that makes one (preprocess.hip: letterbox_kernel,
// letterbox_yuv420_kernel; slice.hip: the overview image of slice_gather_kernel).  Geometry and tables come from letterbox.h.
//
// The resize is OpenCV's 8-bit fixed-point bilinear (cv2.resize INTER_LINEAR), restated bit for bit: 11-bit coefficients,
// horizontal pass x2048 in int32, vertical pass (((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2; outside the resized frame
// the canvas is copyMakeBorder's 114.
#pragma once

#include "kernels.h"

namespace rtmodt {

// source functor of packed BGR24 frames: the BGR of source pixel (x, y)
struct Bgr24Source {
    const uint8_t *__restrict__ f; int pitch;
    __device__ __forceinline__ void operator()(int x, int y, int &b, int &g, int &r) const {
        const uint8_t *p = f + (long)y * pitch + x * 3;
        b = p[0]; g = p[1]; r = p[2];
    }
};

// B, G, R (0..255) of canvas position (x, y); src(sx, sy, b, g, r) reads one source pixel
template <typename Source>
__device__ __forceinline__ void letterbox_pixel(int x, int y, const LetterboxGeom &g, const ResizeTables &t, const Source &src, int &c0, int &c1,
                                                int &c2) {
    const int sy = y - g.top, sx = x - g.left;
    c0 = 114; c1 = 114; c2 = 114;
    if (sy >= 0 && sy < g.new_h && sx >= 0 && sx < g.new_w) {
        if (!g.resize) {
            src(sx, sy, c0, c1, c2);
        } else {
            const int xi = t.xofs[sx], a0 = t.xa0[sx], a1 = t.xa1[sx];
            const int yi = t.yofs[sy], b0 = t.yb0[sy], b1 = t.yb1[sy];
            const int xj = min(xi + 1, g.src_w - 1), yj = min(yi + 1, g.src_h - 1);
            int p00[3], p01[3], p10[3], p11[3];
            src(xi, yi, p00[0], p00[1], p00[2]);
            src(xj, yi, p01[0], p01[1], p01[2]);
            src(xi, yj, p10[0], p10[1], p10[2]);
            src(xj, yj, p11[0], p11[1], p11[2]);
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int h0 = p00[c] * a0 + p01[c] * a1;
                const int h1 = p10[c] * a0 + p11[c] * a1;
                const int o = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                v[c] = min(max(o, 0), 255);
            }
            c0 = v[0]; c1 = v[1]; c2 = v[2];
        }
    }
}

}  // namespace rtmodt
