// lens_model.h -- the one statement of the lens corrector's rules: where an output (rectified) pixel reads the source picture, how
// that position becomes four taps with integer weights, what one output byte is, and how single points travel between the original
// and the rectified picture (csrc/lens.hip samples frames through the table built here).  Plain C++, no HIP: the host entry points
// and tests/native/lens_model_check.cpp (built under the address and UB sanitizers) take it from here, and tests/lens_ref.py
// restates it with NumPy float64 and Python integers.  Every float64 step is one of + - x / (and floor / a comparison, which are
// exact), each rounded on its own (no contraction into a fused multiply-add), in exactly the order written: NumPy reproduces it bit
// for bit.  There is no transcendental, hence no fisheye model: such a lens enters as a caller's map.
//
// Lens: OpenCV's pinhole + Brown-Conrady / rational model without a rectification rotation.  Source intrinsics fx fy cx cy,
// coefficients k[8] = k1 k2 p1 p2 k3 k4 k5 k6 (all zero: no distortion), output intrinsics nfx nfy ncx ncy (nfx == 0: all four are
// copied from the source intrinsics), r2_limit (0: none).  Integer pixel coordinates are pixel centres.
//   1. map of output pixel (u, v), widened to float64:
//          x  = (u - ncx) / nfx                 y  = (v - ncy) / nfy
//          xx = x x     yy = y y     xy = x y   r2 = xx + yy
//          num = 1 + r2 (k1 + r2 (k2 + r2 k3))  den = 1 + r2 (k4 + r2 (k5 + r2 k6))         (Horner, innermost product first)
//          rad = num / den
//          dx = (2 p1) xy + p2 (r2 + 2 xx)      dy = p1 (r2 + 2 yy) + (2 p2) xy
//          xd = x rad + dx                      yd = y rad + dy
//          sx = fx xd + cx                      sy = fy yd + cy
//      OUTSIDE when den is not > 0, or r2_limit > 0 and r2 > r2_limit (the fold-back of a strongly negative k1 far from the axis).
//   2. a position (sx, sy) -- from 1., or a caller's float32 map entry widened to float64 -- is OUTSIDE when sx or sy is not inside
//      (-2^20, 2^20) (a NaN or an infinity fails the comparison).  Else, 5 fractional bits:
//          qx = (int32) floor(sx 32 + 0.5)      x0 = qx >> 5 (arithmetic)      ax = qx & 31          likewise qy, y0, ay
//      the four taps are (x0 + i, y0 + j), i, j in {0, 1}, with weights (32 - ax, ax) x (32 - ay, ay); the pixel is OUTSIDE too when no
//      tap of non-zero weight lies in [0, W) x [0, H).  The canonical table holds qx, qy and outside (0 / 1); qx = qy = 0 where outside.
//   3. sampling, integers only, per channel: out = (sum of weight x tap + 512) >> 10; a tap off the source reads the border colour;
//      an OUTSIDE pixel is the border colour.
//   4. points, float64.  distort (rectified -> original) is 1. without the OUTSIDE tests.  undistort (original -> rectified) is OpenCV's
//      fixed-point scheme: xd = (px - cx) / fx, yd = (py - cy) / fy, start at (x, y) = (xd, yd), then exactly 20 times, no early exit,
//          x <- (xd - dx(x, y)) / rad(x, y)     y <- (yd - dy(x, y)) / rad(x, y)            (both from the old x, y)
//      and u = nfx x + ncx, v = nfy y + ncy.  Its residual is max(|distort(u, v) - (px, py)|) over the two axes in pixels, +infinity
//      when that is not a number: a lens on which the iteration does not converge shows as a number, not as a silently wrong point.
#pragma once

#include <cmath>
#include <cstdint>

namespace rtmodt {

constexpr int LENS_BITS = 5, LENS_ONE = 1 << LENS_BITS, LENS_ITERS = 20, LENS_MAX_DIM = 16384;
constexpr double LENS_LIMIT = 1048576.0;                    // 2^20

struct LensModel {                                          // the layout of rtmodt_lens_params
    double fx, fy, cx, cy;
    double k[8];                                            // k1 k2 p1 p2 k3 k4 k5 k6
    double nfx, nfy, ncx, ncy;
    double r2_limit;
};

inline bool lens_finite(double v) { return v - v == 0.0; }

// nfx == 0: the output intrinsics are the source's
inline LensModel lens_resolve(const LensModel &in) {
    LensModel m = in;
    if (m.nfx == 0.0) { m.nfx = m.fx; m.nfy = m.fy; m.ncx = m.cx; m.ncy = m.cy; }
    return m;
}

// a resolved model's focal lengths are finite and > 0
inline bool lens_model_ok(const LensModel &m) {
    return lens_finite(m.fx) && lens_finite(m.fy) && lens_finite(m.nfx) && lens_finite(m.nfy) && m.fx > 0.0 && m.fy > 0.0 && m.nfx > 0.0 && m.nfy > 0.0;
}

struct LensTerms { double r2, den, rad, dx, dy; };

// rule 1's middle part at the normalised point (x, y)
inline LensTerms lens_terms(const LensModel &m, double x, double y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double k1 = m.k[0], k2 = m.k[1], p1 = m.k[2], p2 = m.k[3], k3 = m.k[4], k4 = m.k[5], k5 = m.k[6], k6 = m.k[7];
    const double xx = x * x, yy = y * y, xy = x * y;
    LensTerms t;
    t.r2 = xx + yy;
    double a = t.r2 * k3;
    a = k2 + a; a = t.r2 * a; a = k1 + a; a = t.r2 * a;
    const double num = 1.0 + a;
    double b = t.r2 * k6;
    b = k5 + b; b = t.r2 * b; b = k4 + b; b = t.r2 * b;
    t.den = 1.0 + b;
    t.rad = num / t.den;
    const double two_p1 = 2.0 * p1, two_p2 = 2.0 * p2;
    const double e0 = two_p1 * xy, e1 = 2.0 * xx, e2 = t.r2 + e1, e3 = p2 * e2;
    t.dx = e0 + e3;
    const double g0 = 2.0 * yy, g1 = t.r2 + g0, g2 = p1 * g1, g3 = two_p2 * xy;
    t.dy = g2 + g3;
    return t;
}

// rule 1 for a resolved model: output position (u, v) -> source position; false: OUTSIDE by den or r2_limit
inline bool lens_map(const LensModel &m, double u, double v, double &sx, double &sy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double x = (u - m.ncx) / m.nfx, y = (v - m.ncy) / m.nfy;
    const LensTerms t = lens_terms(m, x, y);
    const double xr = x * t.rad, yr = y * t.rad;
    const double xd = xr + t.dx, yd = yr + t.dy;
    const double fxd = m.fx * xd, fyd = m.fy * yd;
    sx = fxd + m.cx;
    sy = fyd + m.cy;
    if (!(t.den > 0.0)) return false;
    if (m.r2_limit > 0.0 && t.r2 > m.r2_limit) return false;
    return true;
}

inline bool lens_axis_hit(int32_t q, int size) {
    const int32_t p0 = q >> LENS_BITS, a = q & (LENS_ONE - 1);
    return (p0 >= 0 && p0 < size) || (a > 0 && p0 + 1 >= 0 && p0 + 1 < size);
}

// rule 2: false: OUTSIDE (qx, qy are then 0)
inline bool lens_quantise(double sx, double sy, int src_h, int src_w, int32_t &qx, int32_t &qy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    qx = qy = 0;
    if (!(sx > -LENS_LIMIT && sx < LENS_LIMIT && sy > -LENS_LIMIT && sy < LENS_LIMIT)) return false;
    const double tx = sx * 32.0, ty = sy * 32.0;
    const int32_t ix = (int32_t)floor(tx + 0.5), iy = (int32_t)floor(ty + 0.5);
    if (!(lens_axis_hit(ix, src_w) && lens_axis_hit(iy, src_h))) return false;
    qx = ix; qy = iy;
    return true;
}

// the canonical table of a model (any model: it is resolved here); arrays of out_h x out_w; returns the number of OUTSIDE pixels
inline long long lens_build_model(const LensModel &model, int src_h, int src_w, int out_h, int out_w, int32_t *qx, int32_t *qy, uint8_t *outside) {
    const LensModel m = lens_resolve(model);
    long long n_out = 0;
    for (int v = 0; v < out_h; ++v)
        for (int u = 0; u < out_w; ++u) {
            const size_t i = (size_t)v * out_w + u;
            double sx, sy;
            const bool in = lens_map(m, (double)u, (double)v, sx, sy) && lens_quantise(sx, sy, src_h, src_w, qx[i], qy[i]);
            if (!in) { qx[i] = qy[i] = 0; ++n_out; }
            outside[i] = in ? 0 : 1;
        }
    return n_out;
}

// the canonical table of a caller's map (float32 [out_h][out_w] each, the form cv2.remap takes)
inline long long lens_build_from_map(const float *map_x, const float *map_y, int src_h, int src_w, int out_h, int out_w, int32_t *qx, int32_t *qy,
                                     uint8_t *outside) {
    long long n_out = 0;
    const size_t n = (size_t)out_h * out_w;
    for (size_t i = 0; i < n; ++i) {
        const bool in = lens_quantise((double)map_x[i], (double)map_y[i], src_h, src_w, qx[i], qy[i]);
        if (!in) ++n_out;
        outside[i] = in ? 0 : 1;
    }
    return n_out;
}

// rule 3 on one channel of one pixel; tap(x, y) is only called inside the source
template <typename Tap> inline int lens_sample(int32_t qx, int32_t qy, int src_h, int src_w, int border, Tap tap) {
    const int32_t x0 = qx >> LENS_BITS, y0 = qy >> LENS_BITS, ax = qx & (LENS_ONE - 1), ay = qy & (LENS_ONE - 1);
    int32_t sum = 0;
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) {
            const int32_t x = x0 + i, y = y0 + j, w = (i ? ax : LENS_ONE - ax) * (j ? ay : LENS_ONE - ay);
            const bool in = x >= 0 && x < src_w && y >= 0 && y < src_h;
            sum += w * (in ? tap(x, y) : border);
        }
    return (sum + 512) >> 10;
}

// rule 4: a point of the rectified picture -> the original picture
inline void lens_distort_point(const LensModel &model, double u, double v, double &px, double &py) {
    const LensModel m = lens_resolve(model);
    lens_map(m, u, v, px, py);
}

// rule 4: a point of the original picture -> the rectified picture, with its residual in pixels
inline void lens_undistort_point(const LensModel &model, double px, double py, double &u, double &v, double &residual) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const LensModel m = lens_resolve(model);
    const double xd = (px - m.cx) / m.fx, yd = (py - m.cy) / m.fy;
    double x = xd, y = yd;
    for (int it = 0; it < LENS_ITERS; ++it) {
        const LensTerms t = lens_terms(m, x, y);
        const double nx = xd - t.dx, ny = yd - t.dy;
        x = nx / t.rad;
        y = ny / t.rad;
    }
    const double ux = m.nfx * x, vy = m.nfy * y;
    u = ux + m.ncx;
    v = vy + m.ncy;
    double bx, by;
    lens_map(m, u, v, bx, by);
    const double ex = fabs(bx - px), ey = fabs(by - py);
    const double e = ey > ex ? ey : ex;
    residual = (ex == ex && ey == ey) ? e : INFINITY;
}

}  // namespace rtmodt
