// ground_plane.h -- the one statement of the speed estimator's per-point rules: where a float32 box touches a world ground plane,
// in integer millimetres, and what distance and speed two such points give (csrc/speed.hip keeps the per-track ledger; its header
// states the ledger and alarm rules).  Plain C++, no HIP: the host entry points and the device code of speed.hip and
// tests/native/ground_plane_check.cpp (built under the address and UB sanitizers) all take it from here, and tests/speed_ref.py
// restates it with Python integers and NumPy float64.  A fixed camera and ONE plane per stream: H maps image pixels to world
// millimetres, row-major, [X' Y' W]^T = H [u v 1]^T.
//   1. anchor, float32:  FOOT (u, v) = ((x1 + x2) / 2, y2) -- the point that stands on the ground; CENTRE ((x1 + x2) / 2, (y1 + y2) / 2).
//      A box with a non-finite coordinate has no anchor.
//   2. projection, float64 after widening u and v, in exactly this operation order, every product and sum rounded on its own (no
//      contraction into a fused multiply-add):
//          w  = (H6 u + H7 v) + H8        xn = (H0 u + H1 v) + H2        yn = (H3 u + H4 v) + H5
//          fx = floor(xn / w + 0.5)       fy = floor(yn / w + 0.5)
//      the point is ON the plane iff w > 0 and -2^29 <= fx, fy <= 2^29 (a NaN fails every comparison); X = (int32) fx, Y = (int32) fy.
//      A point off the plane is not sampled; nothing is clamped.
//   3. after the rounding everything is integer: d = isqrt(dx^2 + dy^2), the exact floor square root (|dx|, |dy| <= 2^30, so the sum
//      stays below 2^61); speed in mm/s = d * 1 000 000 / dt_us (floor, int64), saturated to int32.
// The plane is fitted from >= 4 surveyed correspondences by gp_fit_plane (host only): Hartley-normalised DLT with h8 = 1 in the
// normalised frames, the 8 x 8 normal equations solved in float64 by Gaussian elimination with partial pivoting.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef GP_HD
#define GP_HD
#endif

namespace rtmodt {

constexpr int GP_FOOT = 0, GP_CENTRE = 1;
constexpr int32_t GP_LIMIT = 1 << 29;

GP_HD inline bool gp_finite(float v) { return v - v == 0.0f; }
GP_HD inline bool gp_finite64(double v) { return v - v == 0.0; }

// the anchor of a box; false: a coordinate is not finite
GP_HD inline bool gp_anchor(int kind, float x1, float y1, float x2, float y2, float &u, float &v) {
    if (!(gp_finite(x1) && gp_finite(y1) && gp_finite(x2) && gp_finite(y2))) return false;
    u = (x1 + x2) / 2.0f;
    v = kind == GP_CENTRE ? (y1 + y2) / 2.0f : y2;
    return gp_finite(u) && gp_finite(v);                    // (a float32 sum may overflow)
}

// image point -> world millimetres; false: off the plane
GP_HD inline bool gp_project(const double *H, float uf, float vf, int32_t &X, int32_t &Y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double u = (double)uf, v = (double)vf;
    const double a6 = H[6] * u, b6 = H[7] * v, a0 = H[0] * u, b0 = H[1] * v, a3 = H[3] * u, b3 = H[4] * v;
    const double w = (a6 + b6) + H[8];
    const double xn = (a0 + b0) + H[2];
    const double yn = (a3 + b3) + H[5];
    if (!(w > 0.0)) return false;
    const double qx = xn / w, qy = yn / w;
    const double fx = floor(qx + 0.5), fy = floor(qy + 0.5);
    const double lim = (double)GP_LIMIT;
    if (!(fx >= -lim && fx <= lim && fy >= -lim && fy <= lim)) return false;
    X = (int32_t)fx;
    Y = (int32_t)fy;
    return true;
}

// exact floor(sqrt(n)), n >= 0, bit by bit
GP_HD inline int64_t gp_isqrt(int64_t n) {
    uint64_t x = (uint64_t)n, r = 0, bit = 1ull << 62;
    while (bit > x) bit >>= 2;
    while (bit) {
        if (x >= r + bit) { x -= r + bit; r = (r >> 1) + bit; }
        else r >>= 1;
        bit >>= 2;
    }
    return (int64_t)r;
}

GP_HD inline int64_t gp_dist2(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay;
    return dx * dx + dy * dy;
}

// mm over microseconds -> mm/s, saturated; dt_us > 0
GP_HD inline int32_t gp_speed(int64_t d_mm, int64_t dt_us) {
    const int64_t s = d_mm * 1000000 / dt_us;
    return s > 2147483647 ? 2147483647 : (int32_t)s;
}

// det(H) != 0 and every entry finite
inline bool gp_plane_ok(const double *H) {
    for (int i = 0; i < 9; ++i)
        if (!gp_finite64(H[i])) return false;
    const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
    return gp_finite64(det) && det != 0.0;
}

// A x = b, n x n (n <= 8), row-major, partial pivoting; false: a pivot not above `tol` times the largest entry of the matrix
inline bool gp_solve(double *A, double *b, int n, double tol) {
    double big = 0.0;
    for (int i = 0; i < n * n; ++i) big = fabs(A[i]) > big ? fabs(A[i]) : big;
    if (!(big > 0.0)) return false;
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r)
            if (fabs(A[r * n + c]) > fabs(A[p * n + c])) p = r;
        if (!(fabs(A[p * n + c]) > tol * big)) return false;
        if (p != c) {
            for (int k = 0; k < n; ++k) { const double t = A[c * n + k]; A[c * n + k] = A[p * n + k]; A[p * n + k] = t; }
            const double t = b[c]; b[c] = b[p]; b[p] = t;
        }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[r * n + c] / A[c * n + c];
            for (int k = c; k < n; ++k) A[r * n + k] -= f * A[c * n + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double s = b[r];
        for (int k = r + 1; k < n; ++k) s -= A[r * n + k] * b[k];
        b[r] = s / A[r * n + r];
    }
    return true;
}

// the similarity x' = s (x - cx) that moves the centroid to the origin and the mean distance from it to sqrt(2); false: all points equal
inline bool gp_normaliser(const double *xy, int n, bool normalise, double &cx, double &cy, double &s) {
    cx = cy = 0.0;
    s = 1.0;
    if (!normalise) return true;
    for (int i = 0; i < n; ++i) { cx += xy[2 * i]; cy += xy[2 * i + 1]; }
    cx /= n; cy /= n;
    double m = 0.0;
    for (int i = 0; i < n; ++i) m += sqrt((xy[2 * i] - cx) * (xy[2 * i] - cx) + (xy[2 * i + 1] - cy) * (xy[2 * i + 1] - cy));
    m /= n;
    if (!(m > 0.0) || !gp_finite64(m)) return false;
    s = sqrt(2.0) / m;
    return true;
}

// the continuous projection (no rounding), for residuals
inline bool gp_project64(const double *H, double u, double v, double &x, double &y) {
    const double w = (H[6] * u + H[7] * v) + H[8];
    if (!(w > 0.0)) return false;
    x = ((H[0] * u + H[1] * v) + H[2]) / w;
    y = ((H[3] * u + H[4] * v) + H[5]) / w;
    return true;
}

// n >= 4 correspondences image (u, v) -> world (x, y) mm; H_out scaled so that w = 1 at the image centroid; *max_residual_mm = the
// largest distance between a world point and the projection of its image point.  false: degenerate (n < 4, three of four points
// collinear, coincident points, a point at or behind the horizon of the fitted plane).  `normalise` is false only in the tests.
inline bool gp_fit_plane(const double *img_xy, const double *world_xy, int n, double *H_out, double *max_residual_mm, bool normalise = true) {
    if (n < 4 || !img_xy || !world_xy || !H_out) return false;
    for (int i = 0; i < 2 * n; ++i)
        if (!gp_finite64(img_xy[i]) || !gp_finite64(world_xy[i])) return false;
    double icx, icy, is, wcx, wcy, ws;
    if (!gp_normaliser(img_xy, n, normalise, icx, icy, is) || !gp_normaliser(world_xy, n, normalise, wcx, wcy, ws)) return false;
    double M[64] = {0}, r[8] = {0};
    for (int i = 0; i < n; ++i) {
        const double u = is * (img_xy[2 * i] - icx), v = is * (img_xy[2 * i + 1] - icy);
        const double x = ws * (world_xy[2 * i] - wcx), y = ws * (world_xy[2 * i + 1] - wcy);
        const double row[2][8] = {{u, v, 1, 0, 0, 0, -u * x, -v * x}, {0, 0, 0, u, v, 1, -u * y, -v * y}};
        const double rhs[2] = {x, y};
        for (int e = 0; e < 2; ++e)
            for (int a = 0; a < 8; ++a) {
                for (int b = 0; b < 8; ++b) M[a * 8 + b] += row[e][a] * row[e][b];
                r[a] += row[e][a] * rhs[e];
            }
    }
    if (!gp_solve(M, r, 8, normalise ? 1e-12 : 0.0)) return false;        // (in normalised frames a pivot below 1e-12 means collinear points)
    // H = Tw^-1 Hn Ti, with Ti = [is 0 -is icx; 0 is -is icy; 0 0 1] and Tw^-1 = [1/ws 0 wcx; 0 1/ws wcy; 0 0 1]
    const double Hn[9] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], 1.0};
    if (normalise) {                                       // collinear WORLD points fit a plane that collapses onto a line: rank 2
        double big = 1.0;
        for (int i = 0; i < 8; ++i) big = fabs(Hn[i]) > big ? fabs(Hn[i]) : big;
        const double det = Hn[0] * (Hn[4] * Hn[8] - Hn[5] * Hn[7]) - Hn[1] * (Hn[3] * Hn[8] - Hn[5] * Hn[6]) + Hn[2] * (Hn[3] * Hn[7] - Hn[4] * Hn[6]);
        if (!(fabs(det) > 1e-10 * big * big * big)) return false;
    }
    double A[9];
    for (int k = 0; k < 3; ++k) {
        A[3 * k + 0] = Hn[3 * k + 0] * is;
        A[3 * k + 1] = Hn[3 * k + 1] * is;
        A[3 * k + 2] = Hn[3 * k + 2] - is * (Hn[3 * k + 0] * icx + Hn[3 * k + 1] * icy);
    }
    double H[9];
    for (int c = 0; c < 3; ++c) {
        H[c] = A[c] / ws + wcx * A[6 + c];
        H[3 + c] = A[3 + c] / ws + wcy * A[6 + c];
        H[6 + c] = A[6 + c];
    }
    double mu = 0.0, mv = 0.0;
    for (int i = 0; i < n; ++i) { mu += img_xy[2 * i]; mv += img_xy[2 * i + 1]; }
    const double wc = (H[6] * (mu / n) + H[7] * (mv / n)) + H[8];
    if (!gp_finite64(wc) || wc == 0.0) return false;
    for (int i = 0; i < 9; ++i) H[i] /= wc;
    if (!gp_plane_ok(H)) return false;
    double worst = 0.0;
    for (int i = 0; i < n; ++i) {
        double x, y;
        if (!gp_project64(H, img_xy[2 * i], img_xy[2 * i + 1], x, y)) return false;
        const double e = sqrt((x - world_xy[2 * i]) * (x - world_xy[2 * i]) + (y - world_xy[2 * i + 1]) * (y - world_xy[2 * i + 1]));
        if (!gp_finite64(e)) return false;
        worst = e > worst ? e : worst;
    }
    for (int i = 0; i < 9; ++i) H_out[i] = H[i];
    if (max_residual_mm) *max_residual_mm = worst;
    return true;
}

}  // namespace rtmodt
