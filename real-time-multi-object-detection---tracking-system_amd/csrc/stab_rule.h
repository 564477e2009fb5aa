// stab_rule.h -- the one statement of the stabiliser's rules: how one frame-to-frame similarity moves a stream's camera path, how the
// path is limited, how it becomes four integer coefficients, where an output pixel reads the source frame, and how single points
// travel between the stabilised picture and the raw frame (csrc/stab.hip runs these rules, one lane per stream and one thread per
// run of output pixels).  Plain C++, no HIP: the kernels, the host entry points and tests/native/stab_rule_check.cpp (built under
// the address and UB sanitizers) take it from here, and tests/stab_ref.py restates it with Python floats and integers.  Every
// float64 step is one of + - x / (and a comparison, which is exact), each rounded on its own (no contraction into a fused
// multiply-add), in exactly the order written.  The sampling rule is lens_model.h's rule 3 (lens_sample), included, not restated.
//
// Path of a stream: J = (za, zb, tx, ty), four doubles, in coordinates centred on (cx, cy) = ((w - 1) / 2, (h - 1) / 2).  J maps a
// point of the stabilised picture to the current frame: p_cur = (za x - zb y + tx, zb x + za y + ty).  Fresh or reset: (1, 0, 0, 0).
//   1. input: W = [a, -b, t0; b, a, t1], float32, previous frame -> this frame in full-resolution pixels (what gmc writes), and a
//      valid flag.  Read are W[0] = a, W[3] = b, W[2] = t0, W[5] = t1, widened to double.  The input counts as invalid as well when one
//      of the six floats is not finite or |W0 W4 - W1 W3| < 1e-6.  Invalid: a = 1, b = t0 = t1 = 0, hold = hold + 1, status HOLD.
//      Valid: hold = 0.  Conjugated into centred coordinates once:
//          wtx = ((a cx - b cy) + t0) - cx          wty = ((b cx + a cy) + t1) - cy
//   2. decay, k = 1 - 2^-leak_shift (leak_shift 1..16; 0: no decay, J' = J):
//          za' = 1 + (za - 1) k     zb' = zb k     tx' = tx k     ty' = ty k
//   3. compose J = W o J':
//          za = a za' - b zb'       zb = b za' + a zb'       tx = (a tx' - b ty') + wtx       ty = (b tx' + a ty') + wty
//   4. reset: reset_after > 0 and hold >= reset_after: J = (1, 0, 0, 0), hold = 0, status RESET.
//   5. limits, per component, else: tx, ty into [-max_shift_px, max_shift_px], zb into [-max_rot_milli / 1000, max_rot_milli / 1000],
//      za into [1 - max_zoom_milli / 1000, 1 + max_zoom_milli / 1000]; status CLAMPED when a component moved and the input was valid.
//   6. quantise, with z = crop_zoom_milli / 1000 (>= 1, a fixed enlargement about the centre):
//          sa = za / z     sb = zb / z
//          U = ((tx + cx) - sa cx) + sb cy          V = ((ty + cy) - sb cx) - sa cy
//      and A, B, U, V = round half to even of (sa, sb, U, V) x 65536 as int64: (v + 1.5 x 2^52) - 1.5 x 2^52, exact below 2^51.
//   7. sample, integers only: output pixel (x, y): X = A x - B y + U, Y = B x + A y + V (int64), qx = (X + 1024) >> 11, qy = (Y + 1024)
//      >> 11 (arithmetic; 5 fractional bits), then lens_model.h rule 3 with (qx, qy): four taps, (sum + 512) >> 10, border for a tap
//      off the source.  With every limit at its largest |X| < 2^34, so |qx| < 2^23.
//   8. points, float64, from J (no rounding to Q16): stabilised (x, y) -> source: X = (sa x - sb y) + U, Y = (sb x + sa y) + V; source
//      -> stabilised: d = sa sa + sb sb, ex = X - U, ey = Y - V, x = (sa ex + sb ey) / d, y = (sa ey - sb ex) / d.
#pragma once

#include <cstdint>

#include "lens_model.h"

namespace rtmodt {

constexpr int STAB_OK = 0, STAB_HOLD = 1, STAB_CLAMPED = 2, STAB_RESET = 3;
constexpr int STAB_MAX_DIM = 16384, STAB_MAX_LEAK = 16, STAB_MAX_SHIFT = 16384, STAB_MAX_MILLI = 500, STAB_MAX_CROP = 8000, STAB_MAX_HOLD = 1 << 30;
constexpr double STAB_ROUND = 6755399441055744.0;          // 1.5 x 2^52
constexpr double STAB_MIN_DET = 1e-6;

struct StabRule {                                          // the fields of rtmodt_stab_cfg the rule reads
    int h, w, leak_shift, max_shift_px, max_rot_milli, max_zoom_milli, crop_zoom_milli, reset_after;
};
struct StabPath { double za, zb, tx, ty; };
struct StabCoef { int64_t A, B, U, V; };
struct StabAffine { double sa, sb, U, V; };                // rule 6 before the rounding: what the point helpers use

inline bool stab_rule_ok(const StabRule &r) {
    return r.h >= 1 && r.w >= 1 && r.h <= STAB_MAX_DIM && r.w <= STAB_MAX_DIM && r.leak_shift >= 0 && r.leak_shift <= STAB_MAX_LEAK && r.max_shift_px >= 0 &&
           r.max_shift_px <= STAB_MAX_SHIFT && r.max_rot_milli >= 0 && r.max_rot_milli <= STAB_MAX_MILLI && r.max_zoom_milli >= 0 &&
           r.max_zoom_milli <= STAB_MAX_MILLI && r.crop_zoom_milli >= 1000 && r.crop_zoom_milli <= STAB_MAX_CROP && r.reset_after >= 0 &&
           r.reset_after <= STAB_MAX_HOLD;
}

// rule 1's test of the six floats
inline bool stab_input_ok(const float *W) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    for (int k = 0; k < 6; ++k)
        if (!lens_finite((double)W[k])) return false;
    const double p = (double)W[0] * (double)W[4], q = (double)W[1] * (double)W[3], det = p - q;
    return det >= STAB_MIN_DET || det <= -STAB_MIN_DET;
}

inline bool stab_clamp(double &v, double lo, double hi) {
    if (v > hi) { v = hi; return true; }
    if (v < lo) { v = lo; return true; }
    return false;
}

// a path inside rule 5's limits (what load_state accepts: the bound of rule 7 rests on it); a NaN fails
inline bool stab_path_ok(const StabRule &r, const StabPath &j) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double M = (double)r.max_shift_px, R = (double)r.max_rot_milli / 1000.0, Z = (double)r.max_zoom_milli / 1000.0;
    const double lo = 1.0 - Z, hi = 1.0 + Z;
    return j.tx >= -M && j.tx <= M && j.ty >= -M && j.ty <= M && j.zb >= -R && j.zb <= R && j.za >= lo && j.za <= hi;
}

// rules 1 to 5: W == nullptr is the identity; returns the status
inline int stab_step(const StabRule &r, StabPath &j, int32_t &hold, const float *W, bool valid) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double cx = (double)(r.w - 1) / 2.0, cy = (double)(r.h - 1) / 2.0;
    double a = 1.0, b = 0.0, t0 = 0.0, t1 = 0.0;
    const bool ok = valid && (!W || stab_input_ok(W));
    if (ok && W) { a = (double)W[0]; b = (double)W[3]; t0 = (double)W[2]; t1 = (double)W[5]; }
    hold = ok ? 0 : (hold < STAB_MAX_HOLD ? hold + 1 : hold);
    const double m0 = a * cx, m1 = b * cy, d0 = m0 - m1, e0 = d0 + t0, wtx = e0 - cx;
    const double m2 = b * cx, m3 = a * cy, d1 = m2 + m3, e1 = d1 + t1, wty = e1 - cy;
    double za = j.za, zb = j.zb, tx = j.tx, ty = j.ty;
    if (r.leak_shift > 0) {
        const double k = 1.0 - 1.0 / (double)(1 << r.leak_shift);
        const double g = za - 1.0, gk = g * k;
        za = 1.0 + gk; zb = zb * k; tx = tx * k; ty = ty * k;
    }
    const double p0 = a * za, p1 = b * zb, p2 = b * za, p3 = a * zb;
    const double q0 = a * tx, q1 = b * ty, q2 = b * tx, q3 = a * ty;
    const double r0 = q0 - q1, r1 = q2 + q3;
    j.za = p0 - p1; j.zb = p2 + p3; j.tx = r0 + wtx; j.ty = r1 + wty;
    if (r.reset_after > 0 && hold >= r.reset_after) {
        j.za = 1.0; j.zb = 0.0; j.tx = 0.0; j.ty = 0.0;
        hold = 0;
        return STAB_RESET;
    }
    const double M = (double)r.max_shift_px, R = (double)r.max_rot_milli / 1000.0, Z = (double)r.max_zoom_milli / 1000.0;
    const double lo = 1.0 - Z, hi = 1.0 + Z;
    bool clamped = stab_clamp(j.tx, -M, M);
    clamped = stab_clamp(j.ty, -M, M) || clamped;
    clamped = stab_clamp(j.zb, -R, R) || clamped;
    clamped = stab_clamp(j.za, lo, hi) || clamped;
    return !ok ? STAB_HOLD : clamped ? STAB_CLAMPED : STAB_OK;
}

// rule 6 before the rounding
inline StabAffine stab_affine(const StabRule &r, const StabPath &j) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double cx = (double)(r.w - 1) / 2.0, cy = (double)(r.h - 1) / 2.0, z = (double)r.crop_zoom_milli / 1000.0;
    StabAffine f;
    f.sa = j.za / z; f.sb = j.zb / z;
    const double u0 = f.sa * cx, u1 = f.sb * cy, u2 = j.tx + cx, u3 = u2 - u0;
    f.U = u3 + u1;
    const double v0 = f.sb * cx, v1 = f.sa * cy, v2 = j.ty + cy, v3 = v2 - v0;
    f.V = v3 - v1;
    return f;
}

inline int64_t stab_q16(double v) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double s = v * 65536.0, t = s + STAB_ROUND, u = t - STAB_ROUND;
    return (int64_t)u;
}

// rule 6
inline StabCoef stab_quantise(const StabRule &r, const StabPath &j) {
    const StabAffine f = stab_affine(r, j);
    StabCoef c;
    c.A = stab_q16(f.sa); c.B = stab_q16(f.sb); c.U = stab_q16(f.U); c.V = stab_q16(f.V);
    return c;
}

// rule 7's position of output pixel (x, y): X, Y in Q16 (one pixel further along a row is X + A, Y + B), then 5 fractional bits
inline void stab_xy(const StabCoef &c, int x, int y, int64_t &X, int64_t &Y) {
    X = c.A * x - c.B * y + c.U;
    Y = c.B * x + c.A * y + c.V;
}
inline int32_t stab_q5(int64_t X) { return (int32_t)((X + 1024) >> 11); }
inline void stab_position(const StabCoef &c, int x, int y, int32_t &qx, int32_t &qy) {
    int64_t X, Y;
    stab_xy(c, x, y, X, Y);
    qx = stab_q5(X);
    qy = stab_q5(Y);
}

// rule 7 on one channel of one output pixel; tap(x, y) is only called inside the source
template <typename Tap> inline int stab_sample(const StabCoef &c, int x, int y, int h, int w, int border, Tap tap) {
    int32_t qx, qy;
    stab_position(c, x, y, qx, qy);
    return lens_sample(qx, qy, h, w, border, tap);
}

// rule 8: to_source != 0: a point of the stabilised picture -> the raw frame; else the inverse
inline void stab_point(const StabRule &r, const StabPath &j, bool to_source, double px, double py, double &ox, double &oy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const StabAffine f = stab_affine(r, j);
    if (to_source) {
        const double a0 = f.sa * px, a1 = f.sb * py, a2 = a0 - a1, b0 = f.sb * px, b1 = f.sa * py, b2 = b0 + b1;
        ox = a2 + f.U; oy = b2 + f.V;
        return;
    }
    const double s0 = f.sa * f.sa, s1 = f.sb * f.sb, d = s0 + s1, ex = px - f.U, ey = py - f.V;
    const double n0 = f.sa * ex, n1 = f.sb * ey, n2 = n0 + n1, n3 = f.sa * ey, n4 = f.sb * ex, n5 = n3 - n4;
    ox = n2 / d; oy = n5 / d;
}

}  // namespace rtmodt
