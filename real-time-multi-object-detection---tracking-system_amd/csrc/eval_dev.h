// eval_dev.h -- the float64 device helpers shared by the evaluation kernels (eval.hip: coco_match; errors.hip: detection_errors).
// Both translation units are built with -ffp-contract=off and IEEE division: every operation below rounds separately, as NumPy's do.
#pragma once

#include "common.h"

namespace rtmodt {

#pragma clang fp contract(off)

// pycocotools' bbIou (maskApi.c): det d, GT g as x, y, w, h; the union of a crowd GT is the detection's area
__device__ __forceinline__ double coco_iou(const double4 d, const double4 g, bool crowd) {
    double w = fmin(d.x + d.z, g.x + g.z) - fmax(d.x, g.x);
    if (w <= 0) return 0.0;
    double h = fmin(d.y + d.w, g.y + g.w) - fmax(d.y, g.y);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double da = d.z * d.w;
    const double u = crowd ? da : da + g.z * g.w - i;
    return i / u;
}

// an order-preserving unsigned image of a float64 (-0.0 folded into +0.0; NaN is rejected by the host)
__device__ __forceinline__ uint64_t score_key(double s) {
    if (s == 0.0) s = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

}  // namespace rtmodt
