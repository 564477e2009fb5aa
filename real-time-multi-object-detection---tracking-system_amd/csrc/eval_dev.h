// eval_dev.h -- the float64 device helpers shared by the evaluation kernels (eval.hip: coco_match, mot_pairs; errors.hip:
// detection_errors; hota.hip) and the workgroup scan.
// These translation units are built with -ffp-contract=off and IEEE division: every operation below rounds separately, as NumPy's do.
#pragma once

#include "common.h"

#include <algorithm>
#include <vector>

namespace rtmodt {

#pragma clang fp contract(off)

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int MOT_MAX_ROWS = 1024;

// inclusive scan over the workgroup in thread order; `wtot`: LDS T[EV_WAVES]; two barriers
template <typename T, typename Op>
__device__ __forceinline__ T block_scan(T v, Op op, T *wtot, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    T tot = wtot[0];
    for (int w = 1; w < EV_WAVES; ++w) tot = op(tot, wtot[w]);
    for (int w = 0; w < wave; ++w) v = op(wtot[w], v);
    __syncthreads();
    total = tot;
    return v;
}

// motmetrics' boxiou in float64 (x, y, w, h): the similarity S of hota.hip, and mot_eval's distance d = 1 - S
__device__ __forceinline__ double mot_iou(const double *a, const double *b) {
    const double iw = fmax(fmin(a[0] + a[2], b[0] + b[2]) - fmax(a[0], b[0]), 0.0);
    const double ih = fmax(fmin(a[1] + a[3], b[1] + b[3]) - fmax(a[1], b[1]), 0.0);
    const double i = iw * ih;
    const double u = (a[2] * a[3] + b[2] * b[3]) - i;
    return i == 0.0 ? 0.0 : i / u;
}
__device__ __forceinline__ double mot_dist(const double *a, const double *b) { return 1.0 - mot_iou(a, b); }

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
