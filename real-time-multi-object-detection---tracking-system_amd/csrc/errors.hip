// errors.hip -- what a detector gets wrong: every detection and every ground truth of an image set typed by its error
// (TECHNICAL_DESIGN_DOCUMENT.md D.5: localization, classification, duplicate, background false positive, missed), the counts
// clustered by class, by object size and by image region, and the confusion matrix that D.6 step 4 plots (the reference has only
// src/evaluation/metrics.py:110-123, build_confusion_matrix on already-matched label pairs, and nothing that produces the pairs).
// PARITY UNPINNED: neither tidecv nor ultralytics is installed anywhere this runs; the rules are INTEGRATION.md section 14,
// tests/errors_ref.py states them in NumPy loops and the GPU tests require equality with it.
//
// detection_errors: ONE launch, one 256-thread workgroup per image, all of the image's categories together, float64 IoU
// (eval_dev.h: coco_iou, the function coco_match uses).  In order:
//   rank     the detections with score >= conf_thr ranked by (-score, file index) on their order-preserving score keys (a
//            count of the keys ahead, as coco_match does); the first max_det are kept, every other row is NOT_EVALUATED
//   step 2   (hoisted: it reads no matching state) per kept detection the best non-crowd GT of its own category and of the
//            other categories (first GT on equal IoU) -> the type it takes if step 1 leaves it unmatched
//   step 1   class-aware greedy matching, serial in rank on wave 0, the GTs spread over its lanes: a wave max-reduction of
//            (non-crowd, IoU, GT position), the LAST GT on equal IoU -> TP / IGNORED
//   step 3   GT states; a LOCALIZATION / CLASSIFICATION detection marks the GT it points at as covered
//   cm       the class-agnostic one-to-one matching in the total order (IoU descending, rank ascending, GT ascending): the
//            greedy pass over that order takes exactly the LOCALLY DOMINANT pairs round by round -- a pair that is the best
//            remaining one of both its detection and its GT.  Each side caches its best free partner and looks again only
//            when that partner was taken by somebody else; the best remaining pair of the image is always dominant, so every
//            round takes at least one pair and the loop ends after at most min(D, G) + 1 rounds, at once when there is no pair
//   counts   by_size in LDS first (21 cells that every image hits), everything else (sparse per image) straight to the global
//            int64 histograms with integer atomics: sums of integers, the same whatever the arrival order
//
// Every loop is sized by the image's own rows: an image without rows, or with crowd GTs only, falls through all of them.
// Built with -ffp-contract=off and IEEE division, like eval.o.
#include "common.h"
#include "eval_dev.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace rtmodt {

#pragma clang fp contract(off)

constexpr int ER_THREADS = 256;
constexpr int ER_MAX_GT = 1024, ER_MAX_DT = 4096, ER_MAX_DET = 1024, ER_MAX_GRID = 64;
constexpr int ER_NCOL = 7;                                 // TP, LOCALIZATION, CLASSIFICATION, BOTH, DUPLICATE, BACKGROUND, MISSED
enum { ET_TP = 0, ET_LOC = 1, ET_CLS = 2, ET_BOTH = 3, ET_DUP = 4, ET_BKG = 5, ET_MISSED_COL = 6, ET_IGNORED = 6, ET_NOT_EVALUATED = 7 };
enum { EG_CROWD = 0, EG_MATCHED = 1, EG_MISSED_COVERED = 2, EG_MISSED = 3 };

struct ErrArgs {
    double conf_thr, iou_fg, iou_bg, cm_iou;               // the IoU thresholds already min(t, 1 - 1e-10)
    int max_det, gx, gy, K;
    const double *img_wh;                                  // [n_img][2]
    const int32_t *gt_start, *dt_start;                    // [n_img + 1]
    const int32_t *gt_cat, *gt_crowd, *dt_cat;
    const double *gt_box, *gt_area, *dt_box, *dt_score;
    int32_t *dt_type, *dt_gt, *gt_state, *gt_dt;           // per row; dt_gt / gt_dt are row indices of the call's arrays
    unsigned long long *by_class, *by_size, *by_cell, *missed_uncovered, *cm, *cm_dropped;
    int max_gt, max_dt, max_keep;                          // LDS sizing: the largest image
};

// LDS of detection_errors.  One carve for both sides: the host sizes the launch with err_carve(nullptr, ...).end.
struct ErrSmem {
    double4 *gbox;                 // [max_gt]
    double4 *dbox;                 // [max_keep] by rank
    unsigned long long *key;       // [max_dt] score keys by file position; 0 = below conf_thr
    int *order;                    // [max_keep] rank -> file position in the image
    int *dcat;                     // [max_keep]
    int *dtype;                    // [max_keep] step 2's type, then the final one
    int *dgt;                      // [max_keep] the GT that decided the type (-1 none)
    int *cmd;                      // [max_keep] cm partner (GT position), -1 free
    int *bestg;                    // [max_keep] cached best free GT: -1 look again, -2 none left
    int *gcat;                     // [max_gt]
    int *gdt;                      // [max_gt] step 1's detection (rank), -1 unmatched
    int *cmg;                      // [max_gt] cm partner (rank), -1 free
    int *bestd;                    // [max_gt]
    int *size_hist;                // [3][ER_NCOL]
    unsigned char *gcrowd;         // [max_gt]
    unsigned char *gcov;           // [max_gt] pointed at by a LOCALIZATION / CLASSIFICATION detection
    uintptr_t end;
};
__host__ __device__ inline ErrSmem err_carve(unsigned char *base, int max_gt, int max_dt, int max_keep) {
    ErrSmem S;
    S.gbox = (double4 *)base;
    S.dbox = S.gbox + max_gt;
    S.key = (unsigned long long *)(S.dbox + max_keep);
    S.order = (int *)(S.key + max_dt);
    S.dcat = S.order + max_keep;
    S.dtype = S.dcat + max_keep;
    S.dgt = S.dtype + max_keep;
    S.cmd = S.dgt + max_keep;
    S.bestg = S.cmd + max_keep;
    S.gcat = S.bestg + max_keep;
    S.gdt = S.gcat + max_gt;
    S.cmg = S.gdt + max_gt;
    S.bestd = S.cmg + max_gt;
    S.size_hist = S.bestd + max_gt;
    S.gcrowd = (unsigned char *)(S.size_hist + 3 * ER_NCOL);
    S.gcov = S.gcrowd + max_gt;
    S.end = (uintptr_t)(S.gcov + max_gt);
    return S;
}
static size_t errors_smem(int max_gt, int max_dt, int max_keep) { return (size_t)err_carve(nullptr, max_gt, max_dt, max_keep).end + 16; }

__device__ __forceinline__ int size_bin(double area) { return area < 1024.0 ? 0 : (area < 9216.0 ? 1 : 2); }

// clamp((int)floor(((x + 0.5 * w) * n) / W), 0, n - 1), clamped before the conversion (boxes are finite, W > 0)
__device__ __forceinline__ int grid_index(double x, double w, int n, double W) {
    const double f = floor(((x + 0.5 * w) * (double)n) / W);
    if (!(f > 0.0)) return 0;
    return f >= (double)(n - 1) ? n - 1 : (int)f;
}

__global__ __launch_bounds__(ER_THREADS) void detection_errors(ErrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ErrSmem S = err_carve(smem, a.max_gt, a.max_dt, a.max_keep);
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = a.gt_start[img], G = a.gt_start[img + 1] - g0;
    const int d0 = a.dt_start[img], Draw = a.dt_start[img + 1] - d0;
    __shared__ int s_nel;

    if (tid == 0) s_nel = 0;
    for (int i = tid; i < 3 * ER_NCOL; i += ER_THREADS) S.size_hist[i] = 0;
    __syncthreads();
    int nel = 0;
    for (int i = tid; i < Draw; i += ER_THREADS) {
        const double s = a.dt_score[d0 + i];
        const bool el = s >= a.conf_thr;
        S.key[i] = el ? score_key(s) : 0ull;               // (a key is never 0: the key of -inf is 0x000f...)
        nel += el;
    }
    for (int g = tid; g < G; g += ER_THREADS) {
        const double *b = a.gt_box + (size_t)(g0 + g) * 4;
        S.gbox[g] = double4{b[0], b[1], b[2], b[3]};
        S.gcat[g] = a.gt_cat[g0 + g];
        S.gcrowd[g] = a.gt_crowd[g0 + g] != 0;
        S.gdt[g] = -1; S.cmg[g] = -1; S.bestd[g] = -1; S.gcov[g] = 0;
    }
    if (nel) atomicAdd(&s_nel, nel);
    __syncthreads();
    const int D = min(s_nel, a.max_det);                   // kept detections
    // ---- rank by (-score, file index) among the rows at or above conf_thr ----
    for (int i = tid; i < Draw; i += ER_THREADS) {
        const unsigned long long k = S.key[i];
        int r = D;
        if (k != 0ull) {
            r = 0;
            for (int j = 0; j < Draw; ++j) {
                const unsigned long long t = S.key[j];
                r += (t > k) || (t == k && j < i);
            }
        }
        if (r < D) {
            S.order[r] = i;
        } else {
            a.dt_type[d0 + i] = ET_NOT_EVALUATED;
            a.dt_gt[d0 + i] = -1;
        }
    }
    __syncthreads();
    for (int r = tid; r < D; r += ER_THREADS) {
        const int i = S.order[r];
        const double *b = a.dt_box + (size_t)(d0 + i) * 4;
        S.dbox[r] = double4{b[0], b[1], b[2], b[3]};
        S.dcat[r] = a.dt_cat[d0 + i];
        S.cmd[r] = -1; S.bestg[r] = -1;
    }
    __syncthreads();
    // ---- step 2 (no detection depends on another): the type of a detection that step 1 leaves unmatched ----
    for (int r = tid; r < D; r += ER_THREADS) {
        const double4 db = S.dbox[r];
        const int c = S.dcat[r];
        double sv = 0.0, ov = 0.0;
        int si = -1, oi = -1;
        for (int g = 0; g < G; ++g) {
            if (S.gcrowd[g]) continue;
            const double v = coco_iou(db, S.gbox[g], false);
            if (S.gcat[g] == c) {
                if (si < 0 || v > sv) { sv = v; si = g; }
            } else {
                if (oi < 0 || v > ov) { ov = v; oi = g; }
            }
        }
        int ty, gi;
        if (sv >= a.iou_fg) { ty = ET_DUP; gi = si; }
        else if (ov >= a.iou_fg) { ty = ET_CLS; gi = oi; }
        else if (sv >= a.iou_bg) { ty = ET_LOC; gi = si; }
        else if (ov >= a.iou_bg) { ty = ET_BOTH; gi = oi; }
        else { ty = ET_BKG; gi = -1; }
        S.dtype[r] = ty;
        S.dgt[r] = gi;
    }
    __syncthreads();
    // ---- step 1: class-aware matching, serial in rank, on wave 0 ----
    if (wave == 0) {
        for (int r = 0; r < D; ++r) {
            const double4 db = S.dbox[r];
            const int c = S.dcat[r];
            int bn = 0, bg = -1;                           // best key (non-crowd, IoU, GT position); -1 = none
            double bv = 0.0;
            for (int g = lane; g < G; g += 64) {
                if (S.gcat[g] != c) continue;
                const bool crowd = S.gcrowd[g];
                if (!crowd && S.gdt[g] >= 0) continue;
                const double v = coco_iou(db, S.gbox[g], crowd);
                if (v < a.iou_fg) continue;
                const int n = !crowd;
                if (bg < 0 || n > bn || (n == bn && (v > bv || (v == bv && g > bg)))) { bn = n; bv = v; bg = g; }
            }
            for (int s = 32; s >= 1; s >>= 1) {
                const int on = __shfl_xor(bn, s), og = __shfl_xor(bg, s);
                const double ov = __shfl_xor(bv, s);
                const bool take = og >= 0 && (bg < 0 || on > bn || (on == bn && (ov > bv || (ov == bv && og > bg))));
                if (take) { bn = on; bv = ov; bg = og; }
            }
            if (lane == 0 && bg >= 0) {
                if (bn) { S.gdt[bg] = r; S.dtype[r] = ET_TP; }
                else S.dtype[r] = ET_IGNORED;
                S.dgt[r] = bg;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    // ---- step 3: covered GTs ----
    for (int r = tid; r < D; r += ER_THREADS) {
        const int ty = S.dtype[r];
        if ((ty == ET_LOC || ty == ET_CLS) && S.dgt[r] >= 0) S.gcov[S.dgt[r]] = 1;
    }
    // ---- cm: class-agnostic one-to-one matching, the locally dominant pairs round by round ----
    for (;;) {
        int have = 0;
        for (int r = tid; r < D; r += ER_THREADS) {
            if (S.cmd[r] >= 0) continue;
            if (S.bestg[r] == -1) {
                const double4 db = S.dbox[r];
                double bv = 0.0;
                int bg = -2;
                for (int g = 0; g < G; ++g) {
                    if (S.gcrowd[g] || S.cmg[g] >= 0) continue;
                    const double v = coco_iou(db, S.gbox[g], false);
                    if (v >= a.cm_iou && (bg < 0 || v > bv)) { bv = v; bg = g; }
                }
                S.bestg[r] = bg;
            }
            have |= S.bestg[r] >= 0;
        }
        for (int g = tid; g < G; g += ER_THREADS) {
            if (S.gcrowd[g] || S.cmg[g] >= 0 || S.bestd[g] != -1) continue;
            const double4 gb = S.gbox[g];
            double bv = 0.0;
            int br = -2;
            for (int r = 0; r < D; ++r) {
                if (S.cmd[r] >= 0) continue;
                const double v = coco_iou(S.dbox[r], gb, false);
                if (v >= a.cm_iou && (br < 0 || v > bv)) { bv = v; br = r; }
            }
            S.bestd[g] = br;
        }
        if (!__syncthreads_or(have)) break;
        for (int r = tid; r < D; r += ER_THREADS) {
            const int g = S.bestg[r];
            if (S.cmd[r] < 0 && g >= 0 && S.bestd[g] == r) { S.cmd[r] = g; S.cmg[g] = r; }
        }
        __syncthreads();
        for (int r = tid; r < D; r += ER_THREADS)
            if (S.cmd[r] < 0 && S.bestg[r] >= 0 && S.cmg[S.bestg[r]] >= 0) S.bestg[r] = -1;
        for (int g = tid; g < G; g += ER_THREADS)
            if (S.cmg[g] < 0 && S.bestd[g] >= 0 && S.cmd[S.bestd[g]] >= 0) S.bestd[g] = -1;
        __syncthreads();
    }
    // ---- per-row outputs and counts ----
    const double W = a.img_wh[2 * (size_t)img], H = a.img_wh[2 * (size_t)img + 1];
    const size_t K1 = (size_t)a.K + 1;
    for (int r = tid; r < D; r += ER_THREADS) {
        const int row = d0 + S.order[r], ty = S.dtype[r], c = S.dcat[r];
        const double4 db = S.dbox[r];
        a.dt_type[row] = ty;
        a.dt_gt[row] = S.dgt[r] >= 0 ? g0 + S.dgt[r] : -1;
        if (ty <= ET_BKG) {
            const int ix = grid_index(db.x, db.z, a.gx, W), iy = grid_index(db.y, db.w, a.gy, H);
            atomicAdd(&a.by_class[(size_t)c * ER_NCOL + ty], 1ull);
            atomicAdd(&a.by_cell[((size_t)iy * a.gx + ix) * ER_NCOL + ty], 1ull);
            atomicAdd(&S.size_hist[size_bin(db.z * db.w) * ER_NCOL + ty], 1);
        }
        if (S.cmd[r] >= 0) {
            atomicAdd(&a.cm[(size_t)S.gcat[S.cmd[r]] * K1 + c], 1ull);
        } else {
            bool drop = false;                             // a free detection on a crowd GT of its own category is dropped
            for (int g = 0; g < G && !drop; ++g)
                drop = S.gcrowd[g] && S.gcat[g] == c && coco_iou(db, S.gbox[g], true) >= a.cm_iou;
            if (drop) atomicAdd(&a.cm_dropped[c], 1ull);
            else atomicAdd(&a.cm[(size_t)a.K * K1 + c], 1ull);
        }
    }
    for (int g = tid; g < G; g += ER_THREADS) {
        const int row = g0 + g, c = S.gcat[g];
        int st;
        if (S.gcrowd[g]) st = EG_CROWD;
        else if (S.gdt[g] >= 0) st = EG_MATCHED;
        else st = S.gcov[g] ? EG_MISSED_COVERED : EG_MISSED;
        a.gt_state[row] = st;
        a.gt_dt[row] = S.gdt[g] >= 0 ? d0 + S.order[S.gdt[g]] : -1;
        if (st == EG_MISSED_COVERED || st == EG_MISSED) {
            const double4 gb = S.gbox[g];
            const int ix = grid_index(gb.x, gb.z, a.gx, W), iy = grid_index(gb.y, gb.w, a.gy, H);
            atomicAdd(&a.by_class[(size_t)c * ER_NCOL + ET_MISSED_COL], 1ull);
            atomicAdd(&a.by_cell[((size_t)iy * a.gx + ix) * ER_NCOL + ET_MISSED_COL], 1ull);
            atomicAdd(&S.size_hist[size_bin(a.gt_area[row]) * ER_NCOL + ET_MISSED_COL], 1);
            if (st == EG_MISSED) atomicAdd(&a.missed_uncovered[c], 1ull);
        }
        if (!S.gcrowd[g] && S.cmg[g] < 0) atomicAdd(&a.cm[(size_t)c * K1 + a.K], 1ull);
    }
    __syncthreads();
    for (int i = tid; i < 3 * ER_NCOL; i += ER_THREADS)
        if (S.size_hist[i]) atomicAdd(&a.by_size[i], (unsigned long long)S.size_hist[i]);
}

}  // namespace rtmodt

using namespace rtmodt;

extern "C" int rtmodt_detection_errors(int device, const rtmodt_error_params *params, int K, int n_img, const double *img_wh,
                                       const int32_t *gt_start, const int32_t *gt_cat, const double *gt_box, const double *gt_area,
                                       const int32_t *gt_crowd, const int32_t *dt_start, const int32_t *dt_cat, const double *dt_box,
                                       const double *dt_score, int32_t *dt_type, int32_t *dt_gt, int32_t *gt_state, int32_t *gt_dt,
                                       int64_t *by_class, int64_t *by_size, int64_t *by_cell, int64_t *missed_uncovered, int64_t *cm,
                                       int64_t *cm_dropped) {
    // ---- every check comes before the first HIP call ----
    RT_CHECK(params, RTMODT_E_INVALID, "detection_errors: null params");
    RT_CHECK(by_class && by_size && by_cell && missed_uncovered && cm && cm_dropped, RTMODT_E_INVALID, "detection_errors: null histogram output");
    const rtmodt_error_params &p = *params;
    RT_CHECK(p.conf_thr == p.conf_thr, RTMODT_E_INVALID, "detection_errors: conf_thr is NaN");
    RT_CHECK(p.iou_fg == p.iou_fg, RTMODT_E_INVALID, "detection_errors: iou_fg is NaN");
    RT_CHECK(p.iou_bg == p.iou_bg, RTMODT_E_INVALID, "detection_errors: iou_bg is NaN");
    RT_CHECK(p.cm_iou == p.cm_iou, RTMODT_E_INVALID, "detection_errors: cm_iou is NaN");
    RT_CHECK(p.iou_bg <= p.iou_fg, RTMODT_E_INVALID, "detection_errors: iou_bg %g > iou_fg %g", p.iou_bg, p.iou_fg);
    RT_CHECK(p.max_det >= 1 && p.max_det <= ER_MAX_DET, RTMODT_E_INVALID, "detection_errors: max_det %d outside 1..%d", p.max_det, ER_MAX_DET);
    RT_CHECK(p.grid_x >= 1 && p.grid_x <= ER_MAX_GRID && p.grid_y >= 1 && p.grid_y <= ER_MAX_GRID, RTMODT_E_INVALID,
             "detection_errors: grid %d x %d outside 1..%d", p.grid_x, p.grid_y, ER_MAX_GRID);
    RT_CHECK(K >= 1 && n_img >= 0, RTMODT_E_INVALID, "detection_errors: K %d, images %d", K, n_img);
    if (n_img) RT_CHECK(img_wh && gt_start && dt_start, RTMODT_E_INVALID, "detection_errors: null image arrays");
    if (n_img) RT_CHECK(gt_start[0] == 0 && dt_start[0] == 0, RTMODT_E_INVALID, "detection_errors: CSR must start at 0");
    int max_gt = 1, max_dt = 1;
    for (int i = 0; i < n_img; ++i) {
        const int ng = gt_start[i + 1] - gt_start[i], nd = dt_start[i + 1] - dt_start[i];
        RT_CHECK(ng >= 0 && nd >= 0, RTMODT_E_INVALID, "detection_errors: image %d: malformed CSR", i);
        RT_CHECK(img_wh[2 * i] > 0 && img_wh[2 * i + 1] > 0 && std::isfinite(img_wh[2 * i]) && std::isfinite(img_wh[2 * i + 1]), RTMODT_E_INVALID,
                 "detection_errors: image %d: width %g, height %g must be > 0", i, img_wh[2 * i], img_wh[2 * i + 1]);
        RT_CHECK(ng <= ER_MAX_GT, RTMODT_E_CAPACITY, "detection_errors: image %d holds %d GTs > %d", i, ng, ER_MAX_GT);
        RT_CHECK(nd <= ER_MAX_DT, RTMODT_E_CAPACITY, "detection_errors: image %d holds %d detections > %d", i, nd, ER_MAX_DT);
        max_gt = std::max(max_gt, ng);
        max_dt = std::max(max_dt, nd);
    }
    const int n_gt = n_img ? gt_start[n_img] : 0, n_dt = n_img ? dt_start[n_img] : 0;
    if (n_gt) RT_CHECK(gt_cat && gt_box && gt_area && gt_crowd && gt_state && gt_dt, RTMODT_E_INVALID, "detection_errors: null GT arrays");
    if (n_dt) RT_CHECK(dt_cat && dt_box && dt_score && dt_type && dt_gt, RTMODT_E_INVALID, "detection_errors: null detection arrays");
    for (int g = 0; g < n_gt; ++g) {
        RT_CHECK(gt_cat[g] >= 0 && gt_cat[g] < K, RTMODT_E_INVALID, "detection_errors: GT row %d: category index %d outside 0..%d", g, gt_cat[g], K - 1);
        RT_CHECK(gt_area[g] == gt_area[g], RTMODT_E_INVALID, "detection_errors: GT row %d has a NaN area", g);
        for (int q = 0; q < 4; ++q)
            RT_CHECK(std::isfinite(gt_box[4 * (size_t)g + q]), RTMODT_E_INVALID, "detection_errors: GT row %d has a NaN or infinite box", g);
    }
    for (int d = 0; d < n_dt; ++d) {
        RT_CHECK(dt_cat[d] >= 0 && dt_cat[d] < K, RTMODT_E_INVALID, "detection_errors: detection row %d: category index %d outside 0..%d", d, dt_cat[d],
                 K - 1);
        RT_CHECK(dt_score[d] == dt_score[d], RTMODT_E_INVALID, "detection_errors: detection row %d has a NaN score", d);
        for (int q = 0; q < 4; ++q)
            RT_CHECK(std::isfinite(dt_box[4 * (size_t)d + q]), RTMODT_E_INVALID, "detection_errors: detection row %d has a NaN or infinite box", d);
    }
    const int max_keep = std::min(max_dt, p.max_det);
    const size_t smem = errors_smem(max_gt, max_dt, max_keep);
    RT_CHECK(smem <= 160 * 1024, RTMODT_E_CAPACITY, "detection_errors: the largest image (%d GTs, %d detections) needs %zu B of LDS", max_gt, max_dt, smem);
    const size_t n_class = (size_t)K * ER_NCOL, n_size = 3 * ER_NCOL, n_cell = (size_t)p.grid_x * p.grid_y * ER_NCOL, n_cm = ((size_t)K + 1) * (K + 1);

    RT_HIP(hipSetDevice(device));
    DevBufs B;
    ErrArgs ea{};
    ea.conf_thr = p.conf_thr;
    ea.iou_fg = std::fmin(p.iou_fg, 1.0 - 1e-10); ea.iou_bg = std::fmin(p.iou_bg, 1.0 - 1e-10); ea.cm_iou = std::fmin(p.cm_iou, 1.0 - 1e-10);
    ea.max_det = p.max_det; ea.gx = p.grid_x; ea.gy = p.grid_y; ea.K = K;
    ea.max_gt = max_gt; ea.max_dt = max_dt; ea.max_keep = max_keep;
    double *d_wh, *d_gbox, *d_garea, *d_dbox, *d_dsc;
    int32_t *d_gs, *d_ds, *d_gcat, *d_crowd, *d_dcat;
    RT_TRY(B.up(&d_wh, img_wh, (size_t)n_img * 2));
    RT_TRY(B.up(&d_gs, gt_start, n_img ? n_img + 1 : 0)); RT_TRY(B.up(&d_ds, dt_start, n_img ? n_img + 1 : 0));
    RT_TRY(B.up(&d_gcat, gt_cat, n_gt)); RT_TRY(B.up(&d_crowd, gt_crowd, n_gt));
    RT_TRY(B.up(&d_gbox, gt_box, (size_t)n_gt * 4)); RT_TRY(B.up(&d_garea, gt_area, n_gt));
    RT_TRY(B.up(&d_dcat, dt_cat, n_dt)); RT_TRY(B.up(&d_dbox, dt_box, (size_t)n_dt * 4)); RT_TRY(B.up(&d_dsc, dt_score, n_dt));
    ea.img_wh = d_wh; ea.gt_start = d_gs; ea.dt_start = d_ds; ea.gt_cat = d_gcat; ea.gt_crowd = d_crowd; ea.gt_box = d_gbox;
    ea.gt_area = d_garea; ea.dt_cat = d_dcat; ea.dt_box = d_dbox; ea.dt_score = d_dsc;
    RT_TRY(B.alloc(&ea.dt_type, n_dt)); RT_TRY(B.alloc(&ea.dt_gt, n_dt)); RT_TRY(B.alloc(&ea.gt_state, n_gt)); RT_TRY(B.alloc(&ea.gt_dt, n_gt));
    // one zeroed block for every histogram: by_class, by_size, by_cell, missed_uncovered, cm, cm_dropped
    unsigned long long *d_hist;
    const size_t n_hist = n_class + n_size + n_cell + (size_t)K + n_cm + (size_t)K;
    RT_TRY(B.alloc(&d_hist, n_hist));
    RT_HIP(hipMemset(d_hist, 0, n_hist * sizeof(*d_hist)));
    ea.by_class = d_hist; ea.by_size = ea.by_class + n_class; ea.by_cell = ea.by_size + n_size; ea.missed_uncovered = ea.by_cell + n_cell;
    ea.cm = ea.missed_uncovered + K; ea.cm_dropped = ea.cm + n_cm;
    if (n_img) {
        static DynLdsSeen seen;
        RT_TRY(raise_dynamic_lds((const void *)detection_errors, smem, seen));
        hipLaunchKernelGGL(detection_errors, dim3(n_img), dim3(ER_THREADS), smem, 0, ea);
        RT_HIP(hipGetLastError());
    }
    RT_HIP(hipDeviceSynchronize());
    if (n_dt) {
        RT_HIP(hipMemcpy(dt_type, ea.dt_type, (size_t)n_dt * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(dt_gt, ea.dt_gt, (size_t)n_dt * 4, hipMemcpyDeviceToHost));
    }
    if (n_gt) {
        RT_HIP(hipMemcpy(gt_state, ea.gt_state, (size_t)n_gt * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(gt_dt, ea.gt_dt, (size_t)n_gt * 4, hipMemcpyDeviceToHost));
    }
    std::vector<int64_t> hist(n_hist);
    RT_HIP(hipMemcpy(hist.data(), d_hist, n_hist * 8, hipMemcpyDeviceToHost));
    const int64_t *h = hist.data();
    memcpy(by_class, h, n_class * 8); h += n_class;
    memcpy(by_size, h, n_size * 8); h += n_size;
    memcpy(by_cell, h, n_cell * 8); h += n_cell;
    memcpy(missed_uncovered, h, (size_t)K * 8); h += K;
    memcpy(cm, h, n_cm * 8); h += n_cm;
    memcpy(cm_dropped, h, (size_t)K * 8);
    return RTMODT_OK;
}
