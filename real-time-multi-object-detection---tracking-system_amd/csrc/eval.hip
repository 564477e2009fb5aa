// eval.hip -- offline accuracy evaluation on the GPU: COCO bbox AP (pycocotools' COCOeval.evaluate / accumulate) and
// MOTChallenge CLEAR MOT + IDF1 (motmetrics' MOTAccumulator with the 'iou' distance), restating the reference's
// src/evaluation/metrics.py without either library.  PARITY UNPINNED: neither library is installed anywhere this runs;
// the rules below are the normative restatement, tests/eval_ref.py states them in NumPy and
// the GPU tests require bit identity with it.
//
// COCO (rtmodt_coco_eval), all float64:
//   coco_match       one 256-thread workgroup per non-empty (category, image) cell: a stable rank sort of the cell's
//                    detections by (-score, file index) in LDS, the first maxDets[-1] kept; per (area range, IoU
//                    threshold) one wave runs the greedy matcher det by det.  The matcher's pick is the LAST GT attaining
//                    the maximum IoU >= thr among the eligible non-ignored GTs, else among the eligible ignored ones: a
//                    wave max-reduction of the key (non-ignored, IoU, GT position).  Output per kept det: a code per
//                    (a, t) (0 fp, 1 tp, 2 ignored), its rank in the cell and an order-preserving 64-bit score key.
//   (rocPRIM)        segmented_radix_sort_pairs_desc by category segment: stable, and the input is already in (image,
//                    rank) order, so the result is ordered by the unique key (category, -score, image index, rank).
//   coco_accumulate  one workgroup per (k, a, m, t): a block scan of the packed (tp, fp) counts in sorted order, the
//                    precision at every true positive, a suffix-max scan and 101 binary searches.  Every step is an
//                    integer count, one IEEE division or a max, so precision / recall are bit-identical to NumPy.
// MOT (rtmodt_mot_eval):
//   mot_pairs        one wave per frame of every sequence, twice: a count pass, then (after a host scan of the counts)
//                    the valid (d = 1 - IoU <= 0.5) pairs compacted in (GT row, hyp row) order into the frame's CSR slice,
//                    each with its (sequence, o, h) key.  rocPRIM radix_sort_keys + run_length_encode turn the keys into
//                    the sparse IDF1 co-occurrence counts n(o, h).
//   mot_accumulate   one workgroup per sequence, walking its frames: continuation, then the maximum-cardinality /
//                    minimum-sum-of-d assignment (isolated edges directly, the contested rest with lap.h's solver on
//                    lexicographic (count, d) costs), then the MATCH / SWITCH / MISS / FP counts.
//   IDTP             a maximum-weight matching of the integer count graph, on the host (lap_solve<long long>).
//
// Built with -ffp-contract=off: every float64 operation rounds separately, as NumPy's do.
#include "common.h"
#include "eval_dev.h"
#include "lap.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

namespace rtmodt {

#pragma clang fp contract(off)

constexpr int COCO_MAX_GT_CELL = 1024, COCO_MAX_DT_CELL = 4096, COCO_MAX_DETS = 1024, COCO_MAX_AT = 256;

// ======================================================================================================================
// COCO
// ======================================================================================================================
struct CocoArgs {
    const double *iou_thrs, *area_rng;      // [T], [A][2]
    int T, A, maxdet;                       // maxdet = maxDets[-1]
    int n_cells;
    const int32_t *gt_start, *dt_start;     // [n_cells + 1] into the GT / detection rows (file order inside a cell)
    const double *gt_box, *gt_area;         // [n_gt][4] x, y, w, h; [n_gt]
    const int32_t *gt_crowd;                // [n_gt]
    const int64_t *gt_id;                   // [n_gt]
    const double *dt_box, *dt_score;        // [n_dt][4], [n_dt]
    const int32_t *out_start;               // [n_cells + 1]: kept detections, min(n, maxdet) per cell
    uint8_t *code;                          // [n_out][A * T]
    int32_t *rank;                          // [n_out]
    uint64_t *key;                          // [n_out]
    int32_t *npig;                          // [n_cells][A]
    int max_gt, max_dt;                     // LDS sizing (largest cell)
};

__global__ __launch_bounds__(EV_THREADS) void coco_match(CocoArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int cell = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = a.gt_start[cell], G = a.gt_start[cell + 1] - g0;
    const int d0 = a.dt_start[cell], Draw = a.dt_start[cell + 1] - d0;
    const int D = min(Draw, a.maxdet);
    const int o0 = a.out_start[cell];
    const int A = a.A, T = a.T;
    // LDS carve (host: coco_match_smem)
    double4 *gbox = (double4 *)smem;                       // [max_gt]
    double4 *dbox = gbox + a.max_gt;                       // [maxdet]
    double *garea = (double *)(dbox + a.maxdet);           // [max_gt]
    double *dsc = garea + a.max_gt;                        // [max_dt]
    int *order = (int *)(dsc + a.max_dt);                  // [maxdet] rank -> detection (file position in the cell)
    int *perm = order + a.maxdet;                          // [A][max_gt] area-range order: non-ignored GTs first, stable
    unsigned char *gcrowd = (unsigned char *)(perm + A * a.max_gt);   // [max_gt]
    unsigned char *gig = gcrowd + a.max_gt;                // [A][max_gt] by original position
    unsigned char *gzero = gig + A * a.max_gt;             // [max_gt] annotation id == 0
    unsigned char *gtm = gzero + a.max_gt;                 // [EV_WAVES][max_gt] matched flags of the wave's (a, t), by order position

    for (int i = tid; i < Draw; i += EV_THREADS) dsc[i] = a.dt_score[d0 + i];
    for (int g = tid; g < G; g += EV_THREADS) {
        const double *b = a.gt_box + (size_t)(g0 + g) * 4;
        gbox[g] = double4{b[0], b[1], b[2], b[3]};
        garea[g] = a.gt_area[g0 + g];
        gcrowd[g] = a.gt_crowd[g0 + g] != 0;
        gzero[g] = a.gt_id[g0 + g] == 0;
    }
    __syncthreads();
    // ---- stable rank sort of the detections by (-score, file index) ----
    for (int i = tid; i < Draw; i += EV_THREADS) {
        const double s = dsc[i];
        int r = 0;
        for (int j = 0; j < Draw; ++j) {
            const double t = dsc[j];
            r += (t > s) || (t == s && j < i);
        }
        if (r < D) order[r] = i;
    }
    // ---- GT ignore flags and the stable non-ignored-first order per area range ----
    for (int ar = wave; ar < A; ar += EV_WAVES) {
        const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
        int base_n = 0, base_i = 0, nig_total = 0;
        for (int cb = 0; cb < G; cb += 64) {                 // count the non-ignored first
            const int g = cb + lane;
            const bool ig = g < G && (gcrowd[g] || garea[g] < lo || garea[g] > hi);
            nig_total += __popcll(__ballot(g < G && !ig));
        }
        for (int cb = 0; cb < G; cb += 64) {
            const int g = cb + lane;
            const bool in = g < G;
            const bool ig = in && (gcrowd[g] || garea[g] < lo || garea[g] > hi);
            const unsigned long long mn = __ballot(in && !ig), mi = __ballot(in && ig);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (in) {
                gig[ar * a.max_gt + g] = ig;
                perm[ar * a.max_gt + (ig ? nig_total + base_i + __popcll(mi & below) : base_n + __popcll(mn & below))] = g;
            }
            base_n += __popcll(mn);
            base_i += __popcll(mi);
        }
        if (lane == 0) a.npig[(size_t)cell * A + ar] = nig_total;
    }
    __syncthreads();
    for (int r = tid; r < D; r += EV_THREADS) {
        const int i = order[r];
        const double *b = a.dt_box + (size_t)(d0 + i) * 4;
        dbox[r] = double4{b[0], b[1], b[2], b[3]};
        a.rank[o0 + r] = r;
        a.key[o0 + r] = score_key(dsc[i]);
    }
    __syncthreads();
    // ---- the greedy matcher, one wave per (area range, threshold) ----
    unsigned char *my_gtm = gtm + wave * a.max_gt;
    for (int at = wave; at < A * T; at += EV_WAVES) {
        const int ar = at / T, t = at - ar * T;
        const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
        const double thr0 = fmin(a.iou_thrs[t], 1.0 - 1e-10);
        const int *pm = perm + ar * a.max_gt;
        const unsigned char *ig = gig + ar * a.max_gt;
        for (int p = lane; p < G; p += 64) my_gtm[p] = 0;
        __builtin_amdgcn_wave_barrier();
        for (int r = 0; r < D; ++r) {
            const double4 db = dbox[r];
            // best key (non-ignored, IoU, position); position -1 = none
            int bn = 0, bp = -1;
            double bv = 0.0;
            for (int p = lane; p < G; p += 64) {
                const int g = pm[p];
                if (my_gtm[p] && !gcrowd[g]) continue;
                const double v = coco_iou(db, gbox[g], gcrowd[g]);
                if (v < thr0) continue;
                const int n = !ig[g];
                if (bp < 0 || n > bn || (n == bn && (v > bv || (v == bv && p > bp)))) { bn = n; bv = v; bp = p; }
            }
            for (int s = 32; s >= 1; s >>= 1) {
                const int on = __shfl_xor(bn, s), op = __shfl_xor(bp, s);
                const double ov = __shfl_xor(bv, s);
                const bool take = op >= 0 && (bp < 0 || on > bn || (on == bn && (ov > bv || (ov == bv && op > bp))));
                if (take) { bn = on; bv = ov; bp = op; }
            }
            if (lane == 0) {
                bool matched = false, dig = false;
                if (bp >= 0) {
                    const int g = pm[bp];
                    my_gtm[bp] = 1;
                    dig = ig[g];
                    matched = !gzero[g];                    // pycocotools: "matched" means a nonzero annotation id
                }
                if (!matched) {
                    const double da = db.z * db.w;
                    if (da < lo || da > hi) dig = true;
                }
                a.code[(size_t)(o0 + r) * (A * T) + at] = dig ? 2 : (matched ? 1 : 0);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

static size_t coco_match_smem(int max_gt, int max_dt, int maxdet, int A) {
    return (size_t)max_gt * 32 + (size_t)maxdet * 32 + (size_t)max_gt * 8 + (size_t)max_dt * 8 + (size_t)maxdet * 4 + (size_t)A * max_gt * 4 +
           (size_t)max_gt * (1 + A + 1 + EV_WAVES) + 64;
}

struct AccArgs {
    const double *rec_thrs;                 // [R]
    const int32_t *max_dets;                // [M]
    int T, R, K, A, M;
    const int32_t *cat_out_start;           // [K + 1] into the sorted detections
    const int32_t *cat_cell_start;          // [K + 1] into the cells
    const int32_t *sorted;                  // [n_out] detection (output row) in (category, -score, image, rank) order
    const uint8_t *code;                    // [n_out][A * T]
    const int32_t *rank;                    // [n_out]
    const int32_t *npig;                    // [n_cells][A]
    const int64_t *scratch_start;           // [K * A * M * T + 1]
    double *scratch;
    double *precision;                      // [T][R][K][A][M]
    double *recall;                         // [T][K][A][M]
};

__global__ __launch_bounds__(EV_THREADS) void coco_accumulate(AccArgs a) {
    __shared__ unsigned long long wtot64[EV_WAVES];
    __shared__ double wtotd[EV_WAVES];
    __shared__ int wtoti[EV_WAVES];
    const int tid = threadIdx.x;
    int b = blockIdx.x;                                    // ((k * A + ar) * M + m) * T + t
    const int t = b % a.T; b /= a.T;
    const int m = b % a.M; b /= a.M;
    const int ar = b % a.A;
    const int k = b / a.A;
    const int AT = a.A * a.T;
    const int at = ar * a.T + t;
    const int c0 = a.cat_cell_start[k], c1 = a.cat_cell_start[k + 1];
    const size_t pidx = (size_t)(k * a.A + ar) * a.M + m;  // [K][A][M] part of the output index
    const size_t KAM = (size_t)a.K * a.A * a.M;
    int npig = 0;
    for (int c = c0 + tid; c < c1; c += EV_THREADS) npig += a.npig[(size_t)c * a.A + ar];
    int tot;
    block_scan(npig, [](int x, int y) { return x + y; }, wtoti, tot);
    npig = tot;
    if (c1 == c0 || npig == 0) {                           // no cell, or nothing to recall: -1 stays
        for (int r = tid; r < a.R; r += EV_THREADS) a.precision[((size_t)t * a.R + r) * KAM + pidx] = -1.0;
        if (tid == 0) a.recall[(size_t)t * KAM + pidx] = -1.0;
        return;
    }
    const int maxdet = a.max_dets[m];
    double *P = a.scratch + a.scratch_start[blockIdx.x];
    const int64_t cap = a.scratch_start[blockIdx.x + 1] - a.scratch_start[blockIdx.x];
    // ---- tp / fp counts in sorted order; the precision at the c-th true positive -> P[c - 1] ----
    unsigned long long carry = 0;                          // (tp << 32) | fp so far
    int nd = 0;
    const int s0 = a.cat_out_start[k], s1 = a.cat_out_start[k + 1];
    for (int base = s0; base < s1; base += EV_THREADS) {
        const int i = base + tid;
        int code = 2, in = 0;
        if (i < s1) {
            const int o = a.sorted[i];
            in = a.rank[o] < maxdet;
            if (in) code = a.code[(size_t)o * AT + at];
        }
        const unsigned long long v = code == 1 ? (1ull << 32) : (code == 0 ? 1ull : 0ull);
        unsigned long long ctot;
        const unsigned long long inc = block_scan(v, [](unsigned long long x, unsigned long long y) { return x + y; }, wtot64, ctot) + carry;
        int ntot;
        block_scan(in, [](int x, int y) { return x + y; }, wtoti, ntot);
        if (code == 1) {
            const long long c = (long long)(inc >> 32), fp = (long long)(inc & 0xffffffffull);
            if (c <= cap) P[c - 1] = (double)c / (((double)c + (double)fp) + 2.220446049250313e-16);
        }
        carry += ctot;
        nd += ntot;
    }
    const int TP = (int)min((long long)(carry >> 32), (long long)cap);   // (never clipped: TP <= min(npig, nd) = cap)
    __syncthreads();                                       // P[] written by the whole workgroup (global memory, same workgroup)
    // ---- running maximum from the right: Q[c] = max(P[c..TP)) ----
    double cmax = 0.0;
    for (int end = TP; end > 0; end -= EV_THREADS) {
        const int i = end - 1 - tid;
        double v = i >= 0 ? P[i] : 0.0;
        double mx;
        v = block_scan(v, [](double x, double y) { return fmax(x, y); }, wtotd, mx);
        if (i >= 0) P[i] = fmax(v, cmax);
        cmax = fmax(cmax, mx);
    }
    __syncthreads();
    // ---- searchsorted(rc, r, 'left') and the precision at it, per recall threshold ----
    const double dn = (double)npig;
    for (int r = tid; r < a.R; r += EV_THREADS) {
        const double thr = a.rec_thrs[r];
        double q = 0.0;
        if (nd > 0) {
            if (0.0 >= thr) {
                q = TP > 0 ? P[0] : 0.0;                   // rc[0] >= thr: index 0, the maximum over everything
            } else {
                int lo = 1, hi = TP + 1;                   // first c in [1, TP] with c / npig >= thr, TP + 1 if none
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((double)mid / dn >= thr) hi = mid; else lo = mid + 1;
                }
                if (lo <= TP) q = P[lo - 1];
            }
        }
        a.precision[((size_t)t * a.R + r) * KAM + pidx] = q;
    }
    if (tid == 0) a.recall[(size_t)t * KAM + pidx] = nd > 0 ? (double)TP / dn : 0.0;
}

// ======================================================================================================================
// MOT
// ======================================================================================================================
struct MotArgs {
    int n_frames, n_seq;
    const int32_t *frame_seq;               // [n_frames]
    const int32_t *seq_frame_start;         // [n_seq + 1]
    const int32_t *gt_start, *hyp_start;    // [n_frames + 1] into the GT / hypothesis rows
    const int32_t *gt_oid, *hyp_hid;        // [n_gt], [n_hyp]: dense ids within the sequence
    const double *gt_box, *hyp_box;         // [n][4] x, y, w, h
    const int64_t *pair_start;              // [n_frames + 1]: CSR of the valid pairs (exclusive scan of the count pass)
    int32_t *pair_o, *pair_h;               // local row indices, (GT row, hyp row) order inside a frame
    double *pair_d;
    uint64_t *pair_key;                     // key_base[seq] + oid * n_hid + hid: the IDF1 co-occurrence key of the pair
    int32_t *pair_n;                        // [n_frames] valid pairs of the frame (count pass)
    const uint64_t *key_base;               // [n_seq]
    const int32_t *seq_n_hid;               // [n_seq]
    const int64_t *state_start;             // [n_seq] per-object state slice
    int32_t *st_m, *st_last, *st_present, *st_tracked;
    const int32_t *seq_n_oid;               // [n_seq]
    int64_t *counts;                        // [n_seq][MOT_NCOUNT]
    double *dist;                           // [n_seq]
    int max_rows;                           // LDS sizing
};
enum { MC_MATCH, MC_SWITCH, MC_MISS, MC_FP, MC_OBJ, MC_PRED, MC_MT, MC_ML, MC_ERR, MC_ERR_FRAME, MOT_NCOUNT };

// WRITE = false: the count pass (pair_n only); WRITE = true: the same decisions again, compacted into the frame's CSR slice
template <bool WRITE>
__global__ __launch_bounds__(EV_THREADS) void mot_pairs(MotArgs a) {
    const int f = blockIdx.x * EV_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= a.n_frames) return;
    const int go = a.gt_start[f], nO = a.gt_start[f + 1] - go;
    const int gh = a.hyp_start[f], nH = a.hyp_start[f + 1] - gh;
    const int s = a.frame_seq[f];
    const uint64_t nh_ids = (uint64_t)a.seq_n_hid[s];
    const int64_t p0 = WRITE ? a.pair_start[f] : 0;
    const int total = nO * nH;
    int cnt = 0;
    for (int base = 0; base < total; base += 64) {
        const int p = base + lane;
        bool valid = false;
        int o = 0, h = 0;
        double d = 0.0;
        if (p < total) {
            o = p / nH; h = p - o * nH;
            d = mot_dist(a.gt_box + (size_t)(go + o) * 4, a.hyp_box + (size_t)(gh + h) * 4);
            valid = d <= 0.5;
        }
        const unsigned long long mk = __ballot(valid);
        if (WRITE && valid) {
            const int64_t e = p0 + cnt + __popcll(mk & ((1ull << lane) - 1ull));
            a.pair_o[e] = o; a.pair_h[e] = h; a.pair_d[e] = d;
            a.pair_key[e] = a.key_base[s] + (uint64_t)a.gt_oid[go + o] * nh_ids + (uint64_t)a.hyp_hid[gh + h];
        }
        cnt += __popcll(mk);
    }
    if (!WRITE && lane == 0) a.pair_n[f] = cnt;
}

constexpr int MK_NONE = 0, MK_MATCH = 1, MK_SWITCH = 2;

// LDS of mot_accumulate: the LexCost solver state, then the frame's rows (R = the most rows of a frame).  One carve for
// both sides: the host sizes the launch with mot_carve(nullptr, R).end.
struct MotSmem {
    LapSmemT<LexCost> L;
    int *oid, *hid;                        // [R] dense ids of the frame's GT / hypothesis rows
    int *omark, *hmark, *okind;            // [R] matched H row / O row (-1 none), MK_* per O row
    int *odeg, *hdeg, *oedge;              // [R] degrees of the unmarked valid pairs, a row's last such pair
    int *rbeg, *rend;                      // [R] each O row's range in the frame's pairs (they are in row order)
    double *odist;                         // [R] d of the O row's match
    uintptr_t end;
};
__host__ __device__ inline MotSmem mot_carve(unsigned char *base, int R) {
    MotSmem S;
    LapSmemT<LexCost> &L = S.L;
    L.ecost = (LexCost *)base;
    L.u = L.ecost + LAP_EDGES;
    L.v = L.u + LAP_ROWS;
    L.minv = L.v + LAP_COLS;
    L.colmap = (int *)(L.minv + LAP_COLS);                 // [R] H row -> contested column
    L.hrow = L.colmap + R;
    L.hcol = L.hrow + LAP_ROWS;
    L.estart = L.hcol + LAP_COLS;
    L.ecol = L.estart + LAP_ROWS + 1;
    L.p = L.ecol + LAP_EDGES;
    L.rm = L.p + LAP_COLS;
    L.wayrow = L.rm + LAP_ROWS;
    L.touched = L.wayrow + LAP_COLS;
    L.usedl = L.touched + LAP_COLS;
    S.oid = L.usedl + LAP_COLS;
    S.hid = S.oid + R;
    S.omark = S.hid + R;
    S.hmark = S.omark + R;
    S.okind = S.hmark + R;
    S.odeg = S.okind + R;
    S.hdeg = S.odeg + R;
    S.oedge = S.hdeg + R;
    S.rbeg = S.oedge + R;
    S.rend = S.rbeg + R;
    S.odist = (double *)(((uintptr_t)(S.rend + R) + 7) & ~(uintptr_t)7);
    L.used = (unsigned char *)(S.odist + R);               // [LAP_COLS]
    S.end = (uintptr_t)(L.used + LAP_COLS);
    return S;
}

__global__ __launch_bounds__(EV_THREADS) void mot_accumulate(MotArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const MotSmem S = mot_carve(smem, a.max_rows);
    const LapSmemT<LexCost> &L = S.L;
    int *oid = S.oid, *hid = S.hid, *omark = S.omark, *hmark = S.hmark, *okind = S.okind;
    int *odeg = S.odeg, *hdeg = S.hdeg, *oedge = S.oedge, *rbeg = S.rbeg, *rend = S.rend;
    double *odist = S.odist;
    __shared__ int s_err;
    __shared__ int wtoti[EV_WAVES];

    const int f0 = a.seq_frame_start[s], f1 = a.seq_frame_start[s + 1];
    const int n_oid = a.seq_n_oid[s];
    int32_t *m = a.st_m + a.state_start[s], *last = a.st_last + a.state_start[s];
    int32_t *present = a.st_present + a.state_start[s], *tracked = a.st_tracked + a.state_start[s];
    for (int o = tid; o < n_oid; o += EV_THREADS) { m[o] = -1; last[o] = -1; present[o] = 0; tracked[o] = 0; }
    if (tid == 0) s_err = 0;
    long long c_match = 0, c_switch = 0, c_miss = 0, c_fp = 0, c_obj = 0, c_pred = 0;
    double dsum = 0.0;
    int last_update = -1;
    __syncthreads();
    for (int f = f0; f < f1; ++f) {
        const int fl = f - f0;                             // frame position in the sequence
        const int go = a.gt_start[f], nO = a.gt_start[f + 1] - go;
        const int gh = a.hyp_start[f], nH = a.hyp_start[f + 1] - gh;
        const int np = a.pair_n[f];
        const int64_t p0 = a.pair_start[f];
        for (int r = tid; r < nO; r += EV_THREADS) {
            oid[r] = a.gt_oid[go + r]; omark[r] = -1; okind[r] = MK_NONE; odeg[r] = 0; rbeg[r] = 0; rend[r] = 0;
        }
        for (int r = tid; r < nH; r += EV_THREADS) { hid[r] = a.hyp_hid[gh + r]; hmark[r] = -1; hdeg[r] = 0; L.colmap[r] = -1; }
        __syncthreads();
        for (int e = tid; e < np; e += EV_THREADS) {       // each O row's pair range (the pairs are in row order)
            const int r = a.pair_o[p0 + e];
            if (e == 0 || a.pair_o[p0 + e - 1] != r) rbeg[r] = e;
            if (e == np - 1 || a.pair_o[p0 + e + 1] != r) rend[r] = e + 1;
        }
        // ---- 1. continuation: o keeps last frame's hypothesis (distinct targets: order-free) ----
        for (int e = tid; e < np; e += EV_THREADS) {
            const int r = a.pair_o[p0 + e], c = a.pair_h[p0 + e];
            const int o = oid[r];
            if (m[o] >= 0 && last[o] == last_update && m[o] == hid[c]) {
                omark[r] = c; hmark[c] = r; okind[r] = MK_MATCH; odist[r] = a.pair_d[p0 + e];
            }
        }
        __syncthreads();
        // ---- 2. degrees of the unmarked valid pairs ----
        for (int e = tid; e < np; e += EV_THREADS) {
            const int r = a.pair_o[p0 + e], c = a.pair_h[p0 + e];
            if (omark[r] < 0 && hmark[c] < 0) { atomicAdd(&odeg[r], 1); atomicAdd(&hdeg[c], 1); oedge[r] = e; }
        }
        __syncthreads();
        // isolated edges resolve directly; a row is contested when it or its one column has another edge
        int nhr = 0;
        for (int base = 0; base < nO; base += EV_THREADS) {
            const int r = base + tid;
            bool hard = false;
            if (r < nO && omark[r] < 0 && odeg[r] > 0) {
                const int e = oedge[r];
                if (odeg[r] == 1 && hdeg[a.pair_h[p0 + e]] == 1) {
                    const int c = a.pair_h[p0 + e];
                    omark[r] = c; hmark[c] = r; odist[r] = a.pair_d[p0 + e];
                    okind[r] = (m[oid[r]] >= 0 && m[oid[r]] != hid[c]) ? MK_SWITCH : MK_MATCH;
                } else {
                    hard = true;
                }
            }
            int tot;
            const int pos = block_scan((int)hard, [](int x, int y) { return x + y; }, wtoti, tot) - (int)hard;
            if (hard && nhr + pos < LAP_ROWS) L.hrow[nhr + pos] = r;
            nhr += tot;
        }
        __syncthreads();
        if (nhr > 0 && tid == 0) {                         // the contested remainder: one lane, lexicographic (count, d)
            bool over = nhr > LAP_ROWS;
            int ne = 0, nhc = 0;
            for (int h = 0; h < nhr && !over; ++h) {
                const int r = L.hrow[h];
                L.estart[h] = ne;
                L.u[h] = LapCost<LexCost>::zero();
                L.rm[h] = -1;
                for (int e = rbeg[r]; e < rend[r]; ++e) {
                    const int c = a.pair_h[p0 + e];
                    if (hmark[c] >= 0) continue;
                    if (L.colmap[c] < 0) {
                        if (nhc == LAP_COLS) { over = true; break; }
                        L.colmap[c] = nhc; L.hcol[nhc] = c;
                        L.v[nhc] = LapCost<LexCost>::zero(); L.minv[nhc] = LapCost<LexCost>::inf(); L.p[nhc] = -1; L.used[nhc] = 0;
                        ++nhc;
                    }
                    if (ne == LAP_EDGES) { over = true; break; }
                    L.ecol[ne] = L.colmap[c];
                    L.ecost[ne] = LexCost{-1, a.pair_d[p0 + e]};
                    ++ne;
                }
            }
            if (over) {
                s_err = 1;
                a.counts[(size_t)s * MOT_NCOUNT + MC_ERR_FRAME] = fl;
            } else {
                L.estart[nhr] = ne;
                lap_solve(L, nhr);
                for (int h = 0; h < nhr; ++h)
                    if (L.rm[h] >= 0) {
                        const int r = L.hrow[h], c = L.hcol[L.rm[h]];
                        omark[r] = c; hmark[c] = r;
                        for (int e = rbeg[r]; e < rend[r]; ++e)
                            if (a.pair_h[p0 + e] == c) { odist[r] = a.pair_d[p0 + e]; break; }
                        okind[r] = (m[oid[r]] >= 0 && m[oid[r]] != hid[c]) ? MK_SWITCH : MK_MATCH;
                    }
            }
        }
        __syncthreads();
        if (s_err) break;
        // ---- 3. / 4. events and per-object counters ----
        for (int r = tid; r < nO; r += EV_THREADS) {
            const int o = oid[r];
            present[o] += 1;
            if (okind[r] != MK_NONE) {
                tracked[o] += 1;
                m[o] = hid[omark[r]];
                last[o] = fl;
            }
        }
        if (tid == 0) {
            int nm = 0;
            for (int r = 0; r < nO; ++r) {                 // row order: a deterministic sum of d
                if (okind[r] == MK_NONE) continue;
                ++nm;
                if (okind[r] == MK_SWITCH) ++c_switch; else ++c_match;
                dsum += odist[r];
            }
            c_miss += nO - nm;
            c_fp += nH - nm;
            c_obj += nO;
            c_pred += nH;
        }
        last_update = fl;
        __syncthreads();
    }
    // ---- mostly tracked / mostly lost ----
    int mt = 0, ml = 0;
    if (!s_err)
        for (int o = tid; o < n_oid; o += EV_THREADS) {
            if (present[o] == 0) continue;
            const double ratio = (double)tracked[o] / (double)present[o];
            mt += ratio >= 0.8;
            ml += ratio < 0.2;
        }
    int mt_tot, ml_tot;
    block_scan(mt, [](int x, int y) { return x + y; }, wtoti, mt_tot);
    block_scan(ml, [](int x, int y) { return x + y; }, wtoti, ml_tot);
    if (tid == 0) {
        int64_t *c = a.counts + (size_t)s * MOT_NCOUNT;
        c[MC_MATCH] = c_match; c[MC_SWITCH] = c_switch; c[MC_MISS] = c_miss; c[MC_FP] = c_fp;
        c[MC_OBJ] = c_obj; c[MC_PRED] = c_pred; c[MC_MT] = mt_tot; c[MC_ML] = ml_tot; c[MC_ERR] = s_err;
        a.dist[s] = dsum;
    }
}

static size_t mot_acc_smem(int R) { return (size_t)mot_carve(nullptr, R).end + 16; }

// IDTP: maximum-weight matching of the integer co-occurrence graph (rows = objects, columns = hypotheses, weight n > 0).
// edges: (object, hypothesis, n) of one sequence, ascending by object.
struct IdEdge { int o, h; long long n; };
static long long idtp_host(const IdEdge *edges, size_t n_edges, int n_oid, int n_hid) {
    if (n_edges == 0) return 0;
    std::vector<int> estart(n_oid + 1, 0), ecol(n_edges), colmap(n_hid, -1);
    std::vector<long long> ecost(n_edges);
    int nc = 0;
    for (size_t e = 0; e < n_edges; ++e) {
        const IdEdge &g = edges[e];
        ++estart[g.o + 1];
        if (colmap[g.h] < 0) colmap[g.h] = nc++;
        ecol[e] = colmap[g.h];
        ecost[e] = -g.n;
    }
    for (int o = 0; o < n_oid; ++o) estart[o + 1] += estart[o];
    std::vector<long long> u(n_oid, 0), v(nc, 0), minv(nc, LapCost<long long>::inf());
    std::vector<int> hrow(n_oid), hcol(nc), p(nc, -1), rm(n_oid, -1), wayrow(nc), touched(nc), usedl(nc);
    std::vector<unsigned char> used(nc, 0);
    LapSmemT<long long> L;
    L.colmap = nullptr; L.ecost = ecost.data(); L.u = u.data(); L.v = v.data(); L.minv = minv.data();
    L.hrow = hrow.data(); L.hcol = hcol.data(); L.estart = estart.data(); L.ecol = ecol.data();
    L.p = p.data(); L.rm = rm.data(); L.wayrow = wayrow.data(); L.touched = touched.data(); L.usedl = usedl.data(); L.used = used.data();
    lap_solve(L, n_oid);
    long long w = 0;
    for (int o = 0; o < n_oid; ++o)
        if (rm[o] >= 0)
            for (int e = estart[o]; e < estart[o + 1]; ++e)
                if (ecol[e] == rm[o]) { w -= ecost[e]; break; }
    return w;
}

}  // namespace rtmodt

using namespace rtmodt;

extern "C" {

int rtmodt_coco_eval(int device, const double *iou_thrs, int T, const double *rec_thrs, int R, const int32_t *max_dets, int M,
                     const double *area_rng, int A, int K, int n_cells, const int32_t *cell_cat, const int32_t *gt_start,
                     const double *gt_box, const double *gt_area, const int32_t *gt_crowd, const int64_t *gt_id,
                     const int32_t *dt_start, const double *dt_box, const double *dt_score, double *precision, double *recall) {
    RT_CHECK(iou_thrs && rec_thrs && max_dets && area_rng && precision && recall, RTMODT_E_INVALID, "coco_eval: null argument");
    RT_CHECK(T >= 1 && R >= 1 && M >= 1 && A >= 1 && K >= 1 && n_cells >= 0, RTMODT_E_INVALID,
             "coco_eval: T %d, R %d, M %d, A %d, K %d, cells %d", T, R, M, A, K, n_cells);
    RT_CHECK(A * T <= COCO_MAX_AT, RTMODT_E_CAPACITY, "coco_eval: %d area ranges x %d IoU thresholds > %d", A, T, COCO_MAX_AT);
    for (int i = 0; i < M; ++i)
        RT_CHECK(max_dets[i] >= 1 && (i == 0 || max_dets[i] >= max_dets[i - 1]), RTMODT_E_INVALID, "coco_eval: maxDets must ascend from 1");
    const int maxdet = max_dets[M - 1];
    RT_CHECK(maxdet <= COCO_MAX_DETS, RTMODT_E_CAPACITY, "coco_eval: maxDets[-1] = %d > %d", maxdet, COCO_MAX_DETS);
    for (int t = 0; t < T; ++t) RT_CHECK(iou_thrs[t] == iou_thrs[t], RTMODT_E_INVALID, "coco_eval: NaN IoU threshold");
    for (int r = 0; r < R; ++r) RT_CHECK(rec_thrs[r] == rec_thrs[r], RTMODT_E_INVALID, "coco_eval: NaN recall threshold");
    // host checks: CSR shape, per-cell capacity, category order
    std::vector<int32_t> out_start(n_cells + 1, 0), cat_cell_start(K + 1, 0), cat_out_start(K + 1, 0);
    int max_gt = 1, max_dt = 1;
    if (n_cells) RT_CHECK(cell_cat && gt_start && dt_start, RTMODT_E_INVALID, "coco_eval: null cell arrays");
    if (n_cells) RT_CHECK(gt_start[0] == 0 && dt_start[0] == 0, RTMODT_E_INVALID, "coco_eval: CSR must start at 0");
    for (int c = 0; c < n_cells; ++c) {
        const int ng = gt_start[c + 1] - gt_start[c], nd = dt_start[c + 1] - dt_start[c];
        RT_CHECK(ng >= 0 && nd >= 0 && ng + nd > 0, RTMODT_E_INVALID, "coco_eval: cell %d is empty or malformed", c);
        RT_CHECK(cell_cat[c] >= 0 && cell_cat[c] < K && (c == 0 || cell_cat[c] >= cell_cat[c - 1]), RTMODT_E_INVALID,
                 "coco_eval: cells must be grouped by category (cell %d)", c);
        RT_CHECK(ng <= COCO_MAX_GT_CELL, RTMODT_E_CAPACITY, "coco_eval: cell %d (category index %d) holds %d GTs > %d", c, cell_cat[c], ng,
                 COCO_MAX_GT_CELL);
        RT_CHECK(nd <= COCO_MAX_DT_CELL, RTMODT_E_CAPACITY, "coco_eval: cell %d (category index %d) holds %d detections > %d", c,
                 cell_cat[c], nd, COCO_MAX_DT_CELL);
        max_gt = std::max(max_gt, ng);
        max_dt = std::max(max_dt, nd);
        out_start[c + 1] = out_start[c] + std::min(nd, maxdet);
        cat_cell_start[cell_cat[c] + 1] = c + 1;
    }
    for (int k = 0; k < K; ++k) cat_cell_start[k + 1] = std::max(cat_cell_start[k + 1], cat_cell_start[k]);
    for (int k = 0; k <= K; ++k) cat_out_start[k] = out_start[cat_cell_start[k]];
    const int n_gt = n_cells ? gt_start[n_cells] : 0, n_dt = n_cells ? dt_start[n_cells] : 0, n_out = out_start[n_cells];
    if (n_gt) RT_CHECK(gt_box && gt_area && gt_crowd && gt_id, RTMODT_E_INVALID, "coco_eval: null GT arrays");
    if (n_dt) RT_CHECK(dt_box && dt_score, RTMODT_E_INVALID, "coco_eval: null detection arrays");
    for (int i = 0; i < n_dt; ++i) RT_CHECK(dt_score[i] == dt_score[i], RTMODT_E_INVALID, "coco_eval: detection %d has a NaN score", i);
    // scratch per (k, a, m, t): the true positives, at most min(non-ignored GTs, kept detections)
    std::vector<int64_t> npig_ka((size_t)K * A, 0), nd_km((size_t)K * M, 0);
    for (int c = 0; c < n_cells; ++c) {
        const int k = cell_cat[c];
        for (int g = gt_start[c]; g < gt_start[c + 1]; ++g)
            for (int ar = 0; ar < A; ++ar)
                npig_ka[(size_t)k * A + ar] += !(gt_crowd[g] || gt_area[g] < area_rng[2 * ar] || gt_area[g] > area_rng[2 * ar + 1]);
        const int nd = dt_start[c + 1] - dt_start[c];
        for (int m = 0; m < M; ++m) nd_km[(size_t)k * M + m] += std::min(nd, max_dets[m]);
    }
    const size_t nblk = (size_t)K * A * M * T;
    std::vector<int64_t> scratch_start(nblk + 1, 0);
    for (size_t b = 0; b < nblk; ++b) {
        size_t q = b / T;
        const int m = (int)(q % M); q /= M;
        const int ar = (int)(q % A);
        const int k = (int)(q / A);
        scratch_start[b + 1] = scratch_start[b] + std::min(npig_ka[(size_t)k * A + ar], nd_km[(size_t)k * M + m]);
    }
    RT_CHECK(nblk <= (size_t)INT_MAX, RTMODT_E_CAPACITY, "coco_eval: too many (category, area, maxDet, threshold) blocks");
    const size_t smem = coco_match_smem(max_gt, max_dt, maxdet, A);
    RT_CHECK(smem <= 160 * 1024, RTMODT_E_CAPACITY, "coco_eval: the largest cell (%d GTs, %d detections) needs %zu B of LDS", max_gt, max_dt, smem);

    RT_HIP(hipSetDevice(device));
    DevBufs B;
    CocoArgs ca{};
    ca.T = T; ca.A = A; ca.maxdet = maxdet; ca.n_cells = n_cells; ca.max_gt = max_gt; ca.max_dt = max_dt;
    double *d_iou, *d_area, *d_gbox, *d_garea, *d_dbox, *d_dsc;
    int32_t *d_gs, *d_ds, *d_crowd, *d_os;
    int64_t *d_gid;
    RT_TRY(B.up(&d_iou, iou_thrs, T)); RT_TRY(B.up(&d_area, area_rng, 2 * A));
    RT_TRY(B.up(&d_gs, gt_start, n_cells + 1)); RT_TRY(B.up(&d_ds, dt_start, n_cells + 1)); RT_TRY(B.up(&d_os, out_start.data(), n_cells + 1));
    RT_TRY(B.up(&d_gbox, gt_box, (size_t)n_gt * 4)); RT_TRY(B.up(&d_garea, gt_area, n_gt));
    RT_TRY(B.up(&d_crowd, gt_crowd, n_gt)); RT_TRY(B.up(&d_gid, gt_id, n_gt));
    RT_TRY(B.up(&d_dbox, dt_box, (size_t)n_dt * 4)); RT_TRY(B.up(&d_dsc, dt_score, n_dt));
    ca.iou_thrs = d_iou; ca.area_rng = d_area; ca.gt_start = d_gs; ca.dt_start = d_ds; ca.out_start = d_os;
    ca.gt_box = d_gbox; ca.gt_area = d_garea; ca.gt_crowd = d_crowd; ca.gt_id = d_gid; ca.dt_box = d_dbox; ca.dt_score = d_dsc;
    RT_TRY(B.alloc(&ca.code, (size_t)n_out * A * T)); RT_TRY(B.alloc(&ca.rank, n_out)); RT_TRY(B.alloc(&ca.key, n_out));
    RT_TRY(B.alloc(&ca.npig, (size_t)n_cells * A));
    if (n_cells) {
        static DynLdsSeen seen;
        RT_TRY(raise_dynamic_lds((const void *)coco_match, smem, seen));
        hipLaunchKernelGGL(coco_match, dim3(n_cells), dim3(EV_THREADS), smem, 0, ca);
        RT_HIP(hipGetLastError());
    }
    // per-category order of the kept detections
    AccArgs aa{};
    uint64_t *d_key_out;
    int32_t *d_idx_in, *d_sorted, *d_cos, *d_ccs, *d_md;
    double *d_rec;
    int64_t *d_ss;
    RT_TRY(B.alloc(&d_key_out, n_out)); RT_TRY(B.alloc(&d_sorted, n_out));
    std::vector<int32_t> iota(n_out);
    for (int i = 0; i < n_out; ++i) iota[i] = i;
    RT_TRY(B.up(&d_idx_in, iota.data(), n_out));
    RT_TRY(B.up(&d_cos, cat_out_start.data(), K + 1)); RT_TRY(B.up(&d_ccs, cat_cell_start.data(), K + 1));
    if (n_out) {
        size_t tmp_bytes = 0;
        RT_HIP(rocprim::segmented_radix_sort_pairs_desc(nullptr, tmp_bytes, ca.key, d_key_out, d_idx_in, d_sorted, (unsigned)n_out, (unsigned)K,
                                                        d_cos, d_cos + 1));
        unsigned char *tmp;
        RT_TRY(B.alloc(&tmp, tmp_bytes));
        RT_HIP(rocprim::segmented_radix_sort_pairs_desc((void *)tmp, tmp_bytes, ca.key, d_key_out, d_idx_in, d_sorted, (unsigned)n_out, (unsigned)K,
                                                        d_cos, d_cos + 1));
    }
    RT_TRY(B.up(&d_rec, rec_thrs, R)); RT_TRY(B.up(&d_md, max_dets, M)); RT_TRY(B.up(&d_ss, scratch_start.data(), nblk + 1));
    aa.rec_thrs = d_rec; aa.max_dets = d_md; aa.T = T; aa.R = R; aa.K = K; aa.A = A; aa.M = M;
    aa.cat_out_start = d_cos; aa.cat_cell_start = d_ccs; aa.sorted = d_sorted; aa.code = ca.code; aa.rank = ca.rank; aa.npig = ca.npig;
    aa.scratch_start = d_ss;
    RT_TRY(B.alloc(&aa.scratch, (size_t)scratch_start[nblk]));
    RT_TRY(B.alloc(&aa.precision, (size_t)T * R * K * A * M)); RT_TRY(B.alloc(&aa.recall, (size_t)T * K * A * M));
    hipLaunchKernelGGL(coco_accumulate, dim3((unsigned)nblk), dim3(EV_THREADS), 0, 0, aa);
    RT_HIP(hipGetLastError());
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(precision, aa.precision, (size_t)T * R * K * A * M * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(recall, aa.recall, (size_t)T * K * A * M * 8, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_mot_eval(int device, int n_seq, const int32_t *seq_frame_start, const int64_t *frame_id, const int32_t *gt_start,
                    const int32_t *hyp_start, const int32_t *gt_oid, const double *gt_box, const int32_t *hyp_hid, const double *hyp_box,
                    const int32_t *seq_n_oid, const int32_t *seq_n_hid, rtmodt_mot_counts *out) {
    RT_CHECK(n_seq >= 1 && seq_frame_start && frame_id && gt_start && hyp_start && seq_n_oid && seq_n_hid && out, RTMODT_E_INVALID,
             "mot_eval: bad argument");
    RT_CHECK(seq_frame_start[0] == 0, RTMODT_E_INVALID, "mot_eval: frame CSR must start at 0");
    const int n_frames = seq_frame_start[n_seq];
    RT_CHECK(n_frames >= 0 && gt_start[0] == 0 && hyp_start[0] == 0, RTMODT_E_INVALID, "mot_eval: row CSR must start at 0");
    std::vector<int32_t> frame_seq(n_frames);
    std::vector<int64_t> state_start(n_seq + 1, 0);
    std::vector<uint64_t> key_base(n_seq + 1, 0);
    int max_rows = 1;
    for (int s = 0; s < n_seq; ++s) {
        RT_CHECK(seq_frame_start[s + 1] >= seq_frame_start[s] && seq_n_oid[s] >= 0 && seq_n_hid[s] >= 0, RTMODT_E_INVALID,
                 "mot_eval: sequence %d is malformed", s);
        for (int f = seq_frame_start[s]; f < seq_frame_start[s + 1]; ++f) {
            frame_seq[f] = s;
            const int nO = gt_start[f + 1] - gt_start[f], nH = hyp_start[f + 1] - hyp_start[f];
            RT_CHECK(nO >= 0 && nH >= 0, RTMODT_E_INVALID, "mot_eval: sequence %d frame %lld: malformed rows", s, (long long)frame_id[f]);
            RT_CHECK(nO <= MOT_MAX_ROWS && nH <= MOT_MAX_ROWS, RTMODT_E_CAPACITY,
                     "mot_eval: sequence %d frame %lld holds %d GT / %d hypothesis rows (at most %d each)", s, (long long)frame_id[f], nO, nH,
                     MOT_MAX_ROWS);
            for (int r = gt_start[f]; r < gt_start[f + 1]; ++r)
                RT_CHECK(gt_oid[r] >= 0 && gt_oid[r] < seq_n_oid[s], RTMODT_E_INVALID, "mot_eval: GT row %d: object index out of range", r);
            for (int r = hyp_start[f]; r < hyp_start[f + 1]; ++r)
                RT_CHECK(hyp_hid[r] >= 0 && hyp_hid[r] < seq_n_hid[s], RTMODT_E_INVALID, "mot_eval: hypothesis row %d: index out of range", r);
            max_rows = std::max(max_rows, std::max(nO, nH));
        }
        key_base[s + 1] = key_base[s] + (uint64_t)seq_n_oid[s] * (uint64_t)seq_n_hid[s];   // < 2^62 per sequence
        RT_CHECK(key_base[s + 1] >= key_base[s], RTMODT_E_CAPACITY, "mot_eval: the id key space of one call overflows 64 bits");
        state_start[s + 1] = state_start[s] + seq_n_oid[s];
    }
    const int n_gt = gt_start[n_frames], n_hyp = hyp_start[n_frames];
    RT_CHECK((n_gt == 0 || (gt_oid && gt_box)) && (n_hyp == 0 || (hyp_hid && hyp_box)), RTMODT_E_INVALID, "mot_eval: null row arrays");
    const size_t smem = mot_acc_smem(max_rows);
    RT_CHECK(smem <= 160 * 1024, RTMODT_E_CAPACITY, "mot_eval: %d rows per frame need %zu B of LDS", max_rows, smem);

    RT_HIP(hipSetDevice(device));
    DevBufs B;
    MotArgs ma{};
    ma.n_frames = n_frames; ma.n_seq = n_seq; ma.max_rows = max_rows;
    int32_t *d_fs, *d_sfs, *d_gs, *d_hs, *d_oid, *d_hid, *d_nh, *d_no;
    double *d_gb, *d_hb;
    int64_t *d_ps, *d_ss;
    uint64_t *d_kb;
    RT_TRY(B.up(&d_fs, frame_seq.data(), n_frames)); RT_TRY(B.up(&d_sfs, seq_frame_start, n_seq + 1));
    RT_TRY(B.up(&d_gs, gt_start, n_frames + 1)); RT_TRY(B.up(&d_hs, hyp_start, n_frames + 1));
    RT_TRY(B.up(&d_oid, gt_oid, n_gt)); RT_TRY(B.up(&d_hid, hyp_hid, n_hyp));
    RT_TRY(B.up(&d_gb, gt_box, (size_t)n_gt * 4)); RT_TRY(B.up(&d_hb, hyp_box, (size_t)n_hyp * 4));
    RT_TRY(B.up(&d_ss, state_start.data(), n_seq + 1)); RT_TRY(B.up(&d_kb, key_base.data(), n_seq + 1));
    RT_TRY(B.up(&d_nh, seq_n_hid, n_seq)); RT_TRY(B.up(&d_no, seq_n_oid, n_seq));
    ma.frame_seq = d_fs; ma.seq_frame_start = d_sfs; ma.gt_start = d_gs; ma.hyp_start = d_hs; ma.gt_oid = d_oid; ma.hyp_hid = d_hid;
    ma.gt_box = d_gb; ma.hyp_box = d_hb; ma.state_start = d_ss; ma.key_base = d_kb; ma.seq_n_hid = d_nh; ma.seq_n_oid = d_no;
    RT_TRY(B.alloc(&ma.pair_n, n_frames));
    // ---- count pass, then the per-frame CSR of the valid pairs ----
    std::vector<int32_t> pair_n(n_frames);
    std::vector<int64_t> pair_start(n_frames + 1, 0);
    if (n_frames) {
        hipLaunchKernelGGL(mot_pairs<false>, dim3(cdiv(n_frames, EV_WAVES)), dim3(EV_THREADS), 0, 0, ma);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpy(pair_n.data(), ma.pair_n, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
    }
    for (int f = 0; f < n_frames; ++f) pair_start[f + 1] = pair_start[f] + pair_n[f];
    const size_t npairs = (size_t)pair_start[n_frames], nstate = (size_t)state_start[n_seq];
    RT_CHECK(npairs <= (size_t(1) << 28), RTMODT_E_CAPACITY, "mot_eval: %zu valid (d <= 0.5) pairs in one call (at most 2^28)", npairs);
    RT_TRY(B.up(&d_ps, pair_start.data(), n_frames + 1));
    ma.pair_start = d_ps;
    RT_TRY(B.alloc(&ma.pair_o, npairs)); RT_TRY(B.alloc(&ma.pair_h, npairs)); RT_TRY(B.alloc(&ma.pair_d, npairs));
    RT_TRY(B.alloc(&ma.pair_key, npairs));
    RT_TRY(B.alloc(&ma.st_m, nstate)); RT_TRY(B.alloc(&ma.st_last, nstate)); RT_TRY(B.alloc(&ma.st_present, nstate)); RT_TRY(B.alloc(&ma.st_tracked, nstate));
    RT_TRY(B.alloc(&ma.counts, (size_t)n_seq * MOT_NCOUNT)); RT_TRY(B.alloc(&ma.dist, n_seq));
    RT_HIP(hipMemset(ma.counts, 0, (size_t)n_seq * MOT_NCOUNT * 8));
    if (n_frames) {
        hipLaunchKernelGGL(mot_pairs<true>, dim3(cdiv(n_frames, EV_WAVES)), dim3(EV_THREADS), 0, 0, ma);
        RT_HIP(hipGetLastError());
    }
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)mot_accumulate, smem, seen));
    hipLaunchKernelGGL(mot_accumulate, dim3(n_seq), dim3(EV_THREADS), smem, 0, ma);
    RT_HIP(hipGetLastError());
    // ---- IDF1 co-occurrence counts: sort the pair keys, run-length encode -> the sparse (sequence, o, h, n) table ----
    uint64_t *d_sorted, *d_unique;
    uint32_t *d_cnt, *d_nruns;
    RT_TRY(B.alloc(&d_sorted, npairs)); RT_TRY(B.alloc(&d_unique, npairs)); RT_TRY(B.alloc(&d_cnt, npairs)); RT_TRY(B.alloc(&d_nruns, 1));
    uint32_t nruns = 0;
    if (npairs) {
        size_t tb = 0, tb2 = 0;
        RT_HIP(rocprim::radix_sort_keys(nullptr, tb, ma.pair_key, d_sorted, (unsigned)npairs));
        RT_HIP(rocprim::run_length_encode(nullptr, tb2, d_sorted, (unsigned)npairs, d_unique, d_cnt, d_nruns));
        unsigned char *tmp;
        RT_TRY(B.alloc(&tmp, std::max(tb, tb2)));
        RT_HIP(rocprim::radix_sort_keys((void *)tmp, tb, ma.pair_key, d_sorted, (unsigned)npairs));
        RT_HIP(rocprim::run_length_encode((void *)tmp, tb2, d_sorted, (unsigned)npairs, d_unique, d_cnt, d_nruns));
        RT_HIP(hipMemcpy(&nruns, d_nruns, 4, hipMemcpyDeviceToHost));
    }
    RT_HIP(hipDeviceSynchronize());
    std::vector<int64_t> counts((size_t)n_seq * MOT_NCOUNT);
    std::vector<double> dist(n_seq);
    std::vector<uint64_t> ukey(nruns);
    std::vector<uint32_t> ucnt(nruns);
    RT_HIP(hipMemcpy(counts.data(), ma.counts, counts.size() * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(dist.data(), ma.dist, n_seq * 8, hipMemcpyDeviceToHost));
    if (nruns) {
        RT_HIP(hipMemcpy(ukey.data(), d_unique, (size_t)nruns * 8, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(ucnt.data(), d_cnt, (size_t)nruns * 4, hipMemcpyDeviceToHost));
    }
    std::vector<IdEdge> edges(nruns);
    std::vector<size_t> seq_edge(n_seq + 1, 0);                // keys ascend, so do sequences, then objects
    for (size_t i = 0, s = 0; i < nruns; ++i) {
        while (ukey[i] >= key_base[s + 1]) seq_edge[++s] = i;
        const uint64_t k = ukey[i] - key_base[s];
        edges[i] = IdEdge{(int)(k / (uint64_t)seq_n_hid[s]), (int)(k % (uint64_t)seq_n_hid[s]), (long long)ucnt[i]};
        seq_edge[s + 1] = i + 1;
    }
    for (int s = 0; s < n_seq; ++s) seq_edge[s + 1] = std::max(seq_edge[s + 1], seq_edge[s]);
    for (int s = 0; s < n_seq; ++s) {
        const int64_t *c = counts.data() + (size_t)s * MOT_NCOUNT;
        RT_CHECK(c[MC_ERR] == 0, RTMODT_E_CAPACITY,
                 "mot_eval: sequence %d frame %lld: the contested assignment exceeds %d rows / %d columns / %d pairs", s,
                 (long long)frame_id[seq_frame_start[s] + c[MC_ERR_FRAME]], LAP_ROWS, LAP_COLS, LAP_EDGES);
        rtmodt_mot_counts &o = out[s];
        o.num_frames = seq_frame_start[s + 1] - seq_frame_start[s];
        o.num_objects = c[MC_OBJ]; o.num_predictions = c[MC_PRED];
        o.num_matches = c[MC_MATCH]; o.num_switches = c[MC_SWITCH]; o.num_misses = c[MC_MISS]; o.num_false_positives = c[MC_FP];
        o.mostly_tracked = c[MC_MT]; o.mostly_lost = c[MC_ML];
        o.num_unique_objects = seq_n_oid[s];
        o.idtp = idtp_host(edges.data() + seq_edge[s], seq_edge[s + 1] - seq_edge[s], seq_n_oid[s], seq_n_hid[s]);
        o.idfp = o.num_predictions - o.idtp; o.idfn = o.num_objects - o.idtp;
        o.dist_sum = dist[s];
    }
    return RTMODT_OK;
}

}  // extern "C"
