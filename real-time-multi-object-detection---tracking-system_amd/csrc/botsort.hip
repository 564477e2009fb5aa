// botsort.hip -- BoT-SORT (Aharon et al., "BoT-SORT: Robust Associations Multi-Pedestrian Tracking", 2022), the tracker the
// reference's comparison ranks best (TECHNICAL_DESIGN_DOCUMENT.md H.2, row 3: IDF1 0.83, 38 switches, "Req. Re-ID Model: Yes"), with
// the state resident on the device.  The rules are the published algorithm (bot_sort.py, kalman_filter.py, matching.py) as this
// project reads it, restated in tests/botsort_ref.py.  PARITY UNPINNED: BoT-SORT and boxmot are installed nowhere this runs; the
// kernel is pinned to the restatement, bit for bit.
//
// One call = a fixed number of launches for all streams, no host hop between them:
//   appearance_hist + appearance_quant (appearance.hip) or the network (reid.hip)   descriptors, unless the caller brings them
//   appearance_dotmax                  (appearance.hip)   track features x descriptors on the int8 matrix cores (one row per track)
//   botsort_update                     (here)             one 1024-thread workgroup per stream
// Motion only (embedder none) runs botsort_update alone.  Per frame and stream, float32 with one rounding per operation (FMA
// contraction off, correctly rounded division) unless said otherwise:
//   state     one list in creation order, deletions compacted; flag 1 = new (seen once, not activated), 2 = tracked, 3 = lost; ids
//             from 1 in detection order; frame_count in meta[5]
//   filter    8 states (cx, cy, w, h, vx, vy, vw, vh), weights 1/20 and 1/160; noise on x and w scales with w, on y and h with h
//             (initiate 2 sp / 10 sv, predict sp / sv, project sp).  The covariance is two symmetric 4x4 blocks, (cx, cy, vx, vy) and
//             (w, h, vw, vh), each held as its upper triangle row-major (cov[0:10], cov[10:20]); F, H, Q, R and the warp keep it so.
//             Predict: A + (B + B') + C, B + C, C over the 2x2 parts [[A, B], [B', C]], sums left to right, Q last.  Update of a
//             block with its 2-vector: S = A + diag(r); S^-1 by the adjugate, s11 / det, (-s01) / det, s00 / det with det =
//             s00 s11 - s01 s01; K = P H' S^-1 (two products, one sum per entry); x + (K0 y0 + K1 y1); P - K H P on the upper
//             triangle (DESIGN.md section 21 chose this form; the published P - K S K' rounds differently)
//   predict   tracked and lost tracks (a lost track's vw, vh are zeroed first); new tracks are not predicted; age += 1, tsu += 1
//   warp      the caller's 2x3 affine [R | t] of the stream, after predict, on every track: each pair (cx, cy), (w, h), (vx, vy),
//             (vw, vh) times R, t added to (cx, cy), each block M P M' with M = diag(R, R) as T = R X, then T R' per 2x2 part.  No
//             warp, or exactly the identity: the step is skipped and the state keeps its bits.  The six floats come by value in
//             the kernel arguments, or (warp_dev) from the device buffer the estimator of gmc.hip wrote them to
//   split     high: conf > track_high_thresh; low: track_low_thresh < conf < track_high_thresh (both strict), input order kept
//   feature   int8 descriptor rows f; a track holds s16[dim] (int16, norm 16256 = 127 * 128) and s8[dim] (the int8 row the matrix
//             cores read).  On a match v = 9 s16 + 128 f (a birth: v = 128 f) in int32, r = isqrt64(sum v^2), s16 = sign(v) ((16256 |v|
//             + r / 2) / r), s8 = sign(v) min(127, (127 |v| + r / 2) / r); r == 0: zeros.  That is the published alpha = 0.9 EMA with
//             renormalisation, in integers
//   cost      iou = iou_ref(box of the predicted mean, detection); d = 1.0 - (double)iou; far = d > proximity_thresh; with
//             fuse_score d = 1.0 - (double)iou * (double)conf; with Re-ID c = max(0, 16129 - <s8, f>), emb = (double)c / 32258.0,
//             emb = 1.0 when emb > appearance_thresh or far, cost = emb < d ? emb : d.  Admissible when cost <= thr; gain (thr +
//             1e-5) - cost in double; the matching is the maximum-gain one over the admissible pairs (assoc_sparse<double>)
//   first     tracked + lost tracks x high detections, thr = match_thresh.  Matched: filter update with (cx, cy, w, h) of the
//             detection, feature update, flag = 2, tsu = 0, last_frame = frame_count; the id is kept on re-activation
//   second    still unmatched tracks with flag 2 x low detections: cost 1.0 - (double)iou, thr 0.5; no feature update
//   lost      unmatched tracks with flag 2 get flag 3
//   new       tracks with flag 1 x remaining high detections: the fused cost, thr 0.7; matched: update, flag 2; unmatched: deleted
//   births    remaining high detections with conf >= new_track_thresh, detection order: flag 1, or 2 on the stream's first frame
//   expiry    a lost track with frame_count - last_frame > track_buffer is deleted
//   duplicate for every (not lost, lost) pair of the resulting list, births included, with 1.0 - (double)iou < 0.15 on the boxes of
//             the current means: the one with the shorter frame_count - start_frame is deleted, on a tie the one that is not lost.
//             All pairs are judged before any removal.  max_tracks is judged before the duplicates go; ids are not reused
//   returned  tracks with flag 2, matched this frame or not; their number goes to meta[3]
// lap.h's contested-pair limits (256 rows / 256 columns / 2048 pairs) raise the sticky error 2, more than max_tracks tracks error 1.
#include <vector>

#include "track_host.h"
#include "frame_stage.h"
#include "lap.h"

#include <climits>
#include <cmath>

namespace rtmodt {

#include "track_dev.h"

struct BotWarps { float m[BOT_MAX_STREAMS][6]; };            // by value in the kernel arguments: no copy to wait for

struct BotArgs {
    int max_tracks, max_dets, dim;                           // dim 0: motion only
    float high, low, newt; int track_buffer, fuse;
    double match, prox, app;
    BotState *states; int64_t *meta;                         // meta[stream][8] = {cur, n_tracks, err, n_returned, next_id, frame_count, 0, 0}
    const float4 *det_box; const float *det_conf; const int32_t *det_cls; const int32_t *det_n; int det_stride;
    const int8_t *desc; int desc_stride;                     // [stream][desc_stride][dim]
    const int32_t *dot;                                      // [stream][max_tracks][max_dets], columns = detection index
    int16_t *feat16; int8_t *feat8;                          // [stream][2][max_tracks][dim]
    int has_warp; BotWarps warp;
    const float *warp_dev;                                   // not null: [stream][6] on the device (gmc.hip), read instead of `warp`
};

constexpr float BOT_WP = 0.05f, BOT_WV = 0.00625f;
constexpr double BOT_SECOND = 0.5, BOT_NEW_MATCH = 0.7, BOT_DUP = 0.15;
constexpr long long BOT_DOT_ONE = 16129, BOT_FEAT_NORM = 16256;

struct BotKf { float4 pos, vel; float c[20]; };
__device__ __forceinline__ BotKf bot_load(const float4 *kf, int Mc, int i) {
    BotKf k;
    k.pos = kf[i]; k.vel = kf[Mc + i];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const float4 v = kf[(2 + q) * Mc + i];
        k.c[4 * q] = v.x; k.c[4 * q + 1] = v.y; k.c[4 * q + 2] = v.z; k.c[4 * q + 3] = v.w;
    }
    return k;
}
__device__ __forceinline__ void bot_store(float4 *kf, int Mc, int i, const BotKf &k) {
    kf[i] = k.pos; kf[Mc + i] = k.vel;
#pragma unroll
    for (int q = 0; q < 5; ++q) kf[(2 + q) * Mc + i] = float4{k.c[4 * q], k.c[4 * q + 1], k.c[4 * q + 2], k.c[4 * q + 3]};
}
__device__ __forceinline__ float4 bot_box_to_xywh(const float4 b) {
    const float w = b.z - b.x, h = b.w - b.y;
    return float4{b.x + w * 0.5f, b.y + h * 0.5f, w, h};
}
__device__ __forceinline__ float4 bot_mean_to_box(const float4 m) {
    const float x1 = m.x - m.z * 0.5f, y1 = m.y - m.w * 0.5f;
    return float4{x1, y1, x1 + m.z, y1 + m.w};
}
__device__ __forceinline__ BotKf bot_initiate(const float4 z) {
    BotKf k;
    k.pos = z; k.vel = float4{0.f, 0.f, 0.f, 0.f};
    const float spw = (2.0f * BOT_WP) * z.z, sph = (2.0f * BOT_WP) * z.w, svw = (10.0f * BOT_WV) * z.z, svh = (10.0f * BOT_WV) * z.w;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        float *P = k.c + 10 * b;
#pragma unroll
        for (int q = 0; q < 10; ++q) P[q] = 0.f;
        P[0] = spw * spw; P[4] = sph * sph; P[7] = svw * svw; P[9] = svh * svh;
    }
    return k;
}
// upper triangle of a block: 0 (0,0)  1 (0,1)  2 (0,2)  3 (0,3)  4 (1,1)  5 (1,2)  6 (1,3)  7 (2,2)  8 (2,3)  9 (3,3)
__device__ __forceinline__ void bot_blk_predict(float &p0, float &p1, const float v0, const float v1, float *P, const float qp0, const float qp1,
                                                const float qv0, const float qv1) {
    const float P00 = P[0], P01 = P[1], P02 = P[2], P03 = P[3], P11 = P[4], P12 = P[5], P13 = P[6], P22 = P[7], P23 = P[8], P33 = P[9];
    p0 = p0 + v0; p1 = p1 + v1;
    P[0] = ((P00 + (P02 + P02)) + P22) + qp0;
    P[1] = (P01 + (P03 + P12)) + P23;
    P[4] = ((P11 + (P13 + P13)) + P33) + qp1;
    P[2] = P02 + P22; P[3] = P03 + P23; P[5] = P12 + P23; P[6] = P13 + P33;
    P[7] = P22 + qv0; P[8] = P23; P[9] = P33 + qv1;
}
__device__ __forceinline__ void bot_predict(BotKf &k) {
    const float spw = BOT_WP * k.pos.z, sph = BOT_WP * k.pos.w, svw = BOT_WV * k.pos.z, svh = BOT_WV * k.pos.w;
    const float qp0 = spw * spw, qp1 = sph * sph, qv0 = svw * svw, qv1 = svh * svh;
    bot_blk_predict(k.pos.x, k.pos.y, k.vel.x, k.vel.y, k.c, qp0, qp1, qv0, qv1);
    bot_blk_predict(k.pos.z, k.pos.w, k.vel.z, k.vel.w, k.c + 10, qp0, qp1, qv0, qv1);
}
__device__ __forceinline__ void bot_blk_update(float &x0, float &x1, float &x2, float &x3, float *P, const float z0, const float z1, const float r0,
                                               const float r1) {
    const float G[4][4] = {{P[0], P[1], P[2], P[3]}, {P[1], P[4], P[5], P[6]}, {P[2], P[5], P[7], P[8]}, {P[3], P[6], P[8], P[9]}};
    const float s00 = G[0][0] + r0, s01 = G[0][1], s11 = G[1][1] + r1;
    const float det = s00 * s11 - s01 * s01;
    const float i00 = s11 / det, i01 = (-s01) / det, i11 = s00 / det;
    float K0[4], K1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        K0[k] = G[k][0] * i00 + G[k][1] * i01;
        K1[k] = G[k][0] * i01 + G[k][1] * i11;
    }
    const float y0 = z0 - x0, y1 = z1 - x1;
    x0 = x0 + (K0[0] * y0 + K1[0] * y1);
    x1 = x1 + (K0[1] * y0 + K1[1] * y1);
    x2 = x2 + (K0[2] * y0 + K1[2] * y1);
    x3 = x3 + (K0[3] * y0 + K1[3] * y1);
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int l = k; l < 4; ++l) P[n++] = G[k][l] - (K0[k] * G[0][l] + K1[k] * G[1][l]);
}
__device__ __forceinline__ void bot_update(BotKf &k, const float4 z) {
    const float spw = BOT_WP * k.pos.z, sph = BOT_WP * k.pos.w;
    const float r0 = spw * spw, r1 = sph * sph;
    bot_blk_update(k.pos.x, k.pos.y, k.vel.x, k.vel.y, k.c, z.x, z.y, r0, r1);
    bot_blk_update(k.pos.z, k.pos.w, k.vel.z, k.vel.w, k.c + 10, z.z, z.w, r0, r1);
}
// R X R' of a 2x2 part: T = R X, then T R'
__device__ __forceinline__ float4 bot_rxr(const float4 R, const float x00, const float x01, const float x10, const float x11) {
    const float t00 = R.x * x00 + R.y * x10, t01 = R.x * x01 + R.y * x11;
    const float t10 = R.z * x00 + R.w * x10, t11 = R.z * x01 + R.w * x11;
    return float4{t00 * R.x + t01 * R.y, t00 * R.z + t01 * R.w, t10 * R.x + t11 * R.y, t10 * R.z + t11 * R.w};
}
__device__ __forceinline__ void bot_pair(const float4 R, float &p, float &q) {
    const float a = p, b = q;
    p = R.x * a + R.y * b;
    q = R.z * a + R.w * b;
}
__device__ __forceinline__ void bot_warp(BotKf &k, const float4 R, const float tx, const float ty) {
    bot_pair(R, k.pos.x, k.pos.y); bot_pair(R, k.pos.z, k.pos.w); bot_pair(R, k.vel.x, k.vel.y); bot_pair(R, k.vel.z, k.vel.w);
    k.pos.x = k.pos.x + tx; k.pos.y = k.pos.y + ty;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        float *P = k.c + 10 * blk;
        const float4 a = bot_rxr(R, P[0], P[1], P[1], P[4]), b = bot_rxr(R, P[2], P[3], P[5], P[6]), c = bot_rxr(R, P[7], P[8], P[8], P[9]);
        P[0] = a.x; P[1] = a.y; P[2] = b.x; P[3] = b.y; P[4] = a.w; P[5] = b.z; P[6] = b.w; P[7] = c.x; P[8] = c.y; P[9] = c.w;
    }
}
// one step of the integer feature by a whole wave: s_in == nullptr is a birth.  s_in / o16 may be the same row.
__device__ __forceinline__ void bot_feat_step(const int16_t *s_in, const int8_t *f, int16_t *o16, int8_t *o8, int D, int lane) {
    long long v[8], n2 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int d = lane + 64 * k;
        v[k] = 0;
        if (d < D) {
            long long x = 128 * (long long)f[d];
            if (s_in) x += 9 * (long long)s_in[d];
            v[k] = x;
            n2 += x * x;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) n2 += __shfl_xor(n2, d);
    const long long r = isqrt64(n2);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int d = lane + 64 * k;
        if (d < D) {
            const long long a = v[k] < 0 ? -v[k] : v[k];
            long long q16 = 0, q8 = 0;
            if (r > 0) { q16 = (BOT_FEAT_NORM * a + r / 2) / r; q8 = min(127ll, (127 * a + r / 2) / r); }
            o16[d] = (int16_t)(v[k] < 0 ? -q16 : q16);
            o8[d] = (int8_t)(v[k] < 0 ? -q8 : q8);
        }
    }
}

__global__ __launch_bounds__(TRK_THREADS) void botsort_update(BotArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // every LDS byte is dynamic: the base stays 16-byte aligned
    const int s = blockIdx.x, tid = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Mc = a.max_tracks, Nc = a.max_dets, D = a.dim;
    float4 *tbox = (float4 *)smem;       // box of the track's mean: predicted, then current
    float4 *bbox = tbox + Mc;            // box of a birth's mean
    float4 *dbox = bbox + Mc;            // this frame's detections, input order
    float *dconf = (float *)(dbox + Nc);
    int *d_used = (int *)(dconf + Nc);   // detection -> matched
    int *cols = d_used + Nc;
    int *col_winner = cols + Nc;
    int *rows = col_winner + Nc;
    int *row_best = rows + Mc;
    int *rowcand = row_best + Mc;
    int *t_match = rowcand + Mc;         // track -> detection, -1 unmatched
    int *t_flag = t_match + Mc;
    int *t_feat = t_flag + Mc;           // the match updates the feature
    int *t_alive = t_feat + Mc;
    int *t_start = t_alive + Mc;
    int *t_kill = t_start + Mc;          // duplicate: an old track / a birth goes
    int *b_kill = t_kill + Mc;
    int *t_new = b_kill + Mc;            // track -> position in the next list
    int *lost = t_new + Mc;              // the lost tracks of the resulting list
    int *born = lost + Mc;               // the births that stay
    int *wsum = born + Mc;               // [TRK_WAVES + 1]
    int *shared = wsum + TRK_WAVES + 1;  // [0] assignment error, [1] returned tracks
    unsigned char *lap_base = (unsigned char *)(((uintptr_t)(shared + 2) + 7) & ~(uintptr_t)7);
    const LapSmemT<double> L = lap_carve_t<double>(lap_base, Nc);
    if (tid == 0) { shared[0] = 0; shared[1] = 0; }
    __syncthreads();

    BotState st = a.states[s];
    long long *meta = (long long *)a.meta + (size_t)s * 8;
    const int cur = (int)meta[0] & 1;
    const int M = min(max((int)meta[1], 0), Mc);
    const long long next_id = meta[4], frame_count = meta[5] + 1;
    const int fc = (int)frame_count;
#define BOT_SEL(f) auto *c_##f = cur ? st.f[1] : st.f[0]; auto *n_##f = cur ? st.f[0] : st.f[1]
    BOT_SEL(ids); BOT_SEL(dbox); BOT_SEL(conf); BOT_SEL(cls); BOT_SEL(flag); BOT_SEL(age); BOT_SEL(tsu); BOT_SEL(start); BOT_SEL(last); BOT_SEL(kf);
#undef BOT_SEL
    const size_t fbuf = (size_t)Mc * D;
    int16_t *c_f16 = a.feat16 + ((size_t)s * 2 + cur) * fbuf, *n_f16 = a.feat16 + ((size_t)s * 2 + (cur ^ 1)) * fbuf;
    int8_t *c_f8 = a.feat8 + ((size_t)s * 2 + cur) * fbuf, *n_f8 = a.feat8 + ((size_t)s * 2 + (cur ^ 1)) * fbuf;
    int n = a.det_n[s];
    n = min(max(n, 0), min(Nc, a.det_stride));
    const float4 *gb = a.det_box + (size_t)s * a.det_stride;
    const float *gc = a.det_conf + (size_t)s * a.det_stride;
    const int32_t *gk = a.det_cls + (size_t)s * a.det_stride;
    const int8_t *desc = a.desc + (size_t)s * a.desc_stride * D;
    const int32_t *dm = a.dot + (size_t)s * Mc * Nc;
    const float *wm = a.warp_dev ? a.warp_dev + 6 * s : a.warp.m[s];
    const float4 R = float4{wm[0], wm[1], wm[3], wm[4]};
    const float wtx = wm[2], wty = wm[5];
    const bool warped = (a.has_warp || a.warp_dev) && !(R.x == 1.0f && R.y == 0.0f && R.z == 0.0f && R.w == 1.0f && wtx == 0.0f && wty == 0.0f);

    // ---- predict, warp ----
    for (int i = tid; i < M; i += TRK_THREADS) {
        BotKf k = bot_load(c_kf, Mc, i);
        const int fl = c_flag[i];
        if (fl != 1) {
            if (fl == 3) { k.vel.z = 0.0f; k.vel.w = 0.0f; }
            bot_predict(k);
        }
        if (warped) bot_warp(k, R, wtx, wty);
        bot_store(c_kf, Mc, i, k);
        c_age[i] += 1;
        c_tsu[i] += 1;
        tbox[i] = bot_mean_to_box(k.pos);
        t_flag[i] = fl;
        t_match[i] = -1;
        t_feat[i] = 0;
        t_start[i] = c_start[i];
        t_kill[i] = 0;
    }
    for (int i = tid; i < Mc; i += TRK_THREADS) b_kill[i] = 0;
    for (int j = tid; j < n; j += TRK_THREADS) {
        dbox[j] = gb[j];
        dconf[j] = gc[j];
        d_used[j] = 0;
    }
    __syncthreads();
    const float high = a.high, low = a.low, newt = a.newt;
    auto is_high = [&](int j) { return dconf[j] > high; };
    auto is_low = [&](int j) { const float c = dconf[j]; return c > low && c < high; };
    auto take = [&](int nr, int feature) {                 // the matched pairs of the stage just solved
        for (int r = tid; r < nr; r += TRK_THREADS) {
            const int c = row_best[r];
            if (c >= 0 && col_winner[c] == r) { t_match[rows[r]] = cols[c]; t_feat[rows[r]] = feature; d_used[cols[c]] = 1; }
        }
        __syncthreads();
    };
    const double prox = a.prox, app = a.app;
    const bool fuse = a.fuse != 0, reid = D > 0;
    auto fused = [&](int i, int j, double thr, double &cost) -> bool {
        const float v = iou_ref(tbox[i], dbox[j]);
        double d = 1.0 - (double)v;
        const bool far = d > prox;
        if (fuse) d = 1.0 - (double)v * (double)dconf[j];
        double c = d;
        if (reid) {
            long long cc = BOT_DOT_ONE - (long long)dm[(size_t)i * Nc + j];
            if (cc < 0) cc = 0;
            double emb = (double)cc / 32258.0;
            if (emb > app || far) emb = 1.0;
            c = emb < d ? emb : d;
        }
        if (!(c <= thr)) return false;
        cost = c - (thr + 1e-5);
        return true;
    };

    // ---- first association: tracked + lost tracks against the high detections ----
    {
        const double thr = a.match;
        auto edge = [&](int r, int c, double &cost) -> bool { return fused(rows[r], cols[c], thr, cost); };
        const int nr = block_compact([&](int i) { return t_flag[i] != 1; }, M, rows, wsum);
        const int nc = nr ? block_compact(is_high, n, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge, nr, nc, row_best, col_winner, rowcand, L, wsum, &shared[0]);
            take(nr, 1);
        }
    }
    // ---- second association: the still unmatched tracked tracks against the low detections, plain IoU ----
    {
        auto edge = [&](int r, int c, double &cost) -> bool {
            const double d = 1.0 - (double)iou_ref(tbox[rows[r]], dbox[cols[c]]);
            if (!(d <= BOT_SECOND)) return false;
            cost = d - (BOT_SECOND + 1e-5);
            return true;
        };
        const int nr = block_compact([&](int i) { return t_flag[i] == 2 && t_match[i] < 0; }, M, rows, wsum);
        const int nc = nr ? block_compact(is_low, n, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge, nr, nc, row_best, col_winner, rowcand, L, wsum, &shared[0]);
            take(nr, 0);
        }
    }
    // ---- new tracks against the remaining high detections ----
    {
        auto edge = [&](int r, int c, double &cost) -> bool { return fused(rows[r], cols[c], BOT_NEW_MATCH, cost); };
        const int nr = block_compact([&](int i) { return t_flag[i] == 1; }, M, rows, wsum);
        const int nc = nr ? block_compact([&](int j) { return is_high(j) && !d_used[j]; }, n, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge, nr, nc, row_best, col_winner, rowcand, L, wsum, &shared[0]);
            take(nr, 1);
        }
    }

    // ---- update in place, life cycle ----
    for (int i = tid; i < M; i += TRK_THREADS) {
        const int j = t_match[i];
        int fl = t_flag[i], alive = 1;
        if (j >= 0) {
            BotKf k = bot_load(c_kf, Mc, i);
            bot_update(k, bot_box_to_xywh(dbox[j]));
            bot_store(c_kf, Mc, i, k);
            tbox[i] = bot_mean_to_box(k.pos);
            fl = 2;
            c_tsu[i] = 0; c_last[i] = fc;
            c_dbox[i] = dbox[j]; c_conf[i] = dconf[j]; c_cls[i] = gk[j];
        } else {
            if (fl == 1) alive = 0;
            if (fl == 2) fl = 3;
            if (fc - c_last[i] > a.track_buffer) alive = 0;
        }
        t_flag[i] = fl;
        t_alive[i] = alive;
    }
    if (reid)
        for (int i = wave; i < M; i += TRK_WAVES)             // a wave per track
            if (t_match[i] >= 0 && t_feat[i])
                bot_feat_step(c_f16 + (size_t)i * D, desc + (size_t)t_match[i] * D, c_f16 + (size_t)i * D, c_f8 + (size_t)i * D, D, lane);
    __syncthreads();
    const int kept = block_compact([&](int i) { return t_alive[i] != 0; }, M, rows, wsum);
    // ---- births, detection order ----
    int nsp = block_compact([&](int j) { return is_high(j) && !d_used[j] && dconf[j] >= newt; }, n, cols, wsum);
    int err = 0;
    if (kept + nsp > Mc) { err = 1; nsp = Mc - kept; }
    for (int q = tid; q < nsp; q += TRK_THREADS) bbox[q] = bot_mean_to_box(bot_box_to_xywh(dbox[cols[q]]));
    // ---- duplicates: every (not lost, lost) pair of the list, judged before any removal ----
    const int nl = block_compact([&](int i) { return t_alive[i] && t_flag[i] == 3; }, M, lost, wsum);
    if (nl > 0) {
        const int total = (kept + nsp) * nl;
        for (int idx = tid; idx < total; idx += TRK_THREADS) {
            const int pi = idx / nl, q = lost[idx - pi * nl];
            const int p = pi < kept ? rows[pi] : -1;
            if (p >= 0 && t_flag[p] == 3) continue;
            const float4 pb = p >= 0 ? tbox[p] : bbox[pi - kept];
            const int tp = p >= 0 ? fc - t_start[p] : 0, tq = fc - t_start[q];
            if (1.0 - (double)iou_ref(pb, tbox[q]) < BOT_DUP) {
                if (tp > tq) t_kill[q] = 1;
                else if (p >= 0) t_kill[p] = 1;
                else b_kill[pi - kept] = 1;
            }
        }
    }
    __syncthreads();
    // ---- compaction into the other buffer ----
    const int kept2 = block_compact([&](int i) { return t_alive[i] && !t_kill[i]; }, M, rows, wsum);
    const int nb = block_compact([&](int q) { return !b_kill[q]; }, nsp, born, wsum);
    for (int i = tid; i < M; i += TRK_THREADS) t_new[i] = -1;
    __syncthreads();
    for (int o = tid; o < kept2; o += TRK_THREADS) t_new[rows[o]] = o;
    __syncthreads();
    for (int i = tid; i < M; i += TRK_THREADS) {
        const int o = t_new[i];
        if (o < 0) continue;
        const int fl = t_flag[i];
        n_ids[o] = c_ids[i]; n_dbox[o] = c_dbox[i]; n_conf[o] = c_conf[i]; n_cls[o] = c_cls[i]; n_flag[o] = fl; n_age[o] = c_age[i];
        n_tsu[o] = c_tsu[i]; n_start[o] = c_start[i]; n_last[o] = c_last[i];
        bot_store(n_kf, Mc, o, bot_load(c_kf, Mc, i));
        if (fl == 2) atomicAdd(&shared[1], 1);
    }
    if (reid) {
        const int D16 = D / 16, D8 = D / 8;
        for (int idx = tid; idx < kept2 * D16; idx += TRK_THREADS) {
            const int o = idx / D16, part = idx - o * D16;
            *(int4 *)(n_f8 + (size_t)o * D + part * 16) = *(const int4 *)(c_f8 + (size_t)rows[o] * D + part * 16);
        }
        for (int idx = tid; idx < kept2 * D8; idx += TRK_THREADS) {
            const int o = idx / D8, part = idx - o * D8;
            *(int4 *)(n_f16 + (size_t)o * D + part * 8) = *(const int4 *)(c_f16 + (size_t)rows[o] * D + part * 8);
        }
    }
    for (int b = tid; b < nb; b += TRK_THREADS) {
        const int q = born[b], j = cols[q], o = kept2 + b;
        const int fl = fc == 1 ? 2 : 1;
        n_ids[o] = next_id + q; n_dbox[o] = dbox[j]; n_conf[o] = dconf[j]; n_cls[o] = gk[j]; n_flag[o] = fl; n_age[o] = 0; n_tsu[o] = 0;
        n_start[o] = fc; n_last[o] = fc;
        bot_store(n_kf, Mc, o, bot_initiate(bot_box_to_xywh(dbox[j])));
        if (fl == 2) atomicAdd(&shared[1], 1);
    }
    if (reid)
        for (int b = wave; b < nb; b += TRK_WAVES)
            bot_feat_step(nullptr, desc + (size_t)cols[born[b]] * D, n_f16 + (size_t)(kept2 + b) * D, n_f8 + (size_t)(kept2 + b) * D, D, lane);
    __syncthreads();
    if (tid == 0) {
        meta[0] = cur ^ 1;
        meta[1] = kept2 + nb;
        if (err) meta[2] = 1;
        else if (shared[0]) meta[2] = shared[0];
        meta[3] = shared[1];
        meta[4] = next_id + nsp;
        meta[5] = frame_count;
    }
}

static size_t bot_smem_bytes(int Mc, int Nc) {
    return (size_t)Mc * (16 * 2 + 4 * 13) + (size_t)Nc * (16 + 4 + 4 * 3) + (TRK_WAVES + 1 + 2) * 4 + 16 + lap_smem_bytes(Nc);
}

static int launch_botsort_update(const BotArgs &a, int n_streams, hipStream_t s) {
    const size_t smem = bot_smem_bytes(a.max_tracks, a.max_dets);
    RT_CHECK(smem <= 150 * 1024, RTMODT_E_INVALID, "botsort: max_tracks %d / max_dets %d need %zu B of LDS", a.max_tracks, a.max_dets, smem);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)botsort_update, smem, seen));
    hipLaunchKernelGGL(botsort_update, dim3(n_streams), dim3(TRK_THREADS), smem, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

}  // namespace rtmodt

using namespace rtmodt;

struct rtmodt_botsort : TrackHandleBase {
    EventTimer<4> timer;                   // describe | distance | update boundaries of the last call
    bool described = false;
    rtmodt_botsort_cfg cfg = {};
    int dim = 0;                             // 0: motion only
    char *pool = nullptr;                    // all state arrays but the features (track_layout.h: carve_botsort)
    BotState *d_states = nullptr; std::vector<BotState> h_states;
    int16_t *d_feat16 = nullptr; int8_t *d_feat8 = nullptr;        // [S][2][Mc][dim]
    int8_t *d_desc = nullptr; int32_t *d_counts = nullptr, *d_dot = nullptr;
    FrameStage stage;                        // host frames
    rtmodt_reid *reid = nullptr;             // embedder = a .rtreid file
};

namespace rtmodt {
int botsort_device_view(rtmodt_botsort *t, BotDeviceView *out) {
    RT_CHECK(t && out, RTMODT_E_INVALID, "null argument");
    out->states = t->d_states;
    return track_view(t, out);
}
int botsort_feature_view(rtmodt_botsort *t, const int8_t **feat8, int *dim) {
    RT_CHECK(t && feat8 && dim, RTMODT_E_INVALID, "null argument");
    *feat8 = t->d_feat8; *dim = t->dim;
    return RTMODT_OK;
}
}  // namespace rtmodt

static int bot_create_impl(rtmodt_botsort *t) {
    RT_TRY(track_open(t));
    RT_TRY(t->timer.create());
    t->h_states.assign(t->S, BotState{});
    const size_t total = carve_botsort(t->h_states.data(), t->S, t->Mc, nullptr);
    RT_HIP(hipMalloc((void **)&t->pool, total));
    RT_HIP(handle_zero(t->pool, total, t->stream));
    carve_botsort(t->h_states.data(), t->S, t->Mc, t->pool);
    RT_HIP(hipMalloc((void **)&t->d_states, sizeof(BotState) * t->S));
    RT_HIP(hipMemcpy(t->d_states, t->h_states.data(), sizeof(BotState) * t->S, hipMemcpyHostToDevice));
    if (!t->dim) return RTMODT_OK;
    const size_t F = (size_t)t->S * 2 * t->Mc * t->dim, SN = (size_t)t->S * t->Nc;
    RT_HIP(hipMalloc((void **)&t->d_feat16, F * 2)); RT_HIP(handle_zero(t->d_feat16, F * 2, t->stream));
    RT_HIP(hipMalloc((void **)&t->d_feat8, F)); RT_HIP(handle_zero(t->d_feat8, F, t->stream));
    RT_HIP(hipMalloc((void **)&t->d_desc, SN * t->dim)); RT_HIP(handle_zero(t->d_desc, SN * t->dim, t->stream));
    RT_HIP(hipMalloc((void **)&t->d_counts, SN * APP_DIM * 4));
    RT_HIP(hipMalloc((void **)&t->d_dot, (size_t)t->S * t->Mc * t->Nc * 4));
    RT_HIP(handle_zero(t->d_dot, (size_t)t->S * t->Mc * t->Nc * 4, t->stream));
    return RTMODT_OK;
}

static BotArgs bot_args(rtmodt_botsort *t, const float *warp, int count) {
    BotArgs a{};
    a.max_tracks = t->Mc; a.max_dets = t->Nc; a.dim = t->dim;
    a.high = t->cfg.track_high_thresh; a.low = t->cfg.track_low_thresh; a.newt = t->cfg.new_track_thresh; a.track_buffer = t->cfg.track_buffer;
    a.fuse = t->cfg.fuse_score ? 1 : 0; a.match = t->cfg.match_thresh; a.prox = t->cfg.proximity_thresh; a.app = t->cfg.appearance_thresh;
    a.states = t->d_states; a.meta = t->d_meta;
    a.det_box = t->d_box; a.det_conf = t->d_conf; a.det_cls = t->d_cls; a.det_n = t->d_n; a.det_stride = t->Nc;
    a.desc = t->d_desc; a.desc_stride = t->Nc; a.dot = t->d_dot; a.feat16 = t->d_feat16; a.feat8 = t->d_feat8;
    a.has_warp = warp != nullptr;
    if (warp) memcpy(a.warp.m, warp, sizeof(float) * 6 * count);
    return a;
}

// the launches of one call on stream q, detections described by `a`'s det_* fields for streams [0, count)
static int bot_run(rtmodt_botsort *t, const BotArgs &a, int count, const AppFrames *frames, int fh, int fw, int pitch, hipStream_t q) {
    RT_TRY(t->timer.record(0, q));
    t->described = frames != nullptr;
    if (frames && t->reid) {
        RT_TRY(reid_run(t->reid, *frames, count, fh, fw, pitch, a.det_box, a.det_n, a.det_stride, std::min(a.det_stride, t->Nc), t->d_desc, t->Nc, q));
    } else if (frames) {
        DescribeArgs d{};
        d.frames = *frames; d.h = fh; d.w = fw; d.pitch = pitch;
        d.box = a.det_box; d.box_n = a.det_n; d.box_stride = a.det_stride; d.max_boxes = std::min(a.det_stride, t->Nc);
        d.counts = t->d_counts; d.desc = t->d_desc; d.desc_stride = t->Nc;
        RT_TRY(launch_describe(d, count, q));
    }
    RT_TRY(t->timer.record(1, q));
    if (t->dim) {
        DotmaxArgs m{};
        m.gallery = t->d_feat8; m.gallery_stream_stride = (size_t)2 * t->Mc * t->dim; m.gallery_cur_stride = (size_t)t->Mc * t->dim;
        m.meta = t->d_meta; m.meta_rows = 1;
        m.budget = 1; m.dim = t->dim; m.dets = t->d_desc; m.det_stride = t->Nc; m.n_dets_dev = a.det_n; m.max_dets = std::min(a.det_stride, t->Nc);
        m.out = t->d_dot; m.out_stream_stride = (size_t)t->Mc * t->Nc; m.out_row_stride = t->Nc;
        RT_TRY(launch_dotmax(m, t->Mc, m.max_dets, count, q));
    }
    RT_TRY(t->timer.record(2, q));
    RT_TRY(launch_botsort_update(a, count, q));
    RT_TRY(t->timer.record(3, q));
    t->timer.timed = true;
    return RTMODT_OK;
}

static int bot_check_sticky(rtmodt_botsort *t, int s, int64_t err) { return track_check_sticky(t, s, err, "assignment"); }

// frames of a call -> device pointers (host frames are staged on stream q), as DeepSORT takes them
static int bot_stage(rtmodt_botsort *t, const uint8_t *const *frames, int count, int fh, int fw, int pitch, int mem_kind, hipStream_t q, AppFrames *out) {
    RT_CHECK(t->reid || t->dim == APP_DIM, RTMODT_E_INVALID, "this handle takes caller descriptors of dimension %d; the built-in descriptor has %d", t->dim, APP_DIM);
    RT_TRY(check_frames(frames, count, fh, fw, pitch, mem_kind, kAppFrames));
    RT_TRY(t->stage.in(frames, count, fh, fw, pitch, mem_kind, q, FRAMES_AS_GIVEN));
    for (int i = 0; i < count; ++i) out->p[i] = t->stage.at(frames, i);
    return RTMODT_OK;
}

extern "C" {

int rtmodt_botsort_check_warp(const float *warp, int n_streams) {
    RT_CHECK(n_streams >= 1 && n_streams <= BOT_MAX_STREAMS, RTMODT_E_INVALID, "n_streams %d", n_streams);
    if (!warp) return RTMODT_OK;
    for (int s = 0; s < n_streams; ++s) {
        const float *w = warp + 6 * s;
        for (int k = 0; k < 6; ++k) RT_CHECK(w[k] == w[k] && w[k] - w[k] == 0.0f, RTMODT_E_INVALID, "stream %d: warp entry %d is not finite", s, k);
        const double det = (double)w[0] * (double)w[4] - (double)w[1] * (double)w[3];
        RT_CHECK(std::fabs(det) >= 1e-6, RTMODT_E_INVALID, "stream %d: the warp is singular (|det R| = %g < 1e-6)", s, std::fabs(det));
    }
    return RTMODT_OK;
}

void rtmodt_botsort_destroy(rtmodt_botsort *t) {
    if (!t) return;
    track_close(t, [t] {
        t->timer.destroy();
        hipFree(t->pool); hipFree(t->d_states); hipFree(t->d_feat16); hipFree(t->d_feat8); hipFree(t->d_desc); hipFree(t->d_counts); hipFree(t->d_dot);
        t->stage.release();
        reid_close(t->reid);
    });
    delete t;
}

int rtmodt_botsort_create(const rtmodt_botsort_cfg *cfg, rtmodt_botsort **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    const char *e = cfg->embedder;
    const size_t elen = e ? strlen(e) : 0;
    const bool none = !e || !*e || strcmp(e, "none") == 0;
    const bool net = elen > 7 && strcmp(e + elen - 7, ".rtreid") == 0;
    RT_CHECK(none || net || strcmp(e, "colorhist") == 0, RTMODT_E_UNSUPPORTED,
             "embedder '%s': only the built-in \"colorhist\" descriptor and an OSNet x0.25 .rtreid file (tools/convert_weights.py --reid) are computed "
             "here; bring embeddings of another model as caller descriptors", e);
    RT_CHECK(!net || cfg->dim == 0 || cfg->dim == 512, RTMODT_E_INVALID, "descriptor dimension %d: the network's is 512 (or 0)", cfg->dim);
    RT_CHECK(!none || cfg->dim == 0, RTMODT_E_INVALID, "descriptor dimension %d without an embedder: caller descriptors go with embedder \"colorhist\"", cfg->dim);
    const int dim = none ? 0 : net ? 512 : cfg->dim ? cfg->dim : APP_DIM;
    RT_CHECK(dim == 0 || (dim >= 64 && dim <= 512 && dim % 64 == 0), RTMODT_E_INVALID, "descriptor dimension %d: 64..512 in multiples of 64", dim);
    const auto fin = [](double v) { return v == v && v - v == 0.0; };
    RT_CHECK(fin(cfg->track_high_thresh) && fin(cfg->track_low_thresh) && fin(cfg->new_track_thresh) && fin(cfg->match_thresh) && fin(cfg->proximity_thresh) &&
                 fin(cfg->appearance_thresh) && cfg->match_thresh >= 0 && cfg->match_thresh <= 1 && cfg->track_buffer >= 1 && cfg->track_buffer <= 100000,
             RTMODT_E_INVALID, "bad parameter (track_high_thresh %g, track_low_thresh %g, new_track_thresh %g, track_buffer %d, match_thresh %g, "
             "proximity_thresh %g, appearance_thresh %g)", (double)cfg->track_high_thresh, (double)cfg->track_low_thresh, (double)cfg->new_track_thresh,
             cfg->track_buffer, cfg->match_thresh, cfg->proximity_thresh, cfg->appearance_thresh);
    RT_CHECK(cfg->max_tracks >= 1 && cfg->max_dets >= 1 && cfg->n_streams >= 1, RTMODT_E_INVALID, "max_tracks %d / max_dets %d / n_streams %d must be positive",
             cfg->max_tracks, cfg->max_dets, cfg->n_streams);
    RT_CHECK(cfg->max_tracks <= BOT_MAX_TRACKS && cfg->max_dets <= BOT_MAX_DETS && cfg->n_streams <= BOT_MAX_STREAMS, RTMODT_E_CAPACITY,
             "max_tracks %d / max_dets %d / n_streams %d: at most %d / %d / %d", cfg->max_tracks, cfg->max_dets, cfg->n_streams, BOT_MAX_TRACKS, BOT_MAX_DETS,
             BOT_MAX_STREAMS);
    rtmodt_botsort *t = new rtmodt_botsort();
    t->cfg = *cfg; t->cfg.embedder = nullptr;
    t->device = cfg->device; t->S = cfg->n_streams; t->Mc = cfg->max_tracks; t->Nc = cfg->max_dets; t->dim = dim;
    int rc = net ? reid_open(e, cfg->device, cfg->n_streams, cfg->max_dets, false, &t->reid) : RTMODT_OK;     // the file is checked before the device is touched
    if (rc == RTMODT_OK) rc = bot_create_impl(t);
    return handle_created(rc, t, rtmodt_botsort_destroy, out);
}

int rtmodt_botsort_reset(rtmodt_botsort *t, int stream) { return track_reset_meta(t, stream); }

int rtmodt_botsort_update_batch(rtmodt_botsort *t, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                                const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind, const int8_t *desc, const float *warp,
                                int32_t *n_returned_out) {
    bool any = false;
    RT_TRY(track_batch_check(t, xyxy, conf, cls, n, &any));
    RT_CHECK(!(frames && desc), RTMODT_E_INVALID, "give frames or descriptors, not both");
    RT_CHECK(t->dim || !(frames || desc), RTMODT_E_INVALID, "this handle tracks on motion only (embedder none): it takes neither frames nor descriptors");
    RT_CHECK(!(t->reid && desc), RTMODT_E_INVALID, "this handle computes its descriptors with its embedder network: give frames, not descriptors");
    RT_CHECK(!t->dim || !any || frames || desc, RTMODT_E_INVALID, "detections need frames (built-in descriptor) or caller descriptors");
    RT_TRY(rtmodt_botsort_check_warp(warp, t->S));
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    hipStream_t q = t->stream;
    AppFrames fp{};
    if (frames && any) RT_TRY(bot_stage(t, frames, t->S, h, w, stride_bytes, mem_kind, q, &fp));
    RT_TRY(track_batch_stage(t, xyxy, conf, cls, n, any));
    if (any && desc) RT_HIP(hipMemcpyAsync(t->d_desc, desc, (size_t)t->S * t->Nc * t->dim, hipMemcpyHostToDevice, q));
    RT_TRY(bot_run(t, bot_args(t, warp, t->S), t->S, frames && any ? &fp : nullptr, h, w, stride_bytes, q));
    RT_HIP(hipMemcpyAsync(t->h_meta, t->d_meta, sizeof(int64_t) * 8 * t->S, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    for (int s = 0; s < t->S; ++s)
        if (n_returned_out) n_returned_out[s] = (int32_t)t->h_meta[8 * s + 3];
    for (int s = 0; s < t->S; ++s) RT_TRY(bot_check_sticky(t, s, t->h_meta[8 * s + 2]));
    return RTMODT_OK;
}

int rtmodt_botsort_update_from_detector(rtmodt_botsort *t, rtmodt_detector *det, const uint8_t *const *frames, int n_frames, int h, int w,
                                        int stride_bytes, int mem_kind, const float *warp) {
    RT_CHECK(t && det, RTMODT_E_INVALID, "null argument");
    RT_CHECK(t->dim ? frames != nullptr : frames == nullptr, RTMODT_E_INVALID,
             t->dim ? "this handle describes the detections: give the frames the detector ran on" : "this handle tracks on motion only (embedder none): it takes no frames");
    RT_CHECK(!t->dim || t->reid || t->dim == APP_DIM, RTMODT_E_INVALID, "a handle for caller descriptors cannot describe a detector's boxes");
    DetOutputs o;
    RT_TRY(track_detector_outputs(t, det, &o));
    RT_CHECK(!frames || n_frames == o.count, RTMODT_E_INVALID, "%d frames for the detector's batch of %d", n_frames, o.count);
    RT_TRY(rtmodt_botsort_check_warp(warp, o.count >= 1 && o.count <= BOT_MAX_STREAMS ? o.count : 1));
    RT_TRY(track_detector_fits(t, o, o.count));
    AppFrames fp{};
    if (frames) RT_TRY(bot_stage(t, frames, o.count, h, w, stride_bytes, mem_kind, o.stream, &fp));
    BotArgs a = bot_args(t, warp, o.count);                // the warp travels in the kernel arguments: nothing to copy, nothing to wait for
    a.det_box = o.box; a.det_conf = o.conf; a.det_cls = o.cls; a.det_n = o.n; a.det_stride = o.stride;
    RT_TRY(bot_run(t, a, o.count, frames ? &fp : nullptr, h, w, stride_bytes, o.stream));
    return track_detector_done(t, o.stream);
}

int rtmodt_botsort_update_from_detector_gmc(rtmodt_botsort *t, rtmodt_detector *det, rtmodt_gmc *gmc, const uint8_t *const *frames, int n_frames, int h,
                                            int w, int stride_bytes, int mem_kind) {
    RT_CHECK(t && det && gmc && frames, RTMODT_E_INVALID, "null argument");
    RT_CHECK(!t->dim || t->reid || t->dim == APP_DIM, RTMODT_E_INVALID, "a handle for caller descriptors cannot describe a detector's boxes");
    DetOutputs o;
    RT_TRY(track_detector_outputs(t, det, &o));
    RT_CHECK(n_frames == o.count, RTMODT_E_INVALID, "%d frames for the detector's batch of %d", n_frames, o.count);
    RT_TRY(track_detector_fits(t, o, o.count));
    const float *warp_dev = nullptr;
    RT_TRY(gmc_enqueue_detector(gmc, o, frames, n_frames, h, w, stride_bytes, mem_kind, &warp_dev));      // first: refused before anything of this call is queued
    AppFrames fp{};
    if (t->dim) RT_TRY(bot_stage(t, frames, o.count, h, w, stride_bytes, mem_kind, o.stream, &fp));
    BotArgs a = bot_args(t, nullptr, o.count);
    a.warp_dev = warp_dev;
    a.det_box = o.box; a.det_conf = o.conf; a.det_cls = o.cls; a.det_n = o.n; a.det_stride = o.stride;
    RT_TRY(bot_run(t, a, o.count, t->dim ? &fp : nullptr, h, w, stride_bytes, o.stream));
    return track_detector_done(t, o.stream);
}

int rtmodt_botsort_state(rtmodt_botsort *t, int stream, int64_t *ids, int32_t *flag, int32_t *age, int32_t *tsu, int32_t *start_frame,
                         int32_t *last_frame, float *xyxy, float *conf, int32_t *cls, float *mean, float *cov, int16_t *feat16, int8_t *feat8,
                         int32_t *n, int64_t *next_id, int64_t *frame_count) {
    RT_CHECK(t && stream >= 0 && stream < t->S, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    RT_HIP(hipStreamSynchronize(t->stream));
    int64_t m[8];
    RT_HIP(hipMemcpy(m, t->d_meta + 8 * stream, sizeof(m), hipMemcpyDeviceToHost));
    const int cur = (int)m[0] & 1, cnt = (int)m[1];
    RT_CHECK(cnt >= 0 && cnt <= t->Mc, RTMODT_E_INVALID, "stream %d: corrupt track count", stream);
    if (n) *n = cnt;
    if (next_id) *next_id = m[4];
    if (frame_count) *frame_count = m[5];
    const BotState &st = t->h_states[stream];
    const size_t c = (size_t)cnt;
    if (cnt) {
        if (ids) RT_HIP(hipMemcpy(ids, st.ids[cur], c * 8, hipMemcpyDeviceToHost));
        if (flag) RT_HIP(hipMemcpy(flag, st.flag[cur], c * 4, hipMemcpyDeviceToHost));
        if (age) RT_HIP(hipMemcpy(age, st.age[cur], c * 4, hipMemcpyDeviceToHost));
        if (tsu) RT_HIP(hipMemcpy(tsu, st.tsu[cur], c * 4, hipMemcpyDeviceToHost));
        if (start_frame) RT_HIP(hipMemcpy(start_frame, st.start[cur], c * 4, hipMemcpyDeviceToHost));
        if (last_frame) RT_HIP(hipMemcpy(last_frame, st.last[cur], c * 4, hipMemcpyDeviceToHost));
        if (xyxy) RT_HIP(hipMemcpy(xyxy, st.dbox[cur], c * 16, hipMemcpyDeviceToHost));
        if (conf) RT_HIP(hipMemcpy(conf, st.conf[cur], c * 4, hipMemcpyDeviceToHost));
        if (cls) RT_HIP(hipMemcpy(cls, st.cls[cur], c * 4, hipMemcpyDeviceToHost));
        if (mean || cov) {
            std::vector<float4> buf((size_t)7 * t->Mc);
            RT_HIP(hipMemcpy(buf.data(), st.kf[cur], buf.size() * sizeof(float4), hipMemcpyDeviceToHost));
            botsort_unpack(&buf[0].x, t->Mc, cnt, mean, cov);
        }
        if (t->dim) {
            const size_t off = ((size_t)stream * 2 + cur) * t->Mc * t->dim;
            if (feat16) RT_HIP(hipMemcpy(feat16, t->d_feat16 + off, c * t->dim * 2, hipMemcpyDeviceToHost));
            if (feat8) RT_HIP(hipMemcpy(feat8, t->d_feat8 + off, c * t->dim, hipMemcpyDeviceToHost));
        }
    }
    return bot_check_sticky(t, stream, m[2]);              // after the copies: a stream in error stays readable
}

int rtmodt_botsort_last_ms(rtmodt_botsort *t, float *describe_ms, float *distance_ms, float *update_ms) {
    RT_CHECK(t, RTMODT_E_INVALID, "null argument");
    float a = 0, b = 0, c = 0;
    RT_TRY(t->timer.elapsed(t->device, 2, 3, &c, "no update has run yet"));      // (the last event first: it waits for the call)
    RT_TRY(t->timer.elapsed(t->device, 0, 1, &a, "no update has run yet"));
    RT_TRY(t->timer.elapsed(t->device, 1, 2, &b, "no update has run yet"));
    if (describe_ms) *describe_ms = t->described ? a : 0.f;
    if (distance_ms) *distance_ms = t->dim ? b : 0.f;
    if (update_ms) *update_ms = c;
    return RTMODT_OK;
}

}  // extern "C"
