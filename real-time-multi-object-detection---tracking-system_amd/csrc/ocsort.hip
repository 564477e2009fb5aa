// ocsort.hip -- OC-SORT (Cao et al., "Observation-Centric SORT", CVPR 2023), the motion-only tracker of the reference's tracker
// comparison (TECHNICAL_DESIGN_DOCUMENT.md H.2, row 4: no Re-ID model), with the state resident on the device.  The rules are the
// published algorithm (ocsort.py, association.py, kalmanfilter.py) as this project reads it, restated in tests/ocsort_ref.py.
// PARITY UNPINNED: ocsort, boxmot and filterpy are installed nowhere this runs; the kernel is pinned to the restatement, bit for bit.
//
// One call = ONE launch for all streams (ocsort_update: one 1024-thread workgroup per stream, the frame's working set in LDS, the
// pair gains computed where they are needed -- 256 x 1024 pairs are never stored), whatever the track and detection counts; no host
// hop.  Per frame and stream, in float32 with one rounding per operation unless said otherwise:
//   split     high: conf > det_thresh; low: low_thresh < conf < det_thresh (both strict; a confidence equal to det_thresh is in
//             neither set); low detections are used only with use_byte
//   filter    SORT's 7-state filter on (x, y, s = w h, r = w / (h + 1e-6)) with velocities for x, y, s: the block-diagonal Kf of
//             track_dev.h with constant noises, r the fourth lane with zero velocity and zero cross terms.  P0 = diag(10, 10, 10, 10,
//             1e4, 1e4, 1e4), Q = diag(1, 1, 1, 1, 1e-2, 1e-2, 1e-4), R = diag(1, 1, 10, 10); covariance update P - K H P (filterpy's
//             Joseph form rounds differently).  Box of a state: w = sqrt(s r), h = s / w, (x -+ w / 2, y -+ h / 2)
//   predict   if s + vs <= 0 then vs = 0; predict; age += 1; if tsu > 0 then hit_streak = 0; tsu += 1.  A track whose predicted box
//             has a non-finite coordinate is deleted: it takes no part in the frame
//   OCM       high detections x predicted boxes: admissible when iou_ref >= iou_threshold; gain (float64) = iou + angle, angle =
//             ((pi/2 - acos_fixed(c)) / pi) * inertia * conf_det for a track with an observation (hits > 0), else 0; c = the float32
//             dot product, clamped to [-1, 1], of the track's stored direction ((0, 0) when none) and the unit direction (dy, dx) /
//             (sqrt(dx^2 + dy^2) + 1e-6) from the centre of the track's reference observation to the detection's centre.  Reference
//             observation: the one stored at age - delta_t, else the nearest later stored age below age, else the last observation.
//             create refuses iou_threshold <= inertia / 2 (our rule), so every admissible gain is positive for conf <= 1; a pair
//             whose gain is not positive is inadmissible
//   BYTE      (use_byte) low detections x predicted boxes of the still unmatched tracks: iou >= iou_threshold, gain = iou
//   OCR       still unmatched high detections x LAST OBSERVATIONS of the still unmatched tracks that have one: same rule
//   update    matched with detection z: a track with an observation takes the unit direction from its reference observation to z and,
//             if tsu >= 2, is first re-updated (ORU): the filter state saved at its first missed frame walks g = tsu virtual
//             observations last + i (z - last) / g in (x, y, w, h), i = 1..g, s = w h, r = w / h, update then predict (the plain filter
//             predict), the last step update only.  Then the ordinary update with z (the endpoint is applied twice, as published);
//             last observation = z, ring[age] = z, tsu = 0, hits += 1, hit_streak += 1.  Unmatched with tsu == 1: the (predicted)
//             filter state is saved.  Unmatched with tsu > max_age: deleted
//   births    every unmatched high detection, in detection order: hits = hit_streak = age = tsu = 0, no observation, no direction,
//             ids from 1; the box, confidence and class it reports until its first match are the detection's
//   returned  tsu == 0 and (hit_streak >= min_hits or frame_count <= min_hits); list order = creation order, deletions compacted
// Every matching is the exact maximum of the summed gain over the admissible pairs (assoc_sparse<double> of track_dev.h: the
// isolated-pair shortcut in front of lap.h's solver); the published code runs the Hungarian method on the dense matrix and drops
// pairs below the threshold afterwards.  lap.h's contested-pair limits (256 rows / 256 columns / 2048 pairs) raise the sticky error 2.
#include <vector>

#include "track_host.h"
#include "lap.h"

#include <climits>
#include <cmath>

namespace rtmodt {

#include "track_dev.h"
#include "wg_dev.h"

struct OcArgs {
    int max_tracks, max_dets;
    float det_thresh, low_thresh, iou_thr; double inertia; int max_age, min_hits, delta_t, use_byte;
    OcState *states; int64_t *meta;          // meta[stream][8] = {cur, n_tracks, err, n_returned, next_id, frame_count, 0, 0}
    const float4 *det_box; const float *det_conf; const int32_t *det_cls; const int32_t *det_n; int det_stride;
};

__device__ __forceinline__ void oc_predict(Kf &k) {
    kf_predict1(k.pos.x, k.vel.x, k.pa.x, k.pb.x, k.pc.x, 1.0f, 1e-2f);
    kf_predict1(k.pos.y, k.vel.y, k.pa.y, k.pb.y, k.pc.y, 1.0f, 1e-2f);
    kf_predict1(k.pos.z, k.vel.z, k.pa.z, k.pb.z, k.pc.z, 1.0f, 1e-4f);
    kf_predict1(k.pos.w, k.vel.w, k.pa.w, k.pb.w, k.pc.w, 1.0f, 0.0f);
}
__device__ __forceinline__ void oc_update(Kf &k, const float4 z) {
    kf_update1(k.pos.x, k.vel.x, k.pa.x, k.pb.x, k.pc.x, z.x, 1.0f);
    kf_update1(k.pos.y, k.vel.y, k.pa.y, k.pb.y, k.pc.y, z.y, 1.0f);
    kf_update1(k.pos.z, k.vel.z, k.pa.z, k.pb.z, k.pc.z, z.z, 10.0f);
    kf_update1(k.pos.w, k.vel.w, k.pa.w, k.pb.w, k.pc.w, z.w, 10.0f);
}
__device__ __forceinline__ Kf oc_initiate(const float4 z) {
    Kf k;
    k.pos = z; k.vel = float4{0.f, 0.f, 0.f, 0.f};
    k.pa = float4{10.f, 10.f, 10.f, 10.f};
    k.pb = float4{0.f, 0.f, 0.f, 0.f};
    k.pc = float4{1e4f, 1e4f, 1e4f, 0.f};
    return k;
}
__device__ __forceinline__ float4 oc_box_to_z(const float4 b) {
    const float w = b.z - b.x, h = b.w - b.y;
    return float4{b.x + w * 0.5f, b.y + h * 0.5f, w * h, w / (h + 1e-6f)};
}
__device__ __forceinline__ float4 oc_state_to_box(const float4 m) {
    const float w = __builtin_sqrtf(m.z * m.w);
    const float h = m.z / w;
    const float hw = w * 0.5f, hh = h * 0.5f;
    return float4{m.x - hw, m.y - hh, m.x + hw, m.y + hh};
}
__device__ __forceinline__ float2 oc_centre(const float4 b) { return float2{(b.x + b.z) * 0.5f, (b.y + b.w) * 0.5f}; }
// unit direction (dy, dx) from centre a to centre b
__device__ __forceinline__ float2 oc_direction(const float2 a, const float2 b) {
    const float dx = b.x - a.x, dy = b.y - a.y;
    const float norm = __builtin_sqrtf(dx * dx + dy * dy) + 1e-6f;
    return float2{dy / norm, dx / norm};
}

constexpr int OC_ALIVE = 1, OC_HAS_OBS = 2;

__global__ __launch_bounds__(TRK_THREADS) void ocsort_update(OcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // every LDS byte is dynamic: the base stays 16-byte aligned
    const int s = blockIdx.x, tid = threadIdx.x;
    const int Mc = a.max_tracks, Nc = a.max_dets;
    float4 *tbox = (float4 *)smem;       // predicted boxes
    float4 *tlast = tbox + Mc;           // last observations
    float4 *dbox = tlast + Mc;           // this frame's detections, input order
    float2 *tref = (float2 *)(dbox + Nc);    // centre of the reference observation
    float2 *tdir = tref + Mc;            // stored direction (dy, dx)
    float *dconf = (float *)(tdir + Mc);
    int *d_used = (int *)(dconf + Nc);   // detection -> matched
    int *cols = d_used + Nc;
    int *col_winner = cols + Nc;
    int *rows = col_winner + Nc;
    int *row_best = rows + Mc;
    int *rowcand = row_best + Mc;
    int *t_match = rowcand + Mc;         // track -> detection, -1 unmatched
    int *t_flag = t_match + Mc;          // OC_ALIVE | OC_HAS_OBS
    int *t_tsu = t_flag + Mc;
    int *t_new = t_tsu + Mc;             // track -> position in the next list, -1 deleted
    int *wsum = t_new + Mc;              // [TRK_WAVES + 1]
    int *shared = wsum + TRK_WAVES + 1;  // [0] assignment error, [1] returned tracks
    unsigned char *lap_base = (unsigned char *)(((uintptr_t)(shared + 2) + 7) & ~(uintptr_t)7);
    const LapSmemT<double> L = lap_carve_t<double>(lap_base, Nc);
    if (tid == 0) { shared[0] = 0; shared[1] = 0; }
    __syncthreads();

    OcState st = a.states[s];
    long long *meta = (long long *)a.meta + (size_t)s * 8;
    const int cur = (int)meta[0] & 1;
    const int M = min(max((int)meta[1], 0), Mc);
    const long long next_id = meta[4], frame_count = meta[5] + 1;
#define OC_SEL(f) auto *c_##f = cur ? st.f[1] : st.f[0]; auto *n_##f = cur ? st.f[0] : st.f[1]
    OC_SEL(ids); OC_SEL(obox); OC_SEL(conf); OC_SEL(cls); OC_SEL(hits); OC_SEL(streak); OC_SEL(age); OC_SEL(tsu); OC_SEL(dir); OC_SEL(kf);
    OC_SEL(saved); OC_SEL(ring); OC_SEL(ring_age);
#undef OC_SEL
    int n = a.det_n[s];
    n = min(max(n, 0), min(Nc, a.det_stride));
    const float4 *gb = a.det_box + (size_t)s * a.det_stride;
    const float *gc = a.det_conf + (size_t)s * a.det_stride;
    const int32_t *gk = a.det_cls + (size_t)s * a.det_stride;
    const float det_thresh = a.det_thresh, low_thresh = a.low_thresh, iou_thr = a.iou_thr;
    const int delta_t = min(max(a.delta_t, 1), OC_RING);

    // ---- predict ----
    for (int i = tid; i < M; i += TRK_THREADS) {
        Kf k = kf_load(c_kf, Mc, i);
        if (k.pos.z + k.vel.z <= 0.0f) k.vel.z = 0.0f;
        oc_predict(k);
        kf_store(c_kf, Mc, i, k);
        const int age = c_age[i] + 1;
        c_age[i] = age;
        const int tsu0 = c_tsu[i];
        if (tsu0 > 0) c_streak[i] = 0;
        c_tsu[i] = tsu0 + 1;
        t_tsu[i] = tsu0 + 1;
        const float4 pb = oc_state_to_box(k.pos);
        tbox[i] = pb;
        const float4 last = c_obox[i];
        tlast[i] = last;
        float4 ref = last;
        for (int dt = delta_t; dt >= 1; --dt) {
            const int want = age - dt;
            if (want < 0) continue;
            const int slot = want & (OC_RING - 1);
            if (c_ring_age[slot * Mc + i] == want) { ref = c_ring[slot * Mc + i]; break; }
        }
        tref[i] = oc_centre(ref);
        tdir[i] = c_dir[i];
        const bool alive = finite_bits(pb.x) && finite_bits(pb.y) && finite_bits(pb.z) && finite_bits(pb.w);
        t_flag[i] = (alive ? OC_ALIVE : 0) | (c_hits[i] > 0 ? OC_HAS_OBS : 0);
        t_match[i] = -1;
    }
    for (int j = tid; j < n; j += TRK_THREADS) {
        dbox[j] = gb[j];
        dconf[j] = gc[j];
        d_used[j] = 0;
    }
    __syncthreads();
    auto is_high = [&](int j) { return dconf[j] > det_thresh; };
    auto is_low = [&](int j) { const float c = dconf[j]; return c > low_thresh && c < det_thresh; };
    auto take = [&](int nr) {                              // the matched pairs of the stage just solved
        for (int r = tid; r < nr; r += TRK_THREADS) {
            const int c = row_best[r];
            if (c >= 0 && col_winner[c] == r) { t_match[rows[r]] = cols[c]; d_used[cols[c]] = 1; }
        }
        __syncthreads();
    };

    // ---- OCM: high detections against the predicted boxes, IoU + direction consistency ----
    {
        const double inertia = a.inertia;
        auto edge = [&](int r, int c, double &cost) -> bool {
            const int i = rows[r], j = cols[c];
            const float4 d = dbox[j];
            const float v = iou_ref(tbox[i], d);
            if (!(v >= iou_thr)) return false;
            double g = (double)v;
            if (t_flag[i] & OC_HAS_OBS) {
                const float2 u = oc_direction(tref[i], oc_centre(d)), w = tdir[i];
                float cs = w.y * u.y + w.x * u.x;
                cs = fminf(fmaxf(cs, -1.0f), 1.0f);
                g = g + ((ACOS_HALF_PI - acos_fixed(cs)) / ACOS_PI) * inertia * (double)dconf[j];
            }
            if (!(g > 0.0)) return false;
            cost = -g;
            return true;
        };
        const int nr = block_compact([&](int i) { return (t_flag[i] & OC_ALIVE) != 0; }, M, rows, wsum);
        const int nc = nr ? block_compact(is_high, n, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge, nr, nc, row_best, col_winner, rowcand, L, wsum, &shared[0]);
            take(nr);
        }
    }
    // ---- BYTE: low detections against the predicted boxes of the unmatched tracks ----
    auto edge_pred = [&](int r, int c, double &cost) -> bool {
        const float v = iou_ref(tbox[rows[r]], dbox[cols[c]]);
        if (!(v >= iou_thr)) return false;
        cost = -(double)v;
        return true;
    };
    if (a.use_byte) {
        const int nr = block_compact([&](int i) { return (t_flag[i] & OC_ALIVE) && t_match[i] < 0; }, M, rows, wsum);
        const int nc = nr ? block_compact(is_low, n, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge_pred, nr, nc, row_best, col_winner, rowcand, L, wsum, &shared[0]);
            take(nr);
        }
    }
    // ---- OCR: unmatched high detections against the last observations of the unmatched tracks ----
    {
        auto edge_last = [&](int r, int c, double &cost) -> bool {
            const float v = iou_ref(tlast[rows[r]], dbox[cols[c]]);
            if (!(v >= iou_thr)) return false;
            cost = -(double)v;
            return true;
        };
        const int nr = block_compact([&](int i) { return t_flag[i] == (OC_ALIVE | OC_HAS_OBS) && t_match[i] < 0; }, M, rows, wsum);
        const int nc = nr ? block_compact([&](int j) { return is_high(j) && !d_used[j]; }, n, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge_last, nr, nc, row_best, col_winner, rowcand, L, wsum, &shared[0]);
            take(nr);
        }
    }

    // ---- update, deaths, compaction into the other buffer ----
    const int kept = block_compact([&](int i) { return (t_flag[i] & OC_ALIVE) && (t_match[i] >= 0 || t_tsu[i] <= a.max_age); }, M, rows, wsum);
    for (int i = tid; i < M; i += TRK_THREADS) t_new[i] = -1;
    __syncthreads();
    for (int o = tid; o < kept; o += TRK_THREADS) t_new[rows[o]] = o;
    __syncthreads();
    for (int i = tid; i < M; i += TRK_THREADS) {
        const int o = t_new[i];
        if (o < 0) continue;
        const int j = t_match[i];
        Kf k = kf_load(c_kf, Mc, i);
        Kf sv = kf_load(c_saved, Mc, i);
        int hits = c_hits[i], streak = c_streak[i], tsu = t_tsu[i];
        const int age = c_age[i];
        float4 ob = tlast[i];
        float cf = c_conf[i];
        int cl = c_cls[i];
        float2 dir = tdir[i];
#pragma unroll
        for (int q = 0; q < OC_RING; ++q) { n_ring[q * Mc + o] = c_ring[q * Mc + i]; n_ring_age[q * Mc + o] = c_ring_age[q * Mc + i]; }
        if (j >= 0) {
            const float4 z = dbox[j];
            if (t_flag[i] & OC_HAS_OBS) {
                dir = oc_direction(tref[i], oc_centre(z));
                if (tsu >= 2) {                            // ORU: walk the virtual observations from the state saved at the first miss
                    k = sv;
                    const float w1 = ob.z - ob.x, h1 = ob.w - ob.y;
                    const float x1 = ob.x + w1 * 0.5f, y1 = ob.y + h1 * 0.5f;
                    const float w2 = z.z - z.x, h2 = z.w - z.y;
                    const float x2 = z.x + w2 * 0.5f, y2 = z.y + h2 * 0.5f;
                    const float g = (float)tsu;
                    const float dx = (x2 - x1) / g, dy = (y2 - y1) / g, dw = (w2 - w1) / g, dh = (h2 - h1) / g;
                    for (int q = 1; q <= tsu; ++q) {
                        const float fq = (float)q;
                        const float x = x1 + fq * dx, y = y1 + fq * dy, w = w1 + fq * dw, h = h1 + fq * dh;
                        oc_update(k, float4{x, y, w * h, w / h});
                        if (q < tsu) oc_predict(k);
                    }
                }
            }
            oc_update(k, oc_box_to_z(z));
            ob = z; cf = dconf[j]; cl = gk[j];
            const int slot = age & (OC_RING - 1);
            n_ring[slot * Mc + o] = z;
            n_ring_age[slot * Mc + o] = age;
            tsu = 0;
            hits += 1;
            streak += 1;
        } else if (tsu == 1) {
            sv = k;
        }
        if (tsu == 0 && (streak >= a.min_hits || frame_count <= (long long)a.min_hits)) atomicAdd(&shared[1], 1);
        n_ids[o] = c_ids[i]; n_obox[o] = ob; n_conf[o] = cf; n_cls[o] = cl; n_hits[o] = hits; n_streak[o] = streak; n_age[o] = age; n_tsu[o] = tsu;
        n_dir[o] = dir;
        kf_store(n_kf, Mc, o, k);
        kf_store(n_saved, Mc, o, sv);
    }
    // ---- births, detection order ----
    int nsp = block_compact([&](int j) { return is_high(j) && !d_used[j]; }, n, cols, wsum);
    int err = 0;
    if (kept + nsp > Mc) { err = 1; nsp = Mc - kept; }
    for (int q = tid; q < nsp; q += TRK_THREADS) {
        const int j = cols[q], o = kept + q;
        const float4 z = dbox[j];
        n_ids[o] = next_id + q; n_obox[o] = z; n_conf[o] = dconf[j]; n_cls[o] = gk[j];
        n_hits[o] = 0; n_streak[o] = 0; n_age[o] = 0; n_tsu[o] = 0;
        n_dir[o] = float2{0.f, 0.f};
        const Kf k = oc_initiate(oc_box_to_z(z));
        kf_store(n_kf, Mc, o, k);
        kf_store(n_saved, Mc, o, k);
#pragma unroll
        for (int r = 0; r < OC_RING; ++r) { n_ring[r * Mc + o] = float4{0.f, 0.f, 0.f, 0.f}; n_ring_age[r * Mc + o] = -1; }
        if (0 >= a.min_hits || frame_count <= (long long)a.min_hits) atomicAdd(&shared[1], 1);
    }
    __syncthreads();
    if (tid == 0) {
        meta[0] = cur ^ 1;
        meta[1] = kept + nsp;
        if (err) meta[2] = 1;
        else if (shared[0]) meta[2] = shared[0];
        meta[3] = shared[1];
        meta[4] = next_id + nsp;
        meta[5] = frame_count;
    }
}

static size_t oc_smem_bytes(int Mc, int Nc) {
    return (size_t)Mc * (16 * 2 + 8 * 2 + 4 * 7) + (size_t)Nc * (16 + 4 + 4 * 3) + (TRK_WAVES + 1 + 2) * 4 + 16 + lap_smem_bytes(Nc);
}

static int launch_ocsort_update(const OcArgs &a, int n_streams, hipStream_t s) {
    const size_t smem = oc_smem_bytes(a.max_tracks, a.max_dets);
    RT_CHECK(smem <= 150 * 1024, RTMODT_E_INVALID, "ocsort: max_tracks %d / max_dets %d need %zu B of LDS", a.max_tracks, a.max_dets, smem);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)ocsort_update, smem, seen));
    hipLaunchKernelGGL(ocsort_update, dim3(n_streams), dim3(TRK_THREADS), smem, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

}  // namespace rtmodt

using namespace rtmodt;

struct rtmodt_ocsort : TrackHandleBase {
    EventTimer<2> timer;
    rtmodt_ocsort_cfg cfg = {};
    char *pool = nullptr;                    // all state arrays (track_layout.h: carve_ocsort)
    OcState *d_states = nullptr; std::vector<OcState> h_states;
};

namespace rtmodt {
int ocsort_device_view(rtmodt_ocsort *t, OcDeviceView *out) {
    RT_CHECK(t && out, RTMODT_E_INVALID, "null argument");
    out->states = t->d_states; out->min_hits = t->cfg.min_hits;
    return track_view(t, out);
}
}  // namespace rtmodt

static int oc_create_impl(rtmodt_ocsort *t) {
    RT_TRY(track_open(t));
    RT_TRY(t->timer.create());
    t->h_states.assign(t->S, OcState{});
    const size_t total = carve_ocsort(t->h_states.data(), t->S, t->Mc, OC_RING, nullptr);
    RT_HIP(hipMalloc((void **)&t->pool, total));
    RT_HIP(handle_zero(t->pool, total, t->stream));
    carve_ocsort(t->h_states.data(), t->S, t->Mc, OC_RING, t->pool);
    RT_HIP(hipMalloc((void **)&t->d_states, sizeof(OcState) * t->S));
    RT_HIP(hipMemcpy(t->d_states, t->h_states.data(), sizeof(OcState) * t->S, hipMemcpyHostToDevice));
    return RTMODT_OK;
}

static OcArgs oc_args(rtmodt_ocsort *t) {
    OcArgs a{};
    a.max_tracks = t->Mc; a.max_dets = t->Nc;
    a.det_thresh = t->cfg.det_thresh; a.low_thresh = t->cfg.low_thresh; a.iou_thr = t->cfg.iou_threshold; a.inertia = t->cfg.inertia;
    a.max_age = t->cfg.max_age; a.min_hits = t->cfg.min_hits; a.delta_t = t->cfg.delta_t; a.use_byte = t->cfg.use_byte ? 1 : 0;
    a.states = t->d_states; a.meta = t->d_meta;
    a.det_box = t->d_box; a.det_conf = t->d_conf; a.det_cls = t->d_cls; a.det_n = t->d_n; a.det_stride = t->Nc;
    return a;
}

static int oc_run(rtmodt_ocsort *t, const OcArgs &a, int count, hipStream_t q) {
    RT_TRY(t->timer.record(0, q));
    RT_TRY(launch_ocsort_update(a, count, q));
    RT_TRY(t->timer.record(1, q));
    t->timer.timed = true;
    return RTMODT_OK;
}

static int oc_check_sticky(rtmodt_ocsort *t, int s, int64_t err) { return track_check_sticky(t, s, err, "assignment"); }

extern "C" {

void rtmodt_ocsort_destroy(rtmodt_ocsort *t) {
    if (!t) return;
    track_close(t, [t] {
        t->timer.destroy();
        hipFree(t->pool); hipFree(t->d_states);
    });
    delete t;
}

int rtmodt_ocsort_create(const rtmodt_ocsort_cfg *cfg, rtmodt_ocsort **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    const auto fin = [](double v) { return v == v && v - v == 0.0; };
    RT_CHECK(fin(cfg->det_thresh) && fin(cfg->low_thresh) && fin(cfg->iou_threshold) && fin(cfg->inertia) && cfg->inertia >= 0 && cfg->max_age >= 1 &&
                 cfg->max_age <= 100000 && cfg->min_hits >= 0 && cfg->delta_t >= 1, RTMODT_E_INVALID,
             "bad parameter (det_thresh %g, low_thresh %g, iou_threshold %g, inertia %g, max_age %d, min_hits %d, delta_t %d)", (double)cfg->det_thresh,
             (double)cfg->low_thresh, (double)cfg->iou_threshold, cfg->inertia, cfg->max_age, cfg->min_hits, cfg->delta_t);
    // our rule: angle >= -inertia / 2 for conf <= 1, so iou >= iou_threshold > inertia / 2 makes every admissible gain positive
    RT_CHECK((double)cfg->iou_threshold > cfg->inertia / 2, RTMODT_E_INVALID, "iou_threshold %g must exceed inertia / 2 = %g: an admissible pair's gain must be positive",
             (double)cfg->iou_threshold, cfg->inertia / 2);
    RT_CHECK(cfg->max_tracks >= 1 && cfg->max_dets >= 1 && cfg->n_streams >= 1, RTMODT_E_INVALID, "max_tracks %d / max_dets %d / n_streams %d must be positive",
             cfg->max_tracks, cfg->max_dets, cfg->n_streams);
    RT_CHECK(cfg->max_tracks <= OC_MAX_TRACKS && cfg->max_dets <= OC_MAX_DETS && cfg->n_streams <= OC_MAX_STREAMS && cfg->delta_t <= OC_RING, RTMODT_E_CAPACITY,
             "max_tracks %d / max_dets %d / n_streams %d / delta_t %d: at most %d / %d / %d / %d", cfg->max_tracks, cfg->max_dets, cfg->n_streams, cfg->delta_t,
             OC_MAX_TRACKS, OC_MAX_DETS, OC_MAX_STREAMS, OC_RING);
    rtmodt_ocsort *t = new rtmodt_ocsort();
    t->cfg = *cfg;
    t->device = cfg->device; t->S = cfg->n_streams; t->Mc = cfg->max_tracks; t->Nc = cfg->max_dets;
    return handle_created(oc_create_impl(t), t, rtmodt_ocsort_destroy, out);
}

int rtmodt_ocsort_reset(rtmodt_ocsort *t, int stream) { return track_reset_meta(t, stream); }

int rtmodt_ocsort_update_batch(rtmodt_ocsort *t, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n, int32_t *n_returned_out) {
    bool any = false;
    RT_TRY(track_batch_check(t, xyxy, conf, cls, n, &any));
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    hipStream_t q = t->stream;
    RT_TRY(track_batch_stage(t, xyxy, conf, cls, n, any));
    RT_TRY(oc_run(t, oc_args(t), t->S, q));
    RT_HIP(hipMemcpyAsync(t->h_meta, t->d_meta, sizeof(int64_t) * 8 * t->S, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    for (int s = 0; s < t->S; ++s)
        if (n_returned_out) n_returned_out[s] = (int32_t)t->h_meta[8 * s + 3];
    for (int s = 0; s < t->S; ++s) RT_TRY(oc_check_sticky(t, s, t->h_meta[8 * s + 2]));
    return RTMODT_OK;
}

int rtmodt_ocsort_update_from_detector(rtmodt_ocsort *t, rtmodt_detector *det) {
    RT_CHECK(t && det, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(track_detector_outputs(t, det, &o));
    RT_TRY(track_detector_fits(t, o, o.count));
    OcArgs a = oc_args(t);
    a.det_box = o.box; a.det_conf = o.conf; a.det_cls = o.cls; a.det_n = o.n; a.det_stride = o.stride;
    RT_TRY(oc_run(t, a, o.count, o.stream));
    return track_detector_done(t, o.stream);
}

int rtmodt_ocsort_state(rtmodt_ocsort *t, int stream, int64_t *ids, int32_t *hits, int32_t *hit_streak, int32_t *age, int32_t *tsu, float *xyxy,
                        float *conf, int32_t *cls, float *mean, float *cov, float *direction, int32_t *n, int64_t *next_id, int64_t *frame_count) {
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
    const OcState &st = t->h_states[stream];
    const size_t c = (size_t)cnt;
    if (cnt) {
        if (ids) RT_HIP(hipMemcpy(ids, st.ids[cur], c * 8, hipMemcpyDeviceToHost));
        if (hits) RT_HIP(hipMemcpy(hits, st.hits[cur], c * 4, hipMemcpyDeviceToHost));
        if (hit_streak) RT_HIP(hipMemcpy(hit_streak, st.streak[cur], c * 4, hipMemcpyDeviceToHost));
        if (age) RT_HIP(hipMemcpy(age, st.age[cur], c * 4, hipMemcpyDeviceToHost));
        if (tsu) RT_HIP(hipMemcpy(tsu, st.tsu[cur], c * 4, hipMemcpyDeviceToHost));
        if (xyxy) RT_HIP(hipMemcpy(xyxy, st.obox[cur], c * 16, hipMemcpyDeviceToHost));
        if (conf) RT_HIP(hipMemcpy(conf, st.conf[cur], c * 4, hipMemcpyDeviceToHost));
        if (cls) RT_HIP(hipMemcpy(cls, st.cls[cur], c * 4, hipMemcpyDeviceToHost));
        if (direction) RT_HIP(hipMemcpy(direction, st.dir[cur], c * 8, hipMemcpyDeviceToHost));
        if (mean || cov) {
            std::vector<float4> buf((size_t)5 * t->Mc);
            RT_HIP(hipMemcpy(buf.data(), st.kf[cur], buf.size() * sizeof(float4), hipMemcpyDeviceToHost));
            kalman_unpack(&buf[0].x, t->Mc, cnt, mean, cov);
        }
    }
    return oc_check_sticky(t, stream, m[2]);               // after the copies: a stream in error stays readable
}

int rtmodt_ocsort_last_ms(rtmodt_ocsort *t, float *update_ms) {
    RT_CHECK(t, RTMODT_E_INVALID, "null argument");
    float a = 0;
    RT_TRY(t->timer.elapsed(t->device, 0, 1, &a, "no update has run yet"));
    if (update_ms) *update_ms = a;
    return RTMODT_OK;
}

}  // extern "C"
