// deepsort.hip -- the DeepSORT tracker the reference's config offers (config/default.yaml: `tracking.algorithm: "deepsort"` and
// its `deepsort:` block) but never wired (src/tracking/tracker.py:212-214 raises).  The algorithm is the published one (Wojke et
// al.; deep_sort's tracker.py, linear_assignment.py, nn_matching.py, kalman_filter.py), restated in tests/deepsort_ref.py.
// PARITY UNPINNED: deep_sort_realtime is installed nowhere this runs.
//
// One call = a fixed number of launches for all streams, no host hop between them:
//   appearance_hist + appearance_quant (appearance.hip)   descriptors of the frame's boxes, unless the caller brings them
//   appearance_dotmax                  (appearance.hip)   gallery x descriptors on the int8 matrix cores
//   deepsort_update                    (here)             one 1024-thread workgroup per stream: predict, confidence filter,
//                                                         gating, matching cascade, IoU stage, life cycle, compaction
// Per frame and stream (deep_sort tracker.py: predict + update):
//   predict   every track: Kalman predict (the height velocity is never zeroed), age += 1, time_since_update += 1
//   filter    detections with conf >= min_confidence (float32), input order kept
//   gating    d2 = sum_k y_k^2 / (a_k + r_k) against the projected state (diagonal S: the covariance is block-diagonal), float32,
//             one rounding per operation, k = 0..3 in order; d2 > 9.4877f is inadmissible
//   cascade   confirmed tracks, level = time_since_update 1..max_age: maximum-gain matching over the admissible pairs with the
//             integer gain thr + 1 - c, c = max(0, 16129 - dotmax), admissible when c <= thr = floor(max_dist * 16129)
//   IoU       tentative tracks + unmatched confirmed tracks with time_since_update == 1 against the remaining detections on
//             the predicted boxes: cost = 1 - iou (float32), admissible when cost <= max_iou_distance, gain
//             (max_iou_distance + 1e-5) - cost in double
//   life      matched: Kalman update, descriptor appended to the track's ring, hits += 1, time_since_update = 0, confirmed at
//             hits >= n_init; unmatched tentative: deleted; unmatched confirmed: deleted when time_since_update > max_age;
//             unmatched detection: a tentative track, ids from 1 in detection order; list order = creation order
// Both matchings use assoc_sparse (track_dev.h: the isolated-pair shortcut in front of lap.h's sparse exact solver); its
// contested-pair limits (256 rows / 256 columns / 2048 pairs) raise the sticky error 2.
#include <vector>

#include "track_host.h"
#include "frame_stage.h"
#include "lap.h"

#include <climits>
#include <cmath>

namespace rtmodt {

#include "track_dev.h"

struct DsArgs {
    int max_tracks, max_dets, budget, dim;
    float min_conf; long long thr; double max_iou; int max_age, n_init;
    DsState *states; int64_t *meta;          // meta[stream][8] = {cur, n_tracks, err, n_returned, next_id, 0, 0, 0}
    const float4 *det_box; const float *det_conf; const int32_t *det_cls; const int32_t *det_n; int det_stride;
    const int8_t *desc; int desc_stride;     // [stream][desc_stride][dim]
    const int32_t *dotmax;                   // [stream][max_tracks][max_dets], columns = raw detection index
    int8_t *gallery; size_t gallery_stream_stride;
};

constexpr float DS_GATE = 9.4877f;           // chi-square 0.95 quantile, 4 degrees of freedom (deep_sort kalman_filter.chi2inv95[4])
constexpr long long DS_DOT_ONE = 16129;      // 127 * 127

__global__ __launch_bounds__(TRK_THREADS) void deepsort_update(DsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int Mc = a.max_tracks, Nc = a.max_dets, D = a.dim;
    float4 *tbox = (float4 *)smem;       // predicted boxes
    float4 *tmean = tbox + Mc;           // predicted (cx, cy, a, h)
    float4 *tS = tmean + Mc;             // projected variances a_k + r_k
    float4 *dbox = tS + Mc;              // filtered detections
    float4 *dxyah = dbox + Nc;
    int *draw = (int *)(dxyah + Nc);     // filtered -> raw index
    int *d_match = draw + Nc;            // filtered detection -> track, -1 free
    int *cols = d_match + Nc;
    int *col_winner = cols + Nc;
    int *rows = col_winner + Nc;
    int *row_best = rows + Mc;
    int *rowcand = row_best + Mc;
    int *t_match = rowcand + Mc;         // track -> filtered detection, -1 unmatched
    int *t_flag = t_match + Mc;
    int *t_tsu = t_flag + Mc;
    int *t_new = t_tsu + Mc;             // track -> position in the next list, -1 deleted
    int *wsum = t_new + Mc;
    unsigned char *lap_base = (unsigned char *)(((uintptr_t)(wsum + TRK_WAVES + 1) + 7) & ~(uintptr_t)7);
    const LapSmemT<long long> Li = lap_carve_t<long long>(lap_base, Nc);
    const LapSmemT<double> Ld = lap_carve_t<double>(lap_base, Nc);
    __shared__ int lap_err, s_maxlv, s_ret;
    if (tid == 0) { lap_err = 0; s_maxlv = 0; s_ret = 0; }
    __syncthreads();

    DsState st = a.states[s];
    long long *meta = (long long *)a.meta + (size_t)s * 8;
    const int cur = (int)meta[0];
    const int M = min((int)meta[1], Mc);
    const long long next_id = meta[4];
#define DS_SEL(f) auto *c_##f = cur ? st.f[1] : st.f[0]; auto *n_##f = cur ? st.f[0] : st.f[1]
    DS_SEL(ids); DS_SEL(dbox); DS_SEL(conf); DS_SEL(cls); DS_SEL(flag); DS_SEL(hits); DS_SEL(age); DS_SEL(tsu); DS_SEL(slot); DS_SEL(gcount); DS_SEL(kf);
#undef DS_SEL
    int n = a.det_n[s];
    n = min(max(n, 0), min(Nc, a.det_stride));
    const float4 *gb = a.det_box + (size_t)s * a.det_stride;
    const float *gc = a.det_conf + (size_t)s * a.det_stride;
    const int32_t *gk = a.det_cls + (size_t)s * a.det_stride;
    int8_t *gal = a.gallery + (size_t)s * a.gallery_stream_stride;
    const int8_t *desc = a.desc + (size_t)s * a.desc_stride * D;
    const int32_t *dm = a.dotmax + (size_t)s * Mc * Nc;

    // ---- predict ----
    for (int i = tid; i < M; i += TRK_THREADS) {
        Kf k = kf_load(c_kf, Mc, i);
        kf_predict(k);
        kf_store(c_kf, Mc, i, k);
        tmean[i] = k.pos;
        tbox[i] = xyah_to_xyxy(k.pos);
        const float sp = KF_WP * k.pos.w;
        const float r = sp * sp;
        tS[i] = float4{k.pa.x + r, k.pa.y + r, k.pa.z + 1e-1f * 1e-1f, k.pa.w + r};
        c_age[i] += 1;
        const int tsu = c_tsu[i] + 1;
        c_tsu[i] = tsu;
        t_tsu[i] = tsu;
        const int fl = c_flag[i];
        t_flag[i] = fl;
        t_match[i] = -1;
        if (fl == 2) atomicMax(&s_maxlv, tsu);
    }
    // ---- confidence filter, input order kept ----
    const float min_conf = a.min_conf;
    const int nd = block_compact([&](int i) { return gc[i] >= min_conf; }, n, draw, wsum);
    for (int j = tid; j < nd; j += TRK_THREADS) {
        const float4 b = gb[draw[j]];
        dbox[j] = b;
        dxyah[j] = xyxy_to_xyah(b);
        d_match[j] = -1;
    }
    __syncthreads();

    // ---- matching cascade over the confirmed tracks ----
    const long long thr = a.thr;
    auto edge_app = [&](int r, int c, long long &cost) -> bool {
        const int i = rows[r], j = cols[c];
        const float4 z = dxyah[j], m = tmean[i], S = tS[i];
        const float y0 = z.x - m.x, y1 = z.y - m.y, y2 = z.z - m.z, y3 = z.w - m.w;
        float d2 = (y0 * y0) / S.x;
        d2 = d2 + (y1 * y1) / S.y;
        d2 = d2 + (y2 * y2) / S.z;
        d2 = d2 + (y3 * y3) / S.w;
        if (d2 > DS_GATE) return false;
        long long cc = DS_DOT_ONE - (long long)dm[(size_t)i * Nc + draw[j]];
        if (cc < 0) cc = 0;
        if (cc > thr) return false;
        cost = cc - (thr + 1);
        return true;
    };
    const int maxlv = min(a.max_age, s_maxlv);
    for (int lv = 1; lv <= maxlv; ++lv) {
        const int nr = block_compact([&](int i) { return t_flag[i] == 2 && t_tsu[i] == lv; }, M, rows, wsum);
        if (nr == 0) continue;
        const int nc = block_compact([&](int j) { return d_match[j] < 0; }, nd, cols, wsum);
        if (nc == 0) break;
        assoc_sparse<long long>(edge_app, nr, nc, row_best, col_winner, rowcand, Li, wsum, &lap_err);
        for (int r = tid; r < nr; r += TRK_THREADS) {
            const int c = row_best[r];
            if (c >= 0 && col_winner[c] == r) { t_match[rows[r]] = cols[c]; d_match[cols[c]] = rows[r]; }
        }
        __syncthreads();
    }

    // ---- IoU stage: tentative tracks + unmatched confirmed tracks seen in the previous frame ----
    {
        const double max_iou = a.max_iou, limit = a.max_iou + 1e-5;
        auto edge_iou = [&](int r, int c, double &cost) -> bool {
            const float v = iou_ref(tbox[rows[r]], dbox[cols[c]]);
            const double cd = (double)(1.0f - v);
            if (!(cd <= max_iou)) return false;
            cost = cd - limit;
            return true;
        };
        const int nr = block_compact([&](int i) { return t_match[i] < 0 && (t_flag[i] == 1 || t_tsu[i] == 1); }, M, rows, wsum);
        const int nc = nr ? block_compact([&](int j) { return d_match[j] < 0; }, nd, cols, wsum) : 0;
        if (nr > 0 && nc > 0) {
            assoc_sparse<double>(edge_iou, nr, nc, row_best, col_winner, rowcand, Ld, wsum, &lap_err);
            for (int r = tid; r < nr; r += TRK_THREADS) {
                const int c = row_best[r];
                if (c >= 0 && col_winner[c] == r) { t_match[rows[r]] = cols[c]; d_match[cols[c]] = rows[r]; }
            }
            __syncthreads();
        }
    }

    // ---- life cycle ----
    const int D16 = D / 16;
    for (int idx = tid; idx < M * D16; idx += TRK_THREADS) {              // matched: append the descriptor to the ring
        const int i = idx / D16, part = idx - i * D16;
        const int j = t_match[i];
        if (j >= 0) {
            const int pos = c_gcount[i] % a.budget;
            const int4 v = *(const int4 *)(desc + (size_t)draw[j] * D + part * 16);
            *(int4 *)(gal + ((size_t)c_slot[i] * a.budget + pos) * D + part * 16) = v;
        }
    }
    __syncthreads();
    const int kept = block_compact([&](int i) { return t_match[i] >= 0 || (t_flag[i] == 2 && t_tsu[i] <= a.max_age); }, M, rows, wsum);
    for (int i = tid; i < M; i += TRK_THREADS) t_new[i] = -1;
    __syncthreads();
    for (int o = tid; o < kept; o += TRK_THREADS) t_new[rows[o]] = o;
    __syncthreads();
    for (int i = tid; i < M; i += TRK_THREADS) {
        const int o = t_new[i];
        if (o < 0) { st.slot_used[c_slot[i]] = 0; continue; }
        const int j = t_match[i];
        Kf k = kf_load(c_kf, Mc, i);
        int fl = t_flag[i], hits = c_hits[i], tsu = t_tsu[i], gcnt = c_gcount[i];
        float4 db = c_dbox[i];
        float cf = c_conf[i];
        int cl = c_cls[i];
        if (j >= 0) {
            kf_update(k, dxyah[j]);
            hits += 1;
            tsu = 0;
            if (fl == 1 && hits >= a.n_init) fl = 2;
            gcnt += 1;
            db = dbox[j]; cf = gc[draw[j]]; cl = gk[draw[j]];
            if (fl == 2) atomicAdd(&s_ret, 1);
        }
        n_ids[o] = c_ids[i]; n_dbox[o] = db; n_conf[o] = cf; n_cls[o] = cl; n_flag[o] = fl; n_hits[o] = hits;
        n_age[o] = c_age[i]; n_tsu[o] = tsu; n_slot[o] = c_slot[i]; n_gcount[o] = gcnt;
        kf_store(n_kf, Mc, o, k);
    }
    __syncthreads();                                       // slot_used is final for the old tracks
    // ---- new tentative tracks, detection order ----
    int nsp = block_compact([&](int j) { return d_match[j] < 0; }, nd, cols, wsum);
    int err = 0;
    if (kept + nsp > Mc) { err = 1; nsp = Mc - kept; }
    const int nfree = block_compact([&](int q) { return st.slot_used[q] == 0; }, Mc, rows, wsum);
    if (nsp > nfree) { err = 1; nsp = nfree; }             // (cannot happen: free slots = Mc - kept)
    for (int k = tid; k < nsp; k += TRK_THREADS) {
        const int j = cols[k], o = kept + k, q = rows[k];
        st.slot_used[q] = 1;
        n_ids[o] = next_id + k; n_dbox[o] = dbox[j]; n_conf[o] = gc[draw[j]]; n_cls[o] = gk[draw[j]];
        n_flag[o] = 1; n_hits[o] = 1; n_age[o] = 1; n_tsu[o] = 0; n_slot[o] = q; n_gcount[o] = 1;
        kf_store(n_kf, Mc, o, kf_initiate(dxyah[j]));
    }
    for (int idx = tid; idx < nsp * D16; idx += TRK_THREADS) {
        const int k = idx / D16, part = idx - k * D16;
        const int4 v = *(const int4 *)(desc + (size_t)draw[cols[k]] * D + part * 16);
        *(int4 *)(gal + ((size_t)rows[k] * a.budget) * D + part * 16) = v;
    }
    __syncthreads();
    if (tid == 0) {
        meta[0] = cur ^ 1;
        meta[1] = kept + nsp;
        if (err) meta[2] = 1;
        else if (lap_err) meta[2] = lap_err;
        meta[3] = s_ret;
        meta[4] = next_id + nsp;
    }
}

static size_t ds_smem_bytes(int Mc, int Nc) {
    return (size_t)Mc * 16 * 3 + (size_t)Nc * 16 * 2 + (size_t)Nc * 4 * 4 + (size_t)Mc * 4 * 7 + (TRK_WAVES + 1) * 4 + 16 + lap_smem_bytes(Nc);
}

static int launch_deepsort_update(const DsArgs &a, int n_streams, hipStream_t s) {
    const size_t smem = ds_smem_bytes(a.max_tracks, a.max_dets);
    RT_CHECK(smem <= 150 * 1024, RTMODT_E_INVALID, "deepsort: max_tracks %d / max_dets %d need %zu B of LDS", a.max_tracks, a.max_dets, smem);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)deepsort_update, smem, seen));
    hipLaunchKernelGGL(deepsort_update, dim3(n_streams), dim3(TRK_THREADS), smem, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

}  // namespace rtmodt

using namespace rtmodt;

struct rtmodt_deepsort : TrackHandleBase {
    EventTimer<4> timer;                   // describe | distance | update boundaries of the last call
    bool described = false;
    int budget = 0, dim = APP_DIM;
    float min_conf = 0.3f; double max_dist = 0.2, max_iou = 0.7; long long thr = 0; int max_age = 70, n_init = 3;
    char *pool = nullptr; int8_t *gallery = nullptr;      // pool: all state arrays (track_layout.h: carve_deepsort)
    DsState *d_states = nullptr; std::vector<DsState> h_states;
    int8_t *d_desc = nullptr; int32_t *d_counts = nullptr, *d_dotmax = nullptr;
    FrameStage stage;                        // host frames
    rtmodt_reid *reid = nullptr;             // embedder = a .rtreid file: the network of reid.hip describes the boxes instead of the histogram
};

static size_t ds_gallery_stream_bytes(const rtmodt_deepsort *t) { return (size_t)t->Mc * t->budget * t->dim; }

namespace rtmodt {
int deepsort_device_view(rtmodt_deepsort *t, DsDeviceView *out) {
    RT_CHECK(t && out, RTMODT_E_INVALID, "null argument");
    out->states = t->d_states;
    return track_view(t, out);
}
int deepsort_gallery_view(rtmodt_deepsort *t, const int8_t **gallery, int *dim, int *budget) {
    RT_CHECK(t && gallery && dim && budget, RTMODT_E_INVALID, "null argument");
    *gallery = t->gallery; *dim = t->dim; *budget = t->budget;
    return RTMODT_OK;
}
}  // namespace rtmodt

static int ds_create_impl(rtmodt_deepsort *t) {
    RT_TRY(track_open(t));
    RT_TRY(t->timer.create());
    t->h_states.assign(t->S, DsState{});
    const size_t total = carve_deepsort(t->h_states.data(), t->S, t->Mc, nullptr);
    RT_HIP(hipMalloc((void **)&t->pool, total));
    RT_HIP(handle_zero(t->pool, total, t->stream));
    carve_deepsort(t->h_states.data(), t->S, t->Mc, t->pool);
    RT_HIP(hipMalloc((void **)&t->d_states, sizeof(DsState) * t->S));
    RT_HIP(hipMemcpy(t->d_states, t->h_states.data(), sizeof(DsState) * t->S, hipMemcpyHostToDevice));
    RT_HIP(hipMalloc((void **)&t->gallery, ds_gallery_stream_bytes(t) * t->S));
    RT_HIP(handle_zero(t->gallery, ds_gallery_stream_bytes(t) * t->S, t->stream));
    const size_t SN = (size_t)t->S * t->Nc;
    RT_HIP(hipMalloc((void **)&t->d_desc, SN * t->dim)); RT_HIP(handle_zero(t->d_desc, SN * t->dim, t->stream));
    RT_HIP(hipMalloc((void **)&t->d_counts, SN * APP_DIM * 4));
    RT_HIP(hipMalloc((void **)&t->d_dotmax, (size_t)t->S * t->Mc * t->Nc * 4));
    RT_HIP(handle_zero(t->d_dotmax, (size_t)t->S * t->Mc * t->Nc * 4, t->stream));
    return RTMODT_OK;
}

// the launches of one call on stream q, detections described by `a`'s det_* fields for streams [0, count)
static int ds_run(rtmodt_deepsort *t, DsArgs a, int count, const AppFrames *frames, int fh, int fw, int pitch, hipStream_t q) {
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
    DotmaxArgs m{};
    m.gallery = t->gallery; m.gallery_stream_stride = ds_gallery_stream_bytes(t); m.states = t->d_states; m.meta = t->d_meta;
    m.budget = t->budget; m.dim = t->dim; m.dets = t->d_desc; m.det_stride = t->Nc; m.n_dets_dev = a.det_n; m.max_dets = std::min(a.det_stride, t->Nc);
    m.out = t->d_dotmax; m.out_stream_stride = (size_t)t->Mc * t->Nc; m.out_row_stride = t->Nc;
    RT_TRY(launch_dotmax(m, t->Mc, m.max_dets, count, q));
    RT_TRY(t->timer.record(2, q));
    RT_TRY(launch_deepsort_update(a, count, q));
    RT_TRY(t->timer.record(3, q));
    t->timer.timed = true;
    return RTMODT_OK;
}

static DsArgs ds_args(rtmodt_deepsort *t) {
    DsArgs a{};
    a.max_tracks = t->Mc; a.max_dets = t->Nc; a.budget = t->budget; a.dim = t->dim;
    a.min_conf = t->min_conf; a.thr = t->thr; a.max_iou = t->max_iou; a.max_age = t->max_age; a.n_init = t->n_init;
    a.states = t->d_states; a.meta = t->d_meta;
    a.det_box = t->d_box; a.det_conf = t->d_conf; a.det_cls = t->d_cls; a.det_n = t->d_n; a.det_stride = t->Nc;
    a.desc = t->d_desc; a.desc_stride = t->Nc; a.dotmax = t->d_dotmax;
    a.gallery = t->gallery; a.gallery_stream_stride = ds_gallery_stream_bytes(t);
    return a;
}

static int ds_check_sticky(rtmodt_deepsort *t, int s, int64_t err) { return track_check_sticky(t, s, err, "assignment"); }

// frames of a call -> device pointers (host frames are staged on stream q)
static int ds_stage(rtmodt_deepsort *t, const uint8_t *const *frames, int count, int fh, int fw, int pitch, int mem_kind, hipStream_t q, AppFrames *out) {
    RT_CHECK(t->reid || t->dim == APP_DIM, RTMODT_E_INVALID, "this handle takes caller descriptors of dimension %d; the built-in descriptor has %d", t->dim, APP_DIM);
    RT_TRY(check_frames(frames, count, fh, fw, pitch, mem_kind, kAppFrames));
    RT_TRY(t->stage.in(frames, count, fh, fw, pitch, mem_kind, q, FRAMES_AS_GIVEN));
    for (int i = 0; i < count; ++i) out->p[i] = t->stage.at(frames, i);
    return RTMODT_OK;
}

extern "C" {

void rtmodt_deepsort_destroy(rtmodt_deepsort *t) {
    if (!t) return;
    track_close(t, [t] {
        t->timer.destroy();
        hipFree(t->pool); hipFree(t->gallery); hipFree(t->d_states); hipFree(t->d_desc); hipFree(t->d_counts); hipFree(t->d_dotmax);
        t->stage.release();
        reid_close(t->reid);
    });
    delete t;
}

int rtmodt_deepsort_create(const rtmodt_deepsort_cfg *cfg, rtmodt_deepsort **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    const size_t elen = cfg->embedder ? strlen(cfg->embedder) : 0;
    const bool net = elen > 7 && strcmp(cfg->embedder + elen - 7, ".rtreid") == 0;
    RT_CHECK(net || !cfg->embedder || !*cfg->embedder || strcmp(cfg->embedder, "colorhist") == 0, RTMODT_E_UNSUPPORTED,
             "embedder '%s': only the built-in \"colorhist\" descriptor and an OSNet x0.25 .rtreid file (tools/convert_weights.py --reid) are computed "
             "here; bring embeddings of another model as caller descriptors", cfg->embedder);
    RT_CHECK(!net || cfg->dim == 0 || cfg->dim == 512, RTMODT_E_INVALID, "descriptor dimension %d: the network's is 512 (or 0)", cfg->dim);
    const int dim = net ? 512 : cfg->dim ? cfg->dim : APP_DIM;
    RT_CHECK(dim >= 64 && dim <= 512 && dim % 64 == 0, RTMODT_E_INVALID, "descriptor dimension %d: 64..512 in multiples of 64", dim);
    RT_CHECK(cfg->max_dist == cfg->max_dist && cfg->max_dist >= 0 && cfg->max_dist <= 2 && cfg->max_iou_distance == cfg->max_iou_distance &&
                 cfg->min_confidence == cfg->min_confidence && cfg->max_age >= 1 && cfg->n_init >= 1, RTMODT_E_INVALID,
             "bad parameter (max_dist %g, max_iou_distance %g, min_confidence %g, max_age %d, n_init %d)", cfg->max_dist, cfg->max_iou_distance,
             (double)cfg->min_confidence, cfg->max_age, cfg->n_init);
    RT_CHECK(cfg->max_tracks >= 1 && cfg->max_dets >= 1 && cfg->n_streams >= 1 && cfg->nn_budget >= 1, RTMODT_E_INVALID,
             "max_tracks %d / max_dets %d / n_streams %d / nn_budget %d must be positive", cfg->max_tracks, cfg->max_dets, cfg->n_streams, cfg->nn_budget);
    RT_CHECK(cfg->max_tracks <= DS_MAX_TRACKS && cfg->max_dets <= DS_MAX_DETS && cfg->nn_budget <= DS_MAX_BUDGET && cfg->n_streams <= DS_MAX_STREAMS,
             RTMODT_E_CAPACITY, "max_tracks %d / max_dets %d / nn_budget %d / n_streams %d: at most %d / %d / %d / %d", cfg->max_tracks, cfg->max_dets,
             cfg->nn_budget, cfg->n_streams, DS_MAX_TRACKS, DS_MAX_DETS, DS_MAX_BUDGET, DS_MAX_STREAMS);
    rtmodt_deepsort *t = new rtmodt_deepsort();
    t->device = cfg->device; t->S = cfg->n_streams; t->Mc = cfg->max_tracks; t->Nc = cfg->max_dets; t->budget = cfg->nn_budget; t->dim = dim;
    t->min_conf = cfg->min_confidence; t->max_dist = cfg->max_dist; t->max_iou = cfg->max_iou_distance; t->max_age = cfg->max_age; t->n_init = cfg->n_init;
    t->thr = (long long)std::floor(cfg->max_dist * 16129.0);
    int rc = net ? reid_open(cfg->embedder, cfg->device, cfg->n_streams, cfg->max_dets, false, &t->reid) : RTMODT_OK;     // the file is checked before the device is touched
    if (rc == RTMODT_OK) rc = ds_create_impl(t);
    return handle_created(rc, t, rtmodt_deepsort_destroy, out);
}

int rtmodt_deepsort_reset(rtmodt_deepsort *t, int stream) {
    RT_TRY(track_reset_meta(t, stream));
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? t->S : stream + 1;
    for (int s = s0; s < s1; ++s) RT_HIP(handle_zero(t->h_states[s].slot_used, (size_t)t->Mc * 4, t->stream));
    RT_TRY(handle_wait(t->stream));
    return RTMODT_OK;
}

int rtmodt_deepsort_update_batch(rtmodt_deepsort *t, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                                 const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind, const int8_t *desc,
                                 int32_t *n_returned_out) {
    bool any = false;
    RT_TRY(track_batch_check(t, xyxy, conf, cls, n, &any));
    RT_CHECK(!(frames && desc), RTMODT_E_INVALID, "give frames or descriptors, not both");
    RT_CHECK(!(t->reid && desc), RTMODT_E_INVALID, "this handle computes its descriptors with its embedder network: give frames, not descriptors");
    RT_CHECK(!any || frames || desc, RTMODT_E_INVALID, "detections need frames (built-in descriptor) or caller descriptors");
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    hipStream_t q = t->stream;
    AppFrames fp{};
    if (frames && any) RT_TRY(ds_stage(t, frames, t->S, h, w, stride_bytes, mem_kind, q, &fp));
    RT_TRY(track_batch_stage(t, xyxy, conf, cls, n, any));
    if (any && desc) RT_HIP(hipMemcpyAsync(t->d_desc, desc, (size_t)t->S * t->Nc * t->dim, hipMemcpyHostToDevice, q));
    RT_TRY(ds_run(t, ds_args(t), t->S, frames && any ? &fp : nullptr, h, w, stride_bytes, q));
    RT_HIP(hipMemcpyAsync(t->h_meta, t->d_meta, sizeof(int64_t) * 8 * t->S, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    for (int s = 0; s < t->S; ++s) {
        if (n_returned_out) n_returned_out[s] = (int32_t)t->h_meta[8 * s + 3];
        RT_TRY(ds_check_sticky(t, s, t->h_meta[8 * s + 2]));
    }
    return RTMODT_OK;
}

int rtmodt_deepsort_update_from_detector(rtmodt_deepsort *t, rtmodt_detector *det, const uint8_t *const *frames, int n_frames, int h, int w,
                                         int stride_bytes, int mem_kind) {
    RT_CHECK(t && det && frames, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(track_detector_outputs(t, det, &o));
    RT_CHECK(n_frames == o.count, RTMODT_E_INVALID, "%d frames for the detector's batch of %d", n_frames, o.count);
    RT_TRY(track_detector_fits(t, o, o.count));
    AppFrames fp{};
    RT_TRY(ds_stage(t, frames, o.count, h, w, stride_bytes, mem_kind, o.stream, &fp));
    DsArgs a = ds_args(t);
    a.det_box = o.box; a.det_conf = o.conf; a.det_cls = o.cls; a.det_n = o.n; a.det_stride = o.stride;
    RT_TRY(ds_run(t, a, o.count, &fp, h, w, stride_bytes, o.stream));
    return track_detector_done(t, o.stream);
}

int rtmodt_deepsort_state(rtmodt_deepsort *t, int stream, int64_t *ids, int32_t *state, int32_t *hits, int32_t *age, int32_t *tsu, float *xyxy,
                          float *conf, int32_t *cls, float *mean, float *cov, int32_t *gallery_count, int8_t *gallery, int32_t *n, int64_t *next_id) {
    RT_CHECK(t && stream >= 0 && stream < t->S, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(t->device));
    RT_TRY(track_join(t));
    RT_HIP(hipStreamSynchronize(t->stream));
    int64_t m[8];
    RT_HIP(hipMemcpy(m, t->d_meta + 8 * stream, sizeof(m), hipMemcpyDeviceToHost));
    RT_TRY(ds_check_sticky(t, stream, m[2]));
    const int cur = (int)m[0], cnt = (int)m[1];
    if (n) *n = cnt;
    if (next_id) *next_id = m[4];
    if (!cnt) return RTMODT_OK;
    const DsState &st = t->h_states[stream];
    const size_t c = (size_t)cnt;
    if (ids) RT_HIP(hipMemcpy(ids, st.ids[cur], c * 8, hipMemcpyDeviceToHost));
    if (state) RT_HIP(hipMemcpy(state, st.flag[cur], c * 4, hipMemcpyDeviceToHost));
    if (hits) RT_HIP(hipMemcpy(hits, st.hits[cur], c * 4, hipMemcpyDeviceToHost));
    if (age) RT_HIP(hipMemcpy(age, st.age[cur], c * 4, hipMemcpyDeviceToHost));
    if (tsu) RT_HIP(hipMemcpy(tsu, st.tsu[cur], c * 4, hipMemcpyDeviceToHost));
    if (xyxy) RT_HIP(hipMemcpy(xyxy, st.dbox[cur], c * 16, hipMemcpyDeviceToHost));
    if (conf) RT_HIP(hipMemcpy(conf, st.conf[cur], c * 4, hipMemcpyDeviceToHost));
    if (cls) RT_HIP(hipMemcpy(cls, st.cls[cur], c * 4, hipMemcpyDeviceToHost));
    if (mean || cov) {
        std::vector<float4> buf((size_t)5 * t->Mc);
        RT_HIP(hipMemcpy(buf.data(), st.kf[cur], buf.size() * sizeof(float4), hipMemcpyDeviceToHost));
        kalman_unpack(&buf[0].x, t->Mc, cnt, mean, cov);
    }
    if (gallery_count || gallery) {
        std::vector<int32_t> slot(c), total(c);
        RT_HIP(hipMemcpy(slot.data(), st.slot[cur], c * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(total.data(), st.gcount[cur], c * 4, hipMemcpyDeviceToHost));
        const size_t D = (size_t)t->dim, B = (size_t)t->budget;
        std::vector<int8_t> ring(gallery ? B * D : 0);
        for (int i = 0; i < cnt; ++i) {
            const int stored = std::min(total[i], t->budget);
            if (gallery_count) gallery_count[i] = stored;
            if (!gallery) continue;
            RT_CHECK(slot[i] >= 0 && slot[i] < t->Mc, RTMODT_E_INVALID, "stream %d: corrupt gallery slot", stream);
            RT_HIP(hipMemcpy(ring.data(), t->gallery + ds_gallery_stream_bytes(t) * stream + (size_t)slot[i] * B * D, B * D, hipMemcpyDeviceToHost));
            int8_t *o = gallery + (size_t)i * B * D;                     // oldest first
            memset(o, 0, B * D);
            const int first = total[i] - stored;                         // index (since birth) of the oldest stored sample
            for (int k = 0; k < stored; ++k) memcpy(o + (size_t)k * D, ring.data() + (size_t)((first + k) % t->budget) * D, D);
        }
    }
    return RTMODT_OK;
}

int rtmodt_deepsort_last_ms(rtmodt_deepsort *t, float *describe_ms, float *distance_ms, float *update_ms) {
    RT_CHECK(t, RTMODT_E_INVALID, "null argument");
    float a = 0, b = 0, c = 0;
    RT_TRY(t->timer.elapsed(t->device, 2, 3, &c, "no update has run yet"));      // (the last event first: it waits for the call)
    RT_TRY(t->timer.elapsed(t->device, 0, 1, &a, "no update has run yet"));
    RT_TRY(t->timer.elapsed(t->device, 1, 2, &b, "no update has run yet"));
    if (describe_ms) *describe_ms = t->described ? a : 0.f;
    if (distance_ms) *distance_ms = b;
    if (update_ms) *update_ms = c;
    return RTMODT_OK;
}

}  // extern "C"
