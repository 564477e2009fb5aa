// snapshot.hip -- the best-shot thumbnail of every track, kept in device memory: on a track list the host hands over or straight
// on the device-resident state of the four trackers.  snapshot_rule.h states the per-box rules (crop rectangle, fit, exact area
// average, score, replacement) and include/rtmodt.h the ledger rules; tests/snapshot_ref.py restates both and the kernels equal it
// exactly.  TWO launches per call whatever the tracks do, with no host read-back between them:
//   snapshot_decide    one 256-thread workgroup per stream.  Per stream a LEDGER, rows sorted by track id, double-buffered, built
//                      as speed.hip builds its own: the sampled tracks are compacted by a prefix sum, each finds its old row by
//                      binary search (old ids staged in LDS), idle rows are merged by rank (no sort), rows past retire_after leave
//                      through the `retired` list.  One thread owns one sampled track: its plan, its occlusion partners (a sweep
//                      over the other sampled boxes), its score, the replacement test.  SLOTS: one byte per slot in LDS says used
//                      or free; the new rows of a call take the k-th free slot, k their rank among the new rows in list order,
//                      both found by workgroup prefix sums -- no atomic decides an index, so the assignment is reproducible.  The
//                      bitmap that rtmodt_snapshot_state hands out is packed from those bytes.  The kernel leaves a WORK LIST of
//                      the thumbnails to write: {frame, crop, fit, destination}.
//   snapshot_resample  a fixed grid of 256-thread workgroups per stream that stride over (work item, band of SN_BAND thumbnail rows)
//                      and leave at once when the list is empty: a track whose thumbnail is kept costs nothing here.  Per
//                      thumbnail row the source rows of its span are staged in LDS in tiles of SN_TILE bytes -- consecutive
//                      threads read consecutive dwords of the row when the frame's base and pitch are multiples of 4, bytes
//                      otherwise or where a dword would leave the row -- so a crop of any width is walked tile by tile; thread e
//                      owns byte e of the image row (pixel e / 3, channel e % 3) and sums its span of each tile with the integer
//                      weights, 32-bit per source row, 64-bit across rows: one division at the end.
// No floats after conf_milli, no atomics on ledger or atlas.  rtmodt_snapshot_crop builds its work list on the host with the same
// header and runs the same resampler; rtmodt_snapshot_crop_detector builds it on the device (snapshot_pick) from the detector's
// outputs.  Results of one stream lie in one block {header, updated, retired}; the blocks of the streams a call touched come back
// in one copy, and only when an output was asked for.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "track_layout.h"
#include "frame_stage.h"
#include "handle_host.h"
#define TL_HD __host__ __device__
#include "track_ledger_host.h"

#define PV_HD __host__ __device__
#include "snapshot_rule.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_select_dev.h"
#include "track_ledger_dev.h"

constexpr int SN_THREADS = 256, SN_WAVES = SN_THREADS / 64;
constexpr int SN_BAND = 8;                  // thumbnail rows per (work item, band)
constexpr int SN_TILE = 4096;               // bytes of one source row staged at a time
constexpr int SN_EPT = (3 * SN_MAX_THUMB + SN_THREADS - 1) / SN_THREADS;      // image-row bytes per thread
constexpr int SN_GRID_X = 256;              // resampler workgroups per stream

struct SnLedger {                  // one stream, double-buffered
    int64_t *id[2], *score[2], *best_frame[2], *first[2], *last[2];
    float4 *box[2]; float *conf[2];
    int4 *ints[2];                 // {slot, cls, n_rewrites, flags}
};

struct SnHdr { int32_t n_updated, n_retired, n_work, err, n_rewritten, n_sampled, pad0, pad1; };

// one thumbnail to write: the crop of frame `frame` (an index into SnArgs::frames) -> dst
struct SnWork { int32_t frame, cx0, cy0, sw, sh, dw, dh, ox, oy, pad; uint8_t *dst; };

struct SnFrame { const uint8_t *p; int64_t frame_id; };

struct SnArgs {
    SnRuleCfg c;
    int32_t retire_after, max_updated, max_retired;
    uint32_t pad_bgr;
    SnLedger *ledgers;             // [n_streams]
    int64_t *meta;                 // [n_streams][4]: cur, rows, sticky err, 0
    uint32_t *bitmap;              // [n_streams][words]
    uint8_t *atlas; size_t atlas_stride, slot_bytes; int32_t pitch_t, words;
    char *blocks; size_t block_stride, off_updated, off_retired;      // per stream: SnHdr | updated | retired
    SnWork *work;                  // [n_streams][Mc]
    int cap, Mc, stream_base;
    const SnFrame *frames;         // [n_streams] of this call (index: stream - stream_base)
    int fh, fw; int64_t fpitch;
    // source A: a staged list [cnt][Mc], sorted by id; order = the caller's index of a sorted entry, inv = its inverse
    const int64_t *s_ids; const float4 *s_box; const float *s_conf; const int32_t *s_cls; const int32_t *s_order, *s_inv; const int32_t *s_n;
    // sources B..E: a tracker's device state (track_select_dev.h)
    TrackSrc trk;
    // per-stream scratch [n_streams][Mc]
    int32_t *p_idx, *oldpos, *dflags, *upos, *nrank, *freeslot; int64_t *tscore; SnPlan *plan;
    // the resampler's own
    int tw, th; int64_t dst_pitch; const int32_t *n_work_fixed;        // n_work_fixed != null: one list of that many items (crop), no header
};

// ------------------------------------------------------------------------------------------------------------------- decision
__global__ __launch_bounds__(SN_THREADS) void snapshot_decide(SnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x, tid = threadIdx.x;
    const int cap = a.cap, Mc = a.Mc;
    int64_t *old_id = (int64_t *)smem;                    // [cap]
    int *ret_pre = (int *)(old_id + cap);                 // [cap + 1] class of an old row, then the idle rows' rank encoding (track_ledger.h)
    int *ppre = ret_pre + cap + 1;                        // [Mc + 1] exclusive prefix of the list's sampled flags
    int *wsum = ppre + Mc + 1;                            // [SN_WAVES]
    int *s_err = wsum + SN_WAVES;                         // [1]
    uint8_t *used = (uint8_t *)(s_err + 1);               // [cap] one byte per slot

    int64_t *meta = a.meta + (size_t)sidx * 4;
    const int cur = tl_meta_cur(meta), nxt = cur ^ 1, n_old = tl_meta_rows(meta, cap);
    const SnLedger *Lp = a.ledgers + sidx;
    const int64_t *o_id = Lp->id[cur], *o_score = Lp->score[cur], *o_bf = Lp->best_frame[cur], *o_first = Lp->first[cur], *o_last = Lp->last[cur];
    const float4 *o_box = Lp->box[cur]; const float *o_conf = Lp->conf[cur]; const int4 *o_ints = Lp->ints[cur];
    int64_t *n_id = Lp->id[nxt], *n_score = Lp->score[nxt], *n_bf = Lp->best_frame[nxt], *n_first = Lp->first[nxt], *n_last = Lp->last[nxt];
    float4 *n_box = Lp->box[nxt]; float *n_conf = Lp->conf[nxt]; int4 *n_ints = Lp->ints[nxt];
    const int64_t fid = a.frames[blockIdx.x].frame_id;

    // ---- this call's list ----
    TrackSel src;
    const int32_t *order = nullptr, *inv = nullptr;
    if (a.s_ids) {
        const size_t o = (size_t)blockIdx.x * Mc;
        src = select_list(a.s_ids + o, a.s_box + o, a.s_cls + o, a.s_n[blockIdx.x]);
        src.conf = a.s_conf ? a.s_conf + o : nullptr;
        order = a.s_order + o; inv = a.s_inv + o;
    } else src = select_tracks(a.trk, sidx);
    const int n = src.n < 0 ? 0 : (src.n > Mc ? Mc : src.n);      // the host refuses a source whose max_tracks exceeds Mc
    const int64_t *ids = src.ids; const float4 *box = src.box; const int32_t *cls = src.cls;

    if (tid == 0) *s_err = 0;
    // 2: retired by this call; 1: idle unless a sampled track claims it (0)
    ledger_stage_old<SN_THREADS>(o_id, n_old, old_id, ret_pre, [&](int j) { return fid - o_last[j] > (int64_t)a.retire_after ? 2 : 1; });
    __syncthreads();

    const size_t so = (size_t)sidx * Mc;
    int32_t *p_idx = a.p_idx + so, *oldpos = a.oldpos + so, *dflags = a.dflags + so, *upos = a.upos + so, *nrank = a.nrank + so, *freeslot = a.freeslot + so;
    int64_t *tscore = a.tscore + so;
    SnPlan *plan = a.plan + so;
    SnWork *work = a.work + so;
    char *blk = a.blocks + (size_t)sidx * a.block_stride;
    SnHdr *hdr = (SnHdr *)blk;
    rtmodt_snapshot_update *upd = (rtmodt_snapshot_update *)(blk + a.off_updated);
    rtmodt_snapshot_retired *rtd = (rtmodt_snapshot_retired *)(blk + a.off_retired);

    // ---- 1. the sampled tracks, compacted in the list's (id) order; their plans ----
    const int n_s = ledger_compact<SN_THREADS>(n, ppre, p_idx, wsum, [&](int i) {
        if (!selected(src, i)) return false;
        const float4 b = box[i];
        SnPlan P;
        if (!sn_plan(a.c, b.x, b.y, b.z, b.w, cls[i], a.fh, a.fw, P)) return false;
        plan[i] = P;
        return true;
    });
    const bool ascending = ledger_list_ascends<SN_THREADS>(ids, n, s_err);

    // ---- 2. one thread per sampled track: occlusion, score, its old row, the decision ----
    for (int t = tid; t < n_s; t += SN_THREADS) {
        const int i = p_idx[t];
        const PvRect mine = plan[i].box;
        bool occl = false;
        if (a.c.occl_iou_pm > 0)
            for (int u = 0; u < n_s && !occl; ++u)
                if (u != t) occl = sn_occludes(mine, plan[p_idx[u]].box, a.c.occl_iou_pm);
        const int cm = src.conf ? sn_conf_milli(src.conf[i]) : 1000;
        const bool cut = plan[i].cut != 0;
        const int64_t score = sn_score(cm, plan[i].area, cut, occl);
        const int64_t id = ids[i];
        const int j = tl_match(old_id, n_old, id);
        const bool live = j >= 0 && ret_pre[j] == 1;                            // (ids are unique: no other thread touches ret_pre[j])
        oldpos[t] = live ? j : -1;
        if (live) ret_pre[j] = 0;
        int d = (cut ? SN_F_CUT : 0) | (occl ? SN_F_OCCLUDED : 0);
        if (!live) d |= SN_F_NEW;
        else if (sn_replaces(score, o_score[j], a.c.min_gain_pm)) d |= SN_F_REWRITTEN;
        dflags[t] = d;
        tscore[t] = score;
    }
    __syncthreads();

    // ---- 3. the old rows: idle ranks (in place), and the retired rows leave in id order ----
    int n_idle = 0, n_rtd = 0;
    for (int base = 0; base < n_old; base += SN_THREADS) {
        const int j = base + tid;
        const int c = j < n_old ? ret_pre[j] : 0;
        int tot_i, tot_r;
        const int pos_i = block_scan_count<SN_WAVES>(c == 1 ? 1 : 0, wsum, tot_i);
        const int pos_r = block_scan_count<SN_WAVES>(c == 2 ? 1 : 0, wsum, tot_r);
        if (j < n_old) ret_pre[j] = tl_rank_encode(c == 1, n_idle + pos_i);
        if (c == 2 && n_rtd + pos_r < a.max_retired) {
            rtmodt_snapshot_retired r;
            const float4 b = o_box[j];
            const int4 v = o_ints[j];
            r.track_id = old_id[j]; r.best_frame = o_bf[j]; r.first_seen = o_first[j]; r.last_seen = o_last[j];
            r.xyxy[0] = b.x; r.xyxy[1] = b.y; r.xyxy[2] = b.z; r.xyxy[3] = b.w;
            r.conf = o_conf[j]; r.slot = v.x; r.cls = v.y; r.n_rewrites = v.z;
            rtd[n_rtd + pos_r] = r;
        }
        n_idle += tot_i; n_rtd += tot_r;
    }
    if (tid == 0) ret_pre[n_old] = tl_rank_encode(false, n_idle);

    // ---- 4. in the caller's list order: the place of each update in `updated` and the rank of each new row ----
    int n_upd = 0, n_new = 0, n_rew = 0;
    for (int base = 0; base < n; base += SN_THREADS) {
        const int p = base + tid;
        int d = 0, t = 0;
        if (p < n) {
            const int i = inv ? inv[p] : p;
            if (ppre[i + 1] != ppre[i]) { t = ppre[i]; d = dflags[t] & (SN_F_NEW | SN_F_REWRITTEN); }
        }
        int tot_u, tot_n;
        const int pos_u = block_scan_count<SN_WAVES>(d ? 1 : 0, wsum, tot_u);
        const int pos_n = block_scan_count<SN_WAVES>(d & SN_F_NEW ? 1 : 0, wsum, tot_n);
        if (d) upos[t] = n_upd + pos_u;
        if (d & SN_F_NEW) nrank[t] = n_new + pos_n;
        n_upd += tot_u; n_new += tot_n;
    }
    n_rew = n_upd - n_new;
    __syncthreads();
    const bool overflow = tl_overflow(n_s, n_idle, cap) || n_new > cap - n_old;      // (or: no free slot for a new row)
    const TlMerge mg{ids, ppre, n, old_id, ret_pre, n_old, n_s, n_idle, ascending, overflow};
    if (overflow && tid == 0) *s_err = 1;

    // ---- 5. the slots in use when the call began, then the k-th free slot for the k-th new row ----
    for (int s = tid; s < cap; s += SN_THREADS) used[s] = 0;
    __syncthreads();
    auto slot_of = [&](int j) { const int s = o_ints[j].x; return s < 0 ? 0 : (s >= cap ? cap - 1 : s); };
    if (!overflow) {
        for (int j = tid; j < n_old; j += SN_THREADS) used[slot_of(j)] = 1;
    } else {                                              // an overflowing call reuses the idle and the retired rows' slots at once
        for (int t = tid; t < n_s; t += SN_THREADS)
            if (oldpos[t] >= 0) used[slot_of(oldpos[t])] = 1;
    }
    __syncthreads();
    for (int base = 0, run = 0; base < cap && run < n_new; base += SN_THREADS) {      // (run is the same in every thread)
        const int s = base + tid;
        const int f = s < cap && !used[s] ? 1 : 0;
        int tot;
        const int pos = run + block_scan_count<SN_WAVES>(f, wsum, tot);
        if (f && pos < n_new) freeslot[pos] = s;
        run += tot;
    }
    __syncthreads();
    for (int s = tid; s < cap; s += SN_THREADS) used[s] = 0;                  // from here: the slots of the NEW ledger
    __syncthreads();

    // ---- 6. one thread per sampled track: its row, its update, its work item ----
    uint8_t *atlas = a.atlas + (size_t)sidx * a.atlas_stride;
    for (int t = tid; t < n_s; t += SN_THREADS) {
        const int i = p_idx[t], j = oldpos[t], d = dflags[t];
        const int64_t id = ids[i];
        const int np = tl_member_pos(mg, t, id);
        int slot;
        if (j >= 0) {
            int4 v = o_ints[j];
            slot = slot_of(j);
            v.x = slot;
            n_id[np] = id; n_first[np] = o_first[j]; n_last[np] = fid;
            if (d & SN_F_REWRITTEN) {
                n_score[np] = tscore[t]; n_bf[np] = fid; n_box[np] = box[i]; n_conf[np] = src.conf ? src.conf[i] : 1.0f;
                v.y = cls[i]; v.z += 1; v.w = d;
            } else {
                n_score[np] = o_score[j]; n_bf[np] = o_bf[j]; n_box[np] = o_box[j]; n_conf[np] = o_conf[j];
                v.w &= SN_F_CUT | SN_F_OCCLUDED;
            }
            n_ints[np] = v;
        } else {
            int k = nrank[t];
            k = k < 0 ? 0 : (k >= Mc ? Mc - 1 : k);
            slot = freeslot[k];
            slot = slot < 0 ? 0 : (slot >= cap ? cap - 1 : slot);
            n_id[np] = id; n_first[np] = fid; n_last[np] = fid; n_score[np] = tscore[t]; n_bf[np] = fid;
            n_box[np] = box[i]; n_conf[np] = src.conf ? src.conf[i] : 1.0f;
            n_ints[np] = make_int4(slot, cls[i], 0, d);
        }
        used[slot] = 1;
        if (d & (SN_F_NEW | SN_F_REWRITTEN)) {
            const int up = upos[t];
            if (up < a.max_updated) {
                rtmodt_snapshot_update u;
                u.track_id = id; u.score = tscore[t]; u.slot = slot; u.flags = d; u.track = order ? order[i] : i; u.reserved = 0;
                upd[up] = u;
            }
            if (up >= 0 && up < Mc) {
                const SnPlan P = plan[i];
                SnWork w;
                w.frame = blockIdx.x; w.cx0 = P.crop.x0; w.cy0 = P.crop.y0; w.sw = P.sw; w.sh = P.sh; w.dw = P.dw; w.dh = P.dh; w.ox = P.ox; w.oy = P.oy;
                w.pad = 0; w.dst = atlas + (size_t)slot * a.slot_bytes;
                work[up] = w;
            }
        }
    }
    // ---- 7. idle rows move to their merged position; NEW and REWRITTEN are this call's, so they go ----
    for (int j = tid; j < n_old; j += SN_THREADS) {
        const int np = tl_idle_pos(mg, j);
        if (np < 0) continue;
        n_id[np] = old_id[j]; n_score[np] = o_score[j]; n_bf[np] = o_bf[j]; n_first[np] = o_first[j]; n_last[np] = o_last[j];
        n_box[np] = o_box[j]; n_conf[np] = o_conf[j];
        int4 w = o_ints[j];
        w.x = slot_of(j);
        w.w &= SN_F_CUT | SN_F_OCCLUDED;
        n_ints[np] = w;
        used[w.x] = 1;
    }
    __syncthreads();
    uint32_t *bm = a.bitmap + (size_t)sidx * a.words;
    for (int wd = tid; wd < a.words; wd += SN_THREADS) {
        uint32_t v = 0;
        for (int b = 0; b < 32; ++b) {
            const int s = wd * 32 + b;
            if (s < cap && used[s]) v |= 1u << b;
        }
        bm[wd] = v;
    }
    if (tid == 0) {
        tl_meta_write(meta, cur, tl_rows(mg), *s_err);
        hdr->n_updated = n_upd; hdr->n_retired = n_rtd; hdr->n_work = n_upd; hdr->err = (int32_t)meta[2]; hdr->n_rewritten = n_rew;
        hdr->n_sampled = n_s; hdr->pad0 = 0; hdr->pad1 = 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------- resampler
__global__ __launch_bounds__(SN_THREADS) void snapshot_resample(SnArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tile32[SN_TILE / 4];
    const uint8_t *tile = (const uint8_t *)tile32;
    const int tid = threadIdx.x;
    const SnWork *work;
    int n_work;
    if (a.n_work_fixed) { work = a.work; n_work = *a.n_work_fixed; }
    else {
        const int sidx = a.stream_base + blockIdx.y;
        work = a.work + (size_t)sidx * a.Mc;
        n_work = ((const SnHdr *)(a.blocks + (size_t)sidx * a.block_stride))->n_work;
        n_work = n_work < 0 ? 0 : (n_work > a.Mc ? a.Mc : n_work);
    }
    const int tw = a.tw, th = a.th;
    const int bands = (th + SN_BAND - 1) / SN_BAND;
    const long long total = (long long)n_work * bands;
    const uint32_t pad = a.pad_bgr;
    for (long long u = blockIdx.x; u < total; u += gridDim.x) {
        const SnWork w = work[u / bands];
        if (w.sw <= 0 || w.sh <= 0) continue;                           // (crop_detector: a slot past the frame's count, or a box that is not sampled)
        const int band = (int)(u % bands);
        const uint8_t *frame = a.frames[w.frame].p;
        const bool fast = (((uintptr_t)frame | (uintptr_t)a.fpitch) & 3) == 0;
        const int rb0 = 3 * w.cx0, rb1 = 3 * (w.cx0 + w.sw);          // the crop's bytes of a frame row
        const int row_bytes = 3 * a.fw;
        const int t0 = rb0 & ~3;
        const int ty1 = min(th, (band + 1) * SN_BAND);
        for (int ty = band * SN_BAND; ty < ty1; ++ty) {
            uint8_t *drow = w.dst + (size_t)ty * a.dst_pitch;
            const int dy = ty - w.oy;
            if (dy < 0 || dy >= w.dh) {                                 // a row of padding
                for (int e = tid; e < 3 * tw; e += SN_THREADS) drow[e] = (uint8_t)(pad >> (8 * (e % 3)));
                continue;
            }
            int64_t acc[SN_EPT];
#pragma unroll
            for (int k = 0; k < SN_EPT; ++k) acc[k] = 0;
            int sy0, sy1;
            sn_span(w.sh, w.dh, dy, sy0, sy1);
            for (int sy = sy0; sy <= sy1; ++sy) {
                const int wy = sn_weight(w.sh, w.dh, dy, sy);
                const uint8_t *row = frame + (size_t)(w.cy0 + sy) * a.fpitch;
                for (int cb = t0; cb < rb1; cb += SN_TILE) {
                    const int ce = min(cb + SN_TILE, rb1);
                    __syncthreads();                                    // the tile's last readers are done
                    for (int q = tid; 4 * q < ce - cb; q += SN_THREADS) {
                        const int b = cb + 4 * q;
                        if (fast && b + 4 <= row_bytes) tile32[q] = *(const uint32_t *)(row + b);
                        else {
                            uint32_t v = 0;
                            for (int m = 0; m < 4; ++m)
                                if (b + m < row_bytes) v |= (uint32_t)row[b + m] << (8 * m);
                            tile32[q] = v;
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < SN_EPT; ++k) {
                        const int e = tid + k * SN_THREADS;
                        if (e < 3 * w.dw) {
                            const int dx = e / 3, ch = e - 3 * dx;
                            int i0, i1;
                            sn_span(w.sw, w.dw, dx, i0, i1);
                            const int lo = max(i0, (cb - ch + 2) / 3 - w.cx0), hi = min(i1, (ce - 1 - ch) / 3 - w.cx0);
                            uint32_t hs = 0;
                            for (int i = lo; i <= hi; ++i) hs += (uint32_t)sn_weight(w.sw, w.dw, dx, i) * tile[3 * (w.cx0 + i) + ch - cb];
                            acc[k] += (int64_t)hs * wy;
                        }
                    }
                }
            }
            const int64_t tot = (int64_t)w.sw * w.sh;
#pragma unroll
            for (int k = 0; k < SN_EPT; ++k) {
                const int e = tid + k * SN_THREADS;
                if (e < 3 * w.dw) drow[3 * w.ox + e] = (uint8_t)((acc[k] + tot / 2) / tot);
            }
            for (int e = tid; e < 3 * w.ox; e += SN_THREADS) drow[e] = (uint8_t)(pad >> (8 * (e % 3)));
            for (int e = 3 * (w.ox + w.dw) + tid; e < 3 * tw; e += SN_THREADS) drow[e] = (uint8_t)(pad >> (8 * (e % 3)));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- review queue
// The detector's newest batch, read where the NMS left it: per frame the detections with lo <= conf < hi, in slot order, at most
// max_out of them, become work items k = frame * max_out + rank (a workgroup prefix sum gives the rank); the other items of the frame
// are empty.  index[k]: the detection's slot (-1: none); sampled[k]: the box passed snapshot_rule.h; counts[frame].
struct SnPickArgs {
    SnRuleCfg c;
    const float4 *box; const float *conf; const int32_t *n; int stride;
    float lo, hi; int max_out, fh, fw;
    SnWork *work; int32_t *index, *sampled, *counts;
    uint8_t *dst; size_t tbytes;
};

__global__ __launch_bounds__(SN_THREADS) void snapshot_pick(SnPickArgs a) {
    __shared__ int wsum[SN_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x;
    int n = a.n[f];
    n = n < 0 ? 0 : (n > a.stride ? a.stride : n);
    const float4 *box = a.box + (size_t)f * a.stride;
    const float *conf = a.conf + (size_t)f * a.stride;
    int run = 0;
    for (int base = 0; base < n; base += SN_THREADS) {
        const int i = base + tid;
        bool fl = false;
        if (i < n) { const float c = conf[i]; fl = c >= a.lo && c < a.hi; }          // (a NaN confidence is in no band)
        int tot;
        const int pos = run + block_scan_count<SN_WAVES>(fl ? 1 : 0, wsum, tot);
        if (fl && pos < a.max_out) {
            const size_t k = (size_t)f * a.max_out + pos;
            const float4 b = box[i];
            SnPlan P;
            const bool ok = sn_plan(a.c, b.x, b.y, b.z, b.w, 0, a.fh, a.fw, P);
            SnWork w{};
            if (ok) { w.frame = f; w.cx0 = P.crop.x0; w.cy0 = P.crop.y0; w.sw = P.sw; w.sh = P.sh; w.dw = P.dw; w.dh = P.dh; w.ox = P.ox; w.oy = P.oy; }
            w.dst = a.dst + k * a.tbytes;
            a.work[k] = w; a.index[k] = i; a.sampled[k] = ok ? 1 : 0;
        }
        run += tot;
    }
    const int cnt = run < a.max_out ? run : a.max_out;
    for (int k = cnt + tid; k < a.max_out; k += SN_THREADS) {
        const size_t q = (size_t)f * a.max_out + k;
        SnWork w{};
        a.work[q] = w; a.index[q] = -1; a.sampled[q] = 0;
    }
    if (tid == 0) a.counts[f] = cnt;
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_snapshot : HandleBase {
    int S = 1, Mc = 0, cap = 0, words = 0;
    bool filter = false;                  // a class list was given (the list lives on the device)
    rtmodt_snapshot_cfg cfg{};
    hipStream_t last_stream = nullptr;                       // the stream of the most recent launch (its own: HandleBase::stream)
    EventTimer<2> timer;
    char *pool = nullptr;                 // every device array but the atlas lives in this one allocation
    uint8_t *atlas = nullptr; size_t atlas_stride = 0, slot_bytes = 0; int pitch_t = 0;
    SnLedger *d_ledgers = nullptr;
    std::vector<SnLedger> h_ledgers;
    int64_t *d_meta = nullptr; uint32_t *d_bitmap = nullptr; int32_t *d_classes = nullptr, *d_nwork = nullptr;
    int32_t *p_idx = nullptr, *oldpos = nullptr, *dflags = nullptr, *upos = nullptr, *nrank = nullptr, *freeslot = nullptr;
    int64_t *tscore = nullptr; SnPlan *plan = nullptr; SnWork *work = nullptr;
    char *blocks = nullptr; size_t block_stride = 0, off_updated = 0, off_retired = 0;
    char *h_pin = nullptr;                // pinned mirror of the result blocks
    // the command block of a call (frames, frame ids, a host list) goes out in one copy from one of two pinned buffers: a call that
    // asks for no output does not wait, so the buffer the call before it wrote may still be in flight
    CmdBuf cmd[2]; hipEvent_t cmd_ev[2] = {nullptr, nullptr}; bool cmd_busy[2] = {false, false}; int cmd_i = 0;
    FrameStage stage;
    uint8_t *d_crop = nullptr; size_t crop_cap = 0;          // rtmodt_snapshot_crop: thumbnails of a call with a host destination
    char *d_pick = nullptr; size_t pick_cap = 0;             // rtmodt_snapshot_crop_detector: work | index | sampled | counts
    std::vector<int64_t> last_f; std::vector<char> has_f;
};

namespace {

size_t sn_carve(rtmodt_snapshot *z, char *base) {
    Carver c{base};
    const size_t S = z->S, cap = z->cap, Mc = z->Mc;
    z->d_ledgers = c.take<SnLedger>(S);
    z->d_meta = c.take<int64_t>(S * 4);
    z->d_bitmap = c.take<uint32_t>(S * z->words);
    z->d_classes = c.take<int32_t>(std::max(z->cfg.n_classes, 1));
    z->d_nwork = c.take<int32_t>(4);
    if (base) z->h_ledgers.assign(S, SnLedger{});
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            SnLedger tmp{};
            tmp.id[b] = c.take<int64_t>(cap); tmp.score[b] = c.take<int64_t>(cap); tmp.best_frame[b] = c.take<int64_t>(cap);
            tmp.first[b] = c.take<int64_t>(cap); tmp.last[b] = c.take<int64_t>(cap);
            tmp.box[b] = c.take<float4>(cap); tmp.conf[b] = c.take<float>(cap); tmp.ints[b] = c.take<int4>(cap);
            if (base) {
                SnLedger &L = z->h_ledgers[s];
                L.id[b] = tmp.id[b]; L.score[b] = tmp.score[b]; L.best_frame[b] = tmp.best_frame[b]; L.first[b] = tmp.first[b]; L.last[b] = tmp.last[b];
                L.box[b] = tmp.box[b]; L.conf[b] = tmp.conf[b]; L.ints[b] = tmp.ints[b];
            }
        }
    z->p_idx = c.take<int32_t>(S * Mc); z->oldpos = c.take<int32_t>(S * Mc); z->dflags = c.take<int32_t>(S * Mc);
    z->upos = c.take<int32_t>(S * Mc); z->nrank = c.take<int32_t>(S * Mc); z->freeslot = c.take<int32_t>(S * Mc);
    z->tscore = c.take<int64_t>(S * Mc); z->plan = c.take<SnPlan>(S * Mc); z->work = c.take<SnWork>(S * Mc);
    z->off_updated = sizeof(SnHdr);
    z->off_retired = align_up(z->off_updated + sizeof(rtmodt_snapshot_update) * z->cfg.max_updated, 16);
    z->block_stride = align_up(z->off_retired + sizeof(rtmodt_snapshot_retired) * z->cfg.max_retired, 16);
    z->blocks = c.take<char>(S * z->block_stride);
    return c.size();
}

size_t sn_smem(const rtmodt_snapshot *z) { return (size_t)z->cap * 8 + ((size_t)z->cap + 1 + z->Mc + 1 + SN_WAVES + 1) * 4 + (size_t)z->cap + 32; }

SnArgs sn_args(rtmodt_snapshot *z) {
    SnArgs a{};
    const rtmodt_snapshot_cfg &c = z->cfg;
    a.c = SnRuleCfg{c.thumb_h, c.thumb_w, c.margin_pm, c.min_side, c.area_cap, c.occl_iou_pm, c.min_gain_pm, z->filter ? z->d_classes : nullptr,
                    z->filter ? c.n_classes : 0};
    a.retire_after = c.retire_after; a.max_updated = c.max_updated; a.max_retired = c.max_retired;
    a.pad_bgr = (uint32_t)c.pad_bgr[0] | (uint32_t)c.pad_bgr[1] << 8 | (uint32_t)c.pad_bgr[2] << 16;
    a.ledgers = z->d_ledgers; a.meta = z->d_meta; a.bitmap = z->d_bitmap;
    a.atlas = z->atlas; a.atlas_stride = z->atlas_stride; a.slot_bytes = z->slot_bytes; a.pitch_t = z->pitch_t; a.words = z->words;
    a.blocks = z->blocks; a.block_stride = z->block_stride; a.off_updated = z->off_updated; a.off_retired = z->off_retired;
    a.work = z->work; a.cap = z->cap; a.Mc = z->Mc;
    a.p_idx = z->p_idx; a.oldpos = z->oldpos; a.dflags = z->dflags; a.upos = z->upos; a.nrank = z->nrank; a.freeslot = z->freeslot;
    a.tscore = z->tscore; a.plan = z->plan;
    a.tw = c.thumb_w; a.th = c.thumb_h; a.dst_pitch = z->pitch_t;
    return a;
}

// every stream of [s0, s0 + cnt) gets a frame id later than its last one
int sn_check_ids(rtmodt_snapshot *z, int s0, int cnt, const int64_t *frame_id) {
    for (int s = s0; s < s0 + cnt; ++s)
        RT_CHECK(!z->has_f[s] || frame_id[s - s0] > z->last_f[s], RTMODT_E_INVALID, "snapshot stream %d: frame_id %lld is not later than the last call's %lld", s,
                 (long long)frame_id[s - s0], (long long)z->last_f[s]);
    return RTMODT_OK;
}

// the pinned buffer of this call, idle again; `bytes` large
int sn_cmd(rtmodt_snapshot *z, size_t bytes, CmdBuf **out) {
    const int k = z->cmd_i;
    if (z->cmd_busy[k]) { RT_HIP(hipEventSynchronize(z->cmd_ev[k])); z->cmd_busy[k] = false; }
    RT_TRY(z->cmd[k].reserve(bytes));                      // (a regrow waits for the device itself before it frees)
    *out = &z->cmd[k];
    return RTMODT_OK;
}
int sn_cmd_send(rtmodt_snapshot *z, CmdBuf *cb, size_t bytes, hipStream_t q) {
    const int k = z->cmd_i;
    RT_HIP(hipMemcpyAsync(cb->d, cb->h, bytes, hipMemcpyHostToDevice, q));
    RT_HIP(hipEventRecord(z->cmd_ev[k], q));
    z->cmd_busy[k] = true;
    z->cmd_i = k ^ 1;
    return RTMODT_OK;
}

// the two launches on streams [s0, s0 + cnt), queued on q; then the result blocks, if any output is asked for
int sn_run(rtmodt_snapshot *z, SnArgs &a, int s0, int cnt, const int64_t *frame_id, hipStream_t q, bool flat, const rtmodt_snapshot_out *out) {
    a.stream_base = s0;
    const size_t smem = sn_smem(z);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)snapshot_decide, smem, seen));
    RT_TRY(z->timer.record(0, q));
    hipLaunchKernelGGL(snapshot_decide, dim3(cnt), dim3(SN_THREADS), smem, q, a);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(snapshot_resample, dim3(SN_GRID_X, cnt), dim3(SN_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(z->timer.record(1, q));
    z->timer.timed = true;
    z->last_stream = q;
    for (int s = 0; s < cnt; ++s) { z->last_f[s0 + s] = frame_id[s]; z->has_f[s0 + s] = 1; }
    const bool any = out && (out->updated || out->n_updated || out->retired || out->n_retired || out->n_rewritten);
    if (!any) return RTMODT_OK;
    const size_t o0 = (size_t)s0 * z->block_stride;
    RT_HIP(hipMemcpyAsync(z->h_pin + o0, z->blocks + o0, (size_t)cnt * z->block_stride, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    int rc = RTMODT_OK;
    for (int s = s0; s < s0 + cnt; ++s) {
        const char *blk = z->h_pin + (size_t)s * z->block_stride;
        const SnHdr h = *(const SnHdr *)blk;
        const size_t d = flat ? 0 : (size_t)s;
        const int nu = std::min(std::max(h.n_updated, 0), z->cfg.max_updated), nr = std::min(std::max(h.n_retired, 0), z->cfg.max_retired);
        if (out->updated && nu) memcpy(out->updated + d * z->cfg.max_updated, blk + z->off_updated, sizeof(rtmodt_snapshot_update) * nu);
        if (out->n_updated) out->n_updated[d] = nu;
        if (out->retired && nr) memcpy(out->retired + d * z->cfg.max_retired, blk + z->off_retired, sizeof(rtmodt_snapshot_retired) * nr);
        if (out->n_retired) out->n_retired[d] = nr;
        if (out->n_rewritten) out->n_rewritten[d] = h.n_rewritten;
        if (rc == RTMODT_OK) rc = ledger_check_sticky("snapshot", s, h.err, z->cap, "lower retire_after or raise max_tracks");
        if (rc == RTMODT_OK && h.n_updated > z->cfg.max_updated)
            rc = fail(RTMODT_E_CAPACITY, "snapshot stream %d: %d thumbnails written in one call > max_updated %d (the first ones are delivered)", s,
                      h.n_updated, z->cfg.max_updated);
        if (rc == RTMODT_OK && h.n_retired > z->cfg.max_retired)
            rc = fail(RTMODT_E_CAPACITY, "snapshot stream %d: %d rows retired in one call > max_retired %d (the first ones are delivered)", s, h.n_retired,
                      z->cfg.max_retired);
    }
    return rc;
}

// waits for everything the handle has queued, on its own stream and on the stream of the most recent launch
int sn_sync(rtmodt_snapshot *z) {
    RT_HIP(hipSetDevice(z->device));
    RT_HIP(hipStreamSynchronize(z->stream));
    if (z->last_stream && z->last_stream != z->stream) RT_HIP(hipStreamSynchronize(z->last_stream));
    return RTMODT_OK;
}

// the ledger, the atlas and the staged frames are read where the last call left them
int sn_order_after_last(rtmodt_snapshot *z, hipStream_t q) {
    if (z->last_stream && z->last_stream != q) RT_HIP(hipStreamSynchronize(z->last_stream));
    return RTMODT_OK;
}

int sn_check_frame_args(const uint8_t *const *frames, int n, int fh, int fw, int stride_bytes, int mem_kind) {
    RT_CHECK(frames, RTMODT_E_INVALID, "null frames");
    return check_frames(frames, n, fh, fw, stride_bytes, mem_kind, kSnapFrames);
}

// frames (staged when they are the host's) and frame ids of streams [s0, s0 + cnt) -> the head of the command block
int sn_fill_frames(rtmodt_snapshot *z, SnFrame *F, const uint8_t *const *frames, int cnt, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id) {
    RT_TRY(z->stage.place(cnt, fh, fw, stride_bytes, mem_kind, FRAMES_AS_GIVEN));
    for (int i = 0; i < cnt; ++i) { F[i].p = z->stage.at(frames, i); F[i].frame_id = frame_id ? frame_id[i] : 0; }
    return RTMODT_OK;
}

// lists of streams [s0, s0 + cnt) -> the command block, sorted by id with the caller's order both ways; then one call
int sn_process_lists(rtmodt_snapshot *z, int s0, int cnt, const int64_t *track_ids, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                     int stride, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id, bool flat,
                     const rtmodt_snapshot_out *out) {
    RT_CHECK(frame_id, RTMODT_E_INVALID, "null frame_id");
    RT_TRY(sn_check_frame_args(frames, cnt, fh, fw, stride_bytes, mem_kind));
    RT_TRY(sn_check_ids(z, s0, cnt, frame_id));
    for (int s = 0; s < cnt; ++s) {
        RT_CHECK(n[s] >= 0 && n[s] <= stride, RTMODT_E_INVALID, "stream %d: %d tracks in rows of %d", s0 + s, n[s], stride);
        RT_CHECK(n[s] <= z->Mc, RTMODT_E_CAPACITY, "%d tracks > max_tracks %d", n[s], z->Mc);
        RT_CHECK(n[s] == 0 || (track_ids && xyxy && cls), RTMODT_E_INVALID, "null tracks");
    }
    RT_HIP(hipSetDevice(z->device));
    const size_t Mc = z->Mc, m = (size_t)cnt * Mc;
    const size_t o_ids = align_up(sizeof(SnFrame) * cnt, 16), o_box = o_ids + m * 8, o_conf = o_box + m * 16, o_cls = o_conf + m * 4, o_ord = o_cls + m * 4,
                 o_inv = o_ord + m * 4, o_n = o_inv + m * 4, bytes = align_up(o_n + (size_t)cnt * 4, 16);
    CmdBuf *cb;
    RT_TRY(sn_cmd(z, bytes, &cb));
    memset(cb->h, 0, bytes);
    int64_t *ids = (int64_t *)(cb->h + o_ids); float4 *box = (float4 *)(cb->h + o_box); float *cf = (float *)(cb->h + o_conf);
    int32_t *kc = (int32_t *)(cb->h + o_cls), *perm = (int32_t *)(cb->h + o_ord), *inv = (int32_t *)(cb->h + o_inv), *nn = (int32_t *)(cb->h + o_n);
    for (int s = 0; s < cnt; ++s) {
        const int64_t *ti = track_ids + (size_t)s * stride;
        const float *tb = xyxy + (size_t)s * stride * 4;
        const float *tf = conf ? conf + (size_t)s * stride : nullptr;
        const int32_t *tc = cls + (size_t)s * stride;
        int32_t *pm = perm + s * Mc, *iv = inv + s * Mc;
        nn[s] = n[s];
        const int dup = tl_sort_list(ti, n[s], pm, iv);
        RT_CHECK(dup < 0, RTMODT_E_INVALID, "stream %d: track id %lld appears twice", s0 + s, (long long)ti[pm[dup]]);
        for (int i = 0; i < n[s]; ++i) {
            const int p = pm[i];
            ids[s * Mc + i] = ti[p]; kc[s * Mc + i] = tc[p]; cf[s * Mc + i] = tf ? tf[p] : 1.0f;
            box[s * Mc + i] = make_float4(tb[4 * p], tb[4 * p + 1], tb[4 * p + 2], tb[4 * p + 3]);
        }
    }
    hipStream_t q = z->stream;
    RT_TRY(sn_order_after_last(z, q));
    RT_TRY(sn_fill_frames(z, (SnFrame *)cb->h, frames, cnt, fh, fw, stride_bytes, mem_kind, frame_id));
    RT_TRY(z->stage.copy_in(frames, q));
    RT_TRY(sn_cmd_send(z, cb, bytes, q));
    SnArgs a = sn_args(z);
    a.frames = (const SnFrame *)cb->d; a.fh = fh; a.fw = fw; a.fpitch = (int64_t)z->stage.pitch;
    a.s_ids = (const int64_t *)(cb->d + o_ids); a.s_box = (const float4 *)(cb->d + o_box); a.s_conf = conf ? (const float *)(cb->d + o_conf) : nullptr;
    a.s_cls = (const int32_t *)(cb->d + o_cls); a.s_order = (const int32_t *)(cb->d + o_ord); a.s_inv = (const int32_t *)(cb->d + o_inv);
    a.s_n = (const int32_t *)(cb->d + o_n);
    return sn_run(z, a, s0, cnt, frame_id, q, flat, out);
}

// one call on a tracker's device-resident state
template <typename T> int sn_process_tracker(rtmodt_snapshot *z, T *trk, int report_tsu, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                             const int64_t *frame_id, const rtmodt_snapshot_out *out) {
    RT_CHECK(z && trk, RTMODT_E_INVALID, "bad argument");
    TrackSrc src;
    TrackViewBase v;
    RT_TRY(track_src(trk, report_tsu, &src, &v));
    RT_CHECK(frame_id, RTMODT_E_INVALID, "null frame_id");
    RT_TRY(ledger_check_view(v, z->device, z->S, z->Mc, z->Mc, "snapshot gallery", "snapshot gallery"));
    RT_TRY(sn_check_frame_args(frames, v.n_streams, fh, fw, stride_bytes, mem_kind));
    RT_TRY(sn_check_ids(z, 0, v.n_streams, frame_id));
    RT_HIP(hipSetDevice(z->device));
    const size_t bytes = align_up(sizeof(SnFrame) * v.n_streams, 16);
    CmdBuf *cb;
    RT_TRY(sn_cmd(z, bytes, &cb));
    hipStream_t q = v.stream;                              // the stream the tracker's last update ran on: ordered after it
    RT_TRY(sn_order_after_last(z, q));
    RT_TRY(sn_fill_frames(z, (SnFrame *)cb->h, frames, v.n_streams, fh, fw, stride_bytes, mem_kind, frame_id));
    RT_TRY(z->stage.copy_in(frames, q));
    RT_TRY(sn_cmd_send(z, cb, bytes, q));
    SnArgs a = sn_args(z);
    a.frames = (const SnFrame *)cb->d; a.fh = fh; a.fw = fw; a.fpitch = (int64_t)z->stage.pitch;
    a.trk = src;
    return sn_run(z, a, 0, v.n_streams, frame_id, q, false, out);
}

SnRuleCfg sn_host_rule(const rtmodt_snapshot_cfg &c) {
    return SnRuleCfg{c.thumb_h, c.thumb_w, c.margin_pm, c.min_side, c.area_cap, c.occl_iou_pm, c.min_gain_pm, nullptr, 0};
}

int sn_check_cfg(const rtmodt_snapshot_cfg &c) {
    RT_CHECK(c.thumb_h >= SN_MIN_THUMB && c.thumb_h <= SN_MAX_THUMB && c.thumb_w >= SN_MIN_THUMB && c.thumb_w <= SN_MAX_THUMB, RTMODT_E_INVALID,
             "thumb %dx%d outside %d..%d", c.thumb_w, c.thumb_h, SN_MIN_THUMB, SN_MAX_THUMB);
    RT_CHECK(c.margin_pm >= 0 && c.margin_pm <= 1000 && c.min_side >= 1, RTMODT_E_INVALID, "margin_pm %d (0..1000) / min_side %d (>= 1)", c.margin_pm, c.min_side);
    RT_CHECK(c.area_cap >= 1 && c.area_cap <= (1 << 28), RTMODT_E_INVALID, "area_cap %d (1..2^28)", c.area_cap);
    RT_CHECK(c.occl_iou_pm >= 0 && c.occl_iou_pm <= 1000 && c.min_gain_pm >= 0 && c.min_gain_pm <= 10000, RTMODT_E_INVALID,
             "occl_iou_pm %d (0..1000) / min_gain_pm %d (0..10000)", c.occl_iou_pm, c.min_gain_pm);
    RT_CHECK(c.retire_after >= 0, RTMODT_E_INVALID, "retire_after %d", c.retire_after);
    RT_CHECK(!c.classes || (c.n_classes >= 0 && c.n_classes <= SN_MAX_CLASSES), RTMODT_E_INVALID, "n_classes %d (0..%d)", c.n_classes, SN_MAX_CLASSES);
    return RTMODT_OK;
}

}  // namespace

extern "C" {

void rtmodt_snapshot_default_cfg(rtmodt_snapshot_cfg *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->thumb_h = 96; cfg->thumb_w = 96; cfg->margin_pm = 100; cfg->min_side = 8; cfg->area_cap = 1 << 16; cfg->occl_iou_pm = 300;
    cfg->min_gain_pm = 100; cfg->retire_after = 30; cfg->pad_bgr[0] = cfg->pad_bgr[1] = cfg->pad_bgr[2] = 114;
    cfg->max_updated = 1024; cfg->max_retired = 1024;
}

void rtmodt_snapshot_destroy(rtmodt_snapshot *z) {
    if (!z) return;
    handle_close(z, [&] {
        hipFree(z->pool); hipFree(z->atlas); hipFree(z->d_crop); hipFree(z->d_pick);
        hipHostFree(z->h_pin);
        for (int k = 0; k < 2; ++k) { z->cmd[k].release(); if (z->cmd_ev[k]) hipEventDestroy(z->cmd_ev[k]); }
        z->stage.release();
        z->timer.destroy();
    }, z->last_stream);
    delete z;
}

int rtmodt_snapshot_create(const rtmodt_snapshot_cfg *cfg, int n_streams, int max_tracks, rtmodt_snapshot **out) {
    RT_CHECK(out && cfg, RTMODT_E_INVALID, "null argument");
    const rtmodt_snapshot_cfg &c = *cfg;
    RT_TRY(sn_check_cfg(c));
    RT_CHECK(c.max_updated >= 1 && c.max_updated <= (1 << 20) && c.max_retired >= 1 && c.max_retired <= (1 << 20), RTMODT_E_INVALID,
             "max_updated %d / max_retired %d", c.max_updated, c.max_retired);
    RT_CHECK(n_streams >= 1 && n_streams <= 4096 && max_tracks >= 1 && max_tracks <= 4096, RTMODT_E_INVALID, "n_streams %d / max_tracks %d out of range",
             n_streams, max_tracks);
    rtmodt_snapshot *z = new rtmodt_snapshot();
    z->device = c.device; z->S = n_streams; z->Mc = max_tracks; z->cap = 2 * max_tracks; z->words = (z->cap + 31) / 32; z->cfg = c;
    if (!c.classes) z->cfg.n_classes = 0;
    std::vector<int32_t> classes(c.classes ? c.classes : nullptr, c.classes ? c.classes + c.n_classes : nullptr);
    z->filter = c.classes != nullptr;
    z->cfg.classes = nullptr;
    z->last_f.assign(n_streams, 0); z->has_f.assign(n_streams, 0);
    z->pitch_t = (int)tight16_pitch(c.thumb_w);
    z->slot_bytes = (size_t)c.thumb_h * z->pitch_t;
    z->atlas_stride = z->slot_bytes * z->cap;
    auto body = [&]() -> int {
        RT_CHECK(sn_smem(z) <= 150 * 1024, RTMODT_E_INVALID, "snapshot: capacity %d needs %zu B of LDS", z->cap, sn_smem(z));
        RT_TRY(handle_open(z));
        RT_TRY(z->timer.create());
        for (int k = 0; k < 2; ++k) RT_HIP(hipEventCreateWithFlags(&z->cmd_ev[k], hipEventDisableTiming));
        const size_t total = sn_carve(z, nullptr), atlas_bytes = z->atlas_stride * z->S;
        RT_HIP(hipMalloc((void **)&z->pool, total));
        RT_HIP(handle_zero(z->pool, total, z->stream));
        sn_carve(z, z->pool);
        if (hipMalloc((void **)&z->atlas, atlas_bytes) != hipSuccess) {
            z->atlas = nullptr;
            (void)hipGetLastError();
            return fail(RTMODT_E_HIP, "snapshot: the thumbnail atlas of %d streams x %d slots of %dx%d needs %zu bytes of device memory", z->S, z->cap, c.thumb_w,
                        c.thumb_h, atlas_bytes);
        }
        RT_HIP(handle_zero(z->atlas, atlas_bytes, z->stream));
        RT_HIP(hipHostMalloc((void **)&z->h_pin, (size_t)z->S * z->block_stride, hipHostMallocDefault));
        RT_HIP(hipMemcpyAsync(z->d_ledgers, z->h_ledgers.data(), sizeof(SnLedger) * z->S, hipMemcpyHostToDevice, z->stream));      // (behind the zeroing of the pool)
        if (!classes.empty()) RT_HIP(hipMemcpyAsync(z->d_classes, classes.data(), classes.size() * 4, hipMemcpyHostToDevice, z->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), z, rtmodt_snapshot_destroy, out);
}

int rtmodt_snapshot_process(rtmodt_snapshot *z, int stream, const int64_t *track_ids, const float *xyxy, const float *conf, const int32_t *cls, int n,
                            const uint8_t *frame, int fh, int fw, int stride_bytes, int mem_kind, int64_t frame_id, const rtmodt_snapshot_out *out) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n >= 0, RTMODT_E_INVALID, "bad argument");
    const int32_t n32 = n;
    return sn_process_lists(z, stream, 1, track_ids, xyxy, conf, cls, &n32, std::max(n, 1), &frame, fh, fw, stride_bytes, mem_kind, &frame_id, true, out);
}

int rtmodt_snapshot_process_batch(rtmodt_snapshot *z, const int64_t *track_ids, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                                  int stride, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id,
                                  const rtmodt_snapshot_out *out) {
    RT_CHECK(z && n && stride >= 0, RTMODT_E_INVALID, "bad argument");
    return sn_process_lists(z, 0, z->S, track_ids, xyxy, conf, cls, n, stride, frames, fh, fw, stride_bytes, mem_kind, frame_id, false, out);
}

int rtmodt_snapshot_process_tracker(rtmodt_snapshot *z, rtmodt_tracker *trk, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                    const int64_t *frame_id, int report_tsu, const rtmodt_snapshot_out *out) {
    return sn_process_tracker(z, trk, report_tsu, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_snapshot_process_deepsort(rtmodt_snapshot *z, rtmodt_deepsort *ds, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                     const int64_t *frame_id, int report_tsu, const rtmodt_snapshot_out *out) {
    return sn_process_tracker(z, ds, report_tsu, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_snapshot_process_ocsort(rtmodt_snapshot *z, rtmodt_ocsort *oc, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                   const int64_t *frame_id, const rtmodt_snapshot_out *out) {
    return sn_process_tracker(z, oc, 0, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_snapshot_process_botsort(rtmodt_snapshot *z, rtmodt_botsort *bot, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                    const int64_t *frame_id, const rtmodt_snapshot_out *out) {
    return sn_process_tracker(z, bot, 0, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_snapshot_atlas(rtmodt_snapshot *z, int stream, void **dev_ptr, size_t *slot_bytes, int32_t *pitch) {
    RT_CHECK(z && stream >= 0 && stream < z->S, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sn_sync(z));
    if (dev_ptr) *dev_ptr = z->atlas + (size_t)stream * z->atlas_stride;
    if (slot_bytes) *slot_bytes = z->slot_bytes;
    if (pitch) *pitch = z->pitch_t;
    return RTMODT_OK;
}

int rtmodt_snapshot_read(rtmodt_snapshot *z, int stream, const int32_t *slots, int n, uint8_t *out) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n >= 0 && (n == 0 || (slots && out)), RTMODT_E_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) RT_CHECK(slots[i] >= 0 && slots[i] < z->cap, RTMODT_E_INVALID, "slot %d outside 0..%d", slots[i], z->cap - 1);
    RT_TRY(sn_sync(z));
    const size_t tight = (size_t)3 * z->cfg.thumb_w;
    for (int i = 0; i < n; ++i)
        RT_HIP(hipMemcpy2D(out + (size_t)i * tight * z->cfg.thumb_h, tight, z->atlas + (size_t)stream * z->atlas_stride + (size_t)slots[i] * z->slot_bytes,
                           (size_t)z->pitch_t, tight, (size_t)z->cfg.thumb_h, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_snapshot_state(rtmodt_snapshot *z, int stream, int64_t *ids, int64_t *best_score, int64_t *best_frame, int64_t *first_seen, int64_t *last_seen,
                          float *xyxy, float *conf, int32_t *ints, uint32_t *bitmap, int32_t *n) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sn_sync(z));
    int64_t m[4];
    RT_HIP(hipMemcpy(m, z->d_meta + 4 * stream, sizeof(m), hipMemcpyDeviceToHost));
    RT_CHECK(m[2] == 0 || m[2] == 1, RTMODT_E_INVALID, "snapshot stream %d: error %lld", stream, (long long)m[2]);
    const int cur = (int)m[0] & 1, cnt = (int)m[1];
    RT_CHECK(cnt >= 0 && cnt <= z->cap, RTMODT_E_INVALID, "snapshot stream %d: corrupt row count", stream);
    const SnLedger &L = z->h_ledgers[stream];
    *n = cnt;
    // a stream in error still hands its rows out (the rows of the overflowing call and of the calls since), with the error code
    auto full = [&]() -> int {
        RT_CHECK(m[2] != 1, RTMODT_E_CAPACITY, "snapshot stream %d: ledger full (%d rows): lower retire_after or raise max_tracks", stream, z->cap);
        return RTMODT_OK;
    };
    if (bitmap) RT_HIP(hipMemcpy(bitmap, z->d_bitmap + (size_t)stream * z->words, (size_t)z->words * 4, hipMemcpyDeviceToHost));
    if (!cnt) return full();
    const size_t c = (size_t)cnt;
    if (ids) RT_HIP(hipMemcpy(ids, L.id[cur], c * 8, hipMemcpyDeviceToHost));
    if (best_score) RT_HIP(hipMemcpy(best_score, L.score[cur], c * 8, hipMemcpyDeviceToHost));
    if (best_frame) RT_HIP(hipMemcpy(best_frame, L.best_frame[cur], c * 8, hipMemcpyDeviceToHost));
    if (first_seen) RT_HIP(hipMemcpy(first_seen, L.first[cur], c * 8, hipMemcpyDeviceToHost));
    if (last_seen) RT_HIP(hipMemcpy(last_seen, L.last[cur], c * 8, hipMemcpyDeviceToHost));
    if (xyxy) RT_HIP(hipMemcpy(xyxy, L.box[cur], c * 16, hipMemcpyDeviceToHost));
    if (conf) RT_HIP(hipMemcpy(conf, L.conf[cur], c * 4, hipMemcpyDeviceToHost));
    if (ints) RT_HIP(hipMemcpy(ints, L.ints[cur], c * 16, hipMemcpyDeviceToHost));
    return full();
}

int rtmodt_snapshot_reset(rtmodt_snapshot *z, int stream) {
    RT_CHECK(z && stream >= 0 && stream < z->S, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sn_sync(z));
    RT_HIP(handle_zero(z->d_meta + 4 * stream, 4 * sizeof(int64_t), z->stream));
    RT_HIP(handle_zero(z->d_bitmap + (size_t)stream * z->words, (size_t)z->words * 4, z->stream));
    RT_TRY(handle_wait(z->stream));
    z->has_f[stream] = 0; z->last_f[stream] = 0;
    return RTMODT_OK;
}

int rtmodt_snapshot_plan(const rtmodt_snapshot_cfg *cfg, const float *xyxy, int h, int w, rtmodt_snapshot_plan_out *out) {
    RT_CHECK(cfg && xyxy && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(sn_check_cfg(*cfg));
    RT_CHECK(h >= 1 && w >= 1 && h <= SN_MAX_DIM && w <= SN_MAX_DIM, RTMODT_E_INVALID, "frame %dx%d outside 1..%d", w, h, SN_MAX_DIM);
    SnPlan P;
    out->sampled = sn_plan(sn_host_rule(*cfg), xyxy[0], xyxy[1], xyxy[2], xyxy[3], 0, h, w, P) ? 1 : 0;
    if (!out->sampled) return RTMODT_OK;
    const PvRect *r[3] = {&P.raw, &P.box, &P.crop};
    int32_t *d[3] = {out->raw, out->box, out->crop};
    for (int k = 0; k < 3; ++k) { d[k][0] = r[k]->x0; d[k][1] = r[k]->y0; d[k][2] = r[k]->x1; d[k][3] = r[k]->y1; }
    out->sw = P.sw; out->sh = P.sh; out->dw = P.dw; out->dh = P.dh; out->ox = P.ox; out->oy = P.oy; out->cut = P.cut; out->area = P.area;
    return RTMODT_OK;
}

int rtmodt_snapshot_crop(rtmodt_snapshot *z, const uint8_t *const *frames, int n_frames, int fh, int fw, int stride_bytes, int mem_kind, const float *xyxy,
                         const int32_t *frame_idx, int n_boxes, uint8_t *out, int out_mem_kind, int32_t *sampled) {
    RT_CHECK(z && n_frames >= 0 && n_boxes >= 0, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sn_check_frame_args(frames, n_frames, fh, fw, stride_bytes, mem_kind));
    RT_TRY(check_mem_kind(out_mem_kind));
    RT_CHECK(n_frames <= 65535 && n_boxes <= (1 << 20), RTMODT_E_CAPACITY, "%d frames / %d boxes in one call", n_frames, n_boxes);
    if (n_boxes == 0) return RTMODT_OK;
    RT_CHECK(xyxy && frame_idx && out, RTMODT_E_INVALID, "null argument");
    for (int i = 0; i < n_boxes; ++i) RT_CHECK(frame_idx[i] >= 0 && frame_idx[i] < n_frames, RTMODT_E_INVALID, "box %d: frame index %d outside 0..%d", i, frame_idx[i], n_frames - 1);
    RT_HIP(hipSetDevice(z->device));
    const size_t tight = (size_t)3 * z->cfg.thumb_w, tbytes = tight * z->cfg.thumb_h;
    const bool host_out = out_mem_kind == RTMODT_MEM_HOST;
    if (host_out) RT_TRY(dev_grow(&z->d_crop, &z->crop_cap, tbytes * n_boxes));
    uint8_t *dst = host_out ? z->d_crop : out;
    const size_t o_work = align_up(sizeof(SnFrame) * n_frames, 16), bytes = align_up(o_work + sizeof(SnWork) * n_boxes, 16);
    CmdBuf *cb;
    RT_TRY(sn_cmd(z, bytes, &cb));
    hipStream_t q = z->stream;
    RT_TRY(sn_order_after_last(z, q));
    RT_TRY(sn_fill_frames(z, (SnFrame *)cb->h, frames, n_frames, fh, fw, stride_bytes, mem_kind, nullptr));
    const SnRuleCfg rule = sn_host_rule(z->cfg);
    SnWork *W = (SnWork *)(cb->h + o_work);
    int n_work = 0;
    std::vector<int32_t> which;
    for (int i = 0; i < n_boxes; ++i) {
        SnPlan P;
        const bool ok = sn_plan(rule, xyxy[4 * i], xyxy[4 * i + 1], xyxy[4 * i + 2], xyxy[4 * i + 3], 0, fh, fw, P);
        if (sampled) sampled[i] = ok ? 1 : 0;
        if (!ok) continue;
        SnWork w;
        w.frame = frame_idx[i]; w.cx0 = P.crop.x0; w.cy0 = P.crop.y0; w.sw = P.sw; w.sh = P.sh; w.dw = P.dw; w.dh = P.dh; w.ox = P.ox; w.oy = P.oy; w.pad = 0;
        w.dst = dst + (size_t)i * tbytes;
        W[n_work++] = w;
        which.push_back(i);
    }
    if (n_work == 0) return RTMODT_OK;
    RT_TRY(z->stage.copy_in(frames, q));
    RT_TRY(sn_cmd_send(z, cb, bytes, q));
    RT_HIP(hipMemcpyAsync(z->d_nwork, &n_work, sizeof(int32_t), hipMemcpyHostToDevice, q));
    SnArgs a = sn_args(z);
    a.frames = (const SnFrame *)cb->d; a.fh = fh; a.fw = fw; a.fpitch = (int64_t)z->stage.pitch;
    a.work = (SnWork *)(cb->d + o_work); a.n_work_fixed = z->d_nwork; a.dst_pitch = (int64_t)tight;
    const int bands = (z->cfg.thumb_h + SN_BAND - 1) / SN_BAND;
    const int grid = (int)std::min<long long>((long long)n_work * bands, 4096);
    RT_TRY(z->timer.record(0, q));
    hipLaunchKernelGGL(snapshot_resample, dim3(grid), dim3(SN_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(z->timer.record(1, q));
    z->timer.timed = true;
    z->last_stream = q;
    if (host_out)
        for (int i : which) RT_HIP(hipMemcpyAsync(out + (size_t)i * tbytes, z->d_crop + (size_t)i * tbytes, tbytes, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    return RTMODT_OK;
}

int rtmodt_snapshot_crop_detector(rtmodt_snapshot *z, rtmodt_detector *det, const uint8_t *const *frames, int n, int fh, int fw, int stride_bytes, int mem_kind,
                                  float conf_lo, float conf_hi, int max_out, uint8_t *out, int out_mem_kind, int32_t *index, int32_t *counts, int32_t *sampled) {
    RT_CHECK(z && det, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(detector_outputs(det, &o));
    RT_CHECK(o.device == z->device, RTMODT_E_INVALID, "snapshot gallery on device %d, detector on device %d", z->device, o.device);
    RT_CHECK(n >= 0 && n <= o.count, RTMODT_E_INVALID, "%d frames, the detector's newest batch has %d", n, o.count);
    RT_CHECK(max_out >= 1 && max_out <= o.stride, RTMODT_E_INVALID, "max_out %d (1..max_det %d)", max_out, o.stride);
    RT_TRY(sn_check_frame_args(frames, n, fh, fw, stride_bytes, mem_kind));
    RT_TRY(check_mem_kind(out_mem_kind));
    if (n == 0) return RTMODT_OK;
    RT_CHECK(out && index && counts, RTMODT_E_INVALID, "null argument");
    RT_HIP(hipSetDevice(z->device));
    const size_t tight = (size_t)3 * z->cfg.thumb_w, tbytes = tight * z->cfg.thumb_h, m = (size_t)n * max_out;
    const bool host_out = out_mem_kind == RTMODT_MEM_HOST;
    if (host_out) RT_TRY(dev_grow(&z->d_crop, &z->crop_cap, tbytes * m));
    const size_t o_index = align_up(sizeof(SnWork) * m, 16), o_sampled = o_index + align_up(4 * m, 16), o_counts = o_sampled + align_up(4 * m, 16),
                 pbytes = o_counts + align_up((size_t)4 * n, 16);
    RT_TRY(dev_grow(&z->d_pick, &z->pick_cap, pbytes));
    const size_t bytes = align_up(sizeof(SnFrame) * n, 16);
    CmdBuf *cb;
    RT_TRY(sn_cmd(z, bytes, &cb));
    hipStream_t q = o.stream;                              // the detector's post-processing stream: ordered behind its NMS
    RT_TRY(sn_order_after_last(z, q));
    RT_TRY(sn_fill_frames(z, (SnFrame *)cb->h, frames, n, fh, fw, stride_bytes, mem_kind, nullptr));
    RT_TRY(z->stage.copy_in(frames, q));
    RT_TRY(sn_cmd_send(z, cb, bytes, q));
    const int32_t n_work = (int32_t)m;
    RT_HIP(hipMemcpyAsync(z->d_nwork, &n_work, sizeof(int32_t), hipMemcpyHostToDevice, q));
    SnPickArgs p{};
    p.c = sn_host_rule(z->cfg);
    p.box = o.box; p.conf = o.conf; p.n = o.n; p.stride = o.stride; p.lo = conf_lo; p.hi = conf_hi; p.max_out = max_out; p.fh = fh; p.fw = fw;
    p.work = (SnWork *)z->d_pick; p.index = (int32_t *)(z->d_pick + o_index); p.sampled = (int32_t *)(z->d_pick + o_sampled);
    p.counts = (int32_t *)(z->d_pick + o_counts);
    p.dst = host_out ? z->d_crop : out; p.tbytes = tbytes;
    SnArgs a = sn_args(z);
    a.frames = (const SnFrame *)cb->d; a.fh = fh; a.fw = fw; a.fpitch = (int64_t)z->stage.pitch;
    a.work = p.work; a.n_work_fixed = z->d_nwork; a.dst_pitch = (int64_t)tight;
    const int bands = (z->cfg.thumb_h + SN_BAND - 1) / SN_BAND;
    const int grid = (int)std::min<long long>((long long)m * bands, 4096);
    RT_TRY(z->timer.record(0, q));
    hipLaunchKernelGGL(snapshot_pick, dim3(n), dim3(SN_THREADS), 0, q, p);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(snapshot_resample, dim3(grid), dim3(SN_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(z->timer.record(1, q));
    z->timer.timed = true;
    z->last_stream = q;
    std::vector<char> res(pbytes - o_index);               // index | sampled | counts lie behind one another: one copy
    RT_HIP(hipMemcpyAsync(res.data(), z->d_pick + o_index, res.size(), hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    const int32_t *h_sampled = (const int32_t *)(res.data() + (o_sampled - o_index));
    memcpy(index, res.data(), 4 * m);
    if (sampled) memcpy(sampled, h_sampled, 4 * m);
    memcpy(counts, res.data() + (o_counts - o_index), (size_t)4 * n);
    if (host_out) {
        for (size_t k = 0; k < m; ++k)
            if (h_sampled[k]) RT_HIP(hipMemcpyAsync(out + k * tbytes, z->d_crop + k * tbytes, tbytes, hipMemcpyDeviceToHost, q));
        RT_HIP(hipStreamSynchronize(q));
    }
    return RTMODT_OK;
}

int rtmodt_snapshot_last_ms(rtmodt_snapshot *z, float *kernel_ms) {
    RT_CHECK(z && kernel_ms, RTMODT_E_INVALID, "null argument");
    return z->timer.elapsed(z->device, 0, 1, kernel_ms, "no call has been timed yet");
}

}  // extern "C"
