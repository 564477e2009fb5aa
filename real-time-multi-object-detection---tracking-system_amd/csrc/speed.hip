// speed.hip -- track speed, odometer, speeding / stopped / wrong-way alarms, a speed histogram and proximity pairs on a world
// ground plane, on a track list the host hands over or straight on the device-resident state of the four trackers.  A fixed
// camera and one plane per stream; ground_plane.h states the per-point rules (anchor, float64 projection in a fixed operation
// order, integer distance and speed) and include/rtmodt.h the ledger and alarm rules; tests/speed_ref.py restates both and the
// kernels equal it exactly.  TWO launches per call whatever the tracks do:
//   speed_update   one 256-thread workgroup per stream.  Per stream a LEDGER, rows sorted by track id, double-buffered, built by
//                  the steps of track_ledger_dev.h as crossing.hip builds its own: the sampled tracks are compacted by a prefix sum, each finds its old row by binary
//                  search (old ids staged in LDS), idle rows within max_gap_us are retained and merged by rank (no sort), rows
//                  beyond it dropped.  One thread owns one sampled track's row: ring, odometer, speed, alarms.  No atomics except the
//                  integer adds into the histogram; every loop strides over the workgroup, so a list longer than 256 works.
//   speed_pairs    (proximity_mm > 0) one workgroup per stream over the rows the first launch wrote: the world points staged in
//                  LDS, thread i counts its partners j > i, a workgroup prefix sum turns the counts into offsets, and a second
//                  sweep writes the pairs -- in (i, j) order whatever the scheduling.
// Results of one stream lie in one block {header, events, pairs, rows}; the blocks of the streams a call touched come back in one copy.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "handle_host.h"
#include "track_layout.h"

#define GP_HD __host__ __device__
#include "ground_plane.h"
#define TL_HD __host__ __device__
#include "track_ledger_host.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_select_dev.h"
#include "track_ledger_dev.h"

constexpr int SP_THREADS = 256, SP_WAVES = SP_THREADS / 64;
constexpr int SP_MAX_WINDOW = 32, SP_MAX_BINS = 256, SP_MAX_CLASSES = 256;

struct SpLedger {                  // one stream, double-buffered; ring_* are [window][cap]
    int64_t *id[2], *last[2], *odo[2], *since[2], *ring_t[2];
    int2 *ring_xy[2], *anchor[2], *chord[2];
    int4 *a[2], *b[2];             // a = {n_samples, head, speed, peak}; b = {cls, flags, speeding run, wrong-way run}
};

struct SpHdr { int32_t n_rows, n_events, total_pairs, err; };

struct SpCfgDev {
    int anchor, window, min_samples, hold, min_step, limit, stop, ww_min, ax, ay, bins, bin_w, n_classes, max_events, max_pairs;
    int64_t max_gap, stop_us, prox2;
    const int32_t *classes;
};

struct SpArgs {
    SpCfgDev c;
    SpLedger *ledgers;             // [n_streams]
    int64_t *meta;                 // [n_streams][4]: cur, rows, sticky err, 0
    const double *H;               // [n_streams][9]
    int64_t *hist;                 // [n_streams][max(bins, 1)]
    char *blocks; size_t block_stride, off_events, off_pairs, off_rows;       // per stream: SpHdr | events | pairs | rows
    int cap, Mc, stream_base;
    int64_t t_one; const int64_t *t_dev;     // the timestamp of every stream, or one per stream
    // source A: a staged list [n_streams][Mc], sorted by id; order = the caller's index of a sorted entry, inv = its inverse
    const int64_t *s_ids; const float4 *s_box; const int32_t *s_cls; const int32_t *s_order, *s_inv; const int32_t *s_n;
    // sources B..E: a tracker's device state (track_select_dev.h)
    TrackSrc trk;
    // per-stream scratch [n_streams][Mc]
    int32_t *p_idx, *oldpos, *krow, *evbits, *pair_off; int2 *wxy;
};

#pragma clang fp contract(off)

__global__ __launch_bounds__(SP_THREADS) void speed_update(SpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x, tid = threadIdx.x;
    const int cap = a.cap, Mc = a.Mc, W = a.c.window;
    double *sH = (double *)smem;                          // [10] the stream's plane (9 used; every carve offset a multiple of 16)
    int64_t *old_id = (int64_t *)(sH + 10);               // [cap]
    int *ret_pre = (int *)(old_id + cap);                 // [cap + 1] retained flags, then their rank encoding (track_ledger.h)
    int *ppre = ret_pre + cap + 1;                        // [Mc + 1] exclusive prefix of the list's sampled flags
    int *wsum = ppre + Mc + 1;                            // [SP_WAVES]
    int &s_err = wsum[SP_WAVES];                          // [1]

    int64_t *meta = a.meta + (size_t)sidx * 4;
    const int cur = tl_meta_cur(meta), nxt = cur ^ 1, n_old = tl_meta_rows(meta, cap);
    const SpLedger *Lp = a.ledgers + sidx;
    const int64_t *o_id = Lp->id[cur], *o_last = Lp->last[cur], *o_odo = Lp->odo[cur], *o_since = Lp->since[cur], *o_rt = Lp->ring_t[cur];
    const int2 *o_rxy = Lp->ring_xy[cur], *o_anchor = Lp->anchor[cur], *o_chord = Lp->chord[cur];
    const int4 *o_a = Lp->a[cur], *o_b = Lp->b[cur];
    int64_t *n_id = Lp->id[nxt], *n_last = Lp->last[nxt], *n_odo = Lp->odo[nxt], *n_since = Lp->since[nxt], *n_rt = Lp->ring_t[nxt];
    int2 *n_rxy = Lp->ring_xy[nxt], *n_anchor = Lp->anchor[nxt], *n_chord = Lp->chord[nxt];
    int4 *n_a = Lp->a[nxt], *n_b = Lp->b[nxt];
    const int64_t now = a.t_dev ? a.t_dev[sidx] : a.t_one;

    // ---- this call's list ----
    TrackSel src;
    const int32_t *order = nullptr, *inv = nullptr;
    if (a.s_ids) {
        const size_t o = (size_t)sidx * Mc;
        src = select_list(a.s_ids + o, a.s_box + o, a.s_cls + o, a.s_n[sidx]);
        order = a.s_order + o; inv = a.s_inv + o;
    } else src = select_tracks(a.trk, sidx);
    const int n = src.n < 0 ? 0 : (src.n > Mc ? Mc : src.n);      // the host refuses a source whose max_tracks exceeds Mc
    const int64_t *ids = src.ids; const float4 *box = src.box; const int32_t *cls = src.cls;

    if (tid == 0) s_err = 0;
    if (tid < 9) sH[tid] = a.H[(size_t)sidx * 9 + tid];
    // an old row survives this call while now - last <= max_gap_us, whether or not its id is in the list
    ledger_stage_old<SP_THREADS>(o_id, n_old, old_id, ret_pre, [&](int j) { return now - o_last[j] <= a.c.max_gap ? 1 : 0; });
    __syncthreads();

    int32_t *p_idx = a.p_idx + (size_t)sidx * Mc, *oldpos = a.oldpos + (size_t)sidx * Mc, *krow = a.krow + (size_t)sidx * Mc;
    int32_t *evbits = a.evbits + (size_t)sidx * Mc;
    int2 *wxy = a.wxy + (size_t)sidx * Mc;
    char *blk = a.blocks + (size_t)sidx * a.block_stride;
    SpHdr *hdr = (SpHdr *)blk;
    rtmodt_speed_event *evs = (rtmodt_speed_event *)(blk + a.off_events);
    rtmodt_speed_row *rows = (rtmodt_speed_row *)(blk + a.off_rows);

    // ---- 1. the sampled tracks, compacted in the list's (id) order; each finds its old row (an expired one is not this track's
    //         row); the idle rows are ranked ----
    const int n_s = ledger_compact<SP_THREADS>(n, ppre, p_idx, wsum, [&](int i) {
        if (!selected(src, i)) return false;
        bool listed = a.c.classes == nullptr;
        const int k = cls[i];
        for (int q = 0; q < a.c.n_classes && !listed; ++q) listed = a.c.classes[q] == k;
        const float4 b = box[i];
        float u, v;
        int32_t X, Y;
        if (!(listed && gp_anchor(a.c.anchor, b.x, b.y, b.z, b.w, u, v) && gp_project(sH, u, v, X, Y))) return false;
        wxy[i] = make_int2(X, Y);
        return true;
    });
    const bool ascending = ledger_list_ascends<SP_THREADS>(ids, n, &s_err);
    ledger_match<SP_THREADS, true>(ids, p_idx, n_s, old_id, n_old, ret_pre, oldpos);
    const int n_ret = ledger_rank<SP_THREADS>(n_old, ret_pre, wsum);              // (its last barrier: ppre[n] is read below)
    // the row position of each sampled track: the caller's list order (a tracker's list: its own order)
    for (int base = 0, run = 0; base < n; base += SP_THREADS) {
        const int p = base + tid;
        int i = 0;
        bool f = false;
        if (p < n) { i = inv ? inv[p] : p; f = ppre[i + 1] != ppre[i]; }
        int tot;
        const int pos = run + block_scan_count<SP_WAVES>(f ? 1 : 0, wsum, tot);
        if (f) krow[ppre[i]] = pos;
        run += tot;
    }
    __syncthreads();
    const TlMerge mg = ledger_decide(ids, ppre, n, old_id, ret_pre, n_old, n_s, n_ret, ascending, cap, &s_err);

    // ---- 2. one thread per sampled track: its row ----
    int64_t *hist = a.hist + (size_t)sidx * (a.c.bins > 0 ? a.c.bins : 1);
    for (int t = tid; t < n_s; t += SP_THREADS) {
        const int i = p_idx[t], j = oldpos[t];
        const int64_t id = ids[i];
        const int2 P = wxy[i];
        const int np = tl_member_pos(mg, t, id);
        int cnt = 0, head = -1, peak = -1, flags = RTMODT_SPEED_F_NEW, run_s = 0, run_w = 0;
        int64_t odo = 0, since = 0;
        int2 anchor = P;
        if (j >= 0) {
            const int4 oa = o_a[j], ob = o_b[j];
            cnt = oa.x; head = oa.y; peak = oa.w; flags = ob.y & ~RTMODT_SPEED_F_NEW; run_s = ob.z; run_w = ob.w;
            odo = o_odo[j]; since = o_since[j]; anchor = o_anchor[j];
            for (int k = 0; k < W; ++k) {                                     // the ring moves with the row
                n_rxy[(size_t)k * cap + np] = o_rxy[(size_t)k * cap + j];
                n_rt[(size_t)k * cap + np] = o_rt[(size_t)k * cap + j];
            }
            const int64_t step = gp_isqrt(gp_dist2(anchor.x, anchor.y, P.x, P.y));
            if (step >= a.c.min_step) { odo += step; anchor = P; }
        }
        head = head + 1 == W ? 0 : head + 1;
        cnt = cnt < W ? cnt + 1 : W;
        n_rxy[(size_t)head * cap + np] = P;
        n_rt[(size_t)head * cap + np] = now;
        int speed = -1;
        int2 chord = make_int2(0, 0);
        if (cnt >= a.c.min_samples) {
            int os = head - cnt + 1;
            os = os < 0 ? os + W : os;
            const int2 Q = j >= 0 ? o_rxy[(size_t)os * cap + j] : P;          // (cnt >= 2 here: the oldest sample lies in the old row)
            const int64_t tq = j >= 0 ? o_rt[(size_t)os * cap + j] : now;
            chord = make_int2(P.x - Q.x, P.y - Q.y);
            speed = gp_speed(gp_isqrt(gp_dist2(Q.x, Q.y, P.x, P.y)), now - tq);
            if (a.c.bins > 0) atomicAdd((unsigned long long *)&hist[min(speed / a.c.bin_w, a.c.bins - 1)], 1ull);
        }
        peak = speed > peak ? speed : peak;
        int ev = 0;
        if (a.c.limit > 0) {
            if (speed > a.c.limit) {
                run_s = run_s < a.c.hold ? run_s + 1 : run_s;
                if (run_s >= a.c.hold && !(flags & 1)) { flags |= 1; ev |= 1; }
            } else { run_s = 0; flags &= ~1; }
        }
        if (a.c.stop > 0) {
            if (speed >= 0 && speed < a.c.stop) {
                if (!(flags & RTMODT_SPEED_F_TIMER)) { flags |= RTMODT_SPEED_F_TIMER; since = now; }
                if (now - since >= a.c.stop_us && !(flags & 2)) { flags |= 2; ev |= 2; }
            } else flags &= ~(RTMODT_SPEED_F_TIMER | 2);
        }
        if (a.c.ax != 0 || a.c.ay != 0) {
            const int64_t dot = (int64_t)chord.x * a.c.ax + (int64_t)chord.y * a.c.ay;
            if (speed >= 0 && speed >= a.c.ww_min && dot < 0) {
                run_w = run_w < a.c.hold ? run_w + 1 : run_w;
                if (run_w >= a.c.hold && !(flags & 4)) { flags |= 4; ev |= 4; }
            } else { run_w = 0; flags &= ~4; }
        }
        const int k = cls[i];
        n_id[np] = id; n_last[np] = now; n_odo[np] = odo; n_since[np] = since;
        n_anchor[np] = anchor; n_chord[np] = chord;
        n_a[np] = make_int4(cnt, head, speed, peak);
        n_b[np] = make_int4(k, flags, run_s, run_w);
        evbits[t] = ev;
        rtmodt_speed_row r;
        r.track_id = id; r.odometer_mm = odo; r.track = order ? order[i] : i; r.cls = k;
        r.world[0] = P.x; r.world[1] = P.y; r.speed_mm_s = speed; r.peak_mm_s = peak;
        r.heading[0] = chord.x; r.heading[1] = chord.y; r.flags = flags; r.n_samples = cnt;
        rows[krow[t]] = r;
    }
    // ---- 3. idle rows move to their merged position, unchanged ----
    for (int j = tid; j < n_old; j += SP_THREADS) {
        const int np = tl_idle_pos(mg, j);
        if (np < 0) continue;
        n_id[np] = old_id[j]; n_last[np] = o_last[j]; n_odo[np] = o_odo[j]; n_since[np] = o_since[j];
        n_anchor[np] = o_anchor[j]; n_chord[np] = o_chord[j];
        n_a[np] = o_a[j];
        int4 b = o_b[j];
        b.y &= ~RTMODT_SPEED_F_NEW;
        n_b[np] = b;
        for (int k = 0; k < W; ++k) {
            n_rxy[(size_t)k * cap + np] = o_rxy[(size_t)k * cap + j];
            n_rt[(size_t)k * cap + np] = o_rt[(size_t)k * cap + j];
        }
    }
    __syncthreads();

    // ---- 4. events, in list order (the caller's), then kind order ----
    int n_ev = 0;
    for (int base = 0; base < n; base += SP_THREADS) {
        const int p = base + tid;
        int ev = 0, i = 0, t = 0;
        if (p < n) {
            i = inv ? inv[p] : p;
            if (ppre[i + 1] != ppre[i]) { t = ppre[i]; ev = evbits[t]; }
        }
        int tot;
        int pos = n_ev + block_scan_count<SP_WAVES>(__popc(ev), wsum, tot);
        if (ev) {
            const rtmodt_speed_row r = rows[krow[t]];
            const float4 b = box[i];
            for (int k = 0; k < 3; ++k)
                if (ev >> k & 1) {
                    if (pos < a.c.max_events) {
                        rtmodt_speed_event e;
                        e.track_id = r.track_id; e.t_us = now;
                        e.xyxy[0] = b.x; e.xyxy[1] = b.y; e.xyxy[2] = b.z; e.xyxy[3] = b.w;
                        e.world[0] = r.world[0]; e.world[1] = r.world[1];
                        e.kind = k; e.value = r.speed_mm_s; e.cls = r.cls; e.track = r.track;
                        evs[pos] = e;
                    }
                    ++pos;
                }
        }
        n_ev += tot;
    }
    if (tid == 0) {
        tl_meta_write(meta, cur, tl_rows(mg), s_err);
        hdr->n_rows = n_s; hdr->n_events = n_ev; hdr->total_pairs = 0; hdr->err = (int32_t)meta[2];
    }
}

// the pairs (i < j) of the rows speed_update wrote, closer than sqrt(prox2), in (i, j) order
__global__ __launch_bounds__(SP_THREADS) void speed_pairs(SpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x, tid = threadIdx.x;
    int2 *xy = (int2 *)smem;                               // [Mc]
    int *wsum = (int *)(xy + a.Mc);                        // [SP_WAVES]
    char *blk = a.blocks + (size_t)sidx * a.block_stride;
    SpHdr *hdr = (SpHdr *)blk;
    rtmodt_speed_pair *pairs = (rtmodt_speed_pair *)(blk + a.off_pairs);
    const rtmodt_speed_row *rows = (const rtmodt_speed_row *)(blk + a.off_rows);
    int32_t *off = a.pair_off + (size_t)sidx * a.Mc;
    int n = hdr->n_rows;
    n = n < 0 ? 0 : (n > a.Mc ? a.Mc : n);
    for (int i = tid; i < n; i += SP_THREADS) xy[i] = make_int2(rows[i].world[0], rows[i].world[1]);
    __syncthreads();
    int total = 0;
    for (int base = 0; base < n; base += SP_THREADS) {
        const int i = base + tid;
        int c = 0;
        if (i < n) {
            const int2 p = xy[i];
            for (int j = i + 1; j < n; ++j) c += gp_dist2(p.x, p.y, xy[j].x, xy[j].y) < a.c.prox2 ? 1 : 0;
        }
        int tot;
        const int pos = total + block_scan_count<SP_WAVES>(c, wsum, tot);
        if (i < n) off[i] = pos;
        total += tot;
    }
    for (int i = tid; i < n; i += SP_THREADS) {            // (each thread reads back the offset it wrote itself)
        int pos = off[i];
        const int2 p = xy[i];
        for (int j = i + 1; j < n && pos < a.c.max_pairs; ++j) {
            const int64_t d2 = gp_dist2(p.x, p.y, xy[j].x, xy[j].y);
            if (d2 < a.c.prox2) {
                rtmodt_speed_pair r;
                r.track_a = rows[i].track_id; r.track_b = rows[j].track_id; r.a = i; r.b = j;
                r.dist_mm = (int32_t)gp_isqrt(d2); r.reserved = 0;
                pairs[pos++] = r;
            }
        }
    }
    if (tid == 0) hdr->total_pairs = total;
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_speed : HandleBase {
    int S = 1, Mc = 0, cap = 0;
    bool filter = false;                  // a class list was given (cfg.classes itself is not kept: the list lives on the device)
    rtmodt_speed_cfg cfg{};
    hipStream_t last_stream = nullptr;                       // the stream of the most recent launch (its own: HandleBase::stream)
    char *pool = nullptr;                 // every device array below lives in this one allocation
    SpLedger *d_ledgers = nullptr;
    std::vector<SpLedger> h_ledgers;
    int64_t *d_meta = nullptr, *d_hist = nullptr, *d_t = nullptr;
    double *d_H = nullptr;
    int32_t *d_classes = nullptr;
    int64_t *s_ids = nullptr; float4 *s_box = nullptr; int32_t *s_cls = nullptr, *s_order = nullptr, *s_inv = nullptr, *s_n = nullptr;
    int32_t *p_idx = nullptr, *oldpos = nullptr, *krow = nullptr, *evbits = nullptr, *pair_off = nullptr; int2 *wxy = nullptr;
    char *blocks = nullptr; size_t block_stride = 0, off_events = 0, off_pairs = 0, off_rows = 0;
    char *h_pin = nullptr;                // pinned mirror of the result blocks
    std::vector<char> plane_set;
    std::vector<int64_t> last_t; std::vector<char> has_t;
};

namespace {

size_t sp_carve(rtmodt_speed *z, char *base) {
    Carver c{base};
    const size_t S = z->S, cap = z->cap, Mc = z->Mc, W = z->cfg.window;
    z->d_ledgers = c.take<SpLedger>(S);
    z->d_meta = c.take<int64_t>(S * 4);
    z->d_hist = c.take<int64_t>(S * std::max(z->cfg.bins, 1));
    z->d_t = c.take<int64_t>(S);
    z->d_H = c.take<double>(S * 9);
    z->d_classes = c.take<int32_t>(std::max(z->cfg.n_classes, 1));
    if (base) z->h_ledgers.assign(S, SpLedger{});
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            SpLedger tmp{};
            tmp.id[b] = c.take<int64_t>(cap); tmp.last[b] = c.take<int64_t>(cap); tmp.odo[b] = c.take<int64_t>(cap); tmp.since[b] = c.take<int64_t>(cap);
            tmp.ring_t[b] = c.take<int64_t>(cap * W); tmp.ring_xy[b] = c.take<int2>(cap * W);
            tmp.anchor[b] = c.take<int2>(cap); tmp.chord[b] = c.take<int2>(cap); tmp.a[b] = c.take<int4>(cap); tmp.b[b] = c.take<int4>(cap);
            if (base) {
                SpLedger &L = z->h_ledgers[s];
                L.id[b] = tmp.id[b]; L.last[b] = tmp.last[b]; L.odo[b] = tmp.odo[b]; L.since[b] = tmp.since[b]; L.ring_t[b] = tmp.ring_t[b];
                L.ring_xy[b] = tmp.ring_xy[b]; L.anchor[b] = tmp.anchor[b]; L.chord[b] = tmp.chord[b]; L.a[b] = tmp.a[b]; L.b[b] = tmp.b[b];
            }
        }
    z->s_ids = c.take<int64_t>(S * Mc); z->s_box = c.take<float4>(S * Mc); z->s_cls = c.take<int32_t>(S * Mc);
    z->s_order = c.take<int32_t>(S * Mc); z->s_inv = c.take<int32_t>(S * Mc); z->s_n = c.take<int32_t>(S);
    z->p_idx = c.take<int32_t>(S * Mc); z->oldpos = c.take<int32_t>(S * Mc); z->krow = c.take<int32_t>(S * Mc);
    z->evbits = c.take<int32_t>(S * Mc); z->pair_off = c.take<int32_t>(S * Mc); z->wxy = c.take<int2>(S * Mc);
    z->off_events = 16;
    z->off_pairs = align_up(z->off_events + sizeof(rtmodt_speed_event) * z->cfg.max_events, 16);
    z->off_rows = align_up(z->off_pairs + sizeof(rtmodt_speed_pair) * z->cfg.max_pairs, 16);
    z->block_stride = align_up(z->off_rows + sizeof(rtmodt_speed_row) * Mc, 16);
    z->blocks = c.take<char>(S * z->block_stride);
    return c.size();
}

size_t sp_smem(const rtmodt_speed *z) { return 80 + (size_t)z->cap * 8 + ((size_t)z->cap + 1 + z->Mc + 1 + SP_WAVES + 1) * 4 + 32; }

SpArgs sp_args(rtmodt_speed *z) {
    SpArgs a{};
    const rtmodt_speed_cfg &c = z->cfg;
    a.c = SpCfgDev{c.anchor, c.window, c.min_samples, c.hold, c.min_step_mm, c.limit_mm_s, c.stop_mm_s, c.wrong_way_min_mm_s, c.allowed_dir[0],
                   c.allowed_dir[1], c.bins, std::max(c.bin_mm_s, 1), z->filter ? c.n_classes : 0, c.max_events, c.max_pairs, c.max_gap_us, c.stop_us,
                   (int64_t)c.proximity_mm * c.proximity_mm, z->filter ? z->d_classes : nullptr};
    a.ledgers = z->d_ledgers; a.meta = z->d_meta; a.H = z->d_H; a.hist = z->d_hist;
    a.blocks = z->blocks; a.block_stride = z->block_stride; a.off_events = z->off_events; a.off_pairs = z->off_pairs; a.off_rows = z->off_rows;
    a.cap = z->cap; a.Mc = z->Mc; a.stream_base = 0;
    a.p_idx = z->p_idx; a.oldpos = z->oldpos; a.krow = z->krow; a.evbits = z->evbits; a.pair_off = z->pair_off; a.wxy = z->wxy;
    return a;
}

int sp_check_sticky(rtmodt_speed *z, int s, int64_t err) { return ledger_check_sticky("speed", s, err, z->cap, "lower max_gap_us or raise max_tracks"); }

// every stream of [s0, s0 + cnt) has a plane and a timestamp later than its last one
int sp_check_streams(rtmodt_speed *z, int s0, int cnt, const int64_t *t_us) {
    for (int s = s0; s < s0 + cnt; ++s) {
        RT_CHECK(z->plane_set[s], RTMODT_E_INVALID, "speed stream %d: no ground plane set (rtmodt_speed_set_plane / _set_scale)", s);
        RT_CHECK(!z->has_t[s] || t_us[s - s0] > z->last_t[s], RTMODT_E_INVALID, "speed stream %d: t_us %lld is not later than the last call's %lld", s,
                 (long long)t_us[s - s0], (long long)z->last_t[s]);
    }
    return RTMODT_OK;
}

// the two launches on streams [s0, s0 + cnt), queued on q; then the result blocks, if any output is asked for
int sp_run(rtmodt_speed *z, SpArgs &a, int s0, int cnt, const int64_t *t_us, hipStream_t q, bool flat, const rtmodt_speed_out *out) {
    bool same = true;
    for (int s = 1; s < cnt; ++s) same = same && t_us[s] == t_us[0];
    if (z->last_stream && z->last_stream != q) RT_HIP(hipStreamSynchronize(z->last_stream));     // the ledger is read where the last call left it
    a.stream_base = s0;
    a.t_one = t_us[0];
    if (!same) {
        RT_HIP(hipMemcpyAsync(z->d_t + s0, t_us, sizeof(int64_t) * cnt, hipMemcpyHostToDevice, q));
        RT_HIP(hipStreamSynchronize(q));                   // the caller's array is pageable
        a.t_dev = z->d_t;
    }
    const size_t smem = sp_smem(z), smem_p = (size_t)z->Mc * 8 + SP_WAVES * 4 + 16;
    static DynLdsSeen seen, seen_p;
    RT_TRY(raise_dynamic_lds((const void *)speed_update, smem, seen));
    hipLaunchKernelGGL(speed_update, dim3(cnt), dim3(SP_THREADS), smem, q, a);
    RT_HIP(hipGetLastError());
    if (z->cfg.proximity_mm > 0) {
        RT_TRY(raise_dynamic_lds((const void *)speed_pairs, smem_p, seen_p));
        hipLaunchKernelGGL(speed_pairs, dim3(cnt), dim3(SP_THREADS), smem_p, q, a);
        RT_HIP(hipGetLastError());
    }
    z->last_stream = q;
    for (int s = 0; s < cnt; ++s) { z->last_t[s0 + s] = t_us[s]; z->has_t[s0 + s] = 1; }
    const bool any = out && (out->rows || out->n_rows || out->events || out->n_events || out->pairs || out->n_pairs || out->total_pairs);
    if (!any) return RTMODT_OK;
    const size_t o0 = (size_t)s0 * z->block_stride;
    RT_HIP(hipMemcpyAsync(z->h_pin + o0, z->blocks + o0, (size_t)cnt * z->block_stride, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    int rc = RTMODT_OK;
    for (int s = s0; s < s0 + cnt; ++s) {
        const char *blk = z->h_pin + (size_t)s * z->block_stride;
        const SpHdr h = *(const SpHdr *)blk;
        const size_t d = flat ? 0 : (size_t)s;
        const int nr = std::min(std::max(h.n_rows, 0), z->Mc), ne = std::min(std::max(h.n_events, 0), z->cfg.max_events);
        const int np = std::min(std::max(h.total_pairs, 0), z->cfg.max_pairs);
        if (out->rows && nr) memcpy(out->rows + d * z->Mc, blk + z->off_rows, sizeof(rtmodt_speed_row) * nr);
        if (out->n_rows) out->n_rows[d] = nr;
        if (out->events && ne) memcpy(out->events + d * z->cfg.max_events, blk + z->off_events, sizeof(rtmodt_speed_event) * ne);
        if (out->n_events) out->n_events[d] = ne;
        if (out->pairs && np) memcpy(out->pairs + d * z->cfg.max_pairs, blk + z->off_pairs, sizeof(rtmodt_speed_pair) * np);
        if (out->n_pairs) out->n_pairs[d] = np;
        if (out->total_pairs) out->total_pairs[d] = h.total_pairs;
        if (rc == RTMODT_OK) rc = sp_check_sticky(z, s, h.err);
        if (rc == RTMODT_OK && h.n_events > z->cfg.max_events)
            rc = fail(RTMODT_E_CAPACITY, "speed stream %d: %d events in one call > max_events %d (the first ones are delivered)", s, h.n_events,
                      z->cfg.max_events);
        if (rc == RTMODT_OK && h.total_pairs > z->cfg.max_pairs)
            rc = fail(RTMODT_E_CAPACITY, "speed stream %d: %d pairs in one call > max_pairs %d (the first ones are delivered)", s, h.total_pairs,
                      z->cfg.max_pairs);
    }
    return rc;
}

// waits for everything the handle has queued, on its own stream and on the stream of the most recent launch
int sp_sync(rtmodt_speed *z) {
    RT_HIP(hipSetDevice(z->device));
    RT_HIP(hipStreamSynchronize(z->stream));
    if (z->last_stream && z->last_stream != z->stream) RT_HIP(hipStreamSynchronize(z->last_stream));
    return RTMODT_OK;
}

// lists of streams [s0, s0 + cnt) -> the staging arrays, sorted by id with the caller's order both ways; then one call
int sp_process_lists(rtmodt_speed *z, int s0, int cnt, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n, int stride,
                     const int64_t *t_us, bool flat, const rtmodt_speed_out *out) {
    RT_TRY(sp_check_streams(z, s0, cnt, t_us));
    for (int s = 0; s < cnt; ++s) {
        RT_CHECK(n[s] >= 0 && n[s] <= stride, RTMODT_E_INVALID, "stream %d: %d tracks in rows of %d", s0 + s, n[s], stride);
        RT_CHECK(n[s] <= z->Mc, RTMODT_E_CAPACITY, "%d tracks > max_tracks %d", n[s], z->Mc);
        RT_CHECK(n[s] == 0 || (track_ids && xyxy && cls), RTMODT_E_INVALID, "null tracks");
    }
    RT_HIP(hipSetDevice(z->device));
    RT_TRY(ledger_stage_lists(LedgerStaging{z->s_ids, z->s_box, z->s_cls, z->s_order, z->s_inv, z->s_n, z->Mc}, s0, cnt, track_ids, xyxy, cls, n, stride, true,
                              z->stream));
    SpArgs a = sp_args(z);
    a.s_ids = z->s_ids; a.s_box = z->s_box; a.s_cls = z->s_cls; a.s_order = z->s_order; a.s_inv = z->s_inv; a.s_n = z->s_n;
    return sp_run(z, a, s0, cnt, t_us, z->stream, flat, out);
}

// one call on a tracker's device-resident state
template <typename T> int sp_process_tracker(rtmodt_speed *z, T *trk, int report_tsu, const int64_t *t_us, const rtmodt_speed_out *out) {
    RT_CHECK(z && trk, RTMODT_E_INVALID, "bad argument");
    SpArgs a = sp_args(z);
    TrackViewBase v;
    RT_TRY(track_src(trk, report_tsu, &a.trk, &v));
    RT_CHECK(t_us, RTMODT_E_INVALID, "null t_us");
    RT_TRY(ledger_check_view(v, z->device, z->S, z->Mc, z->Mc, "speed estimator", "speed estimator"));
    RT_TRY(sp_check_streams(z, 0, v.n_streams, t_us));
    RT_HIP(hipSetDevice(z->device));
    return sp_run(z, a, 0, v.n_streams, t_us, v.stream, false, out);      // the stream the tracker's last update ran on: ordered after it
}

}  // namespace

extern "C" {

void rtmodt_speed_destroy(rtmodt_speed *z) {
    if (!z) return;
    handle_close(z, [&] { hipFree(z->pool); hipHostFree(z->h_pin); }, z->last_stream);
    delete z;
}

int rtmodt_speed_create(int device, const rtmodt_speed_cfg *cfg, int n_streams, int max_tracks, rtmodt_speed **out) {
    RT_CHECK(out && cfg, RTMODT_E_INVALID, "null argument");
    const rtmodt_speed_cfg &c = *cfg;
    RT_CHECK(c.anchor == RTMODT_SPEED_FOOT || c.anchor == RTMODT_SPEED_CENTRE, RTMODT_E_INVALID, "anchor %d", c.anchor);
    RT_CHECK(c.window >= 2 && c.window <= SP_MAX_WINDOW && c.min_samples >= 2 && c.min_samples <= c.window, RTMODT_E_INVALID,
             "window %d (2..%d) / min_samples %d (2..window)", c.window, SP_MAX_WINDOW, c.min_samples);
    RT_CHECK(c.hold >= 1 && c.max_gap_us >= 0 && c.stop_us >= 0 && c.min_step_mm >= 0, RTMODT_E_INVALID, "hold %d / max_gap_us %lld / stop_us %lld / min_step_mm %d",
             c.hold, (long long)c.max_gap_us, (long long)c.stop_us, c.min_step_mm);
    RT_CHECK(c.limit_mm_s >= 0 && c.stop_mm_s >= 0 && c.wrong_way_min_mm_s >= 0, RTMODT_E_INVALID, "a speed threshold is negative");
    RT_CHECK(std::abs((long long)c.allowed_dir[0]) <= (1 << 20) && std::abs((long long)c.allowed_dir[1]) <= (1 << 20), RTMODT_E_INVALID,
             "allowed_dir outside [-2^20, 2^20]");
    RT_CHECK(c.bins >= 0 && c.bins <= SP_MAX_BINS && (c.bins == 0 || c.bin_mm_s >= 1), RTMODT_E_INVALID, "bins %d (0..%d) / bin_mm_s %d", c.bins, SP_MAX_BINS,
             c.bin_mm_s);
    RT_CHECK(c.proximity_mm >= 0 && c.proximity_mm <= (1 << 30), RTMODT_E_INVALID, "proximity_mm %d (0..2^30)", c.proximity_mm);
    RT_CHECK(c.max_pairs >= 1 && c.max_pairs <= (1 << 20) && c.max_events >= 1 && c.max_events <= (1 << 20), RTMODT_E_INVALID, "max_pairs %d / max_events %d",
             c.max_pairs, c.max_events);
    RT_CHECK(!c.classes || (c.n_classes >= 0 && c.n_classes <= SP_MAX_CLASSES), RTMODT_E_INVALID, "n_classes %d (0..%d)", c.n_classes, SP_MAX_CLASSES);
    RT_CHECK(n_streams >= 1 && n_streams <= 4096 && max_tracks >= 1 && max_tracks <= 4096, RTMODT_E_INVALID, "n_streams %d / max_tracks %d out of range",
             n_streams, max_tracks);
    rtmodt_speed *z = new rtmodt_speed();
    z->device = device; z->S = n_streams; z->Mc = max_tracks; z->cap = 2 * max_tracks; z->cfg = c;
    if (!c.classes) z->cfg.n_classes = 0;
    std::vector<int32_t> classes(c.classes ? c.classes : nullptr, c.classes ? c.classes + c.n_classes : nullptr);
    z->filter = c.classes != nullptr;
    z->cfg.classes = nullptr;
    z->plane_set.assign(n_streams, 0); z->last_t.assign(n_streams, 0); z->has_t.assign(n_streams, 0);
    auto body = [&]() -> int {
        RT_CHECK(sp_smem(z) <= 150 * 1024, RTMODT_E_INVALID, "speed: capacity %d needs %zu B of LDS", z->cap, sp_smem(z));
        RT_TRY(handle_open(z));
        const size_t total = sp_carve(z, nullptr);
        RT_HIP(hipMalloc((void **)&z->pool, total));
        RT_HIP(handle_zero(z->pool, total, z->stream));             // (the copies below go behind it, on the same stream)
        sp_carve(z, z->pool);
        RT_HIP(hipHostMalloc((void **)&z->h_pin, (size_t)z->S * z->block_stride, hipHostMallocDefault));
        RT_HIP(hipMemcpyAsync(z->d_ledgers, z->h_ledgers.data(), sizeof(SpLedger) * z->S, hipMemcpyHostToDevice, z->stream));
        if (!classes.empty()) RT_HIP(hipMemcpyAsync(z->d_classes, classes.data(), classes.size() * 4, hipMemcpyHostToDevice, z->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), z, rtmodt_speed_destroy, out);
}

int rtmodt_speed_set_plane(rtmodt_speed *z, int stream, const double H[9]) {
    RT_CHECK(z && H && stream >= 0 && stream < z->S, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(gp_plane_ok(H), RTMODT_E_INVALID, "speed stream %d: the plane has a non-finite entry or is singular", stream);
    RT_TRY(sp_sync(z));
    RT_HIP(hipMemcpy(z->d_H + (size_t)stream * 9, H, sizeof(double) * 9, hipMemcpyHostToDevice));
    z->plane_set[stream] = 1;
    return RTMODT_OK;
}

int rtmodt_speed_set_scale(rtmodt_speed *z, int stream, double mm_per_pixel) {
    RT_CHECK(gp_finite64(mm_per_pixel) && mm_per_pixel > 0.0, RTMODT_E_INVALID, "mm_per_pixel %g", mm_per_pixel);
    const double H[9] = {mm_per_pixel, 0, 0, 0, mm_per_pixel, 0, 0, 0, 1};
    return rtmodt_speed_set_plane(z, stream, H);
}

int rtmodt_speed_fit_plane(const double *img_xy, const double *world_xy, int n, double H_out[9], double *max_residual_mm) {
    RT_CHECK(img_xy && world_xy && H_out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(n >= 4, RTMODT_E_INVALID, "%d correspondences (at least 4)", n);
    RT_CHECK(gp_fit_plane(img_xy, world_xy, n, H_out, max_residual_mm), RTMODT_E_INVALID, "degenerate correspondences (three of four collinear, or repeated points)");
    return RTMODT_OK;
}

int rtmodt_speed_process(rtmodt_speed *z, int stream, const int64_t *track_ids, const float *xyxy, const int32_t *cls, int n, int64_t t_us,
                         const rtmodt_speed_out *out) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n >= 0, RTMODT_E_INVALID, "bad argument");
    const int32_t n32 = n;
    return sp_process_lists(z, stream, 1, track_ids, xyxy, cls, &n32, std::max(n, 1), &t_us, true, out);
}

int rtmodt_speed_process_batch(rtmodt_speed *z, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n, int stride,
                               const int64_t *t_us, const rtmodt_speed_out *out) {
    RT_CHECK(z && n && t_us && stride >= 0, RTMODT_E_INVALID, "bad argument");
    return sp_process_lists(z, 0, z->S, track_ids, xyxy, cls, n, stride, t_us, false, out);
}

int rtmodt_speed_process_tracker(rtmodt_speed *z, rtmodt_tracker *trk, const int64_t *t_us, int report_tsu, const rtmodt_speed_out *out) {
    return sp_process_tracker(z, trk, report_tsu, t_us, out);
}

int rtmodt_speed_process_deepsort(rtmodt_speed *z, rtmodt_deepsort *ds, const int64_t *t_us, int report_tsu, const rtmodt_speed_out *out) {
    return sp_process_tracker(z, ds, report_tsu, t_us, out);
}

int rtmodt_speed_process_ocsort(rtmodt_speed *z, rtmodt_ocsort *oc, const int64_t *t_us, const rtmodt_speed_out *out) {
    return sp_process_tracker(z, oc, 0, t_us, out);
}

int rtmodt_speed_process_botsort(rtmodt_speed *z, rtmodt_botsort *bot, const int64_t *t_us, const rtmodt_speed_out *out) {
    return sp_process_tracker(z, bot, 0, t_us, out);
}

int rtmodt_speed_histogram(rtmodt_speed *z, int stream, int64_t *hist, int reset) {
    RT_CHECK(z && stream >= 0 && stream < z->S, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sp_sync(z));
    const size_t B = z->cfg.bins;
    if (!B) return RTMODT_OK;
    int64_t *d = z->d_hist + (size_t)stream * B;
    if (hist) RT_HIP(hipMemcpy(hist, d, B * 8, hipMemcpyDeviceToHost));
    if (reset) RT_HIP(handle_zero(d, B * 8, z->stream));
    return handle_wait(z->stream);
}

int rtmodt_speed_state(rtmodt_speed *z, int stream, int64_t *ids, int64_t *last_t_us, int64_t *odometer_mm, int64_t *stop_since, int32_t *ring_xy,
                       int64_t *ring_t, int32_t *odo_anchor_xy, int32_t *heading, int32_t *ints, int32_t *n) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sp_sync(z));
    int64_t m[4];
    RT_HIP(hipMemcpy(m, z->d_meta + 4 * stream, sizeof(m), hipMemcpyDeviceToHost));
    RT_TRY(sp_check_sticky(z, stream, m[2]));
    const int cur = (int)m[0] & 1, cnt = (int)m[1];
    RT_CHECK(cnt >= 0 && cnt <= z->cap, RTMODT_E_INVALID, "speed stream %d: corrupt row count", stream);
    const SpLedger &L = z->h_ledgers[stream];
    *n = cnt;
    if (!cnt) return RTMODT_OK;
    const size_t c = (size_t)cnt, cap = z->cap, W = z->cfg.window;
    if (ids) RT_HIP(hipMemcpy(ids, L.id[cur], c * 8, hipMemcpyDeviceToHost));
    if (last_t_us) RT_HIP(hipMemcpy(last_t_us, L.last[cur], c * 8, hipMemcpyDeviceToHost));
    if (odometer_mm) RT_HIP(hipMemcpy(odometer_mm, L.odo[cur], c * 8, hipMemcpyDeviceToHost));
    if (stop_since) RT_HIP(hipMemcpy(stop_since, L.since[cur], c * 8, hipMemcpyDeviceToHost));
    if (odo_anchor_xy) RT_HIP(hipMemcpy(odo_anchor_xy, L.anchor[cur], c * 8, hipMemcpyDeviceToHost));
    if (heading) RT_HIP(hipMemcpy(heading, L.chord[cur], c * 8, hipMemcpyDeviceToHost));
    if (ints) {
        std::vector<int4> va(c), vb(c);
        RT_HIP(hipMemcpy(va.data(), L.a[cur], c * 16, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(vb.data(), L.b[cur], c * 16, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < c; ++r) {
            const int32_t v[8] = {va[r].x, va[r].y, va[r].z, va[r].w, vb[r].x, vb[r].y, vb[r].z, vb[r].w};
            memcpy(ints + 8 * r, v, sizeof(v));
        }
    }
    if (ring_xy || ring_t) {                               // stored [window][cap]: handed out [row][window]
        std::vector<int2> xy(W * cap);
        std::vector<int64_t> tt(W * cap);
        RT_HIP(hipMemcpy(xy.data(), L.ring_xy[cur], W * cap * 8, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(tt.data(), L.ring_t[cur], W * cap * 8, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < c; ++r)
            for (size_t k = 0; k < W; ++k) {
                if (ring_xy) { ring_xy[(r * W + k) * 2] = xy[k * cap + r].x; ring_xy[(r * W + k) * 2 + 1] = xy[k * cap + r].y; }
                if (ring_t) ring_t[r * W + k] = tt[k * cap + r];
            }
    }
    return RTMODT_OK;
}

}  // extern "C"
