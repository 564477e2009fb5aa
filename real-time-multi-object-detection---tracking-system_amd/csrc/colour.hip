// colour.hip -- the colour names of every track, kept in device memory: on a track list the host hands over or straight on the
// device-resident state of the four trackers.  colour_rule.h states the per-pixel and per-box rules (name, sampled rectangle, grid,
// parts, occluders, accumulation, ageing, label) and include/rtmodt.h the ledger rules; tests/colour_ref.py restates both and the
// kernels equal it exactly.  TWO launches per call for all streams, whatever the tracks do, with no host read-back between them:
//   cl_sample   a grid of (max_tracks, streams) 256-thread workgroups; the workgroup of an entry past its list, not selected by the
//               tracker or not sampled leaves at once.  Every thread computes the entry's plan (it is uniform); the workgroup then
//               sweeps the list for the entry's occluders, compacted in list order by workgroup prefix sums (no atomic decides an
//               index), keeps the first CL_MAX_OCCLUDERS clipped rectangles in LDS, and walks the sample grid with consecutive
//               lanes on consecutive samples of a row: three byte loads, the name, one integer LDS add into the wave's own 2 x 12
//               counters.  The four waves' counters are summed into the entry's frame histogram.
//   cl_merge    one 256-thread workgroup per stream.  Per stream a LEDGER, rows sorted by track id, double-buffered, built as
//               snapshot.hip builds its own by the steps of track_ledger_dev.h: the sampled entries are compacted by a prefix sum,
//               each finds its old row by binary search (old ids staged in LDS), idle rows are merged by rank (no sort), rows
//               past retire_after leave through the `retired` list with their final label.  One thread owns one member's row:
//               accumulation, ageing, labels.  Every loop strides over the workgroup, so a list longer than 256 works.
// No floats after pv_coord, no atomics on the ledger.  Results of one stream lie in one block {header, updated, retired}; the
// blocks of the streams a call touched come back in one copy, and only when an output was asked for.
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
#include "colour_rule.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_select_dev.h"
#include "track_ledger_dev.h"

constexpr int CL_THREADS = 256, CL_WAVES = CL_THREADS / 64;

static_assert(sizeof(rtmodt_colour_row) == 208 && sizeof(rtmodt_colour_label) == sizeof(ClLabel), "rtmodt_colour_row drifted");
static_assert(RTMODT_COLOUR_NAMES == CL_NAMES && RTMODT_COLOUR_F_NEW == CL_F_NEW && RTMODT_COLOUR_F_MANY_OCCLUDERS == CL_F_MANY_OCCLUDERS &&
              RTMODT_COLOUR_F_THIN == CL_F_THIN, "include/rtmodt.h and colour_rule.h disagree");

struct ClLedger {                  // one stream, double-buffered
    int64_t *id[2], *first[2], *last[2];
    uint32_t *hist[2];             // [cap][CL_BINS]
    int4 *ints[2];                 // {cls, frames_used, flags, 0}
};

struct ClHdr { int32_t n_updated, n_retired, err, pad; };

struct ClFrame { const uint8_t *p; int64_t frame_id; };

struct ClArgs {
    ClRuleCfg c;
    int32_t retire_after;
    ClLedger *ledgers;             // [n_streams]
    int64_t *meta;                 // [n_streams][4]: cur, rows, sticky err, 0
    char *blocks; size_t block_stride, off_updated, off_retired;      // per stream: ClHdr | updated [Mc] | retired [cap]
    int cap, Mc, stream_base;
    const ClFrame *frames;         // [streams of this call] (index: stream - stream_base)
    int fh, fw; int64_t fpitch;
    // source A: a staged list [cnt][Mc], sorted by id; order = the caller's index of a sorted entry, inv = its inverse
    const int64_t *s_ids; const float4 *s_box; const int32_t *s_cls; const int32_t *s_order, *s_inv; const int32_t *s_n;
    // sources B..E: a tracker's device state (track_select_dev.h)
    TrackSrc trk;
    // per-stream scratch [n_streams][Mc]
    uint32_t *fhist;               // [..][CL_BINS] the frame histogram of a member, written by cl_sample
    int32_t *fflags, *p_idx, *oldpos, *krow;
};

// this call's list of the stream blockIdx `b` of the call names
__device__ __forceinline__ TrackSel cl_list(const ClArgs &a, int b, const int32_t **order, const int32_t **inv) {
    if (a.s_ids) {
        const size_t o = (size_t)b * a.Mc;
        if (order) *order = a.s_order + o;
        if (inv) *inv = a.s_inv + o;
        return select_list(a.s_ids + o, a.s_box + o, a.s_cls + o, a.s_n[b]);
    }
    return select_tracks(a.trk, a.stream_base + b);
}

__device__ __forceinline__ bool cl_entry_plan(const ClArgs &a, const TrackSel &src, int i, ClPlan &P) {
    if (!selected(src, i)) return false;
    const float4 b = src.box[i];
    return cl_plan(a.c, b.x, b.y, b.z, b.w, src.cls[i], a.fh, a.fw, P);
}

// --------------------------------------------------------------------------------------------------------------------- sampler
__global__ __launch_bounds__(CL_THREADS) void cl_sample(ClArgs a) {
    __shared__ int wsum[CL_WAVES];
    __shared__ PvRect occ[CL_MAX_OCCLUDERS];
    __shared__ uint32_t cnt[CL_WAVES * CL_BINS];
    const int e = blockIdx.x, sidx = a.stream_base + blockIdx.y, tid = threadIdx.x;
    const TrackSel src = cl_list(a, blockIdx.y, nullptr, nullptr);
    const int n = src.n < 0 ? 0 : (src.n > a.Mc ? a.Mc : src.n);      // the host refuses a source whose max_tracks exceeds Mc
    ClPlan P;
    if (e >= n || !cl_entry_plan(a, src, e, P)) return;               // (uniform over the workgroup: no barrier is skipped by a part of it)

    // ---- the occluders, in list order ----
    int n_occ = 0;
    if (a.c.skip_occluded && !cl_empty(P.rect)) {
        const int64_t my_id = src.ids[e];
        for (int base = 0; base < n; base += CL_THREADS) {
            const int k = base + tid;
            bool f = false;
            ClPlan Q;
            if (k < n && k != e && cl_entry_plan(a, src, k, Q)) f = cl_occludes(P, my_id, Q.raw, Q.box, src.ids[k]);
            int tot;
            const int pos = n_occ + block_scan_count<CL_WAVES>(f ? 1 : 0, wsum, tot);
            if (f && pos < CL_MAX_OCCLUDERS) occ[pos] = Q.box;
            n_occ += tot;
        }
    }
    for (int i = tid; i < CL_WAVES * CL_BINS; i += CL_THREADS) cnt[i] = 0;
    __syncthreads();

    // ---- the sample grid: consecutive lanes on consecutive samples of a row ----
    const int used = n_occ < CL_MAX_OCCLUDERS ? n_occ : CL_MAX_OCCLUDERS;
    const uint8_t *frame = a.frames[blockIdx.y].p;
    const int total = P.nx * P.ny;                                    // <= CL_MAX_SIDE^2
    uint32_t *mine = cnt + (tid >> 6) * CL_BINS;
    for (int s = tid; s < total; s += CL_THREADS) {
        const int j = s / P.nx, i = s - j * P.nx;
        const int x = P.rect.x0 + i * P.sx, y = P.rect.y0 + j * P.sy; // inside rect, and rect inside the frame
        bool hidden = false;
        for (int o = 0; o < used; ++o) hidden = hidden || cl_inside(occ[o], x, y);
        if (hidden) continue;
        const uint8_t *px = frame + (size_t)y * (size_t)a.fpitch + (size_t)3 * x;
        const int name = cl_name(a.c, px[0], px[1], px[2]);
        atomicAdd(&mine[cl_part(P, y) * CL_NAMES + name], 1u);
    }
    __syncthreads();
    const size_t slot = (size_t)sidx * a.Mc + e;
    if (tid < CL_BINS) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < CL_WAVES; ++w) v += cnt[w * CL_BINS + tid];
        a.fhist[slot * CL_BINS + tid] = v;
    }
    if (tid == 0) a.fflags[slot] = n_occ > CL_MAX_OCCLUDERS ? CL_F_MANY_OCCLUDERS : 0;
}

// ----------------------------------------------------------------------------------------------------------------------- ledger
__device__ __forceinline__ void cl_fill_row(rtmodt_colour_row &r, int64_t id, int64_t first, int64_t last, const uint32_t *hist, int cls, int used, int flags,
                                            int track, int frame_samples) {
    r.track_id = id; r.first_frame = first; r.last_frame = last;
#pragma unroll
    for (int k = 0; k < CL_BINS; ++k) r.hist[k / CL_NAMES][k % CL_NAMES] = hist[k];
    r.cls = cls; r.frames_used = used; r.flags = flags; r.track = track; r.frame_samples = frame_samples; r.reserved[0] = r.reserved[1] = 0;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const ClLabel L = cl_label(hist, p);
        r.label[p].name = L.name; r.label[p].share_pm = L.share_pm; r.label[p].second = L.second; r.label[p].second_pm = L.second_pm;
        r.label[p].samples = L.samples;
    }
}

__global__ __launch_bounds__(CL_THREADS) void cl_merge(ClArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x, tid = threadIdx.x;
    const int cap = a.cap, Mc = a.Mc;
    int64_t *old_id = (int64_t *)smem;                    // [cap]
    int *ret_pre = (int *)(old_id + cap);                 // [cap + 1] class of an old row, then the idle rows' rank encoding (track_ledger.h)
    int *ppre = ret_pre + cap + 1;                        // [Mc + 1] exclusive prefix of the list's member flags
    int *wsum = ppre + Mc + 1;                            // [CL_WAVES]
    int *s_err = wsum + CL_WAVES;                         // [1]

    int64_t *meta = a.meta + (size_t)sidx * 4;
    const int cur = tl_meta_cur(meta), nxt = cur ^ 1, n_old = tl_meta_rows(meta, cap);
    const ClLedger *Lp = a.ledgers + sidx;
    const int64_t *o_id = Lp->id[cur], *o_first = Lp->first[cur], *o_last = Lp->last[cur];
    const uint32_t *o_hist = Lp->hist[cur]; const int4 *o_ints = Lp->ints[cur];
    int64_t *n_id = Lp->id[nxt], *n_first = Lp->first[nxt], *n_last = Lp->last[nxt];
    uint32_t *n_hist = Lp->hist[nxt]; int4 *n_ints = Lp->ints[nxt];
    const int64_t fid = a.frames[blockIdx.x].frame_id;

    const int32_t *order = nullptr, *inv = nullptr;
    const TrackSel src = cl_list(a, blockIdx.x, &order, &inv);
    const int n = src.n < 0 ? 0 : (src.n > Mc ? Mc : src.n);
    const int64_t *ids = src.ids; const int32_t *cls = src.cls;

    if (tid == 0) *s_err = 0;
    // 2: retired by this call; 1: idle unless a member claims it (0)
    ledger_stage_old<CL_THREADS>(o_id, n_old, old_id, ret_pre, [&](int j) { return fid - o_last[j] > (int64_t)a.retire_after ? 2 : 1; });
    __syncthreads();

    const size_t so = (size_t)sidx * Mc;
    int32_t *p_idx = a.p_idx + so, *oldpos = a.oldpos + so, *krow = a.krow + so;
    const int32_t *fflags = a.fflags + so;
    const uint32_t *fhist = a.fhist + so * CL_BINS;
    char *blk = a.blocks + (size_t)sidx * a.block_stride;
    ClHdr *hdr = (ClHdr *)blk;
    rtmodt_colour_row *upd = (rtmodt_colour_row *)(blk + a.off_updated);
    rtmodt_colour_row *rtd = (rtmodt_colour_row *)(blk + a.off_retired);

    // ---- 1. the members (exactly the entries cl_sample wrote a frame histogram for), compacted in list order ----
    const int n_s = ledger_compact<CL_THREADS>(n, ppre, p_idx, wsum, [&](int i) { ClPlan P; return cl_entry_plan(a, src, i, P); });
    const bool ascending = ledger_list_ascends<CL_THREADS>(ids, n, s_err);

    // ---- 2. every member's old row; a row past retire_after is not this track's row any more ----
    for (int t = tid; t < n_s; t += CL_THREADS) {
        const int j = tl_match(old_id, n_old, ids[p_idx[t]]);
        const bool live = j >= 0 && ret_pre[j] == 1;                            // (ids are unique: no other thread touches ret_pre[j])
        oldpos[t] = live ? j : -1;
        if (live) ret_pre[j] = 0;
    }
    __syncthreads();

    // ---- 3. the old rows: idle ranks (in place), and the retired rows leave in id order with their final label ----
    int n_idle = 0, n_rtd = 0;
    for (int base = 0; base < n_old; base += CL_THREADS) {
        const int j = base + tid;
        const int c = j < n_old ? ret_pre[j] : 0;
        int tot_i, tot_r;
        const int pos_i = block_scan_count<CL_WAVES>(c == 1 ? 1 : 0, wsum, tot_i);
        const int pos_r = block_scan_count<CL_WAVES>(c == 2 ? 1 : 0, wsum, tot_r);
        if (j < n_old) ret_pre[j] = tl_rank_encode(c == 1, n_idle + pos_i);
        if (c == 2) {                                                           // (n_rtd + pos_r < n_old <= cap: the list holds cap rows)
            const int4 v = o_ints[j];
            rtmodt_colour_row r;
            cl_fill_row(r, old_id[j], o_first[j], o_last[j], o_hist + (size_t)j * CL_BINS, v.x, v.y, v.z & ~CL_F_NEW, -1, 0);
            rtd[n_rtd + pos_r] = r;
        }
        n_idle += tot_i; n_rtd += tot_r;
    }
    if (tid == 0) ret_pre[n_old] = tl_rank_encode(false, n_idle);

    // ---- 4. the place of each member in `updated`: the caller's list order (a tracker's list: its own order) ----
    for (int base = 0, run = 0; base < n; base += CL_THREADS) {
        const int p = base + tid;
        int i = 0;
        bool f = false;
        if (p < n) { i = inv ? inv[p] : p; f = ppre[i + 1] != ppre[i]; }
        int tot;
        const int pos = run + block_scan_count<CL_WAVES>(f ? 1 : 0, wsum, tot);
        if (f) krow[ppre[i]] = pos;
        run += tot;
    }
    __syncthreads();
    const TlMerge mg = ledger_decide(ids, ppre, n, old_id, ret_pre, n_old, n_s, n_idle, ascending, cap, s_err);

    // ---- 5. one thread per member: its row and its entry of `updated` ----
    for (int t = tid; t < n_s; t += CL_THREADS) {
        const int i = p_idx[t], j = oldpos[t];
        const int64_t id = ids[i];
        const int np = tl_member_pos(mg, t, id);
        uint32_t row[CL_BINS], fh[CL_BINS];
        uint32_t fs = 0;
#pragma unroll
        for (int k = 0; k < CL_BINS; ++k) {
            row[k] = j >= 0 ? o_hist[(size_t)j * CL_BINS + k] : 0u;
            fh[k] = fhist[(size_t)i * CL_BINS + k];
            fs += fh[k];
        }
        const bool added = cl_accumulate(row, fh, a.c.min_samples);
        const int flags = fflags[i] | (j < 0 ? CL_F_NEW : 0) | (added ? 0 : CL_F_THIN);
        const int used = (j >= 0 ? o_ints[j].y : 0) + (added ? 1 : 0);
        const int64_t first = j >= 0 ? o_first[j] : fid;
        n_id[np] = id; n_first[np] = first; n_last[np] = fid;
#pragma unroll
        for (int k = 0; k < CL_BINS; ++k) n_hist[(size_t)np * CL_BINS + k] = row[k];
        n_ints[np] = make_int4(cls[i], used, flags, 0);
        int kr = krow[t];
        kr = kr < 0 ? 0 : (kr >= Mc ? Mc - 1 : kr);
        rtmodt_colour_row r;
        cl_fill_row(r, id, first, fid, row, cls[i], used, flags, order ? order[i] : i, (int)fs);
        upd[kr] = r;
    }
    // ---- 6. idle rows move to their merged position; NEW is this call's, so it goes ----
    for (int j = tid; j < n_old; j += CL_THREADS) {
        const int np = tl_idle_pos(mg, j);
        if (np < 0) continue;
        n_id[np] = old_id[j]; n_first[np] = o_first[j]; n_last[np] = o_last[j];
        for (int k = 0; k < CL_BINS; ++k) n_hist[(size_t)np * CL_BINS + k] = o_hist[(size_t)j * CL_BINS + k];
        int4 v = o_ints[j];
        v.z &= ~CL_F_NEW;
        n_ints[np] = v;
    }
    __syncthreads();
    if (tid == 0) {
        tl_meta_write(meta, cur, tl_rows(mg), *s_err);
        hdr->n_updated = n_s; hdr->n_retired = n_rtd; hdr->err = (int32_t)meta[2]; hdr->pad = 0;
    }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_colour : HandleBase {
    int S = 1, Mc = 0, cap = 0;
    bool filter = false;                  // a class list was given (the list lives on the device)
    rtmodt_colour_cfg cfg{};
    hipStream_t last_stream = nullptr;                       // the stream of the most recent launch (its own: HandleBase::stream)
    EventTimer<2> timer;
    char *pool = nullptr;                 // every device array lives in this one allocation
    ClLedger *d_ledgers = nullptr;
    std::vector<ClLedger> h_ledgers;
    int64_t *d_meta = nullptr; int32_t *d_classes = nullptr;
    uint32_t *fhist = nullptr; int32_t *fflags = nullptr, *p_idx = nullptr, *oldpos = nullptr, *krow = nullptr;
    char *blocks = nullptr; size_t block_stride = 0, off_updated = 0, off_retired = 0;
    char *h_pin = nullptr;                // pinned mirror of the result blocks
    // the command block of a call (frames, frame ids, a host list) goes out in one copy from one of two pinned buffers: a call that
    // asks for no output does not wait, so the buffer the call before it wrote may still be in flight
    CmdBuf cmd[2]; hipEvent_t cmd_ev[2] = {nullptr, nullptr}; bool cmd_busy[2] = {false, false}; int cmd_i = 0;
    FrameStage stage;
    std::vector<int64_t> last_f; std::vector<char> has_f;
};

namespace {

ClRuleCfg cl_rule_of(const rtmodt_colour_cfg &c, const int32_t *classes, int n_classes) {
    ClRuleCfg r{};
    r.black_max = c.black_max; r.chroma_min = c.chroma_min; r.sat_split = c.sat_split; r.sat_hi_pm = c.sat_hi_pm; r.sat_lo_pm = c.sat_lo_pm;
    r.y_black = c.y_black; r.y_white = c.y_white;
    for (int k = 0; k < CL_HUE_BOUNDS; ++k) r.hue[k] = c.hue[k];
    r.pink_mx = c.pink_mx; r.red_brown_mx = c.red_brown_mx; r.orange_brown_mx = c.orange_brown_mx; r.yellow_brown_mx = c.yellow_brown_mx;
    r.inset_x_pm = c.inset_x_pm; r.top_pm = c.top_pm; r.split_pm = c.split_pm; r.bottom_pm = c.bottom_pm; r.max_side = c.max_side;
    r.skip_occluded = c.skip_occluded; r.min_samples = c.min_samples; r.classes = classes; r.n_classes = n_classes;
    return r;
}

int cl_check_cfg(const rtmodt_colour_cfg &c) {
    RT_CHECK(c.black_max >= 0 && c.black_max <= 256 && c.chroma_min >= 0 && c.chroma_min <= 256 && c.sat_split >= 0 && c.sat_split <= 256, RTMODT_E_INVALID,
             "black_max %d / chroma_min %d / sat_split %d (0..256 each)", c.black_max, c.chroma_min, c.sat_split);
    RT_CHECK(c.sat_hi_pm >= 0 && c.sat_hi_pm <= 1000 && c.sat_lo_pm >= 0 && c.sat_lo_pm <= 1000, RTMODT_E_INVALID, "sat_hi_pm %d / sat_lo_pm %d (0..1000)",
             c.sat_hi_pm, c.sat_lo_pm);
    RT_CHECK(c.y_black >= 0 && c.y_black <= c.y_white && c.y_white <= 256, RTMODT_E_INVALID, "y_black %d / y_white %d (0 <= y_black <= y_white <= 256)", c.y_black,
             c.y_white);
    for (int k = 0; k < CL_HUE_BOUNDS; ++k)
        RT_CHECK(c.hue[k] >= (k ? c.hue[k - 1] : 0) && c.hue[k] <= CL_HUE_STEPS, RTMODT_E_INVALID, "hue[%d] %d: the bounds ascend within 0..%d", k, c.hue[k],
                 CL_HUE_STEPS);
    RT_CHECK(c.pink_mx >= 0 && c.pink_mx <= 256 && c.red_brown_mx >= 0 && c.red_brown_mx <= 256 && c.orange_brown_mx >= 0 && c.orange_brown_mx <= 256 &&
                 c.yellow_brown_mx >= 0 && c.yellow_brown_mx <= 256,
             RTMODT_E_INVALID, "pink_mx %d / red_brown_mx %d / orange_brown_mx %d / yellow_brown_mx %d (0..256 each)", c.pink_mx, c.red_brown_mx, c.orange_brown_mx,
             c.yellow_brown_mx);
    RT_CHECK(c.inset_x_pm >= 0 && c.inset_x_pm <= 499, RTMODT_E_INVALID, "inset_x_pm %d (0..499)", c.inset_x_pm);
    RT_CHECK(c.top_pm >= 0 && c.top_pm < c.split_pm && c.split_pm < c.bottom_pm && c.bottom_pm <= 1000, RTMODT_E_INVALID,
             "top_pm %d / split_pm %d / bottom_pm %d (0 <= top < split < bottom <= 1000)", c.top_pm, c.split_pm, c.bottom_pm);
    RT_CHECK(c.max_side >= 1 && c.max_side <= CL_MAX_SIDE, RTMODT_E_INVALID, "max_side %d (1..%d)", c.max_side, CL_MAX_SIDE);
    RT_CHECK(c.skip_occluded == 0 || c.skip_occluded == 1, RTMODT_E_INVALID, "skip_occluded %d (0 or 1)", c.skip_occluded);
    RT_CHECK(c.min_samples >= 0 && c.min_samples <= CL_MAX_SIDE * CL_MAX_SIDE, RTMODT_E_INVALID, "min_samples %d (0..%d)", c.min_samples, CL_MAX_SIDE * CL_MAX_SIDE);
    RT_CHECK(c.retire_after >= 0, RTMODT_E_INVALID, "retire_after %d", c.retire_after);
    RT_CHECK(!c.classes || (c.n_classes >= 0 && c.n_classes <= CL_MAX_CLASSES), RTMODT_E_INVALID, "n_classes %d (0..%d)", c.n_classes, CL_MAX_CLASSES);
    return RTMODT_OK;
}

size_t cl_carve(rtmodt_colour *z, char *base) {
    Carver c{base};
    const size_t S = z->S, cap = z->cap, Mc = z->Mc;
    z->d_ledgers = c.take<ClLedger>(S);
    z->d_meta = c.take<int64_t>(S * 4);
    z->d_classes = c.take<int32_t>(std::max(z->cfg.n_classes, 1));
    if (base) z->h_ledgers.assign(S, ClLedger{});
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            ClLedger tmp{};
            tmp.id[b] = c.take<int64_t>(cap); tmp.first[b] = c.take<int64_t>(cap); tmp.last[b] = c.take<int64_t>(cap);
            tmp.hist[b] = c.take<uint32_t>(cap * CL_BINS); tmp.ints[b] = c.take<int4>(cap);
            if (base) {
                ClLedger &L = z->h_ledgers[s];
                L.id[b] = tmp.id[b]; L.first[b] = tmp.first[b]; L.last[b] = tmp.last[b]; L.hist[b] = tmp.hist[b]; L.ints[b] = tmp.ints[b];
            }
        }
    z->fhist = c.take<uint32_t>(S * Mc * CL_BINS); z->fflags = c.take<int32_t>(S * Mc);
    z->p_idx = c.take<int32_t>(S * Mc); z->oldpos = c.take<int32_t>(S * Mc); z->krow = c.take<int32_t>(S * Mc);
    z->off_updated = sizeof(ClHdr);
    z->off_retired = align_up(z->off_updated + sizeof(rtmodt_colour_row) * Mc, 16);
    z->block_stride = align_up(z->off_retired + sizeof(rtmodt_colour_row) * cap, 16);
    z->blocks = c.take<char>(S * z->block_stride);
    return c.size();
}

size_t cl_smem(const rtmodt_colour *z) { return (size_t)z->cap * 8 + ((size_t)z->cap + 1 + z->Mc + 1 + CL_WAVES + 1) * 4 + 32; }

ClArgs cl_args(rtmodt_colour *z) {
    ClArgs a{};
    a.c = cl_rule_of(z->cfg, z->filter ? z->d_classes : nullptr, z->filter ? z->cfg.n_classes : 0);
    a.retire_after = z->cfg.retire_after;
    a.ledgers = z->d_ledgers; a.meta = z->d_meta;
    a.blocks = z->blocks; a.block_stride = z->block_stride; a.off_updated = z->off_updated; a.off_retired = z->off_retired;
    a.cap = z->cap; a.Mc = z->Mc;
    a.fhist = z->fhist; a.fflags = z->fflags; a.p_idx = z->p_idx; a.oldpos = z->oldpos; a.krow = z->krow;
    return a;
}

// every stream of [s0, s0 + cnt) gets a frame id later than its last one
int cl_check_ids(rtmodt_colour *z, int s0, int cnt, const int64_t *frame_id) {
    for (int s = s0; s < s0 + cnt; ++s)
        RT_CHECK(!z->has_f[s] || frame_id[s - s0] > z->last_f[s], RTMODT_E_INVALID, "colour stream %d: frame_id %lld is not later than the last call's %lld", s,
                 (long long)frame_id[s - s0], (long long)z->last_f[s]);
    return RTMODT_OK;
}

// the pinned buffer of this call, idle again; `bytes` large
int cl_cmd(rtmodt_colour *z, size_t bytes, CmdBuf **out) {
    const int k = z->cmd_i;
    if (z->cmd_busy[k]) { RT_HIP(hipEventSynchronize(z->cmd_ev[k])); z->cmd_busy[k] = false; }
    RT_TRY(z->cmd[k].reserve(bytes));                      // (a regrow waits for the device itself before it frees)
    *out = &z->cmd[k];
    return RTMODT_OK;
}
int cl_cmd_send(rtmodt_colour *z, CmdBuf *cb, size_t bytes, hipStream_t q) {
    const int k = z->cmd_i;
    RT_HIP(hipMemcpyAsync(cb->d, cb->h, bytes, hipMemcpyHostToDevice, q));
    RT_HIP(hipEventRecord(z->cmd_ev[k], q));
    z->cmd_busy[k] = true;
    z->cmd_i = k ^ 1;
    return RTMODT_OK;
}

int cl_check_sticky(rtmodt_colour *z, int s, long long err) { return ledger_check_sticky("colour", s, err, z->cap, "lower retire_after or raise max_tracks"); }

// the two launches on streams [s0, s0 + cnt), queued on q; then the result blocks, if any output is asked for
int cl_run(rtmodt_colour *z, ClArgs &a, int s0, int cnt, const int64_t *frame_id, hipStream_t q, bool flat, const rtmodt_colour_out *out) {
    a.stream_base = s0;
    const size_t smem = cl_smem(z);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)cl_merge, smem, seen));
    RT_TRY(z->timer.record(0, q));
    hipLaunchKernelGGL(cl_sample, dim3(z->Mc, cnt), dim3(CL_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cl_merge, dim3(cnt), dim3(CL_THREADS), smem, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(z->timer.record(1, q));
    z->timer.timed = true;
    z->last_stream = q;
    for (int s = 0; s < cnt; ++s) { z->last_f[s0 + s] = frame_id[s]; z->has_f[s0 + s] = 1; }
    const bool any = out && (out->updated || out->n_updated || out->retired || out->n_retired);
    if (!any) return RTMODT_OK;
    const size_t o0 = (size_t)s0 * z->block_stride;
    RT_HIP(hipMemcpyAsync(z->h_pin + o0, z->blocks + o0, (size_t)cnt * z->block_stride, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    int rc = RTMODT_OK;
    for (int s = s0; s < s0 + cnt; ++s) {
        const char *blk = z->h_pin + (size_t)s * z->block_stride;
        const ClHdr h = *(const ClHdr *)blk;
        const size_t d = flat ? 0 : (size_t)s;
        const int nu = std::min(std::max(h.n_updated, 0), z->Mc), nr = std::min(std::max(h.n_retired, 0), z->cap);
        if (out->updated && nu) memcpy(out->updated + d * z->Mc, blk + z->off_updated, sizeof(rtmodt_colour_row) * nu);
        if (out->n_updated) out->n_updated[d] = nu;
        if (out->retired && nr) memcpy(out->retired + d * z->cap, blk + z->off_retired, sizeof(rtmodt_colour_row) * nr);
        if (out->n_retired) out->n_retired[d] = nr;
        if (rc == RTMODT_OK) rc = cl_check_sticky(z, s, h.err);
    }
    return rc;
}

// waits for everything the handle has queued, on its own stream and on the stream of the most recent launch
int cl_sync(rtmodt_colour *z) {
    RT_HIP(hipSetDevice(z->device));
    RT_HIP(hipStreamSynchronize(z->stream));
    if (z->last_stream && z->last_stream != z->stream) RT_HIP(hipStreamSynchronize(z->last_stream));
    return RTMODT_OK;
}

// the ledger and the staged frames are read where the last call left them
int cl_order_after_last(rtmodt_colour *z, hipStream_t q) {
    if (z->last_stream && z->last_stream != q) RT_HIP(hipStreamSynchronize(z->last_stream));
    return RTMODT_OK;
}

int cl_check_frame_args(const uint8_t *const *frames, int n, int fh, int fw, int stride_bytes, int mem_kind) {
    RT_CHECK(frames, RTMODT_E_INVALID, "null frames");
    return check_frames(frames, n, fh, fw, stride_bytes, mem_kind, kSnapFrames);
}

// frames (staged when they are the host's) and frame ids of the call's streams -> the head of the command block
int cl_fill_frames(rtmodt_colour *z, ClFrame *F, const uint8_t *const *frames, int cnt, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id) {
    RT_TRY(z->stage.place(cnt, fh, fw, stride_bytes, mem_kind, FRAMES_AS_GIVEN));
    for (int i = 0; i < cnt; ++i) { F[i].p = z->stage.at(frames, i); F[i].frame_id = frame_id[i]; }
    return RTMODT_OK;
}

// lists of streams [s0, s0 + cnt) -> the command block, sorted by id with the caller's order both ways; then one call
int cl_process_lists(rtmodt_colour *z, int s0, int cnt, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n, int stride,
                     const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id, bool flat, const rtmodt_colour_out *out) {
    RT_CHECK(frame_id, RTMODT_E_INVALID, "null frame_id");
    RT_TRY(cl_check_frame_args(frames, cnt, fh, fw, stride_bytes, mem_kind));
    RT_TRY(cl_check_ids(z, s0, cnt, frame_id));
    for (int s = 0; s < cnt; ++s) {
        RT_CHECK(n[s] >= 0 && n[s] <= stride, RTMODT_E_INVALID, "stream %d: %d tracks in rows of %d", s0 + s, n[s], stride);
        RT_CHECK(n[s] <= z->Mc, RTMODT_E_CAPACITY, "%d tracks > max_tracks %d", n[s], z->Mc);
        RT_CHECK(n[s] == 0 || (track_ids && xyxy && cls), RTMODT_E_INVALID, "null tracks");
    }
    RT_HIP(hipSetDevice(z->device));
    const size_t Mc = z->Mc, m = (size_t)cnt * Mc;
    const size_t o_ids = align_up(sizeof(ClFrame) * cnt, 16), o_box = o_ids + m * 8, o_cls = o_box + m * 16, o_ord = o_cls + m * 4, o_inv = o_ord + m * 4,
                 o_n = o_inv + m * 4, bytes = align_up(o_n + (size_t)cnt * 4, 16);
    CmdBuf *cb;
    RT_TRY(cl_cmd(z, bytes, &cb));
    memset(cb->h, 0, bytes);
    int64_t *ids = (int64_t *)(cb->h + o_ids); float4 *box = (float4 *)(cb->h + o_box);
    int32_t *kc = (int32_t *)(cb->h + o_cls), *perm = (int32_t *)(cb->h + o_ord), *inv = (int32_t *)(cb->h + o_inv), *nn = (int32_t *)(cb->h + o_n);
    for (int s = 0; s < cnt; ++s) {
        const int64_t *ti = track_ids + (size_t)s * stride;
        const float *tb = xyxy + (size_t)s * stride * 4;
        const int32_t *tc = cls + (size_t)s * stride;
        int32_t *pm = perm + s * Mc, *iv = inv + s * Mc;
        nn[s] = n[s];
        const int dup = tl_sort_list(ti, n[s], pm, iv);
        RT_CHECK(dup < 0, RTMODT_E_INVALID, "stream %d: track id %lld appears twice", s0 + s, (long long)ti[pm[dup]]);
        for (int i = 0; i < n[s]; ++i) {
            const int p = pm[i];
            ids[s * Mc + i] = ti[p]; kc[s * Mc + i] = tc[p];
            box[s * Mc + i] = make_float4(tb[4 * p], tb[4 * p + 1], tb[4 * p + 2], tb[4 * p + 3]);
        }
    }
    hipStream_t q = z->stream;
    RT_TRY(cl_order_after_last(z, q));
    RT_TRY(cl_fill_frames(z, (ClFrame *)cb->h, frames, cnt, fh, fw, stride_bytes, mem_kind, frame_id));
    RT_TRY(z->stage.copy_in(frames, q));
    RT_TRY(cl_cmd_send(z, cb, bytes, q));
    ClArgs a = cl_args(z);
    a.frames = (const ClFrame *)cb->d; a.fh = fh; a.fw = fw; a.fpitch = (int64_t)z->stage.pitch;
    a.s_ids = (const int64_t *)(cb->d + o_ids); a.s_box = (const float4 *)(cb->d + o_box); a.s_cls = (const int32_t *)(cb->d + o_cls);
    a.s_order = (const int32_t *)(cb->d + o_ord); a.s_inv = (const int32_t *)(cb->d + o_inv); a.s_n = (const int32_t *)(cb->d + o_n);
    return cl_run(z, a, s0, cnt, frame_id, q, flat, out);
}

// one call on a tracker's device-resident state
template <typename T> int cl_process_tracker(rtmodt_colour *z, T *trk, int report_tsu, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                             const int64_t *frame_id, const rtmodt_colour_out *out) {
    RT_CHECK(z && trk, RTMODT_E_INVALID, "bad argument");
    TrackSrc src;
    TrackViewBase v;
    RT_TRY(track_src(trk, report_tsu, &src, &v));
    RT_CHECK(frame_id, RTMODT_E_INVALID, "null frame_id");
    RT_TRY(ledger_check_view(v, z->device, z->S, z->Mc, z->Mc, "colour attributes", "colour attributes"));
    RT_TRY(cl_check_frame_args(frames, v.n_streams, fh, fw, stride_bytes, mem_kind));
    RT_TRY(cl_check_ids(z, 0, v.n_streams, frame_id));
    RT_HIP(hipSetDevice(z->device));
    const size_t bytes = align_up(sizeof(ClFrame) * v.n_streams, 16);
    CmdBuf *cb;
    RT_TRY(cl_cmd(z, bytes, &cb));
    hipStream_t q = v.stream;                              // the stream the tracker's last update ran on: ordered after it
    RT_TRY(cl_order_after_last(z, q));
    RT_TRY(cl_fill_frames(z, (ClFrame *)cb->h, frames, v.n_streams, fh, fw, stride_bytes, mem_kind, frame_id));
    RT_TRY(z->stage.copy_in(frames, q));
    RT_TRY(cl_cmd_send(z, cb, bytes, q));
    ClArgs a = cl_args(z);
    a.frames = (const ClFrame *)cb->d; a.fh = fh; a.fw = fw; a.fpitch = (int64_t)z->stage.pitch;
    a.trk = src;
    return cl_run(z, a, 0, v.n_streams, frame_id, q, false, out);
}

// a stream's meta row, checked; the stream's rows and current buffer
int cl_read_meta(rtmodt_colour *z, int stream, int64_t m[4], int *cur, int *cnt) {
    RT_HIP(hipMemcpy(m, z->d_meta + 4 * stream, 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
    RT_CHECK(m[2] == 0 || m[2] == 1, RTMODT_E_INVALID, "colour stream %d: error %lld", stream, (long long)m[2]);
    *cur = (int)m[0] & 1; *cnt = (int)m[1];
    RT_CHECK(*cnt >= 0 && *cnt <= z->cap, RTMODT_E_INVALID, "colour stream %d: corrupt row count", stream);
    return RTMODT_OK;
}

}  // namespace

extern "C" {

void rtmodt_colour_default_cfg(rtmodt_colour_cfg *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->black_max = 48; cfg->chroma_min = 20; cfg->sat_split = 96; cfg->sat_hi_pm = 180; cfg->sat_lo_pm = 400; cfg->y_black = 64; cfg->y_white = 176;
    const int32_t hue[CL_HUE_BOUNDS] = {64, 192, 299, 725, 853, 1109, 1344, 1472};
    memcpy(cfg->hue, hue, sizeof(hue));
    cfg->pink_mx = 192; cfg->red_brown_mx = 96; cfg->orange_brown_mx = 176; cfg->yellow_brown_mx = 128;
    cfg->inset_x_pm = 200; cfg->top_pm = 150; cfg->split_pm = 500; cfg->bottom_pm = 900; cfg->max_side = 48; cfg->skip_occluded = 1;
    cfg->min_samples = 16; cfg->retire_after = 30;
}

void rtmodt_colour_destroy(rtmodt_colour *z) {
    if (!z) return;
    handle_close(z, [&] {
        hipFree(z->pool);
        hipHostFree(z->h_pin);
        for (int k = 0; k < 2; ++k) { z->cmd[k].release(); if (z->cmd_ev[k]) hipEventDestroy(z->cmd_ev[k]); }
        z->stage.release();
        z->timer.destroy();
    }, z->last_stream);
    delete z;
}

int rtmodt_colour_create(const rtmodt_colour_cfg *cfg, int n_streams, int max_tracks, rtmodt_colour **out) {
    RT_CHECK(out && cfg, RTMODT_E_INVALID, "null argument");
    const rtmodt_colour_cfg &c = *cfg;
    RT_TRY(cl_check_cfg(c));
    RT_CHECK(n_streams >= 1 && n_streams <= 4096 && max_tracks >= 1 && max_tracks <= 4096, RTMODT_E_INVALID, "n_streams %d / max_tracks %d out of range",
             n_streams, max_tracks);
    rtmodt_colour *z = new rtmodt_colour();
    z->device = c.device; z->S = n_streams; z->Mc = max_tracks; z->cap = 2 * max_tracks; z->cfg = c;
    if (!c.classes) z->cfg.n_classes = 0;
    std::vector<int32_t> classes(c.classes ? c.classes : nullptr, c.classes ? c.classes + c.n_classes : nullptr);
    z->filter = c.classes != nullptr;
    z->cfg.classes = nullptr;
    z->last_f.assign(n_streams, 0); z->has_f.assign(n_streams, 0);
    auto body = [&]() -> int {
        RT_CHECK(cl_smem(z) <= 150 * 1024, RTMODT_E_INVALID, "colour: capacity %d needs %zu B of LDS", z->cap, cl_smem(z));
        RT_TRY(handle_open(z));
        RT_TRY(z->timer.create());
        for (int k = 0; k < 2; ++k) RT_HIP(hipEventCreateWithFlags(&z->cmd_ev[k], hipEventDisableTiming));
        const size_t total = cl_carve(z, nullptr);
        RT_HIP(hipMalloc((void **)&z->pool, total));
        RT_HIP(handle_zero(z->pool, total, z->stream));
        cl_carve(z, z->pool);
        RT_HIP(hipHostMalloc((void **)&z->h_pin, (size_t)z->S * z->block_stride, hipHostMallocDefault));
        RT_HIP(hipMemcpyAsync(z->d_ledgers, z->h_ledgers.data(), sizeof(ClLedger) * z->S, hipMemcpyHostToDevice, z->stream));      // (behind the zeroing of the pool)
        if (!classes.empty()) RT_HIP(hipMemcpyAsync(z->d_classes, classes.data(), classes.size() * 4, hipMemcpyHostToDevice, z->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), z, rtmodt_colour_destroy, out);
}

int rtmodt_colour_process(rtmodt_colour *z, int stream, const int64_t *track_ids, const float *xyxy, const int32_t *cls, int n, const uint8_t *frame, int fh,
                          int fw, int stride_bytes, int mem_kind, int64_t frame_id, const rtmodt_colour_out *out) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n >= 0, RTMODT_E_INVALID, "bad argument");
    const int32_t n32 = n;
    return cl_process_lists(z, stream, 1, track_ids, xyxy, cls, &n32, std::max(n, 1), &frame, fh, fw, stride_bytes, mem_kind, &frame_id, true, out);
}

int rtmodt_colour_process_batch(rtmodt_colour *z, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n, int stride,
                                const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id,
                                const rtmodt_colour_out *out) {
    RT_CHECK(z && n && stride >= 0, RTMODT_E_INVALID, "bad argument");
    return cl_process_lists(z, 0, z->S, track_ids, xyxy, cls, n, stride, frames, fh, fw, stride_bytes, mem_kind, frame_id, false, out);
}

int rtmodt_colour_process_tracker(rtmodt_colour *z, rtmodt_tracker *trk, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                  const int64_t *frame_id, int report_tsu, const rtmodt_colour_out *out) {
    return cl_process_tracker(z, trk, report_tsu, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_colour_process_deepsort(rtmodt_colour *z, rtmodt_deepsort *ds, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                   const int64_t *frame_id, int report_tsu, const rtmodt_colour_out *out) {
    return cl_process_tracker(z, ds, report_tsu, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_colour_process_ocsort(rtmodt_colour *z, rtmodt_ocsort *oc, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                 const int64_t *frame_id, const rtmodt_colour_out *out) {
    return cl_process_tracker(z, oc, 0, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_colour_process_botsort(rtmodt_colour *z, rtmodt_botsort *bot, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                  const int64_t *frame_id, const rtmodt_colour_out *out) {
    return cl_process_tracker(z, bot, 0, frames, fh, fw, stride_bytes, mem_kind, frame_id, out);
}

int rtmodt_colour_state(rtmodt_colour *z, int stream, rtmodt_colour_row *rows, int32_t *n) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cl_sync(z));
    int64_t m[4];
    int cur, cnt;
    RT_TRY(cl_read_meta(z, stream, m, &cur, &cnt));
    *n = cnt;
    if (cnt && rows) {
        const ClLedger &L = z->h_ledgers[stream];
        const size_t c = (size_t)cnt;
        std::vector<int64_t> id(c), first(c), last(c);
        std::vector<uint32_t> hist(c * CL_BINS);
        std::vector<int4> ints(c);
        RT_HIP(hipMemcpy(id.data(), L.id[cur], c * 8, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(first.data(), L.first[cur], c * 8, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(last.data(), L.last[cur], c * 8, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(hist.data(), L.hist[cur], c * CL_BINS * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(ints.data(), L.ints[cur], c * 16, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < c; ++r) {
            rtmodt_colour_row &o = rows[r];
            memset(&o, 0, sizeof(o));
            o.track_id = id[r]; o.first_frame = first[r]; o.last_frame = last[r];
            memcpy(o.hist, hist.data() + r * CL_BINS, CL_BINS * 4);
            o.cls = ints[r].x; o.frames_used = ints[r].y; o.flags = ints[r].z; o.track = -1;
            for (int p = 0; p < 3; ++p) {
                const ClLabel lb = cl_label(hist.data() + r * CL_BINS, p);
                memcpy(&o.label[p], &lb, sizeof(lb));
            }
        }
    }
    // a stream in error still hands its rows out (the rows of the overflowing call and of the calls since), with the error code
    RT_CHECK(m[2] != 1, RTMODT_E_CAPACITY, "colour stream %d: ledger full (%d rows): lower retire_after or raise max_tracks", stream, z->cap);
    return RTMODT_OK;
}

int rtmodt_colour_load(rtmodt_colour *z, int stream, const rtmodt_colour_row *rows, int n) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n >= 0 && (n == 0 || rows), RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n <= z->cap, RTMODT_E_INVALID, "%d rows > 2 x max_tracks = %d", n, z->cap);
    int64_t newest = 0;
    for (int r = 0; r < n; ++r) {
        RT_CHECK(r == 0 || rows[r - 1].track_id < rows[r].track_id, RTMODT_E_INVALID, "row %d: track ids do not ascend strictly", r);
        RT_CHECK(rows[r].first_frame <= rows[r].last_frame && rows[r].frames_used >= 0, RTMODT_E_INVALID, "row %d: first_frame %lld > last_frame %lld, or frames_used %d",
                 r, (long long)rows[r].first_frame, (long long)rows[r].last_frame, rows[r].frames_used);
        newest = r == 0 ? rows[r].last_frame : std::max(newest, rows[r].last_frame);
    }
    RT_TRY(cl_sync(z));
    const ClLedger &L = z->h_ledgers[stream];
    if (n) {
        const size_t c = (size_t)n;
        std::vector<int64_t> id(c), first(c), last(c);
        std::vector<uint32_t> hist(c * CL_BINS);
        std::vector<int4> ints(c);
        for (size_t r = 0; r < c; ++r) {
            id[r] = rows[r].track_id; first[r] = rows[r].first_frame; last[r] = rows[r].last_frame;
            memcpy(hist.data() + r * CL_BINS, rows[r].hist, CL_BINS * 4);
            ints[r] = make_int4(rows[r].cls, rows[r].frames_used, rows[r].flags, 0);
        }
        RT_HIP(hipMemcpy(L.id[0], id.data(), c * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(L.first[0], first.data(), c * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(L.last[0], last.data(), c * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(L.hist[0], hist.data(), c * CL_BINS * 4, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(L.ints[0], ints.data(), c * 16, hipMemcpyHostToDevice));
    }
    const int64_t m[4] = {0, n, 0, 0};
    RT_HIP(hipMemcpy(z->d_meta + 4 * stream, m, sizeof(m), hipMemcpyHostToDevice));
    z->has_f[stream] = n > 0; z->last_f[stream] = newest;
    return RTMODT_OK;
}

int rtmodt_colour_reset(rtmodt_colour *z, int stream) {
    RT_CHECK(z && stream >= 0 && stream < z->S, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cl_sync(z));
    RT_HIP(handle_zero(z->d_meta + 4 * stream, 4 * sizeof(int64_t), z->stream));
    RT_TRY(handle_wait(z->stream));
    z->has_f[stream] = 0; z->last_f[stream] = 0;
    return RTMODT_OK;
}

int rtmodt_colour_last_ms(rtmodt_colour *z, float *kernel_ms) {
    RT_CHECK(z && kernel_ms, RTMODT_E_INVALID, "null argument");
    return z->timer.elapsed(z->device, 0, 1, kernel_ms, "no call has been timed yet");
}

int rtmodt_colour_name(int b, int g, int r, const rtmodt_colour_cfg *cfg) {
    RT_CHECK(cfg, RTMODT_E_INVALID, "null argument");
    RT_TRY(cl_check_cfg(*cfg));
    RT_CHECK(b >= 0 && b <= 255 && g >= 0 && g <= 255 && r >= 0 && r <= 255, RTMODT_E_INVALID, "pixel (%d, %d, %d) outside 0..255", b, g, r);
    return cl_name(cl_rule_of(*cfg, nullptr, 0), (uint32_t)b, (uint32_t)g, (uint32_t)r);
}

int rtmodt_colour_plan(const rtmodt_colour_cfg *cfg, const float *xyxy, int h, int w, rtmodt_colour_plan_out *out) {
    RT_CHECK(cfg && xyxy && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(cl_check_cfg(*cfg));
    RT_CHECK(h >= 1 && w >= 1 && h <= CL_MAX_DIM && w <= CL_MAX_DIM, RTMODT_E_INVALID, "frame %dx%d outside 1..%d", w, h, CL_MAX_DIM);
    ClPlan P;
    out->sampled = cl_plan(cl_rule_of(*cfg, nullptr, 0), xyxy[0], xyxy[1], xyxy[2], xyxy[3], 0, h, w, P) ? 1 : 0;
    if (!out->sampled) return RTMODT_OK;
    const PvRect *r[3] = {&P.raw, &P.box, &P.rect};
    int32_t *d[3] = {out->raw, out->box, out->rect};
    for (int k = 0; k < 3; ++k) { d[k][0] = r[k]->x0; d[k][1] = r[k]->y0; d[k][2] = r[k]->x1; d[k][3] = r[k]->y1; }
    out->split_row = P.ys; out->sx = P.sx; out->sy = P.sy; out->nx = P.nx; out->ny = P.ny;
    return RTMODT_OK;
}

}  // extern "C"
