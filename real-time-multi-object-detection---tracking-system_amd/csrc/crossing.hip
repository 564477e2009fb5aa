// crossing.hip -- directional line (tripwire) and gate crossing counts on the GPU: the meaning the reference's config gives a
// `trigger: "crossing"` zone with a `direction` (config/default.yaml:73-77) and its engine never implements (zone_engine.py:150
// parses the direction and nothing reads it).  ONE launch per frame, one 256-thread workgroup per video stream, run on a track
// list the host hands over or straight on the device-resident state of one of the four trackers (track_select_dev.h).
//
// tests/crossing_ref.py states the rules ("Crossing counter"); the kernel equals it exactly.  Everything after the
// centroid is integer arithmetic: coordinates are held to +-2^20, so every cross product is below 2^43.
//
// Per stream a LEDGER, rows sorted by track id, double-buffered: last passed frame, previous passed centroid, per line the last
// non-zero side (two bit masks), per gate an inside bit + the entry centroid and frame.  A frame is:
//   1. the PASSED tracks of the list (finite box; tracker sources: time_since_update == report_tsu, DeepSORT: confirmed) are
//      compacted by a prefix sum; each finds its old row by binary search (old ids staged in LDS); old rows not passed for more
//      than max_gap frames are dropped, the other idle rows are retained;
//   2. the (track, item) pairs are spread over the lanes: P = the item count rounded up to a power of two lanes per track, one
//      lane per line or gate; the pair's new bits travel to the row through a wave ballot (no atomics, no LDS), its count through
//      an integer atomic add (any order gives the same sums);
//   3. the new ledger = passed rows + retained idle rows, merged by rank (prefix sums + binary searches, no sort): the steps of
//      track_ledger_dev.h, which zones.hip, speed.hip and snapshot.hip run too;
//   4. events leave in (list order, lines in order, gates in order) through a workgroup prefix sum.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "handle_host.h"
#include "polygon.h"
#include "track_layout.h"

#define TL_HD __host__ __device__
#include "track_ledger_host.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_select_dev.h"
#include "track_ledger_dev.h"

constexpr int CR_THREADS = 256, CR_WAVES = CR_THREADS / 64;
constexpr int CR_MAX_LINES = 32, CR_MAX_GATES = 32, CR_MAX_POINTS = 2048, CR_MAX_CLASSES = 256;
constexpr int CR_LIMIT = 1 << 20;

struct CrossTable {                // device pointers
    const int4 *line;              // [L] ax, ay, bx, by
    const int32_t *dir;            // [L + G] lines: 0 both, 1 pos, 2 neg; gates: RTMODT_GATE_*
    const int2 *pts;               // all gates' vertices, concatenated
    const int32_t *off;            // [G + 1]
    int L, G, n_pts;
};

struct CrossLedger {               // one stream, double-buffered
    int64_t *id[2], *last[2]; int2 *prev[2]; uint32_t *pos[2], *neg[2], *in[2]; int2 *entry[2]; int64_t *entryf[2];   // entry* [cap][G]
};

struct CrossArgs {
    CrossTable tb;
    CrossLedger *ledgers;          // [n_streams]
    int64_t *meta;                 // [n_streams][4]: cur, rows, sticky err, 0
    int64_t *counts; int64_t counts_stride;   // per stream: line_total [L][2] | line_class [L][2][C] | gate_total [G] | gate_class [G][C]
    int C, cap, max_events, stream_base;
    int64_t max_gap, frame_id;
    // source A: a staged list [n_streams][cap], sorted by id; order = the caller's index of a sorted entry, inv = its inverse
    const int64_t *s_ids; const float4 *s_box; const int32_t *s_cls; const int32_t *s_order, *s_inv; const int32_t *s_n; int s_stride;
    // sources B..E: a tracker's device state (track_select_dev.h)
    TrackSrc trk;
    // per-stream scratch [n_streams][cap]
    int32_t *p_idx, *oldpos; uint64_t *evmask;
    // events [n_streams][max_events]; ev_n = the number that fired (may exceed max_events)
    rtmodt_crossing_event *ev; int32_t *ev_n;
};

// the zone engine's centroid (zones.hip), clamped to +-2^20; false: a coordinate is not finite, the track is not passed
__device__ __forceinline__ bool cr_centroid(const float4 b, int2 &c) {
    if (!(finite_bits(b.x) && finite_bits(b.y) && finite_bits(b.z) && finite_bits(b.w))) return false;
    float fx = (b.x + b.z) / 2.0f, fy = (b.y + b.w) / 2.0f;
    fx = fminf(fmaxf(fx, -(float)CR_LIMIT), (float)CR_LIMIT);
    fy = fminf(fmaxf(fy, -(float)CR_LIMIT), (float)CR_LIMIT);
    c = make_int2((int)fx, (int)fy);
    return true;
}
// sign((a - o) x (b - o))
__device__ __forceinline__ int cr_side(int ox, int oy, int ax, int ay, int bx, int by) {
    const long long v = (long long)(ax - ox) * (by - oy) - (long long)(ay - oy) * (bx - ox);
    return (v > 0) - (v < 0);
}
__device__ __forceinline__ bool cr_gate_fires(int dir, int dx, int dy) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    switch (dir) {
        case RTMODT_GATE_ANY: return true;
        case RTMODT_GATE_LEFT_TO_RIGHT: return dx > 0 && dx >= ay;
        case RTMODT_GATE_RIGHT_TO_LEFT: return -dx > 0 && -dx >= ay;
        case RTMODT_GATE_TOP_TO_BOTTOM: return dy > 0 && dy >= ax;
        case RTMODT_GATE_BOTTOM_TO_TOP: return -dy > 0 && -dy >= ax;
    }
    return false;
}

#pragma clang fp contract(off)

__global__ __launch_bounds__(CR_THREADS) void crossing_update(CrossArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x, tid = threadIdx.x;
    const int L = a.tb.L, G = a.tb.G, NI = L + G, cap = a.cap, C = a.C;
    int64_t *old_id = (int64_t *)smem;                    // [cap]
    int4 *line = (int4 *)(old_id + cap);                  // [CR_MAX_LINES]
    int2 *pts = (int2 *)(line + CR_MAX_LINES);            // [max(n_pts, 1)]
    int *ret_pre = (int *)(pts + (a.tb.n_pts > 0 ? a.tb.n_pts : 1));     // [cap + 1] retained flags, then their rank encoding (track_ledger.h)
    int *ppre = ret_pre + cap + 1;                        // [cap + 1] exclusive prefix of the list's passed flags
    int *idir = ppre + cap + 1;                           // [CR_MAX_LINES + CR_MAX_GATES]
    int *goff = idir + CR_MAX_LINES + CR_MAX_GATES;       // [CR_MAX_GATES + 1]
    int *wsum = goff + CR_MAX_GATES + 1;                  // [CR_WAVES]
    __shared__ int s_err;

    int64_t *meta = a.meta + (size_t)sidx * 4;
    const int cur = tl_meta_cur(meta), nxt = cur ^ 1, n_old = tl_meta_rows(meta, cap);
    const CrossLedger *Lp = a.ledgers + sidx;                 // (indexed where it lies: a local copy indexed by `cur` would live in scratch)
    const int64_t *o_id = Lp->id[cur], *o_last = Lp->last[cur], *o_entryf = Lp->entryf[cur];
    const int2 *o_prev = Lp->prev[cur], *o_entry = Lp->entry[cur];
    const uint32_t *o_pos = Lp->pos[cur], *o_neg = Lp->neg[cur], *o_in = Lp->in[cur];
    int64_t *n_id = Lp->id[nxt], *n_last = Lp->last[nxt], *n_entryf = Lp->entryf[nxt];
    int2 *n_prev = Lp->prev[nxt], *n_entry = Lp->entry[nxt];
    uint32_t *n_pos = Lp->pos[nxt], *n_neg = Lp->neg[nxt], *n_in = Lp->in[nxt];

    // ---- this frame's list ----
    TrackSel src;
    const int32_t *order = nullptr, *inv = nullptr;
    if (a.s_ids) {
        const size_t o = (size_t)sidx * a.s_stride;
        src = select_list(a.s_ids + o, a.s_box + o, a.s_cls + o, a.s_n[sidx]);
        order = a.s_order + o; inv = a.s_inv + o;
    } else src = select_tracks(a.trk, sidx);
    const int n = src.n < 0 ? 0 : (src.n > cap ? cap : src.n);      // host sizes cap >= the source's max_tracks
    const int64_t *ids = src.ids; const float4 *box = src.box; const int32_t *cls = src.cls;

    if (tid == 0) s_err = 0;
    for (int i = tid; i < L; i += CR_THREADS) line[i] = a.tb.line[i];
    for (int i = tid; i < NI; i += CR_THREADS) idir[i] = a.tb.dir[i];
    for (int i = tid; i <= G; i += CR_THREADS) goff[i] = a.tb.off[i];
    for (int i = tid; i < a.tb.n_pts; i += CR_THREADS) pts[i] = a.tb.pts[i];
    // an old row survives this frame while frame_id - last <= max_gap, whether or not its id is in the list
    ledger_stage_old<CR_THREADS>(o_id, n_old, old_id, ret_pre, [&](int j) { return a.frame_id - o_last[j] <= a.max_gap ? 1 : 0; });

    int32_t *p_idx = a.p_idx + (size_t)sidx * cap;
    int32_t *oldpos = a.oldpos + (size_t)sidx * cap;
    uint64_t *evmask = a.evmask + (size_t)sidx * cap;

    // ---- 1. the passed tracks, compacted in list order; each finds its old row (an expired one is not this track's row); the
    //         idle rows are ranked ----
    const int n_pass = ledger_compact<CR_THREADS>(n, ppre, p_idx, wsum, [&](int i) { int2 c; return selected(src, i) && cr_centroid(box[i], c); });
    const bool ascending = ledger_list_ascends<CR_THREADS>(ids, n, &s_err);
    ledger_match<CR_THREADS, true>(ids, p_idx, n_pass, old_id, n_old, ret_pre, oldpos);
    const int n_ret = ledger_rank<CR_THREADS>(n_old, ret_pre, wsum);
    const TlMerge mg = ledger_decide(ids, ppre, n, old_id, ret_pre, n_old, n_pass, n_ret, ascending, cap, &s_err);

    // ---- 2. (track, item) pairs: P lanes per track, lane `sub` of a group takes line `sub` or gate `sub - L` ----
    int P = 1;
    while (P < NI) P <<= 1;                                                   // <= 64: a group never straddles a wave
    const int tpp = CR_THREADS / P, grp = tid / P, sub = tid & (P - 1);
    const int gshift = (tid & 63) & ~(P - 1);
    const uint64_t gmask = P == 64 ? ~0ull : (1ull << P) - 1ull;
    int64_t *cnt = a.counts + (size_t)sidx * a.counts_stride;
    int64_t *line_total = cnt, *line_class = cnt + 2 * L, *gate_total = line_class + (size_t)2 * L * C, *gate_class = gate_total + G;
    for (int base = 0; base < n_pass; base += tpp) {
        const int t = base + grp;
        const bool tv = t < n_pass;
        bool b_pos = false, b_neg = false, b_in = false, b_ev = false;
        int i = 0, j = -1, np = 0;
        int2 c = make_int2(0, 0);
        if (tv) {
            i = p_idx[t]; j = oldpos[t];
            cr_centroid(box[i], c);
            np = tl_member_pos(mg, t, ids[i]);
            if (sub < L) {
                const int4 ab = line[sub];
                const int sd = cr_side(ab.x, ab.y, ab.z, ab.w, c.x, c.y);
                const int stored = j < 0 ? 0 : (o_pos[j] >> sub & 1u) ? 1 : (o_neg[j] >> sub & 1u) ? -1 : 0;
                const int ns = sd != 0 ? sd : stored;                         // on the line: the stored side stays
                b_pos = ns > 0; b_neg = ns < 0;
                if (sd != 0 && stored != 0 && stored != sd) {
                    const int2 q = o_prev[j];
                    if (cr_side(q.x, q.y, c.x, c.y, ab.x, ab.y) * cr_side(q.x, q.y, c.x, c.y, ab.z, ab.w) <= 0) {
                        const int d = sd > 0 ? 0 : 1, want = idir[sub];
                        if (want == RTMODT_LINE_BOTH || want == d + 1) {
                            b_ev = true;
                            atomicAdd((unsigned long long *)&line_total[2 * sub + d], 1ull);
                            const int k = cls[i];
                            if (k >= 0 && k < C) atomicAdd((unsigned long long *)&line_class[((size_t)2 * sub + d) * C + k], 1ull);
                        }
                    }
                }
            } else if (sub < NI) {
                const int g = sub - L, p0 = goff[g];
                const bool in = inside_or_on(pts + p0, goff[g + 1] - p0, c.x, c.y);
                const bool was = j >= 0 && (o_in[j] >> g & 1u);
                b_in = in;
                int2 e = j >= 0 ? o_entry[(size_t)j * G + g] : make_int2(0, 0);
                int64_t ef = j >= 0 ? o_entryf[(size_t)j * G + g] : 0;
                if (in && !was) { e = c; ef = a.frame_id; }                   // entering, or first seen inside
                if (!in && was && cr_gate_fires(idir[sub], c.x - e.x, c.y - e.y)) {
                    b_ev = true;
                    atomicAdd((unsigned long long *)&gate_total[g], 1ull);
                    const int k = cls[i];
                    if (k >= 0 && k < C) atomicAdd((unsigned long long *)&gate_class[(size_t)g * C + k], 1ull);
                }
                n_entry[(size_t)np * G + g] = e;
                n_entryf[(size_t)np * G + g] = ef;
            }
        }
        const uint64_t m_pos = (__ballot(b_pos) >> gshift) & gmask, m_neg = (__ballot(b_neg) >> gshift) & gmask;
        const uint64_t m_in = (__ballot(b_in) >> gshift) & gmask, m_ev = (__ballot(b_ev) >> gshift) & gmask;
        if (tv && sub == 0) {
            n_id[np] = ids[i];
            n_last[np] = a.frame_id;
            n_prev[np] = c;
            n_pos[np] = (uint32_t)m_pos; n_neg[np] = (uint32_t)m_neg; n_in[np] = (uint32_t)(m_in >> L);
            evmask[t] = m_ev;
        }
    }
    // ---- 3. idle rows move to their merged position, unchanged ----
    for (int j = tid; j < n_old; j += CR_THREADS) {
        const int np = tl_idle_pos(mg, j);
        if (np < 0) continue;
        n_id[np] = old_id[j];
        n_last[np] = o_last[j];
        n_prev[np] = o_prev[j];
        n_pos[np] = o_pos[j]; n_neg[np] = o_neg[j]; n_in[np] = o_in[j];
        for (int g = 0; g < G; ++g) { n_entry[(size_t)np * G + g] = o_entry[(size_t)j * G + g]; n_entryf[(size_t)np * G + g] = o_entryf[(size_t)j * G + g]; }
    }
    __syncthreads();

    // ---- 4. events, in list order (the caller's), then item order ----
    rtmodt_crossing_event *evs = a.ev + (size_t)sidx * a.max_events;
    int n_ev = 0;
    for (int base = 0; base < n; base += CR_THREADS) {
        const int p = base + tid;
        uint64_t ev = 0;
        int i = 0, t = 0;
        if (p < n) {
            i = inv ? inv[p] : p;
            if (ppre[i + 1] != ppre[i]) { t = ppre[i]; ev = evmask[t]; }
        }
        int tot;
        int pos = n_ev + block_scan_count<CR_WAVES>(__popcll(ev), wsum, tot);
        if (ev) {
            const int j = oldpos[t];                                          // a crossing or an exit always has an old row
            const float4 b = box[i];
            int2 c = make_int2(0, 0);
            cr_centroid(b, c);
            for (int k = 0; k < NI; ++k)
                if (ev >> k & 1ull) {
                    if (pos < a.max_events && j >= 0) {
                        rtmodt_crossing_event r;
                        const bool is_line = k < L;
                        const int g = k - L;
                        const int2 q = is_line ? o_prev[j] : o_entry[(size_t)j * G + g];
                        r.track_id = ids[i];
                        r.frames = a.frame_id - (is_line ? o_last[j] : o_entryf[(size_t)j * G + g]);
                        r.xyxy[0] = b.x; r.xyxy[1] = b.y; r.xyxy[2] = b.z; r.xyxy[3] = b.w;
                        r.centroid[0] = c.x; r.centroid[1] = c.y;
                        r.prev[0] = q.x; r.prev[1] = q.y;
                        r.track = order ? order[i] : i;
                        r.kind = is_line ? RTMODT_CROSSING_LINE : RTMODT_CROSSING_GATE;
                        r.index = is_line ? k : g;
                        r.direction = is_line ? (cr_side(line[k].x, line[k].y, line[k].z, line[k].w, c.x, c.y) > 0 ? RTMODT_LINE_POS : RTMODT_LINE_NEG) : idir[k];
                        r.cls = cls[i];
                        r.reserved = 0;
                        evs[pos] = r;
                    }
                    ++pos;
                }
        }
        n_ev += tot;
    }
    if (tid == 0) {
        a.ev_n[sidx] = n_ev;
        tl_meta_write(meta, cur, tl_rows(mg), s_err);
    }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_crossing : HandleBase {
    int S = 1, Mc = 0, cap = 0, L = 0, G = 0, C = 0, n_pts = 0, max_events = 0;
    int64_t max_gap = 0;
    char *pool = nullptr;                 // every device array below lives in this one allocation
    CrossTable tb{};
    CrossLedger *d_ledgers = nullptr;
    std::vector<CrossLedger> h_ledgers;
    int64_t *d_meta = nullptr, *d_counts = nullptr;
    size_t counts_stride = 0;
    int64_t *s_ids = nullptr; float4 *s_box = nullptr; int32_t *s_cls = nullptr, *s_order = nullptr, *s_inv = nullptr, *s_n = nullptr;
    int32_t *p_idx = nullptr, *oldpos = nullptr; uint64_t *evmask = nullptr;
    rtmodt_crossing_event *ev = nullptr; int32_t *ev_n = nullptr;
    char *h_pin = nullptr;                // pinned mirror of the event block (records, counts per stream) + meta
    size_t ev_bytes = 0;
};

namespace {

// lays out every device array; base == nullptr -> size only
size_t cr_carve(rtmodt_crossing *z, char *base) {
    Carver c{base};
    const size_t S = z->S, cap = z->cap, L = z->L, G = z->G, E = z->max_events, Gs = std::max(z->G, 1);
    const int4 *line = c.take<int4>(std::max(z->L, 1));
    const int32_t *dir = c.take<int32_t>(std::max<size_t>(L + G, 1));
    const int2 *pts = c.take<int2>(std::max(z->n_pts, 1));
    const int32_t *off = c.take<int32_t>(G + 1);
    z->tb = CrossTable{line, dir, pts, off, z->L, z->G, z->n_pts};
    z->d_ledgers = c.take<CrossLedger>(S);
    z->d_meta = c.take<int64_t>(S * 4);
    z->counts_stride = 2 * L + 2 * L * z->C + G + G * z->C;
    z->d_counts = c.take<int64_t>(std::max<size_t>(S * z->counts_stride, 1));
    if (base) z->h_ledgers.assign(S, CrossLedger{});
    for (size_t s = 0; s < S; ++s)
        for (int b = 0; b < 2; ++b) {
            int64_t *id = c.take<int64_t>(cap), *last = c.take<int64_t>(cap), *entryf = c.take<int64_t>(cap * Gs);
            int2 *prev = c.take<int2>(cap), *entry = c.take<int2>(cap * Gs);
            uint32_t *pos = c.take<uint32_t>(cap), *neg = c.take<uint32_t>(cap), *in = c.take<uint32_t>(cap);
            if (base) {
                CrossLedger &Lg = z->h_ledgers[s];
                Lg.id[b] = id; Lg.last[b] = last; Lg.entryf[b] = entryf; Lg.prev[b] = prev; Lg.entry[b] = entry; Lg.pos[b] = pos; Lg.neg[b] = neg; Lg.in[b] = in;
            }
        }
    z->s_ids = c.take<int64_t>(S * cap); z->s_box = c.take<float4>(S * cap); z->s_cls = c.take<int32_t>(S * cap);
    z->s_order = c.take<int32_t>(S * cap); z->s_inv = c.take<int32_t>(S * cap); z->s_n = c.take<int32_t>(S);
    z->p_idx = c.take<int32_t>(S * cap); z->oldpos = c.take<int32_t>(S * cap); z->evmask = c.take<uint64_t>(S * cap);
    const size_t ev0 = align_up(c.off, 16);
    z->ev = c.take<rtmodt_crossing_event>(S * E); z->ev_n = c.take<int32_t>(S);
    z->ev_bytes = align_up(c.off, 16) - ev0;
    return align_up(c.off, 16);
}

CrossArgs cr_args(rtmodt_crossing *z, int64_t frame_id) {
    CrossArgs a{};
    a.tb = z->tb; a.ledgers = z->d_ledgers; a.meta = z->d_meta; a.counts = z->d_counts; a.counts_stride = (int64_t)z->counts_stride;
    a.C = z->C; a.cap = z->cap; a.max_events = z->max_events; a.stream_base = 0; a.max_gap = z->max_gap; a.frame_id = frame_id;
    a.p_idx = z->p_idx; a.oldpos = z->oldpos; a.evmask = z->evmask; a.ev = z->ev; a.ev_n = z->ev_n;
    return a;
}

size_t cr_smem(const rtmodt_crossing *z) {
    return (size_t)z->cap * 8 + CR_MAX_LINES * 16 + (size_t)std::max(z->n_pts, 1) * 8 +
           (2 * ((size_t)z->cap + 1) + CR_MAX_LINES + CR_MAX_GATES + CR_MAX_GATES + 1 + CR_WAVES) * 4 + 32;
}

int cr_launch(rtmodt_crossing *z, const CrossArgs &a, int n_streams, hipStream_t s) {
    const size_t smem = cr_smem(z);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)crossing_update, smem, seen));
    hipLaunchKernelGGL(crossing_update, dim3(n_streams), dim3(CR_THREADS), smem, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

// the event records, event counts and meta of streams [s0, s0 + cnt) -> pinned host mirror (same layout as the device block), then sync
struct CrEvHost { const rtmodt_crossing_event *ev; const int32_t *n; const int64_t *meta; };
int cr_fetch(rtmodt_crossing *z, hipStream_t s, int s0, int cnt, CrEvHost &h) {
    char *d0 = (char *)z->ev;
    const size_t rec0 = (size_t)s0 * z->max_events * sizeof(rtmodt_crossing_event), n0 = (size_t)((const char *)(z->ev_n + s0) - d0);
    RT_HIP(hipMemcpyAsync(z->h_pin + rec0, d0 + rec0, (size_t)cnt * z->max_events * sizeof(rtmodt_crossing_event), hipMemcpyDeviceToHost, s));
    RT_HIP(hipMemcpyAsync(z->h_pin + n0, d0 + n0, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
    RT_HIP(hipMemcpyAsync(z->h_pin + z->ev_bytes + (size_t)s0 * 32, z->d_meta + 4 * s0, sizeof(int64_t) * 4 * cnt, hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    h.ev = (const rtmodt_crossing_event *)z->h_pin;
    h.n = (const int32_t *)(z->h_pin + ((const char *)z->ev_n - d0));
    h.meta = (const int64_t *)(z->h_pin + z->ev_bytes);
    return RTMODT_OK;
}

int cr_check_sticky(rtmodt_crossing *z, int s, int64_t err) {
    return ledger_check_sticky("crossing", s, err, z->cap, "lower max_gap_frames or raise max_tracks");
}

// copies the events of streams [s0, s0 + cnt) out ([stream][max_events] slots, n_events[stream]); the first failure is reported after every
// stream has been copied
int cr_deliver(rtmodt_crossing *z, const CrEvHost &h, int s0, int cnt, bool flat, rtmodt_crossing_event *events, int32_t *n_events) {
    int rc = RTMODT_OK;
    for (int s = s0; s < s0 + cnt; ++s) {
        const int fired = h.n[s], ne = std::min(fired, z->max_events);
        const size_t eo = (size_t)s * z->max_events, dst = flat ? 0 : eo;
        if (events && ne > 0) memcpy(events + dst, h.ev + eo, sizeof(rtmodt_crossing_event) * ne);
        n_events[flat ? 0 : s] = ne;
        if (rc == RTMODT_OK) rc = cr_check_sticky(z, s, h.meta[4 * s + 2]);
        if (rc == RTMODT_OK && fired > z->max_events)
            rc = fail(RTMODT_E_CAPACITY, "crossing stream %d: %d events in one frame > max_events %d (the counts are complete, the events truncated)", s,
                      fired, z->max_events);
    }
    return rc;
}

// every _process* has synchronised the stream it launched on before it returned: the handle's own stream is all there is to wait for
int cr_sync_own(rtmodt_crossing *z) {
    RT_HIP(hipSetDevice(z->device));
    RT_HIP(hipStreamSynchronize(z->stream));
    return RTMODT_OK;
}

// one frame on a tracker's device-resident state
template <typename T> int cr_process_tracker(rtmodt_crossing *z, T *trk, int report_tsu, int64_t frame_id, rtmodt_crossing_event *events, int32_t *n_events) {
    RT_CHECK(z && trk && n_events, RTMODT_E_INVALID, "bad argument");
    CrossArgs a = cr_args(z, frame_id);
    TrackViewBase v;
    RT_TRY(track_src(trk, report_tsu, &a.trk, &v));
    RT_TRY(ledger_check_view(v, z->device, z->S, z->cap, z->Mc, "crossing counter", "crossing counter"));
    RT_HIP(hipSetDevice(z->device));
    RT_TRY(cr_launch(z, a, v.n_streams, v.stream));         // the stream the tracker's last update ran on: ordered after it
    CrEvHost h;
    RT_TRY(cr_fetch(z, v.stream, 0, v.n_streams, h));
    return cr_deliver(z, h, 0, v.n_streams, false, events, n_events);
}

}  // namespace

extern "C" {

void rtmodt_crossing_destroy(rtmodt_crossing *z) {
    if (!z) return;
    handle_close(z, [&] { hipFree(z->pool); hipHostFree(z->h_pin); });
    delete z;
}

int rtmodt_crossing_create(int device, const rtmodt_line_cfg *lines, int n_lines, const rtmodt_gate_cfg *gates, int n_gates, int n_classes,
                           int n_streams, int max_tracks, int max_events, int64_t max_gap_frames, rtmodt_crossing **out) {
    RT_CHECK(out && (lines || n_lines == 0) && (gates || n_gates == 0), RTMODT_E_INVALID, "null argument");
    RT_CHECK(n_lines >= 0 && n_lines <= CR_MAX_LINES && n_gates >= 0 && n_gates <= CR_MAX_GATES, RTMODT_E_INVALID, "%d lines / %d gates (at most %d / %d)",
             n_lines, n_gates, CR_MAX_LINES, CR_MAX_GATES);
    RT_CHECK(n_classes >= 1 && n_classes <= CR_MAX_CLASSES, RTMODT_E_INVALID, "n_classes %d (1..%d)", n_classes, CR_MAX_CLASSES);
    RT_CHECK(n_streams >= 1 && n_streams <= 4096 && max_tracks >= 1 && max_tracks <= 4096 && max_events >= 1 && max_events <= (1 << 20),
             RTMODT_E_INVALID, "n_streams %d / max_tracks %d / max_events %d out of range", n_streams, max_tracks, max_events);
    RT_CHECK(max_gap_frames >= 0, RTMODT_E_INVALID, "max_gap_frames %lld is negative", (long long)max_gap_frames);
    auto in_range = [](int32_t v) { return v >= -CR_LIMIT && v <= CR_LIMIT; };
    std::vector<int4> ln;
    std::vector<int32_t> dir, off(1, 0);
    std::vector<int2> pts;
    for (int i = 0; i < n_lines; ++i) {
        const rtmodt_line_cfg &c = lines[i];
        RT_CHECK(in_range(c.ax) && in_range(c.ay) && in_range(c.bx) && in_range(c.by), RTMODT_E_INVALID, "line %d: endpoint outside [-2^20, 2^20]", i);
        RT_CHECK(c.direction == RTMODT_LINE_BOTH || c.direction == RTMODT_LINE_POS || c.direction == RTMODT_LINE_NEG, RTMODT_E_INVALID,
                 "line %d: direction %d", i, c.direction);
        ln.push_back(make_int4(c.ax, c.ay, c.bx, c.by));
        dir.push_back(c.direction);
    }
    for (int i = 0; i < n_gates; ++i) {
        const rtmodt_gate_cfg &c = gates[i];
        RT_CHECK(c.n_points >= 0 && (c.n_points == 0 || c.polygon_xy), RTMODT_E_INVALID, "gate %d: bad polygon", i);
        RT_CHECK(c.direction >= RTMODT_GATE_ANY && c.direction <= RTMODT_GATE_BOTTOM_TO_TOP, RTMODT_E_INVALID, "gate %d: direction %d", i, c.direction);
        RT_CHECK((size_t)c.n_points + pts.size() <= (size_t)CR_MAX_POINTS, RTMODT_E_INVALID, "more than %d gate vertices", CR_MAX_POINTS);
        for (int p = 0; p < c.n_points; ++p) {
            RT_CHECK(in_range(c.polygon_xy[2 * p]) && in_range(c.polygon_xy[2 * p + 1]), RTMODT_E_INVALID, "gate %d: vertex %d outside [-2^20, 2^20]", i, p);
            pts.push_back(make_int2(c.polygon_xy[2 * p], c.polygon_xy[2 * p + 1]));
        }
        off.push_back((int32_t)pts.size());
        dir.push_back(c.direction);
    }
    rtmodt_crossing *z = new rtmodt_crossing();
    z->device = device; z->S = n_streams; z->Mc = max_tracks; z->cap = 2 * max_tracks; z->L = n_lines; z->G = n_gates; z->C = n_classes;
    z->n_pts = (int)pts.size(); z->max_events = max_events; z->max_gap = max_gap_frames;
    auto body = [&]() -> int {
        RT_CHECK(cr_smem(z) <= 150 * 1024, RTMODT_E_INVALID, "crossing: capacity %d needs %zu B of LDS", z->cap, cr_smem(z));
        RT_TRY(handle_open(z));
        const size_t total = cr_carve(z, nullptr);
        RT_HIP(hipMalloc((void **)&z->pool, total));
        RT_HIP(handle_zero(z->pool, total, z->stream));             // (the copies below go behind it, on the same stream)
        cr_carve(z, z->pool);
        RT_HIP(hipHostMalloc((void **)&z->h_pin, z->ev_bytes + sizeof(int64_t) * 4 * z->S, hipHostMallocDefault));
        if (!ln.empty()) RT_HIP(hipMemcpyAsync((void *)z->tb.line, ln.data(), ln.size() * sizeof(int4), hipMemcpyHostToDevice, z->stream));
        if (!dir.empty()) RT_HIP(hipMemcpyAsync((void *)z->tb.dir, dir.data(), dir.size() * 4, hipMemcpyHostToDevice, z->stream));
        if (!pts.empty()) RT_HIP(hipMemcpyAsync((void *)z->tb.pts, pts.data(), pts.size() * sizeof(int2), hipMemcpyHostToDevice, z->stream));
        RT_HIP(hipMemcpyAsync((void *)z->tb.off, off.data(), off.size() * 4, hipMemcpyHostToDevice, z->stream));
        RT_HIP(hipMemcpyAsync(z->d_ledgers, z->h_ledgers.data(), sizeof(CrossLedger) * z->S, hipMemcpyHostToDevice, z->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), z, rtmodt_crossing_destroy, out);
}

int rtmodt_crossing_process(rtmodt_crossing *z, int stream, const int64_t *track_ids, const float *xyxy, const int32_t *cls, int n, int64_t frame_id,
                            rtmodt_crossing_event *events, int32_t *n_events) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n >= 0 && n_events, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n == 0 || (track_ids && xyxy && cls), RTMODT_E_INVALID, "null tracks");
    RT_CHECK(n <= z->Mc, RTMODT_E_CAPACITY, "%d tracks > max_tracks %d", n, z->Mc);
    RT_HIP(hipSetDevice(z->device));
    // the ledger is sorted by id: hand the list over in id order, with the caller's order both ways
    const int32_t n32 = n;
    RT_TRY(ledger_stage_lists(LedgerStaging{z->s_ids, z->s_box, z->s_cls, z->s_order, z->s_inv, z->s_n, z->cap}, stream, 1, track_ids, xyxy, cls, &n32, 0, false,
                              z->stream));
    CrossArgs a = cr_args(z, frame_id);
    a.stream_base = stream;
    a.s_ids = z->s_ids; a.s_box = z->s_box; a.s_cls = z->s_cls; a.s_order = z->s_order; a.s_inv = z->s_inv; a.s_n = z->s_n; a.s_stride = z->cap;
    RT_TRY(cr_launch(z, a, 1, z->stream));
    CrEvHost h;
    RT_TRY(cr_fetch(z, z->stream, stream, 1, h));
    return cr_deliver(z, h, stream, 1, true, events, n_events);
}

int rtmodt_crossing_process_tracker(rtmodt_crossing *z, rtmodt_tracker *trk, int64_t frame_id, int report_tsu, rtmodt_crossing_event *events,
                                    int32_t *n_events) {
    return cr_process_tracker(z, trk, report_tsu, frame_id, events, n_events);
}

int rtmodt_crossing_process_deepsort(rtmodt_crossing *z, rtmodt_deepsort *ds, int64_t frame_id, int report_tsu, rtmodt_crossing_event *events,
                                     int32_t *n_events) {
    return cr_process_tracker(z, ds, report_tsu, frame_id, events, n_events);
}

int rtmodt_crossing_process_botsort(rtmodt_crossing *z, rtmodt_botsort *bot, int64_t frame_id, rtmodt_crossing_event *events, int32_t *n_events) {
    return cr_process_tracker(z, bot, 0, frame_id, events, n_events);
}

int rtmodt_crossing_process_ocsort(rtmodt_crossing *z, rtmodt_ocsort *oc, int64_t frame_id, rtmodt_crossing_event *events, int32_t *n_events) {
    return cr_process_tracker(z, oc, 0, frame_id, events, n_events);
}

int rtmodt_crossing_counts(rtmodt_crossing *z, int stream, int64_t *line_total, int64_t *line_class, int64_t *gate_total, int64_t *gate_class) {
    RT_CHECK(z && stream >= 0 && stream < z->S, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cr_sync_own(z));
    const size_t L = z->L, G = z->G, C = z->C;
    const int64_t *c = z->d_counts + (size_t)stream * z->counts_stride;
    if (line_total && L) RT_HIP(hipMemcpy(line_total, c, 2 * L * 8, hipMemcpyDeviceToHost));
    if (line_class && L) RT_HIP(hipMemcpy(line_class, c + 2 * L, 2 * L * C * 8, hipMemcpyDeviceToHost));
    if (gate_total && G) RT_HIP(hipMemcpy(gate_total, c + 2 * L + 2 * L * C, G * 8, hipMemcpyDeviceToHost));
    if (gate_class && G) RT_HIP(hipMemcpy(gate_class, c + 2 * L + 2 * L * C + G, G * C * 8, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_crossing_reset_counts(rtmodt_crossing *z) {
    RT_CHECK(z, RTMODT_E_INVALID, "null argument");
    RT_TRY(cr_sync_own(z));
    if (z->counts_stride) RT_HIP(handle_zero(z->d_counts, (size_t)z->S * z->counts_stride * 8, z->stream));
    return handle_wait(z->stream);
}

int rtmodt_crossing_state(rtmodt_crossing *z, int stream, int64_t *ids, int64_t *last_frame, int32_t *prev_xy, uint32_t *side_pos, uint32_t *side_neg,
                          uint32_t *inside, int32_t *entry_xy, int64_t *entry_frame, int32_t *n) {
    RT_CHECK(z && stream >= 0 && stream < z->S && n, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cr_sync_own(z));
    int64_t m[4];
    RT_HIP(hipMemcpy(m, z->d_meta + 4 * stream, sizeof(m), hipMemcpyDeviceToHost));
    RT_TRY(cr_check_sticky(z, stream, m[2]));
    const int cur = (int)m[0] & 1, cnt = (int)m[1];
    RT_CHECK(cnt >= 0 && cnt <= z->cap, RTMODT_E_INVALID, "crossing stream %d: corrupt row count", stream);
    const CrossLedger &Lg = z->h_ledgers[stream];
    *n = cnt;
    if (cnt) {
        const size_t c = (size_t)cnt;
        if (ids) RT_HIP(hipMemcpy(ids, Lg.id[cur], c * 8, hipMemcpyDeviceToHost));
        if (last_frame) RT_HIP(hipMemcpy(last_frame, Lg.last[cur], c * 8, hipMemcpyDeviceToHost));
        if (prev_xy) RT_HIP(hipMemcpy(prev_xy, Lg.prev[cur], c * 8, hipMemcpyDeviceToHost));
        if (side_pos) RT_HIP(hipMemcpy(side_pos, Lg.pos[cur], c * 4, hipMemcpyDeviceToHost));
        if (side_neg) RT_HIP(hipMemcpy(side_neg, Lg.neg[cur], c * 4, hipMemcpyDeviceToHost));
        if (inside) RT_HIP(hipMemcpy(inside, Lg.in[cur], c * 4, hipMemcpyDeviceToHost));
        if (entry_xy && z->G) RT_HIP(hipMemcpy(entry_xy, Lg.entry[cur], c * z->G * 8, hipMemcpyDeviceToHost));
        if (entry_frame && z->G) RT_HIP(hipMemcpy(entry_frame, Lg.entryf[cur], c * z->G * 8, hipMemcpyDeviceToHost));
    }
    return RTMODT_OK;
}

}  // extern "C"
