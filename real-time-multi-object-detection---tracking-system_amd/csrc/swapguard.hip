// swapguard.hip -- ByteTrack identities verified by appearance, ID swaps reverted online on the GPU: the cure the reference's design
// document asks for three times and never builds (TECHNICAL_DESIGN_DOCUMENT.md B.4 "Re-Identification Considerations": a feature
// buffer per track, the average colour histogram of the last 5 frames; when two tracks swap within 3 frames compare histograms and
// revert if similarity > 0.85; B.4's failure table: "add appearance verification"; G.1 row 1: "add lightweight appearance hash
// verification").  tests/swapguard_ref.py states the rules; the kernel equals it exactly.  All arithmetic is
// integer except the IoU, which is the tracker's iou_ref (float32; this file is built with FMA contraction off and IEEE division).
//
// Per stream a LEDGER keyed by track id.  The index (ids ascending + a slot number) is double-buffered and merged by rank like the
// crossing counter's (crossing.hip); the payload of a row -- last passed frame, a ring of the last `history` int8[192] descriptors
// of csrc/appearance.hip with count and head, the frame of the last contact and the id touched then -- stays in its slot, so a
// frame moves no descriptor but the ones it stores.  A frame of a stream is, whatever the number of tracks:
//   gather           (tracker source only) the passed tracks' boxes, compacted in list order;
//   launch_describe  their descriptors, as appearance.hip computes them;
//   swapguard_step   one 256-thread workgroup per stream:
//     0. rows not passed for more than max_gap frames are dropped;
//     1. a passed track whose descriptor is all zero is BLIND; each passed track finds its row by binary search;
//     2. partner(i) = the other passed track of largest IoU (ties: lowest index; a NaN is never the largest), one thread per track
//        over the boxes in LDS; IN CONTACT iff that IoU > contact_iou;
//     3. a pair i < j with ids A, B is REVERTED iff both rows exist, neither track is in contact or blind, row[A] names B and row[B]
//        names A as the id last touched, both contacts lie at most `window` frames back, both rings hold min_history descriptors,
//        and with sim(q, ref) = 1000 * dot / max(1, isqrt(n2(q) * n2(ref))), ref = the sum of a ring:
//        sim(q_i, ref[B]) and sim(q_j, ref[A]) >= min_similarity_pm, and each exceeds the track's similarity to the history of the
//        id it carries by min_gain_pm.  The contact ids are mutual, so a track is in at most one pair: no matching is needed.  The
//        four 192-wide dot products and the four norms of a pair are one wave's work (three bins a lane, a wave reduction);
//     4. a reverted pair exchanges its two ids in the list (in the tracker's state, in place), clears both contact ids, and emits
//        one event, events in ascending i through a workgroup prefix sum;
//     5. every passed track's row (found or created, under its FINAL id) takes the frame; in contact: the contact frame and the
//        partner's final id; else, unless blind, the descriptor is pushed into the ring.  Descriptors taken during an overlap are
//        never stored: they mix the two objects.  New index = passed rows + retained idle rows, merged by rank.
// A ledger holds 2 x max_tracks rows; one that would pass that drops its idle rows and the stream stays in error (meta[2] = 1).
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "frame_stage.h"
#include "handle_host.h"
#include "lap.h"
#include "track_layout.h"

namespace rtmodt {

#include "track_dev.h"
#include "wg_dev.h"

constexpr int SG_THREADS = 256, SG_WAVES = SG_THREADS / 64;
constexpr int SG_MAX_TRACKS = 1024, SG_MAX_HISTORY = 8, SG_MAX_STREAMS = DS_MAX_STREAMS;
constexpr int SG_WORDS = APP_DIM / 4;                       // a descriptor as 32-bit words
// bins are 0..127, a ring sums at most SG_MAX_HISTORY of them: every dot product and norm fits 31 bits, the product of two norms 63
static_assert((long long)APP_DIM * 127 * 127 * SG_MAX_HISTORY * SG_MAX_HISTORY < (1ll << 31), "a ring's norm must fit an int32");
static_assert((double)APP_DIM * 127 * 127 * ((double)APP_DIM * 127 * 127 * SG_MAX_HISTORY * SG_MAX_HISTORY) < 9.2e18, "n2(q) * n2(ref) must fit an int64");

struct SgLedger {                  // one stream; device pointers
    int64_t *sid[2]; int32_t *sslot[2];                     // the index, double-buffered: ids ascending, and the slot of each [cap]
    int64_t *last, *cframe, *cid; int32_t *count, *head;    // per slot [cap]
    int8_t *ring;                                           // [cap][history][APP_DIM]; positions [0, count) are valid, `head` is written next
};

struct SgArgs {
    SgLedger *ledgers;             // [n_streams]
    int64_t *meta;                 // [n_streams][4]: cur, rows, sticky err, swaps reverted
    int cap, Mc, history, min_history, min_sim, min_gain, max_events, stream_base;
    float contact_iou;
    int64_t window, max_gap, frame_id;
    // the passed tracks [n_streams][Mc]: box, index into the list, count, descriptor
    const float4 *box; const int32_t *src; const int32_t *n; const int8_t *desc;
    // the list's ids: a staged list [n_streams][Mc], or the ByteTrack tracker's state (written in place)
    int64_t *s_ids; TrackerState *t_states; const int64_t *t_meta;
    int32_t *sims;                 // scratch [n_streams][Mc][4]
    rtmodt_swap_event *ev; int32_t *ev_n;      // [n_streams][max_events]; ev_n = the number that fired (may exceed max_events)
};

struct SgGatherArgs {
    const TrackerState *t_states; const int64_t *t_meta; int t_max, report_tsu, Mc;
    float4 *box; int32_t *src; int32_t *n; int64_t *meta;
};

__device__ __forceinline__ int sg_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ int sg_sim(int dot, int n2q, int n2r) {
    long long den = isqrt64((long long)n2q * (long long)n2r);
    if (den < 1) den = 1;
    return (int)((1000ll * dot) / den);
}

// the passed tracks of a ByteTrack state (time_since_update == report_tsu), compacted in list order; more than Mc of them: none, and the
// stream is in error
__global__ __launch_bounds__(SG_THREADS) void swapguard_gather(SgGatherArgs a) {
    __shared__ int wsum[SG_WAVES];
    const int sidx = blockIdx.x, tid = threadIdx.x;
    const TrackerState *st = a.t_states + sidx;
    const int64_t *tm = a.t_meta + (size_t)sidx * 8;
    const int tc = (int)tm[0] & 1;
    int n = (int)tm[1];
    n = n < 0 ? 0 : (n > a.t_max ? a.t_max : n);
    const int32_t *tsu = st->tsu[tc];
    const float4 *box = st->box[tc];
    const size_t po = (size_t)sidx * a.Mc;
    int n_pass = 0;
    for (int base = 0; base < n; base += SG_THREADS) {
        const int i = base + tid;
        const bool f = i < n && tsu[i] == a.report_tsu;
        int tot;
        const int pos = n_pass + block_scan_count<SG_WAVES>(f ? 1 : 0, wsum, tot);
        if (f && pos < a.Mc) { a.box[po + pos] = box[i]; a.src[po + pos] = i; }
        n_pass += tot;
    }
    if (tid == 0) {
        a.n[sidx] = n_pass > a.Mc ? 0 : n_pass;
        if (n_pass > a.Mc) a.meta[(size_t)sidx * 4 + 2] = 2;
    }
}

// flag bits of a passed track
constexpr int SG_CONTACT = 1, SG_BLIND = 2, SG_NEW = 4;

__global__ __launch_bounds__(SG_THREADS) void swapguard_step(SgArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = a.cap, Mc = a.Mc, H = a.history;
    // every array's size is a multiple of 16 bytes (cap and Mc are rounded up to 4 in the carve)
    const int capr = (cap + 4) & ~3, Mr = (Mc + 3) & ~3;
    int64_t *old_id = (int64_t *)smem;                     // [capr] the old index's ids
    int64_t *pid = old_id + capr;                          // [Mr] a passed track's id; from phase 4 on its final id
    int64_t *spid = pid + Mr;                              // [Mr] the final ids, ascending
    float4 *box = (float4 *)(spid + Mr);                   // [Mr]
    int *keep = (int *)(box + Mr);                         // [capr] idle rows that stay: flags, then their exclusive prefix
    int *used = keep + capr;                               // [capr] slots in use, then the list of free slots
    int *slot = used + capr;                               // [Mr] the slot of a passed track's row (-1: none yet)
    int *partner = slot + Mr;                              // [Mr]
    int *flags = partner + Mr;                             // [Mr]
    int *cand = flags + Mr;                                // [Mr] phase 3: the pair's other track (owner: the lower index), else -1; phase 5: ring position to write, else -1
    int *rank = cand + Mr;                                 // [Mr] final ids below this track's
    int *wsum = rank + Mr;                                 // [SG_WAVES]

    int64_t *meta = a.meta + (size_t)sidx * 4;
    const int cur = (int)meta[0] & 1, nxt = cur ^ 1;
    int n_old = (int)meta[1];
    n_old = n_old < 0 ? 0 : (n_old > cap ? cap : n_old);
    const SgLedger *Lp = a.ledgers + sidx;
    const int64_t *o_sid = Lp->sid[cur];
    const int32_t *o_slot = Lp->sslot[cur];
    int64_t *n_sid = Lp->sid[nxt];
    int32_t *n_slot = Lp->sslot[nxt];
    int64_t *r_last = Lp->last, *r_cframe = Lp->cframe, *r_cid = Lp->cid;
    int32_t *r_count = Lp->count, *r_head = Lp->head;
    int8_t *r_ring = Lp->ring;

    int np = a.n[sidx];
    np = np < 0 ? 0 : (np > Mc ? Mc : np);
    const size_t po = (size_t)sidx * Mc;
    const int32_t *src = a.src + po;
    const int8_t *desc = a.desc + po * APP_DIM;
    int64_t *ids;
    if (a.s_ids) {
        ids = a.s_ids + po;
    } else {
        const int tc = (int)a.t_meta[(size_t)sidx * 8] & 1;
        ids = a.t_states[sidx].ids[tc];
    }

    // ---- 0. the old index; rows that have expired ----
    for (int j = tid; j < n_old; j += SG_THREADS) {
        old_id[j] = o_sid[j];
        keep[j] = a.frame_id - r_last[o_slot[j]] <= a.max_gap ? 1 : 0;
    }
    for (int t = tid; t < np; t += SG_THREADS) { box[t] = a.box[po + t]; pid[t] = ids[src[t]]; }
    // ---- 1. blind tracks (one wave per descriptor), rows ----
    for (int t = wave; t < np; t += SG_WAVES) {
        const int v = lane < SG_WORDS ? ((const int32_t *)(desc + (size_t)t * APP_DIM))[lane] : 0;
        const bool any = __ballot(v != 0) != 0ull;
        if (lane == 0) flags[t] = any ? 0 : SG_BLIND;
    }
    __syncthreads();
    for (int t = tid; t < np; t += SG_THREADS) {
        const int64_t id = pid[t];
        const int j = lower_bound_i64(old_id, n_old, id);
        const bool hit = j < n_old && old_id[j] == id;
        slot[t] = hit && keep[j] ? o_slot[j] : -1;          // a row that has expired is not this track's row either
        if (hit) keep[j] = 0;                              // a matched row is no idle row
    }
    // ---- 2. partner and contact ----
    for (int t = tid; t < np; t += SG_THREADS) {
        const float4 b = box[t];
        float best = -__builtin_huge_valf();
        int bj = -1;
        for (int j = 0; j < np; ++j) {
            if (j == t) continue;
            const float v = iou_ref(b, box[j]);
            if (v > best) { best = v; bj = j; }
        }
        partner[t] = bj;
        if (bj >= 0 && best > a.contact_iou) flags[t] |= SG_CONTACT;
    }
    __syncthreads();
    // ---- 3. candidate pairs: everything but the similarities, by the lower track ----
    for (int t = tid; t < np; t += SG_THREADS) {
        int u = -1;
        const int s = slot[t];
        if (s >= 0 && flags[t] == 0) {
            const int64_t B = r_cid[s];
            if (B >= 0) {
                int j = -1;
                for (int k = t + 1; k < np; ++k)
                    if (pid[k] == B) { j = k; break; }
                if (j >= 0) {
                    const int sj = slot[j];
                    if (sj >= 0 && flags[j] == 0 && r_cid[sj] == pid[t] && a.frame_id - r_cframe[s] <= a.window && a.frame_id - r_cframe[sj] <= a.window &&
                        r_count[s] >= a.min_history && r_count[sj] >= a.min_history)
                        u = j;
                }
            }
        }
        cand[t] = u;
    }
    __syncthreads();
    // the similarities: one wave per pair, lane l takes bins l, l + 64, l + 128
    int32_t *sims = a.sims + po * 4;
    for (int t = wave; t < np; t += SG_WAVES) {
        const int u = cand[t];
        if (u < 0) continue;                               // wave-uniform
        const int sa = slot[t], sb = slot[u];
        const int ca = min(r_count[sa], H), cb = min(r_count[sb], H);
        const int8_t *qi = desc + (size_t)t * APP_DIM, *qj = desc + (size_t)u * APP_DIM;
        const int8_t *ra = r_ring + (size_t)sa * H * APP_DIM, *rb = r_ring + (size_t)sb * H * APP_DIM;
        int dAA = 0, dAB = 0, dBB = 0, dBA = 0, nqi = 0, nqj = 0, nra = 0, nrb = 0;
#pragma unroll
        for (int k = 0; k < APP_DIM / 64; ++k) {
            const int d = lane + 64 * k;
            const int vi = qi[d], vj = qj[d];
            int va = 0, vb = 0;
            for (int h = 0; h < ca; ++h) va += ra[h * APP_DIM + d];
            for (int h = 0; h < cb; ++h) vb += rb[h * APP_DIM + d];
            dAA += vi * va; dAB += vi * vb; dBB += vj * vb; dBA += vj * va;
            nqi += vi * vi; nqj += vj * vj; nra += va * va; nrb += vb * vb;
        }
        dAA = sg_wave_sum(dAA); dAB = sg_wave_sum(dAB); dBB = sg_wave_sum(dBB); dBA = sg_wave_sum(dBA);
        nqi = sg_wave_sum(nqi); nqj = sg_wave_sum(nqj); nra = sg_wave_sum(nra); nrb = sg_wave_sum(nrb);
        if (lane == 0) {
            const int sAA = sg_sim(dAA, nqi, nra), sAB = sg_sim(dAB, nqi, nrb), sBB = sg_sim(dBB, nqj, nrb), sBA = sg_sim(dBA, nqj, nra);
            if (sAB >= a.min_sim && sBA >= a.min_sim && sAB >= sAA + a.min_gain && sBA >= sBB + a.min_gain) {
                sims[4 * t] = sAA; sims[4 * t + 1] = sAB; sims[4 * t + 2] = sBB; sims[4 * t + 3] = sBA;
            } else {
                cand[t] = -1;
            }
        }
    }
    __syncthreads();
    // ---- 4. the reverts, events in ascending track ----
    rtmodt_swap_event *evs = a.ev + (size_t)sidx * a.max_events;
    int n_rev = 0;
    for (int base = 0; base < np; base += SG_THREADS) {
        const int t = base + tid;
        const int u = t < np ? cand[t] : -1;
        int tot;
        const int pos = n_rev + block_scan_count<SG_WAVES>(u >= 0 ? 1 : 0, wsum, tot);
        if (u >= 0) {                                      // t and u are in no other pair: nobody else touches their cells
            const int64_t A = pid[t], B = pid[u];
            const int st = slot[t], su = slot[u];
            if (pos < a.max_events) {
                rtmodt_swap_event r;
                r.frame_id = a.frame_id; r.id_a = A; r.id_b = B; r.track_a = src[t]; r.track_b = src[u];
                r.sims[0] = sims[4 * t]; r.sims[1] = sims[4 * t + 1]; r.sims[2] = sims[4 * t + 2]; r.sims[3] = sims[4 * t + 3];
                evs[pos] = r;
            }
            pid[t] = B; pid[u] = A;
            ids[src[t]] = B; ids[src[u]] = A;
            r_cid[st] = -1; r_cid[su] = -1;
            slot[t] = su; slot[u] = st;                    // each track goes on with the row of the id it now carries
        }
        n_rev += tot;
    }
    __syncthreads();
    // ---- 5. the new index (passed rows + idle rows that stay, merged by rank) and the rows' update ----
    for (int t = tid; t < np; t += SG_THREADS) {
        const int64_t id = pid[t];
        int r = 0;
        for (int j = 0; j < np; ++j) r += pid[j] < id ? 1 : 0;
        rank[t] = r;
        spid[r] = id;
    }
    int n_ret = 0;
    for (int base = 0; base < n_old; base += SG_THREADS) {                    // flags -> exclusive prefix, in place
        const int j = base + tid;
        const int f = j < n_old ? keep[j] : 0;
        int tot;
        const int pos = block_scan_count<SG_WAVES>(f, wsum, tot);
        if (j < n_old) keep[j] = f ? n_ret + pos : -(n_ret + pos) - 1;         // stays: its rank; dropped: -(rank of the next that stays) - 1
        n_ret += tot;
    }
    if (tid == 0) keep[n_old] = -n_ret - 1;
    const bool overflow = np + n_ret > cap;                                   // keep this frame's rows, drop the idle ones
    for (int k = tid; k < cap; k += SG_THREADS) used[k] = 0;
    __syncthreads();
    for (int t = tid; t < np; t += SG_THREADS)
        if (slot[t] >= 0) used[slot[t]] = 1;
    if (!overflow)
        for (int j = tid; j < n_old; j += SG_THREADS)
            if (keep[j] >= 0) used[o_slot[j]] = 1;
    __syncthreads();
    int n_free = 0;
    for (int base = 0; base < cap; base += SG_THREADS) {                      // used flags -> the free slots, ascending, in place (entry <= index)
        const int k = base + tid;
        const int f = k < cap && !used[k] ? 1 : 0;
        int tot;
        const int pos = n_free + block_scan_count<SG_WAVES>(f, wsum, tot);
        if (f) used[pos] = k;
        n_free += tot;
    }
    __syncthreads();
    int n_new = 0;
    for (int base = 0; base < np; base += SG_THREADS) {                       // rows to create take the free slots in track order
        const int t = base + tid;
        const bool f = t < np && slot[t] < 0;
        int tot;
        const int pos = n_new + block_scan_count<SG_WAVES>(f ? 1 : 0, wsum, tot);
        if (f && pos < n_free) { slot[t] = used[pos]; flags[t] |= SG_NEW; }   // (pos < n_free always: rows after the frame <= cap)
        n_new += tot;
    }
    __syncthreads();
    for (int t = tid; t < np; t += SG_THREADS) {
        const int s = slot[t];
        int push = -1;
        if (s >= 0) {
            const int64_t id = pid[t];
            int below = 0;
            if (!overflow) { const int v = keep[lower_bound_i64(old_id, n_old, id)]; below = v >= 0 ? v : -v - 1; }
            const int at = rank[t] + below;
            n_sid[at] = id; n_slot[at] = s;
            int cnt = r_count[s], head = r_head[s];
            if (flags[t] & SG_NEW) { cnt = 0; head = 0; r_count[s] = 0; r_head[s] = 0; r_cframe[s] = 0; r_cid[s] = -1; }
            r_last[s] = a.frame_id;
            if (flags[t] & SG_CONTACT) {
                r_cframe[s] = a.frame_id;
                r_cid[s] = pid[partner[t]];
            } else if (!(flags[t] & SG_BLIND)) {
                head = head < 0 || head >= H ? 0 : head;
                push = head;
                r_head[s] = head + 1 == H ? 0 : head + 1;
                r_count[s] = cnt + 1 > H ? H : cnt + 1;
            }
        }
        cand[t] = push;
    }
    if (!overflow)
        for (int j = tid; j < n_old; j += SG_THREADS) {                       // idle rows: the index entry moves, the row stays in its slot
            const int v = keep[j];
            if (v < 0) continue;
            const int at = v + lower_bound_i64(spid, np, old_id[j]);
            n_sid[at] = old_id[j]; n_slot[at] = o_slot[j];
        }
    __syncthreads();
    for (int t = wave; t < np; t += SG_WAVES) {                               // the ring pushes, one wave per descriptor
        const int h = cand[t];
        if (h < 0) continue;
        if (lane < SG_WORDS)
            ((int32_t *)(r_ring + ((size_t)slot[t] * H + h) * APP_DIM))[lane] = ((const int32_t *)(desc + (size_t)t * APP_DIM))[lane];
    }
    if (tid == 0) {
        a.ev_n[sidx] = n_rev;
        meta[0] = nxt;
        meta[1] = np + (overflow ? 0 : n_ret);
        if (overflow) meta[2] = 1;
        meta[3] += n_rev;
    }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_swapguard : HandleBase {
    rtmodt_swapguard_cfg cfg{};
    int S = 1, Mc = 0, cap = 0, H = 0, max_events = 0;
    EventTimer<4> timer;
    char *pool = nullptr;                 // every device array below lives in this one allocation
    SgLedger *d_ledgers = nullptr;
    std::vector<SgLedger> h_ledgers;
    int64_t *d_meta = nullptr;
    int64_t *s_ids = nullptr; float4 *g_box = nullptr; int32_t *g_src = nullptr, *g_n = nullptr;
    int32_t *d_counts = nullptr; int8_t *d_desc = nullptr; int32_t *d_sims = nullptr;
    rtmodt_swap_event *ev = nullptr; int32_t *ev_n = nullptr;
    char *h_pin = nullptr;                // pinned mirror of the event block (records, counts per stream) + meta
    size_t ev_bytes = 0;
    FrameStage stage;                     // host frames are staged here
    std::vector<int32_t> iota;            // 0, 1, 2, ...: the host list is passed as it is
};

namespace {

// lays out every device array; base == nullptr -> size only
size_t sg_carve(rtmodt_swapguard *g, char *base) {
    Carver c{base};
    const size_t S = g->S, cap = g->cap, Mc = g->Mc, E = g->max_events, H = g->H;
    g->d_ledgers = c.take<SgLedger>(S);
    g->d_meta = c.take<int64_t>(S * 4);
    if (base) g->h_ledgers.assign(S, SgLedger{});
    for (size_t s = 0; s < S; ++s) {
        SgLedger L{};
        for (int b = 0; b < 2; ++b) { L.sid[b] = c.take<int64_t>(cap); L.sslot[b] = c.take<int32_t>(cap); }
        L.last = c.take<int64_t>(cap); L.cframe = c.take<int64_t>(cap); L.cid = c.take<int64_t>(cap);
        L.count = c.take<int32_t>(cap); L.head = c.take<int32_t>(cap);
        L.ring = c.take<int8_t>(cap * H * APP_DIM);
        if (base) g->h_ledgers[s] = L;
    }
    g->s_ids = c.take<int64_t>(S * Mc); g->g_box = c.take<float4>(S * Mc); g->g_src = c.take<int32_t>(S * Mc); g->g_n = c.take<int32_t>(S);
    g->d_counts = c.take<int32_t>(S * Mc * APP_DIM); g->d_desc = c.take<int8_t>(S * Mc * APP_DIM); g->d_sims = c.take<int32_t>(S * Mc * 4);
    const size_t ev0 = align_up(c.off, 16);
    g->ev = c.take<rtmodt_swap_event>(S * E); g->ev_n = c.take<int32_t>(S);
    g->ev_bytes = align_up(c.off, 16) - ev0;
    return align_up(c.off, 16);
}

size_t sg_smem(const rtmodt_swapguard *g) {
    const size_t capr = ((size_t)g->cap + 4) & ~(size_t)3, Mr = ((size_t)g->Mc + 3) & ~(size_t)3;
    return capr * 8 + Mr * 8 * 2 + Mr * 16 + capr * 4 * 2 + Mr * 4 * 5 + 16;
}

SgArgs sg_args(rtmodt_swapguard *g, int64_t frame_id) {
    SgArgs a{};
    a.ledgers = g->d_ledgers; a.meta = g->d_meta; a.cap = g->cap; a.Mc = g->Mc; a.history = g->H; a.min_history = g->cfg.min_history;
    a.min_sim = g->cfg.min_similarity_pm; a.min_gain = g->cfg.min_gain_pm; a.max_events = g->max_events; a.stream_base = 0;
    a.contact_iou = g->cfg.contact_iou; a.window = g->cfg.window; a.max_gap = g->cfg.max_gap_frames; a.frame_id = frame_id;
    a.box = g->g_box; a.src = g->g_src; a.n = g->g_n; a.desc = g->d_desc; a.sims = g->d_sims; a.ev = g->ev; a.ev_n = g->ev_n;
    return a;
}

// frames of a call -> device pointers (host frames are staged on stream q)
int sg_stage(rtmodt_swapguard *g, const uint8_t *const *frames, int count, int fh, int fw, int pitch, int mem_kind, hipStream_t q, AppFrames *out) {
    RT_TRY(check_frames(frames, count, fh, fw, pitch, mem_kind, kAppFrames));
    RT_TRY(g->stage.in(frames, count, fh, fw, pitch, mem_kind, q, FRAMES_AS_GIVEN));
    for (int i = 0; i < count; ++i) out->p[i] = g->stage.at(frames, i);
    return RTMODT_OK;
}

// describe + step for streams [s0, s0 + cnt) on stream q; the passed lists are in place
int sg_run(rtmodt_swapguard *g, SgArgs a, int s0, int cnt, int boxes, const AppFrames &fp, int fh, int fw, int pitch, hipStream_t q) {
    const size_t o = (size_t)s0 * g->Mc;
    RT_TRY(g->timer.record(1, q));
    DescribeArgs d{};
    d.frames = fp; d.h = fh; d.w = fw; d.pitch = pitch;
    d.box = g->g_box + o; d.box_n = g->g_n + s0; d.box_stride = g->Mc; d.max_boxes = boxes;
    d.counts = g->d_counts + o * APP_DIM; d.desc = g->d_desc + o * APP_DIM; d.desc_stride = g->Mc;
    RT_TRY(launch_describe(d, cnt, q));
    RT_TRY(g->timer.record(2, q));
    const size_t smem = sg_smem(g);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)swapguard_step, smem, seen));
    a.stream_base = s0;
    hipLaunchKernelGGL(swapguard_step, dim3(cnt), dim3(SG_THREADS), smem, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(g->timer.record(3, q));
    g->timer.timed = true;
    return RTMODT_OK;
}

// the event records, event counts and meta of streams [s0, s0 + cnt) -> pinned host mirror (same layout as the device block), then sync
struct SgEvHost { const rtmodt_swap_event *ev; const int32_t *n; const int64_t *meta; };
int sg_fetch(rtmodt_swapguard *g, hipStream_t q, int s0, int cnt, SgEvHost &h) {
    char *d0 = (char *)g->ev;
    const size_t rec0 = (size_t)s0 * g->max_events * sizeof(rtmodt_swap_event), n0 = (size_t)((const char *)(g->ev_n + s0) - d0);
    RT_HIP(hipMemcpyAsync(g->h_pin + rec0, d0 + rec0, (size_t)cnt * g->max_events * sizeof(rtmodt_swap_event), hipMemcpyDeviceToHost, q));
    RT_HIP(hipMemcpyAsync(g->h_pin + n0, d0 + n0, (size_t)cnt * 4, hipMemcpyDeviceToHost, q));
    RT_HIP(hipMemcpyAsync(g->h_pin + g->ev_bytes + (size_t)s0 * 32, g->d_meta + 4 * s0, sizeof(int64_t) * 4 * cnt, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    h.ev = (const rtmodt_swap_event *)g->h_pin;
    h.n = (const int32_t *)(g->h_pin + ((const char *)g->ev_n - d0));
    h.meta = (const int64_t *)(g->h_pin + g->ev_bytes);
    return RTMODT_OK;
}

int sg_check_sticky(rtmodt_swapguard *g, int s, int64_t err) {
    RT_CHECK(err != 1, RTMODT_E_CAPACITY, "swap guard stream %d: ledger full (%d rows): lower max_gap_frames or raise max_tracks", s, g->cap);
    RT_CHECK(err != 2, RTMODT_E_CAPACITY, "swap guard stream %d: more passed tracks than max_tracks %d", s, g->Mc);
    RT_CHECK(err == 0, RTMODT_E_INVALID, "swap guard stream %d: error %lld", s, (long long)err);
    return RTMODT_OK;
}

// copies the events of streams [s0, s0 + cnt) out; the first failure is reported after every stream has been copied
int sg_deliver(rtmodt_swapguard *g, const SgEvHost &h, int s0, int cnt, bool flat, rtmodt_swap_event *events, int32_t *n_events) {
    int rc = RTMODT_OK;
    for (int s = s0; s < s0 + cnt; ++s) {
        const int fired = h.n[s], ne = std::min(fired, g->max_events);
        const size_t eo = (size_t)s * g->max_events, dst = flat ? 0 : eo;
        if (events && ne > 0) memcpy(events + dst, h.ev + eo, sizeof(rtmodt_swap_event) * ne);
        n_events[flat ? 0 : s] = ne;
        if (rc == RTMODT_OK) rc = sg_check_sticky(g, s, h.meta[4 * s + 2]);
        if (rc == RTMODT_OK && fired > g->max_events)
            rc = fail(RTMODT_E_CAPACITY, "swap guard stream %d: %d reverts in one frame > max_events %d (every revert is applied, the events truncated)", s,
                      fired, g->max_events);
    }
    return rc;
}

// every _process* has synchronised the stream it launched on before it returned: the handle's own stream is all there is to wait for
int sg_sync_own(rtmodt_swapguard *g) {
    RT_HIP(hipSetDevice(g->device));
    RT_HIP(hipStreamSynchronize(g->stream));
    return RTMODT_OK;
}

}  // namespace

extern "C" {

void rtmodt_swapguard_destroy(rtmodt_swapguard *g) {
    if (!g) return;
    handle_close(g, [&] {
        g->timer.destroy();
        hipFree(g->pool); g->stage.release();
        hipHostFree(g->h_pin);
    });
    delete g;
}

int rtmodt_swapguard_create(const rtmodt_swapguard_cfg *cfg, rtmodt_swapguard **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(cfg->history >= 1 && cfg->history <= SG_MAX_HISTORY && cfg->min_history >= 1 && cfg->min_history <= cfg->history, RTMODT_E_INVALID,
             "history %d (1..%d) / min_history %d (1..history)", cfg->history, SG_MAX_HISTORY, cfg->min_history);
    RT_CHECK(cfg->window >= 0 && cfg->min_similarity_pm >= 0 && cfg->min_similarity_pm <= 1000 && cfg->min_gain_pm >= 0 && cfg->min_gain_pm <= 1000,
             RTMODT_E_INVALID, "window %d / min_similarity_pm %d / min_gain_pm %d out of range", cfg->window, cfg->min_similarity_pm, cfg->min_gain_pm);
    RT_CHECK(cfg->contact_iou == cfg->contact_iou, RTMODT_E_INVALID, "contact_iou is NaN");
    RT_CHECK(cfg->max_gap_frames >= 0, RTMODT_E_INVALID, "max_gap_frames %lld is negative", (long long)cfg->max_gap_frames);
    RT_CHECK(cfg->max_tracks >= 1 && cfg->max_tracks <= SG_MAX_TRACKS && cfg->n_streams >= 1 && cfg->n_streams <= SG_MAX_STREAMS && cfg->max_events >= 1 &&
                 cfg->max_events <= (1 << 20), RTMODT_E_INVALID, "max_tracks %d (1..%d) / n_streams %d (1..%d) / max_events %d out of range", cfg->max_tracks,
             SG_MAX_TRACKS, cfg->n_streams, SG_MAX_STREAMS, cfg->max_events);
    rtmodt_swapguard *g = new rtmodt_swapguard();
    g->cfg = *cfg;
    g->device = cfg->device; g->S = cfg->n_streams; g->Mc = cfg->max_tracks; g->cap = 2 * cfg->max_tracks; g->H = cfg->history; g->max_events = cfg->max_events;
    g->iota.resize(g->Mc);
    for (int i = 0; i < g->Mc; ++i) g->iota[i] = i;
    auto body = [&]() -> int {
        RT_CHECK(sg_smem(g) <= 150 * 1024, RTMODT_E_INVALID, "swap guard: capacity %d needs %zu B of LDS", g->cap, sg_smem(g));
        RT_TRY(handle_open(g));
        RT_TRY(g->timer.create());
        const size_t total = sg_carve(g, nullptr);
        RT_HIP(hipMalloc((void **)&g->pool, total));
        RT_HIP(handle_zero(g->pool, total, g->stream));
        sg_carve(g, g->pool);
        RT_HIP(hipHostMalloc((void **)&g->h_pin, g->ev_bytes + sizeof(int64_t) * 4 * g->S, hipHostMallocDefault));
        RT_HIP(hipMemcpyAsync(g->d_ledgers, g->h_ledgers.data(), sizeof(SgLedger) * g->S, hipMemcpyHostToDevice, g->stream));      // (behind the zeroing of the pool)
        return RTMODT_OK;
    };
    return handle_created(body(), g, rtmodt_swapguard_destroy, out);
}

int rtmodt_swapguard_process(rtmodt_swapguard *g, int stream, const int64_t *track_ids, const float *xyxy, int n, const uint8_t *frame, int h, int w,
                             int stride_bytes, int mem_kind, int64_t frame_id, int64_t *ids_out, rtmodt_swap_event *events, int32_t *n_events) {
    RT_CHECK(g && stream >= 0 && stream < g->S && n >= 0 && n_events, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n == 0 || (track_ids && xyxy && ids_out), RTMODT_E_INVALID, "null tracks");
    RT_CHECK(n <= g->Mc, RTMODT_E_CAPACITY, "%d tracks > max_tracks %d", n, g->Mc);
    std::vector<int64_t> sorted(track_ids, track_ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < n; ++i) RT_CHECK(sorted[i] != sorted[i - 1], RTMODT_E_INVALID, "track id %lld appears twice", (long long)sorted[i]);
    RT_HIP(hipSetDevice(g->device));
    hipStream_t q = g->stream;
    AppFrames fp{};
    RT_TRY(sg_stage(g, &frame, 1, h, w, stride_bytes, mem_kind, q, &fp));
    const size_t o = (size_t)stream * g->Mc;
    if (n) {
        RT_HIP(hipMemcpyAsync(g->s_ids + o, track_ids, (size_t)n * 8, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(g->g_box + o, xyxy, (size_t)n * 16, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(g->g_src + o, g->iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, q));
    }
    RT_HIP(hipMemcpyAsync(g->g_n + stream, &n, 4, hipMemcpyHostToDevice, q));
    RT_HIP(hipStreamSynchronize(q));                       // `n` and the caller's arrays are pageable
    SgArgs a = sg_args(g, frame_id);
    a.s_ids = g->s_ids;
    RT_TRY(g->timer.record(0, q));                 // (no gather on this path: the interval up to sg_run's first event is empty)
    RT_TRY(sg_run(g, a, stream, 1, n, fp, h, w, stride_bytes, q));
    if (n) RT_HIP(hipMemcpyAsync(ids_out, g->s_ids + o, (size_t)n * 8, hipMemcpyDeviceToHost, q));
    SgEvHost hst;
    RT_TRY(sg_fetch(g, q, stream, 1, hst));
    return sg_deliver(g, hst, stream, 1, true, events, n_events);
}

int rtmodt_swapguard_process_tracker(rtmodt_swapguard *g, rtmodt_tracker *trk, const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind,
                                     int64_t frame_id, int report_tsu, rtmodt_swap_event *events, int32_t *n_events) {
    RT_CHECK(g && trk && frames && n_events, RTMODT_E_INVALID, "bad argument");
    TrackerDeviceViewMut v;
    RT_TRY(tracker_device_view_mut(trk, &v));
    RT_CHECK(v.device == g->device, RTMODT_E_INVALID, "swap guard on device %d, tracker on device %d", g->device, v.device);
    RT_CHECK(v.n_streams <= g->S, RTMODT_E_INVALID, "tracker (%d streams) larger than the swap guard (%d)", v.n_streams, g->S);
    RT_HIP(hipSetDevice(g->device));
    hipStream_t q = v.stream;                              // the stream the tracker's last update ran on: ordered after it
    AppFrames fp{};
    RT_TRY(sg_stage(g, frames, v.n_streams, h, w, stride_bytes, mem_kind, q, &fp));
    RT_TRY(g->timer.record(0, q));
    SgGatherArgs ga{v.states, v.meta, v.max_tracks, report_tsu, g->Mc, g->g_box, g->g_src, g->g_n, g->d_meta};
    hipLaunchKernelGGL(swapguard_gather, dim3(v.n_streams), dim3(SG_THREADS), 0, q, ga);
    RT_HIP(hipGetLastError());
    SgArgs a = sg_args(g, frame_id);
    a.t_states = v.states; a.t_meta = v.meta;
    RT_TRY(sg_run(g, a, 0, v.n_streams, std::min(g->Mc, v.max_tracks), fp, h, w, stride_bytes, q));
    SgEvHost hst;
    RT_TRY(sg_fetch(g, q, 0, v.n_streams, hst));
    return sg_deliver(g, hst, 0, v.n_streams, false, events, n_events);
}

int rtmodt_swapguard_state(rtmodt_swapguard *g, int stream, int64_t *ids, int64_t *last_frame, int32_t *count, int64_t *contact_frame, int64_t *contact_id,
                           int8_t *ring, int32_t *n) {
    RT_CHECK(g && stream >= 0 && stream < g->S && n, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sg_sync_own(g));
    int64_t m[4];
    RT_HIP(hipMemcpy(m, g->d_meta + 4 * stream, sizeof(m), hipMemcpyDeviceToHost));
    RT_TRY(sg_check_sticky(g, stream, m[2]));
    const int cur = (int)m[0] & 1, rows = (int)m[1];
    RT_CHECK(rows >= 0 && rows <= g->cap, RTMODT_E_INVALID, "swap guard stream %d: corrupt row count", stream);
    *n = rows;
    if (!rows) return RTMODT_OK;
    const SgLedger &L = g->h_ledgers[stream];
    const size_t cap = g->cap, H = g->H, row_bytes = H * APP_DIM;
    std::vector<int64_t> sid(rows), last(cap), cframe(cap), cid(cap);
    std::vector<int32_t> sslot(rows), cnt(cap), head(cap);
    RT_HIP(hipMemcpy(sid.data(), L.sid[cur], (size_t)rows * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(sslot.data(), L.sslot[cur], (size_t)rows * 4, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(last.data(), L.last, cap * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(cframe.data(), L.cframe, cap * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(cid.data(), L.cid, cap * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(cnt.data(), L.count, cap * 4, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(head.data(), L.head, cap * 4, hipMemcpyDeviceToHost));
    std::vector<int8_t> rings;
    if (ring) {
        rings.resize(cap * row_bytes);
        RT_HIP(hipMemcpy(rings.data(), L.ring, rings.size(), hipMemcpyDeviceToHost));
        memset(ring, 0, (size_t)rows * row_bytes);
    }
    for (int r = 0; r < rows; ++r) {
        const int s = sslot[r];
        RT_CHECK(s >= 0 && s < g->cap && cnt[s] >= 0 && cnt[s] <= g->H && head[s] >= 0 && head[s] < g->H, RTMODT_E_INVALID, "swap guard stream %d: corrupt row %d",
                 stream, r);
        if (ids) ids[r] = sid[r];
        if (last_frame) last_frame[r] = last[s];
        if (count) count[r] = cnt[s];
        if (contact_frame) contact_frame[r] = cframe[s];
        if (contact_id) contact_id[r] = cid[s];
        if (ring) {
            const int c = cnt[s], first = c < g->H ? 0 : head[s];             // a full ring's oldest entry is the one written next
            for (int k = 0; k < c; ++k)
                memcpy(ring + (size_t)r * row_bytes + (size_t)k * APP_DIM, rings.data() + (size_t)s * row_bytes + (size_t)((first + k) % g->H) * APP_DIM, APP_DIM);
        }
    }
    return RTMODT_OK;
}

int rtmodt_swapguard_counts(rtmodt_swapguard *g, int stream, int64_t *n_reverted) {
    RT_CHECK(g && stream >= 0 && stream < g->S && n_reverted, RTMODT_E_INVALID, "bad argument");
    RT_TRY(sg_sync_own(g));
    RT_HIP(hipMemcpy(n_reverted, g->d_meta + 4 * stream + 3, 8, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_swapguard_last_ms(rtmodt_swapguard *g, float *describe_ms, float *step_ms) {
    RT_CHECK(g, RTMODT_E_INVALID, "null argument");
    float gather = 0.f, desc = 0.f, step = 0.f;
    RT_TRY(g->timer.elapsed(g->device, 2, 3, &step, "no call has been timed yet"));      // (the last event first: it waits for the call)
    RT_TRY(g->timer.elapsed(g->device, 0, 1, &gather, "no call has been timed yet"));
    RT_TRY(g->timer.elapsed(g->device, 1, 2, &desc, "no call has been timed yet"));
    if (describe_ms) *describe_ms = desc;
    if (step_ms) *step_ms = gather + step;
    return RTMODT_OK;
}

}  // extern "C"
