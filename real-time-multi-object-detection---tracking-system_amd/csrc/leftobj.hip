// leftobj.hip -- left and removed objects on the GPU: a second, slower model per stream on the motion detector's luma grid tells
// STATIC foreground (a bag that was put down, the hole where an exhibit stood) from moving foreground, a device-resident ledger
// follows each static region over time, and the tracks of the frame separate a left object from a person standing still.  The
// reference fires on tracked objects only (zone_engine.py) and has no counterpart; PARITY UNPINNED against any vendor's "left
// object" rule and against any default tuned on real footage.  tests/leftobj_ref.py restates every rule below and the kernels equal
// it exactly: all of it is integer arithmetic (a track's float box is rounded to integers once, leftobj_rule.h says how).
//
// Cell rule, kind, status, track tests, match and timers: leftobj_rule.h.  On top of them, per frame of a stream:
//   Mask.     n3 = the static cells in the 3 x 3 neighbourhood, the cell included, cells outside the grid counting 0;
//             mask = static && n3 >= min_neighbors.  No dilation.
//   Regions.  The 8-connected components of the mask with min_area <= area <= max_area cells, in the raster order of their first
//             cell; the first max_regions are stored, n_regions_total counts all of them.  At its root a region accumulates its
//             area, cell box, minimum and maximum age and the two edge sums cur and bgc (integer atomics, order-free).
//   Events.   At most 2 x max_objects per call: every old row can alarm, and the rows that alarm and are absorbed in the same call
//             make room for births that alarm at once (alarm_frames 1).
//   Ledger.   Per stream, rows sorted by oid, double-buffered, rebuilt by rank each call: the rows that stay keep their order, the
//             births of the call (regions no row matched, raster order) follow with the next oids.  A birth beyond max_objects is
//             dropped and counted.  oid counts from 1 per stream and is never reused.
//
// Kernels (256 threads; nine launches and one memset per call for all its streams, whatever the frames show; no grid-wide
// barrier, no spin on another workgroup, no floats but the one rounding of a track box):
//   leftobj_model   the hot path: every pixel is read once, by cell_grid.h's reader (its thread-to-run mapping and its dword path:
//                   every frame base and the pitch a multiple of 4).  A cell is read and written by one lane with one 8-byte access; the
//                   luma grid is written; the foreground cells are summed per wave and added with one atomic.
//   leftobj_filter  one workgroup per tile of 64 x 16 cells: static through LDS with a halo of 1, the 3 x 3 count; writes the mask,
//                   makes every mask cell its own union-find root with empty accumulators, adds n_static.
//   leftobj_link    union-find over the mask (ccl_dev.h); a cell looks at W, NW, N, NE and skips the links its neighbours make.
//   leftobj_roots   every mask cell adds its area, box, age and edge terms at its root; a wave whose mask cells share one root
//                   adds once.
//   leftobj_count   qualifying roots per chunk of 4096 cells.
//   leftobj_finish  one workgroup per stream: the exclusive scan of the chunk counts, the status, frames_seen (the device decides
//                   the restart after a SCENE_CHANGE: no host round trip).
//   leftobj_emit    a chunk that holds one of the first max_regions qualifying roots ranks them and writes their regions.
//   leftobj_step    one workgroup per stream: the track tests (strided over the tracks, regions in LDS), the match (one region at
//                   a time, the rows compete through one LDS maximum), the timers, the events, the retired list and the rank
//                   rebuild of the ledger through block_scan_count.
//   leftobj_absorb  walks the cells; a cell whose root an absorbed row names takes bg = cand, age = miss = 0.  A stream in which
//                   no row absorbed returns at once.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#define MO_HD __host__ __device__
#include "grid_host.h"
#include "kernels.h"
#include "track_layout.h"
#include "leftobj_rule.h"

namespace rtmodt {

#include "wg_dev.h"
#include "ccl_dev.h"
#include "track_select_dev.h"

constexpr int LO_THREADS = CG_THREADS, LO_WAVES = LO_THREADS / 64, LO_TW = GRID_TW, LO_TH = GRID_TH;
constexpr int LO_MAX_STREAMS = 1024;
constexpr long long LO_MAX_TOTAL_CELLS = 1LL << 28;
static_assert(sizeof(rtmodt_leftobj_result) == 48 && sizeof(rtmodt_leftobj_region) == 64 && sizeof(rtmodt_leftobj_object) == 72 &&
              sizeof(rtmodt_leftobj_event) == 56 && sizeof(rtmodt_leftobj_retired) == 16, "layout");

struct LoSlot { uint64_t frame; int64_t frame_id; int32_t stream, pad; };
struct LoWork { uint32_t n_fg, n_static; };
// at a root; the box as maxima of (gw - cx, gh - cy, cx + 1, cy + 1), the minimum age as the maximum of 65535 - age
struct LoAcc { uint32_t area, bx0, by0, bx1, by1, amin, amax, pad; unsigned long long cur, bgc; };
static_assert(sizeof(LoSlot) == 24 && sizeof(LoWork) == 8 && sizeof(LoAcc) == 48, "layout");

struct LoArgs {
    const LoSlot *slots;
    long long pitch, cells;                     // cells per stream
    int h, w, scale, gw, gh, tiles_x;           // tiles_x: of the launch at hand
    LoRule rule;
    int min_neighbors, scene_pm, min_area, max_area, max_regions, n_chunks;
    int max_objects, miss_frames, alarm_frames, absorb_frames, covered_pm, attend_margin;
    int n_owner, n_report, owner[LO_MAX_CLASSES], report[LO_MAX_CLASSES];
    uint64_t *state; int32_t *seen;             // the cells; frames_seen per stream
    uint8_t *luma, *mask;
    int32_t *parent; LoAcc *acc;
    LoWork *work; int32_t *absorbed;            // [n] each; absorbed: [n][1 + max_objects] = count, roots
    uint32_t *chunk;                            // [n][n_chunks + 1]
    char *blocks; size_t block_stride, off_regions, off_events, off_retired, off_objects;      // per frame of the call: result | regions | ...
    rtmodt_leftobj_object *ledger; int32_t *meta;      // [S][2][max_objects]; [S][4] = cur, rows, oids issued, 0
    // tracks: a staged list per frame of the call, or a tracker's device state (track_select_dev.h)
    int source, list_cap, trk_cap;
    const int64_t *l_ids; const float4 *l_box; const int32_t *l_cls; const int32_t *l_n;
    TrackSrc trk;
};

// ---- model: pixels -> cell luma (cell_grid.h) -> the 8-byte cell ---------------------------------------------------------------
template <int SCALE, bool WIDE> __global__ __launch_bounds__(LO_THREADS) void leftobj_model(LoArgs a) {
    constexpr int CPT = CgRun<SCALE>::CPT;
    const int tid = threadIdx.x;
    const LoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int seen = a.seen[sl.stream];
    const CgLane l = cg_lane<SCALE>(blockIdx.x, a.tiles_x, tid, (const uint8_t *)sl.frame, a.pitch, a.h, a.w, a.gw, a.gh);
    uint32_t n_fg = 0;
    if (l.live) {
        uint32_t sum[CPT];
        cg_read_run<SCALE, WIDE>(l.p, a.pitch, l.npx, l.nrows, sum);
        uint64_t *m = a.state + s_off + (size_t)l.cy * a.gw + l.cxb;
        uint8_t *lu = a.luma + s_off + (size_t)l.cy * a.gw + l.cxb;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            uint32_t yc;
            if (!cg_cell_luma<SCALE>(sum[j], l.cxb + j, l.nrows, a.w, yc)) continue;
            LoCell c = lo_unpack(m[j]);
            n_fg += lo_cell(a.rule, yc, seen, c) ? 1u : 0u;
            m[j] = lo_pack(c);
            lu[j] = (uint8_t)yc;
        }
    }
    n_fg = wave_sum_u32(n_fg);
    if ((tid & 63) == 0 && n_fg) atomicAdd(&a.work[blockIdx.y].n_fg, n_fg);
}

// ---- filter: static -> mask, n_static; mask cells become union-find roots ----------------------------------------------------
__global__ __launch_bounds__(LO_THREADS) void leftobj_filter(LoArgs a) {
    constexpr int LW = LO_TW + 2, LH = LO_TH + 2;
    __shared__ uint8_t s_st[LH][LW];
    const int tid = threadIdx.x;
    const LoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int tx0 = (int)(blockIdx.x % a.tiles_x) * LO_TW, ty0 = (int)(blockIdx.x / a.tiles_x) * LO_TH;
    for (int i = tid; i < LW * LH; i += LO_THREADS) {       // local (lx, ly) is cell (tx0 - 1 + lx, ty0 - 1 + ly)
        const int lx = i % LW, ly = i / LW, cx = tx0 - 1 + lx, cy = ty0 - 1 + ly;
        const bool in = cx >= 0 && cx < a.gw && cy >= 0 && cy < a.gh;
        s_st[ly][lx] = in && lo_static(a.rule, lo_unpack(a.state[s_off + (size_t)cy * a.gw + cx])) ? 1 : 0;
    }
    __syncthreads();
    const int lx = tid & 63, cx = tx0 + lx;
    uint32_t n_static = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, cy = ty0 + ly;
        if (cx >= a.gw || cy >= a.gh) continue;
        int n3 = 0;
#pragma unroll
        for (int dy = 0; dy <= 2; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2; ++dx) n3 += s_st[ly + dy][lx + dx];
        const bool m = s_st[ly + 1][lx + 1] && n3 >= a.min_neighbors;
        const size_t idx = (size_t)cy * a.gw + cx;
        a.mask[s_off + idx] = m ? 1 : 0;
        if (!m) continue;
        a.parent[s_off + idx] = (int32_t)idx;
        a.acc[s_off + idx] = LoAcc{};
        ++n_static;
    }
    n_static = wave_sum_u32(n_static);
    if ((tid & 63) == 0 && n_static) atomicAdd(&a.work[blockIdx.y].n_static, n_static);
}

// ---- labelling ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LO_THREADS) void leftobj_link(LoArgs a) {
    const LoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long idx = (long long)blockIdx.x * LO_THREADS + threadIdx.x;
    if (idx < a.cells) ccl_link_cell(a.mask + s_off, a.parent + s_off, a.gw, idx);
}

__global__ __launch_bounds__(LO_THREADS) void leftobj_roots(LoArgs a) {
    const LoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long idx = (long long)blockIdx.x * LO_THREADS + threadIdx.x;
    const bool m = idx < a.cells && a.mask[s_off + idx];
    int root = -1;
    uint32_t bx0 = 0, by0 = 0, bx1 = 0, by1 = 0, amin = 0, amax = 0, cur = 0, bgc = 0;
    if (m) {
        const int cx = (int)(idx % a.gw), cy = (int)(idx / a.gw);
        root = ccl_find(a.parent + s_off, (int)idx);
        bx0 = (uint32_t)(a.gw - cx); by0 = (uint32_t)(a.gh - cy); bx1 = (uint32_t)(cx + 1); by1 = (uint32_t)(cy + 1);
        const LoCell c = lo_unpack(a.state[s_off + idx]);
        amin = 65535u - c.age; amax = c.age;
        const int cand = (int)(c.cand >> 8), bg = (int)(c.bg >> 8);
        const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int nx = cx + dx[k], ny = cy + dy[k];
            if (nx < 0 || nx >= a.gw || ny < 0 || ny >= a.gh) continue;
            const size_t ni = s_off + (size_t)ny * a.gw + nx;
            if (a.mask[ni]) continue;
            cur += (uint32_t)lo_absdiff(cand, (int)a.luma[ni]);
            bgc += (uint32_t)lo_absdiff(bg, (int)(lo_unpack(a.state[ni]).bg >> 8));
        }
    }
    CclWave wv;
    if (!ccl_wave_roots(m, root, wv)) return;
    const uint32_t wx0 = wave_max_u32(bx0), wy0 = wave_max_u32(by0), wx1 = wave_max_u32(bx1), wy1 = wave_max_u32(by1);
    const uint32_t wmin = wave_max_u32(amin), wmax = wave_max_u32(amax), wcur = wave_sum_u32(cur), wbgc = wave_sum_u32(bgc);
    uint32_t n = 1;
    if (wv.same) {                                          // one add per wave
        if ((int)(threadIdx.x & 63) != wv.lead) return;
        n = wv.n; bx0 = wx0; by0 = wy0; bx1 = wx1; by1 = wy1; amin = wmin; amax = wmax; cur = wcur; bgc = wbgc;
    } else if (!m) {
        return;
    }
    LoAcc *r = a.acc + s_off + root;
    atomicAdd(&r->area, n);
    atomicMax(&r->bx0, bx0); atomicMax(&r->by0, by0); atomicMax(&r->bx1, bx1); atomicMax(&r->by1, by1);
    atomicMax(&r->amin, amin); atomicMax(&r->amax, amax);
    if (cur) atomicAdd(&r->cur, (unsigned long long)cur);
    if (bgc) atomicAdd(&r->bgc, (unsigned long long)bgc);
}

__device__ __forceinline__ bool lo_is_region(const LoArgs &a, size_t s_off, long long idx) {
    if (idx >= a.cells || !a.mask[s_off + idx] || a.parent[s_off + idx] != (int32_t)idx) return false;
    const uint32_t area = a.acc[s_off + idx].area;
    return area >= (uint32_t)a.min_area && area <= (uint32_t)a.max_area;
}

__global__ __launch_bounds__(LO_THREADS) void leftobj_count(LoArgs a) {
    __shared__ int s_wcnt[LO_WAVES];
    const size_t s_off = (size_t)a.slots[blockIdx.y].stream * (size_t)a.cells;
    ccl_count_chunk<LO_WAVES>(a.chunk + (size_t)blockIdx.y * (a.n_chunks + 1), s_wcnt, [&](long long idx) { return lo_is_region(a, s_off, idx); });
}

__global__ __launch_bounds__(LO_THREADS) void leftobj_finish(LoArgs a) {
    __shared__ int s_wcnt[LO_WAVES];
    const int slot = blockIdx.x;
    const uint32_t run = ccl_scan_chunks<LO_WAVES>(a.chunk + (size_t)slot * (a.n_chunks + 1), a.n_chunks, s_wcnt);
    if (threadIdx.x != 0) return;
    const LoSlot sl = a.slots[slot];
    const LoWork wk = a.work[slot];
    const int seen = a.seen[sl.stream];
    rtmodt_leftobj_result r{};
    r.status = lo_status(seen, a.rule.warmup, wk.n_fg, a.scene_pm, a.cells, run);
    r.stream = sl.stream;
    r.frames_seen = lo_next_seen(seen, r.status);
    r.n_fg = wk.n_fg; r.n_static = wk.n_static;
    r.n_regions_total = (int32_t)run;
    r.n_regions = (int32_t)min(run, (uint32_t)a.max_regions);
    *(rtmodt_leftobj_result *)(a.blocks + (size_t)slot * a.block_stride) = r;      // leftobj_step fills in the ledger's counts
    a.seen[sl.stream] = r.frames_seen;
}

__global__ __launch_bounds__(LO_THREADS) void leftobj_emit(LoArgs a) {
    __shared__ int s_wcnt[LO_WAVES];
    const size_t s_off = (size_t)a.slots[blockIdx.y].stream * (size_t)a.cells;
    rtmodt_leftobj_region *regs = (rtmodt_leftobj_region *)(a.blocks + (size_t)blockIdx.y * a.block_stride + a.off_regions);
    ccl_emit_chunk<LO_WAVES>(
        a.chunk + (size_t)blockIdx.y * (a.n_chunks + 1), a.max_regions, s_wcnt, [&](long long idx) { return lo_is_region(a, s_off, idx); },
        [&](long long idx, uint32_t pos) {
            const LoAcc c = a.acc[s_off + idx];
            rtmodt_leftobj_region g{};
            g.cells[0] = a.gw - (int)c.bx0; g.cells[1] = a.gh - (int)c.by0; g.cells[2] = (int)c.bx1 - 1; g.cells[3] = (int)c.by1 - 1;
            mo_px_box(g.cells[0], g.cells[1], g.cells[2], g.cells[3], a.scale, a.w, a.h, g.box);
            g.area = (int32_t)c.area;
            g.kind = lo_kind(c.cur, c.bgc);
            g.age_min = 65535 - (int32_t)c.amin; g.age_max = (int32_t)c.amax;
            g.root = (int32_t)idx;
            regs[pos] = g;
        });
}

// ---- the ledger ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lo_listed(const int32_t *list, int n, int k) {
    bool f = false;
    for (int q = 0; q < n; ++q) f = f || list[q] == k;
    return f;
}

__global__ __launch_bounds__(LO_THREADS) void leftobj_step(LoArgs a) {
    __shared__ int4 s_ocell[LO_MAX_OBJECTS], s_rcell[LO_MAX_REGIONS], s_rpx[LO_MAX_REGIONS];
    __shared__ int s_old_match[LO_MAX_OBJECTS], s_reg_match[LO_MAX_REGIONS], s_cov[LO_MAX_REGIONS], s_att[LO_MAX_REGIONS];
    __shared__ long long s_owner[LO_MAX_REGIONS];
    __shared__ unsigned long long s_best;
    __shared__ int s_wcnt[LO_WAVES], s_nabs;

    const int tid = threadIdx.x, slot = blockIdx.x;
    const LoSlot sl = a.slots[slot];
    const int MO = a.max_objects;
    char *blk = a.blocks + (size_t)slot * a.block_stride;
    rtmodt_leftobj_result *res = (rtmodt_leftobj_result *)blk;
    rtmodt_leftobj_region *regs = (rtmodt_leftobj_region *)(blk + a.off_regions);
    rtmodt_leftobj_event *evs = (rtmodt_leftobj_event *)(blk + a.off_events);
    rtmodt_leftobj_retired *ret = (rtmodt_leftobj_retired *)(blk + a.off_retired);
    rtmodt_leftobj_object *objs = (rtmodt_leftobj_object *)(blk + a.off_objects);
    int32_t *absorbed = a.absorbed + (size_t)slot * (1 + MO);
    int32_t *meta = a.meta + (size_t)sl.stream * 4;
    const int cur = meta[0] & 1, nxt = cur ^ 1;
    const int n_old = min(max(meta[1], 0), MO), issued = meta[2];
    const rtmodt_leftobj_object *old = a.ledger + ((size_t)sl.stream * 2 + cur) * MO;
    rtmodt_leftobj_object *nw = a.ledger + ((size_t)sl.stream * 2 + nxt) * MO;
    const int status = res->status;
    const int R = min(max(res->n_regions, 0), a.max_regions);

    s_cov[tid] = 0; s_att[tid] = 0; s_owner[tid] = LLONG_MIN; s_old_match[tid] = -1; s_reg_match[tid] = -1;
    if (tid == 0) s_nabs = 0;
    if (tid < n_old) s_ocell[tid] = make_int4(old[tid].cells[0], old[tid].cells[1], old[tid].cells[2], old[tid].cells[3]);
    if (tid < R) {
        s_rcell[tid] = make_int4(regs[tid].cells[0], regs[tid].cells[1], regs[tid].cells[2], regs[tid].cells[3]);
        s_rpx[tid] = make_int4(regs[tid].box[0], regs[tid].box[1], regs[tid].box[2], regs[tid].box[3]);
    }
    __syncthreads();

    if (status == LO_SCENE_CHANGE) {                        // (uniform) every row retires; no region is matched or born
        if (tid < n_old) {
            rtmodt_leftobj_retired r{old[tid].oid, LO_RESET, old[tid].alarmed, 0};
            ret[tid] = r;
        }
        if (tid == 0) {
            meta[0] = nxt; meta[1] = 0;
            res->n_objects = 0; res->n_events = 0; res->n_retired = n_old; res->dropped = 0; res->next_oid = issued + 1;
        }
        return;
    }

    // ---- 1. the tracks against every stored region ----
    if (a.source != RTMODT_LEFTOBJ_TRACKS_NONE && R > 0) {
        TrackSel src;
        int cap = a.trk_cap;
        if (a.source == RTMODT_LEFTOBJ_TRACKS_LIST) {
            const size_t o = (size_t)slot * a.list_cap;
            src = select_list(a.l_ids + o, a.l_box + o, a.l_cls + o, a.l_n[slot]);
            cap = a.list_cap;
        } else src = select_tracks(a.trk, sl.stream);
        const int n_t = src.n < 0 ? 0 : (src.n > cap ? cap : src.n);
        for (int i = tid; i < n_t; i += LO_THREADS) {
            if (!selected(src, i)) continue;
            const float4 b = src.box[i];
            int32_t tb[4];
            if (!lo_track_box(b.x, b.y, b.z, b.w, tb)) continue;
            const int k = src.cls[i];
            const bool owner = lo_listed(a.owner, a.n_owner, k), report = lo_listed(a.report, a.n_report, k);
            const long long id = src.ids[i];
            for (int r = 0; r < R; ++r) {
                const int4 q = s_rpx[r];
                const int32_t rp[4] = {q.x, q.y, q.z, q.w};
                if (lo_covered(tb, rp, a.covered_pm)) atomicOr(&s_cov[r], report ? 3 : 1);
                if (owner && lo_attended(tb, rp, a.attend_margin)) {
                    atomicOr(&s_att[r], 1);
                    __hip_atomic_fetch_max(&s_owner[r], id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }
    __syncthreads();

    // ---- 2. the match: regions in raster order, the free rows compete through one maximum ----
    for (int r = 0; r < R; ++r) {                           // (R is uniform)
        if (tid == 0) s_best = 0;
        __syncthreads();
        if (tid < n_old && s_old_match[tid] < 0) {
            const int4 o = s_ocell[tid], q = s_rcell[r];
            const int32_t oc[4] = {o.x, o.y, o.z, o.w}, rc[4] = {q.x, q.y, q.z, q.w};
            const int64_t sh = lo_shared_cells(oc, rc);
            if (sh > 0) atomicMax(&s_best, (unsigned long long)sh << 16 | (unsigned long long)(0xffff - tid));
        }
        __syncthreads();
        const unsigned long long best = s_best;
        if (best && tid == 0) {
            const int j = 0xffff - (int)(best & 0xffffu);
            s_old_match[j] = r; s_reg_match[r] = j;
        }
        __syncthreads();
    }

    // ---- 3. the old rows: timers, retirement, rank among the rows that stay ----
    rtmodt_leftobj_object e{};
    int keep = 0, gone = 0, fired = 0, reason = 0;
    if (tid < n_old) {
        e = old[tid];
        const int r = s_old_match[tid];
        keep = 1;
        if (r >= 0) {
            LoTimer t{e.idle, e.kind, e.alarmed, e.owner};
            fired = lo_timer(t, regs[r].kind, s_att[r] != 0, s_owner[r], (s_cov[r] & 1) != 0, (s_cov[r] & 2) != 0, a.alarm_frames) ? 1 : 0;
            e.idle = t.idle; e.kind = t.kind; e.alarmed = t.alarmed; e.owner = t.owner;
            e.unmatched = 0; e.area = regs[r].area;
            for (int k = 0; k < 4; ++k) { e.cells[k] = regs[r].cells[k]; e.box[k] = regs[r].box[k]; }
            regs[r].oid = e.oid;
            if (lo_absorbs(sl.frame_id, e.first_frame, a.absorb_frames)) {
                keep = 0; reason = LO_ABSORBED;
                absorbed[1 + atomicAdd(&s_nabs, 1)] = regs[r].root;
            }
        } else {
            e.unmatched += 1;
            if (e.unmatched > a.miss_frames) { keep = 0; reason = LO_CLEARED; }
        }
        gone = keep ^ 1;
    }
    int n_keep, n_gone, n_ev;
    const int p_keep = block_scan_count<LO_WAVES>(keep, s_wcnt, n_keep);
    const int p_gone = block_scan_count<LO_WAVES>(gone, s_wcnt, n_gone);
    const int p_ev = block_scan_count<LO_WAVES>(fired, s_wcnt, n_ev);
    if (keep) { nw[p_keep] = e; objs[p_keep] = e; }
    if (gone) {
        rtmodt_leftobj_retired r{e.oid, reason, e.alarmed, 0};
        ret[p_gone] = r;
    }
    if (fired) {
        rtmodt_leftobj_event v{e.first_frame, sl.frame_id, e.owner, e.oid, e.kind, e.area, 0, {e.box[0], e.box[1], e.box[2], e.box[3]}};
        evs[p_ev] = v;
    }

    // ---- 4. the births: the regions no row matched, in raster order, while the ledger has room ----
    const bool born = tid < R && s_reg_match[tid] < 0;
    int n_born, n_ev2;
    const int rank = block_scan_count<LO_WAVES>(born ? 1 : 0, s_wcnt, n_born);
    const int room = MO - n_keep;
    const bool accepted = born && rank < room;
    rtmodt_leftobj_object f{};
    int fired2 = 0;
    if (accepted) {
        f.first_frame = sl.frame_id; f.owner = -1; f.oid = issued + 1 + rank;
        LoTimer t{0, LO_UNKNOWN, 0, -1};
        fired2 = lo_timer(t, regs[tid].kind, s_att[tid] != 0, s_owner[tid], (s_cov[tid] & 1) != 0, (s_cov[tid] & 2) != 0, a.alarm_frames) ? 1 : 0;
        f.idle = t.idle; f.kind = t.kind; f.alarmed = t.alarmed; f.owner = t.owner;
        f.area = regs[tid].area;
        for (int k = 0; k < 4; ++k) { f.cells[k] = regs[tid].cells[k]; f.box[k] = regs[tid].box[k]; }
        regs[tid].oid = f.oid;
        nw[n_keep + rank] = f; objs[n_keep + rank] = f;
    }
    if (tid < R) { regs[tid].covered = s_cov[tid]; regs[tid].attended = s_att[tid]; }
    const int p_ev2 = n_ev + block_scan_count<LO_WAVES>(fired2, s_wcnt, n_ev2);
    if (fired2) {
        rtmodt_leftobj_event v{f.first_frame, sl.frame_id, f.owner, f.oid, f.kind, f.area, 0, {f.box[0], f.box[1], f.box[2], f.box[3]}};
        evs[p_ev2] = v;
    }
    __syncthreads();                                        // (s_nabs is complete)
    if (tid == 0) {
        const int n_acc = min(n_born, max(room, 0));
        meta[0] = nxt; meta[1] = n_keep + n_acc; meta[2] = issued + n_acc;
        res->n_objects = n_keep + n_acc; res->n_events = n_ev + n_ev2; res->n_retired = n_gone; res->dropped = n_born - n_acc;
        res->next_oid = issued + n_acc + 1;
        absorbed[0] = s_nabs;
    }
}

__global__ __launch_bounds__(LO_THREADS) void leftobj_absorb(LoArgs a) {
    const int32_t *absorbed = a.absorbed + (size_t)blockIdx.y * (1 + a.max_objects);
    const int n_abs = min(max(absorbed[0], 0), a.max_objects);
    if (n_abs == 0) return;                                 // (uniform)
    const LoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long idx = (long long)blockIdx.x * LO_THREADS + threadIdx.x;
    if (idx >= a.cells || !a.mask[s_off + idx]) return;
    const int root = ccl_find(a.parent + s_off, (int)idx);
    bool hit = false;
    for (int k = 0; k < n_abs; ++k) hit = hit || absorbed[1 + k] == root;
    if (!hit) return;
    LoCell c = lo_unpack(a.state[s_off + idx]);
    c.bg = c.cand; c.age = c.miss = 0;
    a.state[s_off + idx] = lo_pack(c);
}

// forgets `n` cells from `state` on but for their ignore bit
__global__ __launch_bounds__(LO_THREADS) void leftobj_clear(uint64_t *state, long long n) {
    const long long i = (long long)blockIdx.x * LO_THREADS + threadIdx.x;
    if (i < n) state[i] &= 1ull << 56;
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_leftobj : HandleBase {
    rtmodt_leftobj_cfg cfg{};
    GridGeom g;
    EventTimer<2> timer;
    uint64_t *d_state = nullptr;
    uint8_t *d_luma = nullptr, *d_mask = nullptr;
    int32_t *d_seen = nullptr, *d_parent = nullptr, *d_meta = nullptr;
    LoAcc *d_acc = nullptr;
    uint32_t *d_chunk = nullptr;
    rtmodt_leftobj_object *d_ledger = nullptr;
    char *d_out = nullptr, *h_out = nullptr;    // LoWork[S] | absorbed[S][1 + max_objects] | blocks[n]; the host mirror holds the blocks
    size_t off_abs = 0, off_blocks = 0, block_stride = 0, off_regions = 0, off_events = 0, off_retired = 0, off_objects = 0, out_bytes = 0;
    CmdBuf cmd;                         // slots | list counts | ids | boxes | classes (every call ends with a synchronize)
    FrameStage stage;
    std::vector<uint64_t> h_cells;      // set_ignore / read_ignore
};

namespace {

LoRule lo_rule(const rtmodt_leftobj_cfg &c) {
    return LoRule{c.warmup, c.warm_shift, c.learn_shift, c.threshold, c.stable, c.cand_shift, c.occlusion, c.static_frames};
}

int lo_check_rule(const rtmodt_leftobj_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null left-object config");
    RT_CHECK(c->warmup >= 1 && c->warmup <= 255, RTMODT_E_INVALID, "warmup %d outside 1..255", c->warmup);
    RT_CHECK(c->warm_shift >= 1 && c->warm_shift <= 8, RTMODT_E_INVALID, "warm_shift %d outside 1..8", c->warm_shift);
    RT_CHECK(c->learn_shift >= 1 && c->learn_shift <= 12, RTMODT_E_INVALID, "learn_shift %d outside 1..12", c->learn_shift);
    RT_CHECK(c->threshold >= 1 && c->threshold <= 255, RTMODT_E_INVALID, "threshold %d outside 1..255", c->threshold);
    RT_CHECK(c->stable >= 1 && c->stable <= 255, RTMODT_E_INVALID, "stable %d outside 1..255", c->stable);
    RT_CHECK(c->cand_shift >= 1 && c->cand_shift <= 8, RTMODT_E_INVALID, "cand_shift %d outside 1..8", c->cand_shift);
    RT_CHECK(c->occlusion >= 0 && c->occlusion <= 254, RTMODT_E_INVALID, "occlusion %d outside 0..254", c->occlusion);
    RT_CHECK(c->static_frames >= 1 && c->static_frames <= 65535, RTMODT_E_INVALID, "static_frames %d outside 1..65535", c->static_frames);
    return RTMODT_OK;
}

int lo_check_cfg(const rtmodt_leftobj_cfg *c) {
    RT_TRY(lo_check_rule(c));
    RT_TRY(check_grid_cfg(c->streams, c->height, c->width, c->scale, LO_MAX_STREAMS));
    RT_CHECK(c->min_neighbors >= 1 && c->min_neighbors <= 9, RTMODT_E_INVALID, "min_neighbors %d outside 1..9", c->min_neighbors);
    RT_CHECK(c->min_area >= 1 && c->max_area >= c->min_area, RTMODT_E_INVALID, "min_area %d / max_area %d: 1 <= min_area <= max_area", c->min_area,
             c->max_area);
    RT_CHECK(c->max_regions >= 1 && c->max_regions <= LO_MAX_REGIONS, RTMODT_E_INVALID, "max_regions %d outside 1..%d", c->max_regions, LO_MAX_REGIONS);
    RT_CHECK(c->scene_pm >= 1 && c->scene_pm <= 1000, RTMODT_E_INVALID, "scene_pm %d outside 1..1000", c->scene_pm);
    RT_CHECK(c->max_objects >= 1 && c->max_objects <= LO_MAX_OBJECTS, RTMODT_E_INVALID, "max_objects %d outside 1..%d", c->max_objects, LO_MAX_OBJECTS);
    RT_CHECK(c->miss_frames >= 0 && c->miss_frames <= 65535, RTMODT_E_INVALID, "miss_frames %d outside 0..65535", c->miss_frames);
    RT_CHECK(c->alarm_frames >= 1 && c->alarm_frames <= MO_MAX_SEEN, RTMODT_E_INVALID, "alarm_frames %d outside 1..2^30", c->alarm_frames);
    RT_CHECK(c->absorb_frames >= 0 && c->absorb_frames <= MO_MAX_SEEN, RTMODT_E_INVALID, "absorb_frames %d outside 0..2^30", c->absorb_frames);
    RT_CHECK(c->covered_pm >= 1 && c->covered_pm <= 1000, RTMODT_E_INVALID, "covered_pm %d outside 1..1000", c->covered_pm);
    RT_CHECK(c->attend_margin >= 0 && c->attend_margin <= 32768, RTMODT_E_INVALID, "attend_margin %d outside 0..32768", c->attend_margin);
    RT_CHECK(c->max_tracks >= 1 && c->max_tracks <= LO_MAX_TRACKS, RTMODT_E_INVALID, "max_tracks %d outside 1..%d", c->max_tracks, LO_MAX_TRACKS);
    RT_CHECK(c->n_owner_classes >= 0 && c->n_owner_classes <= LO_MAX_CLASSES && c->n_report_classes >= 0 && c->n_report_classes <= LO_MAX_CLASSES,
             RTMODT_E_INVALID, "n_owner_classes %d / n_report_classes %d outside 0..%d", c->n_owner_classes, c->n_report_classes, LO_MAX_CLASSES);
    return check_grid_cells(c->streams, c->height, c->width, c->scale, LO_MAX_TOTAL_CELLS);
}

void (*const lo_model_kernels[2][4])(LoArgs) = RTMODT_SCALE_KERNELS(leftobj_model);

int lo_sync(rtmodt_leftobj *p) {
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

// the tracker as the call's track source: its stream count must be the handle's; the launches are ordered after its last update (*after)
template <typename T> int lo_take_tracker(rtmodt_leftobj *p, void *trk, int report_tsu, LoArgs &a, hipStream_t *after) {
    TrackViewBase v;
    RT_TRY(track_src((T *)trk, report_tsu, &a.trk, &v));
    RT_CHECK(v.device == p->device, RTMODT_E_INVALID, "left-object detector on device %d, tracker on device %d", p->device, v.device);
    RT_CHECK(v.n_streams == p->cfg.streams, RTMODT_E_INVALID, "a tracker of %d streams, the left-object detector has %d", v.n_streams, p->cfg.streams);
    a.trk_cap = v.max_tracks; *after = v.stream;
    return RTMODT_OK;
}

}  // namespace

extern "C" {

void rtmodt_leftobj_default_cfg(rtmodt_leftobj_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_leftobj_cfg{};
    cfg->streams = 1; cfg->scale = 4; cfg->warmup = 8; cfg->warm_shift = 2; cfg->learn_shift = 6; cfg->threshold = 16; cfg->stable = 10;
    cfg->cand_shift = 3; cfg->occlusion = 50; cfg->static_frames = 100; cfg->min_neighbors = 4; cfg->min_area = 4; cfg->max_area = 1 << 24;
    cfg->max_regions = 32; cfg->scene_pm = 600; cfg->max_objects = 64; cfg->miss_frames = 50; cfg->alarm_frames = 250; cfg->absorb_frames = 0;
    cfg->covered_pm = 500; cfg->attend_margin = 32; cfg->max_tracks = 256; cfg->n_owner_classes = 1; cfg->owner_classes[0] = 0;
}

void rtmodt_leftobj_destroy(rtmodt_leftobj *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_state); hipFree(p->d_luma); hipFree(p->d_mask); hipFree(p->d_seen); hipFree(p->d_parent); hipFree(p->d_meta); hipFree(p->d_acc);
        hipFree(p->d_chunk); hipFree(p->d_ledger); hipFree(p->d_out);
        hipHostFree(p->h_out);
        p->cmd.release(); p->stage.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_leftobj_create(const rtmodt_leftobj_cfg *cfg, rtmodt_leftobj **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(lo_check_cfg(cfg));
    rtmodt_leftobj *p = new rtmodt_leftobj();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->g.set(cfg->height, cfg->width, cfg->scale);
    const size_t S = (size_t)cfg->streams, MO = (size_t)cfg->max_objects;
    p->off_abs = align_up(S * sizeof(LoWork), 16);
    p->off_blocks = align_up(p->off_abs + S * (1 + MO) * sizeof(int32_t), 16);
    p->off_regions = sizeof(rtmodt_leftobj_result);
    p->off_events = p->off_regions + (size_t)cfg->max_regions * sizeof(rtmodt_leftobj_region);
    p->off_retired = p->off_events + 2 * MO * sizeof(rtmodt_leftobj_event);      // a row that alarms and absorbs makes room for a birth that alarms
    p->off_objects = p->off_retired + MO * sizeof(rtmodt_leftobj_retired);
    p->block_stride = align_up(p->off_objects + MO * sizeof(rtmodt_leftobj_object), 16);
    p->out_bytes = p->off_blocks + S * p->block_stride;
    auto body = [&]() -> int {
        const size_t all = S * (size_t)p->g.cells;
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_state, all * sizeof(uint64_t)));
        RT_HIP(hipMalloc((void **)&p->d_luma, all));
        RT_HIP(hipMalloc((void **)&p->d_mask, all));
        RT_HIP(hipMalloc((void **)&p->d_parent, all * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_acc, all * sizeof(LoAcc)));
        RT_HIP(hipMalloc((void **)&p->d_chunk, S * (size_t)(p->g.n_chunks + 1) * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_seen, S * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_meta, S * 4 * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_ledger, S * 2 * MO * sizeof(rtmodt_leftobj_object)));
        RT_HIP(hipMalloc((void **)&p->d_out, p->out_bytes));
        RT_HIP(hipHostMalloc((void **)&p->h_out, S * p->block_stride, hipHostMallocDefault));
        RT_HIP(handle_zero(p->d_state, all * sizeof(uint64_t), p->stream));
        RT_HIP(handle_zero(p->d_luma, all, p->stream));
        RT_HIP(handle_zero(p->d_mask, all, p->stream));
        RT_HIP(handle_zero(p->d_seen, S * sizeof(int32_t), p->stream));
        RT_HIP(handle_zero(p->d_meta, S * 4 * sizeof(int32_t), p->stream));
        RT_HIP(handle_zero(p->d_ledger, S * 2 * MO * sizeof(rtmodt_leftobj_object), p->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_leftobj_destroy, out);
}

int rtmodt_leftobj_cell(const rtmodt_leftobj_cfg *cfg, uint32_t yc, int32_t frames_seen, uint64_t *state, int32_t *fg, int32_t *is_static) {
    RT_CHECK(state && fg && is_static, RTMODT_E_INVALID, "null argument");
    RT_TRY(lo_check_rule(cfg));
    RT_CHECK(yc <= 255 && frames_seen >= 0 && frames_seen <= MO_MAX_SEEN, RTMODT_E_INVALID, "cell luma %u, frames_seen %d", yc, frames_seen);
    const LoRule r = lo_rule(*cfg);
    LoCell c = lo_unpack(*state);
    *fg = lo_cell(r, yc, frames_seen, c) ? 1 : 0;
    *is_static = lo_static(r, c) ? 1 : 0;
    *state = lo_pack(c);
    return RTMODT_OK;
}

int rtmodt_leftobj_process(rtmodt_leftobj *p, const uint8_t *const *frames, const int32_t *streams, const int64_t *frame_ids, int n, int h, int w,
                           int stride_bytes, int mem_kind, const rtmodt_leftobj_tracks *tracks, const rtmodt_leftobj_out *out) {
    RT_CHECK(p && n >= 0 && (n == 0 || (frames && frame_ids)), RTMODT_E_INVALID, "null argument");
    RT_TRY(check_mem_kind(mem_kind));
    RT_CHECK(h == p->cfg.height && w == p->cfg.width, RTMODT_E_INVALID, "frames of %dx%d, the left-object detector was created for %dx%d", w, h,
             p->cfg.width, p->cfg.height);
    RT_CHECK(pitch_holds(stride_bytes, w), RTMODT_E_INVALID, "stride %d below 3 x %d", stride_bytes, w);
    const rtmodt_leftobj_cfg &c = p->cfg;
    const int S = c.streams, Mc = c.max_tracks;
    RT_TRY(check_stream_list(frames, streams, n, S));
    const int source = tracks ? tracks->source : RTMODT_LEFTOBJ_TRACKS_NONE;
    RT_CHECK(source >= RTMODT_LEFTOBJ_TRACKS_NONE && source <= RTMODT_LEFTOBJ_TRACKS_BOTSORT, RTMODT_E_INVALID, "track source %d", source);
    LoArgs a{};
    a.source = source;
    hipStream_t after = nullptr;                            // the tracker's stream
    if (source == RTMODT_LEFTOBJ_TRACKS_LIST) {
        RT_CHECK(tracks->n && tracks->stride >= 0, RTMODT_E_INVALID, "a track list without counts");
        for (int i = 0; i < n; ++i) {
            RT_CHECK(tracks->n[i] >= 0 && tracks->n[i] <= tracks->stride, RTMODT_E_INVALID, "frame %d: %d tracks in rows of %d", i, tracks->n[i], tracks->stride);
            RT_CHECK(tracks->n[i] <= Mc, RTMODT_E_INVALID, "frame %d: %d tracks > max_tracks %d", i, tracks->n[i], Mc);
            RT_CHECK(tracks->n[i] == 0 || (tracks->ids && tracks->xyxy && tracks->cls), RTMODT_E_INVALID, "null tracks");
        }
    } else if (source != RTMODT_LEFTOBJ_TRACKS_NONE) {
        RT_CHECK(tracks->tracker, RTMODT_E_INVALID, "null tracker");
        if (source == RTMODT_LEFTOBJ_TRACKS_BYTETRACK) RT_TRY(lo_take_tracker<rtmodt_tracker>(p, tracks->tracker, tracks->report_tsu, a, &after));
        else if (source == RTMODT_LEFTOBJ_TRACKS_DEEPSORT) RT_TRY(lo_take_tracker<rtmodt_deepsort>(p, tracks->tracker, tracks->report_tsu, a, &after));
        else if (source == RTMODT_LEFTOBJ_TRACKS_OCSORT) RT_TRY(lo_take_tracker<rtmodt_ocsort>(p, tracks->tracker, 0, a, &after));
        else RT_TRY(lo_take_tracker<rtmodt_botsort>(p, tracks->tracker, 0, a, &after));
    }
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    if (after && after != q) RT_HIP(hipStreamSynchronize(after));
    RT_TRY(p->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_AS_GIVEN));

    // the command block: slots | list counts | ids | boxes | classes
    const bool list = source == RTMODT_LEFTOBJ_TRACKS_LIST;
    const size_t o_n = align_up((size_t)n * sizeof(LoSlot), 16), o_ids = align_up(o_n + (size_t)n * 4, 16);
    const size_t o_box = o_ids + (list ? (size_t)n * Mc * 8 : 0), o_cls = o_box + (list ? (size_t)n * Mc * 16 : 0);
    const size_t cmd_bytes = o_cls + (list ? (size_t)n * Mc * 4 : 0);
    RT_TRY(p->cmd.reserve(cmd_bytes));
    memset(p->cmd.h, 0, cmd_bytes);
    LoSlot *sl = (LoSlot *)p->cmd.h;
    for (int i = 0; i < n; ++i) {
        sl[i] = LoSlot{(uint64_t)(uintptr_t)p->stage.at(frames, i), frame_ids[i], streams ? streams[i] : i, 0};
        if (!list) continue;
        const int m = tracks->n[i];
        ((int32_t *)(p->cmd.h + o_n))[i] = m;
        if (m == 0) continue;
        memcpy(p->cmd.h + o_ids + (size_t)i * Mc * 8, tracks->ids + (size_t)i * tracks->stride, (size_t)m * 8);
        memcpy(p->cmd.h + o_box + (size_t)i * Mc * 16, tracks->xyxy + (size_t)i * tracks->stride * 4, (size_t)m * 16);
        memcpy(p->cmd.h + o_cls + (size_t)i * Mc * 4, tracks->cls + (size_t)i * tracks->stride, (size_t)m * 4);
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, cmd_bytes, hipMemcpyHostToDevice, q));
    RT_TRY(p->stage.copy_in(frames, q));

    a.slots = (const LoSlot *)p->cmd.d;
    a.pitch = (long long)p->stage.pitch; a.cells = p->g.cells;
    a.h = h; a.w = w; a.scale = c.scale; a.gw = p->g.gw; a.gh = p->g.gh;
    a.rule = lo_rule(c);
    a.min_neighbors = c.min_neighbors; a.scene_pm = c.scene_pm; a.min_area = c.min_area; a.max_area = c.max_area; a.max_regions = c.max_regions;
    a.n_chunks = p->g.n_chunks;
    a.max_objects = c.max_objects; a.miss_frames = c.miss_frames; a.alarm_frames = c.alarm_frames; a.absorb_frames = c.absorb_frames;
    a.covered_pm = c.covered_pm; a.attend_margin = c.attend_margin;
    a.n_owner = c.n_owner_classes; a.n_report = c.n_report_classes;
    for (int k = 0; k < LO_MAX_CLASSES; ++k) { a.owner[k] = c.owner_classes[k]; a.report[k] = c.report_classes[k]; }
    a.state = p->d_state; a.seen = p->d_seen; a.luma = p->d_luma; a.mask = p->d_mask; a.parent = p->d_parent; a.acc = p->d_acc;
    a.work = (LoWork *)p->d_out; a.absorbed = (int32_t *)(p->d_out + p->off_abs); a.chunk = p->d_chunk;
    a.blocks = p->d_out + p->off_blocks; a.block_stride = p->block_stride;
    a.off_regions = p->off_regions; a.off_events = p->off_events; a.off_retired = p->off_retired; a.off_objects = p->off_objects;
    a.ledger = p->d_ledger; a.meta = p->d_meta;
    a.list_cap = Mc;
    if (list) {
        a.l_n = (const int32_t *)(p->cmd.d + o_n); a.l_ids = (const int64_t *)(p->cmd.d + o_ids);
        a.l_box = (const float4 *)(p->cmd.d + o_box); a.l_cls = (const int32_t *)(p->cmd.d + o_cls);
    }

    const dim3 block(LO_THREADS);
    const GridGeom &g = p->g;
    const size_t blocks_bytes = (size_t)n * p->block_stride;
    RT_TRY(p->timer.record(0, q));
    RT_HIP(hipMemsetAsync(p->d_out, 0, p->off_blocks + blocks_bytes, q));
    LoArgs m = a;
    m.tiles_x = g.model_tiles_x();
    launch_by_scale(lo_model_kernels, c.scale, frames_wide(p->stage, sl, n), g.model_grid(n), q, m);
    LoArgs f = a;
    f.tiles_x = g.filter_tiles_x();
    hipLaunchKernelGGL(leftobj_filter, g.filter_grid(n), block, 0, q, f);
    hipLaunchKernelGGL(leftobj_link, g.per_cell(n), block, 0, q, a);
    hipLaunchKernelGGL(leftobj_roots, g.per_cell(n), block, 0, q, a);
    hipLaunchKernelGGL(leftobj_count, g.per_chunk(n), block, 0, q, a);
    hipLaunchKernelGGL(leftobj_finish, dim3(n), block, 0, q, a);
    hipLaunchKernelGGL(leftobj_emit, g.per_chunk(n), block, 0, q, a);
    hipLaunchKernelGGL(leftobj_step, dim3(n), block, 0, q, a);
    hipLaunchKernelGGL(leftobj_absorb, g.per_cell(n), block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    const bool any = out && (out->results || out->regions || out->events || out->retired || out->objects);
    if (any) RT_HIP(hipMemcpyAsync(p->h_out, p->d_out + p->off_blocks, blocks_bytes, hipMemcpyDeviceToHost, q));      // everything in one copy
    RT_HIP(hipStreamSynchronize(q));
    p->timer.timed = true;
    if (!any) return RTMODT_OK;
    const size_t MO = (size_t)c.max_objects, MR = (size_t)c.max_regions;
    for (int i = 0; i < n; ++i) {
        const char *blk = p->h_out + (size_t)i * p->block_stride;
        const rtmodt_leftobj_result r = *(const rtmodt_leftobj_result *)blk;
        if (out->results) out->results[i] = r;
        if (out->regions) memcpy(out->regions + i * MR, blk + p->off_regions, MR * sizeof(rtmodt_leftobj_region));
        if (out->events) memcpy(out->events + i * 2 * MO, blk + p->off_events, 2 * MO * sizeof(rtmodt_leftobj_event));
        if (out->retired) memcpy(out->retired + i * MO, blk + p->off_retired, MO * sizeof(rtmodt_leftobj_retired));
        if (out->objects) memcpy(out->objects + i * MO, blk + p->off_objects, MO * sizeof(rtmodt_leftobj_object));
    }
    return RTMODT_OK;
}

int rtmodt_leftobj_read_state(rtmodt_leftobj *p, int stream, uint64_t *cells, uint8_t *luma, int32_t *frames_seen) {
    RT_CHECK(p && frames_seen, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    if (cells) RT_HIP(hipMemcpyAsync(cells, p->d_state + (size_t)stream * p->g.cells, (size_t)p->g.cells * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
    if (luma) RT_HIP(hipMemcpyAsync(luma, p->d_luma + (size_t)stream * p->g.cells, (size_t)p->g.cells, hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(frames_seen, p->d_seen + stream, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_leftobj_load_state(rtmodt_leftobj *p, int stream, const uint64_t *cells, const uint8_t *luma, int32_t frames_seen) {
    RT_CHECK(p && cells && luma, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_CHECK(frames_seen >= 0 && frames_seen <= MO_MAX_SEEN, RTMODT_E_INVALID, "frames_seen %d outside 0..%d", frames_seen, MO_MAX_SEEN);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_state + (size_t)stream * p->g.cells, cells, (size_t)p->g.cells * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_luma + (size_t)stream * p->g.cells, luma, (size_t)p->g.cells, hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_seen + stream, &frames_seen, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_leftobj_read_mask(rtmodt_leftobj *p, int stream, uint8_t *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(out, p->d_mask + (size_t)stream * p->g.cells, (size_t)p->g.cells, hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_leftobj_load_mask(rtmodt_leftobj *p, int stream, const uint8_t *mask) {
    RT_CHECK(p && mask, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    for (long long i = 0; i < p->g.cells; ++i) RT_CHECK(mask[i] <= 1, RTMODT_E_INVALID, "mask cell %lld is %d (0 or 1)", i, (int)mask[i]);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_mask + (size_t)stream * p->g.cells, mask, (size_t)p->g.cells, hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_leftobj_read_ledger(rtmodt_leftobj *p, int stream, rtmodt_leftobj_object *objects, int32_t *n, int32_t *next_oid) {
    RT_CHECK(p && n && next_oid, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_TRY(lo_sync(p));
    int32_t m[4];
    RT_HIP(hipMemcpy(m, p->d_meta + 4 * stream, sizeof(m), hipMemcpyDeviceToHost));
    RT_CHECK(m[1] >= 0 && m[1] <= p->cfg.max_objects, RTMODT_E_INVALID, "left-object stream %d: corrupt row count", stream);
    *n = m[1]; *next_oid = m[2] + 1;
    if (objects && m[1])
        RT_HIP(hipMemcpy(objects, p->d_ledger + ((size_t)stream * 2 + (m[0] & 1)) * p->cfg.max_objects, (size_t)m[1] * sizeof(rtmodt_leftobj_object),
                         hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_leftobj_load_ledger(rtmodt_leftobj *p, int stream, const rtmodt_leftobj_object *objects, int n, int32_t next_oid) {
    RT_CHECK(p && (objects || n == 0), RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_CHECK(n >= 0 && n <= p->cfg.max_objects && next_oid >= 1, RTMODT_E_INVALID, "%d rows (0..%d), next oid %d (>= 1)", n, p->cfg.max_objects, next_oid);
    for (int i = 0; i < n; ++i)
        RT_CHECK(objects[i].oid >= 1 && objects[i].oid < next_oid && (i == 0 || objects[i].oid > objects[i - 1].oid), RTMODT_E_INVALID,
                 "row %d: oid %d (ascending, 1..%d)", i, objects[i].oid, next_oid - 1);
    RT_TRY(lo_sync(p));
    const int32_t m[4] = {0, n, next_oid - 1, 0};
    if (n) RT_HIP(hipMemcpy(p->d_ledger + (size_t)stream * 2 * p->cfg.max_objects, objects, (size_t)n * sizeof(rtmodt_leftobj_object), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(p->d_meta + 4 * stream, m, sizeof(m), hipMemcpyHostToDevice));
    return RTMODT_OK;
}

int rtmodt_leftobj_set_ignore(rtmodt_leftobj *p, int stream, const uint8_t *grid) {
    RT_CHECK(p && grid, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_TRY(lo_sync(p));
    p->h_cells.resize((size_t)p->g.cells);
    uint64_t *d = p->d_state + (size_t)stream * p->g.cells;
    RT_HIP(hipMemcpy(p->h_cells.data(), d, (size_t)p->g.cells * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (long long i = 0; i < p->g.cells; ++i) p->h_cells[i] = (p->h_cells[i] & ~(1ull << 56)) | (grid[i] ? 1ull << 56 : 0);
    RT_HIP(hipMemcpy(d, p->h_cells.data(), (size_t)p->g.cells * sizeof(uint64_t), hipMemcpyHostToDevice));
    return RTMODT_OK;
}

int rtmodt_leftobj_read_ignore(rtmodt_leftobj *p, int stream, uint8_t *grid) {
    RT_CHECK(p && grid, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_TRY(lo_sync(p));
    p->h_cells.resize((size_t)p->g.cells);
    RT_HIP(hipMemcpy(p->h_cells.data(), p->d_state + (size_t)stream * p->g.cells, (size_t)p->g.cells * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (long long i = 0; i < p->g.cells; ++i) grid[i] = (uint8_t)(p->h_cells[i] >> 56 & 1);
    return RTMODT_OK;
}

int rtmodt_leftobj_reset(rtmodt_leftobj *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    const size_t first = stream < 0 ? 0 : (size_t)stream, count = stream < 0 ? (size_t)p->cfg.streams : 1;
    const long long nc = (long long)count * p->g.cells;
    hipLaunchKernelGGL(leftobj_clear, dim3((unsigned)((nc + LO_THREADS - 1) / LO_THREADS)), dim3(LO_THREADS), 0, p->stream, p->d_state + first * p->g.cells, nc);
    RT_HIP(hipGetLastError());
    RT_HIP(hipMemsetAsync(p->d_luma + first * p->g.cells, 0, count * p->g.cells, p->stream));
    RT_HIP(hipMemsetAsync(p->d_mask + first * p->g.cells, 0, count * p->g.cells, p->stream));
    RT_HIP(hipMemsetAsync(p->d_seen + first, 0, count * sizeof(int32_t), p->stream));
    RT_HIP(hipMemsetAsync(p->d_meta + first * 4, 0, count * 4 * sizeof(int32_t), p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_leftobj_last_ms(rtmodt_leftobj *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

}  // extern "C"
