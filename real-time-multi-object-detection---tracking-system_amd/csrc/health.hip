// health.hip -- camera health on the GPU: is the picture a stream delivers still a valid picture of the scene the camera was aimed
// at?  Per stream a reference of the scene's coarse structure and fine detail, resident on the device, is compared with every frame
// and answers DARK, BRIGHT, COVERED, MOVED, DEFOCUSED and FROZEN, debounced into latched RAISED / CLEARED events
// (pipeline.run(health=...)).  The reference hands cap.read()'s frame on (rtsp_reader.py) and has no counterpart; PARITY UNPINNED
// against any camera's or NVR's tamper detection and against any default tuned on real footage.  tests/health_ref.py restates every
// rule in NumPy and the kernels equal it exactly: all of it is integer arithmetic, no float appears anywhere.
//
// Rules: health_rule.h (grid, pixel luma and cell luma: motion_model.h).  A stream holds R (uint16 8.8 per cell), the previous Y grid
// (uint8 per cell) and an HlState (ref_sharp, frames_seen, the active mask, owed events, a run and an off counter per condition).
//
// Kernels (256 threads; FOUR launches and one memset per call for all its streams, whatever the frames show; no grid-wide barrier,
// no spin on another workgroup; every sum is an integer sum, so its order cannot change a result):
//   health_pixels  the hot path: every pixel is read once, by cell_grid.h's reader (a thread owns a run of 4 / scale cells of one
//                  cell row; dwords where every frame base and the pitch are multiples of 4) with a visitor that sees each pixel's
//                  luma.  The fine-detail term of a run's last pixel needs the first luma of the run to
//                  its right: it comes from the next lane by a wave shuffle, and from memory (three bytes a row) only for lane 63,
//                  whose neighbour belongs to another wave or tile.  A cell's Y replaces the previous grid's in place (one lane
//                  reads and writes a cell), which gives n_changed.  luma_sum, sharp, n_dark, n_bright and n_changed are summed per
//                  wave, then per workgroup through LDS, and added with one integer atomic each.
//   health_edges   one workgroup per tile of 64 x 16 cells: Y through LDS with a one-cell halo, G per cell (written for the learn
//                  pass), n_edge, n_ref_edge and n_kept against R, summed the same way.
//   health_decide  one thread per stream of the call: hl_step -- the raw conditions, the debounce, the events, ref_sharp,
//                  frames_seen, the relearn -- and the result row.  The device decides; no host round trip.
//   health_learn   R takes the step health_decide chose (none, average, set), one cell per thread.
#include <algorithm>
#include <cstring>
#include <vector>

#define MO_HD __host__ __device__
#include "grid_host.h"
#include "health_rule.h"

namespace rtmodt {

#include "wg_dev.h"

constexpr int HL_THREADS = CG_THREADS, HL_WAVES = HL_THREADS / 64, HL_TW = GRID_TW, HL_TH = GRID_TH;
constexpr int HL_MAX_STREAMS = 1024;
constexpr long long HL_MAX_TOTAL_CELLS = 1LL << 28;
static_assert(sizeof(rtmodt_health_result) == 72 && sizeof(rtmodt_health_event) == 16, "layout");
static_assert(sizeof(rtmodt_health_state) == sizeof(HlState) && sizeof(HlState) == 72, "layout");
static_assert(RTMODT_HEALTH_MAX_EVENTS == HL_MAX_EVENTS && RTMODT_HEALTH_NO_STRUCTURE == HL_NO_STRUCTURE && RTMODT_HEALTH_FROZEN == HL_FROZEN, "constants");

struct HlSlot { uint64_t frame; int64_t frame_id; int32_t stream, pad; };
// the counters of one frame of a call, zeroed before the launches; learn: what health_decide chose for health_learn
struct HlWork { unsigned long long luma, sharp; uint32_t n_dark, n_bright, n_changed, n_edge, n_ref_edge, n_kept; int32_t learn, pad; };
static_assert(sizeof(HlSlot) == 24 && sizeof(HlWork) == 48, "layout");

struct HlArgs {
    const HlSlot *slots;
    long long pitch, cells;                     // cells per stream
    int n, h, w, gw, gh, tiles_x;               // tiles_x: of the launch at hand
    HlRule rule;
    uint16_t *r; uint8_t *y, *g;                // per stream and cell: the reference, the (previous) luma grid, this frame's G
    HlState *state;                             // per stream
    HlWork *work;
    rtmodt_health_result *res; rtmodt_health_event *events;     // [n], [n][HL_MAX_EVENTS]
};

// ---- pixels: cell luma (cell_grid.h), fine detail, the exposure counts, n_changed ---------------------------------------------
template <int SCALE, bool WIDE> __global__ __launch_bounds__(HL_THREADS) void health_pixels(HlArgs a) {
    constexpr int CPT = CgRun<SCALE>::CPT, PX = CgRun<SCALE>::PX, RUN = CgRun<SCALE>::RUN;
    __shared__ uint32_t s_part[HL_WAVES][5];
    const int tid = threadIdx.x, lane = tid & 63;
    const HlSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int seen = a.state[sl.stream].frames_seen;
    const CgLane l = cg_lane<SCALE>(blockIdx.x, a.tiles_x, tid, (const uint8_t *)sl.frame, a.pitch, a.h, a.w, a.gw, a.gh);
    uint32_t luma = 0, n_dark = 0, n_bright = 0, n_changed = 0, fine = 0;
    uint32_t first[SCALE], last[SCALE];                         // the luma of the run's first and last pixel, per pixel row
#pragma unroll
    for (int r = 0; r < SCALE; ++r) first[r] = last[r] = 0;
    if (l.live) {
        uint32_t sum[CPT];
        cg_read_run<SCALE, WIDE>(l.p, a.pitch, l.npx, l.nrows, sum, [&](int r, int i, uint32_t yv) {
            if (i) fine += hl_absdiff(yv, last[r]);                 // (last[r] is the pixel to the left until the row ends)
            else first[r] = yv;
            last[r] = yv;
        });
        uint8_t *yg = a.y + s_off + (size_t)l.cy * a.gw + l.cxb;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            uint32_t yc;
            if (!cg_cell_luma<SCALE>(sum[j], l.cxb + j, l.nrows, a.w, yc)) continue;
            const uint32_t old = yg[j];
            yg[j] = (uint8_t)yc;
            luma += yc;
            n_dark += yc <= (uint32_t)a.rule.dark_level ? 1u : 0u;
            n_bright += yc >= (uint32_t)a.rule.bright_level ? 1u : 0u;
            n_changed += seen == 0 || old != yc ? 1u : 0u;
        }
    }
    // the pixel right of the run: a full run that does not end the row has the next lane's first pixel (same cell row, so the same
    // rows), lane 63 reads it from memory
    const bool need = l.live && l.npx == PX && l.px0 + PX < a.w;
#pragma unroll
    for (int r = 0; r < SCALE; ++r) {
        uint32_t nb = (uint32_t)__shfl_down((int)first[r], 1);      // (every lane of the wave takes part)
        if (need && r < l.nrows) {
            if (lane == 63) {
                const uint8_t *q = l.p + r * a.pitch + RUN;
                nb = mo_luma(q[0], q[1], q[2]);
            }
            fine += hl_absdiff(nb, last[r]);
        }
    }
    luma = wave_sum_u32(luma); n_dark = wave_sum_u32(n_dark); n_bright = wave_sum_u32(n_bright); n_changed = wave_sum_u32(n_changed); fine = wave_sum_u32(fine);
    if (lane == 0) {
        uint32_t *d = s_part[tid >> 6];
        d[0] = luma; d[1] = fine; d[2] = n_dark; d[3] = n_bright; d[4] = n_changed;
    }
    __syncthreads();
    if (tid < 5) {
        uint32_t t = 0;                                             // at most 256 threads x 64 pixels x 255: no overflow
#pragma unroll
        for (int wv = 0; wv < HL_WAVES; ++wv) t += s_part[wv][tid];
        HlWork *wk = a.work + blockIdx.y;
        if (t == 0) return;
        if (tid == 0) atomicAdd(&wk->luma, (unsigned long long)t);
        else if (tid == 1) atomicAdd(&wk->sharp, (unsigned long long)t);
        else atomicAdd(tid == 2 ? &wk->n_dark : tid == 3 ? &wk->n_bright : &wk->n_changed, t);
    }
}

// ---- edges: Y -> G, and the three structure counts against R ------------------------------------------------------------------
__global__ __launch_bounds__(HL_THREADS) void health_edges(HlArgs a) {
    __shared__ uint8_t s_y[HL_TH + 2][HL_TW + 2];
    __shared__ uint32_t s_part[HL_WAVES][3];
    const int tid = threadIdx.x;
    const HlSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int tx0 = (int)(blockIdx.x % a.tiles_x) * HL_TW, ty0 = (int)(blockIdx.x / a.tiles_x) * HL_TH;
    for (int i = tid; i < (HL_TW + 2) * (HL_TH + 2); i += HL_THREADS) {
        const int lx = i % (HL_TW + 2), ly = i / (HL_TW + 2), cx = tx0 - 1 + lx, cy = ty0 - 1 + ly;     // local (lx, ly) is cell (tx0 - 1 + lx, ty0 - 1 + ly)
        s_y[ly][lx] = (cx >= 0 && cx < a.gw && cy >= 0 && cy < a.gh) ? a.y[s_off + (size_t)cy * a.gw + cx] : 0;
    }
    __syncthreads();
    const int lx = tid & 63, cx = tx0 + lx, t = a.rule.edge_threshold;
    uint32_t n_edge = 0, n_ref = 0, n_kept = 0;
#pragma unroll
    for (int k = 0; k < HL_TH / HL_WAVES; ++k) {
        const int ly = (tid >> 6) + HL_WAVES * k, cy = ty0 + ly;
        if (cx >= a.gw || cy >= a.gh) continue;
        const uint32_t g = hl_interior(cx, cy, a.gw, a.gh) ? hl_coarse(s_y[ly + 1][lx], s_y[ly + 1][lx + 2], s_y[ly][lx + 1], s_y[ly + 2][lx + 1]) : 0u;
        const size_t idx = s_off + (size_t)cy * a.gw + cx;
        a.g[idx] = (uint8_t)g;
        const bool ref = hl_ref_edge(a.r[idx], t);
        n_edge += hl_edge(g, t) ? 1u : 0u;
        n_ref += ref ? 1u : 0u;
        n_kept += ref && hl_weak_edge(g, t) ? 1u : 0u;
    }
    n_edge = wave_sum_u32(n_edge); n_ref = wave_sum_u32(n_ref); n_kept = wave_sum_u32(n_kept);
    if ((tid & 63) == 0) {
        uint32_t *d = s_part[tid >> 6];
        d[0] = n_edge; d[1] = n_ref; d[2] = n_kept;
    }
    __syncthreads();
    if (tid < 3) {
        uint32_t s = 0;
#pragma unroll
        for (int wv = 0; wv < HL_WAVES; ++wv) s += s_part[wv][tid];
        HlWork *wk = a.work + blockIdx.y;
        if (s) atomicAdd(tid == 0 ? &wk->n_edge : tid == 1 ? &wk->n_ref_edge : &wk->n_kept, s);
    }
}

// ---- decide: one thread per stream of the call ----------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void health_decide(HlArgs a) {
    const int slot = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (slot >= a.n) return;
    const HlSlot sl = a.slots[slot];
    const HlWork wk = a.work[slot];
    HlState st = a.state[sl.stream];
    const HlCounts k{wk.luma, wk.sharp, wk.n_dark, wk.n_bright, wk.n_changed, wk.n_edge, wk.n_ref_edge, wk.n_kept};
    HlEvent ev[HL_MAX_EVENTS];
    uint32_t raw = 0;
    int32_t learn = 0;
    const int n_ev = hl_step(a.rule, k, a.cells, st, ev, &raw, &learn);
    a.state[sl.stream] = st;
    a.work[slot].learn = learn;
    rtmodt_health_result r{};
    r.stream = sl.stream; r.frames_seen = st.frames_seen; r.raw = raw; r.active = st.active;
    r.n_dark = wk.n_dark; r.n_bright = wk.n_bright; r.n_changed = wk.n_changed; r.n_edge = wk.n_edge; r.n_ref_edge = wk.n_ref_edge; r.n_kept = wk.n_kept;
    r.n_events = n_ev; r.learned = learn;
    r.luma_sum = wk.luma; r.sharp = wk.sharp; r.ref_sharp = st.ref_sharp;
    a.res[slot] = r;
    for (int i = 0; i < n_ev && i < HL_MAX_EVENTS; ++i) a.events[(size_t)slot * HL_MAX_EVENTS + i] = rtmodt_health_event{sl.frame_id, ev[i].condition, ev[i].kind};
}

// ---- learn: R takes the step the decision chose -----------------------------------------------------------------------------------
__global__ __launch_bounds__(HL_THREADS) void health_learn(HlArgs a) {
    const int32_t learn = a.work[blockIdx.y].learn;
    const long long idx = (long long)blockIdx.x * HL_THREADS + threadIdx.x;
    if (learn == HL_LEARN_NONE || idx >= a.cells) return;
    const size_t i = (size_t)a.slots[blockIdx.y].stream * (size_t)a.cells + (size_t)idx;
    a.r[i] = (uint16_t)hl_learn_r(a.r[i], a.g[i], learn, a.rule.ref_shift);
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_health : HandleBase {
    rtmodt_health_cfg cfg{};
    GridGeom g;
    EventTimer<2> timer;
    uint16_t *d_r = nullptr;
    uint8_t *d_y = nullptr, *d_g = nullptr;
    HlState *d_state = nullptr;
    char *d_out = nullptr, *h_out = nullptr;    // HlWork[S] | results[n] | events[n][8]; the host mirror holds the last two
    size_t out_bytes = 0;
    CmdBuf cmd;                         // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage stage;
};

namespace {

HlRule hl_rule(const rtmodt_health_cfg &c) {
    return HlRule{c.edge_threshold, c.ref_shift, c.warmup, c.dark_level, c.dark_pm, c.bright_level, c.bright_pm, c.retain_pm, c.cover_pm, c.defocus_pm,
                  c.min_ref_edges, c.hold_frames, c.clear_frames, c.freeze_frames, c.freeze_cells, c.relearn_frames};
}

int hl_check_rule(const rtmodt_health_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null health config");
    RT_CHECK(c->edge_threshold >= 1 && c->edge_threshold <= 255, RTMODT_E_INVALID, "edge_threshold %d outside 1..255", c->edge_threshold);
    RT_CHECK(c->ref_shift >= 1 && c->ref_shift <= 12, RTMODT_E_INVALID, "ref_shift %d outside 1..12", c->ref_shift);
    RT_CHECK(c->warmup >= 1 && c->warmup <= 255, RTMODT_E_INVALID, "warmup %d outside 1..255", c->warmup);
    RT_CHECK(c->dark_level >= 0 && c->dark_level <= 255 && c->bright_level >= 0 && c->bright_level <= 255, RTMODT_E_INVALID,
             "dark_level %d / bright_level %d outside 0..255", c->dark_level, c->bright_level);
    RT_CHECK(hl_pm_ok(c->dark_pm) && hl_pm_ok(c->bright_pm) && hl_pm_ok(c->retain_pm) && hl_pm_ok(c->cover_pm) && hl_pm_ok(c->defocus_pm), RTMODT_E_INVALID,
             "a per-mille parameter outside 0..1000 (dark %d, bright %d, retain %d, cover %d, defocus %d)", c->dark_pm, c->bright_pm, c->retain_pm, c->cover_pm,
             c->defocus_pm);
    RT_CHECK(c->min_ref_edges >= 0 && c->min_ref_edges <= MO_MAX_CELLS, RTMODT_E_INVALID, "min_ref_edges %d outside 0..2^24", c->min_ref_edges);
    RT_CHECK(c->hold_frames >= 1 && c->hold_frames <= HL_MAX_TIMER && c->clear_frames >= 1 && c->clear_frames <= HL_MAX_TIMER, RTMODT_E_INVALID,
             "hold_frames %d / clear_frames %d outside 1..%d", c->hold_frames, c->clear_frames, HL_MAX_TIMER);
    RT_CHECK(c->freeze_frames >= 0 && c->freeze_frames <= HL_MAX_TIMER, RTMODT_E_INVALID, "freeze_frames %d outside 0..%d", c->freeze_frames, HL_MAX_TIMER);
    RT_CHECK(c->freeze_cells >= 0 && c->freeze_cells <= MO_MAX_CELLS, RTMODT_E_INVALID, "freeze_cells %d outside 0..2^24", c->freeze_cells);
    RT_CHECK(c->relearn_frames >= 0 && c->relearn_frames <= HL_MAX_COUNT, RTMODT_E_INVALID, "relearn_frames %d outside 0..2^30", c->relearn_frames);
    return RTMODT_OK;
}

int hl_check_cfg(const rtmodt_health_cfg *c) {
    RT_TRY(hl_check_rule(c));
    RT_TRY(check_grid_cfg(c->streams, c->height, c->width, c->scale, HL_MAX_STREAMS));
    return check_grid_cells(c->streams, c->height, c->width, c->scale, HL_MAX_TOTAL_CELLS);
}

HlState hl_state_in(const rtmodt_health_state &s) {
    HlState o;
    memcpy(&o, &s, sizeof(o));
    return o;
}
void hl_state_out(const HlState &s, rtmodt_health_state *o) { memcpy(o, &s, sizeof(s)); }

void (*const hl_pixel_kernels[2][4])(HlArgs) = RTMODT_SCALE_KERNELS(health_pixels);

}  // namespace

extern "C" {

void rtmodt_health_default_cfg(rtmodt_health_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_health_cfg{};
    cfg->streams = 1; cfg->height = 0; cfg->width = 0;
    cfg->scale = 4; cfg->edge_threshold = 24; cfg->ref_shift = 6; cfg->warmup = 25;
    cfg->dark_level = 16; cfg->dark_pm = 950; cfg->bright_level = 240; cfg->bright_pm = 950;
    cfg->retain_pm = 500; cfg->cover_pm = 300; cfg->defocus_pm = 500; cfg->min_ref_edges = 16;
    cfg->hold_frames = 25; cfg->clear_frames = 25; cfg->freeze_frames = 50; cfg->freeze_cells = 0; cfg->relearn_frames = 0;
    cfg->device = 0;
}

void rtmodt_health_destroy(rtmodt_health *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_r); hipFree(p->d_y); hipFree(p->d_g); hipFree(p->d_state); hipFree(p->d_out);
        hipHostFree(p->h_out);
        p->cmd.release(); p->stage.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_health_create(const rtmodt_health_cfg *cfg, rtmodt_health **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(hl_check_cfg(cfg));
    rtmodt_health *p = new rtmodt_health();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->g.set(cfg->height, cfg->width, cfg->scale);
    auto body = [&]() -> int {
        const size_t S = (size_t)cfg->streams, all = S * (size_t)p->g.cells;
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_r, all * sizeof(uint16_t)));
        RT_HIP(hipMalloc((void **)&p->d_y, all));
        RT_HIP(hipMalloc((void **)&p->d_g, all));
        RT_HIP(hipMalloc((void **)&p->d_state, S * sizeof(HlState)));
        p->out_bytes = S * (sizeof(HlWork) + sizeof(rtmodt_health_result) + HL_MAX_EVENTS * sizeof(rtmodt_health_event));
        RT_HIP(hipMalloc((void **)&p->d_out, p->out_bytes));
        RT_HIP(hipHostMalloc((void **)&p->h_out, p->out_bytes, hipHostMallocDefault));
        RT_HIP(handle_zero(p->d_r, all * sizeof(uint16_t), p->stream));
        RT_HIP(handle_zero(p->d_y, all, p->stream));
        RT_HIP(handle_zero(p->d_g, all, p->stream));
        RT_HIP(handle_zero(p->d_state, S * sizeof(HlState), p->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_health_destroy, out);
}

int rtmodt_health_decide(const rtmodt_health_cfg *cfg, int64_t cells, int64_t frame_id, rtmodt_health_result *row, rtmodt_health_state *state,
                         rtmodt_health_event *events) {
    RT_CHECK(row && state && events, RTMODT_E_INVALID, "null argument");
    RT_TRY(hl_check_rule(cfg));
    HlState st = hl_state_in(*state);
    RT_CHECK(cells >= 1 && cells <= MO_MAX_CELLS, RTMODT_E_INVALID, "%lld cells outside 1..2^24", (long long)cells);
    RT_CHECK(hl_state_ok(st), RTMODT_E_INVALID, "a health state outside its ranges or with owed events behind no rebase (frames_seen %d, active %u, pending %u)", st.frames_seen, st.active, st.pending);
    const HlCounts k{row->luma_sum, row->sharp, row->n_dark, row->n_bright, row->n_changed, row->n_edge, row->n_ref_edge, row->n_kept};
    const uint32_t most = std::max({k.n_dark, k.n_bright, k.n_changed, k.n_edge, k.n_ref_edge, k.n_kept});
    RT_CHECK((int64_t)most <= cells && k.sharp < (1ull << 40) && k.luma_sum <= 255ull * (uint64_t)cells, RTMODT_E_INVALID, "a count above the %lld cells, or a sum out of range",
             (long long)cells);
    HlEvent ev[HL_MAX_EVENTS];
    uint32_t raw = 0;
    int32_t learn = 0;
    const int n = hl_step(hl_rule(*cfg), k, cells, st, ev, &raw, &learn);
    hl_state_out(st, state);
    row->frames_seen = st.frames_seen; row->raw = raw; row->active = st.active; row->n_events = n; row->learned = learn; row->ref_sharp = st.ref_sharp;
    for (int i = 0; i < HL_MAX_EVENTS; ++i) events[i] = i < n ? rtmodt_health_event{frame_id, ev[i].condition, ev[i].kind} : rtmodt_health_event{};
    return RTMODT_OK;
}

int rtmodt_health_process(rtmodt_health *p, const uint8_t *const *frames, const int32_t *streams, const int64_t *frame_ids, int n, int h, int w,
                          int stride_bytes, int mem_kind, rtmodt_health_result *results, rtmodt_health_event *events) {
    RT_CHECK(p && n >= 0 && (n == 0 || (frames && results && events)), RTMODT_E_INVALID, "null argument");
    RT_TRY(check_mem_kind(mem_kind));
    RT_CHECK(h == p->cfg.height && w == p->cfg.width, RTMODT_E_INVALID, "frames of %dx%d, the health monitor was created for %dx%d", w, h, p->cfg.width,
             p->cfg.height);
    RT_CHECK(pitch_holds(stride_bytes, w), RTMODT_E_INVALID, "stride %d below 3 x %d", stride_bytes, w);
    const int S = p->cfg.streams;
    RT_TRY(check_stream_list(frames, streams, n, S));
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_AS_GIVEN));
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(HlSlot)));
    HlSlot *sl = (HlSlot *)p->cmd.h;
    for (int i = 0; i < n; ++i) sl[i] = HlSlot{(uint64_t)(uintptr_t)p->stage.at(frames, i), frame_ids ? frame_ids[i] : 0, streams ? streams[i] : i, 0};
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(HlSlot), hipMemcpyHostToDevice, q));
    RT_TRY(p->stage.copy_in(frames, q));

    const rtmodt_health_cfg &c = p->cfg;
    const size_t off_res = (size_t)S * sizeof(HlWork), res_bytes = (size_t)n * sizeof(rtmodt_health_result);
    const size_t ev_bytes = (size_t)n * HL_MAX_EVENTS * sizeof(rtmodt_health_event);
    HlArgs a{};
    a.slots = (const HlSlot *)p->cmd.d;
    a.pitch = (long long)p->stage.pitch; a.cells = p->g.cells;
    a.n = n; a.h = h; a.w = w; a.gw = p->g.gw; a.gh = p->g.gh;
    a.rule = hl_rule(c);
    a.r = p->d_r; a.y = p->d_y; a.g = p->d_g; a.state = p->d_state;
    a.work = (HlWork *)p->d_out;
    a.res = (rtmodt_health_result *)(p->d_out + off_res); a.events = (rtmodt_health_event *)(p->d_out + off_res + res_bytes);

    const dim3 block(HL_THREADS);
    const GridGeom &g = p->g;
    RT_TRY(p->timer.record(0, q));
    RT_HIP(hipMemsetAsync(p->d_out, 0, off_res + res_bytes + ev_bytes, q));
    HlArgs m = a;
    m.tiles_x = g.model_tiles_x();
    launch_by_scale(hl_pixel_kernels, c.scale, frames_wide(p->stage, sl, n), g.model_grid(n), q, m);
    HlArgs e = a;
    e.tiles_x = g.filter_tiles_x();
    hipLaunchKernelGGL(health_edges, g.filter_grid(n), block, 0, q, e);
    hipLaunchKernelGGL(health_decide, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, q, a);
    hipLaunchKernelGGL(health_learn, g.per_cell(n), block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_HIP(hipMemcpyAsync(p->h_out, p->d_out + off_res, res_bytes + ev_bytes, hipMemcpyDeviceToHost, q));       // every result in one copy
    RT_HIP(hipStreamSynchronize(q));
    memcpy(results, p->h_out, res_bytes);
    memcpy(events, p->h_out + res_bytes, ev_bytes);
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_health_read_state(rtmodt_health *p, int stream, uint16_t *r, uint8_t *prev_y, rtmodt_health_state *state) {
    RT_CHECK(p && r && prev_y && state, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(r, p->d_r + (size_t)stream * p->g.cells, (size_t)p->g.cells * sizeof(uint16_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(prev_y, p->d_y + (size_t)stream * p->g.cells, (size_t)p->g.cells, hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(state, p->d_state + stream, sizeof(HlState), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_health_load_state(rtmodt_health *p, int stream, const uint16_t *r, const uint8_t *prev_y, const rtmodt_health_state *state) {
    RT_CHECK(p && r && prev_y && state, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    const HlState st = hl_state_in(*state);
    RT_CHECK(hl_state_ok(st), RTMODT_E_INVALID, "a health state outside its ranges or with owed events behind no rebase (frames_seen %d, active %u, pending %u)", st.frames_seen, st.active, st.pending);
    for (long long i = 0; i < p->g.cells; ++i) RT_CHECK(r[i] <= 255u << 8, RTMODT_E_INVALID, "cell %lld: a reference of %u above 255 << 8", i, (unsigned)r[i]);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_r + (size_t)stream * p->g.cells, r, (size_t)p->g.cells * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_y + (size_t)stream * p->g.cells, prev_y, (size_t)p->g.cells, hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_state + stream, &st, sizeof(HlState), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_health_rebase(rtmodt_health *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    HlState st;
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(&st, p->d_state + stream, sizeof(HlState), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    hl_rebase_now(st);
    RT_HIP(hipMemcpyAsync(p->d_state + stream, &st, sizeof(HlState), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_health_reset(rtmodt_health *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    const size_t first = stream < 0 ? 0 : (size_t)stream, count = stream < 0 ? (size_t)p->cfg.streams : 1;
    RT_HIP(hipMemsetAsync(p->d_r + first * p->g.cells, 0, count * p->g.cells * sizeof(uint16_t), p->stream));
    RT_HIP(hipMemsetAsync(p->d_y + first * p->g.cells, 0, count * p->g.cells, p->stream));
    RT_HIP(hipMemsetAsync(p->d_state + first, 0, count * sizeof(HlState), p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_health_last_ms(rtmodt_health *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

}  // extern "C"
