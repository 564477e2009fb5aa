// motion.hip -- motion detection on the GPU: a per-stream background model on a downscaled luma grid tells whether a frame shows
// anything that moves, so that a caller can keep the detector off still scenes (pipeline.run(motion=...)).  The reference drops
// frames blind to content (design document B.1) and has no counterpart; PARITY UNPINNED against OpenCV's BackgroundSubtractorMOG2,
// against Frigate's motion detector and against any default tuned on real footage.  tests/motion_ref.py restates every rule below
// in NumPy and the kernels equal it exactly: all of it is integer arithmetic.
//
// Cell luma, model, pixel boxes and status: motion_model.h.  On top of them, per frame of a stream:
//   Mask.     n3 = the raw cells in the 3 x 3 neighbourhood, the cell included, cells outside the grid counting 0;
//             kept = raw && n3 >= min_neighbors; mask = 1 where a kept cell lies within Chebyshev distance `dilate`.
//   Counts.   n_raw, n_fg (mask cells), luma_sum (the sum of Yc), the mask's bounding box in pixels (all zero when empty) and the
//             block grid: the mask cells in each block x block group of cells, uint32[ceil(gh / block)][ceil(gw / block)].
//   Regions.  The 8-connected components of the mask with at least min_area cells, in the raster order of their first cell; each
//             is (x0, y0, x1, y1, area_cells); the first max_regions are stored, n_regions_total counts all of them.
//
// Kernels (256 threads; seven launches and one memset per call for all its streams, whatever the frames show; no grid-wide
// barrier, no spin on another workgroup):
//   motion_model   the hot path: every pixel is read once, by cell_grid.h's reader (a thread owns a run of 4 / scale cells of one
//                  cell row; dwords where every frame base and the pitch are multiples of 4).  No atomics and no floats on the
//                  model: a cell is read and written by one lane.  n_raw and luma_sum are summed per wave and added with one integer
//                  atomic each.  The kernel also zeroes the stream's block grid.
//   motion_filter  one workgroup per tile of 64 x 16 cells: raw through LDS with a halo of 1 + dilate, the 3 x 3 count, the
//                  dilation; writes the mask, makes every mask cell its own union-find root, adds n_fg, the box and (through LDS)
//                  the block grid.
//   motion_link    union-find over the mask (ccl_dev.h: compare-and-swap hooks the larger root under the smaller, path halving); a
//                  cell looks at W, NW, N, NE and skips the links its neighbours make.
//   motion_roots   every mask cell adds its area and box at its root; a wave whose mask cells share one root adds once.
//   motion_count   qualifying roots (parent == self, area >= min_area) per chunk of 4096 cells.  A root is the smallest index of
//                  its component, that is its first cell in raster order.
//   motion_finish  one workgroup per stream: the exclusive scan of the chunk counts, the status, frames_seen (the device decides a
//                  re-initialisation after a SCENE_CHANGE: no host round trip).
//   motion_emit    a chunk that holds one of the first max_regions qualifying roots ranks them and writes their regions.
#include <algorithm>
#include <cstring>
#include <vector>

#define MO_HD __host__ __device__
#include "grid_host.h"

namespace rtmodt {

#include "wg_dev.h"
#include "ccl_dev.h"

constexpr int MO_THREADS = CG_THREADS, MO_WAVES = MO_THREADS / 64, MO_TW = GRID_TW, MO_TH = GRID_TH, MO_MAX_HALO = 4;
constexpr int MO_MAX_STREAMS = 1024;
constexpr long long MO_MAX_TOTAL_CELLS = 1LL << 28;
static_assert(sizeof(rtmodt_motion_result) == 56, "layout");

struct MoSlot { uint64_t frame; int32_t stream, pad; };
// the counters of one frame of a call, zeroed before the launches; the box as maxima of (gw - cx, gh - cy, cx + 1, cy + 1): 0 = empty
struct MoWork { unsigned long long luma; uint32_t n_raw, n_fg, bx0, by0, bx1, by1; };
static_assert(sizeof(MoSlot) == 16 && sizeof(MoWork) == 32, "layout");

struct MoArgs {
    const MoSlot *slots;
    long long pitch, cells;                     // cells per stream
    int h, w, scale, gw, gh, tiles_x;           // tiles_x: of the launch at hand
    MoRule rule;
    int min_neighbors, dilate, scene_pm, min_area, max_regions, block, bgw, bgh, n_chunks;
    uint32_t *model; int32_t *seen;             // bg | dev << 16 per cell; frames_seen per stream
    uint8_t *raw, *mask;
    int32_t *parent; uint32_t *area; uint4 *box;    // at the roots; box as MoWork's
    uint32_t *blocks;
    MoWork *work; uint32_t *chunk;              // [n][n_chunks + 1]
    rtmodt_motion_result *res; int32_t *regions;
};

// ---- model: pixels -> cell luma (cell_grid.h) -> bg / dev / raw ----------------------------------------------------------
template <int SCALE, bool WIDE> __global__ __launch_bounds__(MO_THREADS) void motion_model(MoArgs a) {
    constexpr int CPT = CgRun<SCALE>::CPT;
    const int tid = threadIdx.x;
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int n_blocks = a.bgw * a.bgh;
    for (int i = blockIdx.x * MO_THREADS + tid; i < n_blocks; i += gridDim.x * MO_THREADS) a.blocks[(size_t)sl.stream * n_blocks + i] = 0;

    const int seen = a.seen[sl.stream];
    const CgLane l = cg_lane<SCALE>(blockIdx.x, a.tiles_x, tid, (const uint8_t *)sl.frame, a.pitch, a.h, a.w, a.gw, a.gh);
    uint32_t luma = 0, n_raw = 0;
    if (l.live) {
        uint32_t sum[CPT];
        cg_read_run<SCALE, WIDE>(l.p, a.pitch, l.npx, l.nrows, sum);
        uint32_t *m = a.model + s_off + (size_t)l.cy * a.gw + l.cxb;
        uint8_t *rw = a.raw + s_off + (size_t)l.cy * a.gw + l.cxb;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            uint32_t yc;
            if (!cg_cell_luma<SCALE>(sum[j], l.cxb + j, l.nrows, a.w, yc)) continue;
            const uint32_t packed = m[j];
            uint32_t bg = packed & 0xffffu, dev = packed >> 16;
            const bool raw = mo_cell(a.rule, yc, seen, bg, dev);
            m[j] = bg | dev << 16;
            rw[j] = raw ? 1 : 0;
            luma += yc;
            n_raw += raw ? 1u : 0u;
        }
    }
    luma = wave_sum_u32(luma);
    n_raw = wave_sum_u32(n_raw);
    if ((tid & 63) == 0) {
        MoWork *wk = a.work + blockIdx.y;
        if (luma) atomicAdd(&wk->luma, (unsigned long long)luma);
        if (n_raw) atomicAdd(&wk->n_raw, n_raw);
    }
}

// ---- filter: raw -> mask, n_fg, box, block grid; mask cells become union-find roots ------------------------------------
__global__ __launch_bounds__(MO_THREADS) void motion_filter(MoArgs a) {
    constexpr int LW = MO_TW + 2 * MO_MAX_HALO, LH = MO_TH + 2 * MO_MAX_HALO;
    __shared__ uint8_t s_raw[LH][LW], s_kept[LH][LW];
    __shared__ uint32_t s_blk[64];

    const int tid = threadIdx.x;
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int tx0 = (int)(blockIdx.x % a.tiles_x) * MO_TW, ty0 = (int)(blockIdx.x / a.tiles_x) * MO_TH;
    const int halo = 1 + a.dilate, d = a.dilate;            // local (lx, ly) is cell (tx0 - halo + lx, ty0 - halo + ly)
    const int lw = MO_TW + 2 * halo, lh = MO_TH + 2 * halo;
    if (tid < 64) s_blk[tid] = 0;
    for (int i = tid; i < lw * lh; i += MO_THREADS) {
        const int lx = i % lw, ly = i / lw, cx = tx0 - halo + lx, cy = ty0 - halo + ly;
        s_raw[ly][lx] = (cx >= 0 && cx < a.gw && cy >= 0 && cy < a.gh) ? a.raw[s_off + (size_t)cy * a.gw + cx] : 0;
    }
    __syncthreads();
    const int kw = MO_TW + 2 * d, kh = MO_TH + 2 * d;       // kept is needed d cells around the tile: local 1 .. lw - 2
    for (int i = tid; i < kw * kh; i += MO_THREADS) {
        const int lx = 1 + i % kw, ly = 1 + i / kw;
        int n3 = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) n3 += s_raw[ly + dy][lx + dx];
        s_kept[ly][lx] = s_raw[ly][lx] && n3 >= a.min_neighbors;
    }
    __syncthreads();
    const int lx = tid & 63, cx = tx0 + lx;
    uint32_t n_fg = 0, bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
    const int bshift = a.block == 4 ? 2 : a.block == 8 ? 3 : a.block == 16 ? 4 : 5, bpr = MO_TW >> bshift;     // blocks per tile row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, cy = ty0 + ly;
        if (cx >= a.gw || cy >= a.gh) continue;
        bool m = false;
        for (int dy = -d; dy <= d; ++dy)
            for (int dx = -d; dx <= d; ++dx) m |= s_kept[halo + ly + dy][halo + lx + dx] != 0;
        const size_t idx = (size_t)cy * a.gw + cx;
        a.mask[s_off + idx] = m ? 1 : 0;
        if (!m) continue;
        a.parent[s_off + idx] = (int32_t)idx;
        a.area[s_off + idx] = 0;
        a.box[s_off + idx] = make_uint4(0u, 0u, 0u, 0u);
        ++n_fg;
        bx0 = max(bx0, (uint32_t)(a.gw - cx)); by0 = max(by0, (uint32_t)(a.gh - cy));
        bx1 = max(bx1, (uint32_t)(cx + 1)); by1 = max(by1, (uint32_t)(cy + 1));
        atomicAdd(&s_blk[(ly >> bshift) * bpr + (lx >> bshift)], 1u);
    }
    n_fg = wave_sum_u32(n_fg);
    bx0 = wave_max_u32(bx0); by0 = wave_max_u32(by0); bx1 = wave_max_u32(bx1); by1 = wave_max_u32(by1);
    if ((tid & 63) == 0 && n_fg) {
        MoWork *wk = a.work + blockIdx.y;
        atomicAdd(&wk->n_fg, n_fg);
        atomicMax(&wk->bx0, bx0); atomicMax(&wk->by0, by0); atomicMax(&wk->bx1, bx1); atomicMax(&wk->by1, by1);
    }
    __syncthreads();
    if (tid < 64 && s_blk[tid]) {                           // a count above 0 has a cell of the grid in it: the block exists
        const int bx = (tx0 >> bshift) + tid % bpr, by = (ty0 >> bshift) + tid / bpr;
        atomicAdd(&a.blocks[(size_t)sl.stream * (a.bgw * a.bgh) + (size_t)by * a.bgw + bx], s_blk[tid]);
    }
}

// ---- labelling (ccl_dev.h) ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void motion_link(MoArgs a) {
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long idx = (long long)blockIdx.x * MO_THREADS + threadIdx.x;
    if (idx < a.cells) ccl_link_cell(a.mask + s_off, a.parent + s_off, a.gw, idx);
}

__global__ __launch_bounds__(MO_THREADS) void motion_roots(MoArgs a) {
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long idx = (long long)blockIdx.x * MO_THREADS + threadIdx.x;
    const bool m = idx < a.cells && a.mask[s_off + idx];
    int root = -1;
    uint32_t bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
    if (m) {
        const int cx = (int)(idx % a.gw), cy = (int)(idx / a.gw);
        root = ccl_find(a.parent + s_off, (int)idx);
        bx0 = (uint32_t)(a.gw - cx); by0 = (uint32_t)(a.gh - cy); bx1 = (uint32_t)(cx + 1); by1 = (uint32_t)(cy + 1);
    }
    CclWave wv;
    if (!ccl_wave_roots(m, root, wv)) return;
    const uint32_t wx0 = wave_max_u32(bx0), wy0 = wave_max_u32(by0), wx1 = wave_max_u32(bx1), wy1 = wave_max_u32(by1);
    uint32_t n = 1;
    if (wv.same) {                                          // one add per wave
        if ((int)(threadIdx.x & 63) != wv.lead) return;
        n = wv.n; bx0 = wx0; by0 = wy0; bx1 = wx1; by1 = wy1;
    } else if (!m) {
        return;
    }
    atomicAdd(&a.area[s_off + root], n);
    uint32_t *b = (uint32_t *)&a.box[s_off + root];
    atomicMax(b, bx0); atomicMax(b + 1, by0); atomicMax(b + 2, bx1); atomicMax(b + 3, by1);
}

// a qualifying root of stream offset s_off: the smallest index of its component, that is its first cell in raster order
__device__ __forceinline__ bool mo_is_region(const MoArgs &a, size_t s_off, long long idx) {
    return idx < a.cells && a.mask[s_off + idx] && a.parent[s_off + idx] == (int32_t)idx && a.area[s_off + idx] >= (uint32_t)a.min_area;
}

__global__ __launch_bounds__(MO_THREADS) void motion_count(MoArgs a) {
    __shared__ int s_wcnt[MO_WAVES];
    const size_t s_off = (size_t)a.slots[blockIdx.y].stream * (size_t)a.cells;
    ccl_count_chunk<MO_WAVES>(a.chunk + (size_t)blockIdx.y * (a.n_chunks + 1), s_wcnt, [&](long long idx) { return mo_is_region(a, s_off, idx); });
}

__global__ __launch_bounds__(MO_THREADS) void motion_finish(MoArgs a) {
    __shared__ int s_wcnt[MO_WAVES];
    const int slot = blockIdx.x;
    const uint32_t run = ccl_scan_chunks<MO_WAVES>(a.chunk + (size_t)slot * (a.n_chunks + 1), a.n_chunks, s_wcnt);
    if (threadIdx.x != 0) return;
    const MoSlot sl = a.slots[slot];
    const MoWork wk = a.work[slot];
    const int seen = a.seen[sl.stream];
    rtmodt_motion_result r{};
    r.status = mo_status(seen, a.rule.warmup, wk.n_raw, a.scene_pm, a.cells, run);
    r.stream = sl.stream;
    r.frames_seen = mo_next_seen(seen, r.status);
    r.n_raw = wk.n_raw; r.n_fg = wk.n_fg;
    r.n_regions_total = (int32_t)run;
    r.n_regions = (int32_t)min(run, (uint32_t)a.max_regions);
    if (wk.n_fg) mo_px_box(a.gw - (int)wk.bx0, a.gh - (int)wk.by0, (int)wk.bx1 - 1, (int)wk.by1 - 1, a.scale, a.w, a.h, r.bbox);
    r.luma_sum = wk.luma;
    a.res[slot] = r;
    a.seen[sl.stream] = r.frames_seen;
}

__global__ __launch_bounds__(MO_THREADS) void motion_emit(MoArgs a) {
    __shared__ int s_wcnt[MO_WAVES];
    const size_t s_off = (size_t)a.slots[blockIdx.y].stream * (size_t)a.cells;
    ccl_emit_chunk<MO_WAVES>(
        a.chunk + (size_t)blockIdx.y * (a.n_chunks + 1), a.max_regions, s_wcnt, [&](long long idx) { return mo_is_region(a, s_off, idx); },
        [&](long long idx, uint32_t pos) {
            const uint4 b = a.box[s_off + idx];
            int32_t *out = a.regions + ((size_t)blockIdx.y * a.max_regions + pos) * 5;
            mo_px_box(a.gw - (int)b.x, a.gh - (int)b.y, (int)b.z - 1, (int)b.w - 1, a.scale, a.w, a.h, out);
            out[4] = (int32_t)a.area[s_off + idx];
        });
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_motion : HandleBase {
    rtmodt_motion_cfg cfg{};
    GridGeom g;
    int bgw = 0, bgh = 0;
    EventTimer<2> timer;
    uint32_t *d_model = nullptr, *d_area = nullptr, *d_blocks = nullptr, *d_chunk = nullptr;
    int32_t *d_seen = nullptr, *d_parent = nullptr;
    uint8_t *d_raw = nullptr, *d_mask = nullptr;
    uint4 *d_box = nullptr;
    char *d_out = nullptr, *h_out = nullptr;    // MoWork[S] | results[n] | regions[n][max_regions][5]; the host mirror holds the last two
    size_t out_bytes = 0;
    CmdBuf cmd;                         // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage stage;
    std::vector<uint32_t> h_model;      // read_state / load_state
};

namespace {

MoRule mo_rule(const rtmodt_motion_cfg &c) { return MoRule{c.learn_shift, c.learn_shift_fg, c.threshold, c.dev_gain, c.warmup}; }

int mo_check_rule(const rtmodt_motion_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null motion config");
    RT_CHECK(c->learn_shift >= 1 && c->learn_shift <= 8, RTMODT_E_INVALID, "learn_shift %d outside 1..8", c->learn_shift);
    RT_CHECK(c->learn_shift_fg == 0 || (c->learn_shift_fg >= c->learn_shift && c->learn_shift_fg <= 12), RTMODT_E_INVALID,
             "learn_shift_fg %d: 0, or learn_shift %d..12", c->learn_shift_fg, c->learn_shift);
    RT_CHECK(c->threshold >= 1 && c->threshold <= 255, RTMODT_E_INVALID, "threshold %d outside 1..255", c->threshold);
    RT_CHECK(c->dev_gain >= 0 && c->dev_gain <= 8, RTMODT_E_INVALID, "dev_gain %d outside 0..8", c->dev_gain);
    RT_CHECK(c->warmup >= 1 && c->warmup <= 255, RTMODT_E_INVALID, "warmup %d outside 1..255", c->warmup);
    return RTMODT_OK;
}

int mo_check_cfg(const rtmodt_motion_cfg *c) {
    RT_TRY(mo_check_rule(c));
    RT_TRY(check_grid_cfg(c->streams, c->height, c->width, c->scale, MO_MAX_STREAMS));
    RT_CHECK(c->min_neighbors >= 1 && c->min_neighbors <= 9, RTMODT_E_INVALID, "min_neighbors %d outside 1..9", c->min_neighbors);
    RT_CHECK(c->dilate >= 0 && c->dilate <= 3, RTMODT_E_INVALID, "dilate %d outside 0..3", c->dilate);
    RT_CHECK(c->scene_pm >= 1 && c->scene_pm <= 1000, RTMODT_E_INVALID, "scene_pm %d outside 1..1000", c->scene_pm);
    RT_CHECK(c->min_area >= 1, RTMODT_E_INVALID, "min_area %d below 1", c->min_area);
    RT_CHECK(c->max_regions >= 1 && c->max_regions <= MO_MAX_REGIONS, RTMODT_E_INVALID, "max_regions %d outside 1..%d", c->max_regions, MO_MAX_REGIONS);
    RT_CHECK(mo_block_ok(c->block), RTMODT_E_INVALID, "block %d: one of 4, 8, 16, 32", c->block);
    return check_grid_cells(c->streams, c->height, c->width, c->scale, MO_MAX_TOTAL_CELLS);
}

void (*const mo_model_kernels[2][4])(MoArgs) = RTMODT_SCALE_KERNELS(motion_model);

}  // namespace

extern "C" {

void rtmodt_motion_default_cfg(rtmodt_motion_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_motion_cfg{};
    cfg->streams = 1; cfg->height = 0; cfg->width = 0;
    cfg->scale = 4; cfg->learn_shift = 4; cfg->learn_shift_fg = 8; cfg->threshold = 12; cfg->dev_gain = 2;
    cfg->min_neighbors = 3; cfg->dilate = 1; cfg->warmup = 8; cfg->scene_pm = 600; cfg->min_area = 4; cfg->max_regions = 32;
    cfg->block = 16; cfg->device = 0;
}

void rtmodt_motion_destroy(rtmodt_motion *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_model); hipFree(p->d_area); hipFree(p->d_blocks); hipFree(p->d_chunk); hipFree(p->d_seen); hipFree(p->d_parent);
        hipFree(p->d_raw); hipFree(p->d_mask); hipFree(p->d_box); hipFree(p->d_out);
        hipHostFree(p->h_out);
        p->cmd.release(); p->stage.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_motion_create(const rtmodt_motion_cfg *cfg, rtmodt_motion **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_cfg(cfg));
    rtmodt_motion *p = new rtmodt_motion();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->g.set(cfg->height, cfg->width, cfg->scale);
    p->bgw = cdiv(p->g.gw, cfg->block); p->bgh = cdiv(p->g.gh, cfg->block);
    auto body = [&]() -> int {
        const size_t S = (size_t)cfg->streams, all = S * (size_t)p->g.cells, nb = S * (size_t)p->bgw * p->bgh;
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_model, all * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_raw, all));
        RT_HIP(hipMalloc((void **)&p->d_mask, all));
        RT_HIP(hipMalloc((void **)&p->d_parent, all * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_area, all * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_box, all * sizeof(uint4)));
        RT_HIP(hipMalloc((void **)&p->d_blocks, nb * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_chunk, S * (size_t)(p->g.n_chunks + 1) * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_seen, S * sizeof(int32_t)));
        p->out_bytes = S * (sizeof(MoWork) + sizeof(rtmodt_motion_result) + (size_t)cfg->max_regions * 5 * sizeof(int32_t));
        RT_HIP(hipMalloc((void **)&p->d_out, p->out_bytes));
        RT_HIP(hipHostMalloc((void **)&p->h_out, p->out_bytes, hipHostMallocDefault));
        RT_HIP(handle_zero(p->d_model, all * sizeof(uint32_t), p->stream));
        RT_HIP(handle_zero(p->d_mask, all, p->stream));
        RT_HIP(handle_zero(p->d_blocks, nb * sizeof(uint32_t), p->stream));
        RT_HIP(handle_zero(p->d_seen, S * sizeof(int32_t), p->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_motion_destroy, out);
}

int rtmodt_motion_cell(const rtmodt_motion_cfg *cfg, uint32_t yc, int32_t frames_seen, uint16_t *bg, uint16_t *dev, int32_t *raw) {
    RT_CHECK(bg && dev && raw, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_rule(cfg));
    RT_CHECK(yc <= 255 && frames_seen >= 0 && frames_seen <= MO_MAX_SEEN, RTMODT_E_INVALID, "cell luma %u, frames_seen %d", yc, frames_seen);
    uint32_t b = *bg, d = *dev;
    *raw = mo_cell(mo_rule(*cfg), yc, frames_seen, b, d) ? 1 : 0;
    *bg = (uint16_t)b; *dev = (uint16_t)d;
    return RTMODT_OK;
}

int rtmodt_motion_process(rtmodt_motion *p, const uint8_t *const *frames, const int32_t *streams, int n, int h, int w, int stride_bytes, int mem_kind,
                          rtmodt_motion_result *results, int32_t *regions) {
    RT_CHECK(p && n >= 0 && (n == 0 || (frames && results && regions)), RTMODT_E_INVALID, "null argument");
    RT_TRY(check_mem_kind(mem_kind));
    RT_CHECK(h == p->cfg.height && w == p->cfg.width, RTMODT_E_INVALID, "frames of %dx%d, the motion detector was created for %dx%d", w, h,
             p->cfg.width, p->cfg.height);
    RT_CHECK(pitch_holds(stride_bytes, w), RTMODT_E_INVALID, "stride %d below 3 x %d", stride_bytes, w);
    const int S = p->cfg.streams;
    RT_TRY(check_stream_list(frames, streams, n, S));
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_AS_GIVEN));
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(MoSlot)));
    MoSlot *sl = (MoSlot *)p->cmd.h;
    for (int i = 0; i < n; ++i) sl[i] = MoSlot{(uint64_t)(uintptr_t)p->stage.at(frames, i), streams ? streams[i] : i, 0};
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(MoSlot), hipMemcpyHostToDevice, q));
    RT_TRY(p->stage.copy_in(frames, q));

    const rtmodt_motion_cfg &c = p->cfg;
    const size_t off_res = (size_t)S * sizeof(MoWork), res_bytes = (size_t)n * sizeof(rtmodt_motion_result);
    const size_t reg_bytes = (size_t)n * c.max_regions * 5 * sizeof(int32_t);
    MoArgs a{};
    a.slots = (const MoSlot *)p->cmd.d;
    a.pitch = (long long)p->stage.pitch; a.cells = p->g.cells;
    a.h = h; a.w = w; a.scale = c.scale; a.gw = p->g.gw; a.gh = p->g.gh;
    a.rule = mo_rule(c);
    a.min_neighbors = c.min_neighbors; a.dilate = c.dilate; a.scene_pm = c.scene_pm; a.min_area = c.min_area; a.max_regions = c.max_regions;
    a.block = c.block; a.bgw = p->bgw; a.bgh = p->bgh; a.n_chunks = p->g.n_chunks;
    a.model = p->d_model; a.seen = p->d_seen; a.raw = p->d_raw; a.mask = p->d_mask; a.parent = p->d_parent; a.area = p->d_area; a.box = p->d_box;
    a.blocks = p->d_blocks; a.work = (MoWork *)p->d_out; a.chunk = p->d_chunk;
    a.res = (rtmodt_motion_result *)(p->d_out + off_res); a.regions = (int32_t *)(p->d_out + off_res + res_bytes);

    const dim3 block(MO_THREADS);
    const GridGeom &g = p->g;
    RT_TRY(p->timer.record(0, q));
    RT_HIP(hipMemsetAsync(p->d_out, 0, off_res + res_bytes + reg_bytes, q));
    MoArgs m = a;
    m.tiles_x = g.model_tiles_x();
    launch_by_scale(mo_model_kernels, c.scale, frames_wide(p->stage, sl, n), g.model_grid(n), q, m);
    MoArgs f = a;
    f.tiles_x = g.filter_tiles_x();
    hipLaunchKernelGGL(motion_filter, g.filter_grid(n), block, 0, q, f);
    hipLaunchKernelGGL(motion_link, g.per_cell(n), block, 0, q, a);
    hipLaunchKernelGGL(motion_roots, g.per_cell(n), block, 0, q, a);
    hipLaunchKernelGGL(motion_count, g.per_chunk(n), block, 0, q, a);
    hipLaunchKernelGGL(motion_finish, dim3(n), block, 0, q, a);
    hipLaunchKernelGGL(motion_emit, g.per_chunk(n), block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_HIP(hipMemcpyAsync(p->h_out, p->d_out + off_res, res_bytes + reg_bytes, hipMemcpyDeviceToHost, q));      // every result in one copy
    RT_HIP(hipStreamSynchronize(q));
    memcpy(results, p->h_out, res_bytes);
    memcpy(regions, p->h_out + res_bytes, reg_bytes);
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_motion_read_mask(rtmodt_motion *p, int stream, uint8_t *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(out, p->d_mask + (size_t)stream * p->g.cells, (size_t)p->g.cells, hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_read_blocks(rtmodt_motion *p, int stream, uint32_t *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    const size_t nb = (size_t)p->bgw * p->bgh;
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(out, p->d_blocks + (size_t)stream * nb, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_read_state(rtmodt_motion *p, int stream, uint16_t *bg, uint16_t *dev, int32_t *frames_seen) {
    RT_CHECK(p && bg && dev && frames_seen, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    p->h_model.resize((size_t)p->g.cells);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->h_model.data(), p->d_model + (size_t)stream * p->g.cells, (size_t)p->g.cells * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(frames_seen, p->d_seen + stream, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    for (long long i = 0; i < p->g.cells; ++i) {
        bg[i] = (uint16_t)(p->h_model[i] & 0xffffu);
        dev[i] = (uint16_t)(p->h_model[i] >> 16);
    }
    return RTMODT_OK;
}

int rtmodt_motion_load_state(rtmodt_motion *p, int stream, const uint16_t *bg, const uint16_t *dev, int32_t frames_seen) {
    RT_CHECK(p && bg && dev, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_CHECK(frames_seen >= 0 && frames_seen <= MO_MAX_SEEN, RTMODT_E_INVALID, "frames_seen %d outside 0..%d", frames_seen, MO_MAX_SEEN);
    p->h_model.resize((size_t)p->g.cells);
    for (long long i = 0; i < p->g.cells; ++i) p->h_model[i] = (uint32_t)bg[i] | (uint32_t)dev[i] << 16;
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_model + (size_t)stream * p->g.cells, p->h_model.data(), (size_t)p->g.cells * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_seen + stream, &frames_seen, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_reset(rtmodt_motion *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    const size_t first = stream < 0 ? 0 : (size_t)stream, count = stream < 0 ? (size_t)p->cfg.streams : 1, nb = (size_t)p->bgw * p->bgh;
    RT_HIP(hipMemsetAsync(p->d_model + first * p->g.cells, 0, count * p->g.cells * sizeof(uint32_t), p->stream));
    RT_HIP(hipMemsetAsync(p->d_mask + first * p->g.cells, 0, count * p->g.cells, p->stream));
    RT_HIP(hipMemsetAsync(p->d_blocks + first * nb, 0, count * nb * sizeof(uint32_t), p->stream));
    RT_HIP(hipMemsetAsync(p->d_seen + first, 0, count * sizeof(int32_t), p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_last_ms(rtmodt_motion *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

}  // extern "C"
