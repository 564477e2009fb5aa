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
//   motion_model   the hot path: every pixel is read once.  A thread owns a run of 4 / scale cells (at least one) of one cell row,
//                  12 bytes of each pixel row (24 at scale 8); lanes are adjacent runs, so a wave reads 768 contiguous bytes per
//                  pixel row.  WIDE (every frame base and the pitch a multiple of 4): the full runs of full cell rows are read as
//                  dwords, all of them issued before the first is used; else byte by byte.  No atomics and no floats on the model:
//                  a cell is read and written by one lane.  n_raw and luma_sum are summed per wave and added with one integer
//                  atomic each.  The kernel also zeroes the stream's block grid.
//   motion_filter  one workgroup per tile of 64 x 16 cells: raw through LDS with a halo of 1 + dilate, the 3 x 3 count, the
//                  dilation; writes the mask, makes every mask cell its own union-find root, adds n_fg, the box and (through LDS)
//                  the block grid.
//   motion_link    union-find over the mask (stitch.hip's: compare-and-swap hooks the larger root under the smaller, path halving);
//                  a cell looks at W, NW, N, NE and skips the links its neighbours make.
//   motion_roots   every mask cell adds its area and box at its root; a wave whose mask cells share one root adds once.
//   motion_count   qualifying roots (parent == self, area >= min_area) per chunk of 4096 cells.  A root is the smallest index of
//                  its component, that is its first cell in raster order.
//   motion_finish  one workgroup per stream: the exclusive scan of the chunk counts, the status, frames_seen (the device decides a
//                  re-initialisation after a SCENE_CHANGE: no host round trip).
//   motion_emit    a chunk that holds one of the first max_regions qualifying roots ranks them and writes their regions.
#include <algorithm>
#include <cstring>
#include <vector>

#include "frame_stage.h"

#define MO_HD __host__ __device__
#include "motion_model.h"

namespace rtmodt {

#include "wg_dev.h"

constexpr int MO_THREADS = 256, MO_WAVES = MO_THREADS / 64, MO_TW = 64, MO_TH = 16, MO_ROWS = 4, MO_CHUNK = 4096, MO_MAX_HALO = 4;
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

__device__ __forceinline__ uint32_t mo_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t mo_wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// ---- model: pixels -> cell luma -> bg / dev / raw ------------------------------------------------------------------------
template <int SCALE, bool WIDE> __global__ __launch_bounds__(MO_THREADS) void motion_model(MoArgs a) {
    constexpr int CPT = SCALE >= 4 ? 1 : 4 / SCALE, PX = SCALE * CPT, RUN = 3 * PX;     // cells, pixels and bytes of a thread's run
    const int tid = threadIdx.x;
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const int n_blocks = a.bgw * a.bgh;
    for (int i = blockIdx.x * MO_THREADS + tid; i < n_blocks; i += gridDim.x * MO_THREADS) a.blocks[(size_t)sl.stream * n_blocks + i] = 0;

    const int seen = a.seen[sl.stream];
    const int cy = (int)(blockIdx.x / a.tiles_x) * MO_ROWS + (tid >> 6);
    const int cxb = ((int)(blockIdx.x % a.tiles_x) * 64 + (tid & 63)) * CPT;
    uint32_t luma = 0, n_raw = 0;
    if (cy < a.gh && cxb < a.gw) {
        const int px0 = cxb * SCALE, npx = min(PX, a.w - px0);
        const int y0 = cy * SCALE, nrows = min(SCALE, a.h - y0);
        const uint8_t *p = (const uint8_t *)sl.frame + (long long)y0 * a.pitch + 3LL * px0;
        uint32_t sum[CPT];
#pragma unroll
        for (int j = 0; j < CPT; ++j) sum[j] = 0;
        if (WIDE && npx == PX && nrows == SCALE) {
            uint32_t v[SCALE][RUN / 4];                             // every load of the run is issued before the first is used
#pragma unroll
            for (int r = 0; r < SCALE; ++r) {
                const uint32_t *q = (const uint32_t *)(p + r * a.pitch);    // base, pitch and 3 * px0 (a multiple of 12) are multiples of 4
#pragma unroll
                for (int k = 0; k < RUN / 4; ++k) v[r][k] = q[k];
            }
#pragma unroll
            for (int r = 0; r < SCALE; ++r)
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    uint32_t c[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k] = (v[r][(3 * i + k) >> 2] >> (8 * ((3 * i + k) & 3))) & 255u;
                    sum[i / SCALE] += mo_luma(c[0], c[1], c[2]);
                }
        } else {
            for (int r = 0; r < nrows; ++r, p += a.pitch)
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (i < npx) sum[i / SCALE] += mo_luma(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        }
        uint32_t *m = a.model + s_off + (size_t)cy * a.gw + cxb;
        uint8_t *rw = a.raw + s_off + (size_t)cy * a.gw + cxb;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const int cols = mo_cell_span(cxb + j, SCALE, a.w);
            if (cols == 0) continue;
            const uint32_t cnt = (uint32_t)(cols * nrows);
            const uint32_t yc = cnt == SCALE * SCALE ? (sum[j] + SCALE * SCALE / 2) / (SCALE * SCALE) : mo_cell_mean(sum[j], cnt);
            const uint32_t packed = m[j];
            uint32_t bg = packed & 0xffffu, dev = packed >> 16;
            const bool raw = mo_cell(a.rule, yc, seen, bg, dev);
            m[j] = bg | dev << 16;
            rw[j] = raw ? 1 : 0;
            luma += yc;
            n_raw += raw ? 1u : 0u;
        }
    }
    luma = mo_wave_sum(luma);
    n_raw = mo_wave_sum(n_raw);
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
    n_fg = mo_wave_sum(n_fg);
    bx0 = mo_wave_max(bx0); by0 = mo_wave_max(by0); bx1 = mo_wave_max(bx1); by1 = mo_wave_max(by1);
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

// ---- labelling: union-find, the larger root under the smaller ---------------------------------------------------------------
__device__ __forceinline__ int mo_ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mo_st(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int mo_find(int32_t *p, int x) {
    int c = mo_ld(&p[x]);
    while (c != x) {                                        // parents only ever point at smaller cells: no cycle
        const int g = mo_ld(&p[c]);
        if (g == c) return c;
        mo_st(&p[x], g);                                    // path halving: any ancestor is a valid parent
        x = c;
        c = g;
    }
    return x;
}
__device__ void mo_unite(int32_t *p, int x, int y) {
    while (true) {
        x = mo_find(p, x);
        y = mo_find(p, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }
        if (atomicCAS(&p[x], x, y) == x) return;
    }
}

__global__ __launch_bounds__(MO_THREADS) void motion_link(MoArgs a) {
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long idx = (long long)blockIdx.x * MO_THREADS + threadIdx.x;
    if (idx >= a.cells) return;
    const uint8_t *mk = a.mask + s_off;
    if (!mk[idx]) return;
    const int cx = (int)(idx % a.gw), cy = (int)(idx / a.gw);
    int32_t *par = a.parent + s_off;
    const bool up = cy > 0;
    const bool W = cx > 0 && mk[idx - 1];
    const bool N = up && mk[idx - a.gw];
    const bool NW = up && cx > 0 && mk[idx - a.gw - 1];
    const bool NE = up && cx + 1 < a.gw && mk[idx - a.gw + 1];
    // N joins W, NW and NE already (N's own W link, NE's W link, W's link upwards); without N, W joins NW
    if (N) { mo_unite(par, (int)idx, (int)(idx - a.gw)); return; }
    if (W) mo_unite(par, (int)idx, (int)idx - 1);
    else if (NW) mo_unite(par, (int)idx, (int)(idx - a.gw - 1));
    if (NE) mo_unite(par, (int)idx, (int)(idx - a.gw + 1));
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
        root = mo_find(a.parent + s_off, (int)idx);
        bx0 = (uint32_t)(a.gw - cx); by0 = (uint32_t)(a.gh - cy); bx1 = (uint32_t)(cx + 1); by1 = (uint32_t)(cy + 1);
    }
    const unsigned long long act = __ballot(m);
    if (!act) return;                                       // (wave-uniform)
    const int lead = __ffsll((long long)act) - 1;
    const int root0 = __shfl(root, lead);
    const bool same = __ballot(m && root != root0) == 0;
    const uint32_t wx0 = mo_wave_max(bx0), wy0 = mo_wave_max(by0), wx1 = mo_wave_max(bx1), wy1 = mo_wave_max(by1);
    uint32_t n = 1;
    if (same) {                                             // one add per wave
        if ((int)(threadIdx.x & 63) != lead) return;
        n = (uint32_t)__popcll(act); bx0 = wx0; by0 = wy0; bx1 = wx1; by1 = wy1;
    } else if (!m) {
        return;
    }
    atomicAdd(&a.area[s_off + root], n);
    uint32_t *b = (uint32_t *)&a.box[s_off + root];
    atomicMax(b, bx0); atomicMax(b + 1, by0); atomicMax(b + 2, bx1); atomicMax(b + 3, by1);
}

__device__ __forceinline__ bool mo_is_region(const MoArgs &a, size_t s_off, long long idx) {
    return idx < a.cells && a.mask[s_off + idx] && a.parent[s_off + idx] == (int32_t)idx && a.area[s_off + idx] >= (uint32_t)a.min_area;
}

__global__ __launch_bounds__(MO_THREADS) void motion_count(MoArgs a) {
    __shared__ int s_wcnt[MO_WAVES];
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long base = (long long)blockIdx.x * MO_CHUNK;
    int mine = 0;
    for (int r = 0; r < MO_CHUNK / MO_THREADS; ++r) mine += mo_is_region(a, s_off, base + r * MO_THREADS + threadIdx.x) ? 1 : 0;
    int total;
    block_scan_count<MO_WAVES>(mine, s_wcnt, total);
    if (threadIdx.x == 0) a.chunk[(size_t)blockIdx.y * (a.n_chunks + 1) + blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(MO_THREADS) void motion_finish(MoArgs a) {
    __shared__ int s_wcnt[MO_WAVES];
    const int tid = threadIdx.x, slot = blockIdx.x;
    uint32_t *ch = a.chunk + (size_t)slot * (a.n_chunks + 1);
    uint32_t run = 0;
    for (int b = 0; b < a.n_chunks; b += MO_THREADS) {
        const int i = b + tid;
        const int v = i < a.n_chunks ? (int)ch[i] : 0;
        int tot;
        const int pos = block_scan_count<MO_WAVES>(v, s_wcnt, tot);
        if (i < a.n_chunks) ch[i] = run + (uint32_t)pos;
        run += (uint32_t)tot;
    }
    if (tid != 0) return;
    ch[a.n_chunks] = run;
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
    const uint32_t *ch = a.chunk + (size_t)blockIdx.y * (a.n_chunks + 1);
    const uint32_t first = ch[blockIdx.x], n_here = ch[blockIdx.x + 1] - first;
    if (n_here == 0 || first >= (uint32_t)a.max_regions) return;       // (uniform)
    const MoSlot sl = a.slots[blockIdx.y];
    const size_t s_off = (size_t)sl.stream * (size_t)a.cells;
    const long long base = (long long)blockIdx.x * MO_CHUNK;
    uint32_t run = first;
    for (int r = 0; r < MO_CHUNK / MO_THREADS; ++r) {
        const long long idx = base + r * MO_THREADS + threadIdx.x;
        const bool f = mo_is_region(a, s_off, idx);
        int tot;
        const uint32_t pos = run + (uint32_t)block_scan_count<MO_WAVES>(f ? 1 : 0, s_wcnt, tot);
        if (f && pos < (uint32_t)a.max_regions) {
            const uint4 b = a.box[s_off + idx];
            int32_t *out = a.regions + ((size_t)blockIdx.y * a.max_regions + pos) * 5;
            mo_px_box(a.gw - (int)b.x, a.gh - (int)b.y, (int)b.z - 1, (int)b.w - 1, a.scale, a.w, a.h, out);
            out[4] = (int32_t)a.area[s_off + idx];
        }
        run += (uint32_t)tot;
    }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_motion {
    int device = 0;
    rtmodt_motion_cfg cfg{};
    int gw = 0, gh = 0, bgw = 0, bgh = 0, n_chunks = 0;
    long long cells = 0;                // per stream
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
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
    RT_CHECK(c->streams >= 1 && c->streams <= MO_MAX_STREAMS, RTMODT_E_INVALID, "streams %d outside 1..%d", c->streams, MO_MAX_STREAMS);
    RT_CHECK(c->height >= 1 && c->width >= 1 && c->height <= MO_MAX_DIM && c->width <= MO_MAX_DIM, RTMODT_E_INVALID, "bad frame geometry %dx%d",
             c->width, c->height);
    RT_CHECK(mo_scale_ok(c->scale), RTMODT_E_INVALID, "scale %d: one of 1, 2, 4, 8", c->scale);
    RT_CHECK(c->min_neighbors >= 1 && c->min_neighbors <= 9, RTMODT_E_INVALID, "min_neighbors %d outside 1..9", c->min_neighbors);
    RT_CHECK(c->dilate >= 0 && c->dilate <= 3, RTMODT_E_INVALID, "dilate %d outside 0..3", c->dilate);
    RT_CHECK(c->scene_pm >= 1 && c->scene_pm <= 1000, RTMODT_E_INVALID, "scene_pm %d outside 1..1000", c->scene_pm);
    RT_CHECK(c->min_area >= 1, RTMODT_E_INVALID, "min_area %d below 1", c->min_area);
    RT_CHECK(c->max_regions >= 1 && c->max_regions <= MO_MAX_REGIONS, RTMODT_E_INVALID, "max_regions %d outside 1..%d", c->max_regions, MO_MAX_REGIONS);
    RT_CHECK(mo_block_ok(c->block), RTMODT_E_INVALID, "block %d: one of 4, 8, 16, 32", c->block);
    const long long cells = (long long)mo_grid(c->height, c->scale) * mo_grid(c->width, c->scale);
    RT_CHECK(cells <= MO_MAX_CELLS, RTMODT_E_CAPACITY, "a grid of %lld cells (at most %lld)", cells, MO_MAX_CELLS);
    RT_CHECK(cells * c->streams <= MO_MAX_TOTAL_CELLS, RTMODT_E_CAPACITY, "%lld cells in all (at most %lld)", cells * c->streams, MO_MAX_TOTAL_CELLS);
    return RTMODT_OK;
}

int mo_check_stream(const rtmodt_motion *p, int stream) {
    RT_CHECK(stream >= 0 && stream < p->cfg.streams, RTMODT_E_INVALID, "stream %d outside 0..%d", stream, p->cfg.streams - 1);
    return RTMODT_OK;
}

template <bool WIDE> void mo_launch_model(int scale, dim3 grid, hipStream_t q, const MoArgs &a) {
    const dim3 block(MO_THREADS);
    switch (scale) {
    case 1: hipLaunchKernelGGL((motion_model<1, WIDE>), grid, block, 0, q, a); break;
    case 2: hipLaunchKernelGGL((motion_model<2, WIDE>), grid, block, 0, q, a); break;
    case 4: hipLaunchKernelGGL((motion_model<4, WIDE>), grid, block, 0, q, a); break;
    default: hipLaunchKernelGGL((motion_model<8, WIDE>), grid, block, 0, q, a); break;
    }
}

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
    hipSetDevice(p->device);
    if (p->stream) hipStreamSynchronize(p->stream);
    hipFree(p->d_model); hipFree(p->d_area); hipFree(p->d_blocks); hipFree(p->d_chunk); hipFree(p->d_seen); hipFree(p->d_parent);
    hipFree(p->d_raw); hipFree(p->d_mask); hipFree(p->d_box); hipFree(p->d_out);
    hipHostFree(p->h_out);
    p->cmd.release(); p->stage.release();
    if (p->ev0) hipEventDestroy(p->ev0);
    if (p->ev1) hipEventDestroy(p->ev1);
    if (p->stream) hipStreamDestroy(p->stream);
    delete p;
}

int rtmodt_motion_create(const rtmodt_motion_cfg *cfg, rtmodt_motion **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_cfg(cfg));
    rtmodt_motion *p = new rtmodt_motion();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->gw = mo_grid(cfg->width, cfg->scale); p->gh = mo_grid(cfg->height, cfg->scale);
    p->bgw = cdiv(p->gw, cfg->block); p->bgh = cdiv(p->gh, cfg->block);
    p->cells = (long long)p->gw * p->gh;
    p->n_chunks = (int)((p->cells + MO_CHUNK - 1) / MO_CHUNK);
    auto body = [&]() -> int {
        const size_t S = (size_t)cfg->streams, all = S * (size_t)p->cells, nb = S * (size_t)p->bgw * p->bgh;
        RT_HIP(hipSetDevice(p->device));
        RT_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        RT_HIP(hipEventCreate(&p->ev0));
        RT_HIP(hipEventCreate(&p->ev1));
        RT_HIP(hipMalloc((void **)&p->d_model, all * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_raw, all));
        RT_HIP(hipMalloc((void **)&p->d_mask, all));
        RT_HIP(hipMalloc((void **)&p->d_parent, all * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_area, all * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_box, all * sizeof(uint4)));
        RT_HIP(hipMalloc((void **)&p->d_blocks, nb * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_chunk, S * (size_t)(p->n_chunks + 1) * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_seen, S * sizeof(int32_t)));
        p->out_bytes = S * (sizeof(MoWork) + sizeof(rtmodt_motion_result) + (size_t)cfg->max_regions * 5 * sizeof(int32_t));
        RT_HIP(hipMalloc((void **)&p->d_out, p->out_bytes));
        RT_HIP(hipHostMalloc((void **)&p->h_out, p->out_bytes, hipHostMallocDefault));
        RT_HIP(hipMemset(p->d_model, 0, all * sizeof(uint32_t)));
        RT_HIP(hipMemset(p->d_mask, 0, all));
        RT_HIP(hipMemset(p->d_blocks, 0, nb * sizeof(uint32_t)));
        RT_HIP(hipMemset(p->d_seen, 0, S * sizeof(int32_t)));
        return RTMODT_OK;
    };
    const int rc = body();
    if (rc != RTMODT_OK) {
        std::string keep = last_error();
        rtmodt_motion_destroy(p);
        last_error() = keep;
        return rc;
    }
    *out = p;
    return RTMODT_OK;
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
    RT_CHECK(n <= S, RTMODT_E_INVALID, "%d frames in one call for %d streams", n, S);
    RT_CHECK(streams || n == S || n == 0, RTMODT_E_INVALID, "%d frames for %d streams and no stream list", n, S);
    std::vector<char> named(S, 0);
    for (int i = 0; i < n; ++i) {
        RT_CHECK(frames[i], RTMODT_E_INVALID, "frame %d is null", i);
        const int s = streams ? streams[i] : i;
        RT_TRY(mo_check_stream(p, s));
        RT_CHECK(!named[s], RTMODT_E_INVALID, "stream %d is named twice in one call", s);
        named[s] = 1;
    }
    p->timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_AS_GIVEN));
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(MoSlot)));
    MoSlot *sl = (MoSlot *)p->cmd.h;
    bool wide = p->stage.pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        sl[i] = MoSlot{(uint64_t)(uintptr_t)p->stage.at(frames, i), streams ? streams[i] : i, 0};
        wide = wide && sl[i].frame % 4 == 0;
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(MoSlot), hipMemcpyHostToDevice, q));
    RT_TRY(p->stage.copy_in(frames, q));

    const rtmodt_motion_cfg &c = p->cfg;
    const size_t off_res = (size_t)S * sizeof(MoWork), res_bytes = (size_t)n * sizeof(rtmodt_motion_result);
    const size_t reg_bytes = (size_t)n * c.max_regions * 5 * sizeof(int32_t);
    MoArgs a{};
    a.slots = (const MoSlot *)p->cmd.d;
    a.pitch = (long long)p->stage.pitch; a.cells = p->cells;
    a.h = h; a.w = w; a.scale = c.scale; a.gw = p->gw; a.gh = p->gh;
    a.rule = mo_rule(c);
    a.min_neighbors = c.min_neighbors; a.dilate = c.dilate; a.scene_pm = c.scene_pm; a.min_area = c.min_area; a.max_regions = c.max_regions;
    a.block = c.block; a.bgw = p->bgw; a.bgh = p->bgh; a.n_chunks = p->n_chunks;
    a.model = p->d_model; a.seen = p->d_seen; a.raw = p->d_raw; a.mask = p->d_mask; a.parent = p->d_parent; a.area = p->d_area; a.box = p->d_box;
    a.blocks = p->d_blocks; a.work = (MoWork *)p->d_out; a.chunk = p->d_chunk;
    a.res = (rtmodt_motion_result *)(p->d_out + off_res); a.regions = (int32_t *)(p->d_out + off_res + res_bytes);

    const dim3 block(MO_THREADS);
    const int cpt = c.scale >= 4 ? 1 : 4 / c.scale;
    const unsigned per_cell = (unsigned)((p->cells + MO_THREADS - 1) / MO_THREADS);
    RT_HIP(hipEventRecord(p->ev0, q));
    RT_HIP(hipMemsetAsync(p->d_out, 0, off_res + res_bytes + reg_bytes, q));
    MoArgs m = a;
    m.tiles_x = cdiv(p->gw, 64 * cpt);
    const dim3 mgrid((unsigned)(m.tiles_x * cdiv(p->gh, MO_ROWS)), n);
    if (wide) mo_launch_model<true>(c.scale, mgrid, q, m);
    else mo_launch_model<false>(c.scale, mgrid, q, m);
    MoArgs f = a;
    f.tiles_x = cdiv(p->gw, MO_TW);
    hipLaunchKernelGGL(motion_filter, dim3((unsigned)(f.tiles_x * cdiv(p->gh, MO_TH)), n), block, 0, q, f);
    hipLaunchKernelGGL(motion_link, dim3(per_cell, n), block, 0, q, a);
    hipLaunchKernelGGL(motion_roots, dim3(per_cell, n), block, 0, q, a);
    hipLaunchKernelGGL(motion_count, dim3((unsigned)p->n_chunks, n), block, 0, q, a);
    hipLaunchKernelGGL(motion_finish, dim3(n), block, 0, q, a);
    hipLaunchKernelGGL(motion_emit, dim3((unsigned)p->n_chunks, n), block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_HIP(hipEventRecord(p->ev1, q));
    RT_HIP(hipMemcpyAsync(p->h_out, p->d_out + off_res, res_bytes + reg_bytes, hipMemcpyDeviceToHost, q));      // every result in one copy
    RT_HIP(hipStreamSynchronize(q));
    memcpy(results, p->h_out, res_bytes);
    memcpy(regions, p->h_out + res_bytes, reg_bytes);
    p->timed = true;
    return RTMODT_OK;
}

int rtmodt_motion_read_mask(rtmodt_motion *p, int stream, uint8_t *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_stream(p, stream));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(out, p->d_mask + (size_t)stream * p->cells, (size_t)p->cells, hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_read_blocks(rtmodt_motion *p, int stream, uint32_t *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_stream(p, stream));
    const size_t nb = (size_t)p->bgw * p->bgh;
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(out, p->d_blocks + (size_t)stream * nb, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_read_state(rtmodt_motion *p, int stream, uint16_t *bg, uint16_t *dev, int32_t *frames_seen) {
    RT_CHECK(p && bg && dev && frames_seen, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_stream(p, stream));
    p->h_model.resize((size_t)p->cells);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->h_model.data(), p->d_model + (size_t)stream * p->cells, (size_t)p->cells * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(frames_seen, p->d_seen + stream, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    for (long long i = 0; i < p->cells; ++i) {
        bg[i] = (uint16_t)(p->h_model[i] & 0xffffu);
        dev[i] = (uint16_t)(p->h_model[i] >> 16);
    }
    return RTMODT_OK;
}

int rtmodt_motion_load_state(rtmodt_motion *p, int stream, const uint16_t *bg, const uint16_t *dev, int32_t frames_seen) {
    RT_CHECK(p && bg && dev, RTMODT_E_INVALID, "null argument");
    RT_TRY(mo_check_stream(p, stream));
    RT_CHECK(frames_seen >= 0 && frames_seen <= MO_MAX_SEEN, RTMODT_E_INVALID, "frames_seen %d outside 0..%d", frames_seen, MO_MAX_SEEN);
    p->h_model.resize((size_t)p->cells);
    for (long long i = 0; i < p->cells; ++i) p->h_model[i] = (uint32_t)bg[i] | (uint32_t)dev[i] << 16;
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_model + (size_t)stream * p->cells, p->h_model.data(), (size_t)p->cells * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_seen + stream, &frames_seen, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_reset(rtmodt_motion *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(mo_check_stream(p, stream));
    RT_HIP(hipSetDevice(p->device));
    const size_t first = stream < 0 ? 0 : (size_t)stream, count = stream < 0 ? (size_t)p->cfg.streams : 1, nb = (size_t)p->bgw * p->bgh;
    RT_HIP(hipMemsetAsync(p->d_model + first * p->cells, 0, count * p->cells * sizeof(uint32_t), p->stream));
    RT_HIP(hipMemsetAsync(p->d_mask + first * p->cells, 0, count * p->cells, p->stream));
    RT_HIP(hipMemsetAsync(p->d_blocks + first * nb, 0, count * nb * sizeof(uint32_t), p->stream));
    RT_HIP(hipMemsetAsync(p->d_seen + first, 0, count * sizeof(int32_t), p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_motion_last_ms(rtmodt_motion *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    RT_CHECK(p->timed, RTMODT_E_INVALID, "no process call has launched yet");
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1));
    return RTMODT_OK;
}

}  // extern "C"
