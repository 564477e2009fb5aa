// heatmap.hip -- occupancy heatmaps on the GPU: one uint32 grid per stream accumulates the footprints of boxes or device-resident
// tracks frame after frame, is blended onto BGR24 frames where they lie, and is summed per polygon.  The reference has no
// counterpart (PARITY UNPINNED against Ultralytics' Heatmap solution, against cv2's colormaps and addWeighted and against any
// default tuned on real footage); tests/heatmap_ref.py restates every rule below in NumPy and the kernels equal it exactly -- every
// rule is integer arithmetic.
//
// Grid.  gh x gw = ceil(h / cell) x ceil(w / cell) cells per stream, cell in {1, 2, 4, 8, 16}, zero at creation; edge cells are
//   clipped to the frame.  heatmap_stamp.h states which cells one box covers (BOX, DISC, FOOT).
// Accumulate, one call per frame for all streams; calls are numbered from 1 per handle.
//   1. decay: if decay_shift != 0 and call % decay_every == 0, every cell of every stream first becomes heat - (heat >> decay_shift);
//   2. stamp: heat = min(heat + weight * count, 2^32 - 1) in 64 bits, count the number of this frame's footprints covering the cell.
//   Every output depends on the grid before the call and on this frame's boxes only: a cell is read and written by one lane, once.
//   No atomics on the grid, so saturation is exact and the result independent of the order of the boxes.
// Overlay, in place.  m = scale_max, or (scale_max == 0) the stream's maximum at the time of the call; m == 0: the frame is
//   untouched.  Level v = min(255, (heat * 255 + m / 2) / m) in 64 bits; pixel (x, y) reads cell (x / cell, y / cell); v < min_level:
//   the pixel keeps its bytes; else each channel becomes (p * (256 - alpha) + lut[v][c] * alpha + 128) >> 8.  The bytes past 3w of a
//   row are never written.  The default table is a closed-form jet: channel = clamp(max(0, 765 - |8v - 510k|) >> 1, 0, 255) with
//   k = 3, 2, 1 for R, G, B (parity with cv2.COLORMAP_JET is UNPINNED).
// Zone sums.  A cell belongs to a polygon when its centre pixel (min(cx * cell + cell / 2, w - 1), min(cy * cell + cell / 2, h - 1))
//   is inside_or_on (polygon.h); a polygon's sum is the uint64 sum of heat over its cells.
//
// Kernels (256 threads; the launch count per call is fixed whatever the number of boxes; no grid-wide barrier, no spin):
//   heatmap_gather      device forms only: one workgroup per stream turns the passed tracks of a tracker's device-resident state
//                       (the selection of privacy_gather, restated) or a detector's detections into stamps;
//   heatmap_accumulate  one workgroup per tile of 64 x 16 cells; the stream's stamps are culled against the tile 256 at a time
//                       through LDS (capacity does not depend on LDS); lane t owns the cells (t % 64, t / 64 + 4k), k < 4, counts
//                       their covers and does a plain read-modify-write with the decay fused in.  Without decay a cell that no
//                       footprint covers is neither read nor written;
//   heatmap_max         overlay with scale_max == 0 only: 64 partial maxima per stream; the overlay reduces them itself;
//   heatmap_overlay     one workgroup per tile of 64 x 16 pixels; a tile whose levels are all below min_level returns before it
//                       reads a byte of the frame;
//   heatmap_zone_sums   64 workgroups per polygon over the cells around its bounding box, 64 partial sums added on the host.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "frame_stage.h"
#include "handle_host.h"
#include "polygon.h"

#define PV_HD __host__ __device__
#include "heatmap_stamp.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_select_dev.h"

constexpr int HM_THREADS = 256, HM_WAVES = HM_THREADS / 64, HM_TW = 64, HM_TH = 16, HM_PARTS = 64;
constexpr int HM_MAX_POLYS = 32, HM_MAX_POINTS = 2048, HM_MAX_BOXES = 65536, HM_MAX_STREAMS = 1024;
constexpr long long HM_MAX_CELLS = 1LL << 30;
static_assert(sizeof(HmStamp) == 40, "layout");

struct HmStream { int64_t stamp_off; int32_t n_stamps, pad; };
struct HmOvFrame { uint64_t ptr; int32_t stream, pad; };
static_assert(sizeof(HmStream) == 16 && sizeof(HmOvFrame) == 16, "layout");

struct HmAccArgs {
    uint32_t *grid; long long gstride;          // cells per stream
    int gw, gh, cell, tiles_x;
    const HmStream *streams; const HmStamp *stamps;
    const int32_t *n_dev; int cap;              // device forms: the gathered count of stream s, at most cap
    int weight, decay_shift;                    // decay_shift 0: no decay in this call
};

struct HmGatherArgs {
    HmStampCfg sc;                              // classes: a device pointer
    int h, w, cap;
    HmStamp *out; int32_t *n_out;
    TrackSrc trk;                               // tracks (track_select_dev.h), or the detections below
    const float4 *det_box; const int32_t *det_cls, *det_n; int det_stride;
};

struct HmOvArgs {
    const HmOvFrame *frames; const uint32_t *grid; long long gstride;
    int gw, cell_shift, h, w, tiles_x;
    long long stride;
    int alpha, min_level; uint32_t scale_max;
    const uint32_t *maxpart; const uint8_t *lut;
};

struct HmZoneArgs {
    const uint32_t *grid;                       // of the one stream
    int gw, gh, cell, h, w;
    const int2 *pts; const int32_t *off; const int4 *bbox;
    unsigned long long *part;                   // [Z][HM_PARTS]
};

// ---- device forms: tracks / detections -> stamps (the selection of track_select_dev.h) ------------------------------------
__global__ __launch_bounds__(HM_THREADS) void heatmap_gather(HmGatherArgs a) {
    __shared__ int s_wcnt[HM_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x;
    TrackSel src;
    if (a.det_box) src = select_list(nullptr, a.det_box + (size_t)f * a.det_stride, a.det_cls + (size_t)f * a.det_stride, a.det_n[f]);
    else src = select_tracks(a.trk, f);
    const float4 *box = src.box; const int32_t *cls = src.cls;
    const int n = src.n < 0 ? 0 : (src.n > a.cap ? a.cap : src.n);
    HmStamp *out = a.out + (size_t)f * a.cap;
    int total = 0;
    for (int base = 0; base < n; base += HM_THREADS) {
        const int i = base + tid;
        bool ok = false;
        HmStamp st{};
        if (i < n) {
            const float4 b = box[i];
            ok = selected(src, i) && finite_bits(b.x) && finite_bits(b.y) && finite_bits(b.z) && finite_bits(b.w) &&
                 hm_stamp(a.sc, b.x, b.y, b.z, b.w, cls[i], a.h, a.w, st);
        }
        int tot;
        const int pos = total + block_scan_count<HM_WAVES>(ok ? 1 : 0, s_wcnt, tot);
        if (ok) out[pos] = st;
        total += tot;
    }
    if (tid == 0) a.n_out[f] = total;
}

// ---- accumulate -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_THREADS) void heatmap_accumulate(HmAccArgs a) {
    __shared__ __attribute__((aligned(8))) HmStamp s_st[HM_THREADS];
    __shared__ int s_wcnt[HM_WAVES];

    const int tid = threadIdx.x, s = blockIdx.y;
    const int tx0 = (blockIdx.x % a.tiles_x) * HM_TW, ty0 = (blockIdx.x / a.tiles_x) * HM_TH;
    const int tx1 = min(tx0 + HM_TW - 1, a.gw - 1), ty1 = min(ty0 + HM_TH - 1, a.gh - 1);
    const int cx = tx0 + (tid & 63), cy0 = ty0 + (tid >> 6);
    uint32_t have = 0;
    if (cx <= tx1)
        for (int k = 0; k < 4; ++k)
            if (cy0 + 4 * k <= ty1) have |= 1u << k;
    int n; const HmStamp *stamps;
    if (a.n_dev) {
        n = a.n_dev[s];
        n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
        stamps = a.stamps + (size_t)s * a.cap;
    } else {
        const HmStream hs = a.streams[s];
        n = hs.n_stamps; stamps = a.stamps + hs.stamp_off;
    }
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};
    for (int ib = 0; ib < n; ib += HM_THREADS) {
        const int i = ib + tid;
        HmStamp st{};
        bool f = false;
        if (i < n) {
            st = stamps[i];
            f = st.cx0 <= tx1 && st.cx1 >= tx0 && st.cy0 <= ty1 && st.cy1 >= ty0;
        }
        int m;
        const int pos = block_scan_count<HM_WAVES>(f ? 1 : 0, s_wcnt, m);
        if (f) s_st[pos] = st;
        __syncthreads();
        if (have)
            for (int e = 0; e < m; ++e) {
                const HmStamp b = s_st[e];
                if (cx < b.cx0 || cx > b.cx1) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (((have >> k) & 1u) && hm_covers(b, a.cell, cx, cy0 + 4 * k)) ++cnt[k];
            }
        __syncthreads();
    }
    uint32_t *g = a.grid + (long long)s * a.gstride + (long long)cy0 * a.gw + cx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((have >> k) & 1u) || (!a.decay_shift && !cnt[k])) continue;       // untouched: neither read nor written
        uint32_t *p = g + 4LL * k * a.gw;
        uint32_t heat = *p;
        if (a.decay_shift) heat -= heat >> a.decay_shift;
        const unsigned long long t = (unsigned long long)heat + (unsigned long long)a.weight * cnt[k];
        *p = t > 0xffffffffull ? 0xffffffffu : (uint32_t)t;
    }
}

// ---- overlay ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_THREADS) void heatmap_max(const uint32_t *grid, long long gstride, uint32_t *maxpart) {
    __shared__ uint32_t s_w[HM_WAVES];
    const int tid = threadIdx.x, s = blockIdx.y;
    const uint32_t *g = grid + (long long)s * gstride;
    uint32_t v = 0;
    for (long long i = (long long)blockIdx.x * HM_THREADS + tid; i < gstride; i += (long long)HM_PARTS * HM_THREADS) v = max(v, g[i]);
    v = wave_max_u32(v);
    if ((tid & 63) == 0) s_w[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) maxpart[(size_t)s * HM_PARTS + blockIdx.x] = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
}

__global__ __launch_bounds__(HM_THREADS) void heatmap_overlay(HmOvArgs a) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint32_t s_m;
    static_assert(HM_PARTS == 64, "one wave reduces the partial maxima");

    const int tid = threadIdx.x;
    const HmOvFrame fr = a.frames[blockIdx.y];
    uint32_t m = a.scale_max;
    if (!m) {                                               // (uniform: a launch argument)
        if (tid < 64) {
            const uint32_t v = wave_max_u32(a.maxpart[(size_t)fr.stream * HM_PARTS + tid]);
            if (tid == 0) s_m = v;
        }
        __syncthreads();
        m = s_m;
    }
    if (m == 0) return;                                     // an all-zero grid: the frame is untouched
    const int x = (blockIdx.x % a.tiles_x) * HM_TW + (tid & 63), y0 = (blockIdx.x / a.tiles_x) * HM_TH + (tid >> 6);
    const uint32_t *g = a.grid + (long long)fr.stream * a.gstride;
    uint32_t level = 0;                                     // byte k: the level of pixel (x, y0 + 4k); 0 never reaches min_level >= 1
    if (x < a.w)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + 4 * k;
            if (y >= a.h) continue;
            const uint32_t heat = g[(long long)(y >> a.cell_shift) * a.gw + (x >> a.cell_shift)];
            uint32_t v = 255;
            if (heat < m) {                                 // (heat >= m: the quotient is at least 255)
                const unsigned long long q = (unsigned long long)heat * 255ull + (m >> 1);
                v = (q >> 32) ? (uint32_t)(q / m) : (uint32_t)q / m;
                v = min(v, 255u);
            }
            if (v >= (uint32_t)a.min_level) level |= v << (8 * k);
        }
    if (!__syncthreads_or(level != 0)) return;              // nothing to blend here: not a byte of the frame is read
    s_lut[tid] = a.lut[3 * tid] | (uint32_t)a.lut[3 * tid + 1] << 8 | (uint32_t)a.lut[3 * tid + 2] << 16;
    __syncthreads();
    uint8_t *px = (uint8_t *)fr.ptr + (long long)y0 * a.stride + 3LL * x;
    const uint32_t al = (uint32_t)a.alpha, na = 256u - al;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = (level >> (8 * k)) & 255u;
        if (!v) continue;
        uint8_t *p = px + 4LL * k * a.stride;
        const uint32_t c = s_lut[v];
        p[0] = (uint8_t)((p[0] * na + (c & 255u) * al + 128u) >> 8);
        p[1] = (uint8_t)((p[1] * na + ((c >> 8) & 255u) * al + 128u) >> 8);
        p[2] = (uint8_t)((p[2] * na + ((c >> 16) & 255u) * al + 128u) >> 8);
    }
}

// ---- zone sums --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_THREADS) void heatmap_zone_sums(HmZoneArgs a) {
    __shared__ int2 s_pts[HM_MAX_POINTS];
    __shared__ unsigned long long s_red[HM_THREADS];
    const int tid = threadIdx.x, z = blockIdx.y;
    const int p0 = a.off[z], np = a.off[z + 1] - p0;
    for (int i = tid; i < np; i += HM_THREADS) s_pts[i] = a.pts[p0 + i];
    __syncthreads();
    const int4 b = a.bbox[z];
    const int x0 = max(b.x, 0), y0 = max(b.y, 0), x1 = min(b.z, a.w - 1), y1 = min(b.w, a.h - 1);
    unsigned long long sum = 0;
    if (np > 0 && x1 >= x0 && y1 >= y0) {
        // a cell's centre pixel lies at most cell / 2 right of its first column: one more cell on either side covers the box
        const int cxa = max(x0 / a.cell - 1, 0), cxb = min(x1 / a.cell + 1, a.gw - 1);
        const int cya = max(y0 / a.cell - 1, 0), cyb = min(y1 / a.cell + 1, a.gh - 1);
        const int nx = cxb - cxa + 1;
        const long long total = (long long)nx * (cyb - cya + 1);
        for (long long i = (long long)blockIdx.x * HM_THREADS + tid; i < total; i += (long long)HM_PARTS * HM_THREADS) {
            const int cy = cya + (int)(i / nx), cx = cxa + (int)(i % nx);
            const int px = min(cx * a.cell + a.cell / 2, a.w - 1), py = min(cy * a.cell + a.cell / 2, a.h - 1);
            if (px >= b.x && px <= b.z && py >= b.y && py <= b.w && inside_or_on(s_pts, np, px, py)) sum += a.grid[(long long)cy * a.gw + cx];
        }
    }
    s_red[tid] = sum;
    __syncthreads();
    for (int d = HM_THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) s_red[tid] += s_red[tid + d];
        __syncthreads();
    }
    if (tid == 0) a.part[(size_t)z * HM_PARTS + blockIdx.x] = s_red[0];
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_heatmap : HandleBase {
    rtmodt_heatmap_cfg cfg{};
    std::vector<int32_t> classes;       // cfg.classes points here (or is null)
    int32_t *d_classes = nullptr;
    int gw = 0, gh = 0;
    long long cells = 0;                // per stream
    uint64_t calls = 0;
    EventTimer<2> timer;
    uint32_t *d_grid = nullptr, *d_maxpart = nullptr;
    unsigned long long *d_part = nullptr, *h_part = nullptr;
    uint8_t *d_lut = nullptr;
    CmdBuf cmd;                         // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage stage;
    HmStamp *d_gather = nullptr; int32_t *d_gn = nullptr;
    size_t gather_bytes = 0;
};

namespace {

int hm_check_cfg(const rtmodt_heatmap_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null heatmap config");
    RT_CHECK(c->n_streams >= 1 && c->n_streams <= HM_MAX_STREAMS, RTMODT_E_INVALID, "n_streams %d outside 1..%d", c->n_streams, HM_MAX_STREAMS);
    RT_CHECK(c->height >= 1 && c->width >= 1 && c->height <= HM_MAX_DIM && c->width <= HM_MAX_DIM, RTMODT_E_INVALID, "bad frame geometry %dx%d",
             c->width, c->height);
    RT_CHECK(hm_cell_ok(c->cell), RTMODT_E_INVALID, "cell %d: one of 1, 2, 4, 8, 16", c->cell);
    RT_CHECK(c->footprint == RTMODT_HEATMAP_BOX || c->footprint == RTMODT_HEATMAP_DISC || c->footprint == RTMODT_HEATMAP_FOOT, RTMODT_E_INVALID,
             "footprint kind %d", c->footprint);
    RT_CHECK(c->foot_radius >= 0 && c->foot_radius <= HM_MAX_FOOT_RADIUS, RTMODT_E_INVALID, "foot_radius %d outside 0..%d", c->foot_radius,
             HM_MAX_FOOT_RADIUS);
    RT_CHECK(c->weight >= 1 && c->weight <= 1024, RTMODT_E_INVALID, "weight %d outside 1..1024", c->weight);
    RT_CHECK(c->decay_shift >= 0 && c->decay_shift <= 16, RTMODT_E_INVALID, "decay_shift %d outside 0..16", c->decay_shift);
    RT_CHECK(c->decay_every >= 1 && c->decay_every <= 65536, RTMODT_E_INVALID, "decay_every %d outside 1..65536", c->decay_every);
    RT_CHECK(!c->classes || (c->n_classes >= 0 && c->n_classes <= PV_MAX_CLASSES), RTMODT_E_INVALID, "%d classes (0..%d)", c->n_classes,
             PV_MAX_CLASSES);
    const long long cells = (long long)cdiv(c->height, c->cell) * cdiv(c->width, c->cell) * c->n_streams;
    RT_CHECK(cells <= HM_MAX_CELLS, RTMODT_E_INVALID, "%lld cells in all (at most %lld)", cells, HM_MAX_CELLS);
    return RTMODT_OK;
}

HmStampCfg hm_stamp_cfg(const rtmodt_heatmap_cfg &c, const int32_t *classes) {
    static_assert(RTMODT_HEATMAP_BOX == HM_BOX && RTMODT_HEATMAP_DISC == HM_DISC && RTMODT_HEATMAP_FOOT == HM_FOOT, "footprint kinds");
    return HmStampCfg{c.footprint, c.foot_radius, c.cell, classes, c.n_classes};
}

// the stamps of one stream's boxes, in box order
int hm_pack_boxes(const HmStampCfg &sc, const float *xyxy, const int32_t *cls, int n_boxes, int h, int w, int stream, std::vector<HmStamp> &out) {
    RT_CHECK(n_boxes >= 0 && (n_boxes == 0 || xyxy), RTMODT_E_INVALID, "stream %d: bad box list", stream);
    RT_CHECK(n_boxes <= HM_MAX_BOXES, RTMODT_E_CAPACITY, "stream %d: %d boxes in one frame (at most %d)", stream, n_boxes, HM_MAX_BOXES);
    RT_CHECK(n_boxes == 0 || cls || !sc.classes, RTMODT_E_INVALID, "stream %d: a class list needs the boxes' classes", stream);
    for (int i = 0; i < n_boxes; ++i) {
        const float *b = xyxy + 4 * (size_t)i;
        RT_CHECK(pv_finite(b[0]) && pv_finite(b[1]) && pv_finite(b[2]) && pv_finite(b[3]), RTMODT_E_INVALID,
                 "stream %d box %d: NaN or infinite coordinate", stream, i);
        HmStamp st;
        if (hm_stamp(sc, b[0], b[1], b[2], b[3], cls ? cls[i] : 0, h, w, st)) out.push_back(st);
    }
    return RTMODT_OK;
}

// Everything after the argument checks of an accumulate call: [gather] + accumulate on stream q, then the call is counted.
// host_stamps: one list per stream (host form); g: the gather launch (device forms).
int hm_accumulate(rtmodt_heatmap *p, hipStream_t q, const std::vector<std::vector<HmStamp>> *host_stamps, HmGatherArgs *g) {
    p->timer.timed = false;
    RT_HIP(hipSetDevice(p->device));
    const rtmodt_heatmap_cfg &c = p->cfg;
    const int S = c.n_streams;
    HmAccArgs a{};
    a.grid = p->d_grid; a.gstride = p->cells; a.gw = p->gw; a.gh = p->gh; a.cell = c.cell;
    a.tiles_x = cdiv(p->gw, HM_TW);
    a.weight = c.weight;
    a.decay_shift = (c.decay_shift && (p->calls + 1) % (uint64_t)c.decay_every == 0) ? c.decay_shift : 0;
    if (host_stamps) {
        size_t n_stamps = 0;
        for (const auto &v : *host_stamps) n_stamps += v.size();
        const size_t off_stamps = align_up((size_t)S * sizeof(HmStream), 16), bytes = off_stamps + std::max<size_t>(n_stamps, 1) * sizeof(HmStamp);
        RT_TRY(p->cmd.reserve(bytes));
        HmStream *hs = (HmStream *)p->cmd.h;
        HmStamp *st = (HmStamp *)(p->cmd.h + off_stamps);
        size_t so = 0;
        for (int s = 0; s < S; ++s) {
            const auto &v = (*host_stamps)[s];
            hs[s] = HmStream{(int64_t)so, (int32_t)v.size(), 0};
            if (!v.empty()) memcpy(st + so, v.data(), v.size() * sizeof(HmStamp));
            so += v.size();
        }
        RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, bytes, hipMemcpyHostToDevice, q));
        a.streams = (const HmStream *)p->cmd.d; a.stamps = (const HmStamp *)(p->cmd.d + off_stamps);
    } else {
        a.stamps = g->out; a.n_dev = g->n_out; a.cap = g->cap;
    }
    const dim3 grid((unsigned)(a.tiles_x * cdiv(p->gh, HM_TH)), S), block(HM_THREADS);
    RT_TRY(p->timer.record(0, q));
    if (g) hipLaunchKernelGGL(heatmap_gather, dim3(S), block, 0, q, *g);
    hipLaunchKernelGGL(heatmap_accumulate, grid, block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_HIP(hipStreamSynchronize(q));
    ++p->calls;
    p->timer.timed = true;
    return RTMODT_OK;
}

// a device form: the gather buffers for the handle's streams of at most cap boxes, then hm_accumulate on the source's stream
template <typename F> int hm_accumulate_view(rtmodt_heatmap *p, int src_device, int n, int cap, hipStream_t q, const char *what, F fill) {
    RT_CHECK(src_device == p->device, RTMODT_E_INVALID, "heatmap on device %d, its source on device %d", p->device, src_device);
    RT_CHECK(n == p->cfg.n_streams, RTMODT_E_INVALID, "%s has %d streams, the heatmap %d", what, n, p->cfg.n_streams);
    RT_CHECK(cap >= 1 && cap <= HM_MAX_BOXES, RTMODT_E_CAPACITY, "the source holds up to %d boxes per frame (at most %d)", cap, HM_MAX_BOXES);
    RT_HIP(hipSetDevice(p->device));
    RT_TRY(dev_grow(&p->d_gather, &p->gather_bytes, (size_t)n * cap * sizeof(HmStamp)));
    HmGatherArgs g{};
    g.sc = hm_stamp_cfg(p->cfg, p->cfg.classes ? p->d_classes : nullptr);
    g.h = p->cfg.height; g.w = p->cfg.width; g.cap = cap; g.out = p->d_gather; g.n_out = p->d_gn;
    fill(g);
    return hm_accumulate(p, q, nullptr, &g);
}

template <typename T> int hm_accumulate_tracker(rtmodt_heatmap *p, T *trk, int report_tsu) {
    RT_CHECK(p && trk, RTMODT_E_INVALID, "null argument");
    TrackSrc src;
    TrackViewBase v;
    RT_TRY(track_src(trk, report_tsu, &src, &v));
    return hm_accumulate_view(p, v.device, v.n_streams, v.max_tracks, v.stream, "the tracker", [&](HmGatherArgs &g) { g.trk = src; });
}

int hm_check_stream(const rtmodt_heatmap *p, int stream) {
    RT_CHECK(stream >= 0 && stream < p->cfg.n_streams, RTMODT_E_INVALID, "stream %d outside 0..%d", stream, p->cfg.n_streams - 1);
    return RTMODT_OK;
}

void hm_jet(uint8_t *lut) {
    for (int v = 0; v < 256; ++v)
        for (int c = 0; c < 3; ++c) {                       // c: B G R; k = 1, 2, 3
            const int t = 8 * v - 510 * (c + 1);
            const int u = std::max(0, 765 - (t < 0 ? -t : t)) >> 1;
            lut[3 * v + c] = (uint8_t)std::min(u, 255);
        }
}

}  // namespace

extern "C" {

void rtmodt_heatmap_default_cfg(rtmodt_heatmap_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_heatmap_cfg{};
    cfg->n_streams = 1; cfg->height = 0; cfg->width = 0;
    cfg->cell = 4; cfg->footprint = RTMODT_HEATMAP_DISC; cfg->foot_radius = 0;
    cfg->weight = 1; cfg->decay_shift = 0; cfg->decay_every = 1;
    cfg->classes = nullptr; cfg->n_classes = 0; cfg->device = 0;
}

void rtmodt_heatmap_destroy(rtmodt_heatmap *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_grid); hipFree(p->d_maxpart); hipFree(p->d_part); hipFree(p->d_lut); p->cmd.release(); p->stage.release();
        hipFree(p->d_gather); hipFree(p->d_gn); hipFree(p->d_classes);
        hipHostFree(p->h_part);
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_heatmap_create(const rtmodt_heatmap_cfg *cfg, rtmodt_heatmap **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(hm_check_cfg(cfg));
    rtmodt_heatmap *p = new rtmodt_heatmap();
    p->device = cfg->device;
    p->cfg = *cfg;
    if (cfg->classes) {
        p->classes.assign(cfg->classes, cfg->classes + cfg->n_classes);
        p->classes.push_back(0);                            // (never read: keeps data() non-null for an empty list)
        p->cfg.classes = p->classes.data();
    } else {
        p->cfg.n_classes = 0;
    }
    p->gw = cdiv(cfg->width, cfg->cell); p->gh = cdiv(cfg->height, cfg->cell);
    p->cells = (long long)p->gw * p->gh;
    auto body = [&]() -> int {
        const size_t S = (size_t)p->cfg.n_streams;
        uint8_t lut[768];
        hm_jet(lut);
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_grid, S * p->cells * sizeof(uint32_t)));
        RT_HIP(handle_zero(p->d_grid, S * p->cells * sizeof(uint32_t), p->stream));
        RT_HIP(hipMalloc((void **)&p->d_maxpart, S * HM_PARTS * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_part, (size_t)HM_MAX_POLYS * HM_PARTS * sizeof(unsigned long long)));
        RT_HIP(hipHostMalloc((void **)&p->h_part, (size_t)HM_MAX_POLYS * HM_PARTS * sizeof(unsigned long long), hipHostMallocDefault));
        RT_HIP(hipMalloc((void **)&p->d_gn, S * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_lut, sizeof(lut)));
        RT_HIP(hipMemcpy(p->d_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
        if (p->cfg.classes) {
            RT_HIP(hipMalloc((void **)&p->d_classes, p->classes.size() * sizeof(int32_t)));
            RT_HIP(hipMemcpy(p->d_classes, p->classes.data(), p->classes.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_heatmap_destroy, out);
}

int rtmodt_heatmap_footprint(const rtmodt_heatmap_cfg *cfg, const float *xyxy, int32_t cls, int32_t *cells_xy, int cap_cells, int32_t *needed) {
    RT_CHECK(needed && xyxy, RTMODT_E_INVALID, "null argument");
    RT_TRY(hm_check_cfg(cfg));
    RT_CHECK(pv_finite(xyxy[0]) && pv_finite(xyxy[1]) && pv_finite(xyxy[2]) && pv_finite(xyxy[3]), RTMODT_E_INVALID, "NaN or infinite coordinate");
    HmStamp st;
    long long n = 0;
    if (hm_stamp(hm_stamp_cfg(*cfg, cfg->classes), xyxy[0], xyxy[1], xyxy[2], xyxy[3], cls, cfg->height, cfg->width, st)) {
        for (int pass = 0; pass < 2; ++pass) {              // count, then write if they fit
            if (pass == 1 && !(cells_xy && cap_cells >= n)) break;
            long long k = 0;
            for (int cy = st.cy0; cy <= st.cy1; ++cy)
                for (int cx = st.cx0; cx <= st.cx1; ++cx)
                    if (hm_covers(st, cfg->cell, cx, cy)) {
                        if (pass == 1) { cells_xy[2 * k] = cx; cells_xy[2 * k + 1] = cy; }
                        ++k;
                    }
            n = k;
        }
    }
    *needed = (int32_t)n;
    return RTMODT_OK;
}

int rtmodt_heatmap_accumulate(rtmodt_heatmap *p, const float *const *xyxy, const int32_t *const *cls, const int32_t *n_boxes) {
    RT_CHECK(p && xyxy && n_boxes, RTMODT_E_INVALID, "null argument");
    const HmStampCfg sc = hm_stamp_cfg(p->cfg, p->cfg.classes);
    std::vector<std::vector<HmStamp>> stamps(p->cfg.n_streams);
    for (int s = 0; s < p->cfg.n_streams; ++s)
        RT_TRY(hm_pack_boxes(sc, xyxy[s], cls ? cls[s] : nullptr, n_boxes[s], p->cfg.height, p->cfg.width, s, stamps[s]));
    return hm_accumulate(p, p->stream, &stamps, nullptr);
}

int rtmodt_heatmap_accumulate_tracker(rtmodt_heatmap *p, rtmodt_tracker *trk, int report_tsu) { return hm_accumulate_tracker(p, trk, report_tsu); }
int rtmodt_heatmap_accumulate_deepsort(rtmodt_heatmap *p, rtmodt_deepsort *ds, int report_tsu) { return hm_accumulate_tracker(p, ds, report_tsu); }
int rtmodt_heatmap_accumulate_ocsort(rtmodt_heatmap *p, rtmodt_ocsort *oc) { return hm_accumulate_tracker(p, oc, 0); }
int rtmodt_heatmap_accumulate_botsort(rtmodt_heatmap *p, rtmodt_botsort *bot) { return hm_accumulate_tracker(p, bot, 0); }

int rtmodt_heatmap_accumulate_detector(rtmodt_heatmap *p, rtmodt_detector *det) {
    RT_CHECK(p && det, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(detector_outputs(det, &o));
    return hm_accumulate_view(p, o.device, o.count, o.stride, o.stream, "the detector's newest batch",
                              [&](HmGatherArgs &g) { g.det_box = o.box; g.det_cls = o.cls; g.det_n = o.n; g.det_stride = o.stride; });
}

int rtmodt_heatmap_set_colormap(rtmodt_heatmap *p, const uint8_t *lut_bgr) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    uint8_t lut[768];
    if (lut_bgr) memcpy(lut, lut_bgr, sizeof(lut));
    else hm_jet(lut);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpy(p->d_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
    return RTMODT_OK;
}

int rtmodt_heatmap_overlay(rtmodt_heatmap *p, uint8_t *const *frames, const int32_t *streams, int n, int h, int w, int stride_bytes, int mem_kind,
                           int alpha, int min_level, uint32_t scale_max) {
    RT_CHECK(p && n >= 0 && (n == 0 || frames), RTMODT_E_INVALID, "bad argument");
    RT_TRY(check_mem_kind(mem_kind));                      // (the geometry is the handle's: this entry point words its own refusals)
    RT_CHECK(h == p->cfg.height && w == p->cfg.width, RTMODT_E_INVALID, "frames of %dx%d, the heatmap was created for %dx%d", w, h, p->cfg.width,
             p->cfg.height);
    RT_CHECK(pitch_holds(stride_bytes, w), RTMODT_E_INVALID, "stride %d below 3 x %d", stride_bytes, w);
    RT_CHECK(alpha >= 0 && alpha <= 256, RTMODT_E_INVALID, "alpha %d outside 0..256", alpha);
    RT_CHECK(min_level >= 1 && min_level <= 255, RTMODT_E_INVALID, "min_level %d outside 1..255", min_level);
    RT_CHECK(n <= 65535, RTMODT_E_CAPACITY, "%d frames in one call (at most 65535)", n);
    RT_CHECK(streams || n == p->cfg.n_streams || n == 0, RTMODT_E_INVALID, "%d frames for %d streams and no stream list", n, p->cfg.n_streams);
    for (int i = 0; i < n; ++i) {
        RT_CHECK(frames[i], RTMODT_E_INVALID, "frame %d is null", i);
        if (streams) RT_TRY(hm_check_stream(p, streams[i]));
    }
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_TIGHT16));
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(HmOvFrame)));
    HmOvFrame *F = (HmOvFrame *)p->cmd.h;
    for (int i = 0; i < n; ++i) F[i] = HmOvFrame{(uint64_t)(uintptr_t)p->stage.at(frames, i), streams ? streams[i] : i, 0};
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(HmOvFrame), hipMemcpyHostToDevice, q));
    RT_TRY(p->stage.copy_in(frames, q));
    HmOvArgs a{};
    a.frames = (const HmOvFrame *)p->cmd.d; a.grid = p->d_grid; a.gstride = p->cells; a.gw = p->gw;
    a.cell_shift = p->cfg.cell == 1 ? 0 : p->cfg.cell == 2 ? 1 : p->cfg.cell == 4 ? 2 : p->cfg.cell == 8 ? 3 : 4;
    a.h = h; a.w = w; a.tiles_x = cdiv(w, HM_TW);
    a.stride = (long long)p->stage.pitch;
    a.alpha = alpha; a.min_level = min_level; a.scale_max = scale_max;
    a.maxpart = p->d_maxpart; a.lut = p->d_lut;
    const dim3 block(HM_THREADS);
    RT_TRY(p->timer.record(0, q));
    if (!scale_max) hipLaunchKernelGGL(heatmap_max, dim3(HM_PARTS, p->cfg.n_streams), block, 0, q, (const uint32_t *)p->d_grid, p->cells, p->d_maxpart);
    hipLaunchKernelGGL(heatmap_overlay, dim3((unsigned)(a.tiles_x * cdiv(h, HM_TH)), n), block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_TRY(p->stage.copy_out(frames, q));
    RT_HIP(hipStreamSynchronize(q));
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_heatmap_zone_sums(rtmodt_heatmap *p, int stream, const int32_t *const *polygons_xy, const int32_t *n_points, int n, uint64_t *sums) {
    RT_CHECK(p && n >= 0 && (n == 0 || (polygons_xy && n_points && sums)), RTMODT_E_INVALID, "bad argument");
    RT_TRY(hm_check_stream(p, stream));
    RT_CHECK(n <= HM_MAX_POLYS, RTMODT_E_CAPACITY, "%d polygons (at most %d)", n, HM_MAX_POLYS);
    PolyTable T;
    RT_TRY(T.build(polygons_xy, n_points, n, HM_MAX_POINTS, "polygon"));
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    const size_t total = T.layout();
    RT_TRY(p->cmd.reserve(total));
    T.write(p->cmd.h);
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, total, hipMemcpyHostToDevice, q));
    HmZoneArgs a{};
    a.grid = p->d_grid + (long long)stream * p->cells;
    a.gw = p->gw; a.gh = p->gh; a.cell = p->cfg.cell; a.h = p->cfg.height; a.w = p->cfg.width;
    T.view(p->cmd.d, &a);
    a.part = p->d_part;
    hipLaunchKernelGGL(heatmap_zone_sums, dim3(HM_PARTS, n), dim3(HM_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_HIP(hipMemcpyAsync(p->h_part, p->d_part, (size_t)n * HM_PARTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    for (int z = 0; z < n; ++z) {
        uint64_t s = 0;
        for (int k = 0; k < HM_PARTS; ++k) s += p->h_part[(size_t)z * HM_PARTS + k];
        sums[z] = s;
    }
    return RTMODT_OK;
}

int rtmodt_heatmap_read(rtmodt_heatmap *p, int stream, uint32_t *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(hm_check_stream(p, stream));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(out, p->d_grid + (long long)stream * p->cells, (size_t)p->cells * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_heatmap_load(rtmodt_heatmap *p, int stream, const uint32_t *in) {
    RT_CHECK(p && in, RTMODT_E_INVALID, "null argument");
    RT_TRY(hm_check_stream(p, stream));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_grid + (long long)stream * p->cells, in, (size_t)p->cells * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_heatmap_reset(rtmodt_heatmap *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(hm_check_stream(p, stream));
    RT_HIP(hipSetDevice(p->device));
    uint32_t *g = p->d_grid + (stream < 0 ? 0 : (long long)stream * p->cells);
    RT_HIP(hipMemsetAsync(g, 0, (size_t)p->cells * sizeof(uint32_t) * (stream < 0 ? p->cfg.n_streams : 1), p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_heatmap_last_ms(rtmodt_heatmap *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no accumulate or overlay call has launched yet");
}

}  // extern "C"
