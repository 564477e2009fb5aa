// privacy.hip -- privacy masking of BGR24 frames on the GPU: tracked people / objects and fixed privacy zones are filled,
// pixelated or blurred before a frame is recorded, encoded or served.  The reference has no counterpart (PARITY UNPINNED against
// cv2.blur / GaussianBlur and against any camera's privacy mask); tests/privacy_ref.py restates every rule below in NumPy and
// the kernels equal it byte for byte -- every rule is integer arithmetic.
//
// Paint rules.  Pixel centres are integer coordinates.
//   mask(x, y): the pixel lies in a region rectangle of its frame (privacy_regions.h turns a box into one), or inside or on one
//     of the handle's privacy polygons -- inside_or_on of polygon.h, the zone engine's test.  Limits (the renderer's): 32
//     polygons, 2048 points, 65536 regions per frame.
//   Unmasked pixels and the bytes past 3w of a row are never written.  A masked pixel becomes
//   FILL:      the constant BGR colour;
//   PIXELATE:  (cell 2..64) the cells form a grid anchored at the frame origin, edge cells clipped to the frame; per channel
//              m = (sum + n/2) / n in integer division over ALL n in-frame pixels of the cell (masked or not) of the frame as
//              it was before the call; the pixel takes its cell's m.  (10, 11, 12, 14 -> 12; a clipped cell of 1, 2 -> 2.)
//   BLUR:      (radius r 1..16, passes 1..3) one pass maps a u8 image to a u8 image: each output is (sum + n/2) / n over the
//              window [x-r, x+r] x [y-r, y+r] clipped to the frame, n the clipped window's pixel count.  Pass k reads the WHOLE
//              pass k-1 image, not only its masked pixels; a masked pixel takes the last pass's value.  Window sums are exact
//              integers (<= 33^2 * 255), so the separable running sums used here give the same bits.
//   Hazard rule: every output is a function of the frame as it was before the call and of nothing else.  FILL reads nothing;
//     a PIXELATE workgroup owns whole cells (its tile is a multiple of the cell both ways) and reads only those; BLUR reads
//     neighbours another workgroup may already have overwritten, so in place it writes the masked pixels of every tile into a
//     scratch image of the handle (with the tile's mask bits) and a second launch commits them.  Out of place (dst != src) dst
//     is first made a copy of src and the kernels read src and write dst.  No grid-wide barrier, no spin, no atomics.
//
// Kernels (256 threads; the launch count per call is fixed: [gather] + paint or blur + [commit], at most three):
//   privacy_gather  device forms only: one workgroup per frame turns the passed tracks of a tracker's device-resident state (the
//                   rule of the matching rtmodt_crossing_process_*) or a detector's device-resident detections into rectangles;
//   privacy_paint   FILL / PIXELATE.  Tile = 64 x 16 (FILL) or cell * (64 / cell) x cell * max(1, 16 / cell) (PIXELATE, at most
//                   64 x 64).  The frame's rectangles are culled against the tile 256 at a time into LDS (capacity does not
//                   depend on LDS), then tested per pixel; the polygons (staged in LDS whole) after them.  A tile that meets no
//                   rectangle and no polygon, or in which no pixel turns out masked, returns before it reads a byte of the frame;
//   privacy_blur    tile 64 x 16 with a halo of radius * passes <= 48 pixels, one channel at a time: a u8 plane (<= 160 x 112)
//                   and a u16 plane of row sums in LDS (54 656 B), each pass a horizontal and a vertical running sum over a
//                   region that shrinks by `radius` per pass; row strides are an odd number of dwords;
//   privacy_commit  in-place BLUR only: copies the masked pixels of the scratch image into the frame.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "frame_stage.h"
#include "handle_host.h"
#include "polygon.h"

#define PV_HD __host__ __device__
#include "privacy_regions.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_select_dev.h"

constexpr int PV_THREADS = 256, PV_WAVES = PV_THREADS / 64, PV_TW = 64, PV_TH = 16;
constexpr int PV_MAX_POLYS = 32, PV_MAX_POINTS = 2048, PV_MAX_REGIONS = 65536;
constexpr int PV_MAX_HALO = 48;
constexpr int PV_A_STRIDE_MAX = ((((PV_TW + 2 * PV_MAX_HALO) + 3) >> 2) | 1) * 4;          // 164 bytes
constexpr int PV_B_STRIDE_MAX = ((((PV_TW + 2 * PV_MAX_HALO) + 1) >> 1) | 1) * 2;          // 162 u16
constexpr int PV_A_BYTES = PV_A_STRIDE_MAX * (PV_TH + 2 * PV_MAX_HALO);                    // 18 368
constexpr int PV_B_BYTES = PV_B_STRIDE_MAX * 2 * (PV_TH + 2 * PV_MAX_HALO);                // 36 288
static_assert(PV_A_BYTES % 16 == 0 && PV_A_BYTES + PV_B_BYTES <= 56 * 1024, "blur LDS");
static_assert(PV_A_BYTES + PV_B_BYTES >= PV_THREADS * 16 + PV_MAX_POINTS * 8, "the mask phase's tables alias the blur planes");

struct PvFrame { uint64_t src, dst; int64_t rect_off; int32_t n_rects, pad; };
static_assert(sizeof(PvFrame) == 32 && sizeof(PvRect) == 16, "layout");

struct PolyView { const int2 *pts; const int32_t *off; const int4 *bbox; int Z, n_pts; int4 stage; };

struct PaintArgs {
    const PvFrame *frames; const PvRect *rects;
    const int32_t *n_dev; int cap;              // device forms: the gathered count of frame f, at most cap
    int h, w, tw, th, tiles_x, tiles;
    long long stride;
    int mode, cell, radius, passes;
    uint32_t fill;
    PolyView pv;
    uint8_t *scratch; long long spitch, sframe; uint8_t *maskbuf;       // in-place BLUR
};

struct GatherArgs {
    PvRegionCfg rc;                             // classes: a device pointer
    int h, w, cap;
    PvRect *out; int32_t *n_out;
    TrackSrc trk;                               // tracks (track_select_dev.h), or the detections below
    const float4 *det_box; const int32_t *det_cls, *det_n; int det_stride;
};

__device__ __forceinline__ bool pv_overlaps(const PvRect &b, int x0, int y0, int x1, int y1) {
    return b.x0 <= x1 && b.x1 >= x0 && b.y0 <= y1 && b.y1 >= y0;
}

// (sum + n/2) / n exactly: sum + n/2 < 2^24, so the float product is within 1 of the quotient and the remainder settles it
__device__ __forceinline__ int pv_div_round(int sum, int n) {
    const int a = sum + (n >> 1);
    int q = (int)((float)a * __builtin_amdgcn_rcpf((float)n));
    const int rem = a - q * n;
    q += (rem >= n ? 1 : 0) - (rem < 0 ? 1 : 0);
    return q;
}

// The mask bits of this thread's pixels (x, y0 + 4k), k < NP, of which those with bit k of `have` set exist, in tile
// (tx0, ty0)..(tx1, ty1).  s_rect[PV_THREADS], s_pts[PV_MAX_POINTS], s_wcnt[PV_WAVES]: LDS.  Uniform control flow.
template <int NP>
__device__ __forceinline__ uint32_t pv_mask(const PaintArgs &a, const PvFrame &fr, int frame, int tx0, int ty0, int tx1, int ty1, int x, int y0,
                                            uint32_t have, PvRect *s_rect, int2 *s_pts, int *s_wcnt) {
    const int tid = threadIdx.x;
    uint32_t mask = 0;
    int nreg = fr.n_rects;
    if (a.n_dev) {
        nreg = a.n_dev[frame];
        nreg = nreg < 0 ? 0 : (nreg > a.cap ? a.cap : nreg);
    }
    const PvRect *rects = a.rects + fr.rect_off;
    for (int ib = 0; ib < nreg; ib += PV_THREADS) {
        const int i = ib + tid;
        PvRect rc{0, 0, -1, -1};
        bool f = false;
        if (i < nreg) {
            rc = rects[i];
            f = pv_overlaps(rc, tx0, ty0, tx1, ty1);
        }
        int m;
        const int pos = block_scan_count<PV_WAVES>(f ? 1 : 0, s_wcnt, m);
        if (f) s_rect[pos] = rc;
        __syncthreads();
        for (int e = 0; e < m && mask != have; ++e) {
            const PvRect b = s_rect[e];
            if (x < b.x0 || x > b.x1) continue;
#pragma unroll
            for (int k = 0; k < NP; ++k)
                if (y0 + 4 * k >= b.y0 && y0 + 4 * k <= b.y1) mask |= 1u << k;
            mask &= have;
        }
        __syncthreads();
    }
    const PolyView &pv = a.pv;
    if (pv.Z > 0 && pv.stage.x <= tx1 && pv.stage.z >= tx0 && pv.stage.y <= ty1 && pv.stage.w >= ty0) {
        for (int i = tid; i < pv.n_pts; i += PV_THREADS) s_pts[i] = pv.pts[i];
        __syncthreads();
        for (int k = 0; k < NP; ++k) {
            if (!((have >> k) & 1u) || ((mask >> k) & 1u)) continue;
            const int y = y0 + 4 * k;
            bool inside = false;
            for (int z = 0; z < pv.Z && !inside; ++z) {
                const int4 b = pv.bbox[z];
                if (x >= b.x && x <= b.z && y >= b.y && y <= b.w) {
                    const int p0 = pv.off[z];
                    inside = inside_or_on(s_pts + p0, pv.off[z + 1] - p0, x, y);
                }
            }
            if (inside) mask |= 1u << k;
        }
    }
    return mask;
}

__device__ __forceinline__ void pv_store_px(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
}

// ---- FILL / PIXELATE -------------------------------------------------------------------------------------------------
constexpr int PV_NP = 16;                       // a tile holds at most 64 x 64 pixels: thread t owns (t % 64, t / 64 + 4k), k < 16

__global__ __launch_bounds__(PV_THREADS) void privacy_paint(PaintArgs a) {
    __shared__ __attribute__((aligned(16))) PvRect s_rect[PV_THREADS];
    __shared__ __attribute__((aligned(16))) unsigned char s_u[PV_MAX_POINTS * 8];       // the polygon points, then the tile's pixels
    __shared__ int s_part[512 * 3];
    __shared__ uint32_t s_mean[256];
    __shared__ int s_wcnt[PV_WAVES];

    const int tid = threadIdx.x, frame = blockIdx.y;
    const PvFrame fr = a.frames[frame];
    const int tw = a.tw, th = a.th;
    const int tx0 = (blockIdx.x % a.tiles_x) * tw, ty0 = (blockIdx.x / a.tiles_x) * th;
    const int tx1 = min(tx0 + tw - 1, a.w - 1), ty1 = min(ty0 + th - 1, a.h - 1);
    const int lx = tid & 63, ly0 = tid >> 6, x = tx0 + lx, y0 = ty0 + ly0;
    uint32_t have = 0;
    if (x <= tx1)
        for (int k = 0; k < PV_NP; ++k)
            if (y0 + 4 * k <= ty1) have |= 1u << k;
    const uint32_t mask = pv_mask<PV_NP>(a, fr, frame, tx0, ty0, tx1, ty1, x, y0, have, s_rect, (int2 *)s_u, s_wcnt);
    if (!__syncthreads_or(mask != 0)) return;               // nothing masked here: not a byte of the frame is read

    uint8_t *dst = (uint8_t *)fr.dst + (long long)y0 * a.stride + 3LL * x;
    if (a.mode == RTMODT_PRIVACY_FILL) {
        for (int k = 0; k < PV_NP; ++k)
            if ((mask >> k) & 1u) pv_store_px(dst + 4LL * k * a.stride, a.fill);
        return;
    }
    // PIXELATE: the tile's in-frame pixels (zeros outside), row sums per (row, cell column), then the cells' means
    const uint8_t *src = (const uint8_t *)fr.src + (long long)y0 * a.stride + 3LL * x;
    const int cell = a.cell, cx = tw / cell, cy = th / cell;
    if (lx < tw)
        for (int k = 0; k < PV_NP && ly0 + 4 * k < th; ++k) {
            uint32_t b = 0, g = 0, r = 0;
            if ((have >> k) & 1u) {
                const uint8_t *s = src + 4LL * k * a.stride;
                b = s[0]; g = s[1]; r = s[2];
            }
            unsigned char *o = s_u + 3 * ((ly0 + 4 * k) * tw + lx);
            o[0] = (unsigned char)b; o[1] = (unsigned char)g; o[2] = (unsigned char)r;
        }
    __syncthreads();
    for (int p = tid; p < th * cx; p += PV_THREADS) {
        const int ly = p / cx, j = p - ly * cx;
        const unsigned char *s = s_u + 3 * (ly * tw + j * cell);
        int b = 0, g = 0, r = 0;
        for (int i = 0; i < cell; ++i) { b += s[3 * i]; g += s[3 * i + 1]; r += s[3 * i + 2]; }
        s_part[3 * p] = b; s_part[3 * p + 1] = g; s_part[3 * p + 2] = r;
    }
    __syncthreads();
    for (int q = tid; q < cx * cy; q += PV_THREADS) {
        const int iy = q / cx, j = q - iy * cx;
        const int x0c = tx0 + j * cell, y0c = ty0 + iy * cell;
        if (x0c >= a.w || y0c >= a.h) continue;
        const int n = (min(x0c + cell, a.w) - x0c) * (min(y0c + cell, a.h) - y0c);
        int b = 0, g = 0, r = 0;
        for (int i = 0; i < cell; ++i) {
            const int *s = s_part + 3 * ((iy * cell + i) * cx + j);
            b += s[0]; g += s[1]; r += s[2];
        }
        s_mean[q] = (uint32_t)pv_div_round(b, n) | (uint32_t)pv_div_round(g, n) << 8 | (uint32_t)pv_div_round(r, n) << 16;
    }
    __syncthreads();
    const int qx = lx / cell;
    for (int k = 0; k < PV_NP; ++k)
        if ((mask >> k) & 1u) pv_store_px(dst + 4LL * k * a.stride, s_mean[((ly0 + 4 * k) / cell) * cx + qx]);
}

// ---- BLUR ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PV_THREADS) void privacy_blur(PaintArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PV_A_BYTES + PV_B_BYTES];
    __shared__ int s_wcnt[PV_WAVES];

    const int tid = threadIdx.x, frame = blockIdx.y;
    const PvFrame fr = a.frames[frame];
    const int tx0 = (blockIdx.x % a.tiles_x) * PV_TW, ty0 = (blockIdx.x / a.tiles_x) * PV_TH;
    const int tx1 = min(tx0 + PV_TW - 1, a.w - 1), ty1 = min(ty0 + PV_TH - 1, a.h - 1);
    const int lx = tid & 63, ly0 = tid >> 6;                                    // pixel k: (lx, ly0 + 4k)
    uint32_t have = 0;
    if (tx0 + lx <= tx1)
        for (int k = 0; k < 4; ++k)
            if (ty0 + ly0 + 4 * k <= ty1) have |= 1u << k;
    const uint32_t mask = pv_mask<4>(a, fr, frame, tx0, ty0, tx1, ty1, tx0 + lx, ty0 + ly0, have, (PvRect *)smem,
                                     (int2 *)(smem + PV_THREADS * sizeof(PvRect)), s_wcnt);
    uint8_t *maskp = a.maskbuf ? a.maskbuf + ((size_t)frame * a.tiles + blockIdx.x) * PV_THREADS + tid : nullptr;
    if (maskp) *maskp = (uint8_t)mask;
    if (!__syncthreads_or(mask != 0)) return;               // nothing masked here: not a byte of the frame is read

    const int r = a.radius, P = a.passes, R = r * P;
    const int RW = PV_TW + 2 * R, RH = PV_TH + 2 * R;
    const int sa = (((RW + 3) >> 2) | 1) * 4, sb = (((RW + 1) >> 1) | 1) * 2;
    unsigned char *A = smem;
    uint16_t *B = (uint16_t *)(smem + PV_A_BYTES);
    const int gx0 = tx0 - R, gy0 = ty0 - R;
    const uint8_t *src = (const uint8_t *)fr.src;
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    for (int c = 0; c < 3; ++c) {
        for (int ry = tid / RW, rx = tid - ry * RW; ry < RH;) {
            const int gx = gx0 + rx, gy = gy0 + ry;
            A[ry * sa + rx] = (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) ? src[(long long)gy * a.stride + 3LL * gx + c] : (uint8_t)0;
            rx += PV_THREADS;
            while (rx >= RW) { rx -= RW; ++ry; }
        }
        __syncthreads();
        for (int p = 0; p < P; ++p) {
            const int m_out = r * (P - 1 - p), m_in = m_out + r;
            const int len = PV_TW + 2 * m_out, xb = R - m_out;
            {   // horizontal: row sums of the rows within m_in of the tile
                const int lines = PV_TH + 2 * m_in, yb = R - m_in;
                const int segs = max(1, PV_THREADS / lines), seglen = (len + segs - 1) / segs;
                const int seg = tid / lines, line = tid - seg * lines;
                const int xs = seg * seglen, xe = min(len, xs + seglen);
                if (seg < segs && xs < xe) {
                    const unsigned char *row = A + (yb + line) * sa;
                    uint16_t *brow = B + (yb + line) * sb;
                    int x = xb + xs, sum = 0;
                    for (int d = -r; d <= r; ++d) sum += row[x + d];
                    brow[x] = (uint16_t)sum;
                    for (++x; x < xb + xe; ++x) {
                        sum += (int)row[x + r] - (int)row[x - r - 1];
                        brow[x] = (uint16_t)sum;
                    }
                }
            }
            __syncthreads();
            {   // vertical: window sums, rounded means; 0 outside the frame
                const int vlen = PV_TH + 2 * m_out, yb = R - m_out;
                const int segs = max(1, PV_THREADS / len), seglen = (vlen + segs - 1) / segs;
                const int seg = tid / len, col = tid - seg * len;
                const int ys = seg * seglen, ye = min(vlen, ys + seglen);
                if (seg < segs && ys < ye) {
                    const int x = xb + col, gx = gx0 + x;
                    const bool xin = gx >= 0 && gx < a.w;
                    const int nx = min(gx + r, a.w - 1) - max(gx - r, 0) + 1;
                    int y = yb + ys, sum = 0;
                    for (int d = -r; d <= r; ++d) sum += B[(y + d) * sb + x];
                    for (;; ++y) {
                        const int gy = gy0 + y;
                        int v = 0;
                        if (xin && gy >= 0 && gy < a.h) v = pv_div_round(sum, nx * (min(gy + r, a.h - 1) - max(gy - r, 0) + 1));
                        A[y * sa + x] = (unsigned char)v;
                        if (y + 1 >= yb + ye) break;
                        sum += (int)B[(y + 1 + r) * sb + x] - (int)B[(y - r) * sb + x];
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] |= (uint32_t)A[(R + ly0 + 4 * k) * sa + R + lx] << (8 * c);
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const int x = tx0 + lx, y = ty0 + ly0 + 4 * k;
        uint8_t *o = a.scratch ? a.scratch + (long long)frame * a.sframe + (long long)y * a.spitch + 3LL * x
                               : (uint8_t *)fr.dst + (long long)y * a.stride + 3LL * x;
        pv_store_px(o, out[k]);
    }
}

__global__ __launch_bounds__(PV_THREADS) void privacy_commit(PaintArgs a) {
    const int tid = threadIdx.x, frame = blockIdx.y;
    const uint32_t mask = a.maskbuf[((size_t)frame * a.tiles + blockIdx.x) * PV_THREADS + tid];
    if (!mask) return;
    const PvFrame fr = a.frames[frame];
    const int x = (blockIdx.x % a.tiles_x) * PV_TW + (tid & 63), y0 = (blockIdx.x / a.tiles_x) * PV_TH + (tid >> 6);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const int y = y0 + 4 * k;
        if (x >= a.w || y >= a.h) continue;
        const uint8_t *s = a.scratch + (long long)frame * a.sframe + (long long)y * a.spitch + 3LL * x;
        uint8_t *o = (uint8_t *)fr.dst + (long long)y * a.stride + 3LL * x;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
}

// ---- device forms: tracks / detections -> rectangles -----------------------------------------------------------------
__global__ __launch_bounds__(PV_THREADS) void privacy_gather(GatherArgs a) {
    __shared__ int s_wcnt[PV_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x;
    TrackSel src;
    if (a.det_box) src = select_list(nullptr, a.det_box + (size_t)f * a.det_stride, a.det_cls + (size_t)f * a.det_stride, a.det_n[f]);
    else src = select_tracks(a.trk, f);
    const float4 *box = src.box; const int32_t *cls = src.cls;
    const int n = src.n < 0 ? 0 : (src.n > a.cap ? a.cap : src.n);
    PvRect *out = a.out + (size_t)f * a.cap;
    int total = 0;
    for (int base = 0; base < n; base += PV_THREADS) {
        const int i = base + tid;
        bool ok = false;
        PvRect rc{0, 0, -1, -1};
        if (i < n) {
            const float4 b = box[i];
            ok = selected(src, i) && finite_bits(b.x) && finite_bits(b.y) && finite_bits(b.z) && finite_bits(b.w) &&
                 pv_region(a.rc, b.x, b.y, b.z, b.w, cls[i], a.h, a.w, rc);
        }
        int tot;
        const int pos = total + block_scan_count<PV_WAVES>(ok ? 1 : 0, s_wcnt, tot);
        if (ok) out[pos] = rc;
        total += tot;
    }
    if (tid == 0) a.n_out[f] = total;
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_privacy : HandleBase {
    rtmodt_privacy_cfg cfg{};
    std::vector<int32_t> classes;       // cfg.classes points here (or is null)
    int32_t *d_classes = nullptr;
    EventTimer<2> timer;
    char *ppool = nullptr;              // polygon table (device)
    size_t ppool_cap = 0;
    PolyView pv{};
    CmdBuf cmd;                         // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage stage;
    uint8_t *d_scratch = nullptr, *d_mask = nullptr;
    size_t scratch_cap = 0, mask_cap = 0;
    PvRect *d_gather = nullptr; int32_t *d_gn = nullptr;
    size_t gather_bytes = 0, gn_bytes = 0;
};

namespace {

int pv_check_cfg(const rtmodt_privacy_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null privacy config");
    RT_CHECK(c->mode == RTMODT_PRIVACY_FILL || c->mode == RTMODT_PRIVACY_PIXELATE || c->mode == RTMODT_PRIVACY_BLUR, RTMODT_E_INVALID,
             "privacy mode %d", c->mode);
    RT_CHECK(c->cell >= 2 && c->cell <= 64, RTMODT_E_INVALID, "cell %d outside 2..64", c->cell);
    RT_CHECK(c->radius >= 1 && c->radius <= 16, RTMODT_E_INVALID, "radius %d outside 1..16", c->radius);
    RT_CHECK(c->passes >= 1 && c->passes <= 3, RTMODT_E_INVALID, "passes %d outside 1..3", c->passes);
    RT_CHECK(c->region == RTMODT_PRIVACY_REGION_BOX || c->region == RTMODT_PRIVACY_REGION_HEAD, RTMODT_E_INVALID, "region kind %d", c->region);
    RT_CHECK(c->head_pm >= 1 && c->head_pm <= 1000, RTMODT_E_INVALID, "head_pm %d outside 1..1000", c->head_pm);
    RT_CHECK(c->expand_px >= 0 && c->expand_px <= PV_MAX_EXPAND, RTMODT_E_INVALID, "expand_px %d outside 0..%d", c->expand_px, PV_MAX_EXPAND);
    RT_CHECK(!c->classes || (c->n_classes >= 0 && c->n_classes <= PV_MAX_CLASSES), RTMODT_E_INVALID, "%d classes (0..%d)", c->n_classes,
             PV_MAX_CLASSES);
    return RTMODT_OK;
}

PvRegionCfg pv_region_cfg(const rtmodt_privacy_cfg &c, const int32_t *classes) {
    return PvRegionCfg{c.region == RTMODT_PRIVACY_REGION_HEAD ? PV_REGION_HEAD : PV_REGION_BOX, c.head_pm, c.expand_px, classes, c.n_classes};
}

// the rectangles of one frame's boxes, in box order
int pv_pack_boxes(const PvRegionCfg &rc, const float *xyxy, const int32_t *cls, int n_boxes, int h, int w, int frame, std::vector<PvRect> &out) {
    RT_CHECK(n_boxes >= 0 && (n_boxes == 0 || xyxy), RTMODT_E_INVALID, "frame %d: bad box list", frame);
    RT_CHECK(n_boxes == 0 || cls || !rc.classes, RTMODT_E_INVALID, "frame %d: a class list needs the boxes' classes", frame);
    for (int i = 0; i < n_boxes; ++i) {
        const float *b = xyxy + 4 * (size_t)i;
        RT_CHECK(pv_finite(b[0]) && pv_finite(b[1]) && pv_finite(b[2]) && pv_finite(b[3]), RTMODT_E_INVALID, "frame %d box %d: NaN or infinite coordinate",
                 frame, i);
        PvRect r;
        if (pv_region(rc, b[0], b[1], b[2], b[3], cls ? cls[i] : 0, h, w, r)) out.push_back(r);
    }
    return RTMODT_OK;
}

int pv_check_frames(uint8_t *const *frames, int n, int h, int w, int stride_bytes, int mem_kind) {
    RT_CHECK(n >= 0 && (n == 0 || frames), RTMODT_E_INVALID, "bad argument");
    return check_frames(frames, n, h, w, stride_bytes, mem_kind, kPaintFrames);
}

// Everything after the argument checks: stage host frames, send the command buffer, [gather], paint / blur, [commit], copy back.
// host_rects: one list per frame (host forms); g: the gather launch (device forms).  q: the stream everything is queued on.
int pv_execute(rtmodt_privacy *p, uint8_t *const *src, uint8_t *const *dst, int n, int h, int w, int stride_bytes, int mem_kind, hipStream_t q,
               const std::vector<std::vector<PvRect>> *host_rects, GatherArgs *g) {
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    const rtmodt_privacy_cfg &c = p->cfg;
    const bool blur = c.mode == RTMODT_PRIVACY_BLUR;
    RT_TRY(p->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_TIGHT16));
    const bool host = p->stage.host;
    bool in_place = false;
    for (int i = 0; i < n; ++i) in_place |= host || !dst || dst[i] == src[i];
    const bool scratch = blur && in_place;

    PaintArgs a{};
    a.h = h; a.w = w; a.stride = (long long)p->stage.pitch;
    a.mode = c.mode; a.cell = c.cell; a.radius = c.radius; a.passes = c.passes;
    a.fill = c.fill_bgr[0] | (uint32_t)c.fill_bgr[1] << 8 | (uint32_t)c.fill_bgr[2] << 16;
    a.tw = PV_TW; a.th = PV_TH;
    if (c.mode == RTMODT_PRIVACY_PIXELATE) { a.tw = c.cell * (PV_TW / c.cell); a.th = c.cell * std::max(1, PV_TH / c.cell); }
    a.tiles_x = cdiv(w, a.tw);
    const long long tiles = (long long)a.tiles_x * cdiv(h, a.th);
    RT_CHECK(tiles <= INT32_MAX, RTMODT_E_INVALID, "frame too large");
    a.tiles = (int)tiles;
    a.pv = p->pv;
    if (scratch) {
        a.spitch = (long long)tight16_pitch(w); a.sframe = (long long)h * a.spitch;      // the blur's scratch copy has the staged layout
        RT_TRY(dev_grow(&p->d_scratch, &p->scratch_cap, (size_t)n * a.sframe));
        RT_TRY(dev_grow(&p->d_mask, &p->mask_cap, (size_t)n * tiles * PV_THREADS));
        a.scratch = p->d_scratch; a.maskbuf = p->d_mask;
    }

    // command buffer: PvFrame[n] | PvRect[...]
    size_t n_rects = 0;
    if (host_rects) for (const auto &v : *host_rects) n_rects += v.size();
    const size_t off_rects = align_up((size_t)n * sizeof(PvFrame), 16), bytes = off_rects + std::max<size_t>(n_rects, 1) * sizeof(PvRect);
    RT_TRY(p->cmd.reserve(bytes));
    PvFrame *F = (PvFrame *)p->cmd.h;
    PvRect *Rr = (PvRect *)(p->cmd.h + off_rects);
    size_t ro = 0;
    for (int i = 0; i < n; ++i) {
        uint8_t *s = p->stage.at(src, i);
        uint8_t *d = host ? s : (dst ? dst[i] : src[i]);
        F[i] = PvFrame{(uint64_t)(uintptr_t)s, (uint64_t)(uintptr_t)d, 0, 0, 0};
        if (host_rects) {
            const auto &v = (*host_rects)[i];
            F[i].rect_off = (int64_t)ro; F[i].n_rects = (int32_t)v.size();
            if (!v.empty()) memcpy(Rr + ro, v.data(), v.size() * sizeof(PvRect));
            ro += v.size();
        } else {
            F[i].rect_off = (int64_t)i * g->cap;
        }
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, bytes, hipMemcpyHostToDevice, q));
    a.frames = (const PvFrame *)p->cmd.d;
    if (host_rects) {
        a.rects = (const PvRect *)(p->cmd.d + off_rects);
    } else {
        a.rects = g->out; a.n_dev = g->n_out; a.cap = g->cap;
    }
    RT_TRY(p->stage.copy_in(src, q));
    for (int i = 0; i < n; ++i)
        if (!host && dst && dst[i] != src[i]) RT_TRY(copy_bgr_rows(dst[i], stride_bytes, src[i], stride_bytes, h, w, hipMemcpyDeviceToDevice, q));
    const dim3 grid((unsigned)tiles, n), block(PV_THREADS);
    RT_TRY(p->timer.record(0, q));
    if (g) hipLaunchKernelGGL(privacy_gather, dim3(n), block, 0, q, *g);
    if (blur) hipLaunchKernelGGL(privacy_blur, grid, block, 0, q, a);
    else hipLaunchKernelGGL(privacy_paint, grid, block, 0, q, a);
    if (scratch) hipLaunchKernelGGL(privacy_commit, grid, block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_TRY(p->stage.copy_out(dst ? dst : src, q));
    RT_HIP(hipStreamSynchronize(q));
    p->timer.timed = true;
    return RTMODT_OK;
}

// a device form: the gather buffers for n frames of at most cap boxes, then pv_execute on the source's stream
template <typename F> int pv_apply_view(rtmodt_privacy *p, int src_device, int n, int cap, hipStream_t q, uint8_t *const *frames, int h, int w,
                                        int stride_bytes, int mem_kind, F fill) {
    RT_CHECK(src_device == p->device, RTMODT_E_INVALID, "privacy masker on device %d, its source on device %d", p->device, src_device);
    RT_CHECK(cap >= 1 && cap <= p->cfg.max_regions, RTMODT_E_CAPACITY, "the source holds up to %d boxes per frame > max_regions %d", cap,
             p->cfg.max_regions);
    RT_TRY(pv_check_frames(frames, n, h, w, stride_bytes, mem_kind));
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(p->device));
    RT_TRY(dev_grow(&p->d_gather, &p->gather_bytes, (size_t)n * cap * sizeof(PvRect)));
    RT_TRY(dev_grow(&p->d_gn, &p->gn_bytes, (size_t)n * sizeof(int32_t)));
    GatherArgs g{};
    g.rc = pv_region_cfg(p->cfg, p->cfg.classes ? p->d_classes : nullptr);
    g.h = h; g.w = w; g.cap = cap; g.out = p->d_gather; g.n_out = p->d_gn;
    fill(g);
    return pv_execute(p, frames, nullptr, n, h, w, stride_bytes, mem_kind, q, nullptr, &g);
}

template <typename T> int pv_apply_tracker(rtmodt_privacy *p, T *trk, int report_tsu, uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind) {
    RT_CHECK(p && trk, RTMODT_E_INVALID, "null argument");
    TrackSrc src;
    TrackViewBase v;
    RT_TRY(track_src(trk, report_tsu, &src, &v));
    return pv_apply_view(p, v.device, v.n_streams, v.max_tracks, v.stream, frames, h, w, stride_bytes, mem_kind, [&](GatherArgs &g) { g.trk = src; });
}

}  // namespace

extern "C" {

void rtmodt_privacy_default_cfg(rtmodt_privacy_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_privacy_cfg{};
    cfg->mode = RTMODT_PRIVACY_PIXELATE;
    cfg->cell = 16; cfg->radius = 8; cfg->passes = 2;
    cfg->region = RTMODT_PRIVACY_REGION_BOX; cfg->head_pm = 300; cfg->expand_px = 0;
    cfg->classes = nullptr; cfg->n_classes = 0;
    cfg->max_regions = PV_MAX_REGIONS; cfg->device = 0;
}

void rtmodt_privacy_destroy(rtmodt_privacy *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->ppool); p->cmd.release(); p->stage.release(); hipFree(p->d_scratch); hipFree(p->d_mask);
        hipFree(p->d_gather); hipFree(p->d_gn); hipFree(p->d_classes);
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_privacy_create(const rtmodt_privacy_cfg *cfg, rtmodt_privacy **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(pv_check_cfg(cfg));
    RT_CHECK(cfg->max_regions >= 1 && cfg->max_regions <= PV_MAX_REGIONS, RTMODT_E_INVALID, "max_regions %d outside 1..%d", cfg->max_regions,
             PV_MAX_REGIONS);
    rtmodt_privacy *p = new rtmodt_privacy();
    p->device = cfg->device;
    p->cfg = *cfg;
    if (cfg->classes) {
        p->classes.assign(cfg->classes, cfg->classes + cfg->n_classes);
        p->classes.push_back(0);                            // (never read: keeps data() non-null for an empty list)
        p->cfg.classes = p->classes.data();
    } else {
        p->cfg.n_classes = 0;
    }
    auto body = [&]() -> int {
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        if (p->cfg.classes) {
            RT_HIP(hipMalloc((void **)&p->d_classes, p->classes.size() * sizeof(int32_t)));
            RT_HIP(hipMemcpy(p->d_classes, p->classes.data(), p->classes.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_privacy_destroy, out);
}

int rtmodt_privacy_set_polygons(rtmodt_privacy *p, const int32_t *const *polygons_xy, const int32_t *n_points, int n) {
    RT_CHECK(p && n >= 0 && (n == 0 || (polygons_xy && n_points)), RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n <= PV_MAX_POLYS, RTMODT_E_CAPACITY, "%d privacy polygons (at most %d)", n, PV_MAX_POLYS);
    PolyTable T;
    RT_TRY(T.build(polygons_xy, n_points, n, PV_MAX_POINTS, "polygon"));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipDeviceSynchronize());                        // a device form may have queued work that reads the table on another stream
    p->pv = PolyView{};
    if (n == 0 || T.pts.empty()) return RTMODT_OK;
    const size_t total = T.layout();
    std::vector<char> hostbuf(total, 0);
    T.write(hostbuf.data());
    RT_TRY(dev_grow(&p->ppool, &p->ppool_cap, total));
    RT_HIP(hipMemcpy(p->ppool, hostbuf.data(), total, hipMemcpyHostToDevice));
    T.view(p->ppool, &p->pv);
    p->pv.Z = n; p->pv.n_pts = (int)T.pts.size(); p->pv.stage = T.stage;
    return RTMODT_OK;
}

int rtmodt_privacy_regions(const rtmodt_privacy_cfg *cfg, const float *xyxy, const int32_t *cls, int n_boxes, int h, int w, int32_t *rects,
                           int cap_rects, int32_t *needed) {
    RT_CHECK(needed, RTMODT_E_INVALID, "null argument");
    RT_TRY(pv_check_cfg(cfg));
    RT_CHECK(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, RTMODT_E_INVALID, "bad frame geometry %dx%d", w, h);
    std::vector<PvRect> v;
    RT_TRY(pv_pack_boxes(pv_region_cfg(*cfg, cfg->classes), xyxy, cls, n_boxes, h, w, 0, v));
    *needed = (int32_t)v.size();
    if (rects && cap_rects >= (int)v.size() && !v.empty()) memcpy(rects, v.data(), v.size() * sizeof(PvRect));
    return RTMODT_OK;
}

int rtmodt_privacy_apply(rtmodt_privacy *p, uint8_t *const *src_frames, uint8_t *const *dst_frames, int n, int h, int w, int stride_bytes,
                         int mem_kind, const float *const *xyxy, const int32_t *const *cls, const int32_t *n_boxes) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    RT_TRY(pv_check_frames(src_frames, n, h, w, stride_bytes, mem_kind));
    RT_CHECK(n == 0 || (xyxy && n_boxes), RTMODT_E_INVALID, "null box lists");
    const size_t span = (size_t)(h - 1) * stride_bytes + (size_t)3 * w;
    if (dst_frames)
        for (int i = 0; i < n; ++i) {
            RT_CHECK(dst_frames[i], RTMODT_E_INVALID, "dst frame %d is null", i);
            const uintptr_t s = (uintptr_t)src_frames[i], d = (uintptr_t)dst_frames[i];
            RT_CHECK(s == d || s + span <= d || d + span <= s, RTMODT_E_INVALID, "dst frame %d overlaps its src without being it", i);
        }
    const PvRegionCfg rc = pv_region_cfg(p->cfg, p->cfg.classes);
    std::vector<std::vector<PvRect>> rects(n);
    for (int i = 0; i < n; ++i) {
        RT_TRY(pv_pack_boxes(rc, xyxy[i], cls ? cls[i] : nullptr, n_boxes[i], h, w, i, rects[i]));
        RT_CHECK(rects[i].size() <= (size_t)p->cfg.max_regions, RTMODT_E_CAPACITY, "frame %d: %zu regions (at most %d)", i, rects[i].size(),
                 p->cfg.max_regions);
    }
    return pv_execute(p, src_frames, dst_frames, n, h, w, stride_bytes, mem_kind, p->stream, &rects, nullptr);
}

int rtmodt_privacy_apply_tracker(rtmodt_privacy *p, rtmodt_tracker *trk, uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind,
                                 int report_tsu) {
    return pv_apply_tracker(p, trk, report_tsu, frames, h, w, stride_bytes, mem_kind);
}

int rtmodt_privacy_apply_deepsort(rtmodt_privacy *p, rtmodt_deepsort *ds, uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind,
                                  int report_tsu) {
    return pv_apply_tracker(p, ds, report_tsu, frames, h, w, stride_bytes, mem_kind);
}

int rtmodt_privacy_apply_ocsort(rtmodt_privacy *p, rtmodt_ocsort *oc, uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind) {
    return pv_apply_tracker(p, oc, 0, frames, h, w, stride_bytes, mem_kind);
}

int rtmodt_privacy_apply_botsort(rtmodt_privacy *p, rtmodt_botsort *bot, uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind) {
    return pv_apply_tracker(p, bot, 0, frames, h, w, stride_bytes, mem_kind);
}

int rtmodt_privacy_apply_detector(rtmodt_privacy *p, rtmodt_detector *det, uint8_t *const *frames, int n, int h, int w, int stride_bytes,
                                  int mem_kind) {
    RT_CHECK(p && det, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(detector_outputs(det, &o));
    RT_CHECK(n >= 0 && n <= o.count, RTMODT_E_INVALID, "%d frames, the detector's newest batch has %d", n, o.count);
    return pv_apply_view(p, o.device, n, o.stride, o.stream, frames, h, w, stride_bytes, mem_kind,
                         [&](GatherArgs &g) { g.det_box = o.box; g.det_cls = o.cls; g.det_n = o.n; g.det_stride = o.stride; });
}

int rtmodt_privacy_last_ms(rtmodt_privacy *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no apply call has launched yet");
}

}  // extern "C"
