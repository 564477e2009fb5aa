// render.hip -- the reference's FrameRenderer.render (src/visualization/renderer.py) on the GPU: boxes, labels, trails, zone
// tint + names and the HUD drawn IN PLACE into BGR24 frames, ONE launch per batch.
//
// Paint rules (tests/render_ref.py restates them in NumPy; cv2 is not available, so parity with cv2 itself is unpinned and
// every departure below is deliberate).  Pixel centres are integer coordinates.  A frame is painted in this order:
//   1. zone tint (show_zones, zones set): overlay = the frame; every pixel inside or on a zone polygon -- inside_or_on of
//      polygon.h, the zone engine's own test, NOT cv2.fillPoly's scan conversion -- becomes BGR (0, 0, 180);
//   2. zone names: white, font 0, baseline-left at (int(m10/m00) - 30, int(m01/m00)) of the polygon's contour moments
//      (float64, computed here on the host), drawn into the FRAME (not the overlay); nothing when m00 == 0;
//   3. blend: out = sat_u8(rint(0.25f * overlay + 0.75f * frame)) per channel in float32, ties to even.  Outside every
//      polygon and every name glyph overlay == frame and the arithmetic is exact: those pixels come back unchanged;
//   4. per track, in list order (a later track overwrites an earlier one), colour = palette[track_id mod 20]:
//      box (show_boxes): the 4 edges with the thickness-2 stroke = every pixel within Euclidean distance 1 of the segment
//        (exact int64 test; corners come out rounded, as cv2's do); corners int(...) of the float32 box;
//      label (show_ids): the filled rectangle (x1, y1 - th - 6)..(x1 + tw, y1) inclusive, then the label text in black
//        with its baseline-left at (x1, y1 - 4); tw = font 0's advance x length, th = its ascent;
//      trail (show_trails, len(trail) > 1): the last trail_length points as an open polyline with the same stroke (one
//        point left: a zero-length segment, i.e. a dot);
//   5. HUD (show_fps): "FPS: {fps:.1f} | Latency: {latency_ms:.1f}ms" in green at (10, 30), font 1.
// Text is a 1-bit bitmap font (font_atlas.h), not Hershey strokes: glyph shapes and metrics differ from cv2.putText.
// Coordinates are clamped to +-2^20 before use (a pathological coordinate far off-frame bends a segment's slope there).
//
// Kernel: the grid is (64 x 16 pixel tiles) x frames, 256 threads; thread t owns the 4-pixel group (t % 16, t / 16) of the
// tile.  The frame's draw list is a list of ITEMS (one per track, one for the HUD), each a bounding box and a range of
// PRIMITIVES (segment, filled rectangle, text run).  A workgroup culls the items against its tile 256 at a time with an
// order-preserving ballot compaction into LDS, then flattens the surviving items' primitives and culls those the same way;
// paint order is therefore the list order, and every pixel is owned by exactly one thread: no atomics, no dependence on
// scheduling.  A tile that meets neither an item nor the zones returns before it reads a byte of the frame; the others
// read their pixels once (dwordx3 per group on a 4-byte-aligned row, bytes at a ragged right edge or an odd stride),
// evaluate everything in registers and write back only groups that changed.  Capacity does not depend on the list: the
// culled sets pass through LDS in chunks; only the zones (32 polygons, 2048 points) are staged in LDS whole.
//
// Command buffer (host -> device in one copy per call; rtmodt_render_pack writes it):
//   CmdHeader | FrameRec[n] | ItemRec[n_items] | Prim[n_prims] | chars[n_chars]      (sections 16-byte aligned)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "font_atlas.h"
#include "frame_stage.h"
#include "handle_host.h"
#include "polygon.h"

namespace rtmodt {

constexpr int RD_THREADS = 256, RD_WAVES = RD_THREADS / 64, RD_TW = 64, RD_TH = 16;
constexpr int RD_MAX_ZONES = 32, RD_MAX_POINTS = 2048, RD_MAX_TEXT = 255, RD_MAX_TRACKS = 65536, RD_MAX_TRAIL = 1024;
constexpr int RD_COORD_MAX = 1 << 20;
constexpr int PRIM_SEG = 0, PRIM_RECT = 1, PRIM_TEXT = 2;
constexpr uint32_t CMD_MAGIC = 0x31524452u;        // "RDR1"

struct CmdHeader { uint32_t magic; int32_t n_frames, n_items, n_prims, n_chars, h, w, pad; int64_t off_frames, off_items, off_prims, off_chars; };
struct FrameRec { uint64_t ptr; int32_t item0, n_items, flags, pad[3]; };                   // flags bit 0: draw the zones
struct ItemRec { int32_t x0, y0, x1, y1, begin, count, pad[2]; };                             // bbox inclusive; prims [begin, begin + count)
// w[0] = type | font << 8, w[1] = colour (B | G << 8 | R << 16); SEG: a.x, a.y, b.x, b.y; RECT: x0, y0, x1, y1 (inclusive);
// TEXT: origin x, baseline y, char offset, length
struct Prim { int32_t w[8]; };
static_assert(sizeof(CmdHeader) == 64 && sizeof(FrameRec) == 32 && sizeof(ItemRec) == 32 && sizeof(Prim) == 32, "layout");

struct FontMetrics { int adv, asc, desc; };
static const FontMetrics kFont[2] = {{ATLAS_FONT0_ADVANCE, ATLAS_FONT0_ASCENT, ATLAS_FONT0_DESCENT},
                                     {ATLAS_FONT1_ADVANCE, ATLAS_FONT1_ASCENT, ATLAS_FONT1_DESCENT}};
__constant__ uint32_t d_font0[] = ATLAS_FONT0_ROWS;
__constant__ uint32_t d_font1[] = ATLAS_FONT1_ROWS;

// the reference's palette (renderer.py:19-25), BGR
static const uint8_t kPalette[20][3] = {{0, 255, 127}, {255, 144, 30}, {0, 215, 255}, {180, 105, 255}, {71, 99, 255}, {50, 205, 50},
                                        {0, 165, 255}, {205, 92, 92}, {238, 130, 238}, {0, 255, 255}, {30, 105, 210}, {128, 0, 0},
                                        {0, 128, 128}, {128, 128, 0}, {255, 0, 255}, {0, 0, 255}, {255, 255, 0}, {0, 128, 0},
                                        {128, 0, 128}, {255, 165, 0}};

struct ZoneView {                       // device pointers into the renderer's zone table
    const int2 *pts; const int32_t *off; const int4 *bbox; const Prim *names; const uint8_t *chars;
    int Z, n_pts;
    int4 stage;                          // union of every polygon's and name's box
};

struct RenderArgs {
    const FrameRec *frames; const ItemRec *items; const Prim *prims; const uint8_t *chars;
    int h, w, tiles_x;
    long long stride;
    ZoneView zv;
};

__host__ __device__ inline int4 prim_bbox(const Prim &p) {
    const int type = p.w[0] & 0xff;
    if (type == PRIM_SEG)
        return make_int4(min(p.w[2], p.w[4]) - 1, min(p.w[3], p.w[5]) - 1, max(p.w[2], p.w[4]) + 1, max(p.w[3], p.w[5]) + 1);
    if (type == PRIM_RECT) return make_int4(p.w[2], p.w[3], p.w[4], p.w[5]);
    const int f = (p.w[0] >> 8) & 1;
    const int adv = f ? ATLAS_FONT1_ADVANCE : ATLAS_FONT0_ADVANCE, asc = f ? ATLAS_FONT1_ASCENT : ATLAS_FONT0_ASCENT;
    const int desc = f ? ATLAS_FONT1_DESCENT : ATLAS_FONT0_DESCENT;
    return make_int4(p.w[2], p.w[3] - asc, p.w[2] + p.w[5] * adv - 1, p.w[3] + desc - 1);   // empty (x1 < x0) for length 0
}

// a 4-pixel BGR24 group: three dwords, 4-byte aligned (the frame pointer and its rows)
typedef uint32_t u32x3 __attribute__((ext_vector_type(3), aligned(4)));
#define GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ bool overlaps(int4 b, int x0, int y0, int x1, int y1) {
    return b.x <= x1 && b.z >= x0 && b.y <= y1 && b.w >= y0 && b.x <= b.z && b.y <= b.w;
}

// every pixel centre within Euclidean distance 1 of segment a-b, exactly
__device__ __forceinline__ bool on_stroke(int ax, int ay, int bx, int by, int x, int y) {
    const long long dx = bx - ax, dy = by - ay, px = x - ax, py = y - ay;
    const long long L = dx * dx + dy * dy, t = px * dx + py * dy;
    if (L == 0 || t <= 0) return px * px + py * py <= 1;
    if (t >= L) {
        const long long qx = x - bx, qy = y - by;
        return qx * qx + qy * qy <= 1;
    }
    long long c = px * dy - py * dx;
    if (c < 0) c = -c;
    return c <= 0x7fffffffll && c * c <= L;                 // distance^2 = c^2 / L
}

__device__ __forceinline__ bool glyph_ink(const Prim &p, const uint8_t *chars, int x, int y) {
    const int f = (p.w[0] >> 8) & 1;
    const int adv = f ? ATLAS_FONT1_ADVANCE : ATLAS_FONT0_ADVANCE, asc = f ? ATLAS_FONT1_ASCENT : ATLAS_FONT0_ASCENT;
    const int H = asc + (f ? ATLAS_FONT1_DESCENT : ATLAS_FONT0_DESCENT);
    const int dx = x - p.w[2], r = y - (p.w[3] - asc);
    if (dx < 0 || dx >= p.w[5] * adv || r < 0 || r >= H) return false;
    const int k = dx / adv, col = dx - k * adv;
    int c = chars[p.w[4] + k];
    if (c < ATLAS_FONT_FIRST || c >= ATLAS_FONT_FIRST + ATLAS_FONT_COUNT) c = '?';
    const int idx = (c - ATLAS_FONT_FIRST) * H + r;
    const uint32_t row = f ? d_font1[idx] : d_font0[idx];
    return (row >> col) & 1u;
}

__device__ __forceinline__ bool covers(const Prim &p, const uint8_t *chars, int x, int y) {
    const int type = p.w[0] & 0xff;
    if (type == PRIM_SEG) return on_stroke(p.w[2], p.w[3], p.w[4], p.w[5], x, y);
    if (type == PRIM_RECT) return x >= p.w[2] && x <= p.w[4] && y >= p.w[3] && y <= p.w[5];
    return glyph_ink(p, chars, x, y);
}

#pragma clang fp contract(off)
__device__ __forceinline__ uint32_t blend_px(uint32_t ov, uint32_t fr) {
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float o = 0.25f * (float)((ov >> (8 * c)) & 0xffu) + 0.75f * (float)((fr >> (8 * c)) & 0xffu);
        const float r = fminf(fmaxf(__builtin_rintf(o), 0.0f), 255.0f);
        out |= (uint32_t)r << (8 * c);
    }
    return out;
}

// position of this thread's flag among the set flags of the workgroup, in thread order; two barriers
__device__ __forceinline__ int wg_compact(bool f, int *s_wcnt, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < RD_WAVES; ++w) {
        const int c = s_wcnt[w];
        if (w < wave) off += c;
        tot += c;
    }
    __syncthreads();
    total = tot;
    return off + below;
}

// exclusive prefix sum of v over the workgroup; two barriers
__device__ __forceinline__ int wg_scan(int v, int *s_wcnt, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wcnt[wave] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < RD_WAVES; ++w) {
        const int s = s_wcnt[w];
        if (w < wave) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + incl - v;
}

__global__ __launch_bounds__(RD_THREADS) void render_tiles(RenderArgs a) {
    __shared__ __attribute__((aligned(16))) Prim s_prim[RD_THREADS];
    __shared__ __attribute__((aligned(16))) int2 s_pts[RD_MAX_POINTS];
    __shared__ int s_item[RD_THREADS];
    __shared__ int s_pre[RD_THREADS + 1];
    __shared__ int s_wcnt[RD_WAVES];

    const int tid = threadIdx.x;
    const FrameRec fr = a.frames[blockIdx.y];
    const int tx0 = (blockIdx.x % a.tiles_x) * RD_TW, ty0 = (blockIdx.x / a.tiles_x) * RD_TH;
    const int tx1 = min(tx0 + RD_TW - 1, a.w - 1), ty1 = min(ty0 + RD_TH - 1, a.h - 1);
    const int x0 = tx0 + 4 * (tid & 15), y = ty0 + (tid >> 4);
    const bool active = y < a.h && x0 < a.w;
    const int npx = active ? min(4, a.w - x0) : 0;
    uint8_t *row = (uint8_t *)fr.ptr + (long long)y * a.stride + 3LL * x0;
    const bool wide = npx == 4 && ((uintptr_t)row & 3u) == 0;
    uint32_t px[4] = {0u, 0u, 0u, 0u}, orig[4];
    bool loaded = false;                                   // uniform over the workgroup
    auto load = [&]() {
        if (wide) {
            const u32x3 d = *(const GLOBAL u32x3 *)row;          // one dwordx3
            const uint32_t d0 = d.x, d1 = d.y, d2 = d.z;
            px[0] = d0 & 0xffffffu;
            px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
            px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
            px[3] = d2 >> 8;
        } else {
            for (int i = 0; i < npx; ++i) px[i] = row[3 * i] | (uint32_t)row[3 * i + 1] << 8 | (uint32_t)row[3 * i + 2] << 16;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) orig[i] = px[i];
        loaded = true;
    };

    // ---- 1-3: zone tint, names, blend ----
    const ZoneView &zv = a.zv;
    if ((fr.flags & 1) && zv.Z > 0 && overlaps(zv.stage, tx0, ty0, tx1, ty1)) {
        for (int i = tid; i < zv.n_pts; i += RD_THREADS) s_pts[i] = zv.pts[i];
        __syncthreads();
        load();
        for (int i = 0; i < npx; ++i) {
            const int x = x0 + i;
            bool inside = false, glyph = false;
            for (int z = 0; z < zv.Z && !inside; ++z) {
                const int4 b = zv.bbox[z];
                if (x >= b.x && x <= b.z && y >= b.y && y <= b.w) {
                    const int p0 = zv.off[z];
                    inside = inside_or_on(s_pts + p0, zv.off[z + 1] - p0, x, y);
                }
            }
            for (int z = 0; z < zv.Z && !glyph; ++z) glyph = glyph_ink(zv.names[z], zv.chars, x, y);
            if (inside || glyph) px[i] = blend_px(inside ? 0xb40000u : px[i], glyph ? 0xffffffu : px[i]);
        }
    }

    // ---- 4-5: the items (tracks, then the HUD) in list order ----
    for (int ib = 0; ib < fr.n_items; ib += RD_THREADS) {
        const int i = ib + tid;
        bool f = false;
        if (i < fr.n_items) {
            const ItemRec it = a.items[fr.item0 + i];
            f = overlaps(make_int4(it.x0, it.y0, it.x1, it.y1), tx0, ty0, tx1, ty1);
        }
        int m;
        const int pos = wg_compact(f, s_wcnt, m);
        if (f) s_item[pos] = fr.item0 + i;
        __syncthreads();
        if (m == 0) continue;
        if (!loaded) load();
        int T;
        const int ex = wg_scan(tid < m ? a.items[s_item[tid]].count : 0, s_wcnt, T);
        if (tid < m) s_pre[tid] = ex;
        if (tid == 0) s_pre[m] = T;
        __syncthreads();
        for (int jb = 0; jb < T; jb += RD_THREADS) {
            const int j = jb + tid;
            bool g = false;
            Prim p;
            if (j < T) {
                int lo = 0, hi = m;                                    // last k with s_pre[k] <= j
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_pre[mid] <= j) lo = mid; else hi = mid;
                }
                p = a.prims[a.items[s_item[lo]].begin + (j - s_pre[lo])];
                g = overlaps(prim_bbox(p), tx0, ty0, tx1, ty1);
            }
            int k;
            const int q = wg_compact(g, s_wcnt, k);
            if (g) s_prim[q] = p;
            __syncthreads();
            for (int e = 0; e < k; ++e) {
                const Prim pe = s_prim[e];
                const uint32_t colour = (uint32_t)pe.w[1];
                for (int u = 0; u < npx; ++u)
                    if (covers(pe, a.chars, x0 + u, y)) px[u] = colour;
            }
            __syncthreads();
        }
    }
    if (!loaded) return;

    bool changed = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) changed |= px[i] != orig[i];
    if (!changed) return;
    if (wide) {
        *(GLOBAL u32x3 *)row = u32x3{px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
    } else {
        for (int i = 0; i < npx; ++i)
            if (px[i] != orig[i]) {
                row[3 * i] = (uint8_t)px[i];
                row[3 * i + 1] = (uint8_t)(px[i] >> 8);
                row[3 * i + 2] = (uint8_t)(px[i] >> 16);
            }
    }
}

// ======================================================================================
// host side: configuration, packing
// ======================================================================================
struct RenderCfg {
    int boxes = 1, ids = 1, trails = 1, zones = 1, fps = 1, trail_length = 30;
    std::vector<uint32_t> palette;      // packed B | G << 8 | R << 16
};

static int parse_cfg(const rtmodt_render_cfg *c, RenderCfg &o) {
    RT_CHECK(c, RTMODT_E_INVALID, "null render config");
    RT_CHECK(c->trail_length >= 1 && c->trail_length <= RD_MAX_TRAIL, RTMODT_E_INVALID, "trail_length %d outside 1..%d", c->trail_length, RD_MAX_TRAIL);
    o.boxes = c->show_boxes != 0; o.ids = c->show_ids != 0; o.trails = c->show_trails != 0; o.zones = c->show_zones != 0; o.fps = c->show_fps != 0;
    o.trail_length = c->trail_length;
    o.palette.clear();
    if (c->palette_bgr) {
        RT_CHECK(c->n_palette >= 1 && c->n_palette <= 256, RTMODT_E_INVALID, "palette of %d colours (1..256)", c->n_palette);
        for (int i = 0; i < c->n_palette; ++i) {
            const uint8_t *p = c->palette_bgr + 3 * i;
            o.palette.push_back(p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
        }
    } else {
        for (auto &p : kPalette) o.palette.push_back(p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
    }
    return RTMODT_OK;
}

static inline int clamp_coord(long long v) { return (int)std::min<long long>(std::max<long long>(v, -RD_COORD_MAX), RD_COORD_MAX); }
static inline int coord_of(float v) { return (int)std::trunc(std::min(std::max(v, (float)-RD_COORD_MAX), (float)RD_COORD_MAX)); }

// text bytes -> chars (outside 32..126: '?'); RTMODT_E_CAPACITY beyond RD_MAX_TEXT
static int put_text(const char *s, std::vector<uint8_t> &chars, int &off, int &len, const char *what) {
    const size_t n = s ? strlen(s) : 0;
    RT_CHECK(n <= (size_t)RD_MAX_TEXT, RTMODT_E_CAPACITY, "%s of %zu characters (at most %d)", what, n, RD_MAX_TEXT);
    off = (int)chars.size();
    len = (int)n;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = (uint8_t)s[i];
        chars.push_back(c >= 32 && c <= 126 ? c : (uint8_t)'?');
    }
    return RTMODT_OK;
}

static Prim make_prim(int type, int font, uint32_t colour, int a, int b, int c, int d, int e = 0, int f = 0) {
    Prim p{};
    p.w[0] = type | font << 8; p.w[1] = (int32_t)colour;
    p.w[2] = a; p.w[3] = b; p.w[4] = c; p.w[5] = d; p.w[6] = e; p.w[7] = f;
    return p;
}
static Prim make_text(int font, uint32_t colour, int ox, int oy, int char_off, int len) {
    return make_prim(PRIM_TEXT, font, colour, ox, oy, char_off, len);
}

// "%.1f" as Python's format() writes it (a NaN has no sign there)
static void fmt1(char *buf, size_t n, double v) {
    if (std::isnan(v)) snprintf(buf, n, "nan");
    else snprintf(buf, n, "%.1f", v);
}

struct Packed { std::vector<FrameRec> frames; std::vector<ItemRec> items; std::vector<Prim> prims; std::vector<uint8_t> chars; };

static int pack_lists(const RenderCfg &cfg, const rtmodt_render_list *lists, int n, int draw_zones, double fps, double latency_ms, Packed &P) {
    RT_CHECK(n >= 0 && (n == 0 || lists), RTMODT_E_INVALID, "bad draw lists");
    const uint32_t black = 0u, green = 0x00ff00u;
    const int npal = (int)cfg.palette.size();
    char hud[1100];
    {
        char f1[512], f2[512];
        fmt1(f1, sizeof(f1), fps); fmt1(f2, sizeof(f2), latency_ms);
        snprintf(hud, sizeof(hud), "FPS: %s | Latency: %sms", f1, f2);
    }
    P.frames.assign(n, FrameRec{});
    for (int fi = 0; fi < n; ++fi) {
        const rtmodt_render_list &L = lists[fi];
        RT_CHECK(L.n_tracks >= 0 && (L.n_tracks == 0 || L.tracks), RTMODT_E_INVALID, "frame %d: bad track list", fi);
        RT_CHECK(L.n_tracks <= RD_MAX_TRACKS, RTMODT_E_CAPACITY, "frame %d: %d tracks (at most %d)", fi, L.n_tracks, RD_MAX_TRACKS);
        FrameRec &F = P.frames[fi];
        F.item0 = (int)P.items.size();
        F.flags = (draw_zones && cfg.zones) ? 1 : 0;
        auto add_item = [&](size_t p0) {
            if (P.prims.size() == p0) return;
            ItemRec it{};
            it.x0 = it.y0 = INT32_MAX; it.x1 = it.y1 = INT32_MIN;
            for (size_t q = p0; q < P.prims.size(); ++q) {
                const int4 b = prim_bbox(P.prims[q]);
                if (b.x > b.z || b.y > b.w) continue;
                it.x0 = std::min(it.x0, b.x); it.y0 = std::min(it.y0, b.y); it.x1 = std::max(it.x1, b.z); it.y1 = std::max(it.y1, b.w);
            }
            it.begin = (int)p0; it.count = (int)(P.prims.size() - p0);
            P.items.push_back(it);
        };
        for (int t = 0; t < L.n_tracks; ++t) {
            const rtmodt_render_track &T = L.tracks[t];
            for (int k = 0; k < 4; ++k)
                RT_CHECK(T.xyxy[k] == T.xyxy[k], RTMODT_E_INVALID, "frame %d track %d: NaN box", fi, t);
            RT_CHECK(T.n_trail >= 0 && (T.n_trail == 0 || T.trail_xy), RTMODT_E_INVALID, "frame %d track %d: bad trail", fi, t);
            const uint32_t colour = cfg.palette[(size_t)(((T.track_id % npal) + npal) % npal)];
            const int x1 = coord_of(T.xyxy[0]), y1 = coord_of(T.xyxy[1]), x2 = coord_of(T.xyxy[2]), y2 = coord_of(T.xyxy[3]);
            const size_t p0 = P.prims.size();
            if (cfg.boxes) {
                P.prims.push_back(make_prim(PRIM_SEG, 0, colour, x1, y1, x2, y1));
                P.prims.push_back(make_prim(PRIM_SEG, 0, colour, x2, y1, x2, y2));
                P.prims.push_back(make_prim(PRIM_SEG, 0, colour, x2, y2, x1, y2));
                P.prims.push_back(make_prim(PRIM_SEG, 0, colour, x1, y2, x1, y1));
            }
            if (cfg.ids) {
                int off, len;
                RT_TRY(put_text(T.label, P.chars, off, len, "label"));
                const int tw = len * kFont[0].adv, th = kFont[0].asc;
                P.prims.push_back(make_prim(PRIM_RECT, 0, colour, x1, y1 - th - 6, x1 + tw, y1));
                if (len) P.prims.push_back(make_text(0, black, x1, y1 - 4, off, len));
            }
            if (cfg.trails && T.n_trail > 1) {
                const int m = std::min(T.n_trail, cfg.trail_length), s = T.n_trail - m;
                auto pt = [&](int i) { return make_int2(clamp_coord(T.trail_xy[2 * (s + i)]), clamp_coord(T.trail_xy[2 * (s + i) + 1])); };
                if (m == 1) {
                    const int2 a = pt(0);
                    P.prims.push_back(make_prim(PRIM_SEG, 0, colour, a.x, a.y, a.x, a.y));
                }
                for (int i = 0; i + 1 < m; ++i) {
                    const int2 a = pt(i), b = pt(i + 1);
                    P.prims.push_back(make_prim(PRIM_SEG, 0, colour, a.x, a.y, b.x, b.y));
                }
            }
            add_item(p0);
        }
        if (cfg.fps) {
            const size_t p0 = P.prims.size();
            int off, len;
            RT_TRY(put_text(hud, P.chars, off, len, "HUD"));
            P.prims.push_back(make_text(1, green, 10, 30, off, len));
            add_item(p0);
        }
        F.n_items = (int)P.items.size() - F.item0;
        RT_CHECK(P.prims.size() < (size_t)INT32_MAX / 2 && P.chars.size() < (size_t)INT32_MAX / 2, RTMODT_E_CAPACITY,
                 "%zu primitives / %zu characters in one call", P.prims.size(), P.chars.size());
    }
    return RTMODT_OK;
}

static size_t cmd_layout(const Packed &P, CmdHeader &H, int h, int w) {
    H = CmdHeader{};
    H.magic = CMD_MAGIC; H.n_frames = (int)P.frames.size(); H.n_items = (int)P.items.size(); H.n_prims = (int)P.prims.size();
    H.n_chars = (int)P.chars.size(); H.h = h; H.w = w;
    size_t off = sizeof(CmdHeader);
    H.off_frames = (int64_t)off; off = align_up(off + P.frames.size() * sizeof(FrameRec), 16);
    H.off_items = (int64_t)off; off = align_up(off + P.items.size() * sizeof(ItemRec), 16);
    H.off_prims = (int64_t)off; off = align_up(off + P.prims.size() * sizeof(Prim), 16);
    H.off_chars = (int64_t)off; off = align_up(off + std::max<size_t>(P.chars.size(), 1), 16);
    return off;
}

static void cmd_write(const Packed &P, const CmdHeader &H, char *out) {
    memcpy(out, &H, sizeof(H));
    if (!P.frames.empty()) memcpy(out + H.off_frames, P.frames.data(), P.frames.size() * sizeof(FrameRec));
    if (!P.items.empty()) memcpy(out + H.off_items, P.items.data(), P.items.size() * sizeof(ItemRec));
    if (!P.prims.empty()) memcpy(out + H.off_prims, P.prims.data(), P.prims.size() * sizeof(Prim));
    if (!P.chars.empty()) memcpy(out + H.off_chars, P.chars.data(), P.chars.size());
}

// float64 contour moments of an int32 polygon (Green's theorem over the closed outline); -> false when m00 == 0
static bool name_anchor(const int32_t *xy, int n, int &ax, int &ay) {
    double a00 = 0, a10 = 0, a01 = 0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + n - 1) % n;
        const double xp = xy[2 * j], yp = xy[2 * j + 1], x = xy[2 * i], y = xy[2 * i + 1];
        const double d = xp * y - x * yp;
        a00 += d; a10 += d * (xp + x); a01 += d * (yp + y);
    }
    if (a00 == 0.0) return false;
    const double m00 = a00 * 0.5, m10 = a10 * (1.0 / 6.0), m01 = a01 * (1.0 / 6.0);   // orientation cancels in the quotients
    ax = clamp_coord((long long)std::trunc(std::min(std::max(m10 / m00, -2.0 * RD_COORD_MAX), 2.0 * RD_COORD_MAX)));
    ay = clamp_coord((long long)std::trunc(std::min(std::max(m01 / m00, -2.0 * RD_COORD_MAX), 2.0 * RD_COORD_MAX)));
    return true;
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_renderer : HandleBase {
    RenderCfg cfg;
    EventTimer<2> timer;
    char *zpool = nullptr;              // zone table (device)
    size_t zpool_cap = 0;
    ZoneView zv{};
    CmdBuf cmd;
    FrameStage stage;                   // host path: frames staged on the device
};

extern "C" {

void rtmodt_renderer_destroy(rtmodt_renderer *r) {
    if (!r) return;
    handle_close(r, [&] {
        hipFree(r->zpool);
        r->cmd.release();
        r->stage.release();
        r->timer.destroy();
    });
    delete r;
}

int rtmodt_renderer_create(int device, const rtmodt_render_cfg *cfg, rtmodt_renderer **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RenderCfg c;
    RT_TRY(parse_cfg(cfg, c));
    rtmodt_renderer *r = new rtmodt_renderer();
    r->device = device;
    r->cfg = c;
    auto body = [&]() -> int {
        RT_TRY(handle_open(r));
        RT_TRY(r->timer.create());
        return RTMODT_OK;
    };
    return handle_created(body(), r, rtmodt_renderer_destroy, out);
}

int rtmodt_renderer_set_zones(rtmodt_renderer *r, const int32_t *const *polygons_xy, const int32_t *n_points, const char *const *names, int n_zones) {
    RT_CHECK(r && n_zones >= 0 && (n_zones == 0 || (polygons_xy && n_points)), RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n_zones <= RD_MAX_ZONES, RTMODT_E_CAPACITY, "%d zones (at most %d)", n_zones, RD_MAX_ZONES);
    PolyTable T;
    std::vector<Prim> nm;
    std::vector<uint8_t> chars;
    for (int z = 0; z < n_zones; ++z) {
        const int np = n_points[z];
        RT_TRY(T.add(polygons_xy[z], np, z, RD_MAX_POINTS, "zone"));
        int ax, ay, co = 0, len = 0;
        if (np > 0 && name_anchor(polygons_xy[z], np, ax, ay)) {
            RT_TRY(put_text(names ? names[z] : nullptr, chars, co, len, "zone name"));
        }
        const Prim p = make_text(0, 0xffffffu, len ? ax - 30 : 0, len ? ay : 0, co, len);
        nm.push_back(p);
        T.enclose(prim_bbox(p));
    }
    RT_HIP(hipSetDevice(r->device));
    RT_HIP(hipStreamSynchronize(r->stream));
    r->zv = ZoneView{};
    if (n_zones == 0) return RTMODT_OK;
    // the zone names go behind the polygon table: names | chars
    const size_t o_nm = T.layout(), o_ch = align_up(o_nm + nm.size() * sizeof(Prim), 16), total = align_up(o_ch + std::max<size_t>(chars.size(), 1), 16);
    std::vector<char> host(total, 0);
    T.write(host.data());
    memcpy(host.data() + o_nm, nm.data(), nm.size() * sizeof(Prim));
    if (!chars.empty()) memcpy(host.data() + o_ch, chars.data(), chars.size());
    RT_TRY(dev_grow(&r->zpool, &r->zpool_cap, total));
    RT_HIP(hipMemcpy(r->zpool, host.data(), total, hipMemcpyHostToDevice));
    ZoneView &v = r->zv;
    T.view(r->zpool, &v);
    v.names = (const Prim *)(r->zpool + o_nm); v.chars = (const uint8_t *)(r->zpool + o_ch);
    v.Z = n_zones; v.n_pts = (int)T.pts.size(); v.stage = T.stage;
    return RTMODT_OK;
}

int rtmodt_render_pack(const rtmodt_render_cfg *cfg, const rtmodt_render_list *lists, int n, int h, int w, int draw_zones, double fps,
                       double latency_ms, void *out, size_t out_bytes, size_t *needed) {
    RT_CHECK(needed, RTMODT_E_INVALID, "null argument");
    RenderCfg c;
    RT_TRY(parse_cfg(cfg, c));
    Packed P;
    RT_TRY(pack_lists(c, lists, n, draw_zones, fps, latency_ms, P));
    CmdHeader H;
    *needed = cmd_layout(P, H, h, w);
    if (out && out_bytes >= *needed) {
        memset(out, 0, *needed);
        cmd_write(P, H, (char *)out);
    }
    return RTMODT_OK;
}

int rtmodt_render_batch(rtmodt_renderer *r, uint8_t *const *frames, int n, int h, int w, int stride_bytes, int mem_kind,
                        const rtmodt_render_list *lists, int draw_zones, double fps, double latency_ms) {
    RT_CHECK(r && n >= 0 && (n == 0 || frames), RTMODT_E_INVALID, "bad argument");
    RT_TRY(check_frames(frames, n, h, w, stride_bytes, mem_kind, kPaintFrames));
    Packed P;
    RT_TRY(pack_lists(r->cfg, lists, n, draw_zones, fps, latency_ms, P));
    r->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(r->device));
    // host frames: staged tightly on the device (16-byte aligned rows), drawn there, copied back row by row
    RT_TRY(r->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_TIGHT16));
    for (int i = 0; i < n; ++i) P.frames[i].ptr = (uint64_t)(uintptr_t)r->stage.at(frames, i);
    CmdHeader H;
    const size_t bytes = cmd_layout(P, H, h, w);
    RT_TRY(r->cmd.reserve(bytes));
    RT_HIP(hipStreamSynchronize(r->stream));               // the pinned buffer may still feed the previous copy
    cmd_write(P, H, r->cmd.h);
    RT_HIP(hipMemcpyAsync(r->cmd.d, r->cmd.h, bytes, hipMemcpyHostToDevice, r->stream));
    RT_TRY(r->stage.copy_in(frames, r->stream));
    RenderArgs a{};
    a.frames = (const FrameRec *)(r->cmd.d + H.off_frames); a.items = (const ItemRec *)(r->cmd.d + H.off_items);
    a.prims = (const Prim *)(r->cmd.d + H.off_prims); a.chars = (const uint8_t *)(r->cmd.d + H.off_chars);
    a.h = h; a.w = w; a.tiles_x = cdiv(w, RD_TW); a.stride = (long long)r->stage.pitch;
    a.zv = r->zv;
    const long long tiles = (long long)a.tiles_x * cdiv(h, RD_TH);
    RT_CHECK(tiles <= INT32_MAX, RTMODT_E_INVALID, "frame too large");
    RT_TRY(r->timer.record(0, r->stream));
    hipLaunchKernelGGL(render_tiles, dim3((unsigned)tiles, n), dim3(RD_THREADS), 0, r->stream, a);
    RT_HIP(hipGetLastError());
    RT_TRY(r->timer.record(1, r->stream));
    RT_TRY(r->stage.copy_out(frames, r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));
    r->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_renderer_last_ms(rtmodt_renderer *r, float *kernel_ms) {
    RT_CHECK(r && kernel_ms, RTMODT_E_INVALID, "null argument");
    return r->timer.elapsed(r->device, 0, 1, kernel_ms, "no render_batch has run a kernel yet");
}

}  // extern "C"
