// compose.hip -- the compositor: video-wall mosaics, sub-streams and zoom insets out of BGR24 sources, BGR24 or 4:2:0 (NV12 / I420)
// out.  The reference has no counterpart (its web page shows one image, tools/run_pipeline.py writes the full frame); PARITY UNPINNED
// against cv2.resize / cv2.cvtColor.  csrc/compose_rule.h states every rule; tests/compose_ref.py restates it: every output byte is equal.
//
// LAYOUT (rtmodt_compose_set_layout, host): every cell is planned with compose_rule.h, the enlarging axes get letterbox.h's tables, and
// every output is cut into tiles of CP_TW x CP_TH pixels.  A tile's entry of the WORK LIST names the cells whose rectangle meets it, in
// painting order, without those a single later cell hides inside the tile.  Cells, outputs, tiles, list and tables live in one device
// pool; a run uploads only {source pointer, pitch} and {plane pointers, pitches}, in one copy.
//
// Kernel compose_tiles (256 threads = one tile, ONE launch per run whatever the outputs and cells; no atomics, no floats):
//   a thread owns one pixel.  It finds its top-most cell by walking the tile's list backwards; the workgroup then walks the list
//   forwards and skips every cell that is top-most for none of its pixels (a covered cell costs nothing).  For a cell that is
//   seen, the source FOOTPRINT of (tile x inner picture) is staged in LDS: per source row the 16-byte blocks that lie wholly inside
//   the row's bytes are moved as one 16-byte load each (a block is aligned in memory AND in LDS, whatever base and pitch are), the
//   ragged first and last block byte by byte -- the fallback is per row.  Each thread then forms, per source row of its span, the
//   horizontal weighted sum (32-bit) once and adds it with the row's weight to a 64-bit accumulator: one division at the end (a
//   shift when Tx Ty is a power of two, a 32-bit division when the numerator cannot pass 2^32, else 64-bit: all three exact).
//   A source byte is therefore fetched from memory once per cell, but for the rows and columns two neighbouring tiles share.
//   A footprint that does not fit the CP_STAGE bytes of LDS (1080p -> 120 x 68) is walked in BANDS of rows, and a row longer than
//   CP_CHUNK pixels in chunks; the accumulators carry over, the sum is the same sum.
//   The tile is assembled in LDS and leaves as 16-byte stores where the destination row allows, byte stores at its ragged ends;
//   nothing outside a row's 3w (plane: w) bytes is written.  4:2:0: Y per pixel, U and V from the 2 x 2 block's mean, from the same LDS tile.
#include <algorithm>
#include <cstring>
#include <vector>

#include "frame_stage.h"
#include "handle_host.h"

#define PV_HD __host__ __device__
#include "compose_rule.h"

namespace rtmodt {

constexpr int CP_TW = 32, CP_TH = 8, CP_THREADS = CP_TW * CP_TH;
constexpr int CP_STAGE = 32768;                 // bytes of LDS the footprint is staged in
constexpr int CP_CHUNK = 10240;                 // source pixels of one row staged at a time: 3 * CP_CHUNK + 30 <= CP_STAGE
constexpr int CP_OSTR = 128, CP_PSTR = 64;      // LDS row pitch of the BGR tile (15 + 3 * CP_TW <= 128) and of a plane tile (15 + CP_TW <= 64)
constexpr long long CP_MAX_TILES = 1ll << 25;
static_assert(CP_THREADS == 256 && CP_TW % 2 == 0 && CP_TH % 2 == 0, "tile");
static_assert((15 + 3 * CP_CHUNK + 15) / 16 * 16 <= CP_STAGE, "a chunk row fits the staging buffer");

struct CpDevCell {
    int32_t rx, ry, rw, rh;        // rectangle
    int32_t ix, iy, iw, ih;        // inner picture (output coordinates)
    int32_t cx, cy, cw, ch;        // effective crop
    int32_t src, kind_x, kind_y;
    int32_t tab_x, tab_y;          // first int32 of the axis tables in the pool (ENLARGE only)
    uint32_t pad, offline;         // b | g << 8 | r << 16
    int32_t reserved[5];
};
static_assert(sizeof(CpDevCell) == 96, "layout");
struct CpDevOut { int32_t h, w, fmt; uint32_t bg; };
struct CpDevTile { int32_t out, x0, y0, first, count, reserved; };
struct CpRunSrc { uint64_t ptr; int64_t pitch; };
struct CpRunDst { uint64_t y, u, v; int64_t pitch, cpitch, reserved; };

struct CpArgs {
    const CpDevCell *cells; const CpDevOut *outs; const CpDevTile *tiles; const uint16_t *list; const int32_t *tabs;
    const CpRunSrc *src; const CpRunDst *dst;
};

__host__ __device__ inline uint32_t cp_pack(const uint8_t *bgr) { return (uint32_t)bgr[0] | (uint32_t)bgr[1] << 8 | (uint32_t)bgr[2] << 16; }

// rows of `nbytes` bytes from an LDS tile to memory: row r of the tile starts at lds + r * stride + (address of the row & 15), so a
// 16-byte block of the row is aligned on both sides; whole blocks go as one store, the ragged ends byte by byte
__device__ __forceinline__ void cp_store_rows(const uint8_t *lds, int stride, uint8_t *g0, long long pitch, int rows, int nbytes, int tid) {
    const int nb = stride >> 4;
    for (int idx = tid; idx < rows * nb; idx += CP_THREADS) {
        const int r = idx / nb, s = idx - r * nb;
        uint8_t *g = g0 + (long long)r * pitch;
        const int mis = (int)((uintptr_t)g & 15);
        const int lo = max(16 * s, mis), hi = min(16 * s + 16, mis + nbytes);
        if (lo >= hi) continue;
        const uint8_t *l = lds + r * stride;
        uint8_t *a = g - mis;
        if (hi - lo == 16) *(uint4 *)(a + 16 * s) = *(const uint4 *)(l + 16 * s);
        else
            for (int b = lo; b < hi; ++b) a[b] = l[b];
    }
}

__global__ __launch_bounds__(CP_THREADS) void compose_tiles(CpArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_src[CP_STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[CP_TH * CP_OSTR];
    __shared__ __attribute__((aligned(16))) uint8_t s_p0[CP_TH * CP_PSTR];
    __shared__ __attribute__((aligned(16))) uint8_t s_p1[CP_TH / 2 * CP_PSTR];
    __shared__ __attribute__((aligned(16))) uint8_t s_p2[CP_TH / 2 * CP_PSTR];

    const int tid = threadIdx.x, tx = tid & (CP_TW - 1), ty = tid / CP_TW;
    const CpDevTile t = a.tiles[blockIdx.x];
    const CpDevOut o = a.outs[t.out];
    const int px = t.x0 + tx, py = t.y0 + ty;
    const bool inside = px < o.w && py < o.h;
    const int tw = min(CP_TW, o.w - t.x0), th = min(CP_TH, o.h - t.y0);

    int top = -1;
    if (inside)
        for (int k = t.count - 1; k >= 0; --k) {
            const CpDevCell &c = a.cells[a.list[t.first + k]];
            if (px >= c.rx && px < c.rx + c.rw && py >= c.ry && py < c.ry + c.rh) { top = k; break; }
        }

    uint32_t val = o.bg;
    for (int k = 0; k < t.count; ++k) {
        const bool mine = top == k;
        if (!__syncthreads_or(mine)) continue;
        const CpDevCell c = a.cells[a.list[t.first + k]];
        const CpRunSrc rs = a.src[c.src];
        if (!rs.ptr) {
            if (mine) val = c.offline;
            continue;
        }
        const bool in_inner = mine && px >= c.ix && px < c.ix + c.iw && py >= c.iy && py < c.iy + c.ih;
        if (mine && !in_inner) val = c.pad;
        // the tile's part of the inner picture, in the picture's own coordinates
        const int jx0 = max(t.x0, c.ix) - c.ix, jx1 = min(t.x0 + tw, c.ix + c.iw) - 1 - c.ix;
        const int jy0 = max(t.y0, c.iy) - c.iy, jy1 = min(t.y0 + th, c.iy + c.ih) - 1 - c.iy;
        if (jx0 > jx1 || jy0 > jy1) continue;
        const int32_t *tabx = a.tabs + c.tab_x, *taby = a.tabs + c.tab_y;
        // its footprint in the crop
        int32_t fx0, fx1, fy0, fy1, u;
        cp_span(c.kind_x, c.cw, c.iw, jx0, tabx, fx0, u);
        cp_span(c.kind_x, c.cw, c.iw, jx1, tabx, u, fx1);
        cp_span(c.kind_y, c.ch, c.ih, jy0, taby, fy0, u);
        cp_span(c.kind_y, c.ch, c.ih, jy1, taby, u, fy1);
        // this thread's taps
        const int jx = px - c.ix, jy = py - c.iy;
        int32_t x0 = 0, x1 = -1, y0 = 0, y1 = -1;
        if (in_inner) {
            cp_span(c.kind_x, c.cw, c.iw, jx, tabx, x0, x1);
            cp_span(c.kind_y, c.ch, c.ih, jy, taby, y0, y1);
        }
        const uint8_t *sbase = (const uint8_t *)rs.ptr;
        const long long spitch = rs.pitch;
        const int cw_max = min(fx1 - fx0 + 1, CP_CHUNK);
        const int nbk = (15 + 3 * cw_max + 15) >> 4, rstr = nbk << 4;       // 16-byte blocks and LDS bytes per staged row
        const int rb = CP_STAGE / rstr;                                    // rows per band
        uint64_t acc0 = 0, acc1 = 0, acc2 = 0;
        for (int yb = fy0; yb <= fy1; yb += rb) {
            const int nr = min(rb, fy1 - yb + 1);
            for (int xc = fx0; xc <= fx1; xc += CP_CHUNK) {
                const int cwc = min(CP_CHUNK, fx1 - xc + 1), nbytes = 3 * cwc;
                for (int idx = tid; idx < nr * nbk; idx += CP_THREADS) {
                    const int r = idx / nbk, s = idx - r * nbk;
                    const uint8_t *g = sbase + (long long)(c.cy + yb + r) * spitch + 3ll * (c.cx + xc);
                    const int mis = (int)((uintptr_t)g & 15);
                    const int lo = max(16 * s, mis), hi = min(16 * s + 16, mis + nbytes);
                    if (lo >= hi) continue;
                    const uint8_t *ga = g - mis;
                    uint8_t *l = s_src + r * rstr;
                    if (hi - lo == 16) *(uint4 *)(l + 16 * s) = *(const uint4 *)(ga + 16 * s);
                    else
                        for (int b = lo; b < hi; ++b) l[b] = ga[b];
                }
                __syncthreads();
                const int ya = max(y0, yb), yz = min(y1, yb + nr - 1), xa = max(x0, xc), xz = min(x1, xc + cwc - 1);
                if (xa <= xz)
                    for (int y = ya; y <= yz; ++y) {
                        const uint32_t wy = (uint32_t)cp_weight(c.kind_y, c.ch, c.ih, jy, y, taby);
                        const uint8_t *g = sbase + (long long)(c.cy + y) * spitch + 3ll * (c.cx + xc);
                        const uint8_t *l = s_src + (y - yb) * rstr + (int)((uintptr_t)g & 15) + 3 * (xa - xc);
                        uint32_t r0 = 0, r1 = 0, r2 = 0;
                        for (int x = xa; x <= xz; ++x, l += 3) {
                            const uint32_t wx = (uint32_t)cp_weight(c.kind_x, c.cw, c.iw, jx, x, tabx);
                            r0 += wx * l[0]; r1 += wx * l[1]; r2 += wx * l[2];
                        }
                        acc0 += (uint64_t)wy * r0; acc1 += (uint64_t)wy * r1; acc2 += (uint64_t)wy * r2;
                    }
                __syncthreads();
            }
        }
        if (in_inner) {
            const uint64_t tot = (uint64_t)cp_total(c.kind_x, c.cw) * (uint64_t)cp_total(c.kind_y, c.ch), half = tot >> 1;
            uint32_t b, g, r;
            if ((tot & (tot - 1)) == 0) {
                const int sh = __ffsll((long long)tot) - 1;
                b = (uint32_t)((acc0 + half) >> sh); g = (uint32_t)((acc1 + half) >> sh); r = (uint32_t)((acc2 + half) >> sh);
            } else if (tot <= (1u << 24)) {                 // 255 tot + tot / 2 < 2^32
                const uint32_t d = (uint32_t)tot;
                b = (uint32_t)(acc0 + half) / d; g = (uint32_t)(acc1 + half) / d; r = (uint32_t)(acc2 + half) / d;
            } else {
                b = (uint32_t)((acc0 + half) / tot); g = (uint32_t)((acc1 + half) / tot); r = (uint32_t)((acc2 + half) / tot);
            }
            val = b | g << 8 | r << 16;
        }
    }

    const CpRunDst d = a.dst[t.out];
    if (o.fmt == RTMODT_PIX_BGR24) {
        uint8_t *g0 = (uint8_t *)d.y + (long long)t.y0 * d.pitch + 3ll * t.x0;
        if (inside) {
            uint8_t *l = s_out + ty * CP_OSTR + (int)((uintptr_t)(g0 + (long long)ty * d.pitch) & 15) + 3 * tx;
            l[0] = (uint8_t)val; l[1] = (uint8_t)(val >> 8); l[2] = (uint8_t)(val >> 16);
        }
        __syncthreads();
        cp_store_rows(s_out, CP_OSTR, g0, d.pitch, th, 3 * tw, tid);
        return;
    }
    // 4:2:0 (w, h and so tw, th are even; a 2 x 2 block lies inside one tile)
    const int vb = val & 255, vg = (val >> 8) & 255, vr = (val >> 16) & 255;
    uint8_t *gy = (uint8_t *)d.y + (long long)t.y0 * d.pitch + t.x0;
    if (inside) {
        uint8_t *l = s_out + ty * CP_OSTR + 3 * tx;
        l[0] = (uint8_t)vb; l[1] = (uint8_t)vg; l[2] = (uint8_t)vr;
        s_p0[ty * CP_PSTR + (int)((uintptr_t)(gy + (long long)ty * d.pitch) & 15) + tx] = (uint8_t)cp_yuv_y(vb, vg, vr);
    }
    __syncthreads();
    const bool nv12 = o.fmt == RTMODT_PIX_NV12;
    const long long crow = (long long)(t.y0 >> 1) * d.cpitch;
    uint8_t *gu = (uint8_t *)d.u + crow + (nv12 ? t.x0 : t.x0 >> 1), *gv = (uint8_t *)d.v + crow + (t.x0 >> 1);
    if (inside && !(tx & 1) && !(ty & 1)) {
        const uint8_t *p = s_out + ty * CP_OSTR + 3 * tx, *q = p + CP_OSTR;
        const int mb = cp_block_mean(p[0], p[3], q[0], q[3]), mg = cp_block_mean(p[1], p[4], q[1], q[4]), mr = cp_block_mean(p[2], p[5], q[2], q[5]);
        const uint8_t U = (uint8_t)cp_yuv_u(mb, mg, mr), V = (uint8_t)cp_yuv_v(mb, mg, mr);
        const int cr = ty >> 1;
        if (nv12) {
            uint8_t *l = s_p1 + cr * CP_PSTR + (int)((uintptr_t)(gu + (long long)cr * d.cpitch) & 15) + tx;
            l[0] = U; l[1] = V;
        } else {
            s_p1[cr * CP_PSTR + (int)((uintptr_t)(gu + (long long)cr * d.cpitch) & 15) + (tx >> 1)] = U;
            s_p2[cr * CP_PSTR + (int)((uintptr_t)(gv + (long long)cr * d.cpitch) & 15) + (tx >> 1)] = V;
        }
    }
    __syncthreads();
    cp_store_rows(s_p0, CP_PSTR, gy, d.pitch, th, tw, tid);
    cp_store_rows(s_p1, CP_PSTR, gu, d.cpitch, th >> 1, nv12 ? tw : tw >> 1, tid);
    if (!nv12) cp_store_rows(s_p2, CP_PSTR, gv, d.cpitch, th >> 1, tw >> 1, tid);
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

namespace {

// a layout as the device holds it; the handle keeps the one in force and swaps a new one in only when it is complete
struct CpLayout {
    std::vector<rtmodt_compose_src_desc> sources;
    std::vector<rtmodt_compose_out_desc> outputs;
    std::vector<rtmodt_compose_cell> cells;
    std::vector<CpPlan> plans;
    std::vector<CpDevCell> dcells;
    long long n_tiles = 0;
    char *d_pool = nullptr;                 // cells | outs | tiles | list | tabs
    size_t o_cells = 0, o_outs = 0, o_tiles = 0, o_list = 0, o_tabs = 0;
    uint8_t *d_own = nullptr;               // the handle's own buffers of the outputs
    std::vector<size_t> own_off, own_pitch;
    std::vector<size_t> stage_off;          // host sources staged at tight16 pitch
    size_t stage_bytes = 0;
    void release() {
        hipFree(d_pool); hipFree(d_own);
        d_pool = nullptr; d_own = nullptr;
    }
};

CpRect cp_cell_rect(const rtmodt_compose_cell &c) { return CpRect{c.x, c.y, c.w, c.h}; }
CpRect cp_cell_crop(const rtmodt_compose_cell &c) { return CpRect{c.crop_x, c.crop_y, c.crop_w, c.crop_h}; }
bool cp_yuv(int pf) { return pf == RTMODT_PIX_NV12 || pf == RTMODT_PIX_I420; }

int cp_check_crop(const CpRect &crop, const rtmodt_compose_src_desc &s, int cell) {
    const bool whole = crop.x == 0 && crop.y == 0 && crop.w == 0 && crop.h == 0;
    RT_CHECK(whole || cp_rect_inside(crop, s.h, s.w), RTMODT_E_INVALID, "cell %d: crop %d,%d %dx%d leaves its %dx%d source", cell, crop.x, crop.y, crop.w,
             crop.h, s.w, s.h);
    return RTMODT_OK;
}

// THE validator of a layout (host only); plans[n_cells] when it passes
int cp_validate(const rtmodt_compose_cfg &lim, const rtmodt_compose_src_desc *sources, int n_sources, const rtmodt_compose_out_desc *outputs, int n_outputs,
                const rtmodt_compose_cell *cells, int n_cells, std::vector<CpPlan> &plans) {
    RT_CHECK(sources && outputs && (cells || n_cells == 0), RTMODT_E_INVALID, "null argument");
    RT_CHECK(n_sources >= 1 && n_outputs >= 1 && n_cells >= 0, RTMODT_E_INVALID, "%d sources, %d outputs, %d cells: at least one source and one output", n_sources,
             n_outputs, n_cells);
    RT_CHECK(n_sources <= lim.max_sources, RTMODT_E_CAPACITY, "%d sources (at most %d)", n_sources, lim.max_sources);
    RT_CHECK(n_outputs <= lim.max_outputs, RTMODT_E_CAPACITY, "%d outputs (at most %d)", n_outputs, lim.max_outputs);
    for (int i = 0; i < n_sources; ++i)
        RT_CHECK(sources[i].h >= 1 && sources[i].w >= 1 && sources[i].h <= lim.max_dim && sources[i].w <= lim.max_dim, RTMODT_E_INVALID,
                 "source %d: size %dx%d outside 1..%d", i, sources[i].w, sources[i].h, lim.max_dim);
    for (int i = 0; i < n_outputs; ++i) {
        const rtmodt_compose_out_desc &o = outputs[i];
        RT_CHECK(o.h >= 1 && o.w >= 1 && o.h <= lim.max_dim && o.w <= lim.max_dim, RTMODT_E_INVALID, "output %d: size %dx%d outside 1..%d", i, o.w, o.h,
                 lim.max_dim);
        RT_CHECK(o.pixel_format == RTMODT_PIX_BGR24 || cp_yuv(o.pixel_format), RTMODT_E_INVALID, "output %d: unknown pixel format %d", i, o.pixel_format);
        RT_CHECK(!cp_yuv(o.pixel_format) || (o.h % 2 == 0 && o.w % 2 == 0), RTMODT_E_INVALID, "output %d: a 4:2:0 output needs an even width and height, got %dx%d",
                 i, o.w, o.h);
    }
    std::vector<int> per_out(n_outputs, 0);
    for (int k = 0; k < n_cells; ++k) {
        const rtmodt_compose_cell &c = cells[k];
        RT_CHECK(c.output >= 0 && c.output < n_outputs, RTMODT_E_INVALID, "cell %d: output %d outside 0..%d", k, c.output, n_outputs - 1);
        RT_CHECK(c.source >= 0 && c.source < n_sources, RTMODT_E_INVALID, "cell %d: source %d outside 0..%d", k, c.source, n_sources - 1);
        RT_CHECK(c.fit == CP_STRETCH || c.fit == CP_FIT || c.fit == CP_FILL, RTMODT_E_INVALID, "cell %d: unknown fit mode %d", k, c.fit);
        RT_CHECK(++per_out[c.output] <= lim.max_cells, RTMODT_E_CAPACITY, "output %d: more than %d cells", c.output, lim.max_cells);
        const rtmodt_compose_out_desc &o = outputs[c.output];
        RT_CHECK(cp_rect_inside(cp_cell_rect(c), o.h, o.w), RTMODT_E_INVALID, "cell %d: rectangle %d,%d %dx%d leaves its %dx%d output", k, c.x, c.y, c.w, c.h, o.w,
                 o.h);
        RT_CHECK(!cp_yuv(o.pixel_format) || ((c.x | c.y | c.w | c.h) & 1) == 0, RTMODT_E_INVALID, "cell %d: rectangle %d,%d %dx%d on a 4:2:0 output must be even", k,
                 c.x, c.y, c.w, c.h);
        RT_TRY(cp_check_crop(cp_cell_crop(c), sources[c.source], k));
    }
    plans.resize(n_cells);
    for (int k = 0; k < n_cells; ++k) {
        const rtmodt_compose_cell &c = cells[k];
        cp_plan(sources[c.source].h, sources[c.source].w, cp_cell_crop(c), cp_cell_rect(c), c.fit, cp_yuv(outputs[c.output].pixel_format), plans[k]);
    }
    return RTMODT_OK;
}

rtmodt_compose_cfg cp_widest() { return rtmodt_compose_cfg{0, CP_MAX_SOURCES, CP_MAX_OUTPUTS, CP_MAX_CELLS, CP_MAX_DIM}; }

// cell k's device record and (into tabs, at the cell's fixed region) the tables of its enlarging axes
void cp_dev_cell(const rtmodt_compose_cell &c, const CpPlan &p, int32_t tab_base, CpDevCell &d, int32_t *tabs) {
    d = CpDevCell{};
    d.rx = c.x; d.ry = c.y; d.rw = c.w; d.rh = c.h;
    d.ix = p.inner.x; d.iy = p.inner.y; d.iw = p.inner.w; d.ih = p.inner.h;
    d.cx = p.crop.x; d.cy = p.crop.y; d.cw = p.crop.w; d.ch = p.crop.h;
    d.src = c.source; d.kind_x = p.kind_x; d.kind_y = p.kind_y;
    d.tab_x = tab_base; d.tab_y = tab_base + 3 * c.w;
    d.pad = cp_pack(c.pad_bgr); d.offline = cp_pack(c.offline_bgr);
    if (p.kind_x == CP_ENLARGE) resize_table(d.iw, d.cw, tabs + d.tab_x, tabs + d.tab_x + d.iw, tabs + d.tab_x + 2 * d.iw);
    if (p.kind_y == CP_ENLARGE) resize_table(d.ih, d.ch, tabs + d.tab_y, tabs + d.tab_y + d.ih, tabs + d.tab_y + 2 * d.ih);
}

// the planes of one destination, resolved: rtmodt_frame_format's defaults and checks as csrc/engine.hip (resolve_frame_format) applies
// them to the frames the detector reads
struct CpPlanes { int64_t pitch = 0, cpitch = 0, uo = 0, vo = 0; int n = 0; int64_t start[3] = {}, end[3] = {}, rowbytes[3] = {}, rows[3] = {}, ppitch[3] = {}; };

int cp_resolve_fmt(int i, const rtmodt_compose_out_desc &o, const rtmodt_frame_format *fmt, CpPlanes &pl) {
    const int pf = fmt ? fmt->pixel_format : o.pixel_format;
    RT_CHECK(pf == o.pixel_format, RTMODT_E_INVALID, "output %d: the destination's pixel format %d is not the layout's %d", i, pf, o.pixel_format);
    const int h = o.h, w = o.w;
    if (pf == RTMODT_PIX_BGR24) {
        pl.pitch = fmt && fmt->pitch ? fmt->pitch : 3 * w;
        RT_CHECK(pl.pitch >= 3 * w, RTMODT_E_INVALID, "output %d: bad frame geometry %dx%d pitch %lld", i, w, h, (long long)pl.pitch);
        pl.n = 1; pl.start[0] = 0; pl.rowbytes[0] = 3 * w; pl.rows[0] = h; pl.ppitch[0] = pl.pitch;
        pl.end[0] = pl.pitch * (h - 1) + 3 * w;
        return RTMODT_OK;
    }
    const bool nv12 = pf == RTMODT_PIX_NV12;
    RT_CHECK(!fmt || fmt->colorspace == 0, RTMODT_E_UNSUPPORTED, "output %d: colorspace %d: only 0 (BT.601 limited range) is implemented", i, fmt->colorspace);
    const int64_t pitch = fmt && fmt->pitch ? fmt->pitch : w;
    const int64_t crow = nv12 ? w : w / 2;
    const int64_t cp = fmt && fmt->chroma_pitch ? fmt->chroma_pitch : (nv12 ? pitch : pitch / 2);
    RT_CHECK(pitch >= w, RTMODT_E_INVALID, "output %d: Y pitch %lld < width %d", i, (long long)pitch, w);
    RT_CHECK(cp >= crow, RTMODT_E_INVALID, "output %d: chroma pitch %lld < %lld bytes per chroma row", i, (long long)cp, (long long)crow);
    const int64_t uo = fmt && fmt->u_offset ? fmt->u_offset : pitch * h;
    const int64_t vo = nv12 ? 0 : (fmt && fmt->v_offset ? fmt->v_offset : uo + cp * (h / 2));
    RT_CHECK(uo > 0 && vo >= 0, RTMODT_E_INVALID, "output %d: negative plane offset (u %lld, v %lld)", i, (long long)uo, (long long)vo);
    const int64_t y_end = pitch * (h - 1) + w, c_rows = h / 2;
    const int64_t u_end = uo + cp * (c_rows - 1) + crow, v_end = nv12 ? 0 : vo + cp * (c_rows - 1) + crow;
    auto apart = [](int64_t a0, int64_t a1, int64_t b0, int64_t b1) { return a1 <= b0 || b1 <= a0; };
    RT_CHECK(apart(0, y_end, uo, u_end), RTMODT_E_INVALID, "output %d: the %s plane [%lld, %lld) overlaps the Y plane [0, %lld)", i, nv12 ? "UV" : "U",
             (long long)uo, (long long)u_end, (long long)y_end);
    if (!nv12) {
        RT_CHECK(apart(0, y_end, vo, v_end), RTMODT_E_INVALID, "output %d: the V plane [%lld, %lld) overlaps the Y plane [0, %lld)", i, (long long)vo,
                 (long long)v_end, (long long)y_end);
        RT_CHECK(apart(uo, u_end, vo, v_end), RTMODT_E_INVALID, "output %d: the V plane [%lld, %lld) overlaps the U plane [%lld, %lld)", i, (long long)vo,
                 (long long)v_end, (long long)uo, (long long)u_end);
    }
    RT_CHECK(pitch <= INT32_MAX && cp <= INT32_MAX && std::max(y_end, std::max(u_end, v_end)) <= ((int64_t)1 << 40), RTMODT_E_INVALID,
             "output %d: frame layout too large", i);
    pl.pitch = pitch; pl.cpitch = cp; pl.uo = uo; pl.vo = vo;
    pl.n = nv12 ? 2 : 3;
    pl.start[0] = 0; pl.end[0] = y_end; pl.rowbytes[0] = w; pl.rows[0] = h; pl.ppitch[0] = pitch;
    pl.start[1] = uo; pl.end[1] = u_end; pl.rowbytes[1] = crow; pl.rows[1] = c_rows; pl.ppitch[1] = cp;
    pl.start[2] = vo; pl.end[2] = v_end; pl.rowbytes[2] = crow; pl.rows[2] = c_rows; pl.ppitch[2] = cp;
    return RTMODT_OK;
}

}  // namespace

struct rtmodt_compose : HandleBase {
    rtmodt_compose_cfg cfg{};
    bool dev_ready = false, has_layout = false;
    EventTimer<2> timer;
    CpLayout lay;
    CmdBuf cmd;                         // (every run ends with a synchronize: the pinned half is idle when the next one writes it)
    uint8_t *d_stage = nullptr;         // host sources
    size_t stage_cap = 0;
};

namespace {

int cp_ensure_device(rtmodt_compose *p) {
    RT_HIP(hipSetDevice(p->device));
    if (p->dev_ready) return RTMODT_OK;
    if (!p->stream) RT_TRY(handle_open(p));
    RT_TRY(p->timer.create());           // (makes the events a failed attempt did not)
    p->dev_ready = true;
    return RTMODT_OK;
}

// the host half of a layout: device records, tables, tiles and list, all in `pool` (the image of the device pool)
int cp_build(CpLayout &L, std::vector<char> &pool) {
    const int n_out = (int)L.outputs.size(), n_cells = (int)L.cells.size();
    long long n_tiles = 0;
    for (const rtmodt_compose_out_desc &o : L.outputs) n_tiles += (long long)cdiv(o.w, CP_TW) * cdiv(o.h, CP_TH);
    RT_CHECK(n_tiles <= CP_MAX_TILES, RTMODT_E_CAPACITY, "%lld tiles of %dx%d pixels (at most %lld)", n_tiles, CP_TW, CP_TH, CP_MAX_TILES);
    L.n_tiles = n_tiles;
    // tables: every cell owns 3 (w + h) int32, whatever its axes are now (set_crop may change their kind)
    std::vector<int32_t> tab_base(n_cells);
    size_t n_tab = 0;
    for (int k = 0; k < n_cells; ++k) {
        tab_base[k] = (int32_t)n_tab;
        n_tab += (size_t)3 * (L.cells[k].w + L.cells[k].h);
    }
    RT_CHECK(n_tab <= (size_t)INT32_MAX, RTMODT_E_CAPACITY, "the cells' rectangles are too large for the axis tables");
    std::vector<int32_t> tabs(std::max<size_t>(n_tab, 1), 0);
    L.dcells.resize(n_cells);
    for (int k = 0; k < n_cells; ++k) cp_dev_cell(L.cells[k], L.plans[k], tab_base[k], L.dcells[k], tabs.data());
    // tiles and their lists
    std::vector<std::vector<int>> of_out(n_out);
    for (int k = 0; k < n_cells; ++k) of_out[L.cells[k].output].push_back(k);
    std::vector<CpDevTile> tiles;
    tiles.reserve((size_t)n_tiles);
    std::vector<uint16_t> list;
    std::vector<int> cand;
    for (int i = 0; i < n_out; ++i) {
        const rtmodt_compose_out_desc &o = L.outputs[i];
        for (int y0 = 0; y0 < o.h; y0 += CP_TH)
            for (int x0 = 0; x0 < o.w; x0 += CP_TW) {
                const int x1 = std::min(x0 + CP_TW, o.w), y1 = std::min(y0 + CP_TH, o.h);
                cand.clear();
                for (int k : of_out[i]) {
                    const rtmodt_compose_cell &c = L.cells[k];
                    if (c.x < x1 && c.x + c.w > x0 && c.y < y1 && c.y + c.h > y0) cand.push_back(k);
                }
                CpDevTile t{i, x0, y0, (int32_t)list.size(), 0, 0};
                for (size_t m = 0; m < cand.size(); ++m) {
                    const rtmodt_compose_cell &c = L.cells[cand[m]];
                    const int ax0 = std::max(c.x, x0), ay0 = std::max(c.y, y0), ax1 = std::min(c.x + c.w, x1), ay1 = std::min(c.y + c.h, y1);
                    bool hidden = false;
                    for (size_t q = m + 1; q < cand.size() && !hidden; ++q) {
                        const rtmodt_compose_cell &e = L.cells[cand[q]];
                        hidden = e.x <= ax0 && e.y <= ay0 && e.x + e.w >= ax1 && e.y + e.h >= ay1;
                    }
                    if (!hidden) { list.push_back((uint16_t)cand[m]); ++t.count; }
                }
                tiles.push_back(t);
            }
    }
    RT_CHECK(list.size() <= (size_t)INT32_MAX, RTMODT_E_CAPACITY, "the tile work list is too long");
    L.o_cells = 0;
    L.o_outs = align_up(std::max<size_t>(n_cells, 1) * sizeof(CpDevCell), 16);
    L.o_tiles = align_up(L.o_outs + n_out * sizeof(CpDevOut), 16);
    L.o_list = align_up(L.o_tiles + tiles.size() * sizeof(CpDevTile), 16);
    L.o_tabs = align_up(L.o_list + std::max<size_t>(list.size(), 1) * sizeof(uint16_t), 16);
    pool.assign(L.o_tabs + tabs.size() * sizeof(int32_t), 0);
    if (n_cells) memcpy(pool.data() + L.o_cells, L.dcells.data(), n_cells * sizeof(CpDevCell));
    for (int i = 0; i < n_out; ++i) {
        const rtmodt_compose_out_desc &o = L.outputs[i];
        const CpDevOut d{o.h, o.w, o.pixel_format, cp_pack(o.background_bgr)};
        memcpy(pool.data() + L.o_outs + i * sizeof(CpDevOut), &d, sizeof(d));
    }
    memcpy(pool.data() + L.o_tiles, tiles.data(), tiles.size() * sizeof(CpDevTile));
    if (!list.empty()) memcpy(pool.data() + L.o_list, list.data(), list.size() * sizeof(uint16_t));
    memcpy(pool.data() + L.o_tabs, tabs.data(), tabs.size() * sizeof(int32_t));
    // the handle's own buffers: rows of align_up(3w | w, 16) bytes, 4:2:0 planes at rtmodt_frame_format's defaults for that pitch
    size_t own = 0;
    L.own_off.resize(n_out); L.own_pitch.resize(n_out);
    for (int i = 0; i < n_out; ++i) {
        const rtmodt_compose_out_desc &o = L.outputs[i];
        const bool yuv = cp_yuv(o.pixel_format);
        L.own_pitch[i] = yuv ? align_up((size_t)o.w, 16) : tight16_pitch(o.w);
        L.own_off[i] = own;
        own += align_up(L.own_pitch[i] * o.h * (yuv ? 3 : 2) / 2, 256);
    }
    L.stage_off.resize(L.sources.size());
    L.stage_bytes = 0;
    for (size_t s = 0; s < L.sources.size(); ++s) {
        L.stage_off[s] = L.stage_bytes;
        L.stage_bytes += align_up(tight16_pitch(L.sources[s].w) * L.sources[s].h, 256);
    }
    L.own_off.push_back(own);           // (the total, read by the allocation)
    return RTMODT_OK;
}

bool cp_meet(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

}  // namespace

extern "C" {

void rtmodt_compose_default_cfg(rtmodt_compose_cfg *cfg) {
    if (!cfg) return;
    *cfg = cp_widest();
}

void rtmodt_compose_destroy(rtmodt_compose *p) {
    if (!p) return;
    if (p->dev_ready || p->stream)
        handle_close(p, [&] {
            p->lay.release();
            hipFree(p->d_stage);
            p->cmd.release();
            p->timer.destroy();
        });
    delete p;
}

int rtmodt_compose_create(const rtmodt_compose_cfg *cfg, rtmodt_compose **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(cfg->device >= 0, RTMODT_E_INVALID, "device %d", cfg->device);
    RT_CHECK(cfg->max_sources >= 1 && cfg->max_sources <= CP_MAX_SOURCES, RTMODT_E_INVALID, "max_sources %d outside 1..%d", cfg->max_sources, CP_MAX_SOURCES);
    RT_CHECK(cfg->max_outputs >= 1 && cfg->max_outputs <= CP_MAX_OUTPUTS, RTMODT_E_INVALID, "max_outputs %d outside 1..%d", cfg->max_outputs, CP_MAX_OUTPUTS);
    RT_CHECK(cfg->max_cells >= 1 && cfg->max_cells <= CP_MAX_CELLS, RTMODT_E_INVALID, "max_cells %d outside 1..%d", cfg->max_cells, CP_MAX_CELLS);
    RT_CHECK(cfg->max_dim >= 1 && cfg->max_dim <= CP_MAX_DIM, RTMODT_E_INVALID, "max_dim %d outside 1..%d", cfg->max_dim, CP_MAX_DIM);
    rtmodt_compose *p = new rtmodt_compose();
    p->device = cfg->device;
    p->cfg = *cfg;
    *out = p;
    return RTMODT_OK;
}

int rtmodt_compose_set_layout(rtmodt_compose *p, const rtmodt_compose_src_desc *sources, int n_sources, const rtmodt_compose_out_desc *outputs, int n_outputs,
                              const rtmodt_compose_cell *cells, int n_cells) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    CpLayout L;
    RT_TRY(cp_validate(p->cfg, sources, n_sources, outputs, n_outputs, cells, n_cells, L.plans));
    L.sources.assign(sources, sources + n_sources);
    L.outputs.assign(outputs, outputs + n_outputs);
    L.cells.assign(cells, cells + n_cells);
    std::vector<char> pool;
    RT_TRY(cp_build(L, pool));
    RT_TRY(cp_ensure_device(p));
    auto body = [&]() -> int {
        RT_HIP(hipMalloc((void **)&L.d_pool, pool.size()));
        RT_HIP(hipMalloc((void **)&L.d_own, std::max<size_t>(L.own_off.back(), 16)));
        RT_HIP(hipMemcpyAsync(L.d_pool, pool.data(), pool.size(), hipMemcpyHostToDevice, p->stream));
        RT_HIP(hipMemsetAsync(L.d_own, 0, std::max<size_t>(L.own_off.back(), 16), p->stream));
        RT_HIP(hipStreamSynchronize(p->stream));
        return RTMODT_OK;
    };
    const int rc = body();
    if (rc != RTMODT_OK) {
        L.release();
        return rc;
    }
    p->lay.release();                   // (every run ended with a synchronize: nothing reads the old pool)
    p->lay = std::move(L);
    p->has_layout = true;
    p->timer.timed = false;
    return RTMODT_OK;
}

int rtmodt_compose_set_crop(rtmodt_compose *p, int cell, int x, int y, int w, int hgt) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    RT_CHECK(p->has_layout, RTMODT_E_INVALID, "no layout has been set");
    CpLayout &L = p->lay;
    RT_CHECK(cell >= 0 && cell < (int)L.cells.size(), RTMODT_E_INVALID, "cell %d outside 0..%d", cell, (int)L.cells.size() - 1);
    rtmodt_compose_cell c = L.cells[cell];
    c.crop_x = x; c.crop_y = y; c.crop_w = w; c.crop_h = hgt;
    const rtmodt_compose_src_desc &s = L.sources[c.source];
    RT_TRY(cp_check_crop(cp_cell_crop(c), s, cell));
    CpPlan plan;
    cp_plan(s.h, s.w, cp_cell_crop(c), cp_cell_rect(c), c.fit, cp_yuv(L.outputs[c.output].pixel_format), plan);
    // the cell's record and its own region of the tables, rebuilt on the host and sent as two copies
    const int32_t base = L.dcells[cell].tab_x, n = 3 * (c.w + c.h);
    std::vector<int32_t> tabs((size_t)n, 0);
    CpDevCell d;
    cp_dev_cell(c, plan, 0, d, tabs.data());
    d.tab_x += base; d.tab_y += base;
    RT_TRY(cp_ensure_device(p));
    RT_HIP(hipMemcpyAsync(L.d_pool + L.o_cells + (size_t)cell * sizeof(CpDevCell), &d, sizeof(d), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(L.d_pool + L.o_tabs + (size_t)base * 4, tabs.data(), (size_t)n * 4, hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    L.cells[cell] = c; L.plans[cell] = plan; L.dcells[cell] = d;
    return RTMODT_OK;
}

int rtmodt_compose_run(rtmodt_compose *p, const uint8_t *const *src, const int32_t *src_pitch, int src_mem_kind, uint8_t *const *dst,
                       const rtmodt_frame_format *dst_fmt, int dst_mem_kind) {
    RT_CHECK(p && src, RTMODT_E_INVALID, "null argument");
    p->timer.timed = false;
    RT_CHECK(p->has_layout, RTMODT_E_INVALID, "no layout has been set");
    RT_TRY(check_mem_kind(src_mem_kind));
    RT_TRY(check_mem_kind(dst_mem_kind));
    CpLayout &L = p->lay;
    const int ns = (int)L.sources.size(), no = (int)L.outputs.size();
    const bool shost = src_mem_kind == RTMODT_MEM_HOST, dhost = dst_mem_kind == RTMODT_MEM_HOST;
    std::vector<int64_t> spitch(ns);
    for (int i = 0; i < ns; ++i) {
        spitch[i] = src_pitch ? src_pitch[i] : 3 * L.sources[i].w;
        RT_CHECK(!src[i] || spitch[i] >= 3ll * L.sources[i].w, RTMODT_E_INVALID, "source %d: bad frame geometry %dx%d, pitch %lld", i, L.sources[i].w,
                 L.sources[i].h, (long long)spitch[i]);
    }
    std::vector<CpPlanes> planes(no);
    for (int i = 0; i < no; ++i) RT_TRY(cp_resolve_fmt(i, L.outputs[i], dst && dst[i] && dst_fmt ? dst_fmt + i : nullptr, planes[i]));
    // a gather cannot work in place, and two destinations may not share a byte
    for (int i = 0; i < no; ++i) {
        if (!shost && (dhost || !dst || !dst[i])) {                       // composed in the handle's own buffer: no device source may lie in it
            const uintptr_t a0 = (uintptr_t)(L.d_own + L.own_off[i]), a1 = (uintptr_t)(L.d_own + L.own_off[i + 1]);
            for (int s = 0; s < ns; ++s) {
                const uintptr_t b0 = (uintptr_t)src[s], b1 = b0 + (uintptr_t)(spitch[s] * (L.sources[s].h - 1) + 3ll * L.sources[s].w);
                RT_CHECK(!src[s] || !cp_meet(a0, a1, b0, b1), RTMODT_E_INVALID, "source %d lies in the handle's own buffer of output %d", s, i);
            }
        }
        if (!dst || !dst[i]) continue;
        const uintptr_t d0 = (uintptr_t)dst[i];
        for (int k = 0; k < planes[i].n; ++k) {
            const uintptr_t a0 = d0 + planes[i].start[k], a1 = d0 + planes[i].end[k];
            for (int s = 0; s < ns; ++s) {
                if (!src[s]) continue;
                const uintptr_t b0 = (uintptr_t)src[s], b1 = b0 + (uintptr_t)(spitch[s] * (L.sources[s].h - 1) + 3ll * L.sources[s].w);
                RT_CHECK(!cp_meet(a0, a1, b0, b1), RTMODT_E_INVALID, "destination %d overlaps source %d of the run", i, s);
            }
            for (int j = 0; j < i; ++j) {
                if (!dst[j]) continue;
                for (int m = 0; m < planes[j].n; ++m)
                    RT_CHECK(!cp_meet(a0, a1, (uintptr_t)dst[j] + planes[j].start[m], (uintptr_t)dst[j] + planes[j].end[m]), RTMODT_E_INVALID,
                             "destination %d overlaps destination %d of the run", i, j);
            }
        }
    }
    RT_TRY(cp_ensure_device(p));
    hipStream_t q = p->stream;
    if (shost) RT_TRY(dev_grow(&p->d_stage, &p->stage_cap, L.stage_bytes));
    const size_t cmd_bytes = ns * sizeof(CpRunSrc) + no * sizeof(CpRunDst);
    RT_TRY(p->cmd.reserve(cmd_bytes));
    CpRunSrc *rs = (CpRunSrc *)p->cmd.h;
    CpRunDst *rd = (CpRunDst *)(p->cmd.h + ns * sizeof(CpRunSrc));
    for (int i = 0; i < ns; ++i) {
        if (!src[i]) { rs[i] = CpRunSrc{0, 0}; continue; }
        if (shost) {
            const size_t tp = tight16_pitch(L.sources[i].w);
            RT_TRY(copy_bgr_rows(p->d_stage + L.stage_off[i], tp, src[i], (size_t)spitch[i], L.sources[i].h, L.sources[i].w, hipMemcpyHostToDevice, q));
            rs[i] = CpRunSrc{(uint64_t)(uintptr_t)(p->d_stage + L.stage_off[i]), (int64_t)tp};
        } else rs[i] = CpRunSrc{(uint64_t)(uintptr_t)src[i], spitch[i]};
    }
    std::vector<CpPlanes> own(no);
    for (int i = 0; i < no; ++i) {
        const bool mine = !dst || !dst[i] || dhost;                       // composed in the handle's own buffer
        CpPlanes pl = planes[i];
        uint8_t *base = dst && dst[i] ? dst[i] : nullptr;
        if (mine) {
            rtmodt_frame_format f{};
            f.pixel_format = L.outputs[i].pixel_format; f.pitch = (int32_t)L.own_pitch[i];
            RT_TRY(cp_resolve_fmt(i, L.outputs[i], &f, pl));
            base = L.d_own + L.own_off[i];
        }
        own[i] = pl;
        rd[i] = CpRunDst{(uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)(base + pl.uo), (uint64_t)(uintptr_t)(base + pl.vo), pl.pitch, pl.cpitch, 0};
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, cmd_bytes, hipMemcpyHostToDevice, q));
    CpArgs a{};
    a.cells = (const CpDevCell *)(L.d_pool + L.o_cells); a.outs = (const CpDevOut *)(L.d_pool + L.o_outs);
    a.tiles = (const CpDevTile *)(L.d_pool + L.o_tiles); a.list = (const uint16_t *)(L.d_pool + L.o_list);
    a.tabs = (const int32_t *)(L.d_pool + L.o_tabs);
    a.src = (const CpRunSrc *)p->cmd.d; a.dst = (const CpRunDst *)(p->cmd.d + ns * sizeof(CpRunSrc));
    RT_TRY(p->timer.record(0, q));
    hipLaunchKernelGGL(compose_tiles, dim3((unsigned)L.n_tiles), dim3(CP_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    if (dhost)
        for (int i = 0; i < no; ++i) {
            if (!dst || !dst[i]) continue;
            const uint8_t *base = L.d_own + L.own_off[i];
            for (int k = 0; k < planes[i].n; ++k)       // rows only: the caller's padding is not touched
                RT_HIP(hipMemcpy2DAsync(dst[i] + planes[i].start[k], (size_t)planes[i].ppitch[k], base + own[i].start[k], (size_t)own[i].ppitch[k],
                                        (size_t)planes[i].rowbytes[k], (size_t)planes[i].rows[k], hipMemcpyDeviceToHost, q));
        }
    RT_HIP(hipStreamSynchronize(q));
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_compose_output(rtmodt_compose *p, int i, uint8_t **dev_ptr, size_t *pitch) {
    RT_CHECK(p && dev_ptr && pitch, RTMODT_E_INVALID, "null argument");
    RT_CHECK(p->has_layout, RTMODT_E_INVALID, "no layout has been set");
    RT_CHECK(i >= 0 && i < (int)p->lay.outputs.size(), RTMODT_E_INVALID, "output %d outside 0..%d", i, (int)p->lay.outputs.size() - 1);
    *dev_ptr = p->lay.d_own + p->lay.own_off[i];
    *pitch = p->lay.own_pitch[i];
    return RTMODT_OK;
}

int rtmodt_compose_last_ms(rtmodt_compose *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no run has launched yet");
}

int rtmodt_compose_plan(const rtmodt_compose_src_desc *sources, int n_sources, const rtmodt_compose_out_desc *outputs, int n_outputs,
                        const rtmodt_compose_cell *cells, int n_cells, rtmodt_compose_plan_out *plans) {
    std::vector<CpPlan> pl;
    RT_TRY(cp_validate(cp_widest(), sources, n_sources, outputs, n_outputs, cells, n_cells, pl));
    RT_CHECK(plans || n_cells == 0, RTMODT_E_INVALID, "null argument");
    for (int k = 0; k < n_cells; ++k) {
        const CpPlan &q = pl[k];
        plans[k] = rtmodt_compose_plan_out{{q.crop.x, q.crop.y, q.crop.w, q.crop.h}, {q.inner.x, q.inner.y, q.inner.w, q.inner.h}, q.kind_x, q.kind_y};
    }
    return RTMODT_OK;
}

}  // extern "C"
