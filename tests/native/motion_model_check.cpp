// Stand-alone program around csrc/motion_model.h and csrc/cell_grid.h (plain C++, no HIP): tests/test_motion_cpu.py builds it plain and
// with the address / undefined-behaviour sanitizers and compares every line with tests/motion_ref.py.
// stdin, one case per line:
//   c learn_shift learn_shift_fg threshold dev_gain warmup yc frames_seen bg dev      one cell through mo_cell
//   f scale h w seed                                                                a frame of h x w pixels from a 32-bit LCG (seed),
//                                                                                   its cell lumas through mo_luma / mo_cell_span / mo_cell_mean
//   r scale h w pitch base_offset wide seed                                         a frame in a buffer of exactly base_offset + (h - 1) * pitch + 3w
//                                                                                   bytes from the LCG, its cell lumas through cell_grid.h's reader
//                                                                                   the way the kernels' threads walk it: every lane of every tile
//   b cx0 cy0 cx1 cy1 scale w h                                                     mo_px_box
//   s frames_seen warmup n_raw scene_pm cells n_regions_total                       mo_status and mo_next_seen
// stdout, one line per case: "raw bg dev" | "gw gh yc yc ..." row by row | "x0 y0 x1 y1" | "status next"; "bad" for a rule, a scale
// or a size outside its range; then "done N".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cell_grid.h"

using namespace rtmodt;

// every thread of every model-grid tile, dead lanes included; false unless every cell of the grid was written exactly once
template <int SCALE> bool read_grid(bool wide, const uint8_t *frame, long long pitch, int h, int w) {
    constexpr int CPT = CgRun<SCALE>::CPT;
    const int gw = mo_grid(w, SCALE), gh = mo_grid(h, SCALE), tiles_x = cg_tiles_x(gw, SCALE), tiles = tiles_x * cg_tiles_y(gh);
    std::vector<uint32_t> yc((size_t)gw * gh, 0);
    std::vector<int> hits((size_t)gw * gh, 0);
    for (int tile = 0; tile < tiles; ++tile)
        for (int tid = 0; tid < CG_THREADS; ++tid) {
            const CgLane l = cg_lane<SCALE>((unsigned)tile, tiles_x, tid, frame, pitch, h, w, gw, gh);
            if (!l.live) continue;
            uint32_t sum[CPT];
            if (wide) cg_read_run<SCALE, true>(l.p, pitch, l.npx, l.nrows, sum);
            else cg_read_run<SCALE, false>(l.p, pitch, l.npx, l.nrows, sum);
            for (int j = 0; j < CPT; ++j) {
                uint32_t y;
                if (!cg_cell_luma<SCALE>(sum[j], l.cxb + j, l.nrows, w, y)) continue;
                yc[(size_t)l.cy * gw + l.cxb + j] = y;
                ++hits[(size_t)l.cy * gw + l.cxb + j];
            }
        }
    for (int v : hits)
        if (v != 1) return false;
    printf("%d %d", gw, gh);
    for (uint32_t v : yc) printf(" %u", v);
    putchar('\n');
    return true;
}

int main() {
    long n = 0;
    char kind;
    while (scanf(" %c", &kind) == 1) {
        ++n;
        if (kind == 'c') {
            MoRule r;
            unsigned yc, bg, dev;
            int seen;
            if (scanf("%d %d %d %d %d %u %d %u %u", &r.learn_shift, &r.learn_shift_fg, &r.threshold, &r.dev_gain, &r.warmup, &yc, &seen, &bg, &dev) != 9)
                return 2;
            if (!mo_rule_ok(r) || yc > 255 || seen < 0 || seen > MO_MAX_SEEN || bg > 65535 || dev > 65535) {
                puts("bad");
                continue;
            }
            uint32_t b = bg, d = dev;
            const bool raw = mo_cell(r, yc, seen, b, d);
            printf("%d %u %u\n", raw ? 1 : 0, b, d);
        } else if (kind == 'f') {
            int scale, h, w;
            unsigned seed;
            if (scanf("%d %d %d %u", &scale, &h, &w, &seed) != 4) return 2;
            if (!mo_scale_ok(scale) || h < 1 || w < 1 || h > 4096 || w > 4096) {
                puts("bad");
                continue;
            }
            std::vector<uint8_t> px((size_t)h * w * 3);
            uint32_t x = seed;
            for (auto &v : px) {
                x = x * 1664525u + 1013904223u;
                v = (uint8_t)(x >> 24);
            }
            const int gw = mo_grid(w, scale), gh = mo_grid(h, scale);
            printf("%d %d", gw, gh);
            for (int cy = 0; cy < gh; ++cy)
                for (int cx = 0; cx < gw; ++cx) {
                    const int cols = mo_cell_span(cx, scale, w), rows = mo_cell_span(cy, scale, h);
                    uint32_t sum = 0;
                    for (int y = cy * scale; y < cy * scale + rows; ++y)
                        for (int xx = cx * scale; xx < cx * scale + cols; ++xx) {
                            const uint8_t *p = &px[((size_t)y * w + xx) * 3];
                            sum += mo_luma(p[0], p[1], p[2]);
                        }
                    printf(" %u", mo_cell_mean(sum, (uint32_t)(cols * rows)));
                }
            putchar('\n');
        } else if (kind == 'r') {
            int scale, h, w, wide;
            long long pitch, base;
            unsigned seed;
            if (scanf("%d %d %d %lld %lld %d %u", &scale, &h, &w, &pitch, &base, &wide, &seed) != 7) return 2;
            // the host takes the dword path only when every base and the pitch are multiples of 4 (grid_host.h: frames_wide)
            if (!mo_scale_ok(scale) || h < 1 || w < 1 || h > 4096 || w > 4096 || pitch < 3LL * w || pitch > 65536 || base < 0 || base > 64 ||
                (wide && (pitch % 4 || base % 4))) {
                puts("bad");
                continue;
            }
            const size_t bytes = (size_t)(base + (h - 1) * pitch + 3LL * w);      // what a frame owns, and not one byte more
            uint8_t *buf = (uint8_t *)malloc(bytes);
            if (!buf) return 3;
            uint32_t x = seed;
            for (size_t i = 0; i < bytes; ++i) {
                x = x * 1664525u + 1013904223u;
                buf[i] = (uint8_t)(x >> 24);
            }
            const uint8_t *frame = buf + base;
            const bool ok = scale == 1 ? read_grid<1>(wide, frame, pitch, h, w) : scale == 2 ? read_grid<2>(wide, frame, pitch, h, w)
                          : scale == 4 ? read_grid<4>(wide, frame, pitch, h, w) : read_grid<8>(wide, frame, pitch, h, w);
            free(buf);
            if (!ok) puts("bad");
        } else if (kind == 'b') {
            int c[4], scale, w, h, out[4];
            if (scanf("%d %d %d %d %d %d %d", &c[0], &c[1], &c[2], &c[3], &scale, &w, &h) != 7) return 2;
            if (!mo_scale_ok(scale)) {
                puts("bad");
                continue;
            }
            mo_px_box(c[0], c[1], c[2], c[3], scale, w, h, out);
            printf("%d %d %d %d\n", out[0], out[1], out[2], out[3]);
        } else if (kind == 's') {
            int seen, warmup, scene_pm;
            unsigned n_raw, total;
            long long cells;
            if (scanf("%d %d %u %d %lld %u", &seen, &warmup, &n_raw, &scene_pm, &cells, &total) != 6) return 2;
            const int st = mo_status(seen, warmup, n_raw, scene_pm, cells, total);
            printf("%d %d\n", st, mo_next_seen(seen, st));
        } else {
            return 2;
        }
    }
    printf("done %ld\n", n);
    return 0;
}
