// Stand-alone program around csrc/colour_rule.h (plain C++, no HIP): tests/test_colour_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers and compares every line with tests/colour_ref.py.  Every array is allocated at exactly its
// documented size: the sample walk reads frames whose last byte is the buffer's last byte.
// stdin, one case per line (every cfg field not named is the default):
//   n b g r                                           -> the name
//   p x0 y0 x1 y1 h w inset top split bottom max_side -> "1 raw[4] box[4] rect[4] ys sx sy nx ny", or "0" (no row)
//   l v0 .. v23                                       -> the three labels, 5 numbers each
//   a min_samples r0 .. r23 f0 .. f23                 -> "added r0 .. r23"
//   w h w pitch base seed max_side skip inset top bottom n  then n x (id x0 y0 x1 y1)
//                                                     a frame of LCG bytes at `base` of a buffer that ends with the frame's last
//                                                     byte; the list walked entry by entry as cl_sample walks it
//                                                     -> per entry "| flags h0 .. h23", or "| x" (no row)
// A case outside the rule's ranges prints "bad".  Then "done N".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "colour_rule.h"

using namespace rtmodt;

static ClRuleCfg defaults() {
    ClRuleCfg c{};
    c.black_max = 48; c.chroma_min = 20; c.sat_split = 96; c.sat_hi_pm = 180; c.sat_lo_pm = 400; c.y_black = 64; c.y_white = 176;
    const int32_t hue[CL_HUE_BOUNDS] = {64, 192, 299, 725, 853, 1109, 1344, 1472};
    for (int k = 0; k < CL_HUE_BOUNDS; ++k) c.hue[k] = hue[k];
    c.pink_mx = 192; c.red_brown_mx = 96; c.orange_brown_mx = 176; c.yellow_brown_mx = 128;
    c.inset_x_pm = 200; c.top_pm = 150; c.split_pm = 500; c.bottom_pm = 900; c.max_side = 48; c.skip_occluded = 1; c.min_samples = 16;
    c.classes = nullptr; c.n_classes = 0;
    return c;
}

static void print_rect(const PvRect &r) { printf(" %d %d %d %d", r.x0, r.y0, r.x1, r.y1); }

int main() {
    long n_cases = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n_cases;
        ClRuleCfg c = defaults();
        if (op == 'n') {
            int b, g, r;
            if (scanf("%d %d %d", &b, &g, &r) != 3) return 2;
            if (b < 0 || b > 255 || g < 0 || g > 255 || r < 0 || r > 255) { puts("bad"); continue; }
            printf("%d\n", cl_name(c, (uint32_t)b, (uint32_t)g, (uint32_t)r));
        } else if (op == 'p') {
            float x0, y0, x1, y1;
            int h, w;
            if (scanf("%f %f %f %f %d %d %d %d %d %d %d", &x0, &y0, &x1, &y1, &h, &w, &c.inset_x_pm, &c.top_pm, &c.split_pm, &c.bottom_pm, &c.max_side) != 11) return 2;
            if (!cl_rule_cfg_ok(c) || h < 1 || w < 1 || h > CL_MAX_DIM || w > CL_MAX_DIM) { puts("bad"); continue; }
            ClPlan P;
            if (!cl_plan(c, x0, y0, x1, y1, 0, h, w, P)) { puts("0"); continue; }
            printf("1");
            print_rect(P.raw); print_rect(P.box); print_rect(P.rect);
            printf(" %d %d %d %d %d\n", P.ys, P.sx, P.sy, P.nx, P.ny);
        } else if (op == 'l') {
            std::vector<uint32_t> v(CL_BINS);
            for (int k = 0; k < CL_BINS; ++k)
                if (scanf("%u", &v[k]) != 1) return 2;
            for (int p = 0; p < 3; ++p) {
                const ClLabel L = cl_label(v.data(), p);
                printf("%s%d %d %d %d %d", p ? " " : "", L.name, L.share_pm, L.second, L.second_pm, L.samples);
            }
            putchar('\n');
        } else if (op == 'a') {
            int min_samples;
            std::vector<uint32_t> row(CL_BINS), fr(CL_BINS);
            if (scanf("%d", &min_samples) != 1) return 2;
            for (int k = 0; k < CL_BINS; ++k)
                if (scanf("%u", &row[k]) != 1) return 2;
            for (int k = 0; k < CL_BINS; ++k)
                if (scanf("%u", &fr[k]) != 1) return 2;
            if (min_samples < 0) { puts("bad"); continue; }
            printf("%d", cl_accumulate(row.data(), fr.data(), min_samples) ? 1 : 0);
            for (int k = 0; k < CL_BINS; ++k) printf(" %u", row[k]);
            putchar('\n');
        } else if (op == 'w') {
            int h, w, base, n;
            long long pitch;
            unsigned seed;
            if (scanf("%d %d %lld %d %u %d %d %d %d %d %d", &h, &w, &pitch, &base, &seed, &c.max_side, &c.skip_occluded, &c.inset_x_pm, &c.top_pm, &c.bottom_pm, &n) != 11)
                return 2;
            if (n < 0 || n > 4096) return 2;
            std::vector<long long> ids(n);
            std::vector<float> box(4 * (size_t)n);
            for (int i = 0; i < n; ++i)
                if (scanf("%lld %f %f %f %f", &ids[i], &box[4 * i], &box[4 * i + 1], &box[4 * i + 2], &box[4 * i + 3]) != 5) return 2;
            if (!cl_rule_cfg_ok(c) || h < 1 || w < 1 || pitch < 3LL * w || base < 0) { puts("bad"); continue; }
            std::vector<uint8_t> buf((size_t)base + (size_t)(h - 1) * pitch + 3 * (size_t)w);      // not one byte more
            uint32_t x = seed;
            for (uint8_t &b : buf) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
            const uint8_t *frame = buf.data() + base;
            std::vector<ClPlan> plans(n);
            std::vector<char> ok(n);
            for (int i = 0; i < n; ++i) ok[i] = cl_plan(c, box[4 * i], box[4 * i + 1], box[4 * i + 2], box[4 * i + 3], 0, h, w, plans[i]);
            for (int e = 0; e < n; ++e) {
                if (!ok[e]) { printf("%s| x", e ? " " : ""); continue; }
                const ClPlan &P = plans[e];
                PvRect occ[CL_MAX_OCCLUDERS];
                int n_occ = 0;
                if (c.skip_occluded && !cl_empty(P.rect))
                    for (int k = 0; k < n; ++k)
                        if (k != e && ok[k] && cl_occludes(P, ids[e], plans[k].raw, plans[k].box, ids[k])) {
                            if (n_occ < CL_MAX_OCCLUDERS) occ[n_occ] = plans[k].box;
                            ++n_occ;
                        }
                const int used = n_occ < CL_MAX_OCCLUDERS ? n_occ : CL_MAX_OCCLUDERS;
                uint32_t hist[CL_BINS] = {};
                for (int s = 0; s < P.nx * P.ny; ++s) {
                    const int j = s / P.nx, i = s - j * P.nx;
                    const int px = P.rect.x0 + i * P.sx, py = P.rect.y0 + j * P.sy;
                    bool hidden = false;
                    for (int o = 0; o < used; ++o) hidden = hidden || cl_inside(occ[o], px, py);
                    if (hidden) continue;
                    const uint8_t *q = frame + (size_t)py * (size_t)pitch + (size_t)3 * px;
                    ++hist[cl_part(P, py) * CL_NAMES + cl_name(c, q[0], q[1], q[2])];
                }
                printf("%s| %d", e ? " " : "", n_occ > CL_MAX_OCCLUDERS ? CL_F_MANY_OCCLUDERS : 0);
                for (int k = 0; k < CL_BINS; ++k) printf(" %u", hist[k]);
            }
            putchar('\n');
        } else return 2;
    }
    printf("done %ld\n", n_cases);
    return 0;
}
