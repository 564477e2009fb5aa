// Stand-alone program around csrc/enhance_rule.h (plain C++, no HIP): tests/test_enhance_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers and compares every line with tests/enhance_ref.py.  Every array is allocated at exactly its
// documented size: the histogram walk reads frames whose last byte is the buffer's last byte.
// stdin, one case per line:
//   c clip_q8 n  h0 .. h255             -> "excess curve0 .. curve255"            (the counts must sum to n, 1..2^28)
//   1 clip_q8 bin n                     the same for n pixels in one bin
//   a px t                              -> "b0 .. bt  k0 f0 tile0  k1 f1 tile1 .."  (bounds; per pixel the table entry and its own tile)
//   e s curve seen shift                -> "s lut8 next_seen"
//   i A B C D fx fy                     -> Y1
//   y strength lo hi luma_sum pixels  Y Y1 -> "eff Y2"
//   p colour c Y Y2                     -> the channel
//   h h w pitch base wide ty tx seed    a frame of LCG bytes at `base` of a buffer that ends with the frame's last byte, walked run by
//                                       run as en_hist walks it -> the ty * tx * 256 counts
// A case outside the rule's ranges prints "bad".  Then "done N".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "enhance_rule.h"

using namespace rtmodt;

static void print_curve(const std::vector<uint32_t> &hist, uint32_t n, int clip_q8) {
    std::vector<uint32_t> curve(EN_LEVELS);
    const uint32_t ex = en_curve_of(hist.data(), n, clip_q8, curve.data());
    printf("%u", ex);
    for (int i = 0; i < EN_LEVELS; ++i) printf(" %u", curve[i]);
    putchar('\n');
}

template <bool WIDE> static void walk(const uint8_t *frame, long long pitch, int h, int w, int ty, int tx, std::vector<uint32_t> &hist) {
    std::vector<int32_t> bx(tx + 1);
    for (int k = 0; k <= tx; ++k) bx[k] = en_bound(k, w, tx);
    const int runs = (w + 3) / 4;
    for (int y = 0; y < h; ++y) {
        const int ky = en_tile_of(y, h, ty);
        uint32_t *row = hist.data() + (size_t)ky * tx * EN_LEVELS;
        for (int lane = 0; lane < 64; ++lane) {              // a lane walks every 64th run with a k of its own, as a wave does
            int32_t k = 0;
            for (int r = lane; r < runs; r += 64) {
                const int x0 = 4 * r, npx = w - x0 < 4 ? w - x0 : 4;
                en_hist_run<WIDE>(frame + (long long)y * pitch + 3LL * x0, pitch, x0, npx, bx.data(), k, [&](uint32_t at, uint32_t cnt) { row[at] += cnt; });
            }
        }
    }
}

int main() {
    long n_cases = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n_cases;
        if (op == 'c' || op == '1') {
            int clip_q8;
            long long n;
            if (scanf("%d", &clip_q8) != 1) return 2;
            std::vector<uint32_t> hist(EN_LEVELS, 0);
            unsigned long long sum = 0;
            if (op == '1') {
                int bin;
                if (scanf("%d %lld", &bin, &n) != 2 || bin < 0 || bin > 255) return 2;
                if (n >= 0 && n <= (long long)EN_MAX_AREA) hist[bin] = (uint32_t)n;
                sum = hist[bin];
            } else {
                if (scanf("%lld", &n) != 1) return 2;
                for (int i = 0; i < EN_LEVELS; ++i) {
                    if (scanf("%u", &hist[i]) != 1) return 2;
                    sum += hist[i];
                }
            }
            if (n < 1 || n > (long long)EN_MAX_AREA || clip_q8 < 0 || clip_q8 > EN_MAX_CLIP_Q8 || sum != (unsigned long long)n) {
                puts("bad");
                continue;
            }
            print_curve(hist, (uint32_t)n, clip_q8);
        } else if (op == 'a') {
            int px, t;
            if (scanf("%d %d", &px, &t) != 2) return 2;
            if (px < 1 || px > EN_MAX_DIM || !en_tiles_ok(t, px)) {
                puts("bad");
                continue;
            }
            for (int k = 0; k <= t; ++k) printf("%s%d", k ? " " : "", en_bound(k, px, t));
            for (int x = 0; x < px; ++x) {
                int32_t k, f;
                en_axis(x, px, t, k, f);
                const uint32_t e = en_axis_pack(k, f);
                printf(" %u %u %d", e >> 9, e & 511u, en_tile_of(x, px, t));
            }
            putchar('\n');
        } else if (op == 'e') {
            unsigned s, curve;
            int seen, shift;
            if (scanf("%u %u %d %d", &s, &curve, &seen, &shift) != 4) return 2;
            if (s > EN_MAX_S || curve > 255 || seen < 0 || seen > EN_MAX_SEEN || shift < 0 || shift > EN_MAX_SHIFT) {
                puts("bad");
                continue;
            }
            const uint32_t v = en_ema(s, curve, seen, shift);
            printf("%u %u %d\n", v, en_lut8(v), en_next_seen(seen));
        } else if (op == 'i') {
            unsigned v[6];
            if (scanf("%u %u %u %u %u %u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 6) return 2;
            if (v[0] > 255 || v[1] > 255 || v[2] > 255 || v[3] > 255 || v[4] > 256 || v[5] > 256) {
                puts("bad");
                continue;
            }
            printf("%u\n", en_interp(v[0], v[1], v[2], v[3], v[4], v[5]));
        } else if (op == 'y') {
            EnRule r{};
            unsigned long long luma, pixels;
            int y, y1;
            if (scanf("%d %d %d %llu %llu %d %d", &r.strength, &r.auto_lo, &r.auto_hi, &luma, &pixels, &y, &y1) != 7) return 2;
            if (!en_rule_ok(r) || pixels < 1 || luma > 255 * pixels || y < 0 || y > 255 || y1 < 0 || y1 > 255) {
                puts("bad");
                continue;
            }
            const uint32_t eff = en_eff(r, luma, pixels);
            printf("%u %d\n", eff, en_y2(y, y1, (int)eff));
        } else if (op == 'p') {
            int colour, c, y, y2;
            if (scanf("%d %d %d %d", &colour, &c, &y, &y2) != 4) return 2;
            if ((colour != EN_SHIFT && colour != EN_GAIN) || c < 0 || c > 255 || y < 0 || y > 255 || y2 < 0 || y2 > 255) {
                puts("bad");
                continue;
            }
            printf("%u\n", en_channel(colour, c, y, y2));
        } else if (op == 'h') {
            int h, w, wide, ty, tx;
            long long pitch, base;
            unsigned seed;
            if (scanf("%d %d %lld %lld %d %d %d %u", &h, &w, &pitch, &base, &wide, &ty, &tx, &seed) != 8) return 2;
            // the host takes the dword path only when every base and the pitch are multiples of 4
            if (h < 1 || w < 1 || h > 4096 || w > 4096 || pitch < 3LL * w || pitch > 65536 || base < 0 || base > 64 || (wide && (pitch % 4 || base % 4)) ||
                !en_tiles_ok(ty, h) || !en_tiles_ok(tx, w)) {
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
            std::vector<uint32_t> hist((size_t)ty * tx * EN_LEVELS, 0);
            if (wide) walk<true>(buf + base, pitch, h, w, ty, tx, hist);
            else walk<false>(buf + base, pitch, h, w, ty, tx, hist);
            free(buf);
            for (size_t i = 0; i < hist.size(); ++i) printf("%s%u", i ? " " : "", hist[i]);
            putchar('\n');
        } else {
            return 2;
        }
    }
    printf("done %ld\n", n_cases);
    return 0;
}
