// Stand-alone program around csrc/denoise_rule.h (plain C++, no HIP): tests/test_denoise_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers and compares every line with tests/denoise_ref.py.  Every array is allocated at exactly its
// documented size: a frame's last pixel is the buffer's last byte, in the source and in the destination, and the runs are read and
// written as csrc/denoise.hip reads and writes them (three dwords for a full run on the wide path, bytes otherwise).
// stdin, one case per line:
//   F h w pitch base wide lo hi shift spatial thr frames  then frames * h * w * 3 byte values
//       -> per frame one line: the h * w * 3 output bytes, the h * w * 3 acc values, n_static n_moving absdiff_static frames_seen,
//          then "pad" and the count of bytes outside the pixels of the destination that changed (0)
//   a lo hi D seen                      -> a
//   m sum n                             -> (sum + n / 2) / n
// A case outside the rule's ranges prints "bad".  Then "done N".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "denoise_rule.h"

using namespace rtmodt;

template <bool WIDE> static void run_frame(const DnRule &r, const uint8_t *src, uint8_t *dst, long long pitch, int h, int w, int seen, std::vector<uint16_t> &acc) {
    // what the kernel stages: every pixel with its luma, and Y(x) - Y(prev) from the state before the call
    std::vector<uint32_t> px((size_t)h * w);
    std::vector<int32_t> dy((size_t)h * w);
    for (int y = 0; y < h; ++y)
        for (int x0 = 0; x0 < w; x0 += DN_RUN) {
            const int npx = w - x0 < DN_RUN ? w - x0 : DN_RUN;
            uint32_t run[DN_RUN];
            dn_load_run<WIDE>(src + (long long)y * pitch + 3LL * x0, npx, run);
            for (int i = 0; i < npx; ++i) {
                const size_t at = (size_t)y * w + x0 + i;
                const uint32_t yv = dn_luma_of(run[i]);
                px[at] = run[i] | yv << 24;
                dy[at] = (int32_t)yv - (int32_t)dn_luma_of(dn_prev_px(acc[3 * at], acc[3 * at + 1], acc[3 * at + 2]));
            }
        }
    unsigned long long absdiff = 0;
    unsigned n_static = 0, n_moving = 0;
    for (int y = 0; y < h; ++y)
        for (int x0 = 0; x0 < w; x0 += DN_RUN) {
            const int npx = w - x0 < DN_RUN ? w - x0 : DN_RUN;
            uint32_t out[DN_RUN] = {0, 0, 0, 0};
            for (int i = 0; i < npx; ++i) {
                const int x = x0 + i;
                uint32_t nb[9], mine[3], inside = 0;
                int32_t nd[9];
                for (int q = 0; q < 9; ++q) {
                    const int qy = y + q / 3 - 1, qx = x + q % 3 - 1;
                    const int cy = qy < 0 ? 0 : (qy >= h ? h - 1 : qy), cx = qx < 0 ? 0 : (qx >= w ? w - 1 : qx);
                    nb[q] = px[(size_t)cy * w + cx]; nd[q] = dy[(size_t)cy * w + cx];
                    if (cy == qy && cx == qx) inside |= 1u << q;
                }
                const size_t at = ((size_t)y * w + x) * 3;
                for (int k = 0; k < 3; ++k) mine[k] = acc[at + k];
                const DnPixel p = dn_pixel(r, nb, nd, inside, seen, mine);
                for (int k = 0; k < 3; ++k) {
                    if (mine[k] > DN_MAX_ACC) exit(4);      // acc' lies between acc and xs << 8
                    acc[at + k] = (uint16_t)mine[k];
                }
                out[i] = p.out & 0xffffffu;
                if ((p.out >> 24) != dn_luma_of(out[i])) exit(5);
                n_static += p.a == 0; n_moving += p.a == 256;
                if (p.a == 0) absdiff += (unsigned)(nd[4] < 0 ? -nd[4] : nd[4]);
            }
            dn_store_run<WIDE>(dst + (long long)y * pitch + 3LL * x0, npx, out);
        }
    for (int y = 0; y < h; ++y)
        for (int i = 0; i < 3 * w; ++i) printf("%u ", dst[(long long)y * pitch + i]);
    for (size_t i = 0; i < acc.size(); ++i) printf("%u ", acc[i]);
    printf("%u %u %llu %d\n", n_static, n_moving, absdiff, dn_next_seen(seen));
}

int main() {
    long n_cases = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n_cases;
        if (op == 'F') {
            int h, w, wide, frames;
            long long pitch, base;
            DnRule r{};
            if (scanf("%d %d %lld %lld %d %d %d %d %d %d %d", &h, &w, &pitch, &base, &wide, &r.motion_lo, &r.motion_hi, &r.temporal_shift, &r.spatial, &r.spatial_thr,
                      &frames) != 11)
                return 2;
            const bool ok = h >= 1 && w >= 1 && h <= 4096 && w <= 4096 && pitch >= 3LL * w && pitch <= 65536 && base >= 0 && base <= 64 &&
                            !(wide && (pitch % 4 || base % 4)) && dn_rule_ok(r) && frames >= 0 && frames <= 64;
            const size_t bytes = ok ? (size_t)(base + (h - 1) * pitch + 3LL * w) : 0;      // what a frame owns, and not one byte more
            std::vector<uint16_t> acc(ok ? (size_t)h * w * 3 : 0, 0);
            int seen = 0;
            for (int f = 0; f < (frames > 0 ? frames : 0); ++f) {
                std::vector<unsigned> vals((size_t)(h > 0 && w > 0 && h <= 4096 && w <= 4096 ? h * w * 3 : 0));
                for (unsigned &v : vals)
                    if (scanf("%u", &v) != 1 || v > 255) return 2;
                if (!ok) continue;
                uint8_t *src = (uint8_t *)malloc(bytes), *dst = (uint8_t *)malloc(bytes);
                if (!src || !dst) return 3;
                for (size_t i = 0; i < bytes; ++i) src[i] = dst[i] = 0xA5;
                for (int y = 0; y < h; ++y)
                    for (int i = 0; i < 3 * w; ++i) src[base + y * pitch + i] = (uint8_t)vals[(size_t)y * 3 * w + i];
                if (wide) run_frame<true>(r, src + base, dst + base, pitch, h, w, seen, acc);
                else run_frame<false>(r, src + base, dst + base, pitch, h, w, seen, acc);
                seen = dn_next_seen(seen);
                size_t changed = 0;
                for (size_t i = 0; i < bytes; ++i) {
                    const long long rel = (long long)i - base;
                    const bool pixel = rel >= 0 && rel % pitch < 3LL * w;
                    if (!pixel && dst[i] != 0xA5) ++changed;
                }
                printf("pad %zu\n", changed);
                free(src); free(dst);
            }
            if (!ok) puts("bad");
        } else if (op == 'a') {
            DnRule r{0, 1, 0, 0, 0};
            int D, seen;
            if (scanf("%d %d %d %d", &r.motion_lo, &r.motion_hi, &D, &seen) != 4) return 2;
            if (!dn_rule_ok(r) || D < 0 || D > DN_MAX_THRESHOLD || seen < 0 || seen > DN_MAX_SEEN) {
                puts("bad");
                continue;
            }
            printf("%d %d\n", dn_alpha(r, D, seen), dn_next_seen(seen));
        } else if (op == 'm') {
            int sum, n;
            if (scanf("%d %d", &sum, &n) != 2) return 2;
            if (n < 1 || n > 9 || sum < 0 || sum > 255 * n) {
                puts("bad");
                continue;
            }
            printf("%d\n", dn_mean(sum, n));
        } else {
            return 2;
        }
    }
    printf("done %ld\n", n_cases);
    return 0;
}
