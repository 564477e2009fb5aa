// Stand-alone program around csrc/compose_rule.h (plain C++, no HIP): tests/test_compose_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers and compares every line with tests/compose_ref.py.  Every array is allocated at exactly its
// documented size.  stdin, one case per line (C = sh sw  crop x y w h  rect x y w h  fit yuv420):
//   p C            -> the plan: "cx cy cw ch  ix iy iw ih  kind_x kind_y"
//   x C seed       -> the plan, then every byte of the inner picture, row-major, of a source whose byte i is
//                     (i * 7919 + seed * 104729 + (i >> 3) * 31) % 251
//   t D S          -> resize_table(D, S): "ofs c0 c1" per destination
//   y b g r        -> "Y U V" of that colour
// then "done N".
#include <cstdio>
#include <vector>

#include "compose_rule.h"

using namespace rtmodt;

static bool read_case(int &sh, int &sw, CpRect &crop, CpRect &rect, int &fit, int &yuv) {
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &sh, &sw, &crop.x, &crop.y, &crop.w, &crop.h, &rect.x, &rect.y, &rect.w, &rect.h, &fit, &yuv) != 12) return false;
    const bool whole = crop.x == 0 && crop.y == 0 && crop.w == 0 && crop.h == 0;
    return sh >= 1 && sw >= 1 && sh <= CP_MAX_DIM && sw <= CP_MAX_DIM && (whole || cp_rect_inside(crop, sh, sw)) && rect.w >= 1 && rect.h >= 1 &&
           rect.w <= CP_MAX_DIM && rect.h <= CP_MAX_DIM && rect.x >= 0 && rect.y >= 0 && fit >= CP_STRETCH && fit <= CP_FILL;
}

static void print_plan(const CpPlan &p) {
    printf("%d %d %d %d %d %d %d %d %d %d", p.crop.x, p.crop.y, p.crop.w, p.crop.h, p.inner.x, p.inner.y, p.inner.w, p.inner.h, p.kind_x, p.kind_y);
}

int main() {
    long n = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n;
        if (op == 'p' || op == 'x') {
            int sh, sw, fit, yuv;
            CpRect crop, rect;
            if (!read_case(sh, sw, crop, rect, fit, yuv)) return 2;
            CpPlan p;
            cp_plan(sh, sw, crop, rect, fit, yuv != 0, p);
            print_plan(p);
            if (op == 'x') {
                long long seed;
                if (scanf("%lld", &seed) != 1 || (long long)sh * sw > 1 << 22) return 2;
                std::vector<uint8_t> src((size_t)sh * sw * 3);
                for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(((long long)i * 7919 + seed * 104729 + ((long long)i >> 3) * 31) % 251);
                std::vector<int32_t> tx(p.kind_x == CP_ENLARGE ? (size_t)3 * p.inner.w : 0), ty(p.kind_y == CP_ENLARGE ? (size_t)3 * p.inner.h : 0);
                if (p.kind_x == CP_ENLARGE) resize_table(p.inner.w, p.crop.w, tx.data(), tx.data() + p.inner.w, tx.data() + 2 * p.inner.w);
                if (p.kind_y == CP_ENLARGE) resize_table(p.inner.h, p.crop.h, ty.data(), ty.data() + p.inner.h, ty.data() + 2 * p.inner.h);
                for (int dy = 0; dy < p.inner.h; ++dy)
                    for (int dx = 0; dx < p.inner.w; ++dx)
                        for (int c = 0; c < 3; ++c) printf(" %d", (int)cp_pixel(src.data(), (int64_t)3 * sw, p, tx.data(), ty.data(), dx, dy, c));
            }
            putchar('\n');
        } else if (op == 't') {
            int D, S;
            if (scanf("%d %d", &D, &S) != 2 || D < 1 || S < 1 || D > CP_MAX_DIM || S > CP_MAX_DIM) return 2;
            std::vector<int32_t> t((size_t)3 * D);
            resize_table(D, S, t.data(), t.data() + D, t.data() + 2 * D);
            for (int d = 0; d < D; ++d) printf("%s%d %d %d", d ? " " : "", t[d], t[D + d], t[2 * D + d]);
            putchar('\n');
        } else if (op == 'y') {
            int b, g, r;
            if (scanf("%d %d %d", &b, &g, &r) != 3) return 2;
            const int m[3] = {cp_block_mean(b, b, b, b), cp_block_mean(g, g, g, g), cp_block_mean(r, r, r, r)};
            printf("%d %d %d\n", cp_yuv_y(b, g, r), cp_yuv_u(m[0], m[1], m[2]), cp_yuv_v(m[0], m[1], m[2]));
        } else return 2;
    }
    printf("done %ld\n", n);
    return 0;
}
