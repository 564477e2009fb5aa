// Stand-alone program around csrc/stab_rule.h (plain C++, no HIP): tests/test_stab_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers and compares every line with tests/stab_ref.py.  Floating-point values travel as bit patterns (hex),
// so nothing is lost in print.  Every array is allocated at exactly its documented size.
// stdin, one case per line (R = the rule's eight integers: h w leak_shift max_shift_px max_rot_milli max_zoom_milli crop_zoom_milli
// reset_after; J = the four float64 bit patterns of a path):
//   t R J hold n  (valid has_warp w0..w5) x n    float32 bits; has_warp 0: the identity (six dummies follow all the same) -> per call
//                                                "status hold za zb tx ty A B U V" (path as float64 bits), all on one line
//   p R J to_source x y                          float64 bits -> "x y" (float64 bits)
//   s R J border  t ...                          h * w taps (decimal) -> the h * w sampled values of the path's coefficients
// then "done N".
#include <cstdio>
#include <cstring>
#include <vector>

#include "stab_rule.h"

using namespace rtmodt;

static float f32(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static double f64(unsigned long long u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}
static unsigned long long bits64(double d) {
    unsigned long long u;
    memcpy(&u, &d, 8);
    return u;
}

static bool read_rule(StabRule &r, StabPath &j) {
    if (scanf("%d %d %d %d %d %d %d %d", &r.h, &r.w, &r.leak_shift, &r.max_shift_px, &r.max_rot_milli, &r.max_zoom_milli, &r.crop_zoom_milli,
              &r.reset_after) != 8 || !stab_rule_ok(r))
        return false;
    unsigned long long b[4];
    for (int i = 0; i < 4; ++i)
        if (scanf("%llx", &b[i]) != 1) return false;
    j = StabPath{f64(b[0]), f64(b[1]), f64(b[2]), f64(b[3])};
    return true;
}

int main() {
    long n = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n;
        StabRule r;
        StabPath j;
        if (!read_rule(r, j)) return 2;
        if (op == 't') {
            int hold, calls;
            if (scanf("%d %d", &hold, &calls) != 2 || calls < 0) return 2;
            int32_t run = hold;
            for (int k = 0; k < calls; ++k) {
                int valid, has;
                unsigned u[6];
                if (scanf("%d %d %x %x %x %x %x %x", &valid, &has, &u[0], &u[1], &u[2], &u[3], &u[4], &u[5]) != 8) return 2;
                std::vector<float> W(6);
                for (int i = 0; i < 6; ++i) W[i] = f32(u[i]);
                const int status = stab_step(r, j, run, has ? W.data() : nullptr, valid != 0);
                const StabCoef c = stab_quantise(r, j);
                printf("%s%d %d %016llx %016llx %016llx %016llx %lld %lld %lld %lld", k ? "  " : "", status, (int)run, bits64(j.za), bits64(j.zb), bits64(j.tx),
                       bits64(j.ty), (long long)c.A, (long long)c.B, (long long)c.U, (long long)c.V);
            }
            putchar('\n');
        } else if (op == 'p') {
            int to_source;
            unsigned long long a, b;
            if (scanf("%d %llx %llx", &to_source, &a, &b) != 3) return 2;
            double x, y;
            stab_point(r, j, to_source != 0, f64(a), f64(b), x, y);
            printf("%016llx %016llx\n", bits64(x), bits64(y));
        } else if (op == 's') {
            int border;
            if (scanf("%d", &border) != 1 || (long long)r.h * r.w > 1 << 20) return 2;
            std::vector<uint8_t> src((size_t)r.h * r.w);
            for (size_t i = 0; i < src.size(); ++i) {
                int t;
                if (scanf("%d", &t) != 1) return 2;
                src[i] = (uint8_t)t;
            }
            const StabCoef c = stab_quantise(r, j);
            for (int y = 0; y < r.h; ++y)
                for (int x = 0; x < r.w; ++x)
                    printf("%s%d", x || y ? " " : "", stab_sample(c, x, y, r.h, r.w, border, [&](int tx, int ty) { return (int)src[(size_t)ty * r.w + tx]; }));
            putchar('\n');
        } else return 2;
    }
    printf("done %ld\n", n);
    return 0;
}
