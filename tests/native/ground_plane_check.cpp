// Stand-alone program around csrc/ground_plane.h (plain C++, no HIP): tests/test_speed_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers and compares every line with tests/speed_ref.py.  Floating-point values travel as bit
// patterns (hex), so nothing is lost in print.
// stdin, one case per line:
//   a kind x1 y1 x2 y2          float32 bits    -> "u v" (float32 bits) or "none"
//   p H0 .. H8 u v              float64 bits x 9, float32 bits x 2   -> "X Y" or "off"
//   q n                         decimal int64   -> isqrt
//   s d dt                      decimal int64   -> speed in mm/s
//   f normalise n  u v x y ...  float64 bits x 4 n   -> "H0 .. H8 residual" (float64 bits) or "bad"
// then "done N".
#include <cstdio>
#include <cstring>
#include <vector>

#include "ground_plane.h"

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
static unsigned bits32(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

int main() {
    long n = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n;
        if (op == 'a') {
            int kind;
            unsigned b[4];
            if (scanf("%d %x %x %x %x", &kind, &b[0], &b[1], &b[2], &b[3]) != 5) return 2;
            float u, v;
            if (gp_anchor(kind, f32(b[0]), f32(b[1]), f32(b[2]), f32(b[3]), u, v)) printf("%08x %08x\n", bits32(u), bits32(v));
            else puts("none");
        } else if (op == 'p') {
            unsigned long long h[9];
            unsigned uv[2];
            for (int i = 0; i < 9; ++i)
                if (scanf("%llx", &h[i]) != 1) return 2;
            if (scanf("%x %x", &uv[0], &uv[1]) != 2) return 2;
            double H[9];
            for (int i = 0; i < 9; ++i) H[i] = f64(h[i]);
            int32_t X, Y;
            if (gp_project(H, f32(uv[0]), f32(uv[1]), X, Y)) printf("%d %d\n", X, Y);
            else puts("off");
        } else if (op == 'q') {
            long long v;
            if (scanf("%lld", &v) != 1) return 2;
            printf("%lld\n", (long long)gp_isqrt(v));
        } else if (op == 's') {
            long long d, dt;
            if (scanf("%lld %lld", &d, &dt) != 2) return 2;
            printf("%d\n", gp_speed(d, dt));
        } else if (op == 'f') {
            int normalise, cnt;
            if (scanf("%d %d", &normalise, &cnt) != 2 || cnt < 0 || cnt > 4096) return 2;
            std::vector<double> img(2 * cnt + 1), world(2 * cnt + 1);
            for (int i = 0; i < cnt; ++i) {
                unsigned long long q[4];
                if (scanf("%llx %llx %llx %llx", &q[0], &q[1], &q[2], &q[3]) != 4) return 2;
                img[2 * i] = f64(q[0]); img[2 * i + 1] = f64(q[1]); world[2 * i] = f64(q[2]); world[2 * i + 1] = f64(q[3]);
            }
            double H[9], res = 0.0;
            if (gp_fit_plane(img.data(), world.data(), cnt, H, &res, normalise != 0)) {
                for (int i = 0; i < 9; ++i) printf("%016llx ", bits64(H[i]));
                printf("%016llx\n", bits64(res));
            } else puts("bad");
        } else return 2;
    }
    printf("done %ld\n", n);
    return 0;
}
