// Stand-alone program around csrc/lens_model.h (plain C++, no HIP): tests/test_lens_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers and compares every line with tests/lens_ref.py.  Floating-point values travel as bit patterns (hex),
// so nothing is lost in print.  Every array is allocated at exactly its documented size.
// stdin, one case per line (L = the 17 float64 bit patterns of a lens: fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 nfx nfy ncx ncy r2_limit):
//   m sh sw oh ow L             -> "n_outside  qx qy outside ..." for every output pixel, row-major
//   c sh sw oh ow  x y ...      float32 bits x 2 per output pixel (a caller's map) -> the same
//   d L x y                     float64 bits -> distort: "x y" (float64 bits)
//   u L x y                     float64 bits -> undistort: "x y residual" (float64 bits)
//   s sh sw border n  t ...  qx qy ...    sh * sw taps (decimal), then n table entries -> n sampled values
// then "done N".
#include <cstdio>
#include <cstring>
#include <vector>

#include "lens_model.h"

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

static bool read_lens(LensModel &m) {
    unsigned long long b[17];
    for (int i = 0; i < 17; ++i)
        if (scanf("%llx", &b[i]) != 1) return false;
    m.fx = f64(b[0]); m.fy = f64(b[1]); m.cx = f64(b[2]); m.cy = f64(b[3]);
    for (int i = 0; i < 8; ++i) m.k[i] = f64(b[4 + i]);
    m.nfx = f64(b[12]); m.nfy = f64(b[13]); m.ncx = f64(b[14]); m.ncy = f64(b[15]); m.r2_limit = f64(b[16]);
    return true;
}

static void print_table(long long n_out, const std::vector<int32_t> &qx, const std::vector<int32_t> &qy, const std::vector<uint8_t> &o) {
    printf("%lld ", n_out);
    for (size_t i = 0; i < qx.size(); ++i) printf(" %d %d %d", qx[i], qy[i], (int)o[i]);
    putchar('\n');
}

int main() {
    long n = 0;
    char op;
    while (scanf(" %c", &op) == 1) {
        ++n;
        if (op == 'm' || op == 'c') {
            int sh, sw, oh, ow;
            if (scanf("%d %d %d %d", &sh, &sw, &oh, &ow) != 4 || oh < 1 || ow < 1 || oh > LENS_MAX_DIM || ow > LENS_MAX_DIM) return 2;
            const size_t cnt = (size_t)oh * ow;
            std::vector<int32_t> qx(cnt), qy(cnt);
            std::vector<uint8_t> o(cnt);
            long long n_out;
            if (op == 'm') {
                LensModel m;
                if (!read_lens(m)) return 2;
                n_out = lens_build_model(m, sh, sw, oh, ow, qx.data(), qy.data(), o.data());
            } else {
                std::vector<float> mx(cnt), my(cnt);
                for (size_t i = 0; i < cnt; ++i) {
                    unsigned a, b;
                    if (scanf("%x %x", &a, &b) != 2) return 2;
                    mx[i] = f32(a); my[i] = f32(b);
                }
                n_out = lens_build_from_map(mx.data(), my.data(), sh, sw, oh, ow, qx.data(), qy.data(), o.data());
            }
            print_table(n_out, qx, qy, o);
        } else if (op == 'd' || op == 'u') {
            LensModel m;
            unsigned long long a, b;
            if (!read_lens(m) || scanf("%llx %llx", &a, &b) != 2) return 2;
            double x, y, r = 0.0;
            if (op == 'd') {
                lens_distort_point(m, f64(a), f64(b), x, y);
                printf("%016llx %016llx\n", bits64(x), bits64(y));
            } else {
                lens_undistort_point(m, f64(a), f64(b), x, y, r);
                printf("%016llx %016llx %016llx\n", bits64(x), bits64(y), bits64(r));
            }
        } else if (op == 's') {
            int sh, sw, border, cnt;
            if (scanf("%d %d %d %d", &sh, &sw, &border, &cnt) != 4 || sh < 1 || sw < 1 || cnt < 0 || (long long)sh * sw > 1 << 20) return 2;
            std::vector<uint8_t> src((size_t)sh * sw);
            for (size_t i = 0; i < src.size(); ++i) {
                int t;
                if (scanf("%d", &t) != 1) return 2;
                src[i] = (uint8_t)t;
            }
            for (int i = 0; i < cnt; ++i) {
                int qx, qy;
                if (scanf("%d %d", &qx, &qy) != 2) return 2;
                printf("%s%d", i ? " " : "", lens_sample(qx, qy, sh, sw, border, [&](int x, int y) { return (int)src[(size_t)y * sw + x]; }));
            }
            putchar('\n');
        } else return 2;
    }
    printf("done %ld\n", n);
    return 0;
}
