// slice_grid_check.cpp -- csrc/slice_grid.h and the csrc/letterbox.h it includes on the host (no HIP): the worked grid values,
// coverage and containment over a sweep, the tile-count limit, the resize tables' index bounds (what the overview kernel
// dereferences) and the letterbox geometry of the overview.
// Built plain and with the address / undefined-behaviour sanitizers by tests/test_slice_cpu.py; runs by itself.
#include <cstdio>
#include <vector>

#include "slice_grid.h"

using namespace rtmodt;

static int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            ++failures;                                 \
        }                                               \
    } while (0)

static void worked(int L, int t, int o, std::vector<int> want, int te) {
    SliceAxis a;
    CHECK(slice_axis(L, t, o, &a), "axis %d %d %d refused", L, t, o);
    CHECK(a.te == te && a.pos == want, "axis %d %d %d: te %d, %zu positions", L, t, o, a.te, a.pos.size());
}

int main() {
    worked(1920, 640, 128, {0, 512, 1024, 1280}, 640);
    worked(1080, 640, 128, {0, 440}, 640);
    worked(640, 640, 128, {0}, 640);
    worked(50, 64, 16, {0}, 50);
    printf("ok worked\n");

    long axes = 0;
    for (int L = 1; L <= 300; ++L)
        for (int t = 1; t <= 80; t += (t < 10 ? 1 : 7))
            for (int o = 0; o < t; o += (o < 4 ? 1 : 5)) {
                SliceAxis a;
                CHECK(slice_axis(L, t, o, &a), "axis %d %d %d refused", L, t, o);
                CHECK(a.te == std::min(t, L) && !a.pos.empty() && a.pos[0] == 0, "axis %d %d %d: start", L, t, o);
                std::vector<char> cov((size_t)L, 0);
                for (size_t k = 0; k < a.pos.size(); ++k) {
                    CHECK(a.pos[k] >= 0 && a.pos[k] + a.te <= L, "axis %d %d %d: tile %zu at %d leaves the frame", L, t, o, k, a.pos[k]);
                    CHECK(k == 0 || a.pos[k] > a.pos[k - 1], "axis %d %d %d: positions not ascending", L, t, o);
                    for (int x = a.pos[k]; x < a.pos[k] + a.te && x < L; ++x) cov[(size_t)x] = 1;
                }
                for (int x = 0; x < L; ++x) CHECK(cov[(size_t)x], "axis %d %d %d: pixel %d uncovered", L, t, o, x);
                CHECK(a.pos.back() + a.te == L, "axis %d %d %d: the last tile does not end at L", L, t, o);
                ++axes;
            }
    printf("ok axes %ld\n", axes);

    SliceAxis bad;
    CHECK(!slice_axis(0, 4, 0, &bad) && !slice_axis(4, 0, 0, &bad) && !slice_axis(4, 4, 4, &bad) && !slice_axis(4, 4, -1, &bad), "bad arguments accepted");
    SliceGrid g;
    CHECK(slice_grid(1920, 1080, 640, 640, 128, 128, &g) == 0 && g.tiles() == 8 && g.te_w == 640 && g.te_h == 640, "1080p grid");
    CHECK(g.x[0] == 0 && g.y[0] == 0 && g.x[3] == 1280 && g.y[3] == 0 && g.x[4] == 0 && g.y[4] == 440 && g.x[7] == 1280 && g.y[7] == 440, "row-major order");
    CHECK(slice_grid(512, 512, 64, 64, 0, 0, &g) == 0 && g.tiles() == SLICE_MAX_TILES, "64 tiles");
    CHECK(slice_grid(513, 512, 64, 64, 0, 0, &g) == 2, "65+ tiles accepted");
    CHECK(slice_grid(100, 100, 64, 64, 64, 0, &g) == 1, "overlap == tile accepted");
    printf("ok grid\n");

    long tables = 0;
    for (int src = 1; src <= 200; src += 3)
        for (int dst = 1; dst <= 70; dst += 2) {
            std::vector<int32_t> t((size_t)3 * dst);
            resize_table(dst, src, t.data(), t.data() + dst, t.data() + 2 * dst);
            for (int d = 0; d < dst; ++d) {
                CHECK(t[(size_t)d] >= 0 && t[(size_t)d] <= src - 1, "table %d <- %d: index %d at %d", dst, src, t[(size_t)d], d);
                CHECK(t[(size_t)dst + d] + t[(size_t)2 * dst + d] == 2048, "table %d <- %d: weights at %d", dst, src, d);
            }
            ++tables;
        }
    printf("ok tables %ld\n", tables);

    for (int h = 1; h <= 240; h += 7)
        for (int w = 1; w <= 320; w += 11)
            for (int t : {32, 50, 64}) {
                const int in_w = std::min(t, w), in_h = std::min(t, h);
                const Letterbox lb = letterbox_geometry(h, w, in_h, in_w);
                const LetterboxGeom &g = lb.g;
                CHECK(g.new_w >= 0 && g.new_h >= 0 && g.new_w <= in_w && g.new_h <= in_h, "letterbox %dx%d -> %dx%d: %dx%d", w, h, in_w, in_h, g.new_w, g.new_h);
                CHECK(g.left >= 0 && g.top >= 0 && g.left + g.new_w <= in_w && g.top + g.new_h <= in_h, "letterbox %dx%d -> %dx%d: pads", w, h, in_w, in_h);
                CHECK((float)lb.gain > 0.f, "letterbox gain");
            }
    const Letterbox hd = letterbox_geometry(1080, 1920, 640, 640);
    CHECK(hd.g.new_w == 640 && hd.g.new_h == 360 && hd.g.top == 140 && hd.g.left == 0 && hd.g.resize == 1 && hd.pad_x == 0 && hd.pad_y == 140, "1080p overview");
    printf("ok letterbox\n");

    if (failures) { printf("FAIL %d checks\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
