// Stand-alone program around csrc/heatmap_stamp.h (plain C++, no HIP): tests/test_heatmap_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers and compares every line with tests/heatmap_ref.py.
// stdin, one case per line:  kind foot_radius cell h w n_classes [class ...] cls x0 y0 x1 y1   (the box as float32 bit patterns, hex;
//                            n_classes -1: no class list)
// stdout, one line per case: "n cx cy cx cy ..." -- the covered cells row by row, found by asking hm_covers about EVERY cell of
//                            the grid; "range" if the stamp's candidate range leaves the grid; "bad" for a configuration outside
//                            its ranges or a non-finite box; then "done N".
#include <cstdio>
#include <cstring>
#include <vector>

#include "heatmap_stamp.h"

using namespace rtmodt;

static float from_bits(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    long n = 0;
    int kind, radius, cell, h, w, nc;
    while (scanf("%d %d %d %d %d %d", &kind, &radius, &cell, &h, &w, &nc) == 6) {
        std::vector<int32_t> classes;
        for (int i = 0; i < nc; ++i) {
            int c;
            if (scanf("%d", &c) != 1) return 2;
            classes.push_back(c);
        }
        int cls;
        unsigned b[4];
        if (scanf("%d %x %x %x %x", &cls, &b[0], &b[1], &b[2], &b[3]) != 5) return 2;
        classes.push_back(0);                               // data() is non-null for an empty list; never read
        const HmStampCfg cfg{kind, radius, cell, nc < 0 ? nullptr : classes.data(), nc < 0 ? 0 : nc};
        const float f[4] = {from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), from_bits(b[3])};
        ++n;
        if (!hm_stamp_cfg_ok(cfg) || h < 1 || w < 1 || h > HM_MAX_DIM || w > HM_MAX_DIM ||
            !(pv_finite(f[0]) && pv_finite(f[1]) && pv_finite(f[2]) && pv_finite(f[3]))) {
            puts("bad");
            continue;
        }
        HmStamp st;
        std::vector<int> cells;
        bool in_range = true;
        if (hm_stamp(cfg, f[0], f[1], f[2], f[3], cls, h, w, st)) {
            const int gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
            in_range = st.cx0 >= 0 && st.cy0 >= 0 && st.cx1 < gw && st.cy1 < gh && st.cx0 <= st.cx1 && st.cy0 <= st.cy1;
            for (int cy = 0; cy < gh; ++cy)
                for (int cx = 0; cx < gw; ++cx)
                    if (hm_covers(st, cell, cx, cy)) {
                        cells.push_back(cx);
                        cells.push_back(cy);
                    }
        }
        if (!in_range) {
            puts("range");
            continue;
        }
        printf("%zu", cells.size() / 2);
        for (int v : cells) printf(" %d", v);
        putchar('\n');
    }
    printf("done %ld\n", n);
    return 0;
}
