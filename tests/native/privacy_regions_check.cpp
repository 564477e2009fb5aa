// Stand-alone program around csrc/privacy_regions.h (plain C++, no HIP): tests/test_privacy_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers and compares every line with tests/privacy_ref.py.
// stdin, one case per line:  kind head_pm expand_px h w n_classes [class ...] cls x0 y0 x1 y1   (the box as float32 bit patterns, hex;
//                            n_classes -1: no class list)
// stdout, one line per case: "x0 y0 x1 y1" (inclusive) or "none"; "bad" for a configuration outside its ranges or a non-finite box;
//                            then "done N".
#include <cstdio>
#include <cstring>
#include <vector>

#include "privacy_regions.h"

using namespace rtmodt;

static float from_bits(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    long n = 0;
    int kind, head_pm, expand, h, w, nc;
    while (scanf("%d %d %d %d %d %d", &kind, &head_pm, &expand, &h, &w, &nc) == 6) {
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
        const PvRegionCfg cfg{kind, head_pm, expand, nc < 0 ? nullptr : classes.data(), nc < 0 ? 0 : nc};
        const float f[4] = {from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), from_bits(b[3])};
        PvRect r;
        if (!pv_region_cfg_ok(cfg) || !(pv_finite(f[0]) && pv_finite(f[1]) && pv_finite(f[2]) && pv_finite(f[3])))
            puts("bad");
        else if (pv_region(cfg, f[0], f[1], f[2], f[3], cls, h, w, r))
            printf("%d %d %d %d\n", r.x0, r.y0, r.x1, r.y1);
        else
            puts("none");
        ++n;
    }
    printf("done %ld\n", n);
    return 0;
}
