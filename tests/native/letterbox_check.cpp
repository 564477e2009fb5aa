// letterbox_check.cpp -- csrc/letterbox.h on the host (no HIP): reads lines "h w in_h in_w rect" on stdin and prints, per line, what
// the library would use for that frame -- the geometry, the bit pattern of (float)gain, the pads, and both axes' resize tables as
// the one contiguous array the device gets, read back through the ResizeTables view of it.  tests/test_letterbox_cpu.py builds it
// plain and with the address / undefined-behaviour sanitizers and compares every line with oracle/yolo_oracle.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "letterbox.h"

using namespace rtmodt;

static void row(const char *name, const int32_t *p, int n) {
    fputs(name, stdout);
    for (int i = 0; i < n; ++i) printf(" %d", p[i]);
    fputc('\n', stdout);
}

int main() {
    int h, w, in_h, in_w, rect;
    long cases = 0;
    while (scanf("%d %d %d %d %d", &h, &w, &in_h, &in_w, &rect) == 5) {
        const Letterbox lb = letterbox_geometry(h, w, in_h, in_w, rect != 0);
        const LetterboxGeom &g = lb.g;
        const float gain = (float)lb.gain;
        uint32_t bits;
        memcpy(&bits, &gain, 4);
        printf("case %d %d %d %d %d\n", h, w, in_h, in_w, rect);
        printf("geom %d %d %d %d %d %d %d\n", g.src_h, g.src_w, g.new_w, g.new_h, g.top, g.left, g.resize);
        printf("back %08x %d %d\n", bits, lb.pad_x, lb.pad_y);
        const std::vector<int32_t> t = resize_tables(g);
        const ResizeTables v = resize_tables_at(t.data(), g);
        row("xofs", v.xofs, g.new_w); row("xa0", v.xa0, g.new_w); row("xa1", v.xa1, g.new_w);
        row("yofs", v.yofs, g.new_h); row("yb0", v.yb0, g.new_h); row("yb1", v.yb1, g.new_h);
        ++cases;
    }
    printf("done %ld\n", cases);
    return 0;
}
