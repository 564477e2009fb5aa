// snapshot_rule_check.cpp -- csrc/snapshot_rule.h on its own: a stand-alone program (no HIP, no Python) that tests/test_snapshot_cpu.py
// builds plain and with -fsanitize=address,undefined and compares with tests/snapshot_ref.py line by line.  One case per input line:
//   p th tw margin_pm min_side area_cap h w x0 y0 x1 y1      (the box as float32 bit patterns, hex)   -> the plan, or 0
//   w S D                                                     -> per destination pixel: first source pixel and the weights
//   r th tw margin_pm min_side h w seed x0 y0 x1 y1          -> the whole thumbnail of the box cut from the seeded frame, hex (pad 114)
//   c conf                                                    (float32 bit pattern)                   -> conf_milli
//   s conf_milli area cut occluded best_score min_gain_pm     -> score, replaces
//   o pm ax0 ay0 ax1 ay1 bx0 by0 bx1 by1                      -> occludes
// The frame of an `r` case: byte k of the tight h x w x 3 image is ((k * 2654435761 + seed * 40503) mod 2^32) >> 24.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "snapshot_rule.h"

using namespace rtmodt;

static float from_bits(const std::string &hex) {
    const uint32_t u = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    std::string line;
    long n_lines = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        ++n_lines;
        if (kind == "p" || kind == "r") {
            SnRuleCfg c{};
            int h, w;
            uint32_t seed = 0;
            in >> c.thumb_h >> c.thumb_w >> c.margin_pm >> c.min_side;
            if (kind == "p") in >> c.area_cap; else c.area_cap = 1 << 16;
            in >> h >> w;
            if (kind == "r") in >> seed;
            std::string b[4];
            in >> b[0] >> b[1] >> b[2] >> b[3];
            SnPlan P;
            const bool ok = sn_plan(c, from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), from_bits(b[3]), 0, h, w, P);
            if (!ok) { printf("0\n"); continue; }
            if (kind == "p") {
                printf("1 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", P.raw.x0, P.raw.y0, P.raw.x1, P.raw.y1, P.box.x0, P.box.y0, P.box.x1,
                       P.box.y1, P.crop.x0, P.crop.y0, P.crop.x1, P.crop.y1, P.sw, P.sh, P.dw, P.dh, P.ox, P.oy, P.cut, P.area);
                continue;
            }
            std::vector<uint8_t> frame((size_t)h * w * 3);
            for (size_t k = 0; k < frame.size(); ++k) frame[k] = (uint8_t)(((uint32_t)k * 2654435761u + seed * 40503u) >> 24);
            std::vector<uint8_t> t((size_t)c.thumb_h * c.thumb_w * 3, 114);
            const uint8_t *src = frame.data() + ((size_t)P.crop.y0 * w + P.crop.x0) * 3;
            for (int y = 0; y < P.dh; ++y)
                for (int x = 0; x < P.dw; ++x)
                    for (int ch = 0; ch < 3; ++ch)
                        t[((size_t)(P.oy + y) * c.thumb_w + P.ox + x) * 3 + ch] = sn_pixel(src, (int64_t)w * 3, P.sw, P.sh, P.dw, P.dh, x, y, ch);
            std::string hex(t.size() * 2, '0');
            static const char *digits = "0123456789abcdef";
            for (size_t k = 0; k < t.size(); ++k) { hex[2 * k] = digits[t[k] >> 4]; hex[2 * k + 1] = digits[t[k] & 15]; }
            printf("1 %s\n", hex.c_str());
        } else if (kind == "w") {
            int S, D;
            in >> S >> D;
            for (int j = 0; j < D; ++j) {
                int32_t i0, i1;
                sn_span(S, D, j, i0, i1);
                printf("%s%d", j ? " | " : "", i0);
                for (int i = i0; i <= i1; ++i) printf(" %d", sn_weight(S, D, j, i));
            }
            printf("\n");
        } else if (kind == "c") {
            std::string b;
            in >> b;
            printf("%d\n", sn_conf_milli(from_bits(b)));
        } else if (kind == "s") {
            int cm, area, cut, occl, gain;
            long long best;
            in >> cm >> area >> cut >> occl >> best >> gain;
            const int64_t s = sn_score(cm, area, cut != 0, occl != 0);
            printf("%" PRId64 " %d\n", s, sn_replaces(s, best, gain) ? 1 : 0);
        } else if (kind == "o") {
            int pm;
            PvRect a, b;
            in >> pm >> a.x0 >> a.y0 >> a.x1 >> a.y1 >> b.x0 >> b.y0 >> b.x1 >> b.y1;
            printf("%d\n", sn_occludes(a, b, pm) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown case '%s'\n", kind.c_str());
            return 2;
        }
    }
    printf("done %ld\n", n_lines);
    return 0;
}
