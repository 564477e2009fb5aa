// Stand-alone program around csrc/leftobj_rule.h (plain C++, no HIP): tests/test_leftobj_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers and compares every line with tests/leftobj_ref.py.
// stdin, one case per line:
//   c warmup warm_shift learn_shift threshold stable cand_shift occlusion static_frames yc frames_seen bg cand age miss flags
//                                                              one cell through lo_cell / lo_static, packed and unpacked on the way
//   t x0 y0 x1 y1 (floats) rx0 ry0 rx1 ry1 covered_pm margin   a track box against a region's pixel box
//   m ax0 ay0 ax1 ay1 bx0 by0 bx1 by1                          lo_shared_cells of two inclusive cell boxes
//   k cur bgc                                                  lo_kind
//   s frames_seen warmup n_fg scene_pm cells n_regions_total   lo_status and lo_next_seen
//   e idle kind alarmed owner region_kind attended owner_id covered covered_report alarm_frames frame_id first_frame absorb_frames
//                                                              lo_timer and lo_absorbs
// stdout, one line per case: "fg static bg cand age miss flags" | "bx0 by0 bx1 by1 covered attended" or "skip" | "shared" | "kind" |
// "status next" | "fired idle kind alarmed owner absorbs"; "bad" for a rule or a value outside its range; then "done N".
#include <cstdio>

#include "leftobj_rule.h"

using namespace rtmodt;

int main() {
    long n = 0;
    char kind;
    while (scanf(" %c", &kind) == 1) {
        ++n;
        if (kind == 'c') {
            LoRule r;
            unsigned yc;
            int seen;
            LoCell c;
            if (scanf("%d %d %d %d %d %d %d %d %u %d %u %u %u %u %u", &r.warmup, &r.warm_shift, &r.learn_shift, &r.threshold, &r.stable, &r.cand_shift,
                      &r.occlusion, &r.static_frames, &yc, &seen, &c.bg, &c.cand, &c.age, &c.miss, &c.flags) != 15)
                return 2;
            if (!lo_rule_ok(r) || yc > 255 || seen < 0 || seen > MO_MAX_SEEN || c.bg > 65535 || c.cand > 65535 || c.age > 65535 || c.miss > 255 || c.flags > 255) {
                puts("bad");
                continue;
            }
            c = lo_unpack(lo_pack(c));
            const bool fg = lo_cell(r, yc, seen, c);
            c = lo_unpack(lo_pack(c));
            printf("%d %d %u %u %u %u %u\n", fg ? 1 : 0, lo_static(r, c) ? 1 : 0, c.bg, c.cand, c.age, c.miss, c.flags);
        } else if (kind == 't') {
            float b[4];
            int g[4], pm, margin, tb[4];
            if (scanf("%f %f %f %f %d %d %d %d %d %d", &b[0], &b[1], &b[2], &b[3], &g[0], &g[1], &g[2], &g[3], &pm, &margin) != 10) return 2;
            if (!lo_track_box(b[0], b[1], b[2], b[3], tb)) {
                puts("skip");
                continue;
            }
            printf("%d %d %d %d %d %d\n", tb[0], tb[1], tb[2], tb[3], lo_covered(tb, g, pm) ? 1 : 0, lo_attended(tb, g, margin) ? 1 : 0);
        } else if (kind == 'm') {
            int a[4], b[4];
            if (scanf("%d %d %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &b[0], &b[1], &b[2], &b[3]) != 8) return 2;
            printf("%lld\n", (long long)lo_shared_cells(a, b));
        } else if (kind == 'k') {
            unsigned long long cur, bgc;
            if (scanf("%llu %llu", &cur, &bgc) != 2) return 2;
            printf("%d\n", lo_kind(cur, bgc));
        } else if (kind == 's') {
            int seen, warmup, scene_pm;
            unsigned n_fg, total;
            long long cells;
            if (scanf("%d %d %u %d %lld %u", &seen, &warmup, &n_fg, &scene_pm, &cells, &total) != 6) return 2;
            const int st = lo_status(seen, warmup, n_fg, scene_pm, cells, total);
            printf("%d %d\n", st, lo_next_seen(seen, st));
        } else if (kind == 'e') {
            LoTimer t;
            long long owner, owner_id, frame_id, first_frame;
            int region_kind, att, cov, covr, alarm_frames, absorb_frames;
            if (scanf("%d %d %d %lld %d %d %lld %d %d %d %lld %lld %d", &t.idle, &t.kind, &t.alarmed, &owner, &region_kind, &att, &owner_id, &cov, &covr,
                      &alarm_frames, &frame_id, &first_frame, &absorb_frames) != 13)
                return 2;
            t.owner = owner;
            const bool fired = lo_timer(t, region_kind, att != 0, owner_id, cov != 0, covr != 0, alarm_frames);
            printf("%d %d %d %d %lld %d\n", fired ? 1 : 0, t.idle, t.kind, t.alarmed, (long long)t.owner, lo_absorbs(frame_id, first_frame, absorb_frames) ? 1 : 0);
        } else {
            return 2;
        }
    }
    printf("done %ld\n", n);
    return 0;
}
