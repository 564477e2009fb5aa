// Stand-alone program around csrc/health_rule.h (plain C++, no HIP): tests/test_health_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers and compares every line with tests/health_ref.py.
// stdin, one case per line:
//   d <the 16 rule fields, edge_threshold .. relearn_frames> cells luma_sum sharp n_dark n_bright n_changed n_edge n_ref_edge n_kept
//     ref_sharp frames_seen active pending run[6] off[6]        one frame through hl_step
//   b ref_sharp frames_seen active pending run[6] off[6]        hl_rebase_now
//   g left right up down                                        hl_coarse
//   r R G learn ref_shift edge_threshold                        hl_learn_r, hl_edge, hl_weak_edge, hl_ref_edge
// stdout, one line per case: "raw learn <state> n (condition kind)*" | "<state>" | "G" | "R edge weak ref_edge", a state being
// "ref_sharp frames_seen active pending run[6] off[6]"; "bad" for a rule, a count or a state outside its range; then "done N".
#include <cinttypes>
#include <cstdio>

#include "health_rule.h"

using namespace rtmodt;

static bool read_state(HlState &s) {
    s.reserved = 0;
    if (scanf("%" SCNu64 " %d %u %u", &s.ref_sharp, &s.frames_seen, &s.active, &s.pending) != 4) return false;
    for (int i = 0; i < HL_CONDITIONS; ++i)
        if (scanf("%d", &s.run[i]) != 1) return false;
    for (int i = 0; i < HL_CONDITIONS; ++i)
        if (scanf("%d", &s.off[i]) != 1) return false;
    return true;
}

static void print_state(const HlState &s) {
    printf("%" PRIu64 " %d %u %u", s.ref_sharp, s.frames_seen, s.active, s.pending);
    for (int i = 0; i < HL_CONDITIONS; ++i) printf(" %d", s.run[i]);
    for (int i = 0; i < HL_CONDITIONS; ++i) printf(" %d", s.off[i]);
}

int main() {
    long n = 0;
    char kind;
    while (scanf(" %c", &kind) == 1) {
        ++n;
        if (kind == 'd') {
            HlRule r;
            HlCounts k;
            HlState s;
            long long cells;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %" SCNu64 " %" SCNu64 " %u %u %u %u %u %u", &r.edge_threshold, &r.ref_shift, &r.warmup,
                      &r.dark_level, &r.dark_pm, &r.bright_level, &r.bright_pm, &r.retain_pm, &r.cover_pm, &r.defocus_pm, &r.min_ref_edges, &r.hold_frames,
                      &r.clear_frames, &r.freeze_frames, &r.freeze_cells, &r.relearn_frames, &cells, &k.luma_sum, &k.sharp, &k.n_dark, &k.n_bright, &k.n_changed,
                      &k.n_edge, &k.n_ref_edge, &k.n_kept) != 25 || !read_state(s))
                return 2;
            if (!hl_rule_ok(r) || !hl_state_ok(s) || cells < 1 || cells > MO_MAX_CELLS || k.sharp >= (1ull << 40)) {
                puts("bad");
                continue;
            }
            HlEvent ev[HL_MAX_EVENTS];
            uint32_t raw = 0;
            int32_t learn = 0;
            const int n_ev = hl_step(r, k, cells, s, ev, &raw, &learn);
            if (n_ev > HL_MAX_EVENTS) return 3;
            printf("%u %d ", raw, learn);
            print_state(s);
            printf(" %d", n_ev);
            for (int i = 0; i < n_ev; ++i) printf(" %d %d", ev[i].condition, ev[i].kind);
            puts("");
        } else if (kind == 'b') {
            HlState s;
            if (!read_state(s)) return 2;
            if (!hl_state_ok(s)) {
                puts("bad");
                continue;
            }
            hl_rebase_now(s);
            print_state(s);
            puts("");
        } else if (kind == 'g') {
            unsigned l, r, u, d;
            if (scanf("%u %u %u %u", &l, &r, &u, &d) != 4) return 2;
            printf("%u\n", hl_coarse(l, r, u, d));
        } else if (kind == 'r') {
            unsigned R, G;
            int learn, shift, thr;
            if (scanf("%u %u %d %d %d", &R, &G, &learn, &shift, &thr) != 5) return 2;
            if (R > 65280u || G > 255u || learn < 0 || learn > 2 || shift < 1 || shift > 12 || thr < 1 || thr > 255) {
                puts("bad");
                continue;
            }
            printf("%u %d %d %d\n", hl_learn_r(R, G, learn, shift), hl_edge(G, thr) ? 1 : 0, hl_weak_edge(G, thr) ? 1 : 0, hl_ref_edge(R, thr) ? 1 : 0);
        } else {
            return 2;
        }
    }
    printf("done %ld\n", n);
    return 0;
}
