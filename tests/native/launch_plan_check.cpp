// launch_plan_check.cpp -- csrc/launch_plan.h on the host, by itself (tests/test_launch_plan_cpu.py builds it plain and with the address /
// undefined-behaviour sanitizers).  argv[1] = profiles/bench_tune_cache.txt.
//   round trip     every record of the committed cache decodes to a Choice and encodes to the same three integers
//   literals       the record table of launch_plan.h, code by code; codes a kind never writes are a miss
//   mark_skips     whole skip vectors of hand-built op lists
//   apply_hooks    every hook at 0 and at 1 over every starting form; the legality guards; no hooks = identity
//   finish_plan    the records are formed BEFORE the hooks are applied
//   for_each_view  the number of views visited per op kind
// Toy ops only: PlanOp plus the member names for_each_view looks for.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "launch_plan.h"

using namespace rtmodt;

static int failures = 0;
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            ++failures; printf("FAIL " __VA_ARGS__); printf("\n"); \
        }                                                        \
    } while (0)

static bool same(const TuneRec &a, const TuneRec &b) { return a.t0 == b.t0 && a.t1 == b.t1 && a.fused == b.fused; }
static bool same(const Choice &a, const Choice &b) {
    return a.tile == b.tile && a.tile2 == b.tile2 && a.tail_tile == b.tail_tile && a.form == b.form && a.tail_timed == b.tail_timed;
}

// ---- round trip over the committed cache
static bool kind_of_key(const std::string &key, OpKind &kind) {
    if (key.rfind("front|", 0) == 0) { kind = OP_STEM; return true; }
    const size_t n = key.rfind("|n");
    if (n == std::string::npos) return false;
    const int members = atoi(key.c_str() + n + 2);
    if (key.find("_(cv1+cv2)") != std::string::npos && members == 2) kind = OP_BNECK;
    else kind = members == 1 ? OP_CONV : OP_GROUP;
    return true;
}
static void check_round_trip(const char *path) {
    std::ifstream f(path);
    std::string line;
    EXPECT(std::getline(f, line) && line.rfind("#rtmodt-tune ", 0) == 0, "%s: no header line", path);
    int records = 0, checked = 0, per_kind[6] = {};
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        ++records;
        std::istringstream in(line);
        std::string key;
        TuneRec r;
        OpKind kind;
        if (!(in >> key >> r.t0 >> r.t1 >> r.fused) || !kind_of_key(key, kind)) { EXPECT(false, "unreadable record: %s", line.c_str()); continue; }
        Choice c;
        if (!decode_choice(kind, r, c)) { EXPECT(false, "a miss: %s", line.c_str()); continue; }
        const TuneRec back = encode_choice(kind, c);
        EXPECT(same(back, r), "%s: %d %d %d came back as %d %d %d", key.c_str(), r.t0, r.t1, r.fused, back.t0, back.t1, back.fused);
        ++checked; ++per_kind[kind];
    }
    EXPECT(records > 0 && checked == records, "%d of %d records checked", checked, records);
    printf("ok round trip %d of %d records (conv %d, group %d, bottleneck %d, front %d)\n", checked, records, per_kind[OP_CONV], per_kind[OP_GROUP],
           per_kind[OP_BNECK], per_kind[OP_STEM]);
}

// ---- literals
static void check_literals() {
    const Form want[5] = {FORM_TWO_LAUNCHES, FORM_FUSED, FORM_FUSED_TAIL_P32, FORM_FUSED, FORM_FUSED_TAIL};
    const bool timed[5] = {false, false, true, true, true};
    for (int code = 0; code <= 4; ++code) {
        Choice c;
        EXPECT(decode_choice(OP_BNECK, TuneRec{21, 23, code}, c), "bottleneck code %d is a miss", code);
        EXPECT(c.form == want[code] && c.tile == 21 && c.tile2 == 23, "bottleneck code %d: form %d tiles %d %d", code, (int)c.form, c.tile, c.tile2);
        if (code) EXPECT(c.tail_timed == timed[code], "bottleneck code %d: tail_timed %d", code, (int)c.tail_timed);
        EXPECT(same(encode_choice(OP_BNECK, c), TuneRec{21, 23, code}), "bottleneck code %d does not come back", code);
    }
    Choice c;
    c.tail_tile = 11;                                      // the build-time default survives a record that has not timed the tail
    EXPECT(decode_choice(OP_CONV, TuneRec{6, 0, 0}, c) && !c.tail_timed && c.form == FORM_PLAIN && c.tile == 6 && c.tail_tile == 11, "conv 6 0 0: not 'not yet timed'");
    EXPECT(decode_choice(OP_CONV, TuneRec{6, 12, 0}, c) && c.tail_timed && c.form == FORM_PLAIN && c.tail_tile == 12, "conv 6 12 0: not 'timed, rejected'");
    EXPECT(decode_choice(OP_CONV, TuneRec{1, 11, 1}, c) && c.tail_timed && c.form == FORM_WITH_TAIL && c.tail_tile == 11 && c.tile == 1, "conv 1 11 1: not 'with tail'");
    EXPECT(decode_choice(OP_GROUP, TuneRec{20, 0, 0}, c) && c.tile == 20, "group 20 0 0");
    EXPECT(decode_choice(OP_STEM, TuneRec{0, 0, 1}, c) && c.form == FORM_FRONT_END, "front 0 0 1");
    EXPECT(decode_choice(OP_STEM, TuneRec{0, 0, 0}, c) && c.form == FORM_PLAIN, "front 0 0 0");
    const Choice before = c;
    for (int bad : {-1, 5, 7}) EXPECT(!decode_choice(OP_BNECK, TuneRec{6, 6, bad}, c), "bottleneck code %d is not a miss", bad);
    for (int bad : {-1, 2}) EXPECT(!decode_choice(OP_CONV, TuneRec{6, 12, bad}, c) && !decode_choice(OP_STEM, TuneRec{0, 0, bad}, c), "conv / front code %d is not a miss", bad);
    EXPECT(!decode_choice(OP_GROUP, TuneRec{6, 0, 1}, c), "group code 1 is not a miss");
    EXPECT(!decode_choice(OP_POOL, TuneRec{}, c) && !decode_choice(OP_UP, TuneRec{}, c), "a pool / upsample record is not a miss");
    EXPECT(same(c, before), "a miss changed the choice");
    printf("ok literals\n");
}

// ---- hand-built op lists
static PlanOp mk(OpKind kind, Form form = FORM_PLAIN, bool has_tail = false) {
    PlanOp op;
    op.kind = kind; op.choice.form = form; op.has_tail = has_tail;
    op.skip = true;                                        // stale on purpose: mark_skips must write every entry
    return op;
}
static std::vector<bool> skips(std::vector<PlanOp> ops) {
    mark_skips(ops);
    std::vector<bool> s;
    for (auto &op : ops) s.push_back(op.skip);
    return s;
}
// stem, layer 1, 2.cv1, 2.m.0, 2.cv2, 3, 4.cv1, pool, 22.stage2
static std::vector<PlanOp> net(Form stem, Form l1, Form bneck, bool bneck_has_tail, Form l3, bool head_final) {
    std::vector<PlanOp> ops = {mk(OP_STEM, stem), mk(OP_CONV, l1, true), mk(OP_CONV), mk(OP_BNECK, bneck, bneck_has_tail), mk(OP_CONV),
                               mk(OP_CONV, l3, true), mk(OP_CONV), mk(OP_POOL), mk(OP_GROUP)};
    ops[0].front_ok = true;
    ops[8].head_final = head_final;
    return ops;
}
static void check_skips() {
    typedef std::vector<bool> V;
    const bool T = true, F = false;
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_FUSED, true, FORM_PLAIN, false)) == (V{F, F, F, F, F, F, F, F, F}), "nothing fused: something is skipped");
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_FUSED, true, FORM_WITH_TAIL, false)) == (V{F, F, F, F, F, F, T, F, F}), "conv tail on: 4.cv1 alone is skipped");
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_FUSED_TAIL_P32, true, FORM_PLAIN, false)) == (V{F, F, F, F, T, F, F, F, F}), "fused bottleneck with the tail (persistent32)");
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_FUSED_TAIL, true, FORM_PLAIN, false)) == (V{F, F, F, F, T, F, F, F, F}), "fused bottleneck with the tail");
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_TWO_LAUNCHES, true, FORM_PLAIN, false)) == (V{F, F, F, F, F, F, F, F, F}), "two launches that could carry the tail: cv2 must run");
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_FUSED_TAIL, false, FORM_PLAIN, false)) == (V{F, F, F, F, F, F, F, F, F}), "a tail form without the capability: cv2 must run");
    EXPECT(skips(net(FORM_FRONT_END, FORM_PLAIN, FORM_FUSED, true, FORM_PLAIN, false)) == (V{F, T, T, F, F, F, F, F, F}), "front end on");
    EXPECT(skips(net(FORM_FRONT_END, FORM_WITH_TAIL, FORM_FUSED, true, FORM_PLAIN, false)) == (V{F, T, T, F, F, F, F, F, F}), "front end on, layer 1's tail on");
    EXPECT(skips(net(FORM_PLAIN, FORM_WITH_TAIL, FORM_FUSED, true, FORM_PLAIN, false)) == (V{F, F, T, F, F, F, F, F, F}), "front end off, layer 1's tail on: 2.cv1 skipped, layer 1 not");
    EXPECT(skips(net(FORM_PLAIN, FORM_PLAIN, FORM_FUSED, true, FORM_PLAIN, true)) == (V{F, F, F, F, F, F, F, F, T}), "head_final");
    {
        auto ops = net(FORM_FRONT_END, FORM_PLAIN, FORM_FUSED, true, FORM_PLAIN, false);
        ops[0].front_ok = false;
        EXPECT(skips(ops) == (V{F, F, F, F, F, F, F, F, F}), "a front-end form where the graph does not allow it");
    }
    EXPECT(skips({mk(OP_STEM, FORM_FRONT_END)}).size() == 1 && skips({}).empty(), "short lists");
    printf("ok mark_skips\n");
}

// tail tiles as engine.hip's tail_tile_legal sees them for a 32 -> 64 conv: 11 (BN 64) fits, 12 (BN 128) does not
static bool tail_legal(const PlanOp &, int tile) { return tile == 11; }

static Form hooked(OpKind kind, Form start, const Hooks &h, bool has_tail = true, int tail_tile = 11) {
    std::vector<PlanOp> ops = {mk(kind, start, has_tail)};
    ops[0].front_ok = kind == OP_STEM;
    ops[0].choice.tail_tile = tail_tile;
    apply_hooks(ops, h, tail_legal);
    return ops[0].choice.form;
}
static Hooks hooks(int bneck, int bneck32, int bneck_tail, int tail, int front) {
    Hooks h;
    h.bneck = bneck; h.bneck32 = bneck32; h.bneck_tail = bneck_tail; h.tail = tail; h.front = front;
    return h;
}
static void check_hooks() {
    const Form conv_forms[] = {FORM_PLAIN, FORM_WITH_TAIL}, stem_forms[] = {FORM_PLAIN, FORM_FRONT_END};
    const Form bneck_forms[] = {FORM_TWO_LAUNCHES, FORM_FUSED, FORM_FUSED_TAIL_P32, FORM_FUSED_TAIL};
    for (Form f : conv_forms) {
        EXPECT(hooked(OP_CONV, f, hooks(-1, -1, -1, 0, -1)) == FORM_PLAIN, "TAIL=0 from %d", (int)f);
        EXPECT(hooked(OP_CONV, f, hooks(-1, -1, -1, 1, -1)) == FORM_WITH_TAIL, "TAIL=1 from %d", (int)f);
        EXPECT(hooked(OP_CONV, f, hooks(-1, -1, -1, 1, -1), true, 12) == FORM_PLAIN, "TAIL=1 with a tail tile whose BN is not cout, from %d", (int)f);
        EXPECT(hooked(OP_CONV, f, hooks(-1, -1, -1, 1, -1), false) == f, "TAIL=1 on a conv without a tail, from %d", (int)f);
        EXPECT(hooked(OP_CONV, f, hooks(0, 0, 0, -1, 0)) == f && hooked(OP_CONV, f, hooks(1, 1, 1, -1, 1)) == f, "another op's hook moved a conv from %d", (int)f);
    }
    for (Form f : stem_forms) {
        EXPECT(hooked(OP_STEM, f, hooks(-1, -1, -1, -1, 0)) == FORM_PLAIN, "FRONT=0 from %d", (int)f);
        EXPECT(hooked(OP_STEM, f, hooks(-1, -1, -1, -1, 1)) == FORM_FRONT_END, "FRONT=1 from %d", (int)f);
        EXPECT(hooked(OP_STEM, f, hooks(0, 0, 0, 0, -1)) == f && hooked(OP_STEM, f, hooks(1, 1, 1, 1, -1)) == f, "another op's hook moved the stem from %d", (int)f);
    }
    {
        std::vector<PlanOp> ops = {mk(OP_STEM, FORM_PLAIN)};      // front_ok = false
        apply_hooks(ops, hooks(-1, -1, -1, -1, 1), tail_legal);
        EXPECT(ops[0].choice.form == FORM_PLAIN, "FRONT=1 where the graph does not allow the front end");
    }
    for (Form f : bneck_forms) {
        const bool two = f == FORM_TWO_LAUNCHES, tail = f == FORM_FUSED_TAIL_P32 || f == FORM_FUSED_TAIL;
        EXPECT(hooked(OP_BNECK, f, hooks(0, -1, -1, -1, -1)) == FORM_TWO_LAUNCHES, "BNECK=0 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(1, -1, -1, -1, -1)) == (two ? FORM_FUSED : f), "BNECK=1 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(-1, -1, 0, -1, -1)) == (two ? f : FORM_FUSED), "BNECK_TAIL=0 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(-1, -1, 1, -1, -1)) == (two ? f : f == FORM_FUSED_TAIL ? f : FORM_FUSED_TAIL_P32), "BNECK_TAIL=1 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(-1, -1, 1, -1, -1), false) == (two ? f : FORM_FUSED), "BNECK_TAIL=1 without the capability, from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(-1, 0, -1, -1, -1)) == (tail ? FORM_FUSED_TAIL : f), "BNECK32=0 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(-1, 1, -1, -1, -1)) == (tail ? FORM_FUSED_TAIL_P32 : f), "BNECK32=1 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(1, 0, 1, -1, -1)) == FORM_FUSED_TAIL, "BNECK=1 BNECK_TAIL=1 BNECK32=0 from %d", (int)f);
        EXPECT(hooked(OP_BNECK, f, hooks(-1, -1, -1, 0, 0)) == f && hooked(OP_BNECK, f, hooks(-1, -1, -1, 1, 1)) == f, "another op's hook moved a bottleneck from %d", (int)f);
    }
    {   // BNECK=0 with BNECK_TAIL=1: two launches, and cv2 behind them runs
        std::vector<PlanOp> ops = {mk(OP_BNECK, FORM_FUSED_TAIL_P32, true), mk(OP_CONV)};
        apply_hooks(ops, hooks(0, -1, 1, -1, -1), tail_legal);
        mark_skips(ops);
        EXPECT(ops[0].choice.form == FORM_TWO_LAUNCHES && !ops[0].skip && !ops[1].skip, "BNECK=0 BNECK_TAIL=1: form %d, cv2 skipped %d", (int)ops[0].choice.form, (int)ops[1].skip);
    }
    {   // no hooks: the identity on every field
        auto ops = net(FORM_FRONT_END, FORM_WITH_TAIL, FORM_FUSED_TAIL, true, FORM_PLAIN, true);
        for (size_t i = 0; i < ops.size(); ++i) { ops[i].choice.tile = (int)i; ops[i].choice.tile2 = 20 - (int)i; ops[i].choice.tail_tile = 11 + (int)(i & 1); ops[i].choice.tail_timed = i & 2; }
        const auto before = ops;
        apply_hooks(ops, Hooks{}, tail_legal);
        for (size_t i = 0; i < ops.size(); ++i) EXPECT(same(ops[i].choice, before[i].choice) && ops[i].skip == before[i].skip, "no hooks changed op %zu", i);
    }
    printf("ok apply_hooks\n");
}

// the records a tuning run stores are those of the cache's / the tuner's choices, whatever the hooks then make of them
static void check_finish_plan() {
    auto ops = net(FORM_FRONT_END, FORM_WITH_TAIL, FORM_FUSED_TAIL_P32, true, FORM_PLAIN, true);
    for (auto &op : ops) { op.choice.tile = 6; op.choice.tile2 = 9; op.choice.tail_tile = 11; op.choice.tail_timed = true; }
    std::vector<TuneRec> want, got;
    for (auto &op : ops) want.push_back(encode_choice(op.kind, op.choice));
    finish_plan(ops, hooks(0, 0, 0, 0, 0), tail_legal, [&](const PlanOp &, const TuneRec &r) { got.push_back(r); });
    EXPECT(got.size() == want.size(), "finish_plan recorded %zu of %zu ops", got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i)
        EXPECT(same(got[i], want[i]), "op %zu: record %d %d %d, the choice before the hooks encodes to %d %d %d", i, got[i].t0, got[i].t1, got[i].fused, want[i].t0, want[i].t1, want[i].fused);
    EXPECT(want[0].fused == 1 && want[1].fused == 1 && want[3].fused == 2, "the case does not tell hooked from unhooked records");
    EXPECT(ops[0].choice.form == FORM_PLAIN && ops[1].choice.form == FORM_PLAIN && ops[3].choice.form == FORM_TWO_LAUNCHES, "finish_plan did not apply the hooks");
    std::vector<bool> s;
    for (auto &op : ops) s.push_back(op.skip);
    EXPECT(s == (std::vector<bool>{false, false, false, false, false, false, false, false, true}), "finish_plan's skips are not those of the hooked plan");
    printf("ok finish_plan\n");
}

// ---- for_each_view over toys with kernels.h's member names
struct ToyView { int seen = 0; };
struct ToyConv { ToyView in, out, res, out2, tail_out, in_lo; };
struct ToyBneck { ToyView in, out, res, tail_in, tail_out; };
struct ToyOp : PlanOp {
    ToyConv conv;
    std::vector<ToyConv> group;
    ToyBneck bneck;
    ToyView v[4];
};
static void check_views() {
    auto count = [](OpKind kind, size_t members) {
        ToyOp op;
        op.kind = kind;
        op.group.resize(members);
        int n = 0;
        for_each_view(op, [&](ToyView &v) { ++v.seen; ++n; });
        int twice = 0, total = 0;                          // every view is a different one
        auto tally = [&](const ToyView &v) { total += v.seen; twice += v.seen > 1; };
        for_each_conv_view(op.conv, tally);
        for (auto &c : op.group) for_each_conv_view(c, tally);
        for_each_bneck_view(op.bneck, tally);
        for (auto &v : op.v) tally(v);
        return twice || total != n ? -1 : n;
    };
    EXPECT(count(OP_CONV, 0) == 6, "conv: %d views, not 6", count(OP_CONV, 0));
    EXPECT(count(OP_GROUP, 6) == 36, "group of 6: %d views, not 36", count(OP_GROUP, 6));
    EXPECT(count(OP_BNECK, 2) == 17, "bottleneck: %d views, not 2 x 6 + 5", count(OP_BNECK, 2));
    for (OpKind k : {OP_STEM, OP_POOL, OP_UP}) EXPECT(count(k, 0) == 4, "kind %d: %d views, not 4", (int)k, count(k, 0));
    {   // the tally itself visits 6 + 5 members: a view dropped from both lists would otherwise cancel out
        ToyConv c; ToyBneck b;
        EXPECT(sizeof(c) == 6 * sizeof(ToyView) && sizeof(b) == 5 * sizeof(ToyView), "toy layouts");
        int n = 0;
        for_each_conv_view(c, [&](ToyView &) { ++n; });
        for_each_bneck_view(b, [&](ToyView &) { ++n; });
        EXPECT(n == 11, "conv + bottleneck lists visit %d views, not 11", n);
    }
    printf("ok for_each_view\n");
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: launch_plan_check <tune cache file>\n"); return 2; }
    check_round_trip(argv[1]);
    check_literals();
    check_skips();
    check_hooks();
    check_finish_plan();
    check_views();
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
