// launch_plan.h -- how each launch of the detector runs, as ONE value per op: the tile(s), the tail tile and the form
// (plain / with a tail / fused / front end) that the tuner, the tune cache or a test hook may decide.  Everything that derives from those decisions --
// the cache record, which ops are skipped because another launch carries them, what a hook overrides -- is computed here and nowhere else.
// Plain C++, no HIP types: tests/native/launch_plan_check.cpp drives it on the host over toy op lists.
#pragma once

#include <cstddef>

namespace rtmodt {

enum OpKind { OP_STEM, OP_CONV, OP_POOL, OP_UP, OP_GROUP, OP_BNECK };

enum Form {
    FORM_PLAIN,                // conv, group, stem: the op's own launch
    FORM_WITH_TAIL,            // conv: the 1x1 behind it runs as the tail of its launch (on `tail_tile`)
    FORM_TWO_LAUNCHES,         // bottleneck: cv1 on `tile`, cv2 on `tile2`
    FORM_FUSED,                // bottleneck: one launch, C2f.cv2 on its own
    FORM_FUSED_TAIL_P32,       // bottleneck: one launch with C2f.cv2 as its tail, BottleneckLaunch::persistent32 = 1 (bneck32.hip where it applies)
    FORM_FUSED_TAIL,           // bottleneck: the same on bottleneck_fused (persistent32 = 0)
    FORM_FRONT_END             // stem: stem + layer 1 + 2.cv1 as one launch (front.hip)
};

struct Choice {
    int tile = 0;              // conv: its tile; group: the tile its members share; bottleneck: cv1's tile as two launches
    int tile2 = 0;             // bottleneck: cv2's tile as two launches
    int tail_tile = 0;         // conv that can carry a tail: the best tail tile
    Form form = FORM_PLAIN;
    bool tail_timed = false;   // the tail (conv: against two launches; fused bottleneck: with cv2 against cv2 alone) has been timed; false = not yet
};

// What mark_skips / apply_hooks need of an op; engine.hip's Op derives from it.  `has_tail`, `front_ok` and `head_final` are fixed by the graph:
// the launch can carry the next op as its tail (conv.tail_wt / bneck.tail_wt is set), the stem may run the fused front end, this group's convs
// run inside head_final.
struct PlanOp {
    OpKind kind = OP_CONV;
    bool has_tail = false, front_ok = false, head_final = false;
    Choice choice;
    bool skip = false;         // derived (mark_skips): another launch does this op's work
};

inline bool is_fused(const PlanOp &op) { return op.kind == OP_BNECK && op.choice.form != FORM_TWO_LAUNCHES; }
// the launch also computes the op behind it
inline bool carries_tail(const PlanOp &op) {
    if (!op.has_tail) return false;
    if (op.kind == OP_CONV) return op.choice.form == FORM_WITH_TAIL;
    return op.kind == OP_BNECK && (op.choice.form == FORM_FUSED_TAIL_P32 || op.choice.form == FORM_FUSED_TAIL);
}
inline bool front_end_on(const PlanOp &op) { return op.kind == OP_STEM && op.front_ok && op.choice.form == FORM_FRONT_END; }

// ---- the tune cache's record "<t0> <t1> <fused>" <-> Choice.  The only place that knows the integers.
//   conv         t0 = tile, t1 = tail tile (0 = TILE_128x128, never a tail tile: the tail is not yet timed), fused = 0 / 1: plain / with the tail
//   group        t0 = shared tile, 0, 0
//   bottleneck   t0, t1 = cv1's and cv2's tiles; fused = 0 two launches, 1 fused and the tail not yet timed, 2 fused with the tail (persistent32),
//                3 fused, the tail timed and rejected, 4 fused with the tail (bottleneck_fused)
//   stem         0, 0, fused = 0 / 1: plain / front end (the "front|..." record)
struct TuneRec { int t0 = 0, t1 = 0, fused = 0; };

// false: the record is not one this kind writes (a miss; the op is tuned again).  Fields the record does not decide keep their value in `c`.
inline bool decode_choice(OpKind kind, const TuneRec &r, Choice &c) {
    switch (kind) {
        case OP_CONV:
            if (r.fused < 0 || r.fused > 1) return false;
            c.tile = r.t0;
            c.tail_timed = r.t1 != 0;
            if (c.tail_timed) c.tail_tile = r.t1;
            c.form = c.tail_timed && r.fused ? FORM_WITH_TAIL : FORM_PLAIN;
            return true;
        case OP_GROUP:
            if (r.fused != 0) return false;
            c.tile = r.t0;
            return true;
        case OP_BNECK: {
            static const Form forms[5] = {FORM_TWO_LAUNCHES, FORM_FUSED, FORM_FUSED_TAIL_P32, FORM_FUSED, FORM_FUSED_TAIL};
            if (r.fused < 0 || r.fused > 4) return false;
            c.tile = r.t0; c.tile2 = r.t1;
            c.form = forms[r.fused];
            c.tail_timed = r.fused >= 2;
            return true;
        }
        case OP_STEM:
            if (r.fused < 0 || r.fused > 1) return false;
            c.form = r.fused ? FORM_FRONT_END : FORM_PLAIN;
            return true;
        default: return false;
    }
}
inline TuneRec encode_choice(OpKind kind, const Choice &c) {
    TuneRec r;
    switch (kind) {
        case OP_CONV:
            r.t0 = c.tile;
            if (c.tail_timed) { r.t1 = c.tail_tile; r.fused = c.form == FORM_WITH_TAIL; }
            break;
        case OP_GROUP: r.t0 = c.tile; break;
        case OP_BNECK:
            r.t0 = c.tile; r.t1 = c.tile2;
            r.fused = c.form == FORM_TWO_LAUNCHES ? 0 : c.form == FORM_FUSED_TAIL_P32 ? 2 : c.form == FORM_FUSED_TAIL ? 4 : (c.tail_timed ? 3 : 1);
            break;
        case OP_STEM: r.fused = c.form == FORM_FRONT_END; break;
        default: break;
    }
    return r;
}

// ---- skip: recomputed for a whole op list (Ops: a random-access container of PlanOp or a type derived from it)
//   the op behind a launch that carries it as a tail (conv -> 1x1; fused Bottleneck -> C2f.cv2)
//   layer 1 and 2.cv1 (ops 1 and 2) when the front end is on; with it off, 2.cv1 exactly when layer 1 carries it
//   Detect's last group under head_final
template <class Ops>
void mark_skips(Ops &ops) {
    const size_t n = ops.size();
    for (size_t i = 0; i < n; ++i) ops[i].skip = ops[i].kind == OP_GROUP && ops[i].head_final;
    for (size_t i = 0; i + 1 < n; ++i)
        if (carries_tail(ops[i])) ops[i + 1].skip = true;
    if (n >= 3 && front_end_on(ops[0])) ops[1].skip = ops[2].skip = true;
}

// ---- the A/B and test hooks RTMODT_BNECK, BNECK32, BNECK_TAIL, TAIL, FRONT: -1 = not set, else 0 / 1
struct Hooks { int bneck = -1, bneck32 = -1, bneck_tail = -1, tail = -1, front = -1; };

// A hook overrides whatever the defaults, the cache or the tuner chose, where the op can run that way: the tail of a conv needs a tail tile that is legal
// for it (`tail_legal(op, tile)`: engine.hip's tail_tile_legal), the tail of a Bottleneck a fused Bottleneck.  Callers apply it LAST and never
// write what it leaves into the cache (finish_plan).
template <class Ops, class TailLegal>
void apply_hooks(Ops &ops, const Hooks &h, TailLegal &&tail_legal) {
    for (auto &op : ops) {
        Form &f = op.choice.form;
        if (op.kind == OP_CONV && op.has_tail && h.tail >= 0) f = h.tail && tail_legal(op, op.choice.tail_tile) ? FORM_WITH_TAIL : FORM_PLAIN;
        if (op.kind == OP_STEM && op.front_ok && h.front >= 0) f = h.front ? FORM_FRONT_END : FORM_PLAIN;
        if (op.kind != OP_BNECK) continue;
        if (h.bneck == 0) f = FORM_TWO_LAUNCHES;
        else if (h.bneck == 1 && f == FORM_TWO_LAUNCHES) f = FORM_FUSED;
        if (f == FORM_TWO_LAUNCHES) continue;
        const bool tail = h.bneck_tail >= 0 ? h.bneck_tail && op.has_tail : f != FORM_FUSED;
        const bool p32 = h.bneck32 >= 0 ? h.bneck32 != 0 : f != FORM_FUSED_TAIL;       // (BottleneckLaunch::persistent32 defaults to 1)
        f = !tail ? FORM_FUSED : (p32 ? FORM_FUSED_TAIL_P32 : FORM_FUSED_TAIL);
    }
}

// The end of every plan, in the one order that is right: the cache records are formed from what the defaults, the cache and the tuner decided
// (`record(op, rec)` for every op; the caller keeps those it stores), THEN the hooks, THEN the skips.
template <class Ops, class TailLegal, class Record>
void finish_plan(Ops &ops, const Hooks &h, TailLegal &&tail_legal, Record &&record) {
    for (auto &op : ops) record(op, encode_choice(op.kind, op.choice));
    apply_hooks(ops, h, tail_legal);
    mark_skips(ops);
}

// ---- every TensorView an op holds (sub-batch shift, arena shift, rebase); Conv / Bneck: kernels.h's ConvLaunch / BottleneckLaunch
template <class Conv, class F>
void for_each_conv_view(Conv &c, F &&fn) { fn(c.in); fn(c.out); fn(c.res); fn(c.out2); fn(c.tail_out); fn(c.in_lo); }
template <class Bneck, class F>
void for_each_bneck_view(Bneck &b, F &&fn) { fn(b.in); fn(b.out); fn(b.res); fn(b.tail_in); fn(b.tail_out); }
template <class OpT, class F>
void for_each_view(OpT &op, F &&fn) {
    if (op.kind == OP_CONV) for_each_conv_view(op.conv, fn);
    else if (op.kind == OP_GROUP || op.kind == OP_BNECK) {
        for (auto &c : op.group) for_each_conv_view(c, fn);
        if (op.kind == OP_BNECK) for_each_bneck_view(op.bneck, fn);
    } else for (auto &v : op.v) fn(v);
}

}  // namespace rtmodt
