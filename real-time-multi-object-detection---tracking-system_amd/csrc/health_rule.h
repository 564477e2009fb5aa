// health_rule.h -- the one statement of the camera-health monitor's rules (csrc/health.hip runs them per frame; its header states the
// launches).  Plain C++, no HIP: the kernels of health.hip, the host-only entry point rtmodt_health_decide and
// tests/native/health_rule_check.cpp (built under the address and UB sanitizers) all take them from here, and tests/health_ref.py
// restates them in NumPy.  Everything is integer arithmetic.  Grid, pixel luma and cell luma Y are motion_model.h's.
//   Fine.     F of a cell = the sum of |y(x + 1, yy) - y(x, yy)| over its pixels with x + 1 < w (y: pixel luma); sharp = the sum of F.
//   Coarse.   G = min(255, |Y[cy][cx+1] - Y[cy][cx-1]| + |Y[cy+1][cx] - Y[cy-1][cx]|) for 1 <= cx <= gw - 2, 1 <= cy <= gh - 2, else 0.
//             Edge: G >= edge_threshold; weak edge: 2 G >= edge_threshold.  R (unsigned 8.8 in 16 bits) is a slow average of G.
//   Counts.   luma_sum, n_dark (Y <= dark_level), n_bright (Y >= bright_level), n_changed (Y differs from the stream's previous grid;
//             every cell when frames_seen == 0), n_edge, n_ref_edge (R >= edge_threshold << 8, R as it was at entry), n_kept
//             (reference edge and weak edge now).
//   Raw.      With frames_seen >= warmup at entry: DARK 1000 n_dark >= dark_pm cells, BRIGHT likewise (a per-mille of 0 disables
//             either); with n_ref_edge >= min_ref_edges besides (else the informational bit NO_STRUCTURE), lost = 1000 n_kept < retain_pm
//             n_ref_edge, COVERED = lost && 1000 n_edge < cover_pm n_ref_edge, MOVED = lost && !COVERED, DEFOCUSED = !lost && 1000 sharp <
//             defocus_pm (ref_sharp >> 8) (a per-mille of 0: the comparison cannot hold).  FROZEN = freeze_frames > 0 && frames_seen >= 1 &&
//             n_changed <= freeze_cells, warm-up or not.
//   Debounce. Per condition, in condition order.  Inactive: run counts consecutive raw frames; at hold_frames (FROZEN: freeze_frames)
//             the condition becomes active, RAISED, run = off = 0.  Active: run counts the frames since (its age), off the consecutive
//             frames without the raw condition; at clear_frames (FROZEN: 1) it becomes inactive, CLEARED, run = off = 0.
//   Learning. Runs iff frames_seen < warmup at entry, or no raw exposure or structure condition holds and none is active after the
//             debounce: a tampered picture is never learned.  frames_seen == 0: R = G << 8, ref_sharp = sharp << 8; else R += ((G << 8)
//             - R) >> ref_shift and the same for ref_sharp (8 fractional bits; arithmetic shifts of the signed value).  Then
//             frames_seen = min(frames_seen + 1, 2^30).
//   Relearn.  relearn_frames > 0 and an active structure condition of age >= relearn_frames: a rebase -- CLEARED for each active
//             structure condition in condition order, REBASED (condition -1), their counters 0, frames_seen = 0: the next frame starts
//             a new reference.  An operator's rebase does the same at once (hl_rebase_now) and owes the events to the stream's next
//             call, which reports them first.
//   Events.   At most HL_MAX_EVENTS = 8 per stream and call.  An owed rebase is at most 3 CLEARED + REBASED and leaves frames_seen 0
//             and no structure condition active, so the frame behind it can only clear DARK, BRIGHT and FROZEN: 7.  Otherwise the
//             debounce gives DARK, BRIGHT and FROZEN one event each (3); the three raw structure conditions exclude one another, so
//             at most one is RAISED, and a relearn adds one CLEARED for each that is still active (one that the debounce just cleared
//             is not) and REBASED: 1 + 3 + 1 = 5, in all 8.  This holds for every state hl_state_ok accepts, whatever its counters.
#pragma once

#include "motion_model.h"

namespace rtmodt {

constexpr int HL_DARK = 0, HL_BRIGHT = 1, HL_COVERED = 2, HL_MOVED = 3, HL_DEFOCUSED = 4, HL_FROZEN = 5, HL_CONDITIONS = 6;
constexpr uint32_t HL_NO_STRUCTURE = 1u << 6, HL_EXPOSURE = 1u << HL_DARK | 1u << HL_BRIGHT;
constexpr uint32_t HL_STRUCTURE = 1u << HL_COVERED | 1u << HL_MOVED | 1u << HL_DEFOCUSED, HL_PENDING_REBASE = 1u << 8;
constexpr int HL_RAISED = 1, HL_CLEARED = 2, HL_REBASED = 3;
constexpr int HL_LEARN_NONE = 0, HL_LEARN_AVERAGE = 1, HL_LEARN_SET = 2;
constexpr int HL_MAX_EVENTS = 8, HL_MAX_COUNT = 1 << 30, HL_MAX_TIMER = 65535;

struct HlRule {
    int32_t edge_threshold, ref_shift, warmup, dark_level, dark_pm, bright_level, bright_pm, retain_pm, cover_pm, defocus_pm, min_ref_edges, hold_frames,
        clear_frames, freeze_frames, freeze_cells, relearn_frames;
};
struct HlCounts { uint64_t luma_sum, sharp; uint32_t n_dark, n_bright, n_changed, n_edge, n_ref_edge, n_kept; };
struct HlState { uint64_t ref_sharp; int32_t frames_seen; uint32_t active, pending; int32_t reserved; int32_t run[HL_CONDITIONS], off[HL_CONDITIONS]; };
struct HlEvent { int32_t condition, kind; };

MO_HD inline bool hl_pm_ok(int32_t v) { return v >= 0 && v <= 1000; }
MO_HD inline bool hl_rule_ok(const HlRule &r) {
    return r.edge_threshold >= 1 && r.edge_threshold <= 255 && r.ref_shift >= 1 && r.ref_shift <= 12 && r.warmup >= 1 && r.warmup <= 255 &&
           r.dark_level >= 0 && r.dark_level <= 255 && r.bright_level >= 0 && r.bright_level <= 255 && hl_pm_ok(r.dark_pm) && hl_pm_ok(r.bright_pm) &&
           hl_pm_ok(r.retain_pm) && hl_pm_ok(r.cover_pm) && hl_pm_ok(r.defocus_pm) && r.min_ref_edges >= 0 && r.min_ref_edges <= MO_MAX_CELLS &&
           r.hold_frames >= 1 && r.hold_frames <= HL_MAX_TIMER && r.clear_frames >= 1 && r.clear_frames <= HL_MAX_TIMER && r.freeze_frames >= 0 &&
           r.freeze_frames <= HL_MAX_TIMER && r.freeze_cells >= 0 && r.freeze_cells <= MO_MAX_CELLS && r.relearn_frames >= 0 && r.relearn_frames <= HL_MAX_COUNT;
}
// a state a handle may hold: what hl_step and hl_rebase_now can have left behind.  Owed events stand only behind a rebase, which
// leaves frames_seen 0 and no structure condition active until the next frame: the bound on a call's events rests on it.
MO_HD inline bool hl_state_ok(const HlState &s) {
    bool ok = s.frames_seen >= 0 && s.frames_seen <= MO_MAX_SEEN && s.active < (1u << HL_CONDITIONS) && (s.pending & ~(HL_STRUCTURE | HL_PENDING_REBASE)) == 0 &&
              (s.pending == 0 || ((s.pending & HL_PENDING_REBASE) && s.frames_seen == 0 && !(s.active & HL_STRUCTURE))) && s.ref_sharp < (1ull << 48);
    for (int i = 0; i < HL_CONDITIONS; ++i) ok = ok && s.run[i] >= 0 && s.run[i] <= HL_MAX_COUNT && s.off[i] >= 0 && s.off[i] <= HL_MAX_COUNT;
    return ok;
}

MO_HD inline uint32_t hl_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
// G of an interior cell from its four neighbours' lumas
MO_HD inline uint32_t hl_coarse(uint32_t left, uint32_t right, uint32_t up, uint32_t down) {
    const uint32_t g = hl_absdiff(right, left) + hl_absdiff(down, up);
    return g < 255u ? g : 255u;
}
MO_HD inline bool hl_interior(int32_t cx, int32_t cy, int32_t gw, int32_t gh) { return cx >= 1 && cy >= 1 && cx <= gw - 2 && cy <= gh - 2; }
MO_HD inline bool hl_edge(uint32_t g, int32_t edge_threshold) { return g >= (uint32_t)edge_threshold; }
MO_HD inline bool hl_weak_edge(uint32_t g, int32_t edge_threshold) { return 2u * g >= (uint32_t)edge_threshold; }
MO_HD inline bool hl_ref_edge(uint32_t r, int32_t edge_threshold) { return r >= ((uint32_t)edge_threshold << 8); }
// one cell's R (8.8, 0..65280) under the learning step `learn`
MO_HD inline uint32_t hl_learn_r(uint32_t r, uint32_t g, int32_t learn, int32_t ref_shift) {
    if (learn == HL_LEARN_SET) return g << 8;
    if (learn == HL_LEARN_AVERAGE) return (uint32_t)((int32_t)r + (((int32_t)(g << 8) - (int32_t)r) >> ref_shift));
    return r;
}

MO_HD inline uint32_t hl_raw(const HlRule &r, const HlCounts &k, int64_t cells, int32_t frames_seen, uint64_t ref_sharp) {
    uint32_t raw = 0;
    if (frames_seen >= r.warmup) {
        if (r.dark_pm && 1000LL * (int64_t)k.n_dark >= (int64_t)r.dark_pm * cells) raw |= 1u << HL_DARK;
        if (r.bright_pm && 1000LL * (int64_t)k.n_bright >= (int64_t)r.bright_pm * cells) raw |= 1u << HL_BRIGHT;
        if ((int64_t)k.n_ref_edge < (int64_t)r.min_ref_edges) {
            raw |= HL_NO_STRUCTURE;
        } else {
            const bool lost = 1000LL * (int64_t)k.n_kept < (int64_t)r.retain_pm * (int64_t)k.n_ref_edge;
            const bool covered = lost && 1000LL * (int64_t)k.n_edge < (int64_t)r.cover_pm * (int64_t)k.n_ref_edge;
            if (covered) raw |= 1u << HL_COVERED;
            if (lost && !covered) raw |= 1u << HL_MOVED;
            if (!lost && 1000ull * k.sharp < (uint64_t)r.defocus_pm * (ref_sharp >> 8)) raw |= 1u << HL_DEFOCUSED;     // sharp < 2^38, ref_sharp < 2^46
        }
    }
    if (r.freeze_frames && frames_seen >= 1 && (int64_t)k.n_changed <= (int64_t)r.freeze_cells) raw |= 1u << HL_FROZEN;
    return raw;
}

MO_HD inline int32_t hl_count_up(int32_t v) { return v + 1 < HL_MAX_COUNT ? v + 1 : HL_MAX_COUNT; }

// the rebase on a state: its CLEARED events and REBASED go to ev[n...]; returns the new n
MO_HD inline int hl_rebase(HlState &s, HlEvent *ev, int n) {
    for (int i = 0; i < HL_CONDITIONS; ++i) {
        if (!(HL_STRUCTURE >> i & 1u)) continue;
        if (s.active >> i & 1u) ev[n++] = HlEvent{i, HL_CLEARED};
        s.run[i] = s.off[i] = 0;
    }
    ev[n++] = HlEvent{-1, HL_REBASED};
    s.active &= ~HL_STRUCTURE;
    s.frames_seen = 0;
    return n;
}
// an operator's rebase: the state is rebased at once, the events are owed to the next frame
MO_HD inline void hl_rebase_now(HlState &s) {
    HlEvent ev[4];
    const int n = hl_rebase(s, ev, 0);
    s.pending |= HL_PENDING_REBASE;
    for (int i = 0; i < n; ++i)
        if (ev[i].kind == HL_CLEARED) s.pending |= 1u << ev[i].condition;
}

// one frame of one stream: decides, debounces, learns ref_sharp and counts frames_seen.  ev[HL_MAX_EVENTS]; returns the number of
// events; *raw and *learn (the step the cells' R takes: hl_learn_r) are the frame's.
MO_HD inline int hl_step(const HlRule &r, const HlCounts &k, int64_t cells, HlState &s, HlEvent *ev, uint32_t *raw_out, int32_t *learn_out) {
    int n = 0;
    if (s.pending) {
        for (int i = 0; i < HL_CONDITIONS; ++i)
            if (s.pending >> i & 1u) ev[n++] = HlEvent{i, HL_CLEARED};
        if (s.pending & HL_PENDING_REBASE) ev[n++] = HlEvent{-1, HL_REBASED};
        s.pending = 0;
    }
    const int32_t seen = s.frames_seen;
    const uint32_t raw = hl_raw(r, k, cells, seen, s.ref_sharp);
    for (int i = 0; i < HL_CONDITIONS; ++i) {
        const bool on = raw >> i & 1u;
        const int32_t hold = i == HL_FROZEN ? r.freeze_frames : r.hold_frames, clear = i == HL_FROZEN ? 1 : r.clear_frames;
        if (!(s.active >> i & 1u)) {
            s.run[i] = on ? hl_count_up(s.run[i]) : 0;
            s.off[i] = 0;
            if (on && s.run[i] >= hold) {
                s.active |= 1u << i;
                s.run[i] = 0;
                ev[n++] = HlEvent{i, HL_RAISED};
            }
        } else {
            s.run[i] = hl_count_up(s.run[i]);
            s.off[i] = on ? 0 : hl_count_up(s.off[i]);
            if (s.off[i] >= clear) {
                s.active &= ~(1u << i);
                s.run[i] = s.off[i] = 0;
                ev[n++] = HlEvent{i, HL_CLEARED};
            }
        }
    }
    int32_t learn = HL_LEARN_NONE;
    if (seen < r.warmup || !((raw | s.active) & (HL_EXPOSURE | HL_STRUCTURE))) {
        learn = seen == 0 ? HL_LEARN_SET : HL_LEARN_AVERAGE;
        const int64_t t = (int64_t)(k.sharp << 8), cur = (int64_t)s.ref_sharp;
        s.ref_sharp = (uint64_t)(seen == 0 ? t : cur + ((t - cur) >> r.ref_shift));
    }
    s.frames_seen = seen + 1 < MO_MAX_SEEN ? seen + 1 : MO_MAX_SEEN;
    if (r.relearn_frames > 0) {
        bool due = false;
        for (int i = 0; i < HL_CONDITIONS; ++i) due = due || ((HL_STRUCTURE & s.active) >> i & 1u && s.run[i] >= r.relearn_frames);
        if (due) n = hl_rebase(s, ev, n);
    }
    *raw_out = raw;
    *learn_out = learn;
    return n;
}

}  // namespace rtmodt
