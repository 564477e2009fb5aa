"""Plain-Python restatement of the crossing counter -- TEST INFRASTRUCTURE ONLY -- and the scenarios that
tests/test_crossing_cpu.py (no GPU) and tests/test_gpu_crossing.py (csrc/crossing.hip through the C ABI) share.

This file is the authority for what ``rtmodt_crossing_*`` computes ("Crossing counter"): one function
per rule, Python ints throughout.  The only floating point is the centroid, which the zone engine defines in
float32 (``oracle.zone_oracle.centroid``, zone_engine.py:91-92); NumPy appears there and nowhere in the arithmetic.
"Inside" is ``oracle.zone_oracle.point_polygon_test(...) >= 0``, the zone engine's own test, not restated here.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import zone_oracle as Z

LIMIT = 1 << 20                                            # centroids are clamped to, and item coordinates accepted in, [-2^20, 2^20]
LINE_DIRECTIONS = ("both", "pos", "neg")
GATE_DIRECTIONS = (None, "left_to_right", "right_to_left", "top_to_bottom", "bottom_to_top")


# ------------------------------------------------------------------------------------------------ rules
def centroid(xyxy):
    """``int((x1 + x2) / 2)``, ``int((y1 + y2) / 2)`` in float32 (truncation toward zero), clamped to +-2^20.
    ``None`` when a coordinate of the box is not finite: the track is then *not passed* this frame.  A float32 sum that
    overflows although both terms are finite is +-inf and clamps like any other large value."""
    b = [np.float32(v) for v in xyxy]
    if not all(math.isfinite(float(v)) for v in b):
        return None
    with np.errstate(over="ignore"):
        fx, fy = float((b[0] + b[2]) / np.float32(2)), float((b[1] + b[3]) / np.float32(2))
    return int(min(max(fx, -float(LIMIT)), float(LIMIT))), int(min(max(fy, -float(LIMIT)), float(LIMIT)))


def sign(v: int) -> int:
    return (v > 0) - (v < 0)


def cross(o, a, b) -> int:
    """(a - o) x (b - o)"""
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def side(a, b, p) -> int:
    """sign((B - A) x (P - A)): +1, 0 (on the infinite line) or -1."""
    return sign(cross(a, b, p))


def path_meets_segment(q, p, a, b) -> bool:
    """The line through Q and P does not have A and B strictly on one side: together with a change of side of the
    line AB between Q's stored side and P, the path Q -> P meets the closed segment AB."""
    return sign(cross(q, p, a)) * sign(cross(q, p, b)) <= 0


def line_step(stored: int, a, b, q, p):
    """One passed frame of one track at one line.  ``stored``: the last non-zero side (0: none yet); ``q``: the previous
    passed centroid (``None`` on a fresh row).  Returns ``(new stored side, "pos" | "neg" | None)``."""
    s = side(a, b, p)
    if s == 0:
        return stored, None                                # on the line: the stored side is left alone
    crossed = stored != 0 and stored != s and q is not None and path_meets_segment(q, p, a, b)
    return s, (("pos" if s > 0 else "neg") if crossed else None)


def gate_fires(direction, dx: int, dy: int) -> bool:
    """Does the displacement entry -> exit agree with the gate's direction (image axes: x right, y down)?"""
    if direction is None:
        return True
    if direction == "left_to_right":
        return dx > 0 and dx >= abs(dy)
    if direction == "right_to_left":
        return -dx > 0 and -dx >= abs(dy)
    if direction == "top_to_bottom":
        return dy > 0 and dy >= abs(dx)
    if direction == "bottom_to_top":
        return -dy > 0 and -dy >= abs(dx)
    raise ValueError(f"gate direction {direction!r}")


@functools.lru_cache(maxsize=None)
def _pip(poly: tuple, x: int, y: int) -> bool:
    return Z.point_polygon_test(np.array(poly, dtype=np.int64).reshape(-1, 2), x, y) >= 0


def inside(poly, p) -> bool:
    return _pip(tuple((int(x), int(y)) for x, y in poly), int(p[0]), int(p[1]))


def gates_from_zone_configs(zone_configs):
    """Exactly the zones with ``trigger == "crossing"`` (config/default.yaml:73-77), as gates."""
    return [{"name": z["name"], "polygon": z["polygon"], "direction": z.get("direction")} for z in zone_configs
            if z.get("trigger", "intrusion") == "crossing"]


# ------------------------------------------------------------------------------------------------ the model
class CrossingRef:
    """One stream of the counter.  ``process(tracks, frame_id)`` takes the PASSED tracks ``(id, xyxy, cls)`` in list
    order (a track with a non-finite box may be among them: it is skipped as not passed)."""

    def __init__(self, lines=(), gates=(), n_classes=80, max_tracks=2048, max_events=256, max_gap_frames=30):
        self.lines = [dict(name=l.get("name", ""), a=(int(l["a"][0]), int(l["a"][1])), b=(int(l["b"][0]), int(l["b"][1])),
                           direction=l.get("direction", "both") or "both") for l in lines]
        self.gates = [dict(name=g.get("name", ""), polygon=[(int(x), int(y)) for x, y in g["polygon"]], direction=g.get("direction"))
                      for g in gates]
        for l in self.lines:
            assert l["direction"] in LINE_DIRECTIONS and all(abs(v) <= LIMIT for v in l["a"] + l["b"])
        for g in self.gates:
            assert g["direction"] in GATE_DIRECTIONS and all(abs(v) <= LIMIT for pt in g["polygon"] for v in pt)
        self.C, self.cap, self.max_events, self.max_gap = int(n_classes), 2 * int(max_tracks), int(max_events), int(max_gap_frames)
        self.rows = {}                 # id -> dict(last, prev, side[L], inside[G], entry[G], entry_frame[G])
        self.ledger_overflow = False
        self.events_truncated = False
        self.reset_counts()
        # figures for the non-vacuity guards, derived from this model's own state
        self.line_crossings = [[0, 0] for _ in self.lines]       # all crossings, before the direction filter
        self.gate_exits = [[0, 0] for _ in self.gates]           # [fired, not fired]
        self.returned_within_gap = 0
        self.returned_after_gap = 0
        self._last_seen_ever = {}

    def reset_counts(self):
        L, G, C = len(self.lines), len(self.gates), self.C
        self.line_total = [[0, 0] for _ in range(L)]
        self.line_class = [[[0] * C for _ in range(2)] for _ in range(L)]
        self.gate_total = [0] * G
        self.gate_class = [[0] * C for _ in range(G)]

    def counts(self):
        return {"line_total": [list(r) for r in self.line_total], "line_class": [[list(c) for c in r] for r in self.line_class],
                "gate_total": list(self.gate_total), "gate_class": [list(r) for r in self.gate_class]}

    def _count(self, total_cell, class_row, k, cls):
        total_cell[k] += 1
        if 0 <= cls < self.C:
            class_row[cls] += 1

    def process(self, tracks, frame_id: int):
        frame_id = int(frame_id)
        for tid in [t for t, r in self.rows.items() if frame_id - r["last"] > self.max_gap]:     # expiry first: an id in this
            del self.rows[tid]                                                                    # very list starts fresh too
        events = []
        seen = set()
        for index, (tid, xyxy, cls) in enumerate(tracks):
            tid, cls = int(tid), int(cls)
            assert tid not in seen, "duplicate track id"
            seen.add(tid)
            p = centroid(xyxy)
            if p is None:
                continue                                   # not passed: its row, if any, stays as it is
            if tid in self._last_seen_ever and frame_id - self._last_seen_ever[tid] > 1:
                if tid in self.rows:
                    self.returned_within_gap += 1
                else:
                    self.returned_after_gap += 1
            self._last_seen_ever[tid] = frame_id
            row = self.rows.get(tid)
            fresh = row is None
            if fresh:
                row = self.rows[tid] = dict(last=frame_id, prev=None, side=[0] * len(self.lines), inside=[False] * len(self.gates),
                                            entry=[(0, 0)] * len(self.gates), entry_frame=[0] * len(self.gates))
            q, since = row["prev"], frame_id - row["last"]
            box = [float(np.float32(v)) for v in xyxy]
            for k, l in enumerate(self.lines):
                row["side"][k], d = line_step(row["side"][k], l["a"], l["b"], q, p)
                if d is None:
                    continue
                self.line_crossings[k][d == "neg"] += 1
                if l["direction"] in ("both", d):
                    self._count(self.line_total[k], self.line_class[k][d == "neg"], int(d == "neg"), cls)
                    events.append(dict(track_id=tid, track=index, kind="line", index=k, direction=d, class_id=cls, bbox_xyxy=box,
                                       centroid=list(p), prev=list(q), frames=since))
            for k, g in enumerate(self.gates):
                now_in = inside(g["polygon"], p)
                if now_in and not row["inside"][k]:        # entering: outside -> inside, or first seen inside
                    row["inside"][k], row["entry"][k], row["entry_frame"][k] = True, p, frame_id
                elif not now_in and row["inside"][k]:      # leaving
                    row["inside"][k] = False
                    e = row["entry"][k]
                    fired = gate_fires(g["direction"], p[0] - e[0], p[1] - e[1])
                    self.gate_exits[k][not fired] += 1
                    if fired:
                        self._count(self.gate_total, self.gate_class[k], k, cls)
                        events.append(dict(track_id=tid, track=index, kind="gate", index=k, direction=g["direction"], class_id=cls,
                                           bbox_xyxy=box, centroid=list(p), prev=list(e), frames=frame_id - row["entry_frame"][k]))
            row["last"], row["prev"] = frame_id, p
        if len(self.rows) > self.cap:
            self.ledger_overflow = True
        self.events_truncated = len(events) > self.max_events
        return events

    def snapshot(self):
        """Rows in ascending id: ``[id, last frame, prev, stored sides, [gate, entry x, entry y, entry frame] of the gates it is in]``."""
        return [[tid, r["last"], list(r["prev"]), list(r["side"]),
                 [[k, r["entry"][k][0], r["entry"][k][1], r["entry_frame"][k]] for k in range(len(self.gates)) if r["inside"][k]]]
                for tid, r in sorted(self.rows.items())]


# ------------------------------------------------------------------------------------------------ helpers
def box(cx, cy, w=10, h=8):
    """float32 box whose centroid is exactly (cx, cy)."""
    return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], np.float32)


def walk(points, tid=1, cls=0, start=0):
    """One track visiting ``points`` on consecutive frames (``None``: absent that frame): ``[(frame_id, [(id, box, cls)])]``."""
    return [(start + f, [] if p is None else [(tid, box(*p), cls)]) for f, p in enumerate(points)]


# ------------------------------------------------------------------------------------------------ hand cases
# A vertical line x = 10 from (10, 0) up to (10, 20) in image axes: A = (10, 0), B = (10, 20), B - A = (0, 20);
# side(P) = sign(0 * (py - 0) - 20 * (px - 10)) = sign(10 - px): +1 on the LEFT (x < 10), -1 on the right.
LINE_V = {"name": "v", "a": [10, 0], "b": [10, 20], "direction": "both"}
SQUARE = [[10, 10], [30, 10], [30, 30], [10, 30]]
CONCAVE = [[0, 0], [40, 0], [40, 40], [20, 10], [0, 40]]   # a notch from the bottom edge up to (20, 10)

# name -> dict(lines, gates, calls, line_total, gate_total[, kwargs]): the totals are worked out by hand in the comments
HAND_CASES = {
    # left -> right: side +1 -> -1, path y = 10 meets the segment: one "neg"
    "line_pass_neg": dict(lines=[LINE_V], calls=walk([(5, 10), (15, 10)]), line_total=[[0, 1]]),
    # right -> left: one "pos"
    "line_pass_pos": dict(lines=[LINE_V], calls=walk([(15, 10), (5, 10)]), line_total=[[1, 0]]),
    # y = 30 and y = 31 (where (15, 30) -> (5, 32) meets x = 10) are past B: not counted either way, though the side flips;
    # coming back through the segment (y = 10) counts once
    "line_beyond_end": dict(lines=[LINE_V], calls=walk([(5, 30), (15, 30), (5, 32)]), line_total=[[0, 0]]),
    "line_beyond_end_then_back_inside": dict(lines=[LINE_V], calls=walk([(5, 30), (15, 30), (15, 10), (5, 10)]), line_total=[[1, 0]]),
    # (0, 30) -> (20, 10) passes exactly through B = (10, 20): cross products -, 0 -> product 0 <= 0: counted
    "line_through_endpoint": dict(lines=[LINE_V], calls=walk([(0, 30), (20, 10)]), line_total=[[0, 1]]),
    # three frames on the line, then on: one count, made on the frame that leaves the line (Q = (10, 10) is on the segment)
    "line_land_then_on": dict(lines=[LINE_V], calls=walk([(5, 10), (10, 10), (10, 12), (10, 8), (15, 10)]), line_total=[[0, 1]]),
    # on the line and back to where it came from: none
    "line_land_then_back": dict(lines=[LINE_V], calls=walk([(5, 10), (10, 10), (10, 11), (4, 10)]), line_total=[[0, 0]]),
    # L R L R L: neg, pos, neg, pos -> 2 / 2, net 0
    "line_oscillate": dict(lines=[LINE_V], calls=walk([(5, 10), (15, 10), (5, 11), (15, 9), (6, 10)]), line_total=[[2, 2]]),
    "line_oscillate_odd": dict(lines=[LINE_V], calls=walk([(5, 10), (15, 10), (5, 11), (15, 9)]), line_total=[[1, 2]]),
    # a "pos"-only line ignores the two "neg" crossings of the same walk
    "line_pos_only": dict(lines=[dict(LINE_V, direction="pos")], calls=walk([(5, 10), (15, 10), (5, 11), (15, 9), (6, 10)]), line_total=[[2, 0]]),
    "line_neg_only": dict(lines=[dict(LINE_V, direction="neg")], calls=walk([(5, 10), (15, 10), (5, 11), (15, 9), (6, 10)]), line_total=[[0, 2]]),
    # gap: seen at frame 0, next at frame 3 with max_gap_frames = 3 -> 3 - 0 = 3, not more than 3: same row, counts
    "gap_exact": dict(lines=[LINE_V], calls=[(0, [(1, box(5, 10), 0)]), (3, [(1, box(15, 10), 0)])], line_total=[[0, 1]], kwargs=dict(max_gap_frames=3)),
    # frame 4: 4 > 3, fresh row, no previous point: nothing
    "gap_one_more": dict(lines=[LINE_V], calls=[(0, [(1, box(5, 10), 0)]), (4, [(1, box(15, 10), 0)])], line_total=[[0, 0]], kwargs=dict(max_gap_frames=3)),
    # calls in between that do not list the id change nothing
    "gap_exact_with_calls_between": dict(lines=[LINE_V], calls=[(0, [(1, box(5, 10), 0)]), (1, []), (2, [(2, box(50, 50), 0)]), (3, [(1, box(15, 10), 0)])],
                                         line_total=[[0, 1]], kwargs=dict(max_gap_frames=3)),
    "gap_one_more_with_calls_between": dict(lines=[LINE_V], calls=[(0, [(1, box(5, 10), 0)]), (1, []), (2, []), (3, []), (4, [(1, box(15, 10), 0)])],
                                            line_total=[[0, 0]], kwargs=dict(max_gap_frames=3)),
    # gates: in at (12, 20), out on the far side
    "gate_left_to_right": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "left_to_right"}], calls=walk([(5, 20), (12, 20), (25, 20), (35, 22)]), gate_total=[1]),
    "gate_left_to_right_walked_backwards": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "left_to_right"}], calls=walk([(35, 20), (28, 20), (15, 20), (5, 22)]),
                                                gate_total=[0]),
    "gate_right_to_left": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "right_to_left"}], calls=walk([(35, 20), (28, 20), (15, 20), (5, 22)]), gate_total=[1]),
    "gate_top_to_bottom": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "top_to_bottom"}], calls=walk([(20, 5), (20, 12), (22, 35)]), gate_total=[1]),
    "gate_bottom_to_top": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "bottom_to_top"}], calls=walk([(20, 35), (20, 28), (22, 5)]), gate_total=[1]),
    "gate_top_to_bottom_walked_sideways": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "top_to_bottom"}], calls=walk([(5, 20), (12, 20), (35, 22)]), gate_total=[0]),
    # entry (12, 12), exit (32, 32): dx = dy = 20 -> dx >= |dy| and dy >= |dx|: the tie fires both axes
    "gate_tie_left_to_right": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "left_to_right"}], calls=walk([(12, 12), (32, 32)]), gate_total=[1]),
    "gate_tie_top_to_bottom": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "top_to_bottom"}], calls=walk([(12, 12), (32, 32)]), gate_total=[1]),
    # entry (12, 12), exit (31, 32): dx 19 < |dy| 20: left_to_right does not fire
    "gate_off_tie": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": "left_to_right"}], calls=walk([(12, 12), (31, 32)]), gate_total=[0]),
    # born inside: the first sighting is the entry
    "gate_born_inside": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": None}], calls=walk([(20, 20), (40, 20)]), gate_total=[1]),
    # dropped while inside (last passed at frame 1, back at frame 4: 3 > 2): the row goes, the return outside is a fresh row: nothing
    "gate_dropped_inside": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": None}], calls=walk([(5, 20), (20, 20), None, None, (40, 20)]), gate_total=[0],
                                kwargs=dict(max_gap_frames=2)),
    # back at frame 3 (2, not more than 2): the row is kept as it is and the exit fires
    "gate_away_within_gap": dict(gates=[{"name": "g", "polygon": SQUARE, "direction": None}], calls=walk([(5, 20), (20, 20), None, (40, 20)]), gate_total=[1],
                                 kwargs=dict(max_gap_frames=2)),
    # concave: (20, 30) lies in the notch (outside); (10, 5) -> (20, 5) inside -> (20, 30) leaves through the notch with dy = 25 >= |dx| = 10
    "gate_concave": dict(gates=[{"name": "g", "polygon": CONCAVE, "direction": "top_to_bottom"}], calls=walk([(10, 5), (20, 5), (20, 30)]), gate_total=[1]),
    "gate_concave_notch_is_outside": dict(gates=[{"name": "g", "polygon": CONCAVE, "direction": None}], calls=walk([(20, 30), (20, 35), (20, 45)]), gate_total=[0]),
}


def run_case(case):
    """Runs a hand case through the model; returns the model."""
    ref = CrossingRef(case.get("lines", ()), case.get("gates", ()), max_tracks=64, **case.get("kwargs", {}))
    for frame_id, tracks in case["calls"]:
        ref.process(tracks, frame_id)
    return ref


# ------------------------------------------------------------------------------------------------ random walk
WALK = dict(n_streams=3, ids=150, lattice=96, step=6, n_frames=120, max_gap_frames=4, n_classes=80, max_tracks=256, max_events=512, seed=3)
WALK_LINES = [
    {"name": "vertical", "a": [48, 0], "b": [48, 95], "direction": "both"},            # axis-aligned
    {"name": "horizontal", "a": [95, 40], "b": [0, 40], "direction": "pos"},           # axis-aligned, one direction only
    {"name": "diagonal", "a": [10, 10], "b": [85, 85], "direction": "neg"},
    {"name": "pixel", "a": [30, 60], "b": [31, 60], "direction": "both"},              # a single pixel long
    {"name": "vee_right", "a": [70, 20], "b": [90, 50], "direction": "both"},          # two sharing an endpoint
    {"name": "vee_left", "a": [70, 20], "b": [50, 50], "direction": "both"},
]
WALK_GATES = [
    {"name": "convex", "polygon": [[10, 10], [40, 12], [44, 40], [12, 44]], "direction": "left_to_right"},
    {"name": "concave", "polygon": [[50, 50], [90, 50], [90, 90], [70, 65], [50, 90]], "direction": "top_to_bottom"},
    {"name": "repeated", "polygon": [[5, 55], [35, 55], [35, 55], [40, 85], [8, 90]], "direction": "right_to_left"},
    {"name": "two_point", "polygon": [[60, 5], [90, 35]], "direction": "bottom_to_top"},   # degenerate: "inside" = on the segment
]


@functools.lru_cache(maxsize=None)
def walk_scenario(seed=None):
    """Three streams through one handle: per stream 150 int64 ids (negative and > 2^32 among them) walk a 96 x 96 integer lattice
    with steps in [-6, 6]; an id is present for 3-12 frames, away for 1 .. max_gap_frames + 3, and so on; the list is handed over
    shuffled; class ids run over [-1, 82) so that some fall outside [0, 80).  Returns the calls in the order they are made:
    ``(stream, frame_id, [(id, xyxy, cls), ...])``."""
    seed = WALK["seed"] if seed is None else seed
    S, P, N, F = WALK["n_streams"], WALK["ids"], WALK["lattice"], WALK["n_frames"]
    calls = []
    rngs = [np.random.default_rng(1000 * seed + s) for s in range(S)]
    state = []
    for rng in rngs:
        ids = np.unique(rng.integers(-(1 << 40), 1 << 40, size=P + 20))[:P]
        rng.shuffle(ids)
        state.append(dict(ids=ids, cls=rng.integers(-1, 82, size=P), pos=rng.integers(0, N, size=(P, 2)), present=rng.random(P) < 0.7,
                          left=rng.integers(1, 8, size=P), wh=2 * rng.integers(2, 9, size=(P, 2))))
    for f in range(F):
        for s in range(S):
            rng, st = rngs[s], state[s]
            idx = np.nonzero(st["present"])[0]
            st["pos"][idx] = np.clip(st["pos"][idx] + rng.integers(-WALK["step"], WALK["step"] + 1, size=(len(idx), 2)), 0, N - 1)
            order = rng.permutation(idx)
            calls.append((s, 10 + f, [(int(st["ids"][i]), box(int(st["pos"][i, 0]), int(st["pos"][i, 1]), int(st["wh"][i, 0]), int(st["wh"][i, 1])),
                                      int(st["cls"][i])) for i in order]))
            st["left"] -= 1
            flip = st["left"] <= 0
            st["present"] = np.where(flip, ~st["present"], st["present"])
            st["left"] = np.where(flip, np.where(st["present"], rng.integers(3, 13, size=P), rng.integers(1, WALK["max_gap_frames"] + 4, size=P)), st["left"])
    return calls


def walk_models():
    return [CrossingRef(WALK_LINES, WALK_GATES, n_classes=WALK["n_classes"], max_tracks=WALK["max_tracks"], max_events=WALK["max_events"],
                        max_gap_frames=WALK["max_gap_frames"]) for _ in range(WALK["n_streams"])]


def walk_guards(models):
    """What the run must have seen for the comparison to mean something, from the models alone."""
    L, G = len(WALK_LINES), len(WALK_GATES)
    fig = dict(lines=[[sum(m.line_crossings[k][d] for m in models) for d in range(2)] for k in range(L)],
               gates=[[sum(m.gate_exits[k][d] for m in models) for d in range(2)] for k in range(G)],
               within=sum(m.returned_within_gap for m in models), after=sum(m.returned_after_gap for m in models),
               out_of_range_class=sum(sum(m.line_total[k]) - sum(map(sum, m.line_class[k])) for m in models for k in range(L)),
               overflow=[m.ledger_overflow for m in models])
    assert all(min(c) >= 1 for c in fig["lines"]), fig             # each direction on every line (none is degenerate: A != B throughout)
    assert all(min(e) >= 1 for e in fig["gates"]), fig             # a firing and a non-firing exit on every gate (all four have a direction)
    assert fig["within"] >= 1 and fig["after"] >= 1 and fig["out_of_range_class"] >= 1 and not any(fig["overflow"]), fig
    return fig


# ------------------------------------------------------------------------------------------------ workgroup boundaries
BOUNDARY_LINES = [{"name": "x100", "a": [100, 0], "b": [100, 4000], "direction": "both"}, {"name": "y2000", "a": [0, 2000], "b": [200, 2000], "direction": "both"}]
BOUNDARY_GATES = [{"name": "strip", "polygon": [[90, 0], [110, 0], [110, 4000], [90, 4000]], "direction": None}]


def boundary_calls():
    """max_tracks = 300: 257, 300, 1 and 300 tracks passed on consecutive frames (more than one pass of the 256-thread loops, then a ledger
    of mostly idle rows, then every idle row matched again); track k sits at y = 10 k and hops over the line x = 100 (and through the
    strip gate around it) from frame to frame."""
    def frame(f, ks):
        return (f, [(7 * k - 900, box(80 + 12 * ((f + k) % 4), 10 * k), k % 90) for k in ks])
    return [frame(0, range(257)), frame(1, range(300)), frame(2, [123]), frame(3, reversed(range(300)))]


NINE_LINE = {"name": "long", "a": [10, 0], "b": [10, 200], "direction": "both"}


def nine_crossings_calls():
    """max_events = 4: nine tracks cross one line in one frame, handed over in descending id order."""
    ks = list(range(9, 0, -1))
    return [(0, [(k, box(5, 10 * k), 1) for k in ks]), (1, [(k, box(15, 10 * k), 1) for k in ks])]


LEDGER_FULL_CALLS = [                                      # max_tracks = 8 -> 16 rows; max_gap_frames large: ids never expire
    (0, [1, 2, 3, 4, 5]),                                  # rows 5
    (1, [6, 7, 8, 9, 10]),                                 # 5 + 5 idle = 10
    (2, [3, 11, 12, 13, 14, 15]),                          # 6 + 9 idle = 15
    (3, [16, 3]),                                          # 2 + 14 idle = 16: exactly full, passes
    (4, [17]),                                             # 1 + 16 idle = 17: ledger full
    (5, [3]),                                              # the stream stays in error
]


# ------------------------------------------------------------------------------------------------ marching boxes (tracker sources)
MARCH_LINES = [{"name": "x200", "a": [200, 0], "b": [200, 400], "direction": "both"}]
MARCH_GATES = [{"name": "exit_gate", "polygon": [[260, 0], [340, 0], [340, 400], [260, 400]], "direction": "left_to_right"}]


def march_scene(n_frames=56, n_boxes=5, reverse=False, early=False):
    """Boxes of 40 x 40 march 4 px per frame along their own rows, left to right from x = 150 (``reverse``: right to left from 374), over
    the line x = 200 and through the gate 260..340; box 1 is not detected on frames 10-13.  ``early``: one more box starts at
    x = 197 and is over the line on its second frame.  Per frame ``(xyxy, conf, cls, object index)``."""
    frames = []
    for f in range(n_frames):
        rows = []
        for k in range(n_boxes + (1 if early else 0)):
            if k == 1 and 10 <= f <= 13:
                continue
            x0 = 197 if k == n_boxes else 150 + 3 * k
            cx = (x0 + 224 - 4 * f) if reverse else x0 + 4 * f
            cy = 30 + 60 * k
            rows.append(([cx - 20, cy - 20, cx + 20, cy + 20], k))
        xy = np.asarray([r[0] for r in rows], np.float32).reshape(-1, 4)
        frames.append((xy, np.full(len(rows), 0.9, np.float32), np.asarray([r[1] % 3 for r in rows], np.int32), np.asarray([r[1] for r in rows])))
    return frames
