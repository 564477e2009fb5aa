"""Ledger model of the zone event engine -- TEST INFRASTRUCTURE ONLY -- and the seeded scenarios that
tests/test_zone_ref_cpu.py (no GPU) and tests/test_gpu_zones.py (csrc/zones.hip through the C ABI) share.

``ZoneLedgerRef`` is ``oracle.zone_oracle.ZoneOracle`` (events, occupancy, cooldown: its ``process``, not restated)
plus what ``include/rtmodt.h`` documents on top of the reference: ``max_idle_frames`` expiry, the row count of the
2 x max_tracks ledger, and the tracker-source mode of ``rtmodt_zones_process_tracker``.  It follows the documented
contract, not the kernel.

Point-in-polygon is memoised per (polygon, cx, cy): every value is one call of the oracle's scalar
``point_polygon_test``, so there is nothing vectorised to cross-check.  The scenarios keep centroids on a coarse lattice
so that the memo stays small.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

from oracle import zone_oracle as Z

# ------------------------------------------------------------------------------------------------ memoised scalar test
_SCALAR_PIP = Z.point_polygon_test
_INTERNED = {}                     # polygon bytes -> the one _Poly with those vertices, shared by every model


class _Poly(np.ndarray):
    """A zone's int32 polygon, hashable by identity so that (polygon, x, y) can key the memo."""
    __hash__ = object.__hash__

    def __eq__(self, other):
        return self is other


def interned(poly):
    a = np.ascontiguousarray(poly, dtype=np.int32).reshape(-1, 2)
    return _INTERNED.setdefault(a.tobytes(), a.view(_Poly))


@functools.lru_cache(maxsize=None)
def _memo_pip(poly, x, y):
    return _SCALAR_PIP(poly, x, y)


def share_memo(oracle):
    """Gives a bare ``ZoneOracle`` the interned polygons (same vertices), so that it can run under ``memoised_pip``."""
    for z in oracle.zones:
        z["polygon"] = interned(z["polygon"])
    return oracle


@contextlib.contextmanager
def memoised_pip():
    """Inside: ``zone_oracle.point_polygon_test`` answers repeated (polygon, x, y) from a table of its own results."""
    saved = Z.point_polygon_test
    Z.point_polygon_test = _memo_pip
    try:
        yield
    finally:
        Z.point_polygon_test = saved


def inside(poly, x, y) -> bool:
    return _memo_pip(interned(poly), int(x), int(y)) >= 0


# ------------------------------------------------------------------------------------------------ the model
class ZoneLedgerRef(Z.ZoneOracle):
    """``ZoneOracle`` + expiry by ``max_idle_frames`` + row accounting (+ figures for the non-vacuity guards).

    Expiry (rtmodt.h, rtmodt_zones_create): at the start of ``process(frame_id)`` every id with
    ``frame_id - last_seen[id] > max_idle_frames`` loses its row, i.e. all its (id, zone) cooldown entries -- an id in
    this frame's list included.  ``None``: never.  A row exists for every id passed and not yet expired; after a frame
    ``rows = n_passed + n_retained_idle``; ``overflow`` = the first frame id at which that exceeded 2 x max_tracks."""

    def __init__(self, zone_configs, max_tracks, max_idle_frames=None):
        super().__init__(zone_configs)
        for z in self.zones:
            z["polygon"] = interned(z["polygon"])
        self.cap = 2 * int(max_tracks)
        self.max_idle = max_idle_frames
        self.last_seen = {}
        self.rows = 0
        self.overflow = None
        self._prev_passed = set()
        self._ever_seen = {}                # id -> frame it was last passed in, kept past expiry (bookkeeping for the guards)
        self._lost_cd = {}                  # (id, zone name) -> the last_alert that expiry dropped
        names = [z["name"] for z in self.zones]
        self._min_cooldown = {n: min(z["cooldown_sec"] for z in self.zones if z["name"] == n) for n in names}
        self._solo = {z["name"]: z for z in self.zones if names.count(z["name"]) == 1}
        # figures for the guards, all derived from this model's own state
        self.history = []                   # per call: (n_passed, n_retained_idle, rows)
        self.n_events = 0
        self.events_by_zone = {}
        self.returned_expired = 0           # (id, call): returned with frame_id - last_seen > max_idle
        self.refired_after_expiry = 0       # ... and fired where the dropped cooldown entry would still have held
        self.returned_live = 0              # (id, call): returned after >= 1 call away, row still there
        self.suppressed_on_return = 0       # ... and a kept cooldown entry suppressed an event that was otherwise due
        self.exact_threshold_firings = 0    # events with now - first == dwell or now - last == cooldown, exactly
        self.tracker_expired = 0
        self.max_tracker_rows = 0

    # -- host-fed source (rtmodt_zones_process) ------------------------------------------------------
    def process(self, tracks, frame_id: int, now: float):
        tracks = list(tracks)
        passed = set(int(t[0]) for t in tracks)
        assert len(passed) == len(tracks), "duplicate track id"
        returning = set(i for i in passed if i in self._ever_seen and i not in self._prev_passed)
        ret_exp = set()
        if self.max_idle is not None:
            dead = set(i for i, seen in self.last_seen.items() if frame_id - seen > self.max_idle)
            for i in dead:
                del self.last_seen[i]
            if dead:
                for key in [k for k in self.cooldown if k[0] in dead]:
                    self._lost_cd[key] = self.cooldown.pop(key)
            ret_exp = set(i for i in returning if frame_id - self._ever_seen[i] > self.max_idle)
            returning -= ret_exp
            self.returned_expired += len(ret_exp)
        dropped = self._lost_cd
        before_cd = dict(self.cooldown) if len(tracks) <= 64 else None        # small scenarios only: exact-threshold figures
        with memoised_pip():
            events = super().process(tracks, frame_id, now)
        self._account(events, now, ret_exp, dropped, returning, before_cd)
        for i in passed:
            self.last_seen[i] = self._ever_seen[i] = frame_id
        self.rows = len(self.last_seen)
        self.history.append((len(passed), self.rows - len(passed), self.rows))
        if self.rows > self.cap and self.overflow is None:
            self.overflow = frame_id
        self._prev_passed = passed
        return events

    def _account(self, events, now, ret_exp, dropped, returning, before_cd):
        self.n_events += len(events)
        fired = set()
        refired = set()
        for e in events:
            key = (e["track_id"], e["zone_name"])
            fired.add(key)
            self.events_by_zone[e["zone_name"]] = self.events_by_zone.get(e["zone_name"], 0) + 1
            if key in dropped and now - dropped[key] < self._min_cooldown[key[1]]:
                refired.add(key[0])
            z = self._solo.get(key[1])
            if z is not None and before_cd is not None:
                first = self.occupancy[key[0]][key[1]]
                if now - first == z["dwell_time_sec"] or (key in before_cd and now - before_cd[key] == z["cooldown_sec"]):
                    self.exact_threshold_firings += 1
        self.refired_after_expiry += len(refired & ret_exp)
        self.returned_live += len(returning)
        for i in returning:                      # inside, dwell met, an entry kept, no event: only the cooldown can have held it
            for name, first in self.occupancy.get(i, {}).items():
                z = self._solo.get(name)
                if z is not None and now - first >= z["dwell_time_sec"] and (i, name) in self.cooldown and (i, name) not in fired:
                    self.suppressed_on_return += 1
                    break

    # -- tracker source (rtmodt_zones_process_tracker) -----------------------------------------------
    def process_tracker(self, ids, tsu, xyxy, cls, report_tsu: int, frame_id: int, now: float):
        """The tracker's whole list is present; passed = ``tsu == report_tsu``; an id the tracker no longer lists loses
        its row at once (``max_idle = -1``)."""
        listed = set(int(i) for i in ids)
        dead = set(self.last_seen) - listed
        self.tracker_expired += len(dead)
        for i in dead:
            del self.last_seen[i]
        if dead:
            for key in [k for k in self.cooldown if k[0] in dead]:
                del self.cooldown[key]
        tracks = [(int(i), xyxy[j], int(cls[j])) for j, i in enumerate(ids) if tsu[j] == report_tsu]
        with memoised_pip():
            events = super().process(tracks, frame_id, now)
        self.n_events += len(events)
        passed = set(t[0] for t in tracks)
        for i in listed:
            if i in passed or i not in self.last_seen:
                self.last_seen[i] = frame_id
        self.rows = len(listed)
        self.max_tracker_rows = max(self.max_tracker_rows, self.rows)
        self.history.append((len(passed), self.rows - len(passed), self.rows))
        return events


# ------------------------------------------------------------------------------------------------ scenario helpers
LATTICE = 16


def _box(cx, cy, w, h):
    """float32 box whose centroid is exactly (cx, cy) (w / 2 and h / 2 are exact in float32 at this size)."""
    return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], np.float32)


def ngon(cx, cy, r, k, phase=0.0):
    a = phase + 2 * np.pi * np.arange(k) / k
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).round().astype(np.int64).tolist()


# ------------------------------------------------------------------------------------------------ a. churn at scale
CHURN_IDLE = (None, 0, 3, 40)
CHURN_ZONES = [
    {"name": "A", "polygon": [[64, 64], [320, 64], [320, 240], [64, 240]], "dwell_time_sec": 0.0, "cooldown_sec": 1e9},
    {"name": "B", "polygon": [[336, 48], [592, 48], [592, 304], [464, 176], [336, 304]], "dwell_time_sec": 0.0, "cooldown_sec": 0.0},   # concave
    {"name": "A", "polygon": [[256, 192], [448, 192], [448, 400], [256, 400]], "dwell_time_sec": 0.5, "cooldown_sec": 2.0},
    {"name": "C", "polygon": [[96, 288], [272, 464]], "dwell_time_sec": 0.0, "cooldown_sec": 30.0},                                     # 2 points
    {"name": "D", "polygon": [[0, 0], [640, 0], [640, 480], [0, 480]], "dwell_time_sec": 1.0, "cooldown_sec": 0.7, "trigger": "loitering"},
    {"name": "C", "polygon": [[480, 320], [624, 320], [624, 464]], "dwell_time_sec": 0.0, "cooldown_sec": 30.0},
    {"name": "E", "polygon": [[32, 256], [240, 256], [240, 448], [32, 448]], "dwell_time_sec": 0.0, "cooldown_sec": 30.0},
    {"name": "F", "polygon": [[400, 16], [560, 32], [608, 160], [496, 240], [384, 128]], "dwell_time_sec": 0.3, "cooldown_sec": 0.0},
]
CHURN = dict(n_streams=3, max_tracks=1024, max_events=8192, n_frames=120, pool=1500, long_leavers=300)


@functools.lru_cache(maxsize=None)
def churn_scenario():
    """Three streams, each its own seed: a pool of 1500 int64 ids (negative and > 2^32 among them), each id present for
    1-5 calls then away for 1-12; 300 of them leave once for 45-60 calls; 300-700 passed per call in shuffled order;
    frame ids advance by 1 and now and then by 5; uneven clock ticks from 1.7e9.  Returns the calls in the interleaved
    order they are made: ``(stream, frame_id, now, [(id, xyxy, cls), ...])``."""
    S, F, P = CHURN["n_streams"], CHURN["n_frames"], CHURN["pool"]
    per_stream = []
    for s in range(S):
        rng = np.random.default_rng(9100 + s)
        ids = np.unique(rng.integers(-(1 << 40), 1 << 40, size=P + 50))[:P]
        rng.shuffle(ids)
        cls = rng.integers(0, 80, size=P)
        wh = rng.choice([20, 30, 41], size=(P, 2))
        gx, gy = rng.integers(0, 640 // LATTICE, size=P), rng.integers(0, 480 // LATTICE, size=P)
        present = rng.random(P) < 0.3
        left = np.where(present, rng.integers(1, 6, size=P), rng.integers(1, 13, size=P))   # calls left in the current run
        long_at = np.full(P, -1)
        long_at[:CHURN["long_leavers"]] = rng.integers(15, 45, size=CHURN["long_leavers"])
        frame_id, now, calls = int(rng.integers(0, 1000)), 1.7e9 + float(rng.random()), []
        for f in range(F):
            frame_id += 5 if rng.random() < 0.1 else 1
            now += float(rng.uniform(0.01, 0.4))
            go_long = long_at == f
            present[go_long], left[go_long] = False, rng.integers(45, 61, size=int(go_long.sum()))
            idx = np.nonzero(present)[0]
            if len(idx) > 700:
                idx = idx[:700]
            assert 300 <= len(idx) <= 700, len(idx)
            step = rng.integers(-1, 2, size=(len(idx), 2))                                   # a present id drifts over the lattice
            gx[idx] = np.clip(gx[idx] + step[:, 0], 0, 640 // LATTICE - 1)
            gy[idx] = np.clip(gy[idx] + step[:, 1], 0, 480 // LATTICE - 1)
            order = rng.permutation(idx)                                                     # caller order: not id order
            calls.append((frame_id, now, [(int(ids[i]), _box(int(gx[i]) * LATTICE, int(gy[i]) * LATTICE, int(wh[i, 0]), int(wh[i, 1])), int(cls[i]))
                                          for i in order]))
            left -= 1
            flip = left <= 0
            present = np.where(flip, ~present, present)
            left = np.where(flip, np.where(present, rng.integers(1, 6, size=P), rng.integers(1, 13, size=P)), left)
        per_stream.append(calls)
    rng = np.random.default_rng(9199)
    out = []
    for f in range(F):
        for s in rng.permutation(S):
            out.append((int(s),) + per_stream[int(s)][f])
    return out


def churn_guards(models, max_idle):
    """Section 4 of the issue, row a, from the per-stream models of one run."""
    fig = dict(max_retained=max(h[1] for m in models for h in m.history),
               big_frames=sum(1 for m in models for h in m.history if h[2] > 512 and h[0] > 256),
               returned_expired=sum(m.returned_expired for m in models), refired=sum(m.refired_after_expiry for m in models),
               returned_live=sum(m.returned_live for m in models), suppressed=sum(m.suppressed_on_return for m in models),
               events=sum(m.n_events for m in models), overflow=[m.overflow for m in models])
    assert fig["overflow"] == [None] * len(models), fig
    assert fig["events"] > 2000, fig
    if max_idle is not None and max_idle >= 3:
        assert fig["max_retained"] > 256 and fig["big_frames"] >= 1, fig
    if max_idle is not None:                       # None never expires: nothing can return after an expired gap
        assert fig["returned_expired"] >= 50 and fig["refired"] >= 10, fig
    if max_idle != 0:                              # 0: a return means frame_id - last_seen >= 2 > 0, never within the limit
        assert fig["returned_live"] >= 50 and fig["suppressed"] >= 50, fig
    return fig


# ------------------------------------------------------------------------------------------------ b. 32 zones, full point table
FULL = dict(max_tracks=1024, max_events=16384, max_idle=5, n_frames=40, n_tracks=600, pool=900)


@functools.lru_cache(maxsize=None)
def full_table_zones(shared_names: bool):
    """32 zones on a 640 x 480 canvas: a star of 1500 vertices, a 0-point, a 1-point and a repeated-vertex polygon, the
    rest 16-gons; 1900 < points <= 2048.  ``shared_names``: names z{i % 11} (groups of three share a key)."""
    star_a = 2 * np.pi * np.arange(1500) / 1500
    star_r = np.where(np.arange(1500) % 2 == 0, 210.0, 130.0)
    star = np.stack([320 + star_r * np.cos(star_a), 240 + star_r * np.sin(star_a)], 1).round().astype(np.int64).tolist()
    rng = np.random.default_rng(77)
    zones = []
    for i in range(32):
        if i == 3:
            poly = star
        elif i == 7:
            poly = []
        elif i == 12:
            poly = [[320, 256]]                                                             # a lattice point
        elif i == 18:
            poly = [[100, 100], [260, 100], [260, 100], [300, 260], [80, 300]]              # repeated vertex
        else:
            cx, cy = int(rng.integers(5, 36)) * LATTICE, int(rng.integers(5, 26)) * LATTICE
            poly = ngon(cx, cy, int(rng.integers(3, 9)) * LATTICE, 16, phase=float(rng.random()))
        zones.append({"name": f"z{i % 11}" if shared_names else f"zone{i}", "polygon": poly, "trigger": "intrusion" if i % 3 else "loitering",
                      "dwell_time_sec": [0.0, 0.0, 0.4, 1.0][i % 4], "cooldown_sec": [0.0, 1.5, 0.5, 1e9, 3.0][i % 5]})
    zones[31]["polygon"] = ngon(480, 160, 96, 16)                                           # zone 31 fires at once: dwell 0
    zones[31]["dwell_time_sec"] = 0.0
    n_pts = sum(len(z["polygon"]) for z in zones)
    assert 1900 < n_pts <= 2048, n_pts
    return zones


@functools.lru_cache(maxsize=None)
def full_table_calls():
    # centroids on a 32-pixel lattice: 300 distinct points, so that the 1500-vertex star is walked 300 times, not 24000
    rng = np.random.default_rng(501)
    P, N = FULL["pool"], FULL["n_tracks"]
    ids = rng.permutation(np.arange(1, P + 1) * 7)
    gx, gy = rng.integers(0, 640 // 32, size=P), rng.integers(0, 480 // 32, size=P)
    cls = rng.integers(0, 80, size=P)
    now, calls = 1.7e9, []
    for f in range(FULL["n_frames"]):
        now += float(rng.uniform(0.05, 0.3))
        idx = rng.choice(P, size=N, replace=False)                                          # two thirds of the pool: idle rows every frame
        step = rng.integers(-1, 2, size=(N, 2))
        gx[idx] = np.clip(gx[idx] + step[:, 0], 0, 640 // 32 - 1)
        gy[idx] = np.clip(gy[idx] + step[:, 1], 0, 480 // 32 - 1)
        calls.append((0, 100 + f, now, [(int(ids[i]), _box(int(gx[i]) * 32, int(gy[i]) * 32, 30, 41), int(cls[i])) for i in idx]))
    return calls


def full_table_guards(model, zones, calls, shared_names):
    fig = dict(events=model.n_events, zone31=model.events_by_zone.get("zone31", 0), max_retained=max(h[1] for h in model.history), split_group=0)
    assert fig["events"] > 2000 and fig["max_retained"] > 100 and model.overflow is None, fig
    if not shared_names:
        assert fig["zone31"] > 0, fig                                                       # key 31, event bit 31
    else:
        polys = [interned(z["polygon"]) for z in zones]
        groups = [[i for i in range(32) if i % 11 == g] for g in range(11)]
        for _, _, _, tracks in calls[:8]:
            for _, xyxy, _ in tracks:
                cx, cy = Z.centroid(xyxy)
                for g in groups:
                    flags = [_memo_pip(polys[i], cx, cy) >= 0 for i in g]
                    fig["split_group"] += any(flags) and not all(flags)
        assert fig["split_group"] > 100, fig                                                # one member inside, one outside, same frame
    return fig


# ------------------------------------------------------------------------------------------------ c. thresholds met exactly
THRESH_ZONES = [
    {"name": "all", "polygon": [[0, 0], [640, 0], [640, 480], [0, 480]], "dwell_time_sec": 0.5, "cooldown_sec": 1.0},
    {"name": "neg", "polygon": [[0, 0], [320, 0], [320, 480], [0, 480]], "dwell_time_sec": -1.0, "cooldown_sec": 0.75},   # negative dwell: due at once
    {"name": "right", "polygon": [[320, 0], [640, 0], [640, 480], [320, 480]], "dwell_time_sec": 0.25, "cooldown_sec": 0.5},
]


def threshold_calls(step: float):
    """40 calls, clock 1.7e9 + k * step (step 0.25: exact in double, so ``now - first == dwell`` and
    ``now - last == cooldown`` happen as equalities; step 0.1: the rounded differences fall on either side)."""
    rng = np.random.default_rng(31)
    enter = rng.integers(0, 8, size=24)
    away = rng.integers(12, 30, size=24)                  # one call away: the occupancy timer restarts, the cooldown entry stays
    calls = []
    for k in range(40):
        now = 1.7e9 + k * step
        tr = [(i + 1, _box(40 + 24 * i, 100 + 8 * i, 20, 20), i % 5) for i in range(24) if k >= enter[i] and k != away[i]]
        calls.append((0, k, now, tr))
    return calls


# ------------------------------------------------------------------------------------------------ d. centroids
# (x1, x2) per case -> int((x1 + x2) / 2) in float32, stated outright (tests/test_zone_ref_cpu.py checks the model's centroid against them)
CENTROID_CASES = [
    ((-7.5, -2.25), -4),                                  # -4.875: truncates toward zero, not down
    ((-0.75, 0.25), 0),                                   # -0.25 -> 0
    ((10.0, 11.0), 10),                                   # exact half 10.5
    ((-10.0, -11.0), -10),                                # exact half -10.5 -> -10
    ((16777218.0, 16777220.0), 16777220),                 # 2^24 + 2, 2^24 + 4: the float32 sum 2^25 + 6 rounds to 2^25 + 8 (true mean 2^24 + 3)
    ((33554432.0, 67108864.0), 50331648),                 # 2^25, 2^26: exact
    ((-67108800.0, -67108792.0), -67108796),              # just inside -2^26: sum -134217592 is a multiple of 8, exact
]


def centroid_scenario():
    """One track per case (its y taken from another case), five zero-dwell / zero-cooldown zones around each track's
    truncated centroid (vx, vy): a corner on it, an edge through it, and three that miss it by one pixel.
    |coordinate| <= 2^26, so the int32 differences of the point-in-polygon test stay far from overflow."""
    n = len(CENTROID_CASES)
    tracks, zones = [], []
    for i, ((x1, x2), vx) in enumerate(CENTROID_CASES[:6]):
        (y1, y2), vy = CENTROID_CASES[(i + 3) % n]
        tracks.append((i + 1, np.array([x1, y1, x2, y2], np.float32), i))
        rect = lambda ax, ay, bx, by: [[ax, ay], [bx, ay], [bx, by], [ax, by]]
        for k, poly in enumerate([rect(vx, vy, vx + 8, vy + 8),            # corner on the centroid: inside
                                  rect(vx + 1, vy - 4, vx + 9, vy + 4),    # starts one pixel to the right: outside
                                  rect(vx - 8, vy - 4, vx - 1, vy + 4),    # ends one pixel to the left: outside
                                  rect(vx - 8, vy - 8, vx, vy + 8),        # right edge through the centroid: inside
                                  rect(vx - 4, vy + 1, vx + 4, vy + 9)]):  # starts one pixel below: outside
            zones.append({"name": f"t{i}k{k}", "polygon": poly, "dwell_time_sec": 0.0, "cooldown_sec": 0.0})
    return zones, tracks


# ------------------------------------------------------------------------------------------------ e. ledger full
LEDGER_FULL_CALLS = [                                      # max_tracks = 8 -> 16 rows; ids never expire
    (0, [1, 2, 3, 4, 5]),                                  # rows 5
    (1, [6, 7, 8, 9, 10]),                                 # 5 + 5 idle = 10
    (2, [3, 11, 12, 13, 14, 15]),                          # 6 + 9 idle = 15
    (3, [16, 3]),                                          # 2 + 14 idle = 16: exactly full, passes
    (4, [17]),                                             # 1 + 16 idle = 17: ledger full
]

# ------------------------------------------------------------------------------------------------ expiry, by hand
# max_idle_frames = 3, one whole-canvas zone with dwell 0 and cooldown 1e9: an id fires once, then only after its row
# expired.  (frame_id, ids passed, ids that fire).  10/11/12 are fillers that keep a call on every frame.
EXPIRY_ZONE = [{"name": "all", "polygon": [[0, 0], [640, 0], [640, 480], [0, 480]], "dwell_time_sec": 0.0, "cooldown_sec": 1e9}]
EXPIRY_CASES = {
    "calls_on_every_frame": [
        (0, [1, 2, 10], [1, 2, 10]),
        (1, [10], []), (2, [10], []),
        (3, [1, 10], []),                                  # 3 - 0 = 3, not more than 3: silent
        (4, [2, 10], [2]),                                 # 4 - 0 = 4 > 3: forgotten, fires again
        (5, [1, 2], []),                                   # both rows are fresh again
    ],
    "frame_ids_jump": [                                    # no call in between: nothing could drop the row earlier
        (100, [1, 2, 3], [1, 2, 3]),
        (103, [1], []),                                    # gap 3: silent
        (104, [2], [2]),                                   # gap 4: fires
        (105, [3], [3]),                                   # gap 5: fires
        (110, [1, 2], [1, 2]),                             # jumps of 5: 110 - 103 = 7, 110 - 104 = 6: both fire
        (115, [1], [1]),                                   # passed on consecutive calls, but 5 frames apart: fires
        (118, [1], []),                                    # gap 3: silent
    ],
}
EXPIRY_ZERO = [                                            # max_idle_frames = 0
    (0, [1, 2], [1, 2]),
    (1, [2], [2]),                                         # 1 - 0 = 1 > 0: with 0 nothing outlives a frame
    (2, [1], [1]),                                         # skipped a single frame: forgotten
]


# ------------------------------------------------------------------------------------------------ f. tracker source at scale
TRACKER = dict(n_streams=4, max_dets=1024, max_tracks=2048, track_buffer=5, n_frames=60, boxes=(400, 470, 540, 600), canvas=1600,
               seed=640, burst=(1, 5), p_start=0.105)
TRACKER_ZONES = [
    {"name": "west", "polygon": [[0, 0], [700, 0], [700, 1600], [0, 1600]], "dwell_time_sec": 0.5, "cooldown_sec": 2.0},
    {"name": "core", "polygon": [[500, 500], [1100, 500], [1100, 1100], [800, 800], [500, 1100]], "dwell_time_sec": 0.0, "cooldown_sec": 1.0},
    {"name": "west", "polygon": [[600, 200], [900, 200], [900, 500], [600, 500]], "dwell_time_sec": 0.0, "cooldown_sec": 5.0},
    {"name": "south", "polygon": [[0, 1200], [1600, 1200], [1600, 1600], [0, 1600]], "dwell_time_sec": 1.0, "cooldown_sec": 1e9, "trigger": "loitering"},
]


def tracker_inputs(box_sequence):
    """Per frame and stream the detections that survive the dropout: ``frames[f][s] = (xyxy, conf, cls)``, plus the
    clock.  A detection drops out for 1-4 frames at a time (an occlusion), 15-30 % of them in every frame: a track that
    misses its box for a few frames often fails the IoU gate when the box returns, lingers as a lost track next to the
    one spawned in its place, and expires from the middle of the list.  ``box_sequence`` is the package's
    ``synth.box_sequence`` (pure NumPy); its confidences U(0.36, 0.99) are squeezed to U(0.45, 0.99): only a detection at
    or above 0.5 can spawn a track, and with 22 % of 600 boxes below it no stream could reach 512 rows.  One in eleven
    still goes through the low-confidence second association."""
    S, F = TRACKER["n_streams"], TRACKER["n_frames"] + 1                    # + 1: the closing report="reference" call
    seqs = [box_sequence(TRACKER["boxes"][s], TRACKER["canvas"], F, seed=TRACKER["seed"] + s) for s in range(S)]
    rng = np.random.default_rng(12)
    out_for = [np.where(rng.random(TRACKER["boxes"][s]) < 0.12, rng.integers(*TRACKER["burst"], size=TRACKER["boxes"][s]), 0) for s in range(S)]
    frames, clock, now = [], [], 1.7e9
    for f in range(F):
        now += float(rng.uniform(0.05, 0.3))
        per = []
        for s in range(S):
            xy, cf, cl = seqs[s]
            cf = (np.float32(0.45) + (cf - np.float32(0.36)) * np.float32(0.54 / 0.63)).astype(np.float32)   # U(0.36, 0.99) -> U(0.45, 0.99)
            n = len(cf)
            start = (out_for[s] == 0) & (rng.random(n) < TRACKER["p_start"])
            out_for[s] = np.where(start, rng.integers(*TRACKER["burst"], size=n), out_for[s])
            keep = out_for[s] == 0
            assert 0.15 <= 1.0 - keep.mean() <= 0.30, (f, s, 1.0 - keep.mean())
            out_for[s] = np.maximum(out_for[s] - 1, 0)
            per.append((xy[f][keep], cf[keep], cl[keep]))
        frames.append(per)
        clock.append(now)
    return frames, clock


def tracker_guards(models):
    fig = dict(max_rows=max(m.max_tracker_rows for m in models), expired=sum(m.tracker_expired for m in models), events=sum(m.n_events for m in models))
    assert fig["max_rows"] > 512 and fig["expired"] > 100 and fig["events"] > 200, fig
    return fig
