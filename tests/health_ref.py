"""The camera-health monitor's rules restated in NumPy: the definition ``csrc/health.hip`` and ``csrc/health_rule.h`` are pinned to with
``==`` (every rule is integer arithmetic).  PARITY UNPINNED: the reference has no counterpart, no camera's or NVR's tamper detection
is available to compare with, and no default has been validated on real footage.

Rules.  Grid, pixel luma and cell luma ``Y`` are the motion detector's (``tests/motion_ref.py`` rule 1).
  1. ``F[cy][cx]`` = the sum of ``|y(x + 1, yy) - y(x, yy)|`` over the cell's pixels with ``x + 1 < w`` (``y``: pixel luma); ``sharp = sum F``.
  2. ``G = min(255, |Y[cy][cx+1] - Y[cy][cx-1]| + |Y[cy+1][cx] - Y[cy-1][cx]|)`` for interior cells, else 0.  Edge: ``G >= edge_threshold``;
     weak edge: ``2 G >= edge_threshold``.
  3. Counts: ``luma_sum``, ``n_dark`` (``Y <= dark_level``), ``n_bright`` (``Y >= bright_level``), ``n_changed`` (``Y`` differs from the previous
     grid; every cell when ``frames_seen == 0``), ``n_edge``, ``n_ref_edge`` (``R >= edge_threshold << 8``, ``R`` as it was at entry),
     ``n_kept`` (reference edge and weak edge now).
  4. Raw conditions (a per-mille parameter of 0 disables one, ``freeze_frames == 0`` disables FROZEN).  With ``frames_seen >= warmup`` at
     entry: DARK ``1000 n_dark >= dark_pm cells``; BRIGHT likewise; and with ``n_ref_edge >= min_ref_edges`` (else the bit NO_STRUCTURE):
     ``lost = 1000 n_kept < retain_pm n_ref_edge``; COVERED ``lost and 1000 n_edge < cover_pm n_ref_edge``; MOVED ``lost and not COVERED``;
     DEFOCUSED ``not lost and 1000 sharp < defocus_pm (ref_sharp >> 8)``.  FROZEN: ``frames_seen >= 1 and n_changed <= freeze_cells``.
  5. Debounce, per condition in condition order.  Inactive: ``run`` counts consecutive raw frames; at ``hold_frames`` (FROZEN:
     ``freeze_frames``) the condition becomes active, RAISED, ``run = off = 0``.  Active: ``run`` counts the frames since (its age), ``off`` the
     consecutive frames without the raw condition; at ``clear_frames`` (FROZEN: 1) it becomes inactive, CLEARED, ``run = off = 0``.
  6. Relearn: ``relearn_frames > 0`` and an active structure condition of age ``>= relearn_frames`` -> a rebase: CLEARED for each active
     structure condition in condition order, REBASED (condition -1), their counters 0, ``frames_seen = 0``.  ``rebase(stream)`` does the same
     at once and owes its events to the stream's next call, which reports them first.
  7. Learning runs iff ``frames_seen < warmup`` at entry, or no raw exposure or structure condition holds and none is active after
     step 5.  ``frames_seen == 0``: ``R = G << 8``, ``ref_sharp = sharp << 8``; else ``R += ((G << 8) - R) >> ref_shift`` and the same for
     ``ref_sharp`` (arithmetic shifts).  Then ``frames_seen = min(frames_seen + 1, 2 ** 30)`` unless step 6 set it to 0.
"""
import numpy as np

import motion_ref as MR

DARK, BRIGHT, COVERED, MOVED, DEFOCUSED, FROZEN = range(6)
NAMES = ("dark", "bright", "covered", "moved", "defocused", "frozen")
N_COND = 6
NO_STRUCTURE = 1 << 6
EXPOSURE = 1 << DARK | 1 << BRIGHT
STRUCTURE = 1 << COVERED | 1 << MOVED | 1 << DEFOCUSED
RAISED, CLEARED, REBASED = 1, 2, 3
PENDING_REBASE = 1 << 8
LEARN_NONE, LEARN_AVERAGE, LEARN_SET = 0, 1, 2
MAX_EVENTS = 8
MAX_COUNT = 2 ** 30
#: none of these has been validated on real footage
DEFAULTS = dict(scale=4, edge_threshold=24, ref_shift=6, warmup=25, dark_level=16, dark_pm=950, bright_level=240, bright_pm=950, retain_pm=500,
                cover_pm=300, defocus_pm=500, min_ref_edges=16, hold_frames=25, clear_frames=25, freeze_frames=50, freeze_cells=0, relearn_frames=0)
COUNTS = ("luma_sum", "sharp", "n_dark", "n_bright", "n_changed", "n_edge", "n_ref_edge", "n_kept")


def config(**kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise TypeError(k)
        c[k] = int(v)
    return c


def names_of(mask):
    return tuple(n for i, n in enumerate(NAMES) if mask >> i & 1)


# ---- 1. fine detail ----------------------------------------------------------------------------------------------------
def fine_detail(frame, scale):
    y = MR.pixel_luma(frame)
    h, w = y.shape
    gh, gw = MR.grid_shape(h, w, scale)
    pad = np.zeros((gh * scale, gw * scale), np.int64)
    pad[:h, :w - 1] = np.abs(y[:, 1:] - y[:, :-1])
    return pad.reshape(gh, scale, gw, scale).sum((1, 3))


def fine_detail_loop(frame, scale):
    h, w = frame.shape[:2]
    gh, gw = MR.grid_shape(h, w, scale)
    y = [[(19595 * int(p[2]) + 38470 * int(p[1]) + 7471 * int(p[0]) + 32768) >> 16 for p in row] for row in frame]
    out = np.zeros((gh, gw), np.int64)
    for yy in range(h):
        for x in range(w):
            if x + 1 < w:
                out[yy // scale, x // scale] += abs(y[yy][x + 1] - y[yy][x])
    return out


# ---- 2. coarse structure -----------------------------------------------------------------------------------------------
def coarse(yc):
    yc = np.asarray(yc, np.int64)
    g = np.zeros(yc.shape, np.int64)
    if yc.shape[0] >= 3 and yc.shape[1] >= 3:
        g[1:-1, 1:-1] = np.minimum(255, np.abs(yc[1:-1, 2:] - yc[1:-1, :-2]) + np.abs(yc[2:, 1:-1] - yc[:-2, 1:-1]))
    return g


def coarse_loop(yc):
    gh, gw = np.asarray(yc).shape
    g = np.zeros((gh, gw), np.int64)
    for cy in range(1, gh - 1):
        for cx in range(1, gw - 1):
            g[cy, cx] = min(255, abs(int(yc[cy][cx + 1]) - int(yc[cy][cx - 1])) + abs(int(yc[cy + 1][cx]) - int(yc[cy - 1][cx])))
    return g


# ---- 3. counts ---------------------------------------------------------------------------------------------------------
def counts_of(yc, f, g, prev, r, seen, c):
    t = c["edge_threshold"]
    ref_edge = r >= t << 8
    return dict(luma_sum=int(yc.sum()), sharp=int(f.sum()), n_dark=int((yc <= c["dark_level"]).sum()), n_bright=int((yc >= c["bright_level"]).sum()),
                n_changed=int(yc.size if seen == 0 else (yc != prev).sum()), n_edge=int((g >= t).sum()), n_ref_edge=int(ref_edge.sum()),
                n_kept=int((ref_edge & (2 * g >= t)).sum()))


# ---- 4. raw conditions -------------------------------------------------------------------------------------------------
def raw_of(k, cells, seen, ref_sharp, c):
    raw = 0
    if seen >= c["warmup"]:
        if c["dark_pm"] and 1000 * k["n_dark"] >= c["dark_pm"] * cells:
            raw |= 1 << DARK
        if c["bright_pm"] and 1000 * k["n_bright"] >= c["bright_pm"] * cells:
            raw |= 1 << BRIGHT
        if k["n_ref_edge"] < c["min_ref_edges"]:
            raw |= NO_STRUCTURE
        else:
            lost = 1000 * k["n_kept"] < c["retain_pm"] * k["n_ref_edge"]
            covered = lost and 1000 * k["n_edge"] < c["cover_pm"] * k["n_ref_edge"]
            if covered:                                      # (retain_pm, cover_pm or defocus_pm of 0: the comparison cannot hold)
                raw |= 1 << COVERED
            if lost and not covered:
                raw |= 1 << MOVED
            if not lost and 1000 * k["sharp"] < c["defocus_pm"] * (ref_sharp >> 8):
                raw |= 1 << DEFOCUSED
    if c["freeze_frames"] and seen >= 1 and k["n_changed"] <= c["freeze_cells"]:
        raw |= 1 << FROZEN
    return raw


def fresh_state():
    return dict(ref_sharp=0, frames_seen=0, active=0, pending=0, run=[0] * N_COND, off=[0] * N_COND)


def rebase_state(st, events):
    """Step 6 on a state: the CLEARED events of the active structure conditions and REBASED go to ``events`` (condition, kind)."""
    for i in range(N_COND):
        if STRUCTURE >> i & 1:
            if st["active"] >> i & 1:
                events.append((i, CLEARED))
            st["run"][i] = st["off"][i] = 0
    events.append((-1, REBASED))
    st["active"] &= ~STRUCTURE
    st["frames_seen"] = 0


def rebase_now(st):
    """``rebase(stream)``: the state is rebased at once, the events are owed to the next call."""
    ev = []
    rebase_state(st, ev)
    st["pending"] |= PENDING_REBASE | sum(1 << i for i, kind in ev if kind == CLEARED)


# ---- 5..7. one frame of one stream -------------------------------------------------------------------------------------
def decide(k, cells, st, c):
    """Counts ``k`` of one frame against the state ``st`` (updated in place) -> (raw, learn, [(condition, kind)])."""
    events = []
    if st["pending"]:
        events += [(i, CLEARED) for i in range(N_COND) if st["pending"] >> i & 1]
        if st["pending"] & PENDING_REBASE:
            events.append((-1, REBASED))
        st["pending"] = 0
    seen = st["frames_seen"]
    raw = raw_of(k, cells, seen, st["ref_sharp"], c)
    for i in range(N_COND):
        r = raw >> i & 1
        hold, clear = (c["freeze_frames"], 1) if i == FROZEN else (c["hold_frames"], c["clear_frames"])
        if not st["active"] >> i & 1:
            st["run"][i] = min(st["run"][i] + 1, MAX_COUNT) if r else 0
            st["off"][i] = 0
            if r and st["run"][i] >= hold:
                st["active"] |= 1 << i
                st["run"][i] = 0
                events.append((i, RAISED))
        else:
            st["run"][i] = min(st["run"][i] + 1, MAX_COUNT)
            st["off"][i] = 0 if r else min(st["off"][i] + 1, MAX_COUNT)
            if st["off"][i] >= clear:
                st["active"] &= ~(1 << i)
                st["run"][i] = st["off"][i] = 0
                events.append((i, CLEARED))
    learn = LEARN_NONE
    if seen < c["warmup"] or not (raw | st["active"]) & (EXPOSURE | STRUCTURE):
        learn = LEARN_SET if seen == 0 else LEARN_AVERAGE
        st["ref_sharp"] = k["sharp"] << 8 if seen == 0 else st["ref_sharp"] + (((k["sharp"] << 8) - st["ref_sharp"]) >> c["ref_shift"])
    st["frames_seen"] = min(seen + 1, MAX_COUNT)
    if c["relearn_frames"] > 0 and any(st["active"] >> i & 1 and st["run"][i] >= c["relearn_frames"] for i in range(N_COND) if STRUCTURE >> i & 1):
        rebase_state(st, events)
    assert len(events) <= MAX_EVENTS
    return raw, learn, events


def learn_r(r, g, learn, c):
    if learn == LEARN_SET:
        return g << 8
    if learn == LEARN_AVERAGE:
        return r + (((g << 8) - r) >> c["ref_shift"])
    return r


class Ref:
    """What a ``CameraHealth(streams, height, width, **cfg)`` holds and answers."""

    def __init__(self, streams, height, width, **cfg):
        self.c = config(**cfg)
        self.streams, self.h, self.w = streams, height, width
        self.gh, self.gw = MR.grid_shape(height, width, self.c["scale"])
        self.r = np.zeros((streams, self.gh, self.gw), np.int64)
        self.prev = np.zeros_like(self.r)
        self.st = [fresh_state() for _ in range(streams)]
        self.frame_no = [0] * streams

    def step(self, s, frame, frame_id=None):
        c, st = self.c, self.st[s]
        if frame_id is None:
            frame_id = self.frame_no[s]
        self.frame_no[s] = frame_id + 1
        yc = MR.cell_luma(frame, c["scale"])
        g = coarse(yc)
        k = counts_of(yc, fine_detail(frame, c["scale"]), g, self.prev[s], self.r[s], st["frames_seen"], c)
        raw, learn, ev = decide(k, self.gh * self.gw, st, c)
        self.r[s] = learn_r(self.r[s], g, learn, c)
        self.prev[s] = yc
        return dict(k, stream=s, raw=raw, active=st["active"], frames_seen=st["frames_seen"], ref_sharp=st["ref_sharp"], learned=learn,
                    events=[(cond, kind, frame_id) for cond, kind in ev])

    def process(self, frames, streams=None, frame_ids=None):
        streams = range(self.streams) if streams is None else streams
        ids = [None] * len(frames) if frame_ids is None else frame_ids
        return [self.step(s, f, i) for s, f, i in zip(streams, frames, ids)]

    def state(self, s):
        st = self.st[s]
        return dict(r=self.r[s].astype(np.uint16), prev=self.prev[s].astype(np.uint8), ref_sharp=st["ref_sharp"], frames_seen=st["frames_seen"],
                    active=st["active"], pending=st["pending"], run=tuple(st["run"]), off=tuple(st["off"]))

    def load_state(self, state, s=0):
        self.r[s], self.prev[s] = np.asarray(state["r"], np.int64), np.asarray(state["prev"], np.int64)
        self.st[s] = dict(ref_sharp=int(state["ref_sharp"]), frames_seen=int(state["frames_seen"]), active=int(state["active"]),
                          pending=int(state["pending"]), run=list(state["run"]), off=list(state["off"]))

    def rebase(self, s):
        rebase_now(self.st[s])

    def reset(self, s=None):
        for k in (range(self.streams) if s is None else [s]):
            self.r[k] = 0; self.prev[k] = 0; self.st[k] = fresh_state()
