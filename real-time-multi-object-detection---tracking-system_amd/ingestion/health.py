"""Camera health on MI355X: is the picture a stream delivers still a valid picture of the scene the camera was aimed at?  Per stream
a reference of the scene's coarse structure and fine detail, resident on the device, is compared with a batch of frames in one call
and answers six conditions -- dark, bright, covered, moved, defocused, frozen -- debounced into latched RAISED / CLEARED events: what
cameras and NVRs ship as "tamper detection" and "video loss".  ``pipeline.run(health=...)`` runs it directly after ``decode``; it
gates nothing, what to do with an alarm is the caller's decision.  The reference hands ``cap.read()``'s frame on
(``rtsp_reader.py``) and its events come from tracks only: it has no counterpart.

The work runs in ``csrc/health.hip`` (rules in ``csrc/health_rule.h``); there is no CPU implementation here.
``tests/health_ref.py`` restates every rule and the kernels equal it exactly: all of it is integer arithmetic.  Unpinned: parity with
any camera's or NVR's tamper detection, and every default -- none has been validated on real footage.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import _ffi

DARK, BRIGHT, COVERED, MOVED, DEFOCUSED, FROZEN = range(6)
CONDITION_NAMES = ("dark", "bright", "covered", "moved", "defocused", "frozen")
NO_STRUCTURE = 64
RAISED, CLEARED, REBASED = 1, 2, 3
KIND_NAMES = {RAISED: "raised", CLEARED: "cleared", REBASED: "rebased"}
MAX_EVENTS = 8
CFG_FIELDS = ("scale", "edge_threshold", "ref_shift", "warmup", "dark_level", "dark_pm", "bright_level", "bright_pm", "retain_pm", "cover_pm",
              "defocus_pm", "min_ref_edges", "hold_frames", "clear_frames", "freeze_frames", "freeze_cells", "relearn_frames")
COUNT_FIELDS = ("luma_sum", "sharp", "n_dark", "n_bright", "n_changed", "n_edge", "n_ref_edge", "n_kept")


def make_cfg(streams=1, height=0, width=0, device=0, **cfg) -> "_ffi.HealthCfg":
    """``rtmodt_health_default_cfg`` with the given fields replaced."""
    c = _ffi.HealthCfg()
    _ffi.lib().rtmodt_health_default_cfg(C.byref(c))
    c.streams, c.height, c.width, c.device = int(streams), int(height), int(width), _ffi.device_ordinal(device)
    for k, v in cfg.items():
        if k not in CFG_FIELDS:
            raise TypeError(f"unknown health parameter {k!r}; one of {CFG_FIELDS}")
        setattr(c, k, int(v))
    return c


def condition_names(mask: int) -> Tuple[str, ...]:
    return tuple(n for i, n in enumerate(CONDITION_NAMES) if mask >> i & 1)


@dataclass
class HealthEvent:
    condition: int                  # DARK .. FROZEN; -1 for REBASED
    kind: int                       # RAISED, CLEARED, REBASED
    frame_id: int

    @property
    def name(self) -> str:
        return (CONDITION_NAMES[self.condition] + " " if self.condition >= 0 else "") + KIND_NAMES[self.kind]


@dataclass
class HealthState:
    """What a stream holds between frames (``CameraHealth.state`` / ``load_state``): ``r`` is ``uint16 (gh, gw)`` in 8.8 fixed point,
    ``prev`` the previous luma grid, ``uint8 (gh, gw)``; ``pending`` the events a ``rebase`` owes the next call."""
    r: np.ndarray
    prev: np.ndarray
    ref_sharp: int
    frames_seen: int
    active: int
    pending: int
    run: Tuple[int, ...]
    off: Tuple[int, ...]


@dataclass
class HealthResult:
    """One stream's answer for one frame.  ``raw``: the conditions this frame shows (and ``NO_STRUCTURE``); ``active``: the latched ones;
    ``ref_sharp`` has 8 fractional bits; ``learned``: 0 the reference stood still, 1 it averaged this frame in, 2 it was set from it."""
    stream: int
    raw: int
    active: int
    names: Tuple[str, ...]
    luma_sum: int
    sharp: int
    n_dark: int
    n_bright: int
    n_changed: int
    n_edge: int
    n_ref_edge: int
    n_kept: int
    mean_luma: float
    ref_sharp: int
    frames_seen: int
    learned: int
    events: List[HealthEvent] = field(default_factory=list)

    @property
    def no_structure(self) -> bool:
        return bool(self.raw & NO_STRUCTURE)


def _state_struct(ref_sharp, frames_seen, active, pending, run, off) -> "_ffi.HealthState":
    st = _ffi.HealthState()
    st.ref_sharp, st.frames_seen, st.active, st.pending = int(ref_sharp), int(frames_seen), int(active), int(pending)
    if len(run) != 6 or len(off) != 6:
        raise ValueError("run and off hold one counter per condition, six each")
    for i in range(6):
        st.run[i], st.off[i] = int(run[i]), int(off[i])
    return st


def health_decide(counts: dict, cells: int, state: dict, frame_id: int = 0, **cfg):
    """``rtmodt_health_decide`` (host only): ``csrc/health_rule.h``'s decision, debounce and relearn on one row of counts
    (``COUNT_FIELDS``) and one state (``ref_sharp``, ``frames_seen``, ``active``, ``pending``, ``run``, ``off``) under the rule fields of ``cfg``
    -> (raw, learned, [(condition, kind, frame_id)], the new state as a dict)."""
    c = make_cfg(1, 1, 1, **cfg)
    row = _ffi.HealthResult()
    for k in COUNT_FIELDS:
        setattr(row, k, int(counts[k]))
    st = _state_struct(state["ref_sharp"], state["frames_seen"], state["active"], state["pending"], state["run"], state["off"])
    ev = (_ffi.HealthEvent * MAX_EVENTS)()
    _ffi.check(_ffi.lib().rtmodt_health_decide(C.byref(c), int(cells), int(frame_id), C.byref(row), C.byref(st), ev))
    new = dict(ref_sharp=st.ref_sharp, frames_seen=st.frames_seen, active=st.active, pending=st.pending, run=list(st.run), off=list(st.off))
    assert (row.frames_seen, row.active, row.ref_sharp) == (st.frames_seen, st.active, st.ref_sharp)
    return row.raw, row.learned, [(e.condition, e.kind, e.frame_id) for e in ev[:row.n_events]], new


class CameraHealth(_ffi.Handle):
    """``streams`` camera-health monitors for ``height x width`` BGR24 frames.

    ``scale`` (1, 2, 4, 8): pixels per cell side of the luma grid.  A cell is an edge when its coarse gradient reaches
    ``edge_threshold`` (1..255).  The reference follows the scene by ``>> ref_shift`` (1..12) per frame, after ``warmup`` (1..255) frames
    that only learn, and never learns a tampered picture.  ``dark_level`` / ``dark_pm`` and ``bright_level`` / ``bright_pm``: a cell at or
    beyond the level, and the per mille of such cells that makes the picture dark or bright.  The reference's structure is lost when
    fewer than ``retain_pm`` per mille of its edges are kept; the picture is then covered if it has fewer than ``cover_pm`` per mille as
    many edges of its own, else moved.  With the structure in place, fine detail below ``defocus_pm`` per mille of the reference's is
    defocused.  The structure tests need ``min_ref_edges`` reference edges.  A per-mille of 0 switches its condition off.  A condition
    is raised after ``hold_frames`` consecutive frames and cleared after ``clear_frames`` without it; a frame with at most ``freeze_cells``
    changed cells is a repeated one, ``freeze_frames`` of them are FROZEN (0: off), which clears on the first changed frame.
    ``relearn_frames`` > 0: a structure condition active that long rebases the stream -- the new view becomes the reference.

    None of the defaults has been validated on real footage."""

    def __init__(self, streams: int, height: int, width: int, *, device=0, **cfg) -> None:
        self._h = None
        self._cfg = make_cfg(streams, height, width, device, **cfg)
        self.streams, self.height, self.width = int(streams), int(height), int(width)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_health_create(C.byref(self._cfg), C.byref(h)))
        self._h = h
        self.scale = self._cfg.scale
        self.grid_shape = (-(-self.height // self.scale), -(-self.width // self.scale))
        self._frame_no = [0] * self.streams         # the frame_id a stream's next frame carries when the caller gives none

    def process(self, frames, streams: Optional[Sequence[int]] = None, frame_ids: Optional[Sequence[int]] = None, *, stride: Optional[int] = None,
                offset: int = 0) -> List[HealthResult]:
        """One frame for each of the named streams (None: one per stream, in order): host arrays (H x W x 3 uint8, rows may be
        padded) or a ``_ffi.DeviceBuffer`` holding the frames one after another from ``offset``, rows ``stride`` bytes apart.  The
        frames are only read.  ``frame_ids``: the number each frame's events carry (None: the stream's own count of frames).
        Streams that are not named keep their state."""
        n = self.streams if streams is None else len(streams)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=self.height, width=self.width, stride=stride, offset=offset, writable=False)
        if n == 0:
            return []
        if frame_ids is not None and len(frame_ids) != n:
            raise ValueError(f"{len(frame_ids)} frame ids for {n} frames")
        fp = (C.c_void_p * n)(*ptrs)
        sp = None if streams is None else np.ascontiguousarray(list(streams), np.int32)
        names = range(n) if streams is None else [int(s) for s in streams]
        known = all(0 <= s < self.streams for s in names)
        ids = np.ascontiguousarray([self._frame_no[s] if known else 0 for s in names] if frame_ids is None else list(frame_ids), np.int64)
        res = (_ffi.HealthResult * n)()
        ev = (_ffi.HealthEvent * (n * MAX_EVENTS))()
        _ffi.check(_ffi.lib().rtmodt_health_process(self._h, fp, _ffi.ptr(sp), _ffi.ptr(ids), n, h, w, st, mem, res, ev))
        for s, i in zip(names, ids):
            self._frame_no[s] = int(i) + 1
        cells = self.grid_shape[0] * self.grid_shape[1]
        return [HealthResult(r.stream, r.raw, r.active, condition_names(r.active), r.luma_sum, r.sharp, r.n_dark, r.n_bright, r.n_changed, r.n_edge,
                             r.n_ref_edge, r.n_kept, r.luma_sum / cells, r.ref_sharp, r.frames_seen, r.learned,
                             [HealthEvent(e.condition, e.kind, e.frame_id) for e in ev[i * MAX_EVENTS:i * MAX_EVENTS + r.n_events]])
                for i, r in enumerate(res)]

    def state(self, stream: int = 0) -> HealthState:
        """A copy of everything one stream holds."""
        r, prev, st = np.zeros(self.grid_shape, np.uint16), np.zeros(self.grid_shape, np.uint8), _ffi.HealthState()
        _ffi.check(_ffi.lib().rtmodt_health_read_state(self._h, int(stream), _ffi.ptr(r), _ffi.ptr(prev), C.byref(st)))
        return HealthState(r, prev, st.ref_sharp, st.frames_seen, st.active, st.pending, tuple(st.run), tuple(st.off))

    def load_state(self, state: HealthState, stream: int = 0) -> None:
        """Replaces one stream's state with a saved one (``state()``'s shapes), so that a monitor survives a restart."""
        r, prev = np.ascontiguousarray(state.r, np.uint16), np.ascontiguousarray(state.prev, np.uint8)
        if r.shape != self.grid_shape or prev.shape != self.grid_shape:
            raise ValueError(f"grids of {r.shape} / {prev.shape}, this monitor's grid is {self.grid_shape}")
        st = _state_struct(state.ref_sharp, state.frames_seen, state.active, state.pending, state.run, state.off)
        _ffi.check(_ffi.lib().rtmodt_health_load_state(self._h, int(stream), _ffi.ptr(r), _ffi.ptr(prev), C.byref(st)))

    def rebase(self, stream: int = 0) -> None:
        """The operator's word that the camera now shows what it should (a new PTZ preset, a moved mount): the stream's structure
        conditions are cleared and its next frame starts a new reference; that call reports the CLEARED and REBASED events."""
        _ffi.check(_ffi.lib().rtmodt_health_rebase(self._h, int(stream)))

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets one stream's reference, counters and conditions, or (None) every stream's; no event."""
        _ffi.check(_ffi.lib().rtmodt_health_reset(self._h, -1 if stream is None else int(stream)))
        for s in (range(self.streams) if stream is None else [int(stream)]):
            self._frame_no[s] = 0

    def last_kernel_ms(self) -> float:
        """Device time of the last ``process`` call's launches (HIP events)."""
        return _ffi.last_ms("rtmodt_health_last_ms", self._h)

    _destroy = "rtmodt_health_destroy"
