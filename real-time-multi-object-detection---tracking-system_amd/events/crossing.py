"""Directional line and gate crossing counts on the native engine.

The reference's config defines a zone with ``trigger: "crossing"`` and ``direction: "left_to_right"``
(config/default.yaml:73-77); its engine parses the direction (src/events/zone_engine.py:150) and never reads it, so that
zone is an intrusion zone under another name.  ``CrossingCounter`` gives it the meaning the config implies -- and adds
plain tripwires -- beside the zone engine, which stays bit-identical to the reference:

* a **line** ``{"name", "a": [x, y], "b": [x, y], "direction": "both" | "pos" | "neg"}`` counts a track whose centroid
  path crosses the segment A -> B, ``"pos"`` when it ends on the side where ``(B - A) x (P - A) > 0``;
* a **gate** ``{"name", "polygon", "direction": None | "left_to_right" | ...}`` counts a track that leaves the polygon
  when the displacement from where it entered agrees with the direction.

The per-frame work -- ledger upkeep, side tests, point-in-polygon, counts, event order -- runs in ``csrc/crossing.hip``
(one launch per frame for all streams); there is no CPU implementation here.  ``tests/crossing_ref.py`` states the rules.
Three ways in: ``process(tracks, frame_id)`` on a host list, and ``process_tracker(tracker, frame_id)`` straight on the
device-resident state of a ``MultiObjectTracker`` / ``_ByteTrackCore``, a ``DeepSortTracker`` / ``_DeepSortCore`` or an
``OcSortTracker`` / ``_OcSortCore``.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import time
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker

log = logging.getLogger("rtmodt.events")

LINE_DIRECTIONS = {"both": 0, "pos": 1, "neg": 2}
GATE_DIRECTIONS = {None: 0, "left_to_right": 1, "right_to_left": 2, "top_to_bottom": 3, "bottom_to_top": 4}
_LINE_NAMES = {1: "pos", 2: "neg"}
_GATE_NAMES = {v: k for k, v in GATE_DIRECTIONS.items()}
LIMIT = 1 << 20


@dataclass
class CrossingEvent:
    """One crossing, as written to the log.  ``previous``: the previous passed centroid (line) or the centroid the track
    entered the gate at; ``frames``: how many frames ago that was."""
    timestamp_utc: str
    event_type: str                  # "line_crossing" | "gate_crossing"
    name: str
    index: int
    direction: Optional[str]
    track_id: int
    class_id: int
    class_name: str
    bbox_xyxy: list
    centroid: list
    previous: list
    frames: int
    frame_id: int
    stream: int = 0

    def to_json(self) -> str:
        return json.dumps(asdict(self), default=str)


def _int_coords(what, values) -> np.ndarray:
    """Coordinates as int32; a value that is not integral, or lies outside +-2^20, is refused rather than truncated."""
    a = np.asarray(values, dtype=np.float64)
    if a.size and (not np.all(np.isfinite(a)) or np.any(a != np.round(a)) or np.any(np.abs(a) > LIMIT)):
        raise ValueError(f"{what}: coordinates must be integers within +-2^20, got {np.asarray(values).tolist()}")
    return a.astype(np.int32)


def gates_from_zone_configs(zone_configs: Sequence) -> list:
    """Exactly the zones with ``trigger == "crossing"`` (config/default.yaml:73-77), as gate dicts (name, polygon, direction)."""
    return [{"name": z["name"], "polygon": z["polygon"], "direction": z.get("direction")} for z in zone_configs
            if z.get("trigger", "intrusion") == "crossing"]


class CrossingCounter(_ffi.Handle):
    """Counts directional crossings of lines and gates; counts and ledger live on the device, one set per stream."""

    def __init__(self, lines: Sequence = (), gates: Sequence = (), *, n_classes: int = 80, device=0, n_streams: int = 1, max_tracks: int = 2048,
                 max_events: int = 256, max_gap_frames: int = 30, log_path=None) -> None:
        self.lines = [dict(name=str(l.get("name", f"line{i}")), a=_int_coords(f"line {i}", l["a"]).reshape(2).tolist(),
                           b=_int_coords(f"line {i}", l["b"]).reshape(2).tolist(), direction=l.get("direction") or "both") for i, l in enumerate(lines)]
        self.gates = [dict(name=str(g.get("name", f"gate{i}")), polygon=np.ascontiguousarray(_int_coords(f"gate {i}", g["polygon"]).reshape(-1, 2)),
                           direction=g.get("direction")) for i, g in enumerate(gates)]
        for l in self.lines:
            if l["direction"] not in LINE_DIRECTIONS:
                raise ValueError(f"line {l['name']!r}: direction {l['direction']!r} (one of {sorted(LINE_DIRECTIONS)})")
        for g in self.gates:
            if g["direction"] not in GATE_DIRECTIONS:
                raise ValueError(f"gate {g['name']!r}: direction {g['direction']!r} (one of {list(GATE_DIRECTIONS)})")
        self.n_classes, self.n_streams, self.max_tracks = int(n_classes), int(n_streams), int(max_tracks)
        self.max_events, self.max_gap_frames = int(max_events), int(max_gap_frames)
        self.log_path = None if log_path is None else Path(log_path)
        if self.log_path is not None:
            self.log_path.parent.mkdir(parents=True, exist_ok=True)
        self._device = _ffi.device_ordinal(device)
        lc = (_ffi.LineCfg * max(len(self.lines), 1))()
        for i, l in enumerate(self.lines):
            lc[i] = _ffi.LineCfg(l["a"][0], l["a"][1], l["b"][0], l["b"][1], LINE_DIRECTIONS[l["direction"]])
        gc = (_ffi.GateCfg * max(len(self.gates), 1))()
        for i, g in enumerate(self.gates):
            gc[i] = _ffi.GateCfg(g["polygon"].ctypes.data_as(C.POINTER(C.c_int32)), len(g["polygon"]), GATE_DIRECTIONS[g["direction"]])
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_crossing_create(self._device, lc, len(self.lines), gc, len(self.gates), self.n_classes, self.n_streams,
                                                     self.max_tracks, self.max_events, self.max_gap_frames, C.byref(h)))
        self._h = h
        self._ev = (_ffi.CrossingEventRec * (self.n_streams * self.max_events))()
        self._n = np.zeros(self.n_streams, np.int32)
        #: the events of the most recent call, one list per stream -- also when that call raised (E_CAPACITY: the first max_events of the frame)
        self.last_events = [[] for _ in range(self.n_streams)]
        log.info("CrossingCounter loaded %d lines, %d gates.", len(self.lines), len(self.gates))

    @classmethod
    def from_zone_configs(cls, zone_configs: Sequence, **kwargs) -> "CrossingCounter":
        """The reference's ``events.zones`` list as written: exactly the zones with ``trigger == "crossing"`` become gates
        (name, polygon, direction); the others are the zone engine's business."""
        return cls(lines=kwargs.pop("lines", ()), gates=gates_from_zone_configs(zone_configs), **kwargs)

    # ------------------------------------------------------------------ per frame
    def process(self, tracks: Sequence, frame_id: int, *, stream: int = 0) -> list:
        """One stream, a list duck-typed on ``track_id / xyxy / class_id / class_name`` like ``ZoneEventEngine.process``.
        More than ``max_events`` crossings in one frame raise ``RtmodtError`` (``E_CAPACITY``): the counts are complete."""
        n = len(tracks)
        ids = np.fromiter((int(t.track_id) for t in tracks), np.int64, n)
        xyxy = np.ascontiguousarray([np.asarray(t.xyxy, np.float32) for t in tracks], np.float32).reshape(n, 4)
        cls = np.fromiter((int(t.class_id) for t in tracks), np.int32, n)
        ne = C.c_int32(0)
        rc = _ffi.lib().rtmodt_crossing_process(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(xyxy), _ffi.ptr(cls), n, int(frame_id),
                                                C.cast(self._ev, C.c_void_p), C.byref(ne))
        events = [self._emit(self._ev[e], frame_id, int(stream), getattr(tracks[self._ev[e].track], "class_name", "")) for e in range(ne.value)] \
            if rc in (_ffi.OK, _ffi.E_CAPACITY) else []
        self.last_events = [events]
        _ffi.check(rc)
        return events

    def process_tracker(self, tracker, frame_id: int, class_names=None) -> list:
        """All streams of ``tracker`` at once, on its device-resident state.  Returns one event list per stream.  A
        ``MultiObjectTracker`` / ``_ByteTrackCore`` passes the tracks ``tracker.report`` names (``"matched"``: matched or spawned
        this frame); a ``DeepSortTracker`` / ``_DeepSortCore`` its confirmed tracks matched this frame; an ``OcSortTracker`` /
        ``_OcSortCore`` the tracks it returns this frame; a ``BotSortTracker`` / ``_BotSortCore`` its returned tracks matched this
        frame."""
        core, suffix, tsu = resolve_tracker(tracker, "process_tracker", "as a list: process(tracks, frame_id)")
        ev, n = C.cast(self._ev, C.c_void_p), _ffi.ptr(self._n)
        rc = getattr(_ffi.lib(), f"rtmodt_crossing_process_{suffix}")(self._h, core._h, int(frame_id), *tsu, ev, n)
        out = []
        if rc in (_ffi.OK, _ffi.E_CAPACITY):
            for s in range(core.n_streams):
                evs = []
                for e in range(int(self._n[s])):
                    r = self._ev[s * self.max_events + e]
                    name = class_names.get(r.cls, str(r.cls)) if isinstance(class_names, dict) else ""
                    evs.append(self._emit(r, frame_id, s, name))
                out.append(evs)
        self.last_events = out
        _ffi.check(rc)
        return out

    # ------------------------------------------------------------------ state
    def counts(self, stream: int = 0) -> dict:
        """``line_total [L, 2]`` (pos, neg), ``line_class [L, 2, C]``, ``gate_total [G]``, ``gate_class [G, C]``, int64, plus the names."""
        L, G, Cn = len(self.lines), len(self.gates), self.n_classes
        lt, lc = np.zeros((L, 2), np.int64), np.zeros((L, 2, Cn), np.int64)
        gt, gc = np.zeros(G, np.int64), np.zeros((G, Cn), np.int64)
        _ffi.check(_ffi.lib().rtmodt_crossing_counts(self._h, int(stream), _ffi.ptr(lt), _ffi.ptr(lc), _ffi.ptr(gt), _ffi.ptr(gc)))
        return {"line_names": [l["name"] for l in self.lines], "gate_names": [g["name"] for g in self.gates], "line_total": lt, "line_class": lc,
                "gate_total": gt, "gate_class": gc}

    def reset_counts(self) -> None:
        """Zeroes every stream's counts; the ledgers stay, so a track halfway through a gate still fires on exit."""
        _ffi.check(_ffi.lib().rtmodt_crossing_reset_counts(self._h))

    def snapshot(self, stream: int = 0) -> list:
        """The ledger in the restatement's canonical form (``tests/crossing_ref.py``: ``CrossingRef.snapshot``), rows in ascending id:
        ``[id, last frame, [px, py], [stored side per line], [[gate, entry x, entry y, entry frame], ...]]``."""
        cap, L, G = 2 * self.max_tracks, len(self.lines), len(self.gates)
        ids, last = np.empty(cap, np.int64), np.empty(cap, np.int64)
        prev = np.empty((cap, 2), np.int32)
        pos, neg, ins = np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        exy, ef = np.empty((cap, max(G, 1), 2), np.int32), np.empty((cap, max(G, 1)), np.int64)
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_crossing_state(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(last), _ffi.ptr(prev), _ffi.ptr(pos), _ffi.ptr(neg),
                                                    _ffi.ptr(ins), _ffi.ptr(exy), _ffi.ptr(ef), C.byref(n)))
        k = n.value
        exy, ef = exy.reshape(-1)[:k * G * 2].reshape(k, G, 2), ef.reshape(-1)[:k * G].reshape(k, G)
        rows = []
        for r in range(k):
            p, m, i = int(pos[r]), int(neg[r]), int(ins[r])
            rows.append([int(ids[r]), int(last[r]), prev[r].tolist(), [(p >> l & 1) - (m >> l & 1) for l in range(L)],
                         [[g, int(exy[r, g, 0]), int(exy[r, g, 1]), int(ef[r, g])] for g in range(G) if i >> g & 1]])
        return rows

    _destroy = "rtmodt_crossing_destroy"

    # ------------------------------------------------------------------ internals
    def _emit(self, r, frame_id, stream, class_name) -> CrossingEvent:
        line = r.kind == 0
        item = self.lines[r.index] if line else self.gates[r.index]
        evt = CrossingEvent(timestamp_utc=time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), event_type="line_crossing" if line else "gate_crossing",
                            name=item["name"], index=int(r.index), direction=_LINE_NAMES[r.direction] if line else _GATE_NAMES[r.direction],
                            track_id=int(r.track_id), class_id=int(r.cls), class_name=class_name, bbox_xyxy=[float(v) for v in r.xyxy],
                            centroid=[int(v) for v in r.centroid], previous=[int(v) for v in r.prev], frames=int(r.frames), frame_id=int(frame_id),
                            stream=stream)
        if self.log_path is not None:
            with open(self.log_path, "a") as f:
                f.write(evt.to_json() + "\n")
        return evt
