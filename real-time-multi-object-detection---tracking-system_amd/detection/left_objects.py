"""Left and removed objects on MI355X: what stopped moving and is no class of the detector.  A bag on a platform, a car in a
no-parking bay, the hole where an exhibit stood: ``MotionDetector`` folds them into its background within a few hundred frames
and the 80 classes do not name them.  A second, slower model per stream on the same luma grid keeps static foreground apart from
moving foreground, a device-resident ledger follows every static region, and the frame's tracks tell a left object from a person
standing still.  "Left object" and "object removed" are standard rules of cameras and NVRs; the reference fires on tracked
objects only (``zone_engine.py``) and has no counterpart.

The work runs in ``csrc/leftobj.hip`` (rules in its header comment and in ``csrc/leftobj_rule.h``); there is no CPU implementation
here.  ``tests/leftobj_ref.py`` restates every rule and the kernels equal it exactly: all of it is integer arithmetic.  Deliberate
limits: a fixed camera (no camera-motion compensation), one luma channel, its own pass over the pixels.  Unpinned: parity with any
vendor's rule, and every default -- none has been validated on real footage.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker

WARMUP, CLEAR, STATIC, SCENE_CHANGE = 0, 1, 2, 3
STATUS_NAMES = ("warmup", "clear", "static", "scene_change")
UNKNOWN, ABANDONED, REMOVED, TRACKED_STATIC = 0, 1, 2, 3
KIND_NAMES = ("unknown", "abandoned", "removed", "tracked_static")
CLEARED, ABSORBED, RESET = 1, 2, 3
REASON_NAMES = ("", "cleared", "absorbed", "reset")
TRACKS_NONE, TRACKS_LIST, TRACKS_BYTETRACK, TRACKS_DEEPSORT, TRACKS_OCSORT, TRACKS_BOTSORT = range(6)
CFG_FIELDS = ("scale", "warmup", "warm_shift", "learn_shift", "threshold", "stable", "cand_shift", "occlusion", "static_frames", "min_neighbors",
              "min_area", "max_area", "max_regions", "scene_pm", "max_objects", "miss_frames", "alarm_frames", "absorb_frames", "covered_pm",
              "attend_margin", "max_tracks")
CELL_DTYPE = np.dtype([("bg", "<u2"), ("cand", "<u2"), ("age", "<u2"), ("miss", "u1"), ("flags", "u1")])     # the 8-byte cell, little endian


def make_cfg(streams=1, height=0, width=0, device=0, owner_classes: Optional[Sequence[int]] = None,
             report_tracked: Optional[Sequence[int]] = None, **cfg) -> "_ffi.LeftObjCfg":
    """``rtmodt_leftobj_default_cfg`` with the given fields replaced."""
    c = _ffi.LeftObjCfg()
    _ffi.lib().rtmodt_leftobj_default_cfg(C.byref(c))
    c.streams, c.height, c.width, c.device = int(streams), int(height), int(width), _ffi.device_ordinal(device)
    for name, vals in (("owner", owner_classes), ("report", report_tracked)):
        if vals is None:
            continue
        vals = [int(v) for v in vals]
        if len(vals) > 8:
            raise ValueError(f"{len(vals)} {name} classes (at most 8)")
        setattr(c, f"n_{name}_classes", len(vals))
        arr = getattr(c, f"{name}_classes")
        for i in range(8):
            arr[i] = vals[i] if i < len(vals) else 0
    for k, v in cfg.items():
        if k not in CFG_FIELDS:
            raise TypeError(f"unknown left-object parameter {k!r}; one of {CFG_FIELDS}")
        setattr(c, k, int(v))
    return c


def pack_cell(bg: int, cand: int, age: int, miss: int, flags: int) -> int:
    return int(bg) | int(cand) << 16 | int(age) << 32 | int(miss) << 48 | int(flags) << 56


def unpack_cell(v: int) -> Tuple[int, int, int, int, int]:
    v = int(v)
    return v & 0xffff, v >> 16 & 0xffff, v >> 32 & 0xffff, v >> 48 & 0xff, v >> 56 & 0xff


def leftobj_cell(yc: int, frames_seen: int, cell: Tuple[int, int, int, int, int], **cfg):
    """``rtmodt_leftobj_cell`` (host only): one cell ``(bg, cand, age, miss, flags)`` of luma ``yc`` under the rule fields of ``cfg``
    -> (cell, fg, static)."""
    c = make_cfg(1, 1, 1, **cfg)
    st, fg, stat = C.c_uint64(pack_cell(*cell)), C.c_int32(0), C.c_int32(0)
    _ffi.check(_ffi.lib().rtmodt_leftobj_cell(C.byref(c), int(yc), int(frames_seen), C.byref(st), C.byref(fg), C.byref(stat)))
    return unpack_cell(st.value), bool(fg.value), bool(stat.value)


def rasterise_polygons(grid_shape, scale: int, polygons, invert: bool = False) -> np.ndarray:
    """Polygons (lists of ``(x, y)`` pixels) -> ``uint8 (gh, gw)``: 1 where a cell's centre ``((cx + 0.5) * scale, (cy + 0.5) * scale)``
    lies inside one of them (even-odd rule, computed in doubled integer coordinates); ``invert`` flips the grid ("only the platform")."""
    gh, gw = grid_shape
    px = (2 * np.arange(gw, dtype=np.int64) + 1) * scale                     # doubled centres
    py = (2 * np.arange(gh, dtype=np.int64) + 1) * scale
    X, Y = np.meshgrid(px, py)
    inside = np.zeros((gh, gw), bool)
    for poly in polygons:
        pts = [(2 * int(x), 2 * int(y)) for x, y in poly]
        if len(pts) < 3:
            raise ValueError("a polygon has at least three points")
        hit = np.zeros((gh, gw), bool)
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if y0 == y1:
                continue
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            span = (Y >= y0) & (Y < y1)
            hit ^= span & ((X - x0) * (y1 - y0) < (x1 - x0) * (Y - y0))    # the centre is left of the edge
        inside |= hit
    return (inside ^ bool(invert)).astype(np.uint8)


@dataclass
class LeftObjectEvent:
    """One alarm.  ``box``: pixels ``(x0, y0, x1, y1)``, x1 / y1 exclusive; ``owner``: the last attending track id, -1 for none."""
    stream: int
    oid: int
    kind: int
    box: Tuple[int, int, int, int]
    area: int
    first_frame: int
    frame_id: int
    owner: int

    @property
    def kind_name(self) -> str:
        return KIND_NAMES[self.kind]


@dataclass
class LeftObjectResult:
    """One stream's answer for one frame.  ``regions``: dicts of the stored static regions; ``events``: the alarms of this frame;
    ``retired``: ``(oid, reason, alarmed)``; ``objects``: the ledger after the call (``want_objects``)."""
    stream: int
    status: int
    frames_seen: int
    n_fg: int
    n_static: int
    n_regions_total: int
    n_objects: int
    dropped: int
    next_oid: int
    regions: List[dict] = field(default_factory=list)
    events: List[LeftObjectEvent] = field(default_factory=list)
    retired: List[Tuple[int, int, int]] = field(default_factory=list)
    objects: Optional[List[dict]] = None

    @property
    def status_name(self) -> str:
        return STATUS_NAMES[self.status]


def _object_dict(o) -> dict:
    return dict(oid=o.oid, kind=o.kind, area=o.area, idle=o.idle, unmatched=o.unmatched, alarmed=o.alarmed, first_frame=o.first_frame,
                owner=o.owner, cells=tuple(o.cells), box=tuple(o.box))


def _region_dict(g) -> dict:
    return dict(box=tuple(g.box), cells=tuple(g.cells), area=g.area, kind=g.kind, age_min=g.age_min, age_max=g.age_max, covered=g.covered,
                attended=g.attended, oid=g.oid, root=g.root)


class LeftObjectDetector(_ffi.Handle):
    """``streams`` models and ledgers for ``height x width`` BGR24 frames.

    The model: ``scale`` (1, 2, 4, 8) pixels per cell side; the first ``warmup`` frames only learn (``warm_shift``); afterwards a cell
    is foreground when it differs from the background by more than ``threshold`` luma levels, background cells learn by
    ``learn_shift`` and foreground never updates the background.  A foreground cell that stays within ``stable`` levels of its
    candidate value ages (``cand_shift``), survives ``occlusion`` frames of something else in front of it, and is static from
    ``static_frames`` on.  The regions: static cells with ``min_neighbors`` static cells in their 3 x 3 neighbourhood, 8-connected,
    ``min_area``..``max_area`` cells, ``max_regions`` stored.  ``scene_pm`` per mille of foreground cells is a scene change: the model
    and the ledger start over.  The ledger: ``max_objects`` entries, ``miss_frames`` unmatched calls until an entry clears,
    ``alarm_frames`` unattended calls until the alarm, ``absorb_frames`` (0: never) until the object is folded into the background.
    The tracks: a region is covered when one track covers ``covered_pm`` per mille of its box (the tracked object itself: no alarm,
    unless the track's class is in ``report_tracked``), attended when a track of ``owner_classes`` comes within ``attend_margin``
    pixels; ``max_tracks`` per list."""

    def __init__(self, streams: int, height: int, width: int, *, owner_classes: Optional[Sequence[int]] = None,
                 report_tracked: Optional[Sequence[int]] = None, device=0, **cfg) -> None:
        self._h = None
        self._cfg = make_cfg(streams, height, width, device, owner_classes, report_tracked, **cfg)
        self.streams, self.height, self.width = int(streams), int(height), int(width)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_leftobj_create(C.byref(self._cfg), C.byref(h)))
        self._h = h
        c = self._cfg
        self.scale, self.max_regions, self.max_objects, self.max_tracks = c.scale, c.max_regions, c.max_objects, c.max_tracks
        self.grid_shape = (-(-self.height // c.scale), -(-self.width // c.scale))
        self._next_frame = [0] * self.streams

    # ---- tracks ----
    def _tracks(self, n: int, tracks, tracker):
        """-> (LeftObjTracks or None, keep-alive)."""
        if tracks is not None and tracker is not None:
            raise ValueError("tracks or tracker, not both")
        if tracker is not None:
            core, suffix, tsu = resolve_tracker(tracker)
            if suffix is not None:
                src = {"tracker": TRACKS_BYTETRACK, "deepsort": TRACKS_DEEPSORT, "ocsort": TRACKS_OCSORT, "botsort": TRACKS_BOTSORT}[suffix]
                return _ffi.LeftObjTracks(src, 0, None, None, None, None, core._h, sum(tsu), 0), [tracker]
            raise TypeError("tracker: the ByteTrack, the DeepSORT, the OC-SORT or the BoT-SORT tracker (their state is read on the device); "
                            "hand any other tracker's tracks over as lists")
        if tracks is None:
            return None, []
        if n == 1 and len(tracks) == 3 and not isinstance(tracks[0], (tuple, list)):
            tracks = [tracks]
        if len(tracks) != n:
            raise ValueError(f"{len(tracks)} track lists for {n} frames")
        lists = []
        for ids, xyxy, cls in tracks:
            ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
            xyxy = np.ascontiguousarray(xyxy, np.float32).reshape(-1, 4)
            cls = np.ascontiguousarray(cls, np.int32).reshape(-1)
            if not len(ids) == len(xyxy) == len(cls):
                raise ValueError(f"a track list of {len(ids)} ids, {len(xyxy)} boxes and {len(cls)} classes")
            lists.append((ids, xyxy, cls))
        stride = max(1, max(len(l[0]) for l in lists))
        ids, xyxy, cls = np.zeros((n, stride), np.int64), np.zeros((n, stride, 4), np.float32), np.zeros((n, stride), np.int32)
        cnt = np.zeros(n, np.int32)
        for i, (a, b, c) in enumerate(lists):
            cnt[i] = len(a)
            ids[i, :len(a)], xyxy[i, :len(a)], cls[i, :len(a)] = a, b, c
        keep = [ids, xyxy, cls, cnt]
        return _ffi.LeftObjTracks(TRACKS_LIST, stride, ids.ctypes.data, xyxy.ctypes.data, cls.ctypes.data, cnt.ctypes.data, None, 0, 0), keep

    def process(self, frames, streams: Optional[Sequence[int]] = None, *, tracks=None, tracker=None, frame_id=None, stride: Optional[int] = None,
                offset: int = 0, want_objects: bool = False, outputs: bool = True) -> List[LeftObjectResult]:
        """One frame for each of the named streams (None: one per stream, in order), as ``MotionDetector.process`` takes them.
        ``tracks``: per frame ``(ids, xyxy, classes)`` (for one frame the triple itself will do); ``tracker``: a ByteTrack, DeepSORT,
        OC-SORT or BoT-SORT tracker of as many streams, read on the device.  ``frame_id``: an int for all frames, one per frame, or
        None: a counter per stream.  ``outputs=False`` copies nothing back and returns []."""
        n = self.streams if streams is None else len(streams)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=self.height, width=self.width, stride=stride, offset=offset, writable=False)
        if n == 0:
            return []
        fp = (C.c_void_p * n)(*ptrs)
        names = list(range(n)) if streams is None else [int(s) for s in streams]
        sp = None if streams is None else np.ascontiguousarray(names, np.int32)
        if frame_id is None:
            fid = np.array([self._next_frame[s] if 0 <= s < self.streams else 0 for s in names], np.int64)
        else:
            fid = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_id, np.int64), (n,)))
        trk, keep = self._tracks(n, tracks, tracker)
        res = (_ffi.LeftObjResult * n)()
        reg = (_ffi.LeftObjRegion * (n * self.max_regions))()
        evs = (_ffi.LeftObjEvent * (n * 2 * self.max_objects))()        # a call emits at most 2 x max_objects events
        ret = (_ffi.LeftObjRetired * (n * self.max_objects))()
        obj = (_ffi.LeftObjObject * (n * self.max_objects))() if want_objects else None
        addr = lambda a: C.cast(a, C.c_void_p) if a is not None else None     # noqa: E731
        out = _ffi.LeftObjOut(addr(res), addr(reg), addr(evs), addr(ret), addr(obj)) if outputs else None
        _ffi.check(_ffi.lib().rtmodt_leftobj_process(self._h, fp, _ffi.ptr(sp), _ffi.ptr(fid), n, h, w, st, mem, C.byref(trk) if trk else None,
                                                     C.byref(out) if out else None))
        del keep
        for i, s in enumerate(names):
            self._next_frame[s] = int(fid[i]) + 1
        if not outputs:
            return []
        results = []
        for i, r in enumerate(res):
            R, O = i * self.max_regions, i * self.max_objects
            results.append(LeftObjectResult(
                r.stream, r.status, r.frames_seen, r.n_fg, r.n_static, r.n_regions_total, r.n_objects, r.dropped, r.next_oid,
                [_region_dict(reg[R + k]) for k in range(r.n_regions)],
                [LeftObjectEvent(r.stream, e.oid, e.kind, tuple(e.box), e.area, e.first_frame, e.frame_id, e.owner) for e in (evs[2 * O + k] for k in range(r.n_events))],
                [(t.oid, t.reason, t.alarmed) for t in (ret[O + k] for k in range(r.n_retired))],
                [_object_dict(obj[O + k]) for k in range(r.n_objects)] if want_objects else None))
        return results

    # ---- state ----
    def mask(self, stream: int = 0) -> np.ndarray:
        """The mask of the stream's last frame, ``uint8 (gh, gw)`` of 0 / 1."""
        out = np.zeros(self.grid_shape, np.uint8)
        _ffi.check(_ffi.lib().rtmodt_leftobj_read_mask(self._h, int(stream), _ffi.ptr(out)))
        return out

    def load_mask(self, mask, stream: int = 0) -> None:
        """Replaces the stream's last mask with a saved one (``mask()``'s shape)."""
        mask = np.ascontiguousarray(mask, np.uint8)
        if mask.shape != self.grid_shape:
            raise ValueError(f"a mask of {mask.shape}, this detector's grid is {self.grid_shape}")
        _ffi.check(_ffi.lib().rtmodt_leftobj_load_mask(self._h, int(stream), _ffi.ptr(mask)))

    def state(self, stream: int = 0):
        """-> (cells, luma, frames_seen): the model as a ``CELL_DTYPE (gh, gw)`` array (bg, cand, age, miss, flags), the last luma
        grid ``uint8 (gh, gw)``."""
        cells, luma, seen = np.zeros(self.grid_shape, np.uint64), np.zeros(self.grid_shape, np.uint8), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_leftobj_read_state(self._h, int(stream), _ffi.ptr(cells), _ffi.ptr(luma), C.byref(seen)))
        return cells.view(CELL_DTYPE), luma, seen.value

    def load_state(self, cells, luma, frames_seen: int, stream: int = 0) -> None:
        """Replaces one stream's model with a saved one (``state()``'s shapes), so that it survives a restart."""
        cells = np.ascontiguousarray(cells)
        cells = cells.view(np.uint64) if cells.dtype == CELL_DTYPE else np.ascontiguousarray(cells, np.uint64)
        luma = np.ascontiguousarray(luma, np.uint8)
        if cells.shape != self.grid_shape or luma.shape != self.grid_shape:
            raise ValueError(f"a model of {cells.shape} / {luma.shape}, this detector's grid is {self.grid_shape}")
        _ffi.check(_ffi.lib().rtmodt_leftobj_load_state(self._h, int(stream), _ffi.ptr(cells), _ffi.ptr(luma), int(frames_seen)))

    def ledger(self, stream: int = 0):
        """-> (objects, next_oid): the live entries in oid order, as dicts."""
        obj = (_ffi.LeftObjObject * self.max_objects)()
        n, nxt = C.c_int32(0), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_leftobj_read_ledger(self._h, int(stream), C.cast(obj, C.c_void_p), C.byref(n), C.byref(nxt)))
        return [_object_dict(obj[k]) for k in range(n.value)], nxt.value

    def load_ledger(self, objects, next_oid: int, stream: int = 0) -> None:
        """Replaces one stream's ledger with ``ledger()``'s answer."""
        objects = list(objects)
        if len(objects) > self.max_objects:
            raise ValueError(f"{len(objects)} entries > max_objects {self.max_objects}")
        obj = (_ffi.LeftObjObject * max(1, len(objects)))()
        for o, d in zip(obj, objects):
            o.first_frame, o.owner, o.oid, o.kind, o.area = d["first_frame"], d["owner"], d["oid"], d["kind"], d["area"]
            o.idle, o.unmatched, o.alarmed = d["idle"], d["unmatched"], d["alarmed"]
            o.cells[:], o.box[:] = d["cells"], d["box"]
        _ffi.check(_ffi.lib().rtmodt_leftobj_load_ledger(self._h, int(stream), C.cast(obj, C.c_void_p), len(objects), int(next_oid)))

    def set_ignore(self, grid, stream: int = 0) -> None:
        """``uint8 (gh, gw)``: a cell whose entry is not 0 is never static."""
        grid = np.ascontiguousarray(grid, np.uint8)
        if grid.shape != self.grid_shape:
            raise ValueError(f"an ignore grid of {grid.shape}, this detector's grid is {self.grid_shape}")
        _ffi.check(_ffi.lib().rtmodt_leftobj_set_ignore(self._h, int(stream), _ffi.ptr(grid)))

    def ignore(self, stream: int = 0) -> np.ndarray:
        out = np.zeros(self.grid_shape, np.uint8)
        _ffi.check(_ffi.lib().rtmodt_leftobj_read_ignore(self._h, int(stream), _ffi.ptr(out)))
        return out

    def ignore_polygons(self, stream: int, polygons, invert: bool = False) -> np.ndarray:
        """Ignores the cells whose centre lies inside one of ``polygons`` (pixel ``(x, y)`` lists) -- a TV screen, a tree -- or, with
        ``invert``, outside all of them ("only the platform").  Rasterised on the host; returns the grid it set."""
        grid = rasterise_polygons(self.grid_shape, self.scale, polygons, invert)
        self.set_ignore(grid, stream)
        return grid

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets one stream's model, mask and ledger, or (None) every stream's; the ignore grid stays."""
        _ffi.check(_ffi.lib().rtmodt_leftobj_reset(self._h, -1 if stream is None else int(stream)))
        for s in (range(self.streams) if stream is None else [int(stream)]):
            self._next_frame[s] = 0

    def last_kernel_ms(self) -> float:
        """Device time of the last ``process`` call's launches (HIP events)."""
        return _ffi.last_ms("rtmodt_leftobj_last_ms", self._h)

    _destroy = "rtmodt_leftobj_destroy"
