"""Track speed and proximity on a world ground plane, on the native engine.

What traffic and site-safety deployments ask of tracks -- speed per vehicle in real units, speeding / stopped-vehicle / wrong-way
alarms, the 85th-percentile speed of a lane, "two tracked objects closer than d metres" -- and Ultralytics lists as
``SpeedEstimator`` and ``DistanceCalculation``.  The reference has nothing of the kind: its ``Track`` carries no velocity.

A **fixed camera** and **one ground plane per stream**: a homography ``H`` maps image pixels to world millimetres (``plane=``,
fitted from a survey with ``fit_plane``), or a single scale (``mm_per_pixel=``, the Ultralytics shorthand ``H = diag(s, s, 1)``).
There is no PTZ handling, no camera-motion compensation and no lens model (rectify the frames first: ``ingestion.LensCorrector``).  A box is sampled at its *foot* ``((x1 + x2) / 2, y2)``
-- the point that stands on the ground -- or its centre, projected in float64 and rounded to integer millimetres; everything after
that rounding is integer arithmetic (``csrc/ground_plane.h``).  The per-frame work -- ledger upkeep, ring, odometer, speed, alarms,
histogram, pair search -- runs in ``csrc/speed.hip`` (two launches per call for all streams); there is no CPU implementation here.
``tests/speed_ref.py`` states the rules and ``include/rtmodt.h`` documents them.

Every call carries a timestamp in microseconds, strictly increasing per stream: the capture clock, or ``frame_time_us(frame_id)``.
Ways in: ``process(tracks, t_us)`` on a host list, ``process_batch(lists, t_us)`` on one list per stream, and
``process_tracker(tracker, t_us)`` straight on the device-resident state of the ByteTrack, DeepSORT, OC-SORT or BoT-SORT tracker
(exactly the tracks ``CrossingCounter.process_tracker`` passes).  Detections carry no ids, so there is no detector form.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import math
import time
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker

log = logging.getLogger("rtmodt.events")

ANCHORS = {"foot": 0, "centre": 1, "center": 1}
KINDS = ("speeding", "stopped", "wrong_way")
F_TIMER, F_NEW = 8, 16


@dataclass
class SpeedEvent:
    """One alarm, as written to the log.  ``speed_mm_s``: the speed at the moment it fired; ``world_mm``: where, on the plane."""
    timestamp_utc: str
    event_type: str                  # "speeding" | "stopped" | "wrong_way"
    track_id: int
    class_id: int
    class_name: str
    speed_mm_s: int
    t_us: int
    bbox_xyxy: list
    world_mm: list
    track: int
    stream: int = 0

    def to_json(self) -> str:
        return json.dumps(asdict(self), default=str)


def percentile_of(hist, bin_mm_s: int, p: float):
    """Nearest-rank percentile of a speed histogram: the upper edge, in mm/s, of the first bin at which the cumulative count reaches
    ``ceil(p / 100 * total)`` (at least 1).  ``None`` for an empty histogram, ``math.inf`` when that bin is the open-ended last one."""
    h = [int(v) for v in hist]
    total = sum(h)
    if total == 0:
        return None
    need = max(1, -(-int(round(p * 1000)) * total // 100000))
    run = 0
    for b, v in enumerate(h):
        run += v
        if run >= need:
            return math.inf if b == len(h) - 1 else (b + 1) * int(bin_mm_s)
    return math.inf


class SpeedEstimator(_ffi.Handle):
    """Speed, odometer, alarms, histogram and proximity pairs per stream; ledgers, histograms and planes live on the device."""

    def __init__(self, *, mm_per_pixel: Optional[float] = None, plane=None, anchor: str = "foot", window: int = 8, min_samples: int = 2,
                 hold: int = 3, max_gap_us: int = 1_000_000, min_step_mm: int = 50, limit_mm_s: int = 0, stop_mm_s: int = 0,
                 stop_us: int = 2_000_000, wrong_way_min_mm_s: int = 500, allowed_dir=(0, 0), bins: int = 0, bin_mm_s: int = 1000,
                 proximity_mm: int = 0, max_pairs: int = 256, max_events: int = 256, classes: Optional[Sequence[int]] = None, device=0,
                 n_streams: int = 1, max_tracks: int = 1024, fps: float = 30.0, log_path=None) -> None:
        if anchor not in ANCHORS:
            raise ValueError(f"anchor {anchor!r} (one of {sorted(ANCHORS)})")
        self.n_streams, self.max_tracks, self.window = int(n_streams), int(max_tracks), int(window)
        self.max_events, self.max_pairs, self.bins, self.bin_mm_s = int(max_events), int(max_pairs), int(bins), int(bin_mm_s)
        self.fps = float(fps)
        self.log_path = None if log_path is None else Path(log_path)
        if self.log_path is not None:
            self.log_path.parent.mkdir(parents=True, exist_ok=True)
        self._device = _ffi.device_ordinal(device)
        self._classes = None if classes is None else np.ascontiguousarray(classes, np.int32).reshape(-1)
        cfg = _ffi.SpeedCfg(ANCHORS[anchor], int(window), int(min_samples), int(hold), int(max_gap_us), int(stop_us), int(min_step_mm), int(limit_mm_s),
                            int(stop_mm_s), int(wrong_way_min_mm_s), (C.c_int32 * 2)(int(allowed_dir[0]), int(allowed_dir[1])), int(bins), int(bin_mm_s),
                            int(proximity_mm), int(max_pairs), int(max_events), 0 if self._classes is None else len(self._classes),
                            None if self._classes is None else C.cast((C.c_int32 * max(len(self._classes), 1))(*self._classes.tolist()), C.POINTER(C.c_int32)))
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_speed_create(self._device, C.byref(cfg), self.n_streams, self.max_tracks, C.byref(h)))
        self._h = h
        S = self.n_streams
        self._rows = (_ffi.SpeedRow * (S * self.max_tracks))()
        self._ev = (_ffi.SpeedEventRec * (S * self.max_events))()
        self._pairs = (_ffi.SpeedPair * (S * self.max_pairs))()
        self._cnt = np.zeros((4, S), np.int32)               # n_rows, n_events, n_pairs, total_pairs
        self._out = _ffi.SpeedOut(C.addressof(self._rows), self._cnt[0].ctypes.data, C.addressof(self._ev), self._cnt[1].ctypes.data,
                                  C.addressof(self._pairs), self._cnt[2].ctypes.data, self._cnt[3].ctypes.data)
        #: the results of the most recent call, one list per stream -- also when that call raised E_CAPACITY (the first ones delivered);
        #: ``last_rows`` and ``last_pairs`` are built from the result block when they are first read (valid until the next call)
        self._rows_cache, self._pairs_cache, self._slots = [[] for _ in range(S)], [[] for _ in range(S)], []
        self.last_events = [[] for _ in range(S)]
        self.last_total_pairs = [0] * S
        if plane is not None and mm_per_pixel is not None:
            raise ValueError("give plane= or mm_per_pixel=, not both")
        if plane is not None:
            self.set_plane(plane)
        elif mm_per_pixel is not None:
            self.set_scale(mm_per_pixel)

    # ------------------------------------------------------------------ the plane
    def set_plane(self, H, stream: Optional[int] = None) -> None:
        """The image-pixel -> world-millimetre homography (3 x 3) of ``stream``, or of every stream."""
        H = np.ascontiguousarray(H, np.float64).reshape(9)
        for s in range(self.n_streams) if stream is None else [int(stream)]:
            _ffi.check(_ffi.lib().rtmodt_speed_set_plane(self._h, s, _ffi.ptr(H)))

    def set_scale(self, mm_per_pixel: float, stream: Optional[int] = None) -> None:
        for s in range(self.n_streams) if stream is None else [int(stream)]:
            _ffi.check(_ffi.lib().rtmodt_speed_set_scale(self._h, s, float(mm_per_pixel)))

    @staticmethod
    def fit_plane(image_xy, world_xy_mm):
        """``(H, max_residual_mm)`` from at least four surveyed correspondences (host only, normalised DLT in float64).  The residual is
        the largest distance between a surveyed world point and the projection of its image point: a bad survey shows there."""
        a = np.ascontiguousarray(image_xy, np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(world_xy_mm, np.float64).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError(f"{len(a)} image points, {len(b)} world points")
        H, res = np.zeros(9, np.float64), C.c_double(0.0)
        _ffi.check(_ffi.lib().rtmodt_speed_fit_plane(_ffi.ptr(a), _ffi.ptr(b), len(a), _ffi.ptr(H), C.byref(res)))
        return H.reshape(3, 3), res.value

    def frame_time_us(self, frame_id: int) -> int:
        """``frame_id * 1e6 / fps`` as an integer, for sources without a capture clock."""
        return int(round(int(frame_id) * 1e6 / self.fps))

    # ------------------------------------------------------------------ per frame
    def process(self, tracks: Sequence, t_us: int, *, stream: int = 0, outputs: bool = True) -> list:
        """One stream, a list duck-typed on ``track_id / xyxy / class_id / class_name``.  Returns the alarms; rows and pairs are in
        ``last_rows`` / ``last_pairs``.  ``outputs=False``: nothing is fetched (and nothing waits for the device)."""
        n = len(tracks)
        ids = np.fromiter((int(t.track_id) for t in tracks), np.int64, n)
        xyxy = np.ascontiguousarray([np.asarray(t.xyxy, np.float32) for t in tracks], np.float32).reshape(n, 4)
        cls = np.fromiter((int(t.class_id) for t in tracks), np.int32, n)
        rc = _ffi.lib().rtmodt_speed_process(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(xyxy), _ffi.ptr(cls), n, int(t_us),
                                             C.byref(self._out) if outputs else None)
        if not outputs:
            _ffi.check(rc)
            return []
        names = {i: getattr(t, "class_name", "") for i, t in enumerate(tracks)}
        self._collect(rc, [int(stream)], flat=True, name_of=lambda r: names.get(r.track, ""))
        _ffi.check(rc)
        return self.last_events[0]

    def process_batch(self, lists: Sequence, t_us, *, outputs: bool = True) -> list:
        """Every stream in one call: ``lists[s]`` is stream ``s``'s track list, ``t_us`` one timestamp or one per stream."""
        S = self.n_streams
        if len(lists) != S:
            raise ValueError(f"{len(lists)} lists for {S} streams")
        stride = max([len(l) for l in lists] + [1])
        ids, xyxy, cls = np.zeros((S, stride), np.int64), np.zeros((S, stride, 4), np.float32), np.zeros((S, stride), np.int32)
        cnt = np.array([len(l) for l in lists], np.int32)
        for s, l in enumerate(lists):
            for i, t in enumerate(l):
                ids[s, i], xyxy[s, i], cls[s, i] = int(t.track_id), np.asarray(t.xyxy, np.float32), int(t.class_id)
        t = self._times(t_us, S)
        rc = _ffi.lib().rtmodt_speed_process_batch(self._h, _ffi.ptr(ids), _ffi.ptr(xyxy), _ffi.ptr(cls), _ffi.ptr(cnt), stride, _ffi.ptr(t),
                                                   C.byref(self._out) if outputs else None)
        if not outputs:
            _ffi.check(rc)
            return [[] for _ in range(S)]
        self._collect(rc, list(range(S)), flat=False, name_of=lambda r, s=None: "", lists=lists)
        _ffi.check(rc)
        return self.last_events

    def process_tracker(self, tracker, t_us, class_names=None, *, outputs: bool = True) -> list:
        """All streams of ``tracker`` at once, on its device-resident state; the tracks are those ``CrossingCounter.process_tracker``
        passes for that tracker.  Returns one alarm list per stream."""
        core, suffix, tsu = resolve_tracker(tracker, "process_tracker", "as a list: process(tracks, t_us)")
        t = self._times(t_us, core.n_streams)
        out = C.byref(self._out) if outputs else None
        rc = getattr(_ffi.lib(), f"rtmodt_speed_process_{suffix}")(self._h, core._h, _ffi.ptr(t), *tsu, out)
        if not outputs:
            _ffi.check(rc)
            return [[] for _ in range(core.n_streams)]
        name_of = (lambda r: class_names.get(r.cls, str(r.cls))) if isinstance(class_names, dict) else (lambda r: "")
        self._collect(rc, list(range(core.n_streams)), flat=False, name_of=name_of)
        _ffi.check(rc)
        return self.last_events

    # ------------------------------------------------------------------ state
    def histogram(self, stream: int = 0, reset: bool = False) -> np.ndarray:
        """The stream's speed histogram, int64 ``[bins]``: one count per sampled track with a known speed per call."""
        h = np.zeros(self.bins, np.int64)
        _ffi.check(_ffi.lib().rtmodt_speed_histogram(self._h, int(stream), _ffi.ptr(h) if self.bins else None, 1 if reset else 0))
        return h

    def percentile(self, p: float = 85.0, stream: int = 0):
        """``percentile_of`` the stream's histogram; the 85th percentile is the traffic engineer's number."""
        return percentile_of(self.histogram(stream), self.bin_mm_s, p)

    def label(self, track_id: int, stream: int = 0) -> str:
        """``"42 km/h"`` from the most recent rows, ``""`` while the speed is unknown or the track was not sampled: text a caller can
        append to a track's label (the renderer itself is untouched)."""
        for r in self.last_rows[stream] if stream < len(self.last_rows) else []:
            if r["track_id"] == int(track_id):
                return "" if r["speed_mm_s"] < 0 else f"{(r['speed_mm_s'] * 36 + 5000) // 10000} km/h"
        return ""

    def snapshot(self, stream: int = 0) -> list:
        """The ledger in the restatement's canonical form (``tests/speed_ref.py``: ``SpeedRef.snapshot``), rows in ascending id:
        ``[id, last t_us, [[X, Y, t_us], ...] oldest first, odometer, [anchor x, y], speed, peak, [heading x, y], class, flags,
        speeding run, wrong-way run, stop timer start or None]``."""
        cap, W = 2 * self.max_tracks, self.window
        ids, last, odo, since = (np.empty(cap, np.int64) for _ in range(4))
        rxy, rt = np.empty((cap, W, 2), np.int32), np.empty((cap, W), np.int64)
        anc, head, ints = np.empty((cap, 2), np.int32), np.empty((cap, 2), np.int32), np.empty((cap, 8), np.int32)
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_speed_state(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(last), _ffi.ptr(odo), _ffi.ptr(since), _ffi.ptr(rxy),
                                                 _ffi.ptr(rt), _ffi.ptr(anc), _ffi.ptr(head), _ffi.ptr(ints), C.byref(n)))
        rows = []
        for r in range(n.value):
            ns, hd, speed, peak, cls, flags, run_s, run_w = (int(v) for v in ints[r])
            slots = [(hd - ns + 1 + k) % W for k in range(ns)]
            rows.append([int(ids[r]), int(last[r]), [[int(rxy[r, k, 0]), int(rxy[r, k, 1]), int(rt[r, k])] for k in slots], int(odo[r]), anc[r].tolist(),
                         speed, peak, head[r].tolist(), cls, flags, run_s, run_w, int(since[r]) if flags & F_TIMER else None])
        return rows

    _destroy = "rtmodt_speed_destroy"

    # ------------------------------------------------------------------ internals
    @staticmethod
    def _times(t_us, n) -> np.ndarray:
        t = np.asarray(t_us, np.int64).reshape(-1)
        if t.size == 1:
            t = np.repeat(t, n)
        if t.size != n:
            raise ValueError(f"{t.size} timestamps for {n} streams")
        return np.ascontiguousarray(t)

    def _collect(self, rc, streams, flat, name_of, lists=None) -> None:
        S = len(streams)
        self.last_events, self.last_total_pairs = [[] for _ in range(S)], [0] * S
        self._rows_cache, self._pairs_cache, self._slots = [[] for _ in range(S)], [[] for _ in range(S)], []
        if rc not in (_ffi.OK, _ffi.E_CAPACITY):
            return
        self._rows_cache = self._pairs_cache = None
        self._slots = [0 if flat else s for s in streams]
        for k, s in enumerate(streams):
            d = self._slots[k]
            evs = []
            for i in range(int(self._cnt[1, d])):
                r = self._ev[d * self.max_events + i]
                name = getattr(lists[s][r.track], "class_name", "") if lists is not None else name_of(r)
                evs.append(self._emit(r, s, name))
            self.last_events[k] = evs
            self.last_total_pairs[k] = int(self._cnt[3, d])

    @property
    def last_rows(self) -> list:
        """One list of row dicts per stream of the most recent call, in list order."""
        if self._rows_cache is None:
            self._rows_cache = [[dict(track_id=int(r.track_id), track=int(r.track), world=[int(r.world[0]), int(r.world[1])], speed_mm_s=int(r.speed_mm_s),
                                      peak_mm_s=int(r.peak_mm_s), heading=[int(r.heading[0]), int(r.heading[1])], odometer_mm=int(r.odometer_mm),
                                      class_id=int(r.cls), flags=int(r.flags), n_samples=int(r.n_samples))
                                 for r in (self._rows[d * self.max_tracks + i] for i in range(int(self._cnt[0, d])))] for d in self._slots]
        return self._rows_cache

    @property
    def last_pairs(self) -> list:
        """One list of ``(track_a, track_b, dist_mm)`` per stream of the most recent call, in (i, j) order of the rows."""
        if self._pairs_cache is None:
            self._pairs_cache = [[(int(p.track_a), int(p.track_b), int(p.dist_mm)) for p in
                                  (self._pairs[d * self.max_pairs + i] for i in range(int(self._cnt[2, d])))] for d in self._slots]
        return self._pairs_cache

    def _emit(self, r, stream, class_name) -> SpeedEvent:
        evt = SpeedEvent(timestamp_utc=time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), event_type=KINDS[r.kind], track_id=int(r.track_id),
                         class_id=int(r.cls), class_name=class_name, speed_mm_s=int(r.value), t_us=int(r.t_us), bbox_xyxy=[float(v) for v in r.xyxy],
                         world_mm=[int(r.world[0]), int(r.world[1])], track=int(r.track), stream=stream)
        if self.log_path is not None:
            with open(self.log_path, "a") as f:
                f.write(evt.to_json() + "\n")
        return evt
