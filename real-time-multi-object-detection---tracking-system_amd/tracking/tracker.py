"""Drop-in for the reference's ``src/tracking/tracker.py`` on MI355X.

Same public surface (``MultiObjectTracker(algorithm, **kwargs)``, ``.update(detections)``,
``Track``; reference lines 27-37, 200-259) over the single-launch HIP tracker behind
``include/rtmodt.h``.  Track state lives on the GPU; ``_core._tracks`` / ``_core._next_id``
(the parity surface, SURVEY.md finding 4) are materialised on demand in the reference's
list-of-dicts form.

Faithful to the reference, ``update()`` returns the tracks with ``time_since_update == 0``
*after* ageing -- which is none (``_age_tracks`` ages every track, reference line 146), so
the facade returns ``[]`` exactly as the reference does.  Set ``tracker.report = "matched"``
to get the tracks matched or spawned in this frame instead (opt-in, not reference behaviour).
"""
from __future__ import annotations

import ctypes as C
import logging
from collections import defaultdict
from dataclasses import dataclass, field

import numpy as np

from .. import _ffi

log = logging.getLogger("rtmodt.tracker")


@dataclass
class Track:
    """One tracked object (reference: tracker.py:27-37)."""
    track_id: int
    xyxy: np.ndarray
    confidence: float
    class_id: int
    class_name: str = ""
    age: int = 0
    time_since_update: int = 0
    trail: list = field(default_factory=list)


class _ByteTrackCore(_ffi.Handle):
    """Host face of the device tracker (reference: tracker.py:43-148).  ``n_streams``
    independent states are advanced by one kernel launch (one workgroup each)."""

    def __init__(self, track_thresh: float = 0.5, track_buffer: int = 30, match_thresh: float = 0.8, *,
                 device=0, max_tracks: int = 2048, max_dets: int = 1024, n_streams: int = 1,
                 assign_mode: int = _ffi.ASSIGN_GREEDY, kalman: bool = False) -> None:
        self.track_thresh = track_thresh
        self.track_buffer = track_buffer
        self.match_thresh = match_thresh
        self.max_tracks, self.max_dets, self.n_streams = max_tracks, max_dets, n_streams
        self._device = _ffi.device_ordinal(device)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_tracker_create(self._device, float(track_thresh), int(track_buffer), float(match_thresh),
                                                    int(assign_mode), int(max_tracks), int(max_dets), int(n_streams), C.byref(h)))
        self._h = h
        self.assign_mode = int(assign_mode)
        if self.assign_mode == _ffi.ASSIGN_LAPJV:        # tracker.py:170: cost_limit = 1 - thresh in Python doubles
            _ffi.check(_ffi.lib().rtmodt_tracker_set_cost_limit(self._h, float(1 - match_thresh)))
        #: opt-in constant-velocity Kalman motion model (no reference counterpart; include/rtmodt.h)
        self.kalman = bool(kalman)
        if self.kalman:
            _ffi.check(_ffi.lib().rtmodt_tracker_enable_kalman(self._h))

    # -- tracker.py:58-141 -------------------------------------------------------------
    def update(self, xyxy: np.ndarray, confidence: np.ndarray, class_id: np.ndarray, stream: int = 0) -> list:
        xyxy = np.ascontiguousarray(xyxy, dtype=np.float32).reshape(-1, 4)
        confidence = np.ascontiguousarray(confidence, dtype=np.float32).reshape(-1)
        class_id = np.ascontiguousarray(class_id, dtype=np.int32).reshape(-1)
        n_active = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_tracker_update(self._h, stream, _ffi.ptr(xyxy), _ffi.ptr(confidence), _ffi.ptr(class_id),
                                                    len(confidence), C.byref(n_active)))
        if n_active.value == 0:                          # always, as in the reference (tracker.py:141 after :146)
            return []
        return [t for t in self.tracks(stream) if t["time_since_update"] == 0]

    def update_batch(self, xyxy: np.ndarray, confidence: np.ndarray, class_id: np.ndarray, counts) -> np.ndarray:
        """All streams at once: arrays shaped [n_streams, max_dets(, 4)], ``counts[n_streams]``."""
        S, N = self.n_streams, self.max_dets
        xyxy = np.ascontiguousarray(xyxy, np.float32).reshape(S, N, 4)
        confidence = np.ascontiguousarray(confidence, np.float32).reshape(S, N)
        class_id = np.ascontiguousarray(class_id, np.int32).reshape(S, N)
        counts = np.ascontiguousarray(counts, np.int32).reshape(S)
        act = np.zeros(S, np.int32)
        _ffi.check(_ffi.lib().rtmodt_tracker_update_batch(self._h, _ffi.ptr(xyxy), _ffi.ptr(confidence), _ffi.ptr(class_id),
                                                          _ffi.ptr(counts), _ffi.ptr(act)))
        return act

    def update_from_detector(self, detector, first_frame: int = 0, n_frames: int = -1, frames_per_stream: int = 1) -> None:
        """Consume the detector's device-resident detections (stream i <- frame first_frame + i), no host hop.
        A batch with F consecutive frames per stream (image f * n_streams + s) takes F calls, f ascending -- or ONE call
        with ``frames_per_stream=F`` (``n_frames`` = streams): each stream's workgroup then walks over its F frames in order
        inside a single launch."""
        if frames_per_stream > 1:
            _ffi.check(_ffi.lib().rtmodt_tracker_update_from_detector_batch(self._h, detector.model.handle, int(first_frame),
                                                                            int(self.n_streams if n_frames < 0 else n_frames), int(frames_per_stream)))
        elif first_frame == 0 and n_frames < 0:
            _ffi.check(_ffi.lib().rtmodt_tracker_update_from_detector(self._h, detector.model.handle))
        else:
            _ffi.check(_ffi.lib().rtmodt_tracker_update_from_detector_frames(self._h, detector.model.handle, int(first_frame),
                                                                             int(self.n_streams if n_frames < 0 else n_frames)))

    def update_from_sliced(self, sliced) -> None:
        """Consume the MERGED detections of a ``SlicedDetector``'s newest batch (stream i <- frame i), device-resident, queued
        behind the merge kernel (``rtmodt_tracker_update_from_slicer``); needs ``max_dets >= sliced.max_out``."""
        _ffi.check(_ffi.lib().rtmodt_tracker_update_from_slicer(self._h, sliced._h))

    # -- parity surface ----------------------------------------------------------------
    def snapshot(self, stream: int = 0) -> dict:
        M = self.max_tracks
        ids, box = np.empty(M, np.int64), np.empty((M, 4), np.float32)
        conf, cls = np.empty(M, np.float32), np.empty(M, np.int32)
        age, tsu = np.empty(M, np.int32), np.empty(M, np.int32)
        n, nid = C.c_int32(0), C.c_int64(0)
        _ffi.check(_ffi.lib().rtmodt_tracker_state(self._h, stream, _ffi.ptr(ids), _ffi.ptr(box), _ffi.ptr(conf), _ffi.ptr(cls),
                                                   _ffi.ptr(age), _ffi.ptr(tsu), C.byref(n), C.byref(nid)))
        k = n.value
        return {"ids": ids[:k].copy(), "xyxy": box[:k].copy(), "conf": conf[:k].copy(), "cls": cls[:k].copy(),
                "age": age[:k].copy(), "tsu": tsu[:k].copy(), "next_id": int(nid.value)}

    def kalman_snapshot(self, stream: int = 0) -> dict:
        """Filter state in list order: ``mean`` (n, 8) = (cx, cy, a, h, vx, vy, va, vh), ``cov`` (n, 12) = (a, b, c) of the
        2x2 covariance block of each coordinate."""
        mean, cov = np.empty((self.max_tracks, 8), np.float32), np.empty((self.max_tracks, 12), np.float32)
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_tracker_kalman_state(self._h, stream, _ffi.ptr(mean), _ffi.ptr(cov), C.byref(n)))
        return {"mean": mean[:n.value].copy(), "cov": cov[:n.value].copy()}

    def tracks(self, stream: int = 0) -> list:
        s = self.snapshot(stream)
        return [{"track_id": int(s["ids"][i]), "xyxy": s["xyxy"][i], "confidence": float(s["conf"][i]),
                 "class_id": int(s["cls"][i]), "age": int(s["age"][i]), "time_since_update": int(s["tsu"][i])}
                for i in range(len(s["ids"]))]

    @property
    def _tracks(self) -> list:                            # the reference's attribute name
        return self.tracks(0)

    @property
    def _next_id(self) -> int:
        return self.snapshot(0)["next_id"]

    def reset(self, stream: int = -1) -> None:
        _ffi.check(_ffi.lib().rtmodt_tracker_reset(self._h, stream))

    _destroy = "rtmodt_tracker_destroy"


class MultiObjectTracker:
    """Tracker facade (reference: tracker.py:200-259)."""

    #: "reference" -> tracks with time_since_update == 0 after ageing (always []);
    #: "matched"   -> tracks matched or spawned this frame (time_since_update == 1).
    report = "reference"
    #: which branch of _linear_assignment (tracker.py:163-194) runs: the reference takes "lapjv" when the
    #: optional ``lap`` package imports and "greedy" otherwise; "greedy" is the branch pinned by fixtures.
    assignment = "greedy"

    def __init__(self, algorithm: str = "bytetrack", **kwargs) -> None:
        self.algorithm = algorithm.lower()
        if self.algorithm == "bytetrack":
            p = kwargs.get("bytetrack", kwargs)           # flat kwargs or nested dict; unknown keys ignored
            self.assignment = p.get("assignment", type(self).assignment)
            self._core = _ByteTrackCore(
                track_thresh=p.get("track_thresh", 0.5),
                track_buffer=p.get("track_buffer", 30),
                match_thresh=p.get("match_thresh", 0.8),
                device=p.get("device", kwargs.get("device", 0)),
                max_tracks=p.get("max_tracks", 2048),
                max_dets=p.get("max_dets", 1024),
                assign_mode={"greedy": _ffi.ASSIGN_GREEDY, "lapjv": _ffi.ASSIGN_LAPJV}[self.assignment],
                kalman=bool(p.get("kalman", kwargs.get("kalman", False))),
            )
        elif self.algorithm == "deepsort":
            raise NotImplementedError("DeepSORT adapter not yet wired. Use bytetrack.")
        else:
            raise ValueError(f"Unknown tracker: {self.algorithm}")
        self._trail_map = defaultdict(list)
        self._trail_maxlen = 30
        log.info("Tracker initialised: %s", self.algorithm)

    def update_from_detector(self, detector, materialize: bool = True) -> list:
        """:meth:`update` fed from ``detector``'s device-resident detections of its last ``detect`` / ``enqueue`` (no host
        hop: the tracker launch is queued behind the detector's NMS).  ``materialize=False`` skips the read-back of the
        track list -- for loops whose next stage consumes the device-resident state (``ZoneEventEngine.process_tracker``)."""
        self._core.update_from_detector(detector)
        if not materialize or self.report != "matched":
            return []                                     # reference mode: tracks with tsu == 0 after ageing -- none (tracker.py:141,146)
        return self._tracks_out([])

    def update_from_sliced(self, sliced, materialize: bool = True) -> list:
        """:meth:`update_from_detector` for a ``SlicedDetector``: the tracker consumes the merged, frame-coordinate detections of
        its last ``detect`` / ``enqueue`` on the device."""
        self._core.update_from_sliced(sliced)
        if not materialize or self.report != "matched":
            return []
        return self._tracks_out([])

    def update(self, detections) -> list:
        """``detections`` is duck-typed on ``.xyxy / .confidence / .class_id`` (tracker.py:234-238)."""
        raw = self._core.update(detections.xyxy, detections.confidence, detections.class_id)
        return self._tracks_out(raw)

    def _tracks_out(self, raw: list) -> list:
        if self.report == "matched":
            st = self._core.snapshot(0)
            raw = [{"track_id": int(st["ids"][i]), "xyxy": st["xyxy"][i], "confidence": float(st["conf"][i]), "class_id": int(st["cls"][i]),
                    "age": int(st["age"][i]), "time_since_update": 1} for i in np.nonzero(st["tsu"] == 1)[0]]
        out = []
        for r in raw:
            tid = r["track_id"]
            b = r["xyxy"]
            cx = int((b[0] + b[2]) / 2)                   # float32 arithmetic, truncation (tracker.py:243-244)
            cy = int((b[1] + b[3]) / 2)
            trail = self._trail_map[tid]
            trail.append((cx, cy))
            if len(trail) > self._trail_maxlen:
                trail.pop(0)
            out.append(Track(track_id=tid, xyxy=b, confidence=r["confidence"], class_id=r["class_id"],
                             age=r["age"], time_since_update=r["time_since_update"], trail=list(trail)))
        return out
