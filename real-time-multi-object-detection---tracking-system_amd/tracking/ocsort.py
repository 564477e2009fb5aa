"""OC-SORT on MI355X: the motion-only tracker of the reference's tracker comparison (TECHNICAL_DESIGN_DOCUMENT.md H.2, row 4: no
Re-ID model), which the reference lists and never builds.  ``MultiObjectTracker`` does not learn ``"ocsort"``; this class is the
way in, as ``DeepSortTracker`` is for DeepSORT.

The algorithm is the published one (Cao et al., "Observation-Centric SORT", CVPR 2023) as this project reads it, with the state
resident on the GPU behind ``rtmodt_ocsort_*`` (``include/rtmodt.h``, ``csrc/ocsort.hip``): direction consistency in the first
association (OCM), recovery on the last observation (OCR), and the re-update of the filter across an occlusion (ORU).  PINNED: the
kernel equals the plain-Python restatement ``tests/ocsort_ref.py`` bit for bit.  PARITY UNPINNED: ``ocsort``, ``boxmot`` and
``filterpy`` are installed nowhere this runs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi
from ._common import TrailKeeper, pad_single_stream
from .tracker import Track

DEFAULT_MAX_TRACKS = 256
DEFAULT_MAX_DETS = 1024


class _OcSortCore(_ffi.Handle):
    """Host face of the device tracker: ``n_streams`` independent states advanced by one call (one launch)."""

    def __init__(self, det_thresh=0.6, low_thresh=0.1, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3, inertia=0.2, use_byte=False, *,
                 device=0, max_tracks: int = DEFAULT_MAX_TRACKS, max_dets: int = DEFAULT_MAX_DETS, n_streams: int = 1) -> None:
        self.max_tracks, self.max_dets, self.n_streams, self.min_hits = int(max_tracks), int(max_dets), int(n_streams), int(min_hits)
        self._device = _ffi.device_ordinal(device)
        cfg = _ffi.OcSortCfg(float(det_thresh), float(low_thresh), float(iou_threshold), float(inertia), int(max_age), int(min_hits), int(delta_t),
                             1 if use_byte else 0, self.max_tracks, self.max_dets, self.n_streams, self._device)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_ocsort_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def update_batch(self, xyxy, confidence, class_id, counts) -> np.ndarray:
        """All streams at once: arrays shaped ``[n_streams, max_dets(, 4)]``, ``counts[n_streams]``.  Returns the number of tracks
        returned this frame, per stream."""
        S, N = self.n_streams, self.max_dets
        xyxy = np.ascontiguousarray(xyxy, np.float32).reshape(S, N, 4)
        confidence = np.ascontiguousarray(confidence, np.float32).reshape(S, N)
        class_id = np.ascontiguousarray(class_id, np.int32).reshape(S, N)
        counts = np.ascontiguousarray(counts, np.int32).reshape(S)
        ret = np.zeros(S, np.int32)
        _ffi.check(_ffi.lib().rtmodt_ocsort_update_batch(self._h, _ffi.ptr(xyxy), _ffi.ptr(confidence), _ffi.ptr(class_id), _ffi.ptr(counts), _ffi.ptr(ret)))
        return ret

    def update(self, xyxy, confidence, class_id, stream: int = 0) -> int:
        """One frame of a single-stream tracker."""
        if self.n_streams != 1 or stream != 0:
            raise ValueError("update() drives a single-stream tracker; use update_batch for several streams")
        bx, cf, cl, n = pad_single_stream(xyxy, confidence, class_id, self.max_dets)
        return int(self.update_batch(bx, cf, cl, [n])[0])

    def update_from_detector(self, detector) -> None:
        """Consume the detector's device-resident detections of its last batch (stream i <- frame i), asynchronously on the
        detector's stream behind its NMS: no host hop."""
        _ffi.check(_ffi.lib().rtmodt_ocsort_update_from_detector(self._h, detector.model.handle))

    def snapshot(self, stream: int = 0, allow_capacity: bool = False) -> dict:
        """The parity surface (``rtmodt_ocsort_state``), list order.  ``allow_capacity``: a stream in sticky ``E_CAPACITY`` error is
        still read (the call fills its outputs before it reports the error) and the dict carries ``"error"``."""
        M = self.max_tracks
        ids = np.zeros(M, np.int64)
        hits, streak, age, tsu, cls = (np.zeros(M, np.int32) for _ in range(5))
        box, conf = np.zeros((M, 4), np.float32), np.zeros(M, np.float32)
        mean, cov, direction = np.zeros((M, 8), np.float32), np.zeros((M, 12), np.float32), np.zeros((M, 2), np.float32)
        n, nid, fc = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        rc = _ffi.lib().rtmodt_ocsort_state(self._h, stream, _ffi.ptr(ids), _ffi.ptr(hits), _ffi.ptr(streak), _ffi.ptr(age), _ffi.ptr(tsu), _ffi.ptr(box),
                                            _ffi.ptr(conf), _ffi.ptr(cls), _ffi.ptr(mean), _ffi.ptr(cov), _ffi.ptr(direction), C.byref(n), C.byref(nid),
                                            C.byref(fc))
        if not (allow_capacity and rc == _ffi.E_CAPACITY):
            _ffi.check(rc)
        k = n.value
        out = {"ids": ids[:k].copy(), "hits": hits[:k].copy(), "hit_streak": streak[:k].copy(), "age": age[:k].copy(), "tsu": tsu[:k].copy(),
               "xyxy": box[:k].copy(), "conf": conf[:k].copy(), "cls": cls[:k].copy(), "mean": mean[:k].copy(), "cov": cov[:k].copy(),
               "dir": direction[:k].copy(), "next_id": int(nid.value), "frame_count": int(fc.value)}
        if rc != _ffi.OK:
            out["error"] = rc
        return out

    def returned(self, st: dict) -> np.ndarray:
        """Indices of the tracks of a snapshot that this frame returns."""
        return np.nonzero((st["tsu"] == 0) & ((st["hit_streak"] >= self.min_hits) | (st["frame_count"] <= self.min_hits)))[0]

    def last_ms(self) -> float:
        """Device time (ms) of the last update's launch."""
        return _ffi.last_ms("rtmodt_ocsort_last_ms", self._h)

    def reset(self, stream: int = -1) -> None:
        _ffi.check(_ffi.lib().rtmodt_ocsort_reset(self._h, stream))

    _destroy = "rtmodt_ocsort_destroy"


class OcSortTracker:
    """``update(detections) -> list[Track]``: the tracks matched in this frame whose hit streak has reached ``min_hits`` (every
    matched or new-born track during the first ``min_hits`` frames, as published); ``xyxy`` = the matched detection, trails as
    ``MultiObjectTracker`` keeps them.  Class-agnostic: a track carries the class of its last matched detection."""

    #: motion only: ``pipeline.run`` does not hand it the frame
    needs_frame = False
    #: the zone engine reads only a ByteTrack handle on the device: ``pipeline.run`` hands it this tracker's materialised list
    zone_events_on_device = False

    def __init__(self, det_thresh: float = 0.6, low_thresh: float = 0.1, max_age: int = 30, min_hits: int = 3, iou_threshold: float = 0.3,
                 delta_t: int = 3, inertia: float = 0.2, use_byte: bool = False, *, device=0, max_tracks: int = DEFAULT_MAX_TRACKS,
                 max_dets: int = DEFAULT_MAX_DETS) -> None:
        self.algorithm = "ocsort"
        self._core = _OcSortCore(det_thresh, low_thresh, max_age, min_hits, iou_threshold, delta_t, inertia, use_byte, device=device,
                                 max_tracks=max_tracks, max_dets=max_dets)
        self._trails = TrailKeeper()

    @classmethod
    def from_config(cls, tracking_cfg: dict, **extra) -> "OcSortTracker":
        """``cfg["tracking"]`` of a configuration in the reference's YAML layout: reads its ``ocsort:`` block (the reference's
        default.yaml has none; the keys are this constructor's)."""
        p = dict(tracking_cfg.get("ocsort", {}))
        p.update(extra)
        known = ("det_thresh", "low_thresh", "max_age", "min_hits", "iou_threshold", "delta_t", "inertia", "use_byte", "device", "max_tracks",
                 "max_dets")
        return cls(**{k: v for k, v in p.items() if k in known})

    def update(self, detections) -> list:
        ret = self._core.update(detections.xyxy, detections.confidence, detections.class_id)
        return self._tracks_out() if ret else []

    def update_from_detector(self, detector, materialize: bool = True) -> list:
        """:meth:`update` fed from ``detector``'s device-resident detections of its last ``detect``."""
        self._core.update_from_detector(detector)
        return self._tracks_out() if materialize else []

    def _tracks_out(self) -> list:
        st = self._core.snapshot(0)
        self._trails.drop_dead(st["ids"])
        out = []
        for i in self._core.returned(st):
            tid, b = int(st["ids"][i]), st["xyxy"][i]
            out.append(Track(track_id=tid, xyxy=b, confidence=float(st["conf"][i]), class_id=int(st["cls"][i]), age=int(st["age"][i]),
                             time_since_update=0, trail=self._trails.push(tid, b)))
        return out

    def close(self) -> None:
        self._core.close()
