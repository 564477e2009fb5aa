"""BoT-SORT on MI355X: the tracker the reference's comparison ranks best (TECHNICAL_DESIGN_DOCUMENT.md H.2, row 3: IDF1 0.83, 38
switches, "Req. Re-ID Model: Yes") and never builds.  ``MultiObjectTracker`` does not learn ``"botsort"``; this class is the way in,
as ``DeepSortTracker`` and ``OcSortTracker`` are for theirs.

The algorithm is the published one (Aharon et al., "BoT-SORT: Robust Associations Multi-Pedestrian Tracking", 2022) as this project
reads it, with the state resident on the GPU behind ``rtmodt_botsort_*`` (``include/rtmodt.h``, ``csrc/botsort.hip``): the Kalman
states are compensated for camera motion by a warp the caller supplies, and IoU is fused with the detection score and with
appearance.  PINNED: the kernel equals the plain-Python restatement ``tests/botsort_ref.py`` bit for bit.  PARITY UNPINNED:
``BoT-SORT`` and ``boxmot`` are installed nowhere this runs.  The warp comes from whoever has it (PTZ telemetry) or, with ``gmc=``, from
``tracking.gmc.CameraMotionEstimator``, which computes it from the frames on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi
from ._common import TrailKeeper, pad_single_stream
from ..reid_weights import FEAT_DIM, SUFFIX
from .reid import check_weights_path
from .tracker import Track

NEW, TRACKED, LOST = 1, 2, 3
DEFAULT_MAX_TRACKS = 256
DEFAULT_MAX_DETS = 1024
#: with an embedder network every detection slot holds the crop's tap tensors and scratch (see ``DeepSortTracker``)
DEFAULT_MAX_DETS_NETWORK = 128
NO_EMBEDDER = "none"
BUILTIN_EMBEDDER = "colorhist"
BUILTIN_DIM = 192


def _mean_to_xyxy(m: np.ndarray) -> np.ndarray:
    """The tracker's own rule (csrc/botsort.hip: bot_mean_to_box), float32 operation by operation."""
    m = np.asarray(m, np.float32).reshape(-1, 4)
    x1 = m[:, 0] - m[:, 2] * np.float32(0.5)
    y1 = m[:, 1] - m[:, 3] * np.float32(0.5)
    return np.stack([x1, y1, x1 + m[:, 2], y1 + m[:, 3]], 1).astype(np.float32)


def check_warp(warp, n_streams: int = 1):
    """``warp`` as ``[n_streams, 2, 3]`` float32 (``None`` stays ``None``); a non-finite entry or ``|det R| < 1e-6`` raises
    (``rtmodt_botsort_check_warp``: no device needed)."""
    if warp is None:
        return None
    warp = np.ascontiguousarray(warp, np.float32).reshape(n_streams, 6)
    _ffi.check(_ffi.lib().rtmodt_botsort_check_warp(_ffi.ptr(warp), int(n_streams)))
    return warp


class _BotSortCore(_ffi.Handle):
    """Host face of the device tracker: ``n_streams`` independent states advanced by one call (a fixed number of launches)."""

    def __init__(self, track_high_thresh=0.6, track_low_thresh=0.1, new_track_thresh=0.7, track_buffer=30, match_thresh=0.8,
                 proximity_thresh=0.5, appearance_thresh=0.25, fuse_score=True, embedder=NO_EMBEDDER, *, dim: int = 0, device=0,
                 max_tracks: int = DEFAULT_MAX_TRACKS, max_dets: int = DEFAULT_MAX_DETS, n_streams: int = 1) -> None:
        self.max_tracks, self.max_dets, self.n_streams = int(max_tracks), int(max_dets), int(n_streams)
        none = embedder in (None, "", NO_EMBEDDER)
        self.dim = 0 if none else int(dim) or (FEAT_DIM if str(embedder).endswith(SUFFIX) else BUILTIN_DIM)
        self._device = _ffi.device_ordinal(device)
        emb = None if embedder is None else str(embedder).encode()
        cfg = _ffi.BotSortCfg(float(track_high_thresh), float(track_low_thresh), float(new_track_thresh), int(track_buffer), float(match_thresh),
                              float(proximity_thresh), float(appearance_thresh), 1 if fuse_score else 0, emb, int(dim), self.max_tracks,
                              self.max_dets, self.n_streams, self._device)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_botsort_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def update_batch(self, xyxy, confidence, class_id, counts, frames=None, embeddings=None, warp=None, *, mem_kind=_ffi.MEM_HOST, height=0,
                     width=0, stride=0) -> np.ndarray:
        """All streams at once: arrays shaped ``[n_streams, max_dets(, 4)]``, ``counts[n_streams]``; with an embedder either
        ``frames`` (one per stream, as ``_DeepSortCore.update_batch`` takes them) or ``embeddings`` (``[n_streams, max_dets, dim]``
        int8); ``warp`` ``[n_streams, 2, 3]`` (row-major ``[R | t]``, the image motion from the previous frame to this one; ``None`` =
        identity).  Returns the number of tracks with flag 2 after the frame, per stream."""
        S, N = self.n_streams, self.max_dets
        xyxy = np.ascontiguousarray(xyxy, np.float32).reshape(S, N, 4)
        confidence = np.ascontiguousarray(confidence, np.float32).reshape(S, N)
        class_id = np.ascontiguousarray(class_id, np.int32).reshape(S, N)
        counts = np.ascontiguousarray(counts, np.int32).reshape(S)
        fp, keep = None, None
        if frames is not None:
            if len(frames) != S:
                raise ValueError(f"{len(frames)} frames for {S} streams")
            fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        if embeddings is not None:
            embeddings = np.ascontiguousarray(embeddings, np.int8)          # (a motion-only handle refuses them: the library says so)
            if self.dim:
                embeddings = embeddings.reshape(S, N, self.dim)
        if warp is not None:
            warp = np.ascontiguousarray(warp, np.float32).reshape(S, 6)
        ret = np.zeros(S, np.int32)
        _ffi.check(_ffi.lib().rtmodt_botsort_update_batch(self._h, _ffi.ptr(xyxy), _ffi.ptr(confidence), _ffi.ptr(class_id), _ffi.ptr(counts), fp,
                                                          int(height), int(width), int(stride), int(mem_kind), _ffi.ptr(embeddings), _ffi.ptr(warp),
                                                          _ffi.ptr(ret)))
        del keep
        return ret

    def update(self, xyxy, confidence, class_id, frame=None, embeddings=None, warp=None, stream: int = 0) -> int:
        """One frame of a single-stream tracker."""
        if self.n_streams != 1 or stream != 0:
            raise ValueError("update() drives a single-stream tracker; use update_batch for several streams")
        bx, cf, cl, n = pad_single_stream(xyxy, confidence, class_id, self.max_dets)
        emb = None
        if embeddings is not None:
            emb = np.zeros((1, self.max_dets, self.dim), np.int8)
            emb[0, :n] = np.asarray(embeddings, np.int8).reshape(n, self.dim)
        return int(self.update_batch(bx, cf, cl, [n], None if frame is None else [frame], emb, warp)[0])

    def update_from_detector(self, detector, frames=None, warp=None, *, mem_kind=_ffi.MEM_HOST, height=0, width=0, stride=0) -> None:
        """Consume the detector's device-resident detections of its last batch (stream i <- frame i), asynchronously on the
        detector's stream: no host hop.  ``frames``: the frames that batch was made of (a handle with an embedder describes the
        detections on them); ``warp`` ``[len(batch), 2, 3]``."""
        fp, keep, n = None, None, 0
        if frames is not None:
            fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
            n = len(frames)
        if warp is not None:
            warp = np.ascontiguousarray(warp, np.float32).reshape(-1, 6)
        _ffi.check(_ffi.lib().rtmodt_botsort_update_from_detector(self._h, detector.model.handle, fp, n, int(height), int(width), int(stride),
                                                                  int(mem_kind), _ffi.ptr(warp)))
        if keep:                                         # pageable host frames: the copy has been issued from them; wait before they may go
            _ffi.check(_ffi.lib().rtmodt_synchronize(self._device))

    def update_from_detector_gmc(self, detector, gmc, frames, *, mem_kind=_ffi.MEM_HOST, height=0, width=0, stride=0) -> None:
        """:meth:`update_from_detector` with the warp estimated by ``gmc`` (a ``CameraMotionEstimator``) from the same frames: the
        estimate and the update are queued on the detector's stream and the warp never leaves the device."""
        fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        _ffi.check(_ffi.lib().rtmodt_botsort_update_from_detector_gmc(self._h, detector.model.handle, gmc.handle, fp, len(frames), int(height),
                                                                      int(width), int(stride), int(mem_kind)))
        gmc._geom = (int(height), int(width))
        if keep:
            _ffi.check(_ffi.lib().rtmodt_synchronize(self._device))

    def snapshot(self, stream: int = 0, allow_capacity: bool = False, features: bool = True) -> dict:
        """The parity surface (``rtmodt_botsort_state``), list order.  ``allow_capacity``: a stream in sticky ``E_CAPACITY`` error is
        still read (the call fills its outputs before it reports the error) and the dict carries ``"error"``."""
        M, D = self.max_tracks, self.dim
        ids = np.zeros(M, np.int64)
        flag, age, tsu, start, last, cls = (np.zeros(M, np.int32) for _ in range(6))
        box, conf = np.zeros((M, 4), np.float32), np.zeros(M, np.float32)
        mean, cov = np.zeros((M, 8), np.float32), np.zeros((M, 20), np.float32)
        f16, f8 = (np.zeros((M, D), np.int16), np.zeros((M, D), np.int8)) if features and D else (None, None)
        n, nid, fc = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        rc = _ffi.lib().rtmodt_botsort_state(self._h, stream, _ffi.ptr(ids), _ffi.ptr(flag), _ffi.ptr(age), _ffi.ptr(tsu), _ffi.ptr(start),
                                             _ffi.ptr(last), _ffi.ptr(box), _ffi.ptr(conf), _ffi.ptr(cls), _ffi.ptr(mean), _ffi.ptr(cov), _ffi.ptr(f16),
                                             _ffi.ptr(f8), C.byref(n), C.byref(nid), C.byref(fc))
        if not (allow_capacity and rc == _ffi.E_CAPACITY):
            _ffi.check(rc)
        k = n.value
        out = {"ids": ids[:k].copy(), "flag": flag[:k].copy(), "age": age[:k].copy(), "tsu": tsu[:k].copy(), "start_frame": start[:k].copy(),
               "last_frame": last[:k].copy(), "xyxy": box[:k].copy(), "conf": conf[:k].copy(), "cls": cls[:k].copy(), "mean": mean[:k].copy(),
               "cov": cov[:k].copy(), "next_id": int(nid.value), "frame_count": int(fc.value)}
        if features:
            out["feat16"] = f16[:k].copy() if D else np.zeros((k, 0), np.int16)
            out["feat8"] = f8[:k].copy() if D else np.zeros((k, 0), np.int8)
        if rc != _ffi.OK:
            out["error"] = rc
        return out

    @staticmethod
    def returned(st: dict) -> np.ndarray:
        """Indices of the tracks of a snapshot that this frame returns."""
        return np.nonzero(st["flag"] == TRACKED)[0]

    def last_ms(self) -> tuple:
        """Device time (ms) of the last update: (descriptors, distance, update)."""
        return _ffi.last_ms("rtmodt_botsort_last_ms", self._h, 3)

    def reset(self, stream: int = -1) -> None:
        _ffi.check(_ffi.lib().rtmodt_botsort_reset(self._h, stream))

    _destroy = "rtmodt_botsort_destroy"


class BotSortTracker:
    """``update(detections, frame=None, warp=None) -> list[Track]``: every activated track (flag 2), matched this frame or not, as
    published; ``xyxy`` = the box of the filter's mean, ``time_since_update`` tells the two apart; trails as ``MultiObjectTracker``
    keeps them.  ``embedder``: ``"none"`` (motion only), ``"colorhist"`` (the built-in descriptor, computed from ``frame``; or with
    ``embedding_dim`` caller descriptors through ``embeddings=``) or an ``.rtreid`` file (the OSNet x0.25 network).  ``warp``: the
    2x3 image motion from the previous frame to this one.  ``gmc``: a ``CameraMotionEstimator``; with one, ``update`` estimates the
    warp from ``frame`` (masking with the frame's detections) when no ``warp`` is passed, ``update_from_detector`` keeps estimate and
    update on the device, and ``pipeline.run`` hands the frame over; passing both ``gmc`` and an explicit ``warp`` raises.  Class-agnostic: a track carries the class of its last matched detection."""

    #: the zone engine reads only a ByteTrack handle on the device: ``pipeline.run`` hands it this tracker's materialised list
    zone_events_on_device = False

    def __init__(self, track_high_thresh: float = 0.6, track_low_thresh: float = 0.1, new_track_thresh: float = 0.7, track_buffer: int = 30,
                 match_thresh: float = 0.8, proximity_thresh: float = 0.5, appearance_thresh: float = 0.25, fuse_score: bool = True,
                 embedder: str = NO_EMBEDDER, *, embedding_dim: int = 0, device=0, max_tracks: int = DEFAULT_MAX_TRACKS,
                 max_dets: int | None = None, gmc=None) -> None:
        if gmc is not None and gmc.n_streams != 1:
            raise ValueError("BotSortTracker drives one stream: its estimator must have n_streams == 1")
        self.gmc = gmc
        if embedder in (None, ""):
            embedder = NO_EMBEDDER
        if str(embedder).endswith(SUFFIX):
            embedder = check_weights_path(embedder)             # FileNotFoundError, as the detector words it
            if embedding_dim not in (0, FEAT_DIM):
                raise ValueError(f"embedding_dim {embedding_dim}: the network's descriptor has {FEAT_DIM} values")
        elif embedder not in (NO_EMBEDDER, BUILTIN_EMBEDDER):
            raise NotImplementedError(
                f"embedder {embedder!r}: no embedding network runs here, only the built-in {BUILTIN_EMBEDDER!r} descriptor. Run the model "
                "yourself and pass its output per detection as update(..., embeddings=) on a tracker built with embedding_dim=<its dimension>. "
                f"An OSNet x0.25 checkpoint converted with tools/convert_weights.py --reid (a {SUFFIX} file) does run here.")
        if embedder == NO_EMBEDDER and embedding_dim:
            embedder = BUILTIN_EMBEDDER                         # caller descriptors of that dimension
        if max_dets is None:
            max_dets = DEFAULT_MAX_DETS_NETWORK if str(embedder).endswith(SUFFIX) else DEFAULT_MAX_DETS
        self.algorithm = "botsort"
        self.embedder = embedder
        self._core = _BotSortCore(track_high_thresh, track_low_thresh, new_track_thresh, track_buffer, match_thresh, proximity_thresh,
                                  appearance_thresh, fuse_score, embedder, dim=embedding_dim, device=device, max_tracks=max_tracks, max_dets=max_dets)
        #: ``pipeline.run`` hands the frame to a tracker that describes its detections on it
        self._describes = str(embedder).endswith(SUFFIX) or (embedder == BUILTIN_EMBEDDER and self._core.dim == BUILTIN_DIM)
        self.needs_frame = self._describes or gmc is not None
        self._trails = TrailKeeper()

    @classmethod
    def from_config(cls, tracking_cfg: dict, **extra) -> "BotSortTracker":
        """``cfg["tracking"]`` of a configuration in the reference's YAML layout: reads its ``botsort:`` block (the reference's
        default.yaml has none; the keys are this constructor's)."""
        p = dict(tracking_cfg.get("botsort", {}))
        p.update(extra)
        known = ("track_high_thresh", "track_low_thresh", "new_track_thresh", "track_buffer", "match_thresh", "proximity_thresh",
                 "appearance_thresh", "fuse_score", "embedder", "embedding_dim", "device", "max_tracks", "max_dets")
        return cls(**{k: v for k, v in p.items() if k in known})

    def _estimate(self, detections, frame, warp):
        if self.gmc is None:
            return warp
        if warp is not None:
            raise ValueError("this tracker estimates the warp itself (gmc=): pass no warp")
        if frame is None:
            raise ValueError("a tracker with an estimator (gmc=) needs the frame")
        return self.gmc.estimate([frame], [detections])[0]

    def update(self, detections, frame=None, warp=None, embeddings=None) -> list:
        n = len(detections.confidence)
        warp = self._estimate(detections, frame, warp)
        if self.embedder == NO_EMBEDDER:
            frame = None                                        # motion only: the frame pipeline.run may offer is not used
            if embeddings is not None:
                raise ValueError("this tracker runs on motion only (embedder 'none'): it takes no embeddings")
        elif n and (frame is None) == (embeddings is None):
            raise ValueError("update() needs exactly one of frame= (the embedder describes the detections) or embeddings= (one row per detection)")
        if embeddings is not None:
            embeddings = np.asarray(embeddings)
            if embeddings.dtype != np.int8:
                embeddings = _ffi.appearance_quantize(embeddings)
        self._core.update(detections.xyxy, detections.confidence, detections.class_id, frame if n else None, embeddings if n else None,
                          check_warp(warp))
        return self._tracks_out()

    def update_from_detector(self, detector, frame=None, materialize: bool = True, warp=None) -> list:
        """:meth:`update` fed from ``detector``'s device-resident detections of its last ``detect`` on ``frame``."""
        if self.needs_frame and frame is None:
            raise ValueError("update_from_detector() needs the frame the detector ran on")
        if self.gmc is not None:
            if warp is not None:
                raise ValueError("this tracker estimates the warp itself (gmc=): pass no warp")
            self._core.update_from_detector_gmc(detector, self.gmc, [frame])
        else:
            self._core.update_from_detector(detector, [frame] if self._describes else None, check_warp(warp))
        return self._tracks_out() if materialize else []

    def _tracks_out(self) -> list:
        st = self._core.snapshot(0, features=False)
        boxes = _mean_to_xyxy(st["mean"][:, :4])
        self._trails.drop_dead(st["ids"])
        out = []
        for i in self._core.returned(st):
            tid, b = int(st["ids"][i]), boxes[i]
            out.append(Track(track_id=tid, xyxy=b, confidence=float(st["conf"][i]), class_id=int(st["cls"][i]), age=int(st["age"][i]),
                             time_since_update=int(st["tsu"][i]), trail=self._trails.push(tid, b)))
        return out

    def close(self) -> None:
        self._core.close()
