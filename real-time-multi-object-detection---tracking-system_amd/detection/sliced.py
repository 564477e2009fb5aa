"""Sliced inference (the SAHI scheme) around :class:`Detector`, for frames much larger than the network input.

The reference feeds 1920 x 1080 frames to a 640 x 640 detector (``config/default.yaml:24-26, 34``) and its design document lists
"Missed small objects" among the failures (B.4) without a cure that keeps the model.  ``SlicedDetector`` cuts every frame into
overlapping tiles at native resolution plus one letterboxed overview, runs the native detector on that image batch and merges
the boxes back in frame coordinates -- the cut and the merge on the GPU (``csrc/slice.hip``), no host round trip in between.

Pinned bit for bit against ``tests/slice_ref.py``: tile bytes, per-image detections, the merge.  Parity with the ``sahi``
package is unpinned (it is installed nowhere this runs), and so is any accuracy gain on real footage.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from .. import _ffi
from .detector import Detections, Detector, _empty

MERGES = {"nmm": _ffi.SLICE_MERGE_NMM, "nms": _ffi.SLICE_MERGE_NMS}
METRICS = {"ios": _ffi.SLICE_METRIC_IOS, "iou": _ffi.SLICE_METRIC_IOU}


def slice_cfg(frame_size, tile=(640, 640), overlap=(128, 128), overview=True, merge="nmm", metric="ios", match_threshold=0.5,
              agnostic=False, max_out=300, max_frames=1, device=0) -> "_ffi.SliceCfg":
    """``rtmodt_slice_cfg`` from (width, height) pairs and names."""
    if str(merge).lower() not in MERGES:
        raise ValueError(f"merge {merge!r}: one of {sorted(MERGES)}")
    if str(metric).lower() not in METRICS:
        raise ValueError(f"metric {metric!r}: one of {sorted(METRICS)}")
    return _ffi.SliceCfg(int(device), int(frame_size[0]), int(frame_size[1]), int(tile[0]), int(tile[1]), int(overlap[0]), int(overlap[1]),
                         int(bool(overview)), MERGES[str(merge).lower()], METRICS[str(metric).lower()], float(match_threshold),
                         int(bool(agnostic)), int(max_out), int(max_frames))


def slice_grid(frame_size, tile=(640, 640), overlap=(128, 128)):
    """Tile origins ``[(x, y), ...]`` in row-major order and the effective tile ``(te_w, te_h)`` (``rtmodt_slice_grid``, host only)."""
    xs, ys = np.zeros(64, np.int32), np.zeros(64, np.int32)
    n, tw, th = C.c_int32(), C.c_int32(), C.c_int32()
    _ffi.check(_ffi.lib().rtmodt_slice_grid(int(frame_size[0]), int(frame_size[1]), int(tile[0]), int(tile[1]), int(overlap[0]), int(overlap[1]),
                                            _ffi.ptr(xs), _ffi.ptr(ys), C.byref(n), C.byref(tw), C.byref(th)))
    return [(int(xs[i]), int(ys[i])) for i in range(n.value)], (tw.value, th.value)


def slice_merge(cfg: "_ffi.SliceCfg", xyxy, conf, cls, counts, device: int = 0, want_ms: bool = False):
    """``rtmodt_slice_merge``: the merge kernel alone on per-image detections ``xyxy[F * I, max_det, 4]``, ``conf / cls[F * I, max_det]``,
    ``counts[F * I]`` -> per frame ``(xyxy, conf, cls, n_merged)`` arrays of its keepers (with ``want_ms``: that list and the launch's
    device ms)."""
    xyxy = np.ascontiguousarray(xyxy, np.float32)
    conf = np.ascontiguousarray(conf, np.float32)
    cls = np.ascontiguousarray(cls, np.int32)
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    images, max_det = conf.shape
    per = len(slice_grid((cfg.frame_w, cfg.frame_h), (cfg.tile_w, cfg.tile_h), (cfg.overlap_w, cfg.overlap_h))[0]) + int(bool(cfg.overview))
    if images % per or xyxy.shape != (images, max_det, 4) or cls.shape != conf.shape or counts.shape != (images,):
        raise ValueError(f"{images} images of {per} per frame; shapes {xyxy.shape}, {conf.shape}, {cls.shape}, {counts.shape}")
    F, mo = images // per, cfg.max_out
    o_xy, o_cf = np.zeros((F, mo, 4), np.float32), np.zeros((F, mo), np.float32)
    o_cl, o_nm, o_n = np.zeros((F, mo), np.int32), np.zeros((F, mo), np.int32), np.zeros(F, np.int32)
    ms = C.c_float(0.0)
    _ffi.check(_ffi.lib().rtmodt_slice_merge(int(device), C.byref(cfg), int(max_det), F, _ffi.ptr(xyxy), _ffi.ptr(conf), _ffi.ptr(cls), _ffi.ptr(counts),
                                             _ffi.ptr(o_xy), _ffi.ptr(o_cf), _ffi.ptr(o_cl), _ffi.ptr(o_nm), _ffi.ptr(o_n), C.byref(ms)))
    out = [(o_xy[f, :o_n[f]].copy(), o_cf[f, :o_n[f]].copy(), o_cl[f, :o_n[f]].copy(), o_nm[f, :o_n[f]].copy()) for f in range(F)]
    return (out, ms.value) if want_ms else out


class SlicedDetector(_ffi.Handle):
    """``Detector`` for frames of one fixed ``frame_size = (width, height)``, run as overlapping tiles plus an overview.

    It owns a :class:`Detector` with ``batch = streams * I`` (``I`` images per frame) and ``input_size = tile``; every other
    keyword goes to that detector (``confidence``, ``iou``, ``max_det``, ``device``, ...).  ``detect`` / ``detect_batch`` /
    ``enqueue`` + ``fetch`` mirror the detector's; the detections they return are the merged ones in frame coordinates, and
    ``n_merged`` / ``last_tiles`` hold what the last fetch merged them from."""

    def __init__(self, model_path: str, *, frame_size, streams: int = 1, tile=(640, 640), overlap=(128, 128), overview: bool = True,
                 merge: str = "nmm", metric: str = "ios", match_threshold: float = 0.5, max_out: int = 300, **detector_kwargs) -> None:
        self.frame_size = (int(frame_size[0]), int(frame_size[1]))
        self.streams = int(streams)
        self.tile, self.overlap, self.overview = tuple(tile), tuple(overlap), bool(overview)
        self.merge, self.metric, self.match_threshold, self.max_out = merge, metric, float(match_threshold), int(max_out)
        self._tiles, self.tile_size = slice_grid(self.frame_size, tile, overlap)            # raises on a bad grid before anything is built
        self.images_per_frame = len(self._tiles) + int(self.overview)
        for k in ("batch", "input_size"):
            if k in detector_kwargs:
                raise TypeError(f"SlicedDetector sets the detector's {k} itself")
        self._ordinal = _ffi.device_ordinal(detector_kwargs.get("device", "cuda:0"))
        self._cfg = slice_cfg(self.frame_size, tile, overlap, overview, merge, metric, match_threshold, detector_kwargs.get("agnostic_nms", False),
                              max_out, self.streams, self._ordinal)
        self._h = None
        self.detector = Detector(model_path, input_size=tuple(tile), batch=self.streams * self.images_per_frame, **detector_kwargs)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_slicer_create(C.byref(self._cfg), int(self.detector.max_det), C.byref(h)))
        self._h = h
        S, mo, md, I = self.streams, self.max_out, self.detector.max_det, self.images_per_frame
        self._xyxy, self._conf = np.empty((S, mo, 4), np.float32), np.empty((S, mo), np.float32)
        self._cls, self._nm, self._n = np.empty((S, mo), np.int32), np.empty((S, mo), np.int32), np.zeros(S, np.int32)
        self._t_xyxy, self._t_conf = np.empty((S * I, md, 4), np.float32), np.empty((S * I, md), np.float32)
        self._t_cls, self._t_n = np.empty((S * I, md), np.int32), np.zeros(S * I, np.int32)
        self._in_flight, self._keepalive = [], []
        #: per frame of the last fetch: how many boxes each merged detection absorbed (NMM) or dropped (NMS)
        self.n_merged: list = []
        #: per frame of the last fetch: the I per-image ``Detections`` (tile coordinates) the merge started from
        self.last_tiles: list = []

    @property
    def model(self):
        return self.detector.model

    def grid(self):
        """``[(x, y), ...]`` tile origins in row-major order and the effective tile ``(te_w, te_h)``."""
        return list(self._tiles), self.tile_size

    # ------------------------------------------------------------------
    def detect(self, frame: np.ndarray) -> Detections:
        return self.detect_batch([frame])[0]

    def detect_batch(self, frames: Sequence[np.ndarray]) -> list:
        while self._in_flight:
            self.fetch()
        self.enqueue(frames)
        return self.fetch()

    def enqueue(self, frames: Sequence, pitch: int = 0) -> None:
        """Asynchronous half of :meth:`detect_batch`: up to ``streams`` frames of ``frame_size``, NumPy ``H x W x 3`` BGR arrays or raw
        device addresses (ints) of frames with row pitch ``pitch`` (0 = packed).  Two batches may be in flight."""
        arr, keep, n, p, kind = self._pointers(frames, pitch)
        _ffi.check(_ffi.lib().rtmodt_slicer_enqueue(self._h, self.detector.model.handle, arr, n, p, kind))
        self._in_flight.append(n)
        self._keepalive.append(keep)

    def _pointers(self, frames: Sequence, pitch: int):
        """``frames`` -> (pointer array, keep-alive list, count, row pitch, memory kind), checked against ``streams`` and ``frame_size``."""
        n = len(frames)
        if n < 1 or n > self.streams:
            raise ValueError(f"{n} frames for a sliced detector built with streams={self.streams}")
        w, h = self.frame_size
        if isinstance(frames[0], (int, np.integer)):
            return (C.c_void_p * n)(*[int(a) for a in frames]), [], n, int(pitch) or 3 * w, _ffi.MEM_DEVICE
        arr, keep, fh, fw, p = _ffi.frame_pointers(list(frames), _ffi.MEM_HOST)
        if (fw, fh) != (w, h):
            raise ValueError(f"frames are {fw}x{fh}, the sliced detector was built for {w}x{h}")
        return arr, keep, n, int(p), _ffi.MEM_HOST

    def fetch(self) -> list:
        """Merged ``Detections`` per frame of the OLDEST batch in flight."""
        if not self._in_flight:
            raise RuntimeError("fetch() without a pending enqueue()")
        n = self._in_flight[0]
        P = _ffi.ptr
        _ffi.check(_ffi.lib().rtmodt_slicer_fetch(self._h, self.detector.model.handle, P(self._xyxy), P(self._conf), P(self._cls), P(self._nm), P(self._n),
                                                  P(self._t_xyxy), P(self._t_conf), P(self._t_cls), P(self._t_n)))
        self._in_flight.pop(0)
        self._keepalive.pop(0)
        names = self.detector.model.names
        I = self.images_per_frame

        def parse(xy, cf, cl, k):
            if k == 0:
                return _empty()
            c = cl[:k].copy()
            return Detections(xy[:k].copy(), cf[:k].copy(), c, [names.get(int(v), str(v)) for v in c])

        self.n_merged = [self._nm[f, :self._n[f]].copy() for f in range(n)]
        self.last_tiles = [[parse(self._t_xyxy[i], self._t_conf[i], self._t_cls[i], int(self._t_n[i])) for i in range(f * I, (f + 1) * I)] for f in range(n)]
        return [parse(self._xyxy[f], self._conf[f], self._cls[f], int(self._n[f])) for f in range(n)]

    def gather(self, frames: Sequence, pitch: int = 0) -> np.ndarray:
        """The image batch ``[n * I, te_h, te_w, 3]`` the detector would be handed for ``frames`` (``rtmodt_slicer_gather``)."""
        arr, keep, n, p, kind = self._pointers(frames, pitch)
        out = np.empty((n * self.images_per_frame, self.tile_size[1], self.tile_size[0], 3), np.uint8)
        _ffi.check(_ffi.lib().rtmodt_slicer_gather(self._h, arr, n, p, kind, _ffi.ptr(out)))
        return out

    def last_ms(self):
        """Device ms (HIP events) of slice_gather of the last enqueue and of slice_merge of the last fetched batch."""
        return _ffi.last_ms("rtmodt_slicer_last_ms", self._h, 2)

    def synchronize(self) -> None:
        self.detector.synchronize()

    _destroy = "rtmodt_slicer_destroy"

    def close(self) -> None:
        super().close()                                      # before the detector: a merge may be queued on its stream
        if getattr(self, "detector", None) is not None:
            self.detector.close()
