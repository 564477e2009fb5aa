"""Privacy masking on MI355X: tracked people / objects and fixed privacy zones are filled, pixelated or blurred in BGR24
frames before they are recorded, encoded or served.  The reference has nothing of the kind (its recordings and annotated
responses show every person in full).

``PrivacyMask`` masks host arrays or frames already in device memory (a ``_ffi.DeviceBuffer``, the fast path: no frame crosses
the host link) with boxes handed over (``apply`` / ``apply_batch``), with the device-resident tracks of any of the four trackers
(``apply_tracker``: exactly the tracks the crossing counter passes, no box crosses to the host) or with every detection of a
detector's last batch (``apply_detector``).  The work runs in ``csrc/privacy.hip`` (paint rules in its header comment, region
arithmetic in ``csrc/privacy_regions.h``); there is no CPU implementation here.  ``tests/privacy_ref.py`` restates the rules and
the kernels equal it byte for byte; parity with cv2's ``blur`` / ``GaussianBlur`` and with any camera's mask is unpinned.

The masker must be the LAST reader of the clean pixels: the detector, the appearance descriptors, Re-ID crops and the swap guard
all come earlier (``pipeline.run`` orders them so).  A caller that still needs the clean frame passes ``out=``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker

MODES = {"fill": 0, "pixelate": 1, "blur": 2}
REGIONS = {"box": 0, "head": 1}
MAX_REGIONS = 65536


def make_cfg(mode="pixelate", cell=16, radius=8, passes=2, region="box", head_fraction=0.3, expand_px=0, classes=None, color=(0, 0, 0),
             device=0, max_regions=MAX_REGIONS):
    """-> (``_ffi.PrivacyCfg``, the class array it points into or None)."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    if region not in REGIONS:
        raise ValueError(f"region {region!r}: one of {sorted(REGIONS)}")
    cfg = _ffi.PrivacyCfg()
    cfg.mode = MODES[mode]
    col = [int(v) for v in color]
    if len(col) != 3 or any(not 0 <= v <= 255 for v in col):
        raise ValueError(f"color {color!r}: three values 0..255 (B, G, R)")
    cfg.fill_bgr[:] = col + [0]
    cfg.cell, cfg.radius, cfg.passes = int(cell), int(radius), int(passes)
    cfg.region = REGIONS[region]
    cfg.head_pm = int(round(float(head_fraction) * 1000))
    cfg.expand_px = int(expand_px)
    cls = None
    if classes is not None:
        cls = np.ascontiguousarray(list(classes), np.int32).reshape(-1)
        keep = cls if len(cls) else np.zeros(1, np.int32)       # a non-null pointer for an empty list (nothing is masked)
        cfg.classes = keep.ctypes.data_as(C.POINTER(C.c_int32))
        cfg.n_classes = len(cls)
        cls = keep
    cfg.max_regions = int(max_regions)
    cfg.device = _ffi.device_ordinal(device)
    return cfg, cls


def regions(boxes, box_classes, height: int, width: int, **cfg_kw) -> np.ndarray:
    """``rtmodt_privacy_regions`` (host only): the inclusive rectangles ``(k, 4)`` int32 (x0, y0, x1, y1) the boxes (of classes ``box_classes``,
    or None) yield in a ``height x width`` frame under ``make_cfg(**cfg_kw)``."""
    cfg, keep = make_cfg(**cfg_kw)
    xy = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    cl = None if box_classes is None else np.ascontiguousarray(box_classes, np.int32).reshape(-1)
    if cl is not None and len(cl) != len(xy):
        raise ValueError(f"{len(xy)} boxes, {len(cl)} classes")
    need = C.c_int32(0)
    L = _ffi.lib()
    _ffi.check(L.rtmodt_privacy_regions(C.byref(cfg), _ffi.ptr(xy), _ffi.ptr(cl), len(xy), int(height), int(width), None, 0, C.byref(need)))
    out = np.zeros((max(need.value, 1), 4), np.int32)
    _ffi.check(L.rtmodt_privacy_regions(C.byref(cfg), _ffi.ptr(xy), _ffi.ptr(cl), len(xy), int(height), int(width), _ffi.ptr(out), need.value,
                                        C.byref(need)))
    return out[:need.value].copy()


def boxes_of(tracks):
    """``Track``-likes (``xyxy`` / ``class_id``), a ``Detections``-like (array ``xyxy`` / ``class_id``), an ``(n, 4)`` array or a
    ``(boxes, classes)`` pair -> (float32 ``(n, 4)``, int32 ``(n,)``)."""
    if isinstance(tracks, tuple) and len(tracks) == 2:
        xy = np.ascontiguousarray(tracks[0], np.float32).reshape(-1, 4)
        cl = np.zeros(len(xy), np.int32) if tracks[1] is None else np.ascontiguousarray(tracks[1], np.int32).reshape(-1)
    elif isinstance(tracks, np.ndarray):
        xy = np.ascontiguousarray(tracks, np.float32).reshape(-1, 4)
        cl = np.zeros(len(xy), np.int32)
    elif hasattr(tracks, "xyxy") and hasattr(tracks, "class_id") and np.ndim(tracks.xyxy) == 2:
        xy = np.ascontiguousarray(tracks.xyxy, np.float32).reshape(-1, 4)
        cl = np.ascontiguousarray(tracks.class_id, np.int32).reshape(-1)
    else:
        tracks = list(tracks)
        xy = np.zeros((len(tracks), 4), np.float32)
        cl = np.zeros(len(tracks), np.int32)
        for i, t in enumerate(tracks):
            xy[i] = np.asarray(t.xyxy, np.float32).reshape(-1)[:4]
            cl[i] = int(getattr(t, "class_id", 0))
    if len(cl) != len(xy):
        raise ValueError(f"{len(xy)} boxes, {len(cl)} classes")
    return xy, cl


class PrivacyMask(_ffi.Handle):
    """Masks boxes (whole, or their head rows), optionally of some classes only, and fixed privacy polygons.

    ``mode``: ``"fill"`` (``color``, BGR), ``"pixelate"`` (``cell`` 2..64) or ``"blur"`` (``passes`` 1..3 box filters of radius
    ``radius`` 1..16).  ``region``: ``"box"`` or ``"head"`` (the top ``head_fraction`` of the box, rounded up to whole rows, at
    least one).  ``expand_px`` 0..256 grows every region.  ``classes``: only boxes of these class ids (None: all).
    ``polygons``: int32 polygons masked in every frame (a camera's fixed privacy masks)."""

    def __init__(self, mode: str = "pixelate", cell: int = 16, radius: int = 8, passes: int = 2, region: str = "box",
                 head_fraction: float = 0.3, expand_px: int = 0, classes: Optional[Sequence[int]] = None, polygons=None,
                 color=(0, 0, 0), device=0, *, max_regions: int = MAX_REGIONS) -> None:
        self.mode = mode
        self._h = None
        self._cfg, self._keep = make_cfg(mode, cell, radius, passes, region, head_fraction, expand_px, classes, color, device, max_regions)
        self._device = self._cfg.device
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_privacy_create(C.byref(self._cfg), C.byref(h)))
        self._h = h
        self.set_polygons(polygons)

    # ------------------------------------------------------------------ configuration
    def set_polygons(self, polygons) -> None:
        """The fixed privacy zones: a list of ``(k, 2)`` integer polygons (None / empty clears them); uploaded once."""
        polys = [np.ascontiguousarray(np.asarray(p).reshape(-1, 2), np.int32) for p in (polygons or [])]
        k = len(polys)
        pp = (C.c_void_p * max(k, 1))(*[p.ctypes.data for p in polys])
        npts = np.array([len(p) for p in polys] or [0], np.int32)
        _ffi.check(_ffi.lib().rtmodt_privacy_set_polygons(self._h, pp, _ffi.ptr(npts), k))

    # ------------------------------------------------------------------ boxes handed over
    def apply(self, frame, tracks):
        """Masks ``frame`` (H x W x 3 uint8 BGR, rows may be padded) in place; returns it."""
        self.apply_batch([frame], [tracks])
        return frame

    def apply_batch(self, frames, tracks_per_frame: Sequence, out=None, *, height: Optional[int] = None, width: Optional[int] = None,
                    stride: Optional[int] = None, offset: int = 0, out_offset: int = 0):
        """Masks ``len(tracks_per_frame)`` frames in one call.  ``frames``: host arrays of one shape and row stride, or a
        ``_ffi.DeviceBuffer`` holding the frames one after another (frame i at ``offset + i * height * stride``).  ``out``
        (same kind, same geometry; a device buffer from ``out_offset``): receives the masked frames and ``frames`` stays
        clean; None: in place.  Returns ``out`` or ``frames``."""
        n = len(tracks_per_frame)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset, writable=out is None)
        dp = None
        if out is not None:
            optrs, oh, ow, ost, omem, _ = _ffi.batch_frames(out, n, height=height, width=width, stride=stride, offset=out_offset)
            if n and (oh, ow, ost, omem) != (h, w, st, mem):
                raise ValueError("out must have the frames' kind, shape and row stride")
            dp = (C.c_void_p * max(n, 1))(*optrs)
        if n == 0:
            return frames if out is None else out
        keep = [boxes_of(t) for t in tracks_per_frame]
        xp = (C.c_void_p * n)(*[xy.ctypes.data for xy, _ in keep])
        cp = (C.c_void_p * n)(*[cl.ctypes.data for _, cl in keep])
        nb = np.asarray([len(xy) for xy, _ in keep], np.int32)
        fp = (C.c_void_p * n)(*ptrs)
        _ffi.check(_ffi.lib().rtmodt_privacy_apply(self._h, fp, dp, n, h, w, st, mem, xp, cp, _ffi.ptr(nb)))
        return frames if out is None else out

    # ------------------------------------------------------------------ device-resident sources
    def apply_tracker(self, tracker, frames, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                      offset: int = 0):
        """Masks ``frames`` (one per stream of ``tracker``) in place with the tracker's device-resident tracks: those the
        crossing counter's ``process_tracker`` passes.  Dispatches on the tracker class; returns ``frames``."""
        core, suffix, tsu = resolve_tracker(tracker, "apply_tracker", "as a list: apply(frame, tracks)")
        n = core.n_streams
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset)
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        _ffi.check(getattr(_ffi.lib(), f"rtmodt_privacy_apply_{suffix}")(self._h, core._h, fp, h, w, st, mem, *tsu))
        return frames

    def apply_detector(self, detector, frames, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                       offset: int = 0, count: Optional[int] = None):
        """Masks the first ``len(frames)`` (``count`` for a device buffer) frames of ``detector``'s newest batch in place with every
        detection of that batch, read from its device-resident outputs; returns ``frames``."""
        n = int(count) if count is not None else (1 if isinstance(frames, _ffi.DeviceBuffer) else len(frames))
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset)
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        _ffi.check(_ffi.lib().rtmodt_privacy_apply_detector(self._h, detector.model.handle, fp, n, h, w, st, mem))
        return frames

    def last_kernel_ms(self) -> float:
        """Device time of the last call's launches (HIP events)."""
        return _ffi.last_ms("rtmodt_privacy_last_ms", self._h)

    _destroy = "rtmodt_privacy_destroy"
