"""Occupancy heatmaps on MI355X: where objects have been.  One ``uint32`` grid per stream accumulates the footprints of boxes or
of device-resident tracks frame after frame, is blended onto BGR24 frames in place and is summed per polygon ("how many
object-frames did this zone see").  The reference accumulates nothing over time (its heat-map plot is the confusion matrix).

``Heatmap`` takes boxes handed over (``accumulate``), the device-resident tracks of any of the four trackers
(``accumulate_tracker``: exactly the tracks ``PrivacyMask.apply_tracker`` masks, no box crosses to the host) or every detection of
a detector's newest batch (``accumulate_detector``); ``overlay`` blends onto host arrays or onto frames already in device memory
(a ``_ffi.DeviceBuffer``).  The work runs in ``csrc/heatmap.hip`` (rules in its header comment, the footprint rule in
``csrc/heatmap_stamp.h``); there is no CPU implementation here.  ``tests/heatmap_ref.py`` restates every rule and the kernels
equal it exactly.  Unpinned: parity with Ultralytics' ``Heatmap`` solution, with cv2's colormaps (the default table is a
closed-form jet whose parity with ``cv2.COLORMAP_JET`` is unpinned) and ``addWeighted``, and any default tuned on real footage.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker
from .privacy import boxes_of

FOOTPRINTS = {"box": 0, "disc": 1, "foot": 2}


def make_cfg(n_streams=1, height=0, width=0, cell=4, footprint="disc", foot_radius=0, weight=1, decay_shift=0, decay_every=1, classes=None,
             device=0):
    """-> (``_ffi.HeatmapCfg``, the class array it points into or None)."""
    if footprint not in FOOTPRINTS:
        raise ValueError(f"footprint {footprint!r}: one of {sorted(FOOTPRINTS)}")
    cfg = _ffi.HeatmapCfg()
    cfg.n_streams, cfg.height, cfg.width, cfg.cell = int(n_streams), int(height), int(width), int(cell)
    cfg.footprint = FOOTPRINTS[footprint]
    cfg.foot_radius, cfg.weight, cfg.decay_shift, cfg.decay_every = int(foot_radius), int(weight), int(decay_shift), int(decay_every)
    cls = None
    if classes is not None:
        cls = np.ascontiguousarray(list(classes), np.int32).reshape(-1)
        keep = cls if len(cls) else np.zeros(1, np.int32)       # a non-null pointer for an empty list (nothing is stamped)
        cfg.classes = keep.ctypes.data_as(C.POINTER(C.c_int32))
        cfg.n_classes = len(cls)
        cls = keep
    cfg.device = _ffi.device_ordinal(device)
    return cfg, cls


def footprint_cells(box, cls, height: int, width: int, **cfg_kw) -> np.ndarray:
    """``rtmodt_heatmap_footprint`` (host only): the cells ``(k, 2)`` int32 (cx, cy), row by row, that one box of class ``cls`` stamps
    on the grid of a ``height x width`` frame under ``make_cfg(**cfg_kw)``."""
    cfg, keep = make_cfg(height=height, width=width, **cfg_kw)
    xy = np.ascontiguousarray(box, np.float32).reshape(4)
    need = C.c_int32(0)
    L = _ffi.lib()
    _ffi.check(L.rtmodt_heatmap_footprint(C.byref(cfg), _ffi.ptr(xy), int(cls), None, 0, C.byref(need)))
    out = np.zeros((max(need.value, 1), 2), np.int32)
    _ffi.check(L.rtmodt_heatmap_footprint(C.byref(cfg), _ffi.ptr(xy), int(cls), _ffi.ptr(out), need.value, C.byref(need)))
    return out[:need.value].copy()


class Heatmap(_ffi.Handle):
    """One grid of ``ceil(height / cell) x ceil(width / cell)`` ``uint32`` cells per stream.

    ``cell``: 1, 2, 4, 8 or 16 pixels.  ``footprint``: ``"box"`` (every cell the box touches), ``"disc"`` (the cells within
    ``min(W, H) / 2`` of the box centre: Ultralytics' circular stamp; parity unpinned) or ``"foot"`` (the cells within
    ``foot_radius`` 0..256 pixels of the bottom-centre pixel, for traffic maps).  Each ``accumulate*`` call is one frame of every
    stream: a covered cell gains ``weight`` (1..1024) per footprint, saturating at ``2^32 - 1``; with ``decay_shift`` 1..16 every
    cell first loses ``heat >> decay_shift`` in every ``decay_every``-th call.  ``classes``: only boxes of these class ids.

    ``alpha`` (0..256), ``min_level`` (1..255) and ``scale_max`` (0: the grid's maximum at the time of the call) are ``overlay``'s
    defaults; ``overlay_enabled`` tells ``pipeline.run`` whether its heatmap stage blends the heat onto the frame."""

    def __init__(self, n_streams: int, height: int, width: int, cell: int = 4, footprint: str = "disc", foot_radius: int = 0, weight: int = 1,
                 decay_shift: int = 0, decay_every: int = 1, classes: Optional[Sequence[int]] = None, alpha: int = 128, min_level: int = 1,
                 scale_max: int = 0, colormap=None, overlay_enabled: bool = True, device=0) -> None:
        self._h = None
        self._cfg, self._keep = make_cfg(n_streams, height, width, cell, footprint, foot_radius, weight, decay_shift, decay_every, classes, device)
        self.n_streams, self.height, self.width, self.cell = int(n_streams), int(height), int(width), int(cell)
        self.alpha, self.min_level, self.scale_max, self.overlay_enabled = int(alpha), int(min_level), int(scale_max), bool(overlay_enabled)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_heatmap_create(C.byref(self._cfg), C.byref(h)))
        self._h = h
        self.grid_shape = (-(-self.height // self.cell), -(-self.width // self.cell))
        if colormap is not None:
            self.set_colormap(colormap)

    # ------------------------------------------------------------------ accumulate
    def accumulate(self, boxes_per_stream: Sequence) -> None:
        """One frame of every stream: ``boxes_per_stream[s]`` is what ``PrivacyMask.apply`` takes as tracks (``Track``-likes, a
        ``Detections``-like, an ``(n, 4)`` array or a ``(boxes, classes)`` pair)."""
        if len(boxes_per_stream) != self.n_streams:
            raise ValueError(f"{len(boxes_per_stream)} box lists, {self.n_streams} streams")
        n = self.n_streams
        keep = [boxes_of(t) for t in boxes_per_stream]
        xp = (C.c_void_p * n)(*[xy.ctypes.data for xy, _ in keep])
        cp = (C.c_void_p * n)(*[cl.ctypes.data for _, cl in keep])
        nb = np.asarray([len(xy) for xy, _ in keep], np.int32)
        _ffi.check(_ffi.lib().rtmodt_heatmap_accumulate(self._h, xp, cp, _ffi.ptr(nb)))

    def accumulate_tracker(self, tracker) -> None:
        """One frame of every stream from the tracker's device-resident tracks: those ``PrivacyMask.apply_tracker`` masks.
        Dispatches on the tracker class; the tracker must have as many streams as the heatmap."""
        core, suffix, tsu = resolve_tracker(tracker, "accumulate_tracker", "as lists: accumulate([tracks])")
        _ffi.check(getattr(_ffi.lib(), f"rtmodt_heatmap_accumulate_{suffix}")(self._h, core._h, *tsu))

    def accumulate_detector(self, detector) -> None:
        """One frame of every stream from every detection of ``detector``'s newest batch (frame i -> stream i), read from its
        device-resident outputs; the batch must hold as many frames as the heatmap has streams."""
        _ffi.check(_ffi.lib().rtmodt_heatmap_accumulate_detector(self._h, detector.model.handle))

    # ------------------------------------------------------------------ overlay
    def set_colormap(self, table) -> None:
        """``table``: 256 x 3 uint8, B G R per level; None restores the default, the closed-form jet of ``csrc/heatmap.hip`` (parity
        with ``cv2.COLORMAP_JET`` unpinned)."""
        if table is None:
            _ffi.check(_ffi.lib().rtmodt_heatmap_set_colormap(self._h, None))
            return
        t = np.ascontiguousarray(table)
        if t.shape != (256, 3) or t.dtype != np.uint8:
            raise ValueError("a colour table is a (256, 3) uint8 array, B G R")
        _ffi.check(_ffi.lib().rtmodt_heatmap_set_colormap(self._h, _ffi.ptr(t)))

    def overlay(self, frames, streams: Optional[Sequence[int]] = None, *, alpha: Optional[int] = None, min_level: Optional[int] = None,
                scale_max: Optional[int] = None, stride: Optional[int] = None, offset: int = 0):
        """Blends the heat onto ``frames`` in place and returns them: host arrays (H x W x 3 uint8, rows may be padded) or a
        ``_ffi.DeviceBuffer`` holding the frames one after another from ``offset``, rows ``stride`` bytes apart.  Frame i shows
        the grid of ``streams[i]``; None: one frame per stream, in order."""
        n = self.n_streams if streams is None else len(streams)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=self.height, width=self.width, stride=stride, offset=offset)
        if n == 0:
            return frames
        fp = (C.c_void_p * n)(*ptrs)
        sp = None if streams is None else np.ascontiguousarray(list(streams), np.int32)
        _ffi.check(_ffi.lib().rtmodt_heatmap_overlay(self._h, fp, _ffi.ptr(sp), n, h, w, st, mem, self.alpha if alpha is None else int(alpha),
                                                     self.min_level if min_level is None else int(min_level),
                                                     self.scale_max if scale_max is None else int(scale_max)))
        return frames

    # ------------------------------------------------------------------ totals and housekeeping
    def zone_sums(self, polygons, stream: int = 0) -> np.ndarray:
        """``uint64`` per polygon (``(k, 2)`` integer arrays): the heat of the cells whose centre pixel lies inside or on it."""
        polys = [np.ascontiguousarray(np.asarray(p).reshape(-1, 2), np.int32) for p in polygons]
        k = len(polys)
        pp = (C.c_void_p * max(k, 1))(*[p.ctypes.data for p in polys])
        npts = np.array([len(p) for p in polys] or [0], np.int32)
        out = np.zeros(max(k, 1), np.uint64)
        _ffi.check(_ffi.lib().rtmodt_heatmap_zone_sums(self._h, int(stream), pp, _ffi.ptr(npts), k, _ffi.ptr(out)))
        return out[:k]

    def grid(self, stream: int = 0) -> np.ndarray:
        """A copy of one stream's grid, ``uint32 (gh, gw)``."""
        out = np.zeros(self.grid_shape, np.uint32)
        _ffi.check(_ffi.lib().rtmodt_heatmap_read(self._h, int(stream), _ffi.ptr(out)))
        return out

    def load(self, grid, stream: int = 0) -> None:
        """Replaces one stream's grid with a saved one (``grid()``'s shape), so that a map survives a restart."""
        g = np.ascontiguousarray(grid, np.uint32)
        if g.shape != self.grid_shape:
            raise ValueError(f"a grid of {g.shape}, this heatmap's is {self.grid_shape}")
        _ffi.check(_ffi.lib().rtmodt_heatmap_load(self._h, int(stream), _ffi.ptr(g)))

    def reset(self, stream: Optional[int] = None) -> None:
        """Zeroes one stream's grid, or (None) every grid."""
        _ffi.check(_ffi.lib().rtmodt_heatmap_reset(self._h, -1 if stream is None else int(stream)))

    def last_kernel_ms(self) -> float:
        """Device time of the last accumulate or overlay call's launches (HIP events)."""
        return _ffi.last_ms("rtmodt_heatmap_last_ms", self._h)

    _destroy = "rtmodt_heatmap_destroy"
