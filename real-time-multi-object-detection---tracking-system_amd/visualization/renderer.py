"""Drop-in for the reference's ``src/visualization/renderer.py`` on MI355X.

``FrameRenderer`` has the reference's constructor and ``render(frame, tracks, zones, fps, latency_ms)``, which draws in place
and returns the frame it was given.  The drawing runs in ``csrc/render.hip`` (one launch per batch, paint rules in its
header comment); there is no CPU implementation here.  ``render_batch`` draws several frames in one call, host arrays or
frames already in device memory (a ``_ffi.DeviceBuffer``), which is the fast path: no frame crosses the host link.

Text is a bundled 1-bit bitmap font (``csrc/font_atlas.h``), not cv2's Hershey font, and the zone tint covers exactly the
pixels the zone engine counts as inside or on a polygon: parity with cv2 itself is unpinned (no OpenCV to run against).
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Optional, Sequence

import numpy as np

from .. import _ffi

log = logging.getLogger("rtmodt.visualization")

COORD_MAX = 1 << 20          # csrc/render.hip: every coordinate is clamped to +-2^20


def printable(text: str) -> str:
    """Characters outside ASCII 32..126 become ``?`` (the font has no other glyphs)."""
    return "".join(c if 32 <= ord(c) <= 126 else "?" for c in str(text))


def label_text(track) -> str:
    """The label above a box (renderer.py:78), as drawn."""
    return printable(f"ID:{track.track_id} {getattr(track, 'class_name', '')} {track.confidence:.2f}")


def hud_text(fps: float, latency_ms: float) -> str:
    """The HUD line (renderer.py:92); the library formats it the same way from the two numbers."""
    return f"FPS: {fps:.1f} | Latency: {latency_ms:.1f}ms"


class FrameRenderer(_ffi.Handle):
    """Draw detection + tracking annotations on frames (reference: renderer.py:28-96)."""

    def __init__(self, show_boxes: bool = True, show_ids: bool = True, show_trails: bool = True, trail_length: int = 30,
                 show_zones: bool = True, show_fps: bool = True, *, device=0, palette: Optional[Sequence] = None) -> None:
        self.show_boxes = show_boxes
        self.show_ids = show_ids
        self.show_trails = show_trails
        self.trail_length = trail_length
        self.show_zones = show_zones
        self.show_fps = show_fps
        self._device = _ffi.device_ordinal(device)
        self._palette = None if palette is None else np.ascontiguousarray(palette, np.uint8).reshape(-1, 3)
        self._h = None
        self._open()

    # ------------------------------------------------------------------ reference API
    def render(self, frame: np.ndarray, tracks: Sequence, zones: Optional[list] = None, fps: float = 0.0,
               latency_ms: float = 0.0) -> np.ndarray:
        """Annotate ``frame`` (H x W x 3 uint8 BGR, rows may be padded) in place; returns the same array."""
        self.render_batch([frame], [tracks], zones=zones, fps=fps, latency_ms=latency_ms)
        return frame

    # ------------------------------------------------------------------ batched
    def render_batch(self, frames, tracks_per_frame: Sequence[Sequence], zones: Optional[list] = None, fps: float = 0.0,
                     latency_ms: float = 0.0, *, height: Optional[int] = None, width: Optional[int] = None,
                     stride: Optional[int] = None, offset: int = 0):
        """Annotate ``len(tracks_per_frame)`` frames in one launch; returns ``frames``.

        ``frames``: a list of host arrays of one shape and row stride, or a ``_ffi.DeviceBuffer`` holding the frames one after
        another (frame i at ``offset + i * height * stride``; ``stride`` defaults to ``3 * width``), drawn where they are."""
        ptrs, h, w, st, mem, n = _ffi.batch_frames(frames, len(tracks_per_frame), height=height, width=width, stride=stride, offset=offset)
        if n == 0 and mem == _ffi.MEM_HOST:
            return frames
        if self._cfg_key() != self._key:                  # a show_* flag or trail_length changed since the handle was made
            self.close()
            self._open()
        draw_zones = self._sync_zones(zones)
        keep = []
        lists = (_ffi.RenderList * max(n, 1))()
        for i, tracks in enumerate(tracks_per_frame):
            arr = self._marshal(tracks, keep)
            keep.append(arr)
            lists[i] = _ffi.RenderList(C.cast(arr, C.POINTER(_ffi.RenderTrack)), len(tracks))
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        _ffi.check(_ffi.lib().rtmodt_render_batch(self._h, fp, n, h, w, st, mem, lists, draw_zones, float(fps), float(latency_ms)))
        return frames

    def last_kernel_ms(self) -> float:
        """Device time of the last batch's kernel (HIP events)."""
        return _ffi.last_ms("rtmodt_renderer_last_ms", self._h)

    def pack(self, tracks_per_frame: Sequence[Sequence], height: int, width: int, zones: bool = False, fps: float = 0.0,
             latency_ms: float = 0.0) -> bytes:
        """The command buffer ``render_batch`` would send for these lists (host only; frame pointers 0)."""
        return pack(self._cfg(), tracks_per_frame, height, width, zones, fps, latency_ms)

    _destroy = "rtmodt_renderer_destroy"

    # ------------------------------------------------------------------ internals
    def _open(self) -> None:
        cfg = self._cfg()
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_renderer_create(self._device, C.byref(cfg), C.byref(h)))
        self._h = h
        self._key = self._cfg_key()
        self._zone_key = None

    def _cfg_key(self) -> tuple:
        return (bool(self.show_boxes), bool(self.show_ids), bool(self.show_trails), bool(self.show_zones), bool(self.show_fps),
                int(self.trail_length))

    def _cfg(self) -> _ffi.RenderCfg:
        tl = int(self.trail_length)
        if not 1 <= tl <= 1024:
            raise ValueError(f"trail_length {tl} outside 1..1024")
        cfg = _ffi.RenderCfg(int(bool(self.show_boxes)), int(bool(self.show_ids)), int(bool(self.show_trails)), int(bool(self.show_zones)),
                             int(bool(self.show_fps)), tl, None, 0)
        if self._palette is not None:
            cfg.palette_bgr = self._palette.ctypes.data_as(C.POINTER(C.c_uint8))
            cfg.n_palette = len(self._palette)
        return cfg

    def _marshal(self, tracks: Sequence, keep: list):
        return marshal_tracks(tracks, self.trail_length, keep)

    def _sync_zones(self, zones) -> int:
        if not (self.show_zones and zones):
            return 0
        polys = [np.ascontiguousarray(np.asarray(p).reshape(-1, 2), np.int32) for _, p in zones]
        names = [printable(n).encode("ascii") for n, _ in zones]
        key = tuple((n, p.tobytes()) for n, p in zip(names, polys))
        if key != self._zone_key:
            k = len(polys)
            pp = (C.c_void_p * max(k, 1))(*[p.ctypes.data for p in polys])
            npts = np.array([len(p) for p in polys], np.int32)
            nm = (C.c_char_p * max(k, 1))(*names)
            _ffi.check(_ffi.lib().rtmodt_renderer_set_zones(self._h, pp, _ffi.ptr(npts), nm, k))
            self._zone_key = key
        return 1


def marshal_tracks(tracks: Sequence, trail_length: int, keep: list):
    """``Track``-likes (track_id / xyxy / confidence / class_name / trail) -> a ``rtmodt_render_track`` array; the arrays and
    strings it points into are appended to ``keep``."""
    arr = (_ffi.RenderTrack * max(len(tracks), 1))()
    # the library applies `len(trail) > 1` and takes the last trail_length points: hand it enough for both
    tail = max(int(trail_length), 2)
    for i, t in enumerate(tracks):
        xy = np.asarray(t.xyxy, np.float32).reshape(-1)[:4]
        r = arr[i]
        r.track_id = int(t.track_id)
        r.xyxy[:] = [float(v) for v in xy]
        lab = label_text(t).encode("ascii")
        keep.append(lab)
        r.label = lab
        trail = getattr(t, "trail", None)
        if trail is None:
            trail = []
        if len(trail):
            pts = np.clip(np.asarray(trail[-tail:], np.int64).reshape(-1, 2), -COORD_MAX, COORD_MAX).astype(np.int32)
            keep.append(pts)
            r.trail_xy = pts.ctypes.data_as(C.POINTER(C.c_int32))
            r.n_trail = len(pts)
    return arr


def pack(cfg: _ffi.RenderCfg, tracks_per_frame: Sequence[Sequence], height: int, width: int, zones: bool = False, fps: float = 0.0,
         latency_ms: float = 0.0) -> bytes:
    """``rtmodt_render_pack``: the command buffer for these draw lists, built on the host alone."""
    keep = []
    n = len(tracks_per_frame)
    lists = (_ffi.RenderList * max(n, 1))()
    for i, tracks in enumerate(tracks_per_frame):
        arr = marshal_tracks(tracks, cfg.trail_length, keep)
        keep.append(arr)
        lists[i] = _ffi.RenderList(C.cast(arr, C.POINTER(_ffi.RenderTrack)), len(tracks))
    need = C.c_size_t(0)
    L = _ffi.lib()
    _ffi.check(L.rtmodt_render_pack(C.byref(cfg), lists, n, int(height), int(width), int(bool(zones)), float(fps), float(latency_ms),
                                    None, 0, C.byref(need)))
    buf = np.zeros(need.value, np.uint8)
    _ffi.check(L.rtmodt_render_pack(C.byref(cfg), lists, n, int(height), int(width), int(bool(zones)), float(fps), float(latency_ms),
                                    _ffi.ptr(buf), buf.nbytes, C.byref(need)))
    return buf.tobytes()
