"""Lens correction on MI355X: frames are undistorted once, directly after decode, so that every later stage -- detector, motion,
trackers, zones, crossings, the ground-plane speed estimator, privacy polygons, heatmap, renderer, JPEG -- runs in the rectified
pixel coordinates it assumes.  The reference has no such step (``src/ingestion/rtsp_reader.py`` hands ``cap.read()``'s frame
straight to the detector; ``cv2.undistort`` appears nowhere in it).

The lens is OpenCV's pinhole + Brown-Conrady / rational model without a rectification rotation; a table per lens is built on the host
when the lens is set and frames are sampled through it in ``csrc/lens.hip`` (rules: ``csrc/lens_model.h``); there is no CPU
implementation here.  ``tests/lens_ref.py`` restates every rule and the table and the output bytes equal it exactly.  Any other lens
(fisheye) enters as a caller's map, the form ``cv2.remap`` takes.  Unpinned: parity with ``cv2.undistort`` /
``initUndistortRectifyMap`` / ``remap`` (cv2's table rounds differently and is not installed where this is tested), the
``fisheye_map`` helper, and any calibration on real footage.

Sizes are ``(height, width)`` throughout; integer pixel coordinates are pixel centres; points are ``(x, y)`` pairs.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from .. import _ffi


def _intrinsics(K) -> Tuple[float, float, float, float]:
    """A 3 x 3 camera matrix (OpenCV's) or ``(fx, fy, cx, cy)`` -> ``(fx, fy, cx, cy)``."""
    K = np.asarray(K, np.float64)
    if K.shape == (3, 3):
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if K.shape == (4,):
        return tuple(float(v) for v in K)
    raise ValueError(f"intrinsics are a 3 x 3 camera matrix or (fx, fy, cx, cy), got shape {K.shape}")


def _coefficients(dist) -> np.ndarray:
    """``dist`` in OpenCV's order (k1 k2 p1 p2 [k3 [k4 k5 k6]]), 4, 5 or 8 long -> all 8."""
    d = np.asarray(dist, np.float64).reshape(-1)
    if d.size not in (4, 5, 8):
        raise ValueError(f"{d.size} distortion coefficients; OpenCV's order k1 k2 p1 p2 [k3 [k4 k5 k6]], 4, 5 or 8 long")
    return np.concatenate([d, np.zeros(8 - d.size)])


def make_params(K, dist, new_K=None, r2_limit: float = 0.0) -> "_ffi.LensParams":
    """``struct rtmodt_lens_params`` of a lens; ``new_K`` None: the output intrinsics are the source's."""
    p = _ffi.LensParams()
    p.fx, p.fy, p.cx, p.cy = _intrinsics(K)
    p.k = (C.c_double * 8)(*_coefficients(dist))
    if new_K is not None:
        p.nfx, p.nfy, p.ncx, p.ncy = _intrinsics(new_K)
    p.r2_limit = float(r2_limit)
    return p


def _points(params, xy, fn, want_residual: bool):
    xy = np.ascontiguousarray(xy, np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"points are an (n, 2) array of (x, y), got shape {xy.shape}")
    out = np.zeros_like(xy)
    res = np.zeros(len(xy), np.float64) if want_residual else None
    _ffi.check(fn(C.byref(params), _ffi.ptr(xy), len(xy), _ffi.ptr(out), _ffi.ptr(res)))
    return (out, res) if want_residual else out


def distort_points(xy, K, dist, new_K=None) -> np.ndarray:
    """Points of the RECTIFIED picture -> the original picture (host only, float64, closed form): a rectified box is drawn back on
    an original frame."""
    return _points(make_params(K, dist, new_K), xy, _ffi.lib().rtmodt_lens_distort_points, False)


def undistort_points(xy, K, dist, new_K=None):
    """Points of the ORIGINAL picture -> ``(rectified points, residuals)`` (host only, float64): zones, tripwires, privacy polygons
    and the surveyed points of ``fit_plane`` are drawn on the original picture and carried over once.  20 fixed iterations of
    OpenCV's scheme; ``residuals[i]`` is ``|distort(undistort(p)) - p|`` (largest axis) in pixels -- a lens on which the iteration
    does not converge there shows as a large number (``inf`` when not a number), not as a silently wrong point."""
    return _points(make_params(K, dist, new_K), xy, _ffi.lib().rtmodt_lens_undistort_points, True)


def build_map(K, dist, src_size, out_size=None, new_K=None, r2_limit: float = 0.0):
    """The canonical table of a lens without a GPU -> ``(qx, qy, outside)`` (``rtmodt_lens_build_map``), as ``LensCorrector.map``."""
    (sh, sw), (oh, ow) = src_size, out_size or src_size
    p = make_params(K, dist, new_K, r2_limit)
    qx, qy, outside = np.zeros((oh, ow), np.int32), np.zeros((oh, ow), np.int32), np.zeros((oh, ow), np.uint8)
    _ffi.check(_ffi.lib().rtmodt_lens_build_map(C.byref(p), int(sh), int(sw), int(oh), int(ow), _ffi.ptr(qx), _ffi.ptr(qy), _ffi.ptr(outside)))
    return qx, qy, outside


def quantise_map(map_x, map_y, src_size):
    """The canonical table of a caller's map without a GPU -> ``(qx, qy, outside)`` (``rtmodt_lens_quantise_map``)."""
    map_x, map_y = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
    if map_x.ndim != 2 or map_x.shape != map_y.shape:
        raise ValueError(f"map_x and map_y are float32 (out_h, out_w) arrays of one shape, got {map_x.shape} and {map_y.shape}")
    oh, ow = map_x.shape
    qx, qy, outside = np.zeros((oh, ow), np.int32), np.zeros((oh, ow), np.int32), np.zeros((oh, ow), np.uint8)
    _ffi.check(_ffi.lib().rtmodt_lens_quantise_map(_ffi.ptr(map_x), _ffi.ptr(map_y), int(src_size[0]), int(src_size[1]), oh, ow, _ffi.ptr(qx),
                                                   _ffi.ptr(qy), _ffi.ptr(outside)))
    return qx, qy, outside


# ---- NumPy-only helpers: their output enters through set_map / set_model, no parity is claimed for them -------------------------
def fisheye_map(K, D4, new_K, out_size):
    """The equidistant Kannala-Brandt (OpenCV ``fisheye``) map, float32 ``(map_x, map_y)`` of ``out_size`` for
    ``LensCorrector.set_map``: theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), the source
    position is ``K`` applied to the normalised point scaled by theta_d / r.  ``np.arctan`` is not pinned to anything."""
    fx, fy, cx, cy = _intrinsics(K)
    nfx, nfy, ncx, ncy = _intrinsics(K if new_K is None else new_K)
    k = np.asarray(D4, np.float64).reshape(-1)
    if k.size != 4:
        raise ValueError(f"{k.size} fisheye coefficients, 4 expected")
    oh, ow = int(out_size[0]), int(out_size[1])
    v, u = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    x, y = (u - ncx) / nfx, (v - ncy) / nfy
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    t2 = th * th
    th_d = th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    scale = np.divide(th_d, r, out=np.ones_like(r), where=r > 0)
    return (fx * (x * scale) + cx).astype(np.float32), (fy * (y * scale) + cy).astype(np.float32)


def monotonic_r2(dist, r2_max: float = 16.0, step: float = 1e-3) -> float:
    """The first normalised r^2 (scanned in steps of ``step`` up to ``r2_max``) at which ``r * rad(r)`` stops growing -- beyond it a
    strongly negative k1 folds the picture back onto itself -- for ``set_model(r2_limit=...)``.  0.0 (no limit) when it grows
    throughout.  The tangential terms are not looked at."""
    k1, k2, _, _, k3, k4, k5, k6 = _coefficients(dist)
    r2 = step * np.arange(0, int(np.floor(r2_max / step)) + 1, dtype=np.float64)
    num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sqrt(r2) * (num / den)
    bad = ~(den[1:] > 0) | ~(f[1:] > f[:-1])
    hit = np.flatnonzero(bad)
    return float(r2[hit[0]]) if hit.size else 0.0


class LensCorrector(_ffi.Handle):
    """``streams`` lenses for BGR24 frames of ``src_size`` -> rectified frames of ``out_size`` (default: the same size).

    A pixel that no source pixel reaches, and every tap off the source, reads ``border`` (b, g, r).  A stream has no lens until
    ``set_model`` or ``set_map`` gave it one; the table is built on the host then, once, not per frame."""

    def __init__(self, streams: int, src_size, out_size=None, border=(0, 0, 0), device=0) -> None:
        self._h = None
        c = _ffi.LensCfg()
        _ffi.lib().rtmodt_lens_default_cfg(C.byref(c))
        self.streams = int(streams)
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.out_size = self.src_size if out_size is None else (int(out_size[0]), int(out_size[1]))
        c.device, c.streams = _ffi.device_ordinal(device), self.streams
        c.src_h, c.src_w = self.src_size
        c.out_h, c.out_w = self.out_size
        c.border_bgr = (C.c_uint8 * 3)(*[int(v) for v in border])
        self._device = c.device
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_lens_create(C.byref(c), C.byref(h)))
        self._h = h

    def set_model(self, stream: int, K, dist, new_K=None, r2_limit: float = 0.0) -> int:
        """Gives ``stream`` the lens ``K`` (3 x 3 or (fx, fy, cx, cy)), ``dist`` (OpenCV's order, 4, 5 or 8 long); ``new_K``: the
        intrinsics of the rectified picture (None: ``K``; a shorter focal length zooms out).  Returns the number of output pixels
        that are border."""
        p = make_params(K, dist, new_K, r2_limit)
        n_out = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_lens_set_model(self._h, int(stream), C.byref(p), C.byref(n_out)))
        return n_out.value

    def set_map(self, stream: int, map_x, map_y) -> int:
        """Gives ``stream`` a caller's map: float32 ``(out_h, out_w)`` source positions, the form ``cv2.remap`` takes.  A NaN, an
        infinity or a position at or beyond +-2^20 is border.  Returns the number of output pixels that are border."""
        map_x, map_y = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        if map_x.shape != self.out_size or map_y.shape != self.out_size:
            raise ValueError(f"maps of {map_x.shape} / {map_y.shape}, this corrector's output is {self.out_size}")
        n_out = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_lens_set_map(self._h, int(stream), _ffi.ptr(map_x), _ffi.ptr(map_y), C.byref(n_out)))
        return n_out.value

    def map(self, stream: int = 0):
        """-> ``(qx, qy, outside)`` as the device holds them: int32 ``(out_h, out_w)`` source positions with 5 fractional bits (0
        where outside) and uint8 0 / 1."""
        qx, qy, outside = np.zeros(self.out_size, np.int32), np.zeros(self.out_size, np.int32), np.zeros(self.out_size, np.uint8)
        _ffi.check(_ffi.lib().rtmodt_lens_read_map(self._h, int(stream), _ffi.ptr(qx), _ffi.ptr(qy), _ffi.ptr(outside)))
        return qx, qy, outside

    def process(self, frames, streams: Optional[Sequence[int]] = None, out=None, *, stride: Optional[int] = None, offset: int = 0,
                out_stride: Optional[int] = None, out_offset: int = 0):
        """Rectifies frame i through the lens of ``streams[i]`` (None: stream i), all in one launch.  ``frames``: host arrays
        (``src_size`` x 3 uint8, rows may be padded) or a ``_ffi.DeviceBuffer`` holding them one after another from ``offset``, rows
        ``stride`` bytes apart.  ``out``: None -- new host arrays; a list of host arrays (``out_size`` x 3 uint8, rows may be padded:
        the padding is not touched); or a ``_ffi.DeviceBuffer``, frame i at ``out_offset + i * out_h * out_stride``.  Returns the host
        arrays, or the given ``DeviceBuffer`` -- frames the detector, ``MotionDetector``, ``FrameRenderer`` and ``JpegEncoder`` take
        as they are.  Source and destination may not overlap."""
        n = len(streams) if streams is not None else (self.streams if isinstance(frames, _ffi.DeviceBuffer) else len(frames))
        sptr, h, w, sst, smem, _ = _ffi.batch_frames(frames, n, height=self.src_size[0], width=self.src_size[1], stride=stride, offset=offset, writable=False)
        if n and (h, w) != self.src_size:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"frames of {w}x{h}, the lens corrector was created for {self.src_size[1]}x{self.src_size[0]}")
        if out is None:
            out = [np.zeros(self.out_size + (3,), np.uint8) for _ in range(n)]
        ret = out
        if not isinstance(out, _ffi.DeviceBuffer):
            out = list(out)
        dptr, oh, ow, dst, dmem, _ = _ffi.batch_frames(out, n, height=self.out_size[0], width=self.out_size[1], stride=out_stride, offset=out_offset, writable=True)
        if n and (oh, ow) != self.out_size:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"output frames of {ow}x{oh}, the lens corrector was created for {self.out_size[1]}x{self.out_size[0]}")
        if n == 0:
            return ret
        sp = None if streams is None else np.ascontiguousarray(list(streams), np.int32)
        _ffi.check(_ffi.lib().rtmodt_lens_process(self._h, (C.c_void_p * n)(*sptr), sst, smem, (C.c_void_p * n)(*dptr), dst, dmem, _ffi.ptr(sp), n))
        return ret

    def last_ms(self) -> float:
        """Device time of the last ``process`` call's launch (HIP events)."""
        return _ffi.last_ms("rtmodt_lens_last_ms", self._h)

    distort_points = staticmethod(distort_points)
    undistort_points = staticmethod(undistort_points)

    _destroy = "rtmodt_lens_destroy"
