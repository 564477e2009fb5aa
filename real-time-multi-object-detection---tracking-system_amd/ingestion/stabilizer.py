"""Stabilisation on MI355X: frames of a camera that shakes on its pole, gantry or bridge are steadied once, directly after decode (and
``undistort``), so that every fixed-camera stage -- ``MotionDetector``, ``LeftObjectDetector``, ``SpeedEstimator``, ``Heatmap``, zones,
tripwires, privacy polygons -- sees a steady picture.  The reference has no such step (``src/ingestion/rtsp_reader.py`` hands
``cap.read()``'s frame to the detector; ``cv2.estimateAffinePartial2D`` / ``warpAffine`` appear nowhere in it).

Per stream a camera path lives on the device; each call moves it by one similarity -- the caller's, or the one a
``tracking.CameraMotionEstimator`` estimates from the same frames, with nothing crossing the host between the estimate and the
pixels -- and resamples the frame (``csrc/stab.hip``; rules: ``csrc/stab_rule.h``); there is no CPU implementation here.
``tests/stab_ref.py`` restates every rule and paths (bit patterns), statuses, coefficients and output bytes equal it exactly.
Unpinned: parity with vidstab, OpenCV's ``videostab`` and ``warpAffine`` (installed nowhere this runs), and every default on real
footage.  Deliberate limits: one similarity per frame (no rolling-shutter or perspective model); causal, no look-ahead; a BoT-SORT
``gmc`` behind the stabiliser sees only the residual motion.

Sizes are ``(height, width)`` throughout; integer pixel coordinates are pixel centres; points are ``(x, y)`` pairs.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

from .. import _ffi

OK, HOLD, CLAMPED, RESET = 0, 1, 2, 3
STATUS_NAMES = {OK: "followed", HOLD: "input invalid, held", CLAMPED: "clamped to a limit", RESET: "reset to the identity"}


class StabResult(NamedTuple):
    status: int
    hold: int
    path: tuple          # (za, zb, tx, ty), float64
    coef: tuple          # (A, B, U, V), Q16 integers


def make_cfg(size, *, streams: int = 1, leak_shift: Optional[int] = None, max_shift_px: Optional[int] = None, max_rot_milli: Optional[int] = None,
             max_zoom_milli: Optional[int] = None, crop_zoom_milli: Optional[int] = None, reset_after: Optional[int] = None, border=(0, 0, 0),
             device=0) -> "_ffi.StabCfg":
    """``struct rtmodt_stab_cfg`` with the library's defaults where an argument is None."""
    c = _ffi.StabCfg()
    _ffi.lib().rtmodt_stab_default_cfg(C.byref(c))
    c.device, c.streams = _ffi.device_ordinal(device), int(streams)
    c.h, c.w = int(size[0]), int(size[1])
    for name, v in (("leak_shift", leak_shift), ("max_shift_px", max_shift_px), ("max_rot_milli", max_rot_milli), ("max_zoom_milli", max_zoom_milli),
                    ("crop_zoom_milli", crop_zoom_milli), ("reset_after", reset_after)):
        if v is not None:
            setattr(c, name, int(v))
    c.border_bgr = (C.c_uint8 * 3)(*[int(v) for v in border])
    return c


def rule_step(cfg, path, hold: int, warp=None, valid: bool = True):
    """``csrc/stab_rule.h`` on one stream's state without a GPU (``rtmodt_stab_step``) -> ``(path, hold, status, coef)``."""
    j = np.ascontiguousarray(path, np.float64).copy()
    w = None if warp is None else np.ascontiguousarray(warp, np.float32).reshape(6)
    h, st, coef = C.c_int32(int(hold)), C.c_int32(0), np.zeros(4, np.int64)
    _ffi.check(_ffi.lib().rtmodt_stab_step(C.byref(cfg), _ffi.ptr(j), C.byref(h), _ffi.ptr(w), int(bool(valid)), C.byref(st), _ffi.ptr(coef)))
    return j, h.value, st.value, coef


def map_points(cfg, path, xy, to_source: bool) -> np.ndarray:
    """Points through a path without a GPU (``rtmodt_stab_points``), float64."""
    xy = np.ascontiguousarray(xy, np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"points are an (n, 2) array of (x, y), got shape {xy.shape}")
    j = np.ascontiguousarray(path, np.float64).reshape(4)
    out = np.zeros_like(xy)
    _ffi.check(_ffi.lib().rtmodt_stab_points(C.byref(cfg), _ffi.ptr(j), int(bool(to_source)), _ffi.ptr(xy), len(xy), _ffi.ptr(out)))
    return out


class Stabilizer(_ffi.Handle):
    """``streams`` camera paths for BGR24 frames of ``size``; ``process`` returns the stabilised frames of the same size.

    ``leak_shift``: the path decays by ``1 - 2^-leak_shift`` per call, so that slow real drift of the mount (and the drift that
    compounded estimates accumulate) is followed while jitter is taken out; 0 anchors on the stream's first frame.  ``max_shift_px``,
    ``max_rot_milli``, ``max_zoom_milli``: per-component limits of the correction.  ``crop_zoom_milli`` (>= 1000): a fixed enlargement
    about the centre that hides the correction band; 1000 shows ``border`` (b, g, r) where nothing maps.  ``reset_after``: consecutive
    calls without a valid input after which the path is the identity again (a camera that was moved, covered or switched; 0: never).
    ``gmc``: a ``tracking.CameraMotionEstimator`` (of at least as many streams) that estimates the warps from the frames themselves,
    or True: one is made with its defaults.  Every default here is validated on no real footage."""

    def __init__(self, streams: int, size, *, leak_shift: int = 6, max_shift_px: int = 32, max_rot_milli: int = 35, max_zoom_milli: int = 50,
                 crop_zoom_milli: int = 1000, reset_after: int = 30, border=(0, 0, 0), gmc=None, device=0) -> None:
        self._h = None
        self._own_gmc = False
        self.streams, self.size = int(streams), (int(size[0]), int(size[1]))
        self.cfg = make_cfg(self.size, streams=self.streams, leak_shift=leak_shift, max_shift_px=max_shift_px, max_rot_milli=max_rot_milli,
                            max_zoom_milli=max_zoom_milli, crop_zoom_milli=crop_zoom_milli, reset_after=reset_after, border=border, device=device)
        self._device = self.cfg.device
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_stab_create(C.byref(self.cfg), C.byref(h)))
        self._h = h
        if gmc is True:
            from ..tracking.gmc import CameraMotionEstimator
            gmc, self._own_gmc = CameraMotionEstimator(n_streams=self.streams, device=device), True
        self.gmc = gmc

    def process(self, frames, warps=None, valid=None, masks=None, *, streams: Optional[Sequence[int]] = None, out=None, stride: Optional[int] = None,
                offset: int = 0, out_stride: Optional[int] = None, out_offset: int = 0):
        """Moves the path of ``streams[i]`` (None: stream i) and stabilises frame i, all frames in two launches.  ``frames``: host
        arrays (``size`` x 3 uint8, rows may be padded) or a ``_ffi.DeviceBuffer`` holding them one after another from ``offset``,
        rows ``stride`` bytes apart.  ``warps``: float32 ``(n, 2, 3)``, previous frame -> this frame in full-resolution pixels, with
        ``valid`` (n booleans; None: all valid); ``warps`` None: the estimator's when the stabiliser has one (``masks``: per frame None
        or something with ``xyxy`` and ``confidence`` in raw-frame coordinates, whose blocks take no part), else the identity.
        ``out``: None -- new host arrays for host frames, a new ``DeviceBuffer`` for device frames; or a list of host arrays (rows may
        be padded: the padding is not touched); or a ``DeviceBuffer``, frame i at ``out_offset + i * h * out_stride``.  Returns the
        host arrays or the ``DeviceBuffer`` -- frames the detector, ``MotionDetector``, ``FrameRenderer`` and ``JpegEncoder`` take as they
        are.  Source and destination may not overlap."""
        H, W = self.size
        on_dev = isinstance(frames, _ffi.DeviceBuffer)
        n = len(streams) if streams is not None else (self.streams if on_dev else len(frames))
        sptr, h, w, sst, smem, _ = _ffi.batch_frames(frames, n, height=H, width=W, stride=stride, offset=offset, writable=False)
        if n and (h, w) != self.size:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"frames of {w}x{h}, the stabiliser was created for {W}x{H}")
        if out is None:
            if on_dev:
                out_stride = 3 * W if out_stride is None else out_stride
                out = _ffi.DeviceBuffer(out_offset + max(n, 1) * H * int(out_stride), self._device)
            else:
                out = [np.zeros(self.size + (3,), np.uint8) for _ in range(n)]
        ret = out
        if not isinstance(out, _ffi.DeviceBuffer):
            out = list(out)
        dptr, oh, ow, dst, dmem, _ = _ffi.batch_frames(out, n, height=H, width=W, stride=out_stride, offset=out_offset, writable=True)
        if n and (oh, ow) != self.size:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"output frames of {ow}x{oh}, the stabiliser was created for {W}x{H}")
        if n == 0:
            return ret
        sp = None if streams is None else np.ascontiguousarray(list(streams), np.int32)
        L = _ffi.lib()
        if warps is None and self.gmc is not None:
            xy = cf = cnt = None
            if masks is not None:
                if len(masks) != n:
                    raise ValueError(f"{len(masks)} mask sets for {n} frames")
                MB = self.gmc.cfg.max_boxes
                xy, cf, cnt = np.zeros((n, MB, 4), np.float32), np.zeros((n, MB), np.float32), np.zeros(n, np.int32)
                for s, d in enumerate(masks):
                    if d is None:
                        continue
                    b = np.asarray(d.xyxy, np.float32).reshape(-1, 4)
                    if len(b) > MB:
                        raise ValueError(f"frame {s}: {len(b)} boxes > max_boxes {MB}")
                    xy[s, :len(b)], cf[s, :len(b)], cnt[s] = b, np.asarray(d.confidence, np.float32).reshape(-1), len(b)
            _ffi.check(L.rtmodt_stab_process_gmc(self._h, self.gmc.handle, (C.c_void_p * n)(*sptr), sst, smem, (C.c_void_p * n)(*dptr), dst, dmem,
                                                 _ffi.ptr(sp), n, _ffi.ptr(xy), _ffi.ptr(cf), _ffi.ptr(cnt)))
            self.gmc._geom = self.size
        else:
            wp = vp = None
            if warps is not None:
                wp = np.ascontiguousarray(warps, np.float32)
                if wp.size != 6 * n:
                    raise ValueError(f"warps of shape {wp.shape} for {n} frames: (n, 2, 3) expected")
            if valid is not None:
                vp = np.ascontiguousarray([1 if v else 0 for v in valid], np.uint8)
                if vp.size != n:
                    raise ValueError(f"{vp.size} valid flags for {n} frames")
            _ffi.check(L.rtmodt_stab_process(self._h, (C.c_void_p * n)(*sptr), sst, smem, (C.c_void_p * n)(*dptr), dst, dmem, _ffi.ptr(sp), n, _ffi.ptr(wp),
                                             _ffi.ptr(vp)))
        return ret

    def result(self):
        """-> one ``StabResult`` per stream: the status of its last call, its HOLD run, its path and the coefficients."""
        arr = (_ffi.StabStreamResult * self.streams)()
        _ffi.check(_ffi.lib().rtmodt_stab_result(self._h, arr))
        return [StabResult(int(r.status), int(r.hold), tuple(float(v) for v in r.j), tuple(int(v) for v in r.coef)) for r in arr]

    def state(self, stream: int = 0):
        """-> ``(path float64[4], hold)`` of one stream, for :meth:`load_state` after a restart."""
        j, hold = np.zeros(4, np.float64), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_stab_state(self._h, int(stream), _ffi.ptr(j), C.byref(hold)))
        return j, hold.value

    def load_state(self, stream: int, path, hold: int = 0) -> None:
        j = np.ascontiguousarray(path, np.float64).reshape(4)
        _ffi.check(_ffi.lib().rtmodt_stab_load_state(self._h, int(stream), _ffi.ptr(j), int(hold)))

    def to_source(self, xy, stream: int = 0) -> np.ndarray:
        """Points of the stabilised picture -> the raw frame the stream last saw (host, float64): a stabilised box drawn back on the
        raw frame, or mask boxes handed to the estimator in raw coordinates."""
        return map_points(self.cfg, self.state(stream)[0], xy, True)

    def to_stable(self, xy, stream: int = 0) -> np.ndarray:
        """Points of the raw frame the stream last saw -> the stabilised picture (the closed-form inverse)."""
        return map_points(self.cfg, self.state(stream)[0], xy, False)

    def reset(self, stream: int = -1) -> None:
        """One stream's path, or every path, back to the identity; the stabiliser's own estimator forgets its previous frame too."""
        _ffi.check(_ffi.lib().rtmodt_stab_reset(self._h, int(stream)))
        if self.gmc is not None and self._own_gmc:
            self.gmc.reset(stream)

    def last_ms(self) -> float:
        """Device time of the last ``process`` call's two launches (HIP events); the estimator's part is ``gmc.last_ms()``."""
        return _ffi.last_ms("rtmodt_stab_last_ms", self._h)

    _destroy = "rtmodt_stab_destroy"

    def close(self) -> None:
        super().close()
        if getattr(self, "_own_gmc", False) and self.gmc is not None:
            self.gmc.close()
            self.gmc = None
