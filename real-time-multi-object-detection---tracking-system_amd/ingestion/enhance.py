"""Frame enhancement on MI355X: at night without IR, at dusk, in backlight or in fog the scene occupies twenty or thirty grey levels out
of 256, and every stage that reads pixels -- ``MotionDetector``'s fixed thresholds, the detector's letterboxed copy -- sees a flat
picture.  ``FrameEnhancer`` lifts such frames by contrast-limited adaptive histogram equalisation (CLAHE) of the luma, what cameras and
NVRs ship as "WDR" or "low-light enhancement": per-tile luma histograms, clipped, integrated into tone curves, interpolated between
tile centres.  A per-frame CLAHE flickers on video and flicker is motion to ``MotionDetector``, so the tone curves are device-resident
state per stream and move by an integer EMA.  ``pipeline.run(enhance=...)`` runs it directly before ``motion``, after ``health`` (which
must judge the raw picture), ``undistort`` and ``stabilize``.  The reference hands ``cap.read()``'s frame on (``rtsp_reader.py``): it
has no counterpart.

The work runs in ``csrc/enhance.hip`` (rules in ``csrc/enhance_rule.h``); there is no CPU implementation here.
``tests/enhance_ref.py`` restates every rule and the kernels equal it exactly: all of it is integer arithmetic.  Unpinned: parity with
``cv2.createCLAHE`` (installed nowhere this runs; its tiles are padded by reflection and its interpolation is float), every default
(``tiles``, ``clip_limit``, ``smooth_shift``) -- none has been validated on real footage -- and any gain in detector recall.  Deliberate
limits: luma only; no denoising (``FrameDenoiser`` runs before it), gamma or white balance; one tile grid per handle; ``auto`` follows the frame mean without hysteresis.

Sizes are ``(height, width)`` and tile grids ``(tiles_y, tiles_x)`` throughout.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .. import _ffi

SHIFT, GAIN = 0, 1
COLOURS = {"shift": SHIFT, "gain": GAIN}
MAX_TILES = 16


class EnhanceResult(NamedTuple):
    stream: int
    frames_seen: int        # after the call
    luma_sum: int           # the sum of the frame's luma
    eff: int                # the strength this frame was enhanced with, 0..256
    clipped: int            # the pixels above the clip limit, summed over the tiles


def clip_q8(clip_limit: float) -> int:
    """A clip limit as OpenCV states it (2.0: a bin holds at most twice the mean) in 1 / 256."""
    return int(round(float(clip_limit) * 256))


def make_cfg(streams=1, height=0, width=0, tiles=(8, 8), clip_limit: Optional[float] = None, strength: Optional[int] = None,
             smooth_shift: Optional[int] = None, auto=None, colour=None, device=0) -> "_ffi.EnhanceCfg":
    """``rtmodt_enhance_default_cfg`` with the given fields replaced (None: the library's default)."""
    c = _ffi.EnhanceCfg()
    _ffi.lib().rtmodt_enhance_default_cfg(C.byref(c))
    c.streams, c.height, c.width, c.device = int(streams), int(height), int(width), _ffi.device_ordinal(device)
    if tiles is not None:
        if len(tiles) != 2:
            raise ValueError(f"tiles are (tiles_y, tiles_x), got {tiles!r}")
        c.tiles_y, c.tiles_x = int(tiles[0]), int(tiles[1])
    if clip_limit is not None:
        c.clip_q8 = clip_q8(clip_limit)
    if strength is not None:
        c.strength = int(strength)
    if smooth_shift is not None:
        c.smooth_shift = int(smooth_shift)
    if auto is not None:
        if len(auto) != 2:
            raise ValueError(f"auto is (auto_lo, auto_hi), got {auto!r}")
        c.auto_lo, c.auto_hi = int(auto[0]), int(auto[1])
    if colour is not None:
        if isinstance(colour, str) and colour not in COLOURS:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"colour {colour!r}: one of {sorted(COLOURS)}")
        c.colour = COLOURS[colour] if isinstance(colour, str) else int(colour)
    return c


def curve(hist, n: int, clip_q8: int):
    """``csrc/enhance_rule.h``'s tone curve of one tile on the host, no GPU (``rtmodt_enhance_curve``): ``hist`` (256 counts that sum
    to the tile's area ``n``) -> ``(curve uint32[256], excess)``."""
    hist = np.ascontiguousarray(hist, np.uint32)
    if hist.shape != (256,):
        raise ValueError(f"a histogram holds 256 counts, got shape {hist.shape}")
    out, ex = np.zeros(256, np.uint32), C.c_uint32(0)
    _ffi.check(_ffi.lib().rtmodt_enhance_curve(_ffi.ptr(hist), int(n), int(clip_q8), _ffi.ptr(out), C.byref(ex)))
    return out, ex.value


def axis_table(px: int, tiles: int):
    """Where each of ``px`` pixels sits among ``tiles`` tiles along one axis, on the host, no GPU (``rtmodt_enhance_axis``) ->
    ``(k int32[px], f int32[px], bounds int32[tiles + 1])``: pixel x interpolates ``f / 256`` of the way from tile ``k`` to tile
    ``min(k + 1, tiles - 1)``."""
    n = max(int(px), 0)
    k, f, b = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(max(int(tiles), 0) + 1, np.int32)
    _ffi.check(_ffi.lib().rtmodt_enhance_axis(int(px), int(tiles), _ffi.ptr(k), _ffi.ptr(f), _ffi.ptr(b)))
    return k, f, b


class FrameEnhancer(_ffi.Handle):
    """``streams`` enhancers for ``height x width`` BGR24 frames.

    ``tiles``: the ``(tiles_y, tiles_x)`` grid, 1..16 each way and no more than the pixels; tiles are not padded and differ in size by
    at most one pixel.  ``clip_limit``: a histogram bin holds at most this multiple of the tile's mean bin, what is above is spread
    over all bins (OpenCV's ``clipLimit``; 0: no clipping -- plain adaptive equalisation).  ``strength`` (0..256): how much of the
    equalised luma is taken.  ``smooth_shift`` (0..7): the tone curves move by ``1 / 2^smooth_shift`` per frame towards the frame's own;
    0 follows the frame at once (and flickers).  ``auto`` ``(lo, hi)`` with ``hi > lo``: the strength falls linearly from ``strength`` at
    a mean luma of ``lo`` to nothing at ``hi`` -- full strength at night, none by day; ``(0, 0)``: always ``strength``.  ``colour``:
    ``"shift"`` adds the luma change to every channel (chroma untouched), ``"gain"`` scales the channels by it (hue and saturation
    kept; chroma noise is amplified with the signal -- ``FrameDenoiser`` ahead of it removes it).  With an effective strength of 0 the output bytes are the input bytes under both.

    None of the defaults has been validated on real footage."""

    def __init__(self, streams: int, height: int, width: int, tiles=(8, 8), clip_limit: float = 2.0, strength: int = 256, smooth_shift: int = 2,
                 auto=(0, 0), colour="shift", device=0) -> None:
        self._h = None
        self._cfg = make_cfg(streams, height, width, tiles, clip_limit, strength, smooth_shift, auto, colour, device)
        self.streams, self.height, self.width = int(streams), int(height), int(width)
        self.tiles = (self._cfg.tiles_y, self._cfg.tiles_x)
        self._device = self._cfg.device
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_enhance_create(C.byref(self._cfg), C.byref(h)))
        self._h = h

    @property
    def state_shape(self):
        return self.tiles + (256,)

    def process(self, frames, out=None, streams: Optional[Sequence[int]] = None, want_results: bool = True, *, stride: Optional[int] = None,
                offset: int = 0, out_stride: Optional[int] = None, out_offset: int = 0) -> Optional[List[EnhanceResult]]:
        """Enhances one frame for each of the named streams (``streams`` None: streams ``0..n-1``; no duplicates), all frames in three
        launches.  ``frames``: host arrays (H x W x 3 uint8, rows may be padded) or a ``_ffi.DeviceBuffer`` holding them one after
        another from ``offset``, rows ``stride`` bytes apart.  ``out`` None: in place; else a list of host arrays or a ``DeviceBuffer``
        (``out_stride``, ``out_offset``) -- any mix of host and device.  A destination may be its own source; any other overlap of a
        destination with a source is refused.  Padding bytes are not touched.  Returns one ``EnhanceResult`` per frame, or None with
        ``want_results=False`` (nothing is copied back then).  Streams that are not named keep their state."""
        H, W = self.height, self.width
        on_dev = isinstance(frames, _ffi.DeviceBuffer)
        if not on_dev:
            frames = list(frames)
        n = len(streams) if streams is not None else (self.streams if on_dev else len(frames))
        sptr, h, w, sst, smem, _ = _ffi.batch_frames(frames, n, height=H, width=W, stride=stride, offset=offset, writable=out is None)
        if out is None:
            dptr, oh, ow, dst, dmem = sptr, h, w, sst, smem
        else:
            if not isinstance(out, _ffi.DeviceBuffer):
                out = list(out)
            dptr, oh, ow, dst, dmem, _ = _ffi.batch_frames(out, n, height=H, width=W, stride=out_stride, offset=out_offset, writable=True)
        if n == 0:
            return [] if want_results else None
        if (oh, ow) != (h, w):
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"output frames of {ow}x{oh} for frames of {w}x{h}")
        sp = np.ascontiguousarray(list(range(n)) if streams is None else list(streams), np.int32)
        res = (_ffi.EnhanceResult * n)() if want_results else None
        _ffi.check(_ffi.lib().rtmodt_enhance_process(self._h, (C.c_void_p * n)(*sptr), sst, smem, (C.c_void_p * n)(*dptr), dst, dmem, _ffi.ptr(sp), n, h, w, res))
        if not want_results:
            return None
        return [EnhanceResult(int(r.stream), int(r.frames_seen), int(r.luma_sum), int(r.eff), int(r.clipped)) for r in res]

    def state(self, stream: int = 0):
        """-> ``(s uint16 (tiles_y, tiles_x, 256) in 8.8 fixed point, frames_seen)`` of one stream, for :meth:`load_state` after a restart."""
        s, seen = np.zeros(self.state_shape, np.uint16), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_enhance_read_state(self._h, int(stream), _ffi.ptr(s), C.byref(seen)))
        return s, seen.value

    def load_state(self, stream: int, state) -> None:
        """Replaces one stream's state with ``state()``'s pair; another shape or a value above ``255 << 8`` is refused."""
        s = np.ascontiguousarray(state[0], np.uint16)
        if s.shape != self.state_shape:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"state of shape {s.shape}, this enhancer's is {self.state_shape}")
        _ffi.check(_ffi.lib().rtmodt_enhance_load_state(self._h, int(stream), _ffi.ptr(s), s.size, int(state[1])))

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets one stream's tone curves, or (None) every stream's: the next frame sets them."""
        _ffi.check(_ffi.lib().rtmodt_enhance_reset(self._h, -1 if stream is None else int(stream)))

    def histograms(self, stream: int = 0) -> np.ndarray:
        """The last call's luma histograms of ``stream``, uint32 ``(tiles_y, tiles_x, 256)``, for tests and tuning."""
        hist = np.zeros(self.state_shape, np.uint32)
        _ffi.check(_ffi.lib().rtmodt_enhance_histograms(self._h, int(stream), _ffi.ptr(hist)))
        return hist

    def kernel_ms(self) -> float:
        """Device time of the last ``process`` call's memset and three launches (HIP events)."""
        return _ffi.last_ms("rtmodt_enhance_last_ms", self._h)

    _destroy = "rtmodt_enhance_destroy"
