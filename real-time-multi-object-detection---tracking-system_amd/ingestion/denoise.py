"""Frame noise reduction on MI355X: high-gain sensor noise is on every pixel of every night frame, and everything that reads pixels
pays for it -- ``FrameEnhancer`` multiplies it, ``JpegEncoder`` spends bytes coding it, ``SnapshotGallery`` and ``ColourAttributes``
keep it.  ``FrameDenoiser`` is what cameras and NVRs ship as "3DNR": per stream a running mean of every pixel in 8.8 fixed point,
device-resident, which a pixel follows slowly while its 3 x 3 neighbourhood is still and at once when it moves; a moving pixel is
smoothed by a sigma filter over its neighbours of similar luma instead.  ``pipeline.run(denoise=...)`` runs it directly after
``stabilize`` (a temporal filter needs registered frames) and directly before ``enhance`` (which should equalise the clean picture,
not the noise).  The reference hands ``cap.read()``'s frame on (``rtsp_reader.py``): it has no counterpart.

The work runs in ``csrc/denoise.hip`` (rules in ``csrc/denoise_rule.h``); there is no CPU implementation here.
``tests/denoise_ref.py`` restates every rule and the kernel equals it exactly: all of it is integer arithmetic.  Unpinned: parity with
any camera's 3DNR, ``cv2.fastNlMeansDenoising`` or ffmpeg's ``hqdn3d`` (installed nowhere this runs), every default -- none has been
validated on real footage -- and any gain in detector recall.  Deliberate limits: no motion compensation (a PTZ move is motion
everywhere and the frame passes unfiltered in time); the thresholds do not adapt to the measured noise (``DenoiseResult.noise_q8``
reports it, the choice stays with the caller); BGR24 only; no in-place form, because an output pixel depends on its neighbours' inputs.

Sizes are ``(height, width)`` throughout.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .. import _ffi

MAX_THRESHOLD = 9 * 255
MAX_ACC = 255 << 8


class DenoiseResult(NamedTuple):
    stream: int
    frames_seen: int        # after the call
    n_static: int           # the pixels the temporal filter held (a == 0)
    n_moving: int           # the pixels that took the frame at once (a == 256)
    absdiff_static: int     # the sum of |Y(x) - Y(prev)| over the static pixels

    @property
    def noise_q8(self) -> int:
        """The mean luma difference of the static pixels in 1 / 256 of a level (0 without static pixels): the noise figure an
        operator tunes ``motion`` with."""
        return 256 * self.absdiff_static // self.n_static if self.n_static else 0


def make_cfg(streams=1, height=0, width=0, motion=None, temporal_shift: Optional[int] = None, spatial: Optional[int] = None,
             spatial_thr: Optional[int] = None, device=0) -> "_ffi.DenoiseCfg":
    """``rtmodt_denoise_default_cfg`` with the given fields replaced (None: the library's default)."""
    c = _ffi.DenoiseCfg()
    _ffi.lib().rtmodt_denoise_default_cfg(C.byref(c))
    c.streams, c.height, c.width, c.device = int(streams), int(height), int(width), _ffi.device_ordinal(device)
    if motion is not None:
        if len(motion) != 2:
            raise ValueError(f"motion is (motion_lo, motion_hi), got {motion!r}")
        c.motion_lo, c.motion_hi = int(motion[0]), int(motion[1])
    if temporal_shift is not None:
        c.temporal_shift = int(temporal_shift)
    if spatial is not None:
        c.spatial = int(spatial)
    if spatial_thr is not None:
        c.spatial_thr = int(spatial_thr)
    return c


def pixel(cur, acc, inside: int = 0x1FF, frames_seen: int = 1, cfg: Optional["_ffi.DenoiseCfg"] = None):
    """``csrc/denoise_rule.h``'s rule for one pixel on the host, no GPU (``rtmodt_denoise_pixel``): ``cur`` (3 x 3 x 3 uint8, the
    frame's neighbourhood, coordinates clamped by the caller), ``acc`` (3 x 3 x 3 uint16, the state's) and the nine ``inside`` bits ->
    ``(out uint8[3], acc uint16[3], a, D)``."""
    cur, acc = np.ascontiguousarray(cur, np.uint8), np.ascontiguousarray(acc, np.uint16)
    if cur.shape != (3, 3, 3) or acc.shape != (3, 3, 3):
        raise ValueError(f"two 3 x 3 x 3 neighbourhoods, got shapes {cur.shape} and {acc.shape}")
    cfg = make_cfg() if cfg is None else cfg
    out, new, a, d = np.zeros(3, np.uint8), np.zeros(3, np.uint16), C.c_int32(0), C.c_int32(0)
    _ffi.check(_ffi.lib().rtmodt_denoise_pixel(C.byref(cfg), _ffi.ptr(cur), _ffi.ptr(acc), int(inside), int(frames_seen), _ffi.ptr(out), _ffi.ptr(new),
                                               C.byref(a), C.byref(d)))
    return out, new, a.value, d.value


class FrameDenoiser(_ffi.Handle):
    """``streams`` denoisers for ``height x width`` BGR24 frames.

    ``motion`` ``(lo, hi)``, ``0 <= lo < hi <= 2295``, in units of the 3 x 3 luma sum: a pixel whose neighbourhood's summed luma
    difference to the state is at most ``lo`` is static, one at ``hi`` or above is moving, between them the two filters blend.  Zero-mean
    noise cancels in the sum, so ``lo`` sits a little above ``3 x`` the noise's standard deviation in luma levels.
    ``temporal_shift`` (0..6): a static pixel moves by ``1 / 2^temporal_shift`` per frame towards the frame's; 0: no temporal filtering.
    ``spatial`` (0..256): how much of the sigma filter's mean a moving pixel takes; ``spatial_thr`` (0..255): a neighbour counts in
    that mean when its luma is at most this far from the pixel's, so edges stay.  ``temporal_shift=0, spatial=0`` returns the input bytes.

    None of the defaults has been validated on real footage."""

    def __init__(self, streams: int, height: int, width: int, motion=(18, 54), temporal_shift: int = 3, spatial: int = 256, spatial_thr: int = 6,
                 device=0) -> None:
        self._h = None
        self._cfg = make_cfg(streams, height, width, motion, temporal_shift, spatial, spatial_thr, device)
        self.streams, self.height, self.width = int(streams), int(height), int(width)
        self._device = self._cfg.device
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_denoise_create(C.byref(self._cfg), C.byref(h)))
        self._h = h

    @property
    def state_shape(self):
        return (self.height, self.width, 3)

    def process(self, frames, out, streams: Optional[Sequence[int]] = None, want_results: bool = True, *, stride: Optional[int] = None,
                offset: int = 0, out_stride: Optional[int] = None, out_offset: int = 0) -> Optional[List[DenoiseResult]]:
        """Filters one frame for each of the named streams (``streams`` None: streams ``0..n-1``; no duplicates), all frames in two
        launches.  ``frames``: host arrays (H x W x 3 uint8, rows may be padded) or a ``_ffi.DeviceBuffer`` holding them one after
        another from ``offset``, rows ``stride`` bytes apart.  ``out``: a list of host arrays or a ``DeviceBuffer`` (``out_stride``,
        ``out_offset``) -- any mix of host and device.  There is no in-place form, because an output pixel depends on its neighbours'
        inputs: a destination that overlaps any source of the call, its own included, is refused.  Padding bytes are not touched.
        Returns one ``DenoiseResult`` per frame, or None with ``want_results=False`` (nothing is copied back then).  Streams that are
        not named keep their state."""
        H, W = self.height, self.width
        on_dev = isinstance(frames, _ffi.DeviceBuffer)
        if not on_dev:
            frames = list(frames)
        n = len(streams) if streams is not None else (self.streams if on_dev else len(frames))
        sptr, h, w, sst, smem, _ = _ffi.batch_frames(frames, n, height=H, width=W, stride=stride, offset=offset, writable=False)
        if not isinstance(out, _ffi.DeviceBuffer):
            out = list(out)
        dptr, oh, ow, dst, dmem, _ = _ffi.batch_frames(out, n, height=H, width=W, stride=out_stride, offset=out_offset, writable=True)
        if n == 0:
            return [] if want_results else None
        if (oh, ow) != (h, w):
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"output frames of {ow}x{oh} for frames of {w}x{h}")
        sp = np.ascontiguousarray(list(range(n)) if streams is None else list(streams), np.int32)
        res = (_ffi.DenoiseResult * n)() if want_results else None
        _ffi.check(_ffi.lib().rtmodt_denoise_process(self._h, (C.c_void_p * n)(*sptr), sst, smem, (C.c_void_p * n)(*dptr), dst, dmem, _ffi.ptr(sp), n, h, w, res))
        if not want_results:
            return None
        return [DenoiseResult(int(r.stream), int(r.frames_seen), int(r.n_static), int(r.n_moving), int(r.absdiff_static)) for r in res]

    def state(self, stream: int = 0):
        """-> ``(acc uint16 (height, width, 3) in 8.8 fixed point, frames_seen)`` of one stream, for :meth:`load_state` after a restart."""
        acc, seen = np.zeros(self.state_shape, np.uint16), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_denoise_read_state(self._h, int(stream), _ffi.ptr(acc), C.byref(seen)))
        return acc, seen.value

    def load_state(self, stream: int, state) -> None:
        """Replaces one stream's state with ``state()``'s pair; another shape or a value above ``255 << 8`` is refused."""
        acc = np.ascontiguousarray(state[0], np.uint16)
        if acc.shape != self.state_shape:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"state of shape {acc.shape}, this denoiser's is {self.state_shape}")
        _ffi.check(_ffi.lib().rtmodt_denoise_load_state(self._h, int(stream), _ffi.ptr(acc), acc.size, int(state[1])))

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets one stream's state, or (None) every stream's: the next frame passes and sets it."""
        _ffi.check(_ffi.lib().rtmodt_denoise_reset(self._h, -1 if stream is None else int(stream)))

    def kernel_ms(self) -> float:
        """Device time of the last ``process`` call's memset and two launches (HIP events)."""
        return _ffi.last_ms("rtmodt_denoise_last_ms", self._h)

    _destroy = "rtmodt_denoise_destroy"
