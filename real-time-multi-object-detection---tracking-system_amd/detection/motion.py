"""Motion detection on MI355X: is anything moving in this stream?  A background model per stream on a downscaled luma grid, resident
on the device, is updated from a batch of frames in one call and answers per stream: warm-up, still, motion or scene change, with
counts, the bounding box of the motion and its connected regions.  ``pipeline.run(motion=...)`` uses the answer to keep the
detector off still frames -- what Frigate's motion detector and DeepStream's ``interval`` are for.  The reference drops frames blind
to content (design document B.1) and offers a smaller model or input against a low frame rate (G.1 row 2, G.3).

The work runs in ``csrc/motion.hip`` (rules in its header comment and in ``csrc/motion_model.h``); there is no CPU implementation
here.  ``tests/motion_ref.py`` restates every rule and the kernels equal it exactly: all of it is integer arithmetic.  Unpinned:
parity with OpenCV's ``BackgroundSubtractorMOG2`` and with Frigate (neither is installed where this runs), and every default -- none
has been validated on real footage.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import _ffi

WARMUP, STILL, MOTION, SCENE_CHANGE = 0, 1, 2, 3
STATUS_NAMES = ("warmup", "still", "motion", "scene_change")
CFG_FIELDS = ("scale", "learn_shift", "learn_shift_fg", "threshold", "dev_gain", "min_neighbors", "dilate", "warmup", "scene_pm", "min_area",
              "max_regions", "block")


def make_cfg(streams=1, height=0, width=0, device=0, **cfg) -> "_ffi.MotionCfg":
    """``rtmodt_motion_default_cfg`` with the given fields replaced."""
    c = _ffi.MotionCfg()
    _ffi.lib().rtmodt_motion_default_cfg(C.byref(c))
    c.streams, c.height, c.width, c.device = int(streams), int(height), int(width), _ffi.device_ordinal(device)
    for k, v in cfg.items():
        if k not in CFG_FIELDS:
            raise TypeError(f"unknown motion parameter {k!r}; one of {CFG_FIELDS}")
        setattr(c, k, int(v))
    return c


def motion_cell(yc: int, frames_seen: int, bg: int, dev: int, **cfg) -> Tuple[int, int, bool]:
    """``rtmodt_motion_cell`` (host only): one cell of luma ``yc`` under the rule fields of ``cfg`` -> (bg, dev, raw)."""
    c = make_cfg(1, 1, 1, **cfg)
    b, d, raw = C.c_uint16(int(bg)), C.c_uint16(int(dev)), C.c_int32(0)
    _ffi.check(_ffi.lib().rtmodt_motion_cell(C.byref(c), int(yc), int(frames_seen), C.byref(b), C.byref(d), C.byref(raw)))
    return b.value, d.value, bool(raw.value)


@dataclass
class MotionResult:
    """One stream's answer for one frame.  ``bbox`` and ``regions`` are pixels ``(x0, y0, x1, y1)`` with x1 / y1 exclusive; a region
    adds its area in cells.  ``regions`` holds the first ``max_regions`` of ``n_regions_total``."""
    stream: int
    status: int
    n_raw: int
    n_fg: int
    mean_luma: float
    bbox: Tuple[int, int, int, int]
    regions: List[Tuple[int, int, int, int, int]] = field(default_factory=list)
    n_regions_total: int = 0
    frames_seen: int = 0
    luma_sum: int = 0

    @property
    def status_name(self) -> str:
        return STATUS_NAMES[self.status]


class MotionDetector(_ffi.Handle):
    """``streams`` background models for ``height x width`` BGR24 frames.

    ``scale`` (1, 2, 4, 8): pixels per cell side of the luma grid.  ``learn_shift`` (1..8) and ``learn_shift_fg`` (0: never, else
    ``learn_shift``..12): how fast background and foreground cells are absorbed.  A cell is raw foreground when it differs from the
    model by more than ``threshold`` (1..255 luma levels) plus ``dev_gain`` (0..8) times its running deviation; it is kept with
    ``min_neighbors`` (1..9) raw cells in its 3 x 3 neighbourhood, and the kept cells are dilated by ``dilate`` (0..3).  The first
    ``warmup`` frames only learn.  ``scene_pm`` per mille of raw cells is a scene change, after which the model starts over.  A
    region is an 8-connected component of at least ``min_area`` cells; ``max_regions`` (1..256) are returned.  ``block``: cells
    per side of a block of the activity grid.

    ``max_still`` is read by ``pipeline.run``: after that many consecutive skipped frames the detector runs anyway (0: never)."""

    def __init__(self, streams: int, height: int, width: int, *, max_still: int = 25, device=0, **cfg) -> None:
        self._h = None
        self._cfg = make_cfg(streams, height, width, device, **cfg)
        self.streams, self.height, self.width = int(streams), int(height), int(width)
        self.max_still = int(max_still)
        if self.max_still < 0:
            raise ValueError(f"max_still {max_still} below 0")
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_motion_create(C.byref(self._cfg), C.byref(h)))
        self._h = h
        c = self._cfg
        self.scale, self.max_regions, self.block = c.scale, c.max_regions, c.block
        self.grid_shape = (-(-self.height // c.scale), -(-self.width // c.scale))
        self.block_shape = (-(-self.grid_shape[0] // c.block), -(-self.grid_shape[1] // c.block))

    def process(self, frames, streams: Optional[Sequence[int]] = None, *, stride: Optional[int] = None, offset: int = 0) -> List[MotionResult]:
        """One frame for each of the named streams (None: one per stream, in order): host arrays (H x W x 3 uint8, rows may be
        padded) or a ``_ffi.DeviceBuffer`` holding the frames one after another from ``offset``, rows ``stride`` bytes apart.  The
        frames are only read.  Streams that are not named keep their state."""
        n = self.streams if streams is None else len(streams)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=self.height, width=self.width, stride=stride, offset=offset, writable=False)
        if n == 0:
            return []
        fp = (C.c_void_p * n)(*ptrs)
        sp = None if streams is None else np.ascontiguousarray(list(streams), np.int32)
        res = (_ffi.MotionResult * n)()
        reg = np.zeros((n, self.max_regions, 5), np.int32)
        _ffi.check(_ffi.lib().rtmodt_motion_process(self._h, fp, _ffi.ptr(sp), n, h, w, st, mem, res, _ffi.ptr(reg)))
        cells = self.grid_shape[0] * self.grid_shape[1]
        return [MotionResult(r.stream, r.status, r.n_raw, r.n_fg, r.luma_sum / cells, tuple(r.bbox),
                             [tuple(int(v) for v in reg[i, k]) for k in range(r.n_regions)], r.n_regions_total, r.frames_seen, r.luma_sum)
                for i, r in enumerate(res)]

    def mask(self, stream: int = 0) -> np.ndarray:
        """The mask of the stream's last frame, ``uint8 (gh, gw)`` of 0 / 1."""
        out = np.zeros(self.grid_shape, np.uint8)
        _ffi.check(_ffi.lib().rtmodt_motion_read_mask(self._h, int(stream), _ffi.ptr(out)))
        return out

    def blocks(self, stream: int = 0) -> np.ndarray:
        """The mask cells per ``block x block`` group of cells, ``uint32``."""
        out = np.zeros(self.block_shape, np.uint32)
        _ffi.check(_ffi.lib().rtmodt_motion_read_blocks(self._h, int(stream), _ffi.ptr(out)))
        return out

    def state(self, stream: int = 0):
        """-> (bg, dev, frames_seen): copies of one stream's model, ``uint16 (gh, gw)`` each in 8.8 fixed point."""
        bg, dev, seen = np.zeros(self.grid_shape, np.uint16), np.zeros(self.grid_shape, np.uint16), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_motion_read_state(self._h, int(stream), _ffi.ptr(bg), _ffi.ptr(dev), C.byref(seen)))
        return bg, dev, seen.value

    def load_state(self, bg, dev, frames_seen: int, stream: int = 0) -> None:
        """Replaces one stream's model with a saved one (``state()``'s shapes), so that it survives a restart."""
        bg, dev = np.ascontiguousarray(bg, np.uint16), np.ascontiguousarray(dev, np.uint16)
        if bg.shape != self.grid_shape or dev.shape != self.grid_shape:
            raise ValueError(f"a model of {bg.shape} / {dev.shape}, this detector's grid is {self.grid_shape}")
        _ffi.check(_ffi.lib().rtmodt_motion_load_state(self._h, int(stream), _ffi.ptr(bg), _ffi.ptr(dev), int(frames_seen)))

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets one stream's model, or (None) every model: the next frame starts a warm-up."""
        _ffi.check(_ffi.lib().rtmodt_motion_reset(self._h, -1 if stream is None else int(stream)))

    def last_kernel_ms(self) -> float:
        """Device time of the last ``process`` call's launches (HIP events)."""
        return _ffi.last_ms("rtmodt_motion_last_ms", self._h)

    _destroy = "rtmodt_motion_destroy"
