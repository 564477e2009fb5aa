"""The DeepSORT embedder of the reference's config (``tracking.deepsort.embedder: "weights/osnet_x0_25.onnx"``,
config/default.yaml:60) on MI355X: OSNet x0.25 behind ``rtmodt_reid_*`` (``include/rtmodt.h``, ``csrc/reid.hip``), from the BGR frame
in HBM to an int8[512] descriptor per box.  PINNED: the crop and the quantiser exactly, the network within a measured fp16 bound
of float64.  PARITY UNPINNED: torchreid, cv2 and ``deep_sort_realtime`` are not installed anywhere this runs.  Weights come from
a ``.rtreid`` file (``reid_weights``); an ``.onnx`` file is not read.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import _ffi
from ..reid_weights import FEAT_DIM, SUFFIX, TAPS

_TAP_SHAPES = {"crop": ((256, 128, 3), np.uint8), "conv1": ((128, 64, 16), np.float16), "maxpool": ((64, 32, 16), np.float16),
               "conv2.0": ((64, 32, 64), np.float16), "conv2.1": ((64, 32, 64), np.float16), "conv2.2": ((32, 16, 64), np.float16),
               "conv3.0": ((32, 16, 96), np.float16), "conv3.1": ((32, 16, 96), np.float16), "conv3.2": ((16, 8, 96), np.float16),
               "conv4.0": ((16, 8, 128), np.float16), "conv4.1": ((16, 8, 128), np.float16), "conv5": ((16, 8, 128), np.float16),
               "feat": ((FEAT_DIM,), np.float32)}
assert tuple(_TAP_SHAPES) == TAPS


def check_weights_path(path) -> str:
    """The path of an existing ``.rtreid`` file, or ``FileNotFoundError`` worded like the detector's."""
    path = str(path)
    if not path.endswith(SUFFIX):
        raise ValueError(f"Re-ID weights are a {SUFFIX} file (python tools/convert_weights.py --reid <checkpoint> <out{SUFFIX}>), got {path!r}")
    if not os.path.exists(path):
        raise FileNotFoundError(f"No Re-ID model found at {path}")
    return path


class ReidEmbedder(_ffi.Handle):
    """``embed(frames, boxes, counts) -> (feat, desc)`` for up to ``max_frames`` frames of up to ``max_boxes`` boxes each."""

    def __init__(self, weights, device=0, max_boxes: int = 128, max_frames: int = 8) -> None:
        self.weights = check_weights_path(weights)
        self.max_boxes, self.max_frames = int(max_boxes), int(max_frames)
        self._device = _ffi.device_ordinal(device)
        cfg = _ffi.ReidCfg(self.weights.encode(), self._device, self.max_frames, self.max_boxes)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_reid_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def embed(self, frames, boxes, counts=None, *, mem_kind=_ffi.MEM_HOST, height=0, width=0, stride=0):
        """``frames``: as ``DeepSortTracker`` takes them (host ``(h, w, 3)`` uint8 BGR arrays, or device addresses with the geometry
        given).  ``boxes``: ``(n_frames, mb, 4)`` xyxy with ``counts[n_frames]`` valid rows each, or a list of ``(n_i, 4)`` arrays.
        Returns ``feat (n_frames, mb, 512) float32`` and ``desc (n_frames, mb, 512) int8``; rows past ``counts`` and rows of empty
        boxes are zero."""
        n = len(frames)
        if counts is None:
            rows = [np.asarray(b, np.float32).reshape(-1, 4) for b in boxes]
            mb = max(1, max((len(b) for b in rows), default=1))
            xy = np.zeros((n, mb, 4), np.float32)
            for i, b in enumerate(rows):
                xy[i, :len(b)] = b
            counts = [len(b) for b in rows]
        else:
            xy = np.ascontiguousarray(boxes, np.float32).reshape(n, -1, 4)
            mb = xy.shape[1]
        counts = np.ascontiguousarray(counts, np.int32).reshape(n)
        fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        feat, desc = np.zeros((n, mb, FEAT_DIM), np.float32), np.zeros((n, mb, FEAT_DIM), np.int8)
        _ffi.check(_ffi.lib().rtmodt_reid_embed(self._h, fp, n, int(height), int(width), int(stride), int(mem_kind), _ffi.ptr(xy), _ffi.ptr(counts), mb,
                                                _ffi.ptr(feat), _ffi.ptr(desc)))
        del keep
        return feat, desc

    def tap(self, name: str) -> np.ndarray:
        """One of ``reid_weights.TAPS`` as the last ``embed`` left it: ``(max_frames, max_boxes, ...)`` (fp16 NHWC maps, the uint8 RGB
        crop, the float32 feature).  Rows of slots without a box hold stale bytes."""
        shape, dt = _TAP_SHAPES[name]
        out = np.zeros((self.max_frames, self.max_boxes) + shape, dt)
        need = C.c_size_t(0)
        _ffi.check(_ffi.lib().rtmodt_reid_tap(self._h, name.encode(), _ffi.ptr(out), out.nbytes, C.byref(need)))
        assert need.value == out.nbytes
        return out

    def last_ms(self) -> tuple:
        """Device time (ms) of the last embed: (crop, network + quantiser)."""
        return _ffi.last_ms("rtmodt_reid_last_ms", self._h, 2)

    _destroy = "rtmodt_reid_destroy"
