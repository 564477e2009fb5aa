"""What the reference's ``cap.read()`` does for a Motion-JPEG camera (``src/ingestion/rtsp_reader.py``: ``cv2.VideoCapture``) and
its web API for an uploaded image (``web/server.py``: ``cv2.imdecode``), on MI355X.

``JpegDecoder`` turns batches of baseline JPEG files into BGR24 frames -- host arrays, or frames inside a ``_ffi.DeviceBuffer`` laid
out as ``FrameRenderer.render_batch`` / ``JpegEncoder.encode_batch`` / ``Detector`` (device frames) take them, so a decoded frame is
detected and drawn on where it lies.  The decoding runs in ``csrc/jpeg_dec.hip``; there is no CPU implementation here.  The pixels
equal libjpeg-turbo's default decoder's (``tests/test_jpeg_dec_cpu.py`` pins the rules against Pillow); what is accepted is listed in
``csrc/jpeg_dec_core.h``.  A stream without restart markers is decoded by one GPU lane per frame: correct, and slow
(``profiles/jpegdec/README.md``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .. import _ffi

_EMPTY = (C.c_char * 1)()                  # what an empty file points at
STATUS_NAMES = ("OK", "UNSUPPORTED", "CORRUPT", "TRUNCATED", "SIZE_MISMATCH")


class JpegDecodeError(ValueError):
    """A file the decoder rejected; ``status`` is one of ``_ffi.JPEG_*``."""

    def __init__(self, status: int, message: str = ""):
        super().__init__(f"JPEG {STATUS_NAMES[status]}" + (f": {message}" if message else ""))
        self.status = status


def probe(file) -> _ffi.JpegInfo:
    """``rtmodt_jpeg_probe``: height, width, components, sampling, restart interval and status of a file's header (host only)."""
    buf = np.frombuffer(bytes(file), np.uint8)
    info = _ffi.JpegInfo()
    _ffi.check(_ffi.lib().rtmodt_jpeg_probe(_ffi.ptr(buf) if len(buf) else None, len(buf), C.byref(info)))
    return info


class JpegDecoder(_ffi.Handle):
    """Baseline JPEG files -> BGR24 frames on the GPU."""

    def __init__(self, *, device=0, max_height: int = 1080, max_width: int = 1920, max_batch: int = 8, max_file_bytes: int = 0) -> None:
        self._device = _ffi.device_ordinal(device)
        self._max = [int(max_height), int(max_width), int(max_batch), int(max_file_bytes) or int(max_height) * int(max_width) * 3 // 4 + 65536]
        self._h = None
        self._open()

    def decode(self, file, *, gray_plane: bool = False) -> np.ndarray:
        """One file -> its H x W x 3 uint8 BGR frame (a one-component file: B = G = R = Y, or the H x W plane with ``gray_plane``).
        Raises ``JpegDecodeError`` for a file that is not decoded."""
        info = probe(file)
        if info.status != _ffi.JPEG_OK:
            raise JpegDecodeError(info.status, info.message.decode(errors="replace"))
        out = np.empty((1, info.h, info.w, 3), np.uint8)
        status = self.decode_batch([file], out=out)[1]
        if status[0] != _ffi.JPEG_OK:
            raise JpegDecodeError(int(status[0]))
        return np.ascontiguousarray(out[0, :, :, 0]) if gray_plane and info.components == 1 else out[0]

    def decode_batch(self, files, *, out=None, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                     offset: int = 0, mem_kind: Optional[int] = None):
        """``(frames, status)``: file i decoded into frame i; ``status`` is an int32 array of ``_ffi.JPEG_*`` (a frame whose status
        is not OK keeps the bytes it had).  ``out``: ``None`` -- a new ``(n, h, w, 3)`` host array with the size of the first file's
        header; a host uint8 array ``(n, h, w, 3)`` whose rows may be padded (``mem_kind`` ``MEM_HOST``); or a ``_ffi.DeviceBuffer``
        with ``height`` / ``width`` given, frame i at ``offset + i * height * stride`` (``stride`` defaults to ``3 * width``), which
        is filled in place and returned (``MEM_DEVICE``)."""
        files = [np.frombuffer(bytes(f), np.uint8) for f in files]
        n = len(files)
        if isinstance(out, _ffi.DeviceBuffer):
            if mem_kind not in (None, _ffi.MEM_DEVICE):
                raise ValueError("a DeviceBuffer is device memory")
            rows = out
        else:
            if mem_kind not in (None, _ffi.MEM_HOST):
                raise ValueError("device frames are passed as a _ffi.DeviceBuffer")
            if out is None:
                if n == 0:
                    return np.empty((0, 0, 0, 3), np.uint8), np.zeros(0, np.int32)
                info = probe(files[0])
                if info.status != _ffi.JPEG_OK:
                    raise JpegDecodeError(info.status, info.message.decode(errors="replace"))
                out = np.zeros((n, info.h, info.w, 3), np.uint8)
            if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 4 or out.shape[0] < n or out.shape[3] != 3 \
                    or out.shape[1] < 1 or out.shape[2] < 1:
                raise ValueError(f"out is a writable (n, h, w, 3) uint8 array of non-empty frames, got {getattr(out, 'shape', type(out))}")
            rows = list(out[:n])                          # frame i as an (h, w, 3) view: the row pitch is out.strides[1]
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(rows, n, height=height, width=width, stride=stride, offset=offset, strict=True)
        if n == 0:
            return out, np.zeros(0, np.int32)
        biggest = max(len(f) for f in files)
        if h > self._max[0] or w > self._max[1] or n > self._max[2] or biggest > self._max[3]:      # a larger frame, batch or file: a larger handle
            self._max = [max(h, self._max[0]), max(w, self._max[1]), max(n, self._max[2]), max(biggest, self._max[3])]
            self.close()
            self._open()
        fp = (C.c_void_p * n)(*[f.ctypes.data if len(f) else C.addressof(_EMPTY) for f in files])
        sizes = (C.c_size_t * n)(*[len(f) for f in files])
        dp = (C.c_void_p * n)(*ptrs)
        status = np.zeros(n, np.int32)
        _ffi.check(_ffi.lib().rtmodt_jpegdec_decode_batch(self._h, fp, sizes, n, dp, h, w, st, mem, _ffi.ptr(status)))
        return out, status

    def coefficients(self, frame: int, component: int) -> np.ndarray:
        """The entropy decoder's output of the last batch: int16 ``[block rows, block cols, 64]``, natural order, not dequantised."""
        rows, cols = C.c_int(0), C.c_int(0)
        L = _ffi.lib()
        _ffi.check(L.rtmodt_jpegdec_coefficients(self._h, int(frame), int(component), None, 0, C.byref(rows), C.byref(cols)))
        out = np.zeros((rows.value, cols.value, 64), np.int16)
        _ffi.check(L.rtmodt_jpegdec_coefficients(self._h, int(frame), int(component), _ffi.ptr(out), out.size, C.byref(rows), C.byref(cols)))
        return out

    def last_kernel_ms(self) -> float:
        """Device time of the last batch's kernels (HIP events)."""
        return _ffi.last_ms("rtmodt_jpegdec_last_ms", self._h)

    _destroy = "rtmodt_jpegdec_destroy"

    def _open(self) -> None:
        cfg = _ffi.JpegDecCfg(self._max[0], self._max[1], self._max[2], self._max[3])
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_jpegdec_create(self._device, C.byref(cfg), C.byref(h)))
        self._h = h
