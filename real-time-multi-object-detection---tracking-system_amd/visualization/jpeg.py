"""What the reference does with an annotated frame (``tools/run_pipeline.py:112-117,160-161``: ``cv2.VideoWriter``, fourcc ``MJPG``
included; ``web/server.py:151-175``: JPEG frames over HTTP) on MI355X.

``JpegEncoder`` turns batches of BGR24 frames -- host arrays or a ``_ffi.DeviceBuffer``, with exactly ``FrameRenderer.render_batch``'s
conventions, so the same buffer goes render -> encode -- into baseline JPEG files.  The encoding runs in ``csrc/jpeg.hip`` (stream
format and integer arithmetic in its header comment); there is no CPU implementation here.  The files equal libjpeg-turbo's for the
same pixels (4:2:0, Annex K Huffman tables, one restart interval per MCU row), which ``tests/test_jpeg_cpu.py`` pins against Pillow.

``MjpegWriter`` has the calls ``run_pipeline.py`` makes on ``cv2.VideoWriter`` (``write`` / ``release``) and stores JPEG bytes as a
RIFF AVI with an ``MJPG`` stream or as a bare ``.mjpeg`` concatenation; ``multipart_chunk`` frames one JPEG for a
``multipart/x-mixed-replace`` HTTP body.  Both are pure Python.  No player is available to test against: parity with players is
unpinned.  ``MjpegRecorder`` joins the two for ``pipeline.run(..., recorder=...)``.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import Optional, Sequence

import numpy as np

from .. import _ffi

AVI_MAX_BYTES = (1 << 31) - 1                 # plain AVI 1.0 (no OpenDML): the file stays below 2 GiB


def header(quality: int, height: int, width: int) -> bytes:
    """``rtmodt_jpeg_header``: SOI up to and including the SOS header (host only)."""
    need = C.c_size_t(0)
    L = _ffi.lib()
    _ffi.check(L.rtmodt_jpeg_header(int(quality), int(height), int(width), None, 0, C.byref(need)))
    buf = np.zeros(need.value, np.uint8)
    _ffi.check(L.rtmodt_jpeg_header(int(quality), int(height), int(width), _ffi.ptr(buf), buf.nbytes, C.byref(need)))
    return buf.tobytes()


class JpegEncoder(_ffi.Handle):
    """Baseline JPEG (4:2:0) of BGR24 frames on the GPU."""

    def __init__(self, quality: int = 95, *, device=0, max_height: int = 1080, max_width: int = 1920, max_batch: int = 8) -> None:
        if not 1 <= int(quality) <= 100:
            raise ValueError(f"quality {quality} outside 1..100")
        self.quality = int(quality)
        self._device = _ffi.device_ordinal(device)
        self._max = (int(max_height), int(max_width), int(max_batch))
        self._h = None
        self._open()

    def encode(self, frame: np.ndarray) -> bytes:
        """One H x W x 3 uint8 BGR frame (rows may be padded) -> its JPEG file."""
        return self.encode_batch([frame])[0]

    def encode_batch(self, frames, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                     offset: int = 0, count: Optional[int] = None, slot_bytes: Optional[int] = None) -> list:
        """One JPEG file per frame.  ``frames``: a list of host arrays of one shape and row stride, or a ``_ffi.DeviceBuffer``
        holding ``count`` frames one after another (frame i at ``offset + i * height * stride``; ``stride`` defaults to
        ``3 * width``; ``count`` defaults to the frames that fit behind ``offset``), read where they are.  ``slot_bytes``: the
        room per file in the first attempt (default: header + ``h * w * 3 / 2``); a file that needs more is encoded again with
        the size the library reported."""
        ptrs, h, w, st, mem, n = _ffi.batch_frames(frames, count if isinstance(frames, _ffi.DeviceBuffer) else None, height=height, width=width,
                                                   stride=stride, offset=offset, writable=False, strict=True)
        if n == 0:
            return []
        if h > self._max[0] or w > self._max[1] or n > self._max[2]:      # a larger frame or batch: a larger handle
            self._max = (max(h, self._max[0]), max(w, self._max[1]), max(n, self._max[2]))
            self.close()
            self._open()
        slot = len(header(self.quality, h, w)) + h * w * 3 // 2 if slot_bytes is None else int(slot_bytes)
        fp = (C.c_void_p * n)(*ptrs)
        try:
            return self._call(fp, n, h, w, st, mem, slot)
        except _ffi.RtmodtError as e:
            if e.code != _ffi.E_CAPACITY or not getattr(e, "needed", 0):
                raise
            return self._call(fp, n, h, w, st, mem, e.needed)

    def _call(self, fp, n, h, w, st, mem, slot) -> list:
        out = np.empty(n * slot, np.uint8)
        sizes = np.zeros(n, np.uint32)
        rc = _ffi.lib().rtmodt_jpeg_encode_batch(self._h, fp, n, h, w, st, mem, _ffi.ptr(out), slot, _ffi.ptr(sizes))
        if rc != _ffi.OK:
            err = _ffi.RtmodtError(rc, _ffi.lib().rtmodt_last_error().decode(errors="replace"))
            err.needed = int(sizes.max()) if rc == _ffi.E_CAPACITY else 0
            err.sizes = sizes
            raise err
        return [out[i * slot:i * slot + int(sizes[i])].tobytes() for i in range(n)]

    def last_kernel_ms(self) -> float:
        """Device time of the last batch's kernels (HIP events)."""
        return _ffi.last_ms("rtmodt_jpeg_last_ms", self._h)

    _destroy = "rtmodt_jpeg_destroy"

    def _open(self) -> None:
        cfg = _ffi.JpegCfg(self.quality, 0, self._max[0], self._max[1], self._max[2])
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_jpeg_create(self._device, C.byref(cfg), C.byref(h)))
        self._h = h


def multipart_chunk(jpeg_bytes: bytes, boundary: bytes = b"frame") -> bytes:
    """One part of a ``multipart/x-mixed-replace; boundary=<boundary>`` body."""
    return (b"--" + boundary + b"\r\nContent-Type: image/jpeg\r\nContent-Length: " + str(len(jpeg_bytes)).encode("ascii") + b"\r\n\r\n"
            + bytes(jpeg_bytes) + b"\r\n")


class MjpegWriter:
    """``cv2.VideoWriter(path, fourcc("MJPG"), fps, frame_size)`` for frames that are already JPEG files: ``write(jpeg_bytes)``,
    ``release()``.  ``*.avi``: RIFF AVI 1.0 (``hdrl`` with ``avih`` and one ``strl`` of ``strh`` / ``strf``, ``movi`` of ``00dc``
    chunks padded to even length, ``idx1``); ``*.mjpeg`` / ``*.mjpg``: the files one after another."""

    _HDRL = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))        # 'hdrl' + avih + LIST strl(strh, strf)
    _MOVI_AT = 12 + 8 + _HDRL                                  # offset of the movi LIST chunk

    def __init__(self, path, fps: float, frame_size) -> None:
        ext = os.path.splitext(str(path))[1].lower()
        if ext not in (".avi", ".mjpeg", ".mjpg"):
            raise ValueError(f"{path}: an MJPEG writer writes .avi, .mjpeg or .mjpg")
        if not fps > 0:
            raise ValueError(f"fps {fps}")
        self.path, self.fps = str(path), float(fps)
        self.width, self.height = int(frame_size[0]), int(frame_size[1])
        self._avi = ext == ".avi"
        self._index = []                                       # (offset from the 'movi' fourcc, length)
        self._max = 0
        self._f = open(self.path, "wb")
        if self._avi:
            self._f.write(self._head())
            self._pos = self._MOVI_AT + 12

    def isOpened(self) -> bool:
        return self._f is not None

    @property
    def frames(self) -> int:
        return len(self._index)

    def write(self, jpeg_bytes) -> None:
        if self._f is None:
            raise ValueError("write after release")
        data = bytes(jpeg_bytes)
        if not self._avi:
            self._f.write(data)
            self._index.append((0, len(data)))
            return
        padded = len(data) + (len(data) & 1)
        if self._pos + 8 + padded + 8 + 16 * (len(self._index) + 1) > AVI_MAX_BYTES:
            raise ValueError(f"{self.path}: frame {len(self._index)} would take the AVI past {AVI_MAX_BYTES} bytes (AVI 1.0, no OpenDML)")
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\x00" * (padded - len(data)))
        self._index.append((self._pos - (self._MOVI_AT + 8), len(data)))
        self._max = max(self._max, len(data))
        self._pos += 8 + padded

    def release(self) -> None:
        if self._f is None:
            return
        if self._avi:
            idx = b"".join(b"00dc" + struct.pack("<III", 0x10, off, ln) for off, ln in self._index)      # AVIIF_KEYFRAME
            self._f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
            self._f.seek(0)
            self._f.write(self._head())
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def _head(self) -> bytes:
        n = len(self._index)
        movi = 4 + sum(8 + ln + (ln & 1) for _, ln in self._index)
        riff = 4 + 8 + self._HDRL + 8 + movi + 8 + 16 * n
        scale, rate = 1000, int(round(self.fps * 1000))
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), int(self._max * self.fps), 0, 0x10, n, 0, 1, self._max, self.width,
                           self.height, 0, 0, 0, 0)                                                 # flags: AVIF_HASINDEX
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, scale, rate, 0, n, self._max, 0xFFFFFFFF, 0,
                                                 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        assert len(avih) == 56 and len(strh) == 56 and len(strf) == 40 and len(hdrl) == self._HDRL
        return (b"RIFF" + struct.pack("<I", riff) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", movi) + b"movi")


class MjpegRecorder:
    """``recorder`` of ``pipeline.run``: every annotated frame is encoded on the GPU and appended to an ``MjpegWriter``."""

    def __init__(self, path, fps: float, encoder: JpegEncoder, frame_size=None) -> None:
        self.path, self.fps, self.encoder, self.writer = path, fps, encoder, None
        self._size = frame_size

    def write(self, frame: np.ndarray) -> None:
        if self.writer is None:
            self.writer = MjpegWriter(self.path, self.fps, self._size or (frame.shape[1], frame.shape[0]))
        self.writer.write(self.encoder.encode(frame))

    def release(self) -> None:
        if self.writer is not None:
            self.writer.release()
