"""Motion-JPEG capture back-end: ``cv2.VideoCapture`` on an MJPEG file or camera stream (``src/ingestion/rtsp_reader.py``) without
OpenCV.  ``MjpegCapture`` reads the three framings ``visualization.MjpegWriter`` / ``multipart_chunk`` write -- a RIFF AVI with an
``MJPG`` stream (``00dc`` chunks), a bare ``.mjpeg`` concatenation, and a ``multipart/x-mixed-replace`` body -- from a file, FIFO or
``-`` (stdin), front to back and without seeking, so a camera's HTTP body piped in works like a file.  Frames are split on the
host by the container's own structure (chunk sizes, ``Content-Length``, JPEG segment lengths up to SOS and then the EOI marker, which
entropy-coded data cannot contain); no pixel is touched on the host.  ``retrieve`` decodes the grabbed frame with
``JpegDecoder`` (``csrc/jpeg_dec.hip``) straight into the array it is handed -- ``FrameReader("x.avi", backend="mjpeg", ring=...)``
decodes into the page-locked ring.
"""
from __future__ import annotations

import struct
import sys
from typing import Optional, Tuple

import numpy as np

from .. import _ffi
from .jpeg_decode import JpegDecoder, probe

_CHUNK = 1 << 16


class _Stream:
    """Buffered front-to-back reads over an unseekable file object."""

    def __init__(self, f):
        self.f, self.buf, self.eof = f, bytearray(), False

    def fill(self, n: int) -> bool:
        """At least n bytes in the buffer?"""
        while len(self.buf) < n and not self.eof:
            want = max(_CHUNK, n - len(self.buf))
            got = self.f.read1(want) if hasattr(self.f, "read1") else self.f.read(want)       # whatever has arrived: a FIFO must not stall a frame
            if not got:
                self.eof = True
            else:
                self.buf += got
        return len(self.buf) >= n

    def take(self, n: int) -> Optional[bytes]:
        if not self.fill(n):
            return None
        out = bytes(self.buf[:n])
        del self.buf[:n]
        return out

    def find(self, needle: bytes, start: int) -> int:
        """Offset of needle at or after start, reading on as needed; -1 at the end of the stream."""
        while True:
            at = self.buf.find(needle, start)
            if at >= 0:
                return at
            start = max(start, len(self.buf) - len(needle) + 1)
            if not self.fill(len(self.buf) + 1):
                return -1


class MjpegCapture:
    """``opened / grab() / retrieve(out=None) / release()`` over an MJPEG source; ``jpeg`` is the file of the frame last grabbed.
    ``framing``: ``"avi"``, ``"mjpeg"``, ``"multipart"`` or ``None`` (told from the first bytes).  ``decoder``: a ``JpegDecoder`` to
    share; by default one is made at the first ``retrieve``."""

    def __init__(self, source: str, resolution: Optional[Tuple[int, int]] = None, framing: Optional[str] = None, decoder: Optional[JpegDecoder] = None,
                 device=0, **_):
        try:
            f = sys.stdin.buffer if source == "-" else open(source, "rb", buffering=0)
        except OSError as e:
            raise ConnectionError(f"Cannot open stream: {source}") from e
        self._owns = source != "-"
        self._s = _Stream(f)
        self._device, self._dec, self._own_dec = device, decoder, decoder is None
        self.resolution = resolution
        self.jpeg: Optional[bytes] = None
        self.frames = 0
        self.opened = True
        if framing not in (None, "avi", "mjpeg", "multipart"):
            self.release()
            raise ValueError(f"unknown MJPEG framing {framing!r}")
        self.framing = framing                                 # None: told from the first bytes, at the first grab (opening never waits for data)
        self._movi_left = -1                                   # bytes of the movi list still ahead; -1: not inside it yet

    # ---- the capture protocol ----
    def grab(self) -> bool:
        if not self.opened:
            return False
        if self.framing is None:
            self._s.fill(4)
            head = bytes(self._s.buf[:4])
            self.framing = "avi" if head == b"RIFF" else "multipart" if head[:2] == b"--" else "mjpeg"
        data = {"avi": self._next_avi, "mjpeg": self._next_concatenated, "multipart": self._next_part}[self.framing]()
        if data is None:
            return False
        self.jpeg = data
        self.frames += 1
        return True

    def retrieve(self, out: Optional[np.ndarray] = None):
        if self.jpeg is None:
            return False, None
        if self._dec is None:
            info = probe(self.jpeg)
            w, h = self.resolution or (info.w, info.h)
            self._dec = JpegDecoder(device=self._device, max_height=max(int(h), 1), max_width=max(int(w), 1), max_batch=1,
                                    max_file_bytes=max(len(self.jpeg) * 2, 1 << 16))
        if out is None:
            if self.resolution:
                out = np.zeros((self.resolution[1], self.resolution[0], 3), np.uint8)
            else:
                info = probe(self.jpeg)
                if info.status != _ffi.JPEG_OK:
                    return False, None
                out = np.zeros((info.h, info.w, 3), np.uint8)
        _, status = self._dec.decode_batch([self.jpeg], out=out[None])
        return (True, out) if status[0] == _ffi.JPEG_OK else (False, None)

    def release(self) -> None:
        if self.opened and self._owns:
            self._s.f.close()
        if self._own_dec and self._dec is not None:
            self._dec.close()
            self._dec = None
        self.opened = False

    # ---- framings ----
    def _next_concatenated(self) -> Optional[bytes]:
        s = self._s
        at = s.find(b"\xff\xd8", 0)                            # (bytes between files are skipped)
        if at < 0:
            return None
        del s.buf[:at]
        i = 2
        while True:                                            # header segments by their lengths, up to and including SOS
            if not s.fill(i + 4):
                return None
            if s.buf[i] != 0xFF:
                return None
            m = s.buf[i + 1]
            if m == 0xFF:                                      # fill byte
                i += 1
                continue
            if m == 0xD9 or m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
                return None
            i += 2 + (s.buf[i + 2] << 8 | s.buf[i + 3])
            if m == 0xDA:
                break
        end = s.find(b"\xff\xd9", i)                           # entropy-coded data holds FF only as FF 00 / FF D0..D7
        return s.take(end + 2) if end >= 0 else None

    def _next_avi(self) -> Optional[bytes]:
        s = self._s
        if self._movi_left < 0:
            head = s.take(12)
            if head is None or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
                return None
            while True:                                        # top-level chunks up to the movi list
                ch = s.take(8)
                if ch is None:
                    return None
                size = struct.unpack("<I", ch[4:8])[0]
                if ch[:4] == b"LIST":
                    kind = s.take(4)
                    if kind is None:
                        return None
                    if kind == b"movi":
                        self._movi_left = size - 4
                        break
                    size -= 4
                if s.take(size + (size & 1)) is None:
                    return None
        while self._movi_left >= 8:
            ch = s.take(8)
            if ch is None:
                return None
            size = struct.unpack("<I", ch[4:8])[0]
            padded = size + (size & 1)
            self._movi_left -= 8 + padded
            if ch[:4] == b"LIST":                              # a 'rec ' list: its chunks follow in line
                if s.take(4) is None:
                    return None
                self._movi_left += padded - 4
                continue
            data = s.take(padded)
            if data is None:
                return None
            if ch[2:4] in (b"dc", b"db") and size:
                return data[:size]
        return None

    def _next_part(self) -> Optional[bytes]:
        s = self._s
        while True:
            eol = s.find(b"\r\n", 0)
            if eol < 0:
                return None
            line = s.take(eol + 2)[:-2]
            if line.startswith(b"--"):
                if line.endswith(b"--") and len(line) > 4:     # the closing boundary
                    return None
                break
        length = None
        while True:
            eol = s.find(b"\r\n", 0)
            if eol < 0:
                return None
            line = s.take(eol + 2)[:-2]
            if not line:
                break
            name, _, value = line.partition(b":")
            if name.strip().lower() == b"content-length":
                try:
                    length = int(value.strip())
                except ValueError:
                    return None
        if length is None or length < 0:
            return None
        return s.take(length)
