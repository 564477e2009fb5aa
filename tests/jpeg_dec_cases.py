"""Files for the JPEG decoder tests (CPU and GPU): frames of a given content, Pillow-written JPEG files of every accepted flavour,
and damaged variants of them."""
import io

import numpy as np
from PIL import Image

import jpeg_dec_ref as D

SUBSAMPLINGS = ["444", "422", "420", "gray"]
MARKERS = {"none": {}, "row": {"restart_marker_rows": 1}, "mcu1": {"restart_marker_blocks": 1}, "mcu3": {"restart_marker_blocks": 3},
           "optimised": {"optimize": True}}


def frame(kind, h, w, seed=0):
    """BGR24 test content: noise (long codes, frequent FF 00), smooth, flat, checker (saturated 3 x 3 cells: the IDCT leaves 0..255 even at quality 100)."""
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx * 3 + yy * 2) % 256], -1).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (10, 200, 90), np.uint8)
    if kind == "checker":
        return np.repeat((((xx // 3 + yy // 3) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    raise ValueError(kind)


def pillow_file(frame_bgr, quality, subsampling, marker="none"):
    """The JPEG file Pillow (libjpeg-turbo) writes for the frame."""
    b = io.BytesIO()
    im = Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1]))
    if subsampling == "gray":
        im.convert("L").save(b, "JPEG", quality=quality, **MARKERS[marker])
    else:
        im.save(b, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[subsampling], **MARKERS[marker])
    return b.getvalue()


def pillow_pixels(file):
    """What libjpeg-turbo decodes: [h, w, 3] BGR or [h, w]."""
    im = np.asarray(Image.open(io.BytesIO(file)))
    return im if im.ndim == 2 else np.ascontiguousarray(im[..., ::-1])


def segments(file):
    """[(marker, offset of the FF, total length with the marker)] of the header segments up to and including SOS."""
    d, i, out = bytes(file), 2, []
    while True:
        m, L = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        out.append((m, i, 2 + L))
        i += 2 + L
        if m == 0xDA:
            return out


def without_segments(file, marker):
    d = bytes(file)
    for m, at, ln in reversed(segments(d)):
        if m == marker:
            d = d[:at] + d[at + ln:]
    return d


def scan_range(file):
    H = D.parse(file)
    return H.scan_off, H.scan_end


def restart_positions(file):
    a, (lo, hi) = np.frombuffer(bytes(file), np.uint8), scan_range(file)
    s = a[lo:hi]
    return (np.nonzero((s[:-1] == 0xFF) & (s[1:] >= 0xD0) & (s[1:] <= 0xD7))[0] + lo).tolist()


def truncated(file, fraction):
    """The file cut inside its scan, `fraction` of the way through."""
    lo, hi = scan_range(file)
    return bytes(file)[:lo + max(1, int((hi - lo) * fraction))]


def flipped(file, rng):
    """One byte of the scan replaced by another value."""
    lo, hi = scan_range(file)
    d = bytearray(file)
    at = int(rng.integers(lo, hi))
    d[at] ^= int(rng.integers(1, 256))
    return bytes(d)


def without_restart(file, k):
    at = restart_positions(file)[k]
    return bytes(file)[:at] + bytes(file)[at + 2:]


def renumbered_restart(file, k):
    d = bytearray(file)
    at = restart_positions(file)[k]
    d[at + 1] = 0xD0 + ((d[at + 1] - 0xD0 + 3) & 7)
    return bytes(d)


def oversubscribed_dht(file):
    """The first DHT's count of 1-bit codes raised to 3: no prefix code."""
    d = bytearray(file)
    at = next(a for m, a, _ in segments(file) if m == 0xC4)
    d[at + 5] = 3
    return bytes(d)
