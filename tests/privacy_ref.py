"""NumPy restatement of the privacy masker: the region arithmetic of ``csrc/privacy_regions.h`` and the paint rules in the
header of ``csrc/privacy.hip``.  Everything is integer arithmetic, so the kernels must equal this byte for byte.

A box becomes an inclusive rectangle: corners ``int(v)`` of the float32 value clamped to +-2^20 (inverted after truncation: no
region); HEAD keeps the top ``max(1, (H * head_pm + 999) // 1000)`` rows; ``expand_px`` on all four sides; clipped to the frame
(empty: no region); a class list drops boxes whose class is not in it.  A pixel is masked when it lies in a rectangle or inside
or on a privacy polygon (``render_ref.inside_or_on``, the zone engine's rule).  Masked pixels become the fill colour, their
cell's rounded mean (grid anchored at the origin, edge cells clipped, all in-frame pixels count), or the last of ``passes`` box
filters ``(sum + n // 2) // n`` over the window clipped to the frame, each pass a whole u8 image.  Unmasked pixels are not
touched; every output is a function of the frame before the call."""
import numpy as np

from render_ref import inside_or_on

COORD_MAX = 1 << 20
BOX, HEAD = "box", "head"


def coord(v) -> int:
    f = float(np.float32(v))
    if f != f or f in (float("inf"), float("-inf")):
        raise ValueError("non-finite coordinate")
    return int(max(-COORD_MAX, min(COORD_MAX, f)))                 # int(): truncation toward zero


def head_rows(H: int, head_pm: int) -> int:
    return max(1, (H * head_pm + 999) // 1000)


def region(box, cls, h, w, kind=BOX, head_pm=300, expand_px=0, classes=None):
    """One box -> (x0, y0, x1, y1) inclusive, or None."""
    if classes is not None and int(cls) not in set(int(c) for c in classes):
        return None
    x0, y0, x1, y1 = (coord(v) for v in box)
    if x1 < x0 or y1 < y0:
        return None
    if kind == HEAD:
        y1 = y0 + head_rows(y1 - y0 + 1, head_pm) - 1
    x0 -= expand_px; y0 -= expand_px; x1 += expand_px; y1 += expand_px
    x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, w - 1); y1 = min(y1, h - 1)
    if x1 < x0 or y1 < y0:
        return None
    return (x0, y0, x1, y1)


def regions(boxes, cls, h, w, **kw) -> np.ndarray:
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    cls = np.zeros(len(boxes), np.int32) if cls is None else np.asarray(cls, np.int32).reshape(-1)
    out = [r for r in (region(b, c, h, w, **kw) for b, c in zip(boxes, cls)) if r is not None]
    return np.asarray(out, np.int32).reshape(-1, 4)


def mask_of(rects, polygons, h, w) -> np.ndarray:
    m = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in np.asarray(rects, np.int64).reshape(-1, 4):
        m[y0:y1 + 1, x0:x1 + 1] = True
    if polygons:
        Y, X = np.mgrid[0:h, 0:w]
        for p in polygons:
            m |= inside_or_on(p, X, Y)
    return m


def pixelate_image(img, cell) -> np.ndarray:
    """Every pixel's cell mean (masked or not)."""
    h, w = img.shape[:2]
    out = np.empty_like(img)
    for y0 in range(0, h, cell):
        for x0 in range(0, w, cell):
            blk = img[y0:y0 + cell, x0:x0 + cell].astype(np.int64)
            n = blk.shape[0] * blk.shape[1]
            out[y0:y0 + cell, x0:x0 + cell] = ((blk.sum(axis=(0, 1)) + n // 2) // n).astype(np.uint8)
    return out


def blur_pass(img, r) -> np.ndarray:
    """One pass over a (h, w, C) u8 image through a summed-area table."""
    h, w = img.shape[:2]
    S = np.zeros((h + 1, w + 1) + img.shape[2:], np.int64)
    S[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    ya = np.maximum(np.arange(h) - r, 0); yb = np.minimum(np.arange(h) + r, h - 1) + 1
    xa = np.maximum(np.arange(w) - r, 0); xb = np.minimum(np.arange(w) + r, w - 1) + 1
    tot = S[yb][:, xb] - S[ya][:, xb] - S[yb][:, xa] + S[ya][:, xa]
    n = ((yb - ya)[:, None] * (xb - xa)[None, :]).astype(np.int64)
    n = n.reshape(n.shape + (1,) * (img.ndim - 2))
    return ((tot + n // 2) // n).astype(np.uint8)


def blur_pass_naive(img, r) -> np.ndarray:
    h, w = img.shape[:2]
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            win = img[max(y - r, 0):min(y + r, h - 1) + 1, max(x - r, 0):min(x + r, w - 1) + 1].astype(np.int64)
            n = win.shape[0] * win.shape[1]
            out[y, x] = (win.sum(axis=(0, 1)) + n // 2) // n
    return out


def blur_image(img, radius, passes, one_pass=blur_pass) -> np.ndarray:
    for _ in range(passes):
        img = one_pass(img, radius)
    return img


def apply(frame, boxes, cls=None, *, mode="pixelate", cell=16, radius=8, passes=2, color=(0, 0, 0), polygons=None, kind=BOX,
          head_pm=300, expand_px=0, classes=None) -> np.ndarray:
    """The masked copy of ``frame`` (h, w, 3) u8."""
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2]
    m = mask_of(regions(boxes, cls, h, w, kind=kind, head_pm=head_pm, expand_px=expand_px, classes=classes), polygons, h, w)
    if mode == "fill":
        src = np.empty_like(frame)
        src[:] = np.asarray(color, np.uint8)
    elif mode == "pixelate":
        src = pixelate_image(frame, cell)
    elif mode == "blur":
        src = blur_image(frame, radius, passes)
    else:
        raise ValueError(mode)
    out = frame.copy()
    out[m] = src[m]
    return out
