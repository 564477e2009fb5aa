"""The frame enhancer's rules restated in NumPy: the definition ``csrc/enhance.hip`` and ``csrc/enhance_rule.h`` are pinned to with
``==`` (every rule is integer arithmetic).  PARITY UNPINNED: ``cv2.createCLAHE`` is installed nowhere this runs (its tiles are padded
by reflection and its interpolation is float), and no default has been validated on real footage.

Rules.  ``ty x tx`` tiles; tile column ``k`` covers the pixels ``[k * w // tx, (k + 1) * w // tx)``, rows likewise; a tile's area ``n``
is its own.
  1. ``Y`` per pixel is ``motion_ref.pixel_luma``; a tile's histogram is the 256 counts of the luma of its pixels.
  2. Curve.  ``clip_q8 > 0``: ``clip = max(1, (clip_q8 * n) >> 16)``, ``excess = sum(max(0, hist - clip))``, ``hist = min(hist, clip)``,
     every bin gains ``excess // 256``, and with ``res = excess % 256``, ``step = max(256 // res, 1)``, bin ``i`` gains 1 more exactly
     when ``i % step == 0 and i // step < res``.  ``curve[v] = (cdf[v] * 255 + n // 2) // n`` over the inclusive prefix sum.
  3. State.  ``s`` (8.8 fixed point) per (stream, tile, level), ``frames_seen`` per stream.  ``frames_seen == 0``: ``s = curve << 8``; else
     ``d = (curve << 8) - s`` and ``s += d >> shift`` for ``d >= 0``, ``s -= (-d) >> shift`` otherwise.  ``lut8 = min(255, (s + 128) >> 8)``.
  4. Axis.  ``c2[k] = b[k] + b[k + 1] - 1``; pixel ``x``, ``p = 2 x``: one tile or ``p <= c2[0]`` -> ``(0, 0)``; ``p >= c2[t - 1]`` -> ``(t - 1, 0)``;
     else ``k`` is the last tile with ``c2[k] <= p`` and ``f = ((p - c2[k]) * 256 + den // 2) // den``, ``den = c2[k + 1] - c2[k]``.
  5. ``Y1 = ((256 - fy) * ((256 - fx) * A + fx * B) + fy * ((256 - fx) * C + fx * D) + 32768) >> 16`` over the ``lut8[Y]`` of the tiles
     ``(ky, kx)``, ``(ky, kx + 1)``, ``(ky + 1, kx)``, ``(ky + 1, kx + 1)`` (neighbour: ``min(k + 1, t - 1)``).
  6. ``eff = strength``, or with ``auto_hi > auto_lo`` and ``m = luma_sum // (h * w)``:
     ``strength * clamp(auto_hi - m, 0, auto_hi - auto_lo) // (auto_hi - auto_lo)``.  ``Y2 = Y + (((Y1 - Y) * eff + 128) >> 8)`` (floor).
  7. SHIFT: ``clamp(c + (Y2 - Y))``.  GAIN: ``Y == 0`` -> ``clamp(c + Y2)``, else ``min(255, (c * Y2 + Y // 2) // Y)``.  ``eff == 0`` gives
     ``Y2 == Y`` and so the input bytes under both.

The ``defect`` arguments switch in one deliberate mistake each; ``tests/test_enhance_cpu.py`` shows that its literals catch them.
"""
import numpy as np

from motion_ref import pixel_luma

SHIFT, GAIN = 0, 1
MAX_SEEN = 2 ** 30
DEFAULTS = dict(tiles_y=8, tiles_x=8, clip_q8=512, strength=256, smooth_shift=2, auto_lo=0, auto_hi=0, colour=SHIFT)


def config(**kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise TypeError(k)
        c[k] = int(v)
    return c


# ---- tiles and histograms ---------------------------------------------------------------------------------------------------------
def bounds(px, t):
    return [k * px // t for k in range(t + 1)]


def histograms(frame, ty, tx):
    """-> int64 (ty, tx, 256)"""
    y = pixel_luma(frame)
    h, w = y.shape
    by, bx = bounds(h, ty), bounds(w, tx)
    out = np.zeros((ty, tx, 256), np.int64)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = np.bincount(y[by[j]:by[j + 1], bx[i]:bx[i + 1]].ravel(), minlength=256)
    return out


# ---- the curve of a tile ------------------------------------------------------------------------------------------------------------
def curve(hist, n, clip_q8, defect=None):
    """-> (curve int64[256], excess, cdf int64[256])"""
    hist = np.asarray(hist, np.int64).copy()
    excess = 0
    if clip_q8 > 0:
        clip = max(1, (clip_q8 * n) >> 16)
        excess = int(np.maximum(hist - clip, 0).sum())
        hist = np.minimum(hist, clip) + excess // 256
        res = excess % 256
        if res and defect != "no_residual":
            step = max(256 // res, 1)
            i = np.arange(256)
            hist = hist + ((i % step == 0) & (i // step < res))
    cdf = np.cumsum(hist)
    prod = cdf * 255
    if defect == "cdf32":
        prod = prod & 0xffffffff
    return (prod + n // 2) // n, excess, cdf


# ---- the state ------------------------------------------------------------------------------------------------------------------------
def ema(s, cur, seen, shift, defect=None):
    s, t = np.asarray(s, np.int64), np.asarray(cur, np.int64) << 8
    if seen == 0 and defect != "no_first":
        return t.copy()
    d = t - s
    return s + np.where(d >= 0, d >> shift, -((-d) >> shift))


def lut8(s):
    return np.minimum(255, (np.asarray(s, np.int64) + 128) >> 8)


# ---- where a pixel sits ---------------------------------------------------------------------------------------------------------------
def axis(px, t, defect=None):
    """-> (k int64[px], f int64[px])"""
    b = bounds(px, t)
    c2 = [2 * b[k] for k in range(t)] if defect == "origins" else [b[k] + b[k + 1] - 1 for k in range(t)]
    k_, f_ = np.zeros(px, np.int64), np.zeros(px, np.int64)
    for x in range(px):
        p = 2 * x
        if t == 1 or p <= c2[0]:
            continue
        if p >= c2[t - 1]:
            k_[x] = t - 1
            continue
        k = max(i for i in range(t) if c2[i] <= p)
        den = c2[k + 1] - c2[k]
        k_[x], f_[x] = k, ((p - c2[k]) * 256 + den // 2) // den
    return k_, f_


# ---- a frame ---------------------------------------------------------------------------------------------------------------------------
def eff_of(c, luma_sum, pixels):
    if c["auto_hi"] <= c["auto_lo"]:
        return c["strength"]
    m, span = luma_sum // pixels, c["auto_hi"] - c["auto_lo"]
    return c["strength"] * min(max(c["auto_hi"] - m, 0), span) // span


def interpolate(y, lut, ty, tx, defect=None):
    """Y1 of every pixel: y int64 (h, w), lut int64 (ty, tx, 256)"""
    h, w = y.shape
    (ky, fy), (kx, fx) = axis(h, ty, defect), axis(w, tx, defect)
    ky, fy, kx, fx = ky[:, None], fy[:, None], kx[None, :], fx[None, :]
    ky1, kx1 = np.minimum(ky + 1, ty - 1), np.minimum(kx + 1, tx - 1)
    a, b, c, d = lut[ky, kx, y], lut[ky, kx1, y], lut[ky1, kx, y], lut[ky1, kx1, y]
    return ((256 - fy) * ((256 - fx) * a + fx * b) + fy * ((256 - fx) * c + fx * d) + 32768) >> 16


def y2_of(y, y1, eff):
    return y + (((y1 - y) * eff + 128) >> 8)


def colour_of(frame, y, y2, colour):
    f = np.asarray(frame).astype(np.int64)
    y, y2 = y[..., None], y2[..., None]
    if colour == SHIFT:
        out = f + (y2 - y)
    else:
        out = np.where(y == 0, f + y2, (f * y2 + y // 2) // np.maximum(y, 1))
    return np.clip(out, 0, 255).astype(np.uint8)


def apply(frame, lut, c, eff, defect=None):
    y = pixel_luma(frame)
    return colour_of(frame, y, y2_of(y, interpolate(y, lut, c["tiles_y"], c["tiles_x"], defect), eff), c["colour"])


class Ref:
    """What a ``FrameEnhancer(streams, height, width, ...)`` holds and answers."""

    def __init__(self, streams, height, width, defect=None, **cfg):
        self.c = config(**cfg)
        self.streams, self.h, self.w, self.defect = streams, height, width, defect
        ty, tx = self.c["tiles_y"], self.c["tiles_x"]
        by, bx = bounds(height, ty), bounds(width, tx)
        self.area = np.array([[(by[j + 1] - by[j]) * (bx[i + 1] - bx[i]) for i in range(tx)] for j in range(ty)], np.int64)
        self.s = np.zeros((streams, ty, tx, 256), np.int64)
        self.seen = [0] * streams
        self.hist = np.zeros((streams, ty, tx, 256), np.int64)

    def step(self, s, frame):
        """-> (the enhanced frame, the result row)"""
        c = self.c
        ty, tx = c["tiles_y"], c["tiles_x"]
        hist = histograms(frame, ty, tx)
        clipped = 0
        for j in range(ty):
            for i in range(tx):
                cur, ex, _ = curve(hist[j, i], int(self.area[j, i]), c["clip_q8"], self.defect)
                clipped += ex
                self.s[s, j, i] = ema(self.s[s, j, i], cur, self.seen[s], c["smooth_shift"], self.defect)
        luma_sum = int((hist * np.arange(256)).sum())
        eff = eff_of(c, luma_sum, self.h * self.w)
        out = apply(frame, lut8(self.s[s]), c, eff, self.defect)
        self.seen[s] = min(self.seen[s] + 1, MAX_SEEN)
        self.hist[s] = hist
        return out, dict(stream=s, frames_seen=self.seen[s], luma_sum=luma_sum, eff=eff, clipped=clipped)

    def state(self, s):
        return self.s[s].astype(np.uint16), self.seen[s]

    def load_state(self, s, state):
        self.s[s], self.seen[s] = np.asarray(state[0], np.int64), int(state[1])

    def reset(self, s=None):
        for k in (range(self.streams) if s is None else [s]):
            self.s[k] = 0
            self.seen[k] = 0
