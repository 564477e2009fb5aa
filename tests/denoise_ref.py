"""The frame denoiser's rules restated in NumPy: the definition ``csrc/denoise.hip`` and ``csrc/denoise_rule.h`` are pinned to with
``==`` (every rule is integer arithmetic).  PARITY UNPINNED: no camera's 3DNR, ``cv2.fastNlMeansDenoising`` or ffmpeg's ``hqdn3d`` runs
where this is tested, and no default has been validated on real footage.

State per stream: ``acc`` (8.8 fixed point, one per channel and pixel) and ``frames_seen``.  For pixel ``p``: ``x`` the frame's channel
value, ``prev = min(255, (acc + 128) >> 8)``, ``Y(.)`` is ``motion_ref.pixel_luma``.
  1. ``D = |sum over the 3 x 3 neighbourhood of (Y(x_q) - Y(prev_q))|``, neighbour coordinates clamped to the frame (nine terms always).
     ``a = 0`` for ``D <= motion_lo``, ``256`` for ``D >= motion_hi``, else ``(D - motion_lo) * 256 // (motion_hi - motion_lo)``;
     ``frames_seen == 0``: ``a = 256`` everywhere.
  2. Among the up to nine neighbours INSIDE the frame, ``q`` counts when ``|Y(x_q) - Y(x_p)| <= spatial_thr``; per channel
     ``s = (sum + n // 2) // n`` and ``xs = x + (((s - x) * a * spatial + 32768) >> 16)``.
  3. ``wmin = 256 >> temporal_shift``, ``w = wmin + (((256 - wmin) * a + 128) >> 8)``,
     ``acc' = acc + ((((xs << 8) - acc) * w + 128) >> 8)`` (``frames_seen == 0``: ``acc`` counts as ``xs << 8``),
     ``out = min(255, (acc' + 128) >> 8)``.
  4. Per call and stream: ``frames_seen`` after the call (capped at 2^30), ``n_static`` (``a == 0``), ``n_moving`` (``a == 256``) and
     ``absdiff_static``, the sum of ``|Y(x) - Y(prev)|`` over the ``a == 0`` pixels.

The ``defect`` arguments switch in one deliberate mistake each; ``tests/test_denoise_cpu.py`` shows that its literals catch them:
``zero_pad`` (zeros outside the frame in D instead of the clamp), ``sum_abs`` (the sum of absolute values in D), ``no_first`` (the first
frame's ``a`` taken from D), ``no_round`` (every ``+ 128`` missing), ``outside_counts`` (the sigma filter counts clamped neighbours),
``static`` (``a = 0`` always).
"""
import numpy as np

from motion_ref import pixel_luma

MAX_SEEN = 2 ** 30
MAX_ACC = 255 << 8
MAX_THRESHOLD = 9 * 255
DEFAULTS = dict(motion_lo=18, motion_hi=54, temporal_shift=3, spatial=256, spatial_thr=6)
DEFECTS = ("zero_pad", "sum_abs", "no_first", "no_round", "outside_counts", "static")
OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def config(**kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise TypeError(k)
        c[k] = int(v)
    return c


def noise_q8(row):
    return 256 * row["absdiff_static"] // row["n_static"] if row["n_static"] else 0


def prev_of(acc, defect=None):
    return np.minimum(255, (np.asarray(acc, np.int64) + (0 if defect == "no_round" else 128)) >> 8)


def alpha_of(d, c):
    d = np.asarray(d, np.int64)
    mid = (d - c["motion_lo"]) * 256 // (c["motion_hi"] - c["motion_lo"])
    return np.where(d <= c["motion_lo"], 0, np.where(d >= c["motion_hi"], 256, mid))


def _windows(plane, mode):
    """The nine shifted copies of a (h, w, ...) array, in OFFSETS order, the outside by `mode` ("edge": the clamp; "constant": zeros)."""
    pad = [(1, 1), (1, 1)] + [(0, 0)] * (plane.ndim - 2)
    p = np.pad(plane, pad, mode=mode)
    h, w = plane.shape[:2]
    return [p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in OFFSETS]


def frame_step(frame, acc, seen, c, defect=None, detail=None):
    """One frame of one stream, vectorised -> (out uint8 (h, w, 3), acc' int64 (h, w, 3), a int64 (h, w), counts dict); a dict given as
    `detail` receives the intermediate D, xs and w"""
    r = 0 if defect == "no_round" else 128
    x = np.asarray(frame, np.int64)
    acc = np.asarray(acc, np.int64)
    yx, yp = pixel_luma(frame).astype(np.int64), pixel_luma(prev_of(acc, defect).astype(np.uint8)).astype(np.int64)
    diff = yx - yp
    terms = _windows(diff, "constant" if defect == "zero_pad" else "edge")
    d = sum(np.abs(t) for t in terms) if defect == "sum_abs" else np.abs(sum(terms))
    a = alpha_of(d, c)
    if seen == 0 and defect != "no_first":
        a = np.full_like(a, 256)
    if defect == "static":
        a = np.zeros_like(a)
    # the sigma filter
    mode = "edge" if defect == "outside_counts" else "constant"
    inside = _windows(np.ones(yx.shape, bool), mode)
    counts = [i & (np.abs(q - yx) <= c["spatial_thr"]) for i, q in zip(inside, _windows(yx, "edge"))]
    n = sum(k.astype(np.int64) for k in counts)
    total = sum(k[..., None] * q for k, q in zip(counts, _windows(x, "edge")))
    s = (total + (n // 2)[..., None]) // n[..., None]
    xs = x + (((s - x) * (a * c["spatial"])[..., None] + 32768) >> 16)
    # the temporal filter
    wmin = 256 >> c["temporal_shift"]
    w = wmin + (((256 - wmin) * a + r) >> 8)
    base = xs << 8 if seen == 0 else acc
    new = base + ((((xs << 8) - base) * w[..., None] + r) >> 8)
    out = np.minimum(255, (new + r) >> 8)
    if detail is not None:
        detail.update(D=d, xs=xs, w=w)
    counts = dict(n_static=int((a == 0).sum()), n_moving=int((a == 256).sum()), absdiff_static=int(np.abs(diff)[a == 0].sum()))
    return out.astype(np.uint8), new, a, counts


def frame_step_loop(frame, acc, seen, c):
    """The same, one pixel at a time in plain Python: the second statement of the rule."""
    h, w_ = frame.shape[:2]
    luma = lambda b, g, r: (19595 * r + 38470 * g + 7471 * b + 32768) >> 16      # noqa: E731
    prev = [[[min(255, (int(acc[y][x][k]) + 128) >> 8) for k in range(3)] for x in range(w_)] for y in range(h)]
    yx = [[luma(*(int(v) for v in frame[y][x])) for x in range(w_)] for y in range(h)]
    yp = [[luma(*prev[y][x]) for x in range(w_)] for y in range(h)]
    out, new, amap = np.zeros((h, w_, 3), np.uint8), np.zeros((h, w_, 3), np.int64), np.zeros((h, w_), np.int64)
    n_static = n_moving = absdiff = 0
    wmin = 256 >> c["temporal_shift"]
    for y in range(h):
        for x in range(w_):
            d = 0
            for dy, dx in OFFSETS:
                qy, qx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w_ - 1)
                d += yx[qy][qx] - yp[qy][qx]
            d = abs(d)
            if seen == 0 or d >= c["motion_hi"]:
                a = 256
            elif d <= c["motion_lo"]:
                a = 0
            else:
                a = (d - c["motion_lo"]) * 256 // (c["motion_hi"] - c["motion_lo"])
            n, tot = 0, [0, 0, 0]
            for dy, dx in OFFSETS:
                qy, qx = y + dy, x + dx
                if 0 <= qy < h and 0 <= qx < w_ and abs(yx[qy][qx] - yx[y][x]) <= c["spatial_thr"]:
                    n += 1
                    for k in range(3):
                        tot[k] += int(frame[qy][qx][k])
            wt = wmin + (((256 - wmin) * a + 128) >> 8)
            for k in range(3):
                v = int(frame[y][x][k])
                s = (tot[k] + n // 2) // n
                xs = v + (((s - v) * a * c["spatial"] + 32768) >> 16)
                old = xs << 8 if seen == 0 else int(acc[y][x][k])
                nv = old + ((((xs << 8) - old) * wt + 128) >> 8)
                new[y, x, k] = nv
                out[y, x, k] = min(255, (nv + 128) >> 8)
            amap[y, x] = a
            n_static += a == 0
            n_moving += a == 256
            if a == 0:
                absdiff += abs(yx[y][x] - yp[y][x])
    return out, new, amap, dict(n_static=int(n_static), n_moving=int(n_moving), absdiff_static=int(absdiff))


def pixel(cur, acc, inside, seen, c):
    """One pixel from its two 3 x 3 neighbourhoods (``cur`` uint8 (3, 3, 3), ``acc`` (3, 3, 3), already clamped by the caller) and the
    nine flags that say which neighbours lie inside the frame -> (out (3,), acc' (3,), a, D)"""
    cur, acc = np.asarray(cur, np.int64), np.asarray(acc, np.int64)
    yx = pixel_luma(cur.astype(np.uint8)).astype(np.int64)
    yp = pixel_luma(prev_of(acc).astype(np.uint8)).astype(np.int64)
    d = abs(int((yx - yp).sum()))
    a = 256 if seen == 0 else int(alpha_of(d, c))
    k = np.asarray(inside, bool).reshape(3, 3) & (np.abs(yx - yx[1, 1]) <= c["spatial_thr"])
    n = int(k.sum())
    s = ((cur * k[..., None]).sum((0, 1)) + n // 2) // n
    x = cur[1, 1]
    xs = x + (((s - x) * a * c["spatial"] + 32768) >> 16)
    wmin = 256 >> c["temporal_shift"]
    w = wmin + (((256 - wmin) * a + 128) >> 8)
    base = xs << 8 if seen == 0 else acc[1, 1]
    new = base + ((((xs << 8) - base) * w + 128) >> 8)
    return np.minimum(255, (new + 128) >> 8), new, a, d


class Ref:
    """``streams`` restated denoisers for ``height x width`` frames; ``defect`` switches one deliberate mistake in."""

    def __init__(self, streams, height, width, defect=None, **cfg):
        self.streams, self.h, self.w, self.c, self.defect = streams, height, width, config(**cfg), defect
        self.acc = [np.zeros((height, width, 3), np.int64) for _ in range(streams)]
        self.seen = [0] * streams
        self.a = [None] * streams                # the a of every pixel in the stream's last frame
        self.history = []                        # (a, whether it was the stream's first frame) of every step

    def step(self, s, frame, loop=False):
        """-> (out uint8 (h, w, 3), row): the row holds rtmodt_denoise_result's fields"""
        assert frame.shape == (self.h, self.w, 3) and frame.dtype == np.uint8
        if loop:
            out, new, a, counts = frame_step_loop(frame, self.acc[s], self.seen[s], self.c)
        else:
            out, new, a, counts = frame_step(frame, self.acc[s], self.seen[s], self.c, self.defect)
        self.acc[s], self.a[s] = new, a
        self.history.append((a, self.seen[s] == 0))
        self.seen[s] = min(self.seen[s] + 1, MAX_SEEN)
        return out, dict(stream=s, frames_seen=self.seen[s], **counts)

    def state(self, s=0):
        return self.acc[s].astype(np.uint16), self.seen[s]

    def load_state(self, s, state):
        self.acc[s], self.seen[s] = np.asarray(state[0], np.int64).copy(), int(state[1])

    def reset(self, s=None):
        for k in range(self.streams) if s is None else [s]:
            self.acc[k][...] = 0
            self.seen[k] = 0
