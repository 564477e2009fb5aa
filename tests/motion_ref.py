"""The motion detector's rules restated in NumPy: the definition ``csrc/motion.hip`` and ``csrc/motion_model.h`` are pinned to with
``==`` (every rule is integer arithmetic).  PARITY UNPINNED: OpenCV's ``BackgroundSubtractorMOG2`` and Frigate are installed nowhere
this runs, and no default has been validated on real footage.

Each step has a vectorised form (what the GPU tests compare with) and a plain loop form (``*_loop``, a flood fill for the
labelling) that ``tests/test_motion_cpu.py`` checks the vectorised form against.

Rules.  Grid ``gw = ceil(W / scale)``, ``gh = ceil(H / scale)``.
  1. ``Y = (19595 R + 38470 G + 7471 B + 32768) >> 16`` per pixel; ``Yc = (sum + cnt // 2) // cnt`` over a cell's pixels inside the frame.
  2. ``frames_seen == 0``: ``bg = Yc << 8``, ``dev = 0``, nothing raw.  Else ``d = (Yc << 8) - bg``, ``ad = |d|``,
     ``raw = frames_seen >= warmup and ad > (threshold << 8) + dev_gain * dev``; ``bg += d >> s`` (arithmetic), ``s = learn_shift_fg``
     for raw cells (0: no update) else ``learn_shift``; ``dev += (ad - dev) >> learn_shift`` for cells that are not raw.
  3. ``n3`` = raw cells in the 3 x 3 neighbourhood (itself included, outside counts 0); ``kept = raw and n3 >= min_neighbors``;
     ``mask`` = a kept cell within Chebyshev distance ``dilate``.
  4. ``n_raw``, ``n_fg``, ``luma_sum``, the mask's pixel box (x1 / y1 exclusive, clipped; zeros when empty), the block grid.
  5. Regions: 8-connected components of ``mask`` with ``>= min_area`` cells in the raster order of their first cell, as
     ``(x0, y0, x1, y1, area)``; the first ``max_regions`` are stored, ``n_regions_total`` counts all.
  6. ``WARMUP`` if ``frames_seen < warmup`` at entry, else ``SCENE_CHANGE`` if ``1000 * n_raw >= scene_pm * gw * gh``, else ``MOTION``
     with a region, else ``STILL``; ``frames_seen`` becomes 0 after a ``SCENE_CHANGE``, else ``min(frames_seen + 1, 2 ** 30)``.
"""
from collections import deque

import numpy as np

WARMUP, STILL, MOTION, SCENE_CHANGE = 0, 1, 2, 3
MAX_SEEN = 2 ** 30
DEFAULTS = dict(scale=4, learn_shift=4, learn_shift_fg=8, threshold=12, dev_gain=2, min_neighbors=3, dilate=1, warmup=8, scene_pm=600, min_area=4,
                max_regions=32, block=16)


def config(**kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise TypeError(k)
        c[k] = int(v)
    return c


def grid_shape(h, w, scale):
    return -(-h // scale), -(-w // scale)


# ---- 1. cell luma ------------------------------------------------------------------------------------------------------
def pixel_luma(frame):
    f = np.asarray(frame).astype(np.int64)
    return (19595 * f[..., 2] + 38470 * f[..., 1] + 7471 * f[..., 0] + 32768) >> 16


def cell_luma(frame, scale):
    y = pixel_luma(frame)
    h, w = y.shape
    gh, gw = grid_shape(h, w, scale)
    pad = np.zeros((gh * scale, gw * scale), np.int64)
    cnt = np.zeros_like(pad)
    pad[:h, :w] = y
    cnt[:h, :w] = 1
    s = pad.reshape(gh, scale, gw, scale).sum((1, 3))
    c = cnt.reshape(gh, scale, gw, scale).sum((1, 3))
    return (s + c // 2) // c


def cell_luma_loop(frame, scale):
    h, w = frame.shape[:2]
    gh, gw = grid_shape(h, w, scale)
    out = np.zeros((gh, gw), np.int64)
    for cy in range(gh):
        for cx in range(gw):
            s = cnt = 0
            for y in range(cy * scale, min(cy * scale + scale, h)):
                for x in range(cx * scale, min(cx * scale + scale, w)):
                    b, g, r = (int(v) for v in frame[y, x])
                    s += (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
                    cnt += 1
            out[cy, cx] = (s + cnt // 2) // cnt
    return out


# ---- 2. model ----------------------------------------------------------------------------------------------------------
def update(yc, bg, dev, seen, c):
    """-> (raw bool, bg, dev) as new int64 arrays."""
    yc, bg, dev = np.asarray(yc, np.int64), np.asarray(bg, np.int64), np.asarray(dev, np.int64)
    t = yc << 8
    if seen == 0:
        return np.zeros(yc.shape, bool), t.copy(), np.zeros_like(t)
    d = t - bg
    ad = np.abs(d)
    raw = (ad > (c["threshold"] << 8) + c["dev_gain"] * dev) if seen >= c["warmup"] else np.zeros(yc.shape, bool)
    fg = bg + (d >> c["learn_shift_fg"]) if c["learn_shift_fg"] else bg
    return raw, np.where(raw, fg, bg + (d >> c["learn_shift"])), np.where(raw, dev, dev + ((ad - dev) >> c["learn_shift"]))


def cell_loop(yc, bg, dev, seen, c):
    """One cell in plain Python integers -> (raw, bg, dev).  ``>>`` of a negative Python int floors, as an arithmetic shift does."""
    yc, bg, dev = int(yc), int(bg), int(dev)
    t = yc * 256
    if seen == 0:
        return False, t, 0
    d = t - bg
    ad = -d if d < 0 else d
    raw = seen >= c["warmup"] and ad > c["threshold"] * 256 + c["dev_gain"] * dev
    if not raw:
        return False, bg + (d >> c["learn_shift"]), dev + ((ad - dev) >> c["learn_shift"])
    if c["learn_shift_fg"]:
        bg += d >> c["learn_shift_fg"]
    return True, bg, dev


# ---- 3. mask -----------------------------------------------------------------------------------------------------------
def _window_sum(a, r):
    gh, gw = a.shape
    p = np.zeros((gh + 2 * r, gw + 2 * r), np.int64)
    p[r:r + gh, r:r + gw] = a
    out = np.zeros((gh, gw), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += p[dy:dy + gh, dx:dx + gw]
    return out


def mask_of(raw, min_neighbors, dilate):
    raw = np.asarray(raw).astype(np.int64)
    kept = (raw > 0) & (_window_sum(raw, 1) >= min_neighbors)
    return (_window_sum(kept, dilate) > 0).astype(np.uint8)


def mask_loop(raw, min_neighbors, dilate):
    raw = np.asarray(raw)
    gh, gw = raw.shape

    def at(a, y, x):
        return bool(a[y, x]) if 0 <= y < gh and 0 <= x < gw else False
    kept = np.zeros((gh, gw), bool)
    for y in range(gh):
        for x in range(gw):
            n3 = sum(at(raw, y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
            kept[y, x] = bool(raw[y, x]) and n3 >= min_neighbors
    out = np.zeros((gh, gw), np.uint8)
    for y in range(gh):
        for x in range(gw):
            out[y, x] = any(at(kept, y + dy, x + dx) for dy in range(-dilate, dilate + 1) for dx in range(-dilate, dilate + 1))
    return out


# ---- 4. counts ---------------------------------------------------------------------------------------------------------
def px_box(cx0, cy0, cx1, cy1, scale, h, w):
    return (cx0 * scale, cy0 * scale, min(w, (cx1 + 1) * scale), min(h, (cy1 + 1) * scale))


def mask_box(mask, scale, h, w):
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return (0, 0, 0, 0)
    return px_box(int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), scale, h, w)


def block_grid(mask, block):
    gh, gw = mask.shape
    bh, bw = -(-gh // block), -(-gw // block)
    p = np.zeros((bh * block, bw * block), np.int64)
    p[:gh, :gw] = mask
    return p.reshape(bh, block, bw, block).sum((1, 3)).astype(np.uint32)


# ---- 5. regions --------------------------------------------------------------------------------------------------------
def components(mask):
    """8-connected components by runs and union-find -> a list of (first cell index, area, cx0, cy0, cx1, cy1), in the raster
    order of the first cell."""
    mask = np.asarray(mask) != 0
    gh, gw = mask.shape
    parent = []
    stats = []                                               # per run: first index, area, x0, y0, x1, y1

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    prev = []                                                # (x0, x1, run id) of the row above
    for y in range(gh):
        row = mask[y]
        edges = np.flatnonzero(np.diff(np.concatenate(([0], row.astype(np.int8), [0]))))
        cur = []
        j = 0                                                # the first run above that does not end left of this one
        for x0, x1 in zip(edges[::2].tolist(), (edges[1::2] - 1).tolist()):
            rid = len(parent)
            parent.append(rid)
            stats.append([y * gw + x0, x1 - x0 + 1, x0, y, x1, y])
            while j < len(prev) and prev[j][1] < x0 - 1:
                j += 1
            k = j
            while k < len(prev) and prev[k][0] <= x1 + 1:    # 8-connectivity: the runs overlap once one is widened by a cell
                a, b = find(prev[k][2]), find(rid)
                if a != b:
                    parent[max(a, b)] = min(a, b)
                k += 1
            cur.append((x0, x1, rid))
        prev = cur
    out = {}
    for rid, st in enumerate(stats):
        r = find(rid)
        if r not in out:
            out[r] = list(st)
        else:
            o = out[r]
            o[0] = min(o[0], st[0]); o[1] += st[1]
            o[2] = min(o[2], st[2]); o[3] = min(o[3], st[3]); o[4] = max(o[4], st[4]); o[5] = max(o[5], st[5])
    return sorted((tuple(v) for v in out.values()), key=lambda v: v[0])


def components_flood(mask):
    """The same by a flood fill from every unvisited mask cell in raster order."""
    mask = np.asarray(mask) != 0
    gh, gw = mask.shape
    seen = np.zeros((gh, gw), bool)
    out = []
    for y in range(gh):
        for x in range(gw):
            if not mask[y, x] or seen[y, x]:
                continue
            q = deque([(y, x)])
            seen[y, x] = True
            area, x0, y0, x1, y1 = 0, x, y, x, y
            while q:
                cy, cx = q.popleft()
                area += 1
                x0, y0, x1, y1 = min(x0, cx), min(y0, cy), max(x1, cx), max(y1, cy)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ny, nx = cy + dy, cx + dx
                        if 0 <= ny < gh and 0 <= nx < gw and mask[ny, nx] and not seen[ny, nx]:
                            seen[ny, nx] = True
                            q.append((ny, nx))
            out.append((y * gw + x, area, x0, y0, x1, y1))
    return out


def regions_of(mask, min_area, max_regions, scale, h, w, comps=None):
    """-> (the stored regions [(x0, y0, x1, y1, area)], n_regions_total)."""
    comps = components(mask) if comps is None else comps
    big = [c for c in comps if c[1] >= min_area]
    return [px_box(c[2], c[3], c[4], c[5], scale, h, w) + (c[1],) for c in big[:max_regions]], len(big)


# ---- 6. status ---------------------------------------------------------------------------------------------------------
def status_of(seen, n_raw, cells, n_regions_total, c):
    if seen < c["warmup"]:
        return WARMUP
    if 1000 * n_raw >= c["scene_pm"] * cells:
        return SCENE_CHANGE
    return MOTION if n_regions_total >= 1 else STILL


def next_seen(seen, status):
    return 0 if status == SCENE_CHANGE else min(seen + 1, MAX_SEEN)


class Ref:
    """What a ``MotionDetector(streams, height, width, **cfg)`` holds and answers."""

    def __init__(self, streams, height, width, **cfg):
        self.c = config(**cfg)
        self.streams, self.h, self.w = streams, height, width
        self.gh, self.gw = grid_shape(height, width, self.c["scale"])
        self.bg = np.zeros((streams, self.gh, self.gw), np.int64)
        self.dev = np.zeros_like(self.bg)
        self.seen = [0] * streams
        self.masks = np.zeros((streams, self.gh, self.gw), np.uint8)
        b = self.c["block"]
        self.block_grids = np.zeros((streams, -(-self.gh // b), -(-self.gw // b)), np.uint32)

    def step(self, s, frame):
        c = self.c
        yc = cell_luma(frame, c["scale"])
        raw, self.bg[s], self.dev[s] = update(yc, self.bg[s], self.dev[s], self.seen[s], c)
        mask = mask_of(raw, c["min_neighbors"], c["dilate"])
        regions, total = regions_of(mask, c["min_area"], c["max_regions"], c["scale"], self.h, self.w)
        n_raw = int(raw.sum())
        status = status_of(self.seen[s], n_raw, self.gh * self.gw, total, c)
        self.seen[s] = next_seen(self.seen[s], status)
        self.masks[s] = mask
        self.block_grids[s] = block_grid(mask, c["block"])
        return dict(stream=s, status=status, n_raw=n_raw, n_fg=int(mask.sum()), luma_sum=int(yc.sum()), bbox=mask_box(mask, c["scale"], self.h, self.w),
                    regions=regions, n_regions_total=total, frames_seen=self.seen[s])

    def process(self, frames, streams=None):
        streams = range(self.streams) if streams is None else streams
        return [self.step(s, f) for s, f in zip(streams, frames)]

    def state(self, s):
        return self.bg[s].astype(np.uint16), self.dev[s].astype(np.uint16), self.seen[s]

    def load_state(self, bg, dev, seen, s=0):
        self.bg[s], self.dev[s], self.seen[s] = np.asarray(bg, np.int64), np.asarray(dev, np.int64), int(seen)

    def reset(self, s=None):
        for k in (range(self.streams) if s is None else [s]):
            self.bg[k] = 0; self.dev[k] = 0; self.seen[k] = 0; self.masks[k] = 0; self.block_grids[k] = 0
