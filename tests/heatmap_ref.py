"""NumPy / plain-loop restatement of the occupancy heatmap: the footprint rule of ``csrc/heatmap_stamp.h`` and the accumulate,
overlay and zone-sum rules in the header of ``csrc/heatmap.hip``.  Everything is integer arithmetic, so the kernels must equal
this exactly.

Grid: ``ceil(h / cell) x ceil(w / cell)`` uint32 cells, cell in {1, 2, 4, 8, 16}, edge cells clipped to the frame.  A box's corners are
``privacy_ref.coord`` of the float32 values (inverted after truncation: no footprint); a class list drops boxes whose class is not
in it.  The candidate pixels are the box's rectangle (BOX, DISC) or the square of radius ``foot_radius`` around the bottom-centre
pixel (FOOT), clipped to the frame (empty: no footprint); the candidate cells are those holding a candidate pixel.  DISC and FOOT
keep the candidates whose doubled centre ``(2 cx cell + cell - 1, 2 cy cell + cell - 1)`` lies within ``d`` of the doubled stamp
centre, plus the cell of the centre pixel if that pixel is in the frame.  ``footprint`` tests EVERY cell of the grid against the
rule (no candidate range is trusted); ``footprint_loop`` does the same in plain Python loops."""
import numpy as np

from privacy_ref import coord
from render_ref import inside_or_on

BOX, DISC, FOOT = "box", "disc", "foot"
U32_MAX = (1 << 32) - 1


def grid_shape(h, w, cell):
    return (-(-h // cell), -(-w // cell))


def _stamp(box, cls, h, w, kind, foot_radius, classes):
    """-> (pixel rectangle x0, y0, x1, y1 clipped, (sx, sy, d) or None, centre pixel or None), or None: no footprint."""
    if classes is not None and int(cls) not in set(int(c) for c in classes):
        return None
    X0, Y0, X1, Y1 = (coord(v) for v in box)
    if X1 < X0 or Y1 < Y0:
        return None
    x0, y0, x1, y1 = X0, Y0, X1, Y1
    disc = centre = None
    if kind == DISC:
        disc = (X0 + X1, Y0 + Y1, min(X1 - X0, Y1 - Y0) + 1)
        centre = ((X0 + X1) // 2, (Y0 + Y1) // 2)                  # floor, also below zero
    elif kind == FOOT:
        r = int(foot_radius)
        centre = ((X0 + X1) // 2, Y1)
        x0, x1, y0, y1 = centre[0] - r, centre[0] + r, Y1 - r, Y1 + r
        disc = (X0 + X1, 2 * Y1, 2 * r + 1)
    elif kind != BOX:
        raise ValueError(kind)
    x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, w - 1); y1 = min(y1, h - 1)
    if x1 < x0 or y1 < y0:
        return None
    if centre is not None and not (0 <= centre[0] < w and 0 <= centre[1] < h):
        centre = None
    return (x0, y0, x1, y1), disc, centre


def footprint(box, cls, h, w, cell, kind=DISC, foot_radius=0, classes=None) -> np.ndarray:
    """One box -> bool (gh, gw): the cells it covers."""
    gh, gw = grid_shape(h, w, cell)
    out = np.zeros((gh, gw), bool)
    st = _stamp(box, cls, h, w, kind, foot_radius, classes)
    if st is None:
        return out
    (x0, y0, x1, y1), disc, centre = st
    cy, cx = np.mgrid[0:gh, 0:gw].astype(np.int64)
    cand = (cx >= x0 // cell) & (cx <= x1 // cell) & (cy >= y0 // cell) & (cy <= y1 // cell)
    if disc is None:
        return cand
    sx, sy, d = disc
    ux = 2 * cx * cell + cell - 1
    uy = 2 * cy * cell + cell - 1
    out = cand & ((ux - sx) ** 2 + (uy - sy) ** 2 <= d * d)
    if centre is not None:
        out[centre[1] // cell, centre[0] // cell] = True
    return out


def footprint_loop(box, cls, h, w, cell, kind=DISC, foot_radius=0, classes=None) -> set:
    """The same as a set of (cx, cy), one cell at a time in Python integers."""
    st = _stamp(box, cls, h, w, kind, foot_radius, classes)
    cells = set()
    if st is None:
        return cells
    (x0, y0, x1, y1), disc, centre = st
    gh, gw = grid_shape(h, w, cell)
    for cy in range(gh):
        for cx in range(gw):
            px0, py0 = cx * cell, cy * cell
            px1, py1 = min(px0 + cell - 1, w - 1), min(py0 + cell - 1, h - 1)
            if px1 < x0 or px0 > x1 or py1 < y0 or py0 > y1:        # the cell holds no candidate pixel
                continue
            if disc is None:
                cells.add((cx, cy))
                continue
            ux, uy = 2 * cx * cell + cell - 1, 2 * cy * cell + cell - 1
            if (ux - disc[0]) ** 2 + (uy - disc[1]) ** 2 <= disc[2] ** 2:
                cells.add((cx, cy))
            elif centre is not None and px0 <= centre[0] <= px1 and py0 <= centre[1] <= py1:
                cells.add((cx, cy))
    return cells


def cells_of(mask) -> list:
    """bool (gh, gw) -> [[cx, cy], ...] row by row (the order of ``rtmodt_heatmap_footprint``)."""
    ys, xs = np.nonzero(mask)
    return [[int(x), int(y)] for x, y in zip(xs, ys)]


def counts(boxes, cls, h, w, cell, **kw) -> np.ndarray:
    """int64 (gh, gw): how many of the frame's footprints cover each cell."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    cls = np.zeros(len(boxes), np.int32) if cls is None else np.asarray(cls, np.int32).reshape(-1)
    out = np.zeros(grid_shape(h, w, cell), np.int64)
    for b, c in zip(boxes, cls):
        out += footprint(b, c, h, w, cell, **kw)
    return out


def decay(grid, shift) -> np.ndarray:
    g = np.asarray(grid, np.uint32).astype(np.int64)
    return (g - (g >> shift)).astype(np.uint32)


def stamp(grid, count, weight=1) -> np.ndarray:
    g = np.asarray(grid, np.uint32).astype(np.int64) + int(weight) * np.asarray(count, np.int64)
    return np.minimum(g, U32_MAX).astype(np.uint32)


class Ref:
    """One stream's grid and the call numbering of a handle: ``accumulate`` is one call."""

    def __init__(self, h, w, cell, kind=DISC, foot_radius=0, weight=1, decay_shift=0, decay_every=1, classes=None):
        self.h, self.w, self.cell = h, w, cell
        self.kw = dict(kind=kind, foot_radius=foot_radius, classes=classes)
        self.weight, self.decay_shift, self.decay_every = weight, decay_shift, decay_every
        self.calls = 0
        self.grid = np.zeros(grid_shape(h, w, cell), np.uint32)

    def accumulate(self, boxes, cls=None) -> np.ndarray:
        self.calls += 1
        if self.decay_shift and self.calls % self.decay_every == 0:
            self.grid = decay(self.grid, self.decay_shift)
        self.grid = stamp(self.grid, counts(boxes, cls, self.h, self.w, self.cell, **self.kw), self.weight)
        return self.grid


def jet_table() -> np.ndarray:
    """(256, 3) uint8, B G R: clamp(max(0, 765 - |8v - 510k|) >> 1, 0, 255), k = 1, 2, 3 for B, G, R."""
    lut = np.zeros((256, 3), np.uint8)
    for v in range(256):
        for c in range(3):
            lut[v, c] = min(max(0, 765 - abs(8 * v - 510 * (c + 1))) >> 1, 255)
    return lut


def levels(grid, m) -> np.ndarray:
    """min(255, (heat * 255 + m // 2) // m) per cell, Python-sized integers via int64 (heat * 255 < 2^40)."""
    g = np.asarray(grid, np.uint32).astype(np.int64)
    return np.minimum(255, (g * 255 + m // 2) // m)


def overlay(frame, grid, cell, alpha=128, min_level=1, scale_max=0, lut=None) -> np.ndarray:
    """The blended copy of ``frame`` (h, w, 3) u8."""
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2]
    m = int(scale_max) if scale_max > 0 else int(np.asarray(grid).max())
    if m == 0:
        return frame.copy()
    lut = jet_table() if lut is None else np.asarray(lut, np.uint8)
    v = levels(grid, m)[np.arange(h)[:, None] // cell, np.arange(w)[None, :] // cell]
    blend = ((frame.astype(np.int64) * (256 - alpha) + lut[v].astype(np.int64) * alpha + 128) >> 8).astype(np.uint8)
    out = frame.copy()
    keep = v >= min_level
    out[keep] = blend[keep]
    return out


def zone_mask(polygon, h, w, cell) -> np.ndarray:
    """bool (gh, gw): the cells whose centre pixel (min(cx cell + cell // 2, w - 1), likewise y) is inside or on the polygon."""
    gh, gw = grid_shape(h, w, cell)
    cy, cx = np.mgrid[0:gh, 0:gw]
    X = np.minimum(cx * cell + cell // 2, w - 1)
    Y = np.minimum(cy * cell + cell // 2, h - 1)
    return inside_or_on(np.asarray(polygon, np.int32).reshape(-1, 2), X, Y)


def zone_sums(grid, polygons, h, w, cell) -> list:
    g = np.asarray(grid, np.uint32)
    return [int(g[zone_mask(p, h, w, cell)].astype(np.uint64).sum(dtype=np.uint64)) if len(p) else 0 for p in polygons]
