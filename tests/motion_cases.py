"""Deterministic scenes for the motion detector's tests (tests/test_motion_cpu.py, tests/test_gpu_motion.py)."""
import numpy as np

#: the 40-frame sequence: warm-up, still, a bright rectangle moving for RECT_FRAMES frames from RECT_FIRST, still, a global step at STEP_AT
N_FRAMES, RECT_FIRST, RECT_FRAMES, STEP_AT, STEP = 40, 12, 12, 30, 60


def background(h, w):
    """A smooth BGR background, 60..130 per channel."""
    y, x = np.mgrid[0:h, 0:w]
    g = 60 + x * 40 // max(w, 1) + y * 30 // max(h, 1)
    return np.stack([g, g + 3, g - 5], -1).astype(np.int64)


def rect_at(h, w, k):
    """The rectangle's pixel box (x0, y0, x1, y1), exclusive, on frame RECT_FIRST + k."""
    rh, rw = max(6, h * 3 // 10), max(6, w // 10)
    x0, y0 = w // 10 + k * max(1, w // 30), h // 4
    return x0, y0, min(w, x0 + rw), min(h, y0 + rh)


def sequence(h, w, seed, n=N_FRAMES):
    """``n`` frames (h, w, 3) uint8: noise of +-3 on the smooth background, the rectangle, then the global +STEP."""
    rng = np.random.default_rng(seed)
    bgd = background(h, w)
    out = []
    for f in range(n):
        fr = bgd + rng.integers(-3, 4, (h, w, 3))
        if RECT_FIRST <= f < RECT_FIRST + RECT_FRAMES:
            x0, y0, x1, y1 = rect_at(h, w, f - RECT_FIRST)
            fr[y0:y1, x0:x1] = 220 + rng.integers(-3, 4, (y1 - y0, x1 - x0, 3))
        if f >= STEP_AT:
            fr = fr + STEP
        out.append(np.clip(fr, 0, 255).astype(np.uint8))
    return out


def cells_to_frame(cells, scale, h, w):
    """A grey frame whose cell (cx, cy) has luma cells[cy, cx] exactly (B = G = R = v gives Y = v)."""
    px = np.kron(np.asarray(cells, np.uint8), np.ones((scale, scale), np.uint8))[:h, :w]
    return np.ascontiguousarray(np.repeat(px[:, :, None], 3, 2))


def speckle(gh, gw, rng, frac=0.12, base=100, lift=80):
    """Cell lumas: ``base`` with a random ``frac`` of the cells raised by ``lift``."""
    return np.where(rng.random((gh, gw)) < frac, base + lift, base).astype(np.uint8)


def spiral(gh, gw):
    """A one-cell-wide rectangular spiral with one-cell gaps, from the outer corner inwards: one component."""
    m = np.zeros((gh, gw), np.uint8)
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    x = y = k = 0
    m[0, 0] = 1
    turned = False
    while True:                                                     # walk ahead while the cell two ahead is free, else turn right once
        dx, dy = dirs[k]
        ax, ay, bx, by = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        ahead = 0 <= ax < gw and 0 <= ay < gh and not m[ay, ax]
        beyond = not (0 <= bx < gw and 0 <= by < gh) or not m[by, bx]
        if ahead and beyond:
            x, y = ax, ay
            m[y, x] = 1
            turned = False
        elif turned:
            return m
        else:
            k = (k + 1) % 4
            turned = True


def comb(gh, gw):
    """Teeth in every other column that join only in the last row."""
    m = np.zeros((gh, gw), np.uint8)
    m[:, ::2] = 1
    m[gh - 1, :] = 1
    return m


def diagonal(gh, gw):
    """A one-cell-wide diagonal across the whole grid (cells that touch only by their corners)."""
    m = np.zeros((gh, gw), np.uint8)
    n = max(gh, gw)
    i = np.arange(n)
    m[i * gh // n, i * gw // n] = 1
    return m


def full(gh, gw):
    return np.ones((gh, gw), np.uint8)


SHAPES = {"spiral": spiral, "comb": comb, "diagonal": diagonal, "full": full}
