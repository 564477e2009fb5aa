"""Cases the CPU and the GPU tests of the colour attributes share: the name literals, hand-worked plans, painted scenes and the
scripted track sequences.  Nothing here computes an expectation with the code under test: literals are written out, scenes are
painted with plain NumPy."""
import numpy as np

# name -> sRGB literals (r, g, b)
NAME_LITERALS = {
    "black": [(0, 0, 0), (40, 60, 45)],
    "white": [(255, 255, 255), (192, 192, 192), (245, 245, 220)],
    "grey": [(128, 128, 128), (54, 69, 79)],
    "red": [(255, 0, 0), (220, 20, 60), (139, 0, 0)],
    "orange": [(255, 165, 0)],
    "yellow": [(255, 255, 0), (255, 215, 0)],
    "green": [(0, 128, 0), (34, 139, 34)],
    "cyan": [(0, 128, 128), (0, 255, 255)],
    "blue": [(0, 0, 255), (0, 0, 128), (21, 96, 189)],
    "purple": [(128, 0, 128), (138, 43, 226)],
    "pink": [(255, 192, 203), (255, 105, 180)],
    "brown": [(139, 69, 19), (160, 82, 45)],
}

# the names on both sides of every hue bound for a bright, saturated pixel (max >= 192, 2 c >= max): (bound, below, from it on)
HUE_SIDES = [(64, "red", "orange"), (192, "orange", "yellow"), (299, "yellow", "green"), (725, "green", "cyan"), (853, "cyan", "blue"),
             (1109, "blue", "purple"), (1344, "purple", "pink"), (1472, "pink", "red")]

# hand-worked plans at the defaults (inset 200, rows 150 / 500 / 900, max_side 48) in a 240 x 320 frame:
# (xyxy, expected) with expected None (no row) or (raw, box, rect, ys, sx, sy, nx, ny)
PLANS = [
    ((100, 50, 139, 149), ((100, 50, 139, 149), (100, 50, 139, 149), (108, 65, 131, 139), 100, 1, 2, 24, 38)),           # W 40, H 100
    ((-20, 50, 19, 149), ((-20, 50, 19, 149), (0, 50, 19, 149), (0, 65, 11, 139), 100, 1, 2, 12, 38)),                   # cut by the left border
    ((100, -30, 139, 69), ((100, -30, 139, 69), (100, 0, 139, 69), (108, 0, 131, 59), 20, 1, 2, 24, 30)),               # ... the top
    ((300, 50, 339, 149), ((300, 50, 339, 149), (300, 50, 319, 149), (308, 65, 319, 139), 100, 1, 2, 12, 38)),           # ... the right
    ((100, 200, 139, 299), ((100, 200, 139, 299), (100, 200, 139, 239), (108, 215, 131, 239), 250, 1, 1, 24, 25)),       # ... the bottom: UPPER only
    ((5, 5, 5, 5), ((5, 5, 5, 5), (5, 5, 5, 5), (5, 5, 5, 4), 5, 1, 1, 0, 0)),                                           # 1 x 1: a row, no sample
    ((400, 300, 450, 380), ((400, 300, 450, 380), (400, 300, 319, 239), (410, 312, 319, 239), 340, 1, 1, 0, 0)),         # wholly outside
    ((10, 10, 89, 73), ((10, 10, 89, 73), (10, 10, 89, 73), (26, 19, 73, 66), 42, 1, 1, 48, 48)),                        # Sw = Sh = max_side
    ((10, 10, 90, 74), ((10, 10, 90, 74), (10, 10, 90, 74), (26, 19, 74, 67), 42, 2, 2, 25, 25)),                        # Sw = Sh = max_side + 1
    ((10, 20, 19, 22), ((10, 20, 19, 22), (10, 20, 19, 22), (12, 20, 17, 21), 21, 1, 1, 6, 2)),                          # H 3: row 21 is the split row, LOWER's first
    ((10, 20, 19, 21), ((10, 20, 19, 21), (10, 20, 19, 21), (12, 20, 17, 20), 21, 1, 1, 6, 1)),                          # H 2: UPPER only
    ((-0.9, 10.7, 9.2, 20.9), ((0, 10, 9, 20), (0, 10, 9, 20), (2, 11, 7, 18), 15, 1, 1, 6, 8)),                          # truncation toward zero
    ((30, 10, 29, 20), None),                                                                                              # x1 < x0
    ((float("nan"), 10, 29, 20), None),
    ((0, 0, float("inf"), 20), None),
]

RGB = {"red": (200, 30, 30), "blue": (30, 40, 200), "yellow": (230, 220, 30), "green": (40, 150, 50), "white": (230, 230, 230), "black": (10, 10, 10),
       "grey": (120, 120, 120), "orange": (240, 150, 20), "purple": (130, 30, 150), "cyan": (30, 200, 200), "pink": (250, 170, 200), "brown": (120, 70, 30)}


def bgr(name):
    r, g, b = RGB[name]
    return np.array([b, g, r], np.int64)


def textured(h, w, rng, base="green", noise=6):
    """An (h, w, 3) BGR frame of one colour with a coarse texture (+-10 in 8 x 8 blocks) and +-noise per channel."""
    tex = rng.integers(-10, 11, ((h + 7) // 8, (w + 7) // 8, 1)).repeat(8, 0).repeat(8, 1)[:h, :w]
    f = bgr(base)[None, None, :] + tex + rng.integers(-noise, noise + 1, (h, w, 3))
    return np.clip(f, 0, 255).astype(np.uint8)


def paint(frame, box, colour, rng, noise=6):
    """Fills the inclusive pixel box x0 y0 x1 y1 (clipped) with `colour` +- noise."""
    h, w = frame.shape[:2]
    x0, y0, x1, y1 = max(int(box[0]), 0), max(int(box[1]), 0), min(int(box[2]), w - 1), min(int(box[3]), h - 1)
    if x1 < x0 or y1 < y0:
        return
    f = bgr(colour)[None, None, :] + rng.integers(-noise, noise + 1, (y1 - y0 + 1, x1 - x0 + 1, 3))
    frame[y0:y1 + 1, x0:x1 + 1] = np.clip(f, 0, 255).astype(np.uint8)


def paint_person(frame, box, upper, lower, rng, split_pm=500):
    x0, y0, x1, y1 = (int(v) for v in box)
    ys = y0 + (y1 - y0 + 1) * split_pm // 1000
    paint(frame, (x0, y0, x1, ys - 1), upper, rng)
    paint(frame, (x0, ys, x1, y1), lower, rng)


def noise_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def strided(frame, stride, lead):
    """The frame copied into a byte buffer at `lead` with rows `stride` apart, ending at the frame's last byte; returns (buffer, view)."""
    h, w = frame.shape[:2]
    buf = np.zeros(lead + (h - 1) * stride + 3 * w, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[lead:], (h, w, 3), (stride, 3, 1))
    view[...] = frame
    return buf, view


# ---- scripted sequences for the ledger: frame f of stream s -> (ids, xyxy, cls) in the CALLER's order (not ascending) -------------------
def churn(f, s):
    """Tracks appear, vanish, return inside retire_after (= 2 in the tests) and retire after it; 37 x 70 frames."""
    rows = [(7 + s, (2 + f, 3, 21 + f, 33), 0), (3, (25, 2 + s, 44, 30 + s), 1)]
    if f in (0, 1, 4, 5):
        rows.append((11, (40, 5, 66, 36), 0))              # absent for frames 2, 3: back within retire_after
    if f in (0, 5):
        rows.append((5, (-6, -4, 13, 25), 2))              # absent for frames 1..4: retired at 3, a new row at 5
    if f == 2:
        rows.append((20 + s, (60, 20, 75, 50), 0))         # one frame only: retires at 5
    rows.append((30, (50, 30, 50, 30), 0))                 # 1 x 1: a row without samples
    if f % 2:
        rows.append((31, (90, 5, 120, 30), 0))             # wholly outside
    order = np.random.default_rng(100 * f + s).permutation(len(rows))
    rows = [rows[i] for i in order]
    return (np.int64([r[0] for r in rows]), np.float32([r[1] for r in rows]).reshape(-1, 4), np.int32([r[2] for r in rows]))
