"""Plain NumPy / Python restatement of the colour attributes (``csrc/colour_rule.h``, ``csrc/colour.hip``): the name of a pixel, the
sampled rectangle and its grid, the parts, the occluders, the accumulation with its ageing, the labels and the id-keyed ledger with
its retention.  The kernels must equal it with ``==``; ``tests/test_colour_cpu.py`` checks it against literals and the header against
it.  Every rule has a ``defect`` switch that breaks it on purpose, so that the literals can be shown to notice."""
import dataclasses

import numpy as np

NAMES = ("black", "grey", "white", "red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown")
BLACK, GREY, WHITE, RED, ORANGE, YELLOW, GREEN, CYAN, BLUE, PURPLE, PINK, BROWN = range(12)
UPPER, LOWER, WHOLE = 0, 1, 2
F_NEW, F_MANY_OCCLUDERS, F_THIN = 1, 2, 4
MAX_OCCLUDERS, AGE_LIMIT, HUE_STEPS = 8, 1 << 24, 1536
DEFECTS = ("trunc_hue", "tie_g_first", "split_upper", "stride_floor", "occl_y0")


@dataclasses.dataclass(frozen=True)
class Cfg:
    black_max: int = 48
    chroma_min: int = 20
    sat_split: int = 96
    sat_hi_pm: int = 180
    sat_lo_pm: int = 400
    y_black: int = 64
    y_white: int = 176
    hue: tuple = (64, 192, 299, 725, 853, 1109, 1344, 1472)
    pink_mx: int = 192
    red_brown_mx: int = 96
    orange_brown_mx: int = 176
    yellow_brown_mx: int = 128
    inset_x_pm: int = 200
    top_pm: int = 150
    split_pm: int = 500
    bottom_pm: int = 900
    max_side: int = 48
    skip_occluded: int = 1
    min_samples: int = 16
    retire_after: int = 30
    classes: tuple = None


def luma(b, g, r):
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


# ---- 1. the name of a pixel --------------------------------------------------------------------------------------------------
def hue_int(b, g, r, defect=None):
    """The hue of a chromatic pixel in plain Python ints (``//`` floors)."""
    mx, c = max(b, g, r), max(b, g, r) - min(b, g, r)
    div = (lambda a: int(a / c)) if defect == "trunc_hue" else (lambda a: a // c)
    order = "grb" if defect == "tie_g_first" else "rgb"
    for ch in order:
        if ch == "r" and r == mx:
            return div((g - b) * 256) % HUE_STEPS
        if ch == "g" and g == mx:
            return (512 + div((b - r) * 256)) % HUE_STEPS
        if ch == "b" and b == mx:
            return (1024 + div((r - g) * 256)) % HUE_STEPS
    raise AssertionError


def name_int(k: Cfg, b, g, r, defect=None):
    b, g, r = int(b), int(g), int(r)
    mx, mn = max(b, g, r), min(b, g, r)
    c = mx - mn
    if mx < k.black_max:
        return BLACK
    sat = k.sat_hi_pm if mx >= k.sat_split else k.sat_lo_pm
    if c < k.chroma_min or c * 1000 <= sat * mx:
        y = luma(b, g, r)
        return BLACK if y < k.y_black else (WHITE if y >= k.y_white else GREY)
    h = hue_int(b, g, r, defect)
    H = k.hue
    if h < H[0] or h >= H[7]:
        return PINK if 2 * c < mx and mx >= k.pink_mx else (BROWN if mx < k.red_brown_mx else RED)
    if h < H[1]:
        return BROWN if mx < k.orange_brown_mx else ORANGE
    if h < H[2]:
        return BROWN if mx < k.yellow_brown_mx else YELLOW
    for bound, nm in ((H[3], GREEN), (H[4], CYAN), (H[5], BLUE), (H[6], PURPLE)):
        if h < bound:
            return nm
    return PINK


def name_vec(k: Cfg, bgr):
    """The same for an array ``(..., 3)`` of BGR pixels, vectorised: int64 arrays, ``np.floor_divide``."""
    p = np.asarray(bgr).astype(np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    mx, mn = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    c = mx - mn
    cs = np.where(c > 0, c, 1)
    h = np.where(r == mx, np.floor_divide((g - b) * 256, cs), np.where(g == mx, 512 + np.floor_divide((b - r) * 256, cs), 1024 + np.floor_divide((r - g) * 256, cs)))
    h = np.mod(h, HUE_STEPS)
    H = k.hue
    out = np.full(p.shape[:-1], PINK, np.int64)
    for bound, nm in ((H[6], PURPLE), (H[5], BLUE), (H[4], CYAN), (H[3], GREEN)):
        out = np.where(h < bound, nm, out)
    out = np.where(h < H[2], np.where(mx < k.yellow_brown_mx, BROWN, YELLOW), out)
    out = np.where(h < H[1], np.where(mx < k.orange_brown_mx, BROWN, ORANGE), out)
    red = np.where((2 * c < mx) & (mx >= k.pink_mx), PINK, np.where(mx < k.red_brown_mx, BROWN, RED))
    out = np.where((h < H[0]) | (h >= H[7]), red, out)
    y = luma(b, g, r)
    grey = np.where(y < k.y_black, BLACK, np.where(y >= k.y_white, WHITE, GREY))
    sat = np.where(mx >= k.sat_split, k.sat_hi_pm, k.sat_lo_pm)
    out = np.where((c < k.chroma_min) | (c * 1000 <= sat * mx), grey, out)
    return np.where(mx < k.black_max, BLACK, out)


# ---- 2. + 3. the sampled rectangle and its grid ------------------------------------------------------------------------------
def coord(v):
    """privacy_regions.h's corner rule: the float32 value clamped to +-2^20, truncated toward zero."""
    v = np.float32(v)
    lim = np.float32(1 << 20)
    return int(np.clip(v, -lim, lim))


def plan(k: Cfg, xyxy, h, w, cls=0, defect=None):
    """None: the box takes no row.  Else a dict: raw, box, rect (inclusive x0 y0 x1 y1; empty when x1 < x0 or y1 < y0), ys, sx, sy,
    nx, ny."""
    if k.classes is not None and int(cls) not in k.classes:
        return None
    if not all(np.isfinite(np.float32(v)) for v in xyxy):
        return None
    x0, y0, x1, y1 = (coord(v) for v in xyxy)
    if x1 < x0 or y1 < y0:
        return None
    W, H = x1 - x0 + 1, y1 - y0 + 1
    inset = W * k.inset_x_pm // 1000
    ra, rb = y0 + H * k.top_pm // 1000, y0 + H * k.bottom_pm // 1000 - 1
    ys = y0 + H * k.split_pm // 1000
    rect = (max(x0 + inset, 0), max(ra, 0), min(x1 - inset, w - 1), min(rb, h - 1))
    P = dict(raw=(x0, y0, x1, y1), box=(max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)), rect=rect, ys=ys, sx=1, sy=1, nx=0, ny=0)
    if rect[2] < rect[0] or rect[3] < rect[1]:
        return P
    sw, sh = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    if defect == "stride_floor":
        P["sx"], P["sy"] = max(1, sw // k.max_side), max(1, sh // k.max_side)
    else:
        P["sx"], P["sy"] = max(1, -(-sw // k.max_side)), max(1, -(-sh // k.max_side))
    P["nx"], P["ny"] = -(-sw // P["sx"]), -(-sh // P["sy"])
    return P


def empty(r):
    return r[2] < r[0] or r[3] < r[1]


def meet(a, b):
    return not empty(a) and not empty(b) and a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]


def part_of(P, y, defect=None):
    if defect == "split_upper":
        return UPPER if y <= P["ys"] else LOWER
    return UPPER if y < P["ys"] else LOWER


# ---- 4. the occluders, then a frame's histograms ------------------------------------------------------------------------------
def occluders(plans, ids, i, defect=None):
    """The clipped RAW rectangles that hide samples of entry i, and whether there were more than MAX_OCCLUDERS: ``plans`` / ``ids``
    in LIST order (None: the entry is not sampled)."""
    me = plans[i]
    key = (lambda P, t: (P["raw"][1], t)) if defect == "occl_y0" else (lambda P, t: (P["raw"][3], t))
    found = [plans[q]["box"] for q in range(len(plans)) if q != i and plans[q] is not None and key(plans[q], ids[q]) > key(me, ids[i]) and meet(plans[q]["box"], me["rect"])]
    return found[:MAX_OCCLUDERS], len(found) > MAX_OCCLUDERS


def frame_hist(k: Cfg, frame, plans, ids, i, defect=None):
    """(hist [2][12] as a list of 24 ints, flags) of entry i of a list."""
    P = plans[i]
    hist = [0] * 24
    occ, many = (occluders(plans, ids, i, defect) if k.skip_occluded and not empty(P["rect"]) else ([], False))
    if P["nx"] and P["ny"]:
        xs = P["rect"][0] + P["sx"] * np.arange(P["nx"])
        ys = P["rect"][1] + P["sy"] * np.arange(P["ny"])
        X, Y = np.meshgrid(xs, ys)
        keep = np.ones(X.shape, bool)
        for o in occ:
            keep &= ~((X >= o[0]) & (X <= o[2]) & (Y >= o[1]) & (Y <= o[3]))
        names = name_vec(k, frame[Y, X]) if defect is None else np.array([[name_int(k, *frame[y, x], defect=defect) for x in xs] for y in ys])
        part = np.array([[part_of(P, int(y), defect) for _ in xs] for y in ys])
        flat = (part * 12 + names)[keep]
        hist = np.bincount(flat, minlength=24).tolist()
    return hist, (F_MANY_OCCLUDERS if many else 0)


# ---- 5. + 6. a row ---------------------------------------------------------------------------------------------------------
def accumulate(row, fh, min_samples):
    """Adds a frame's 24 counts into a row's (in place); returns whether they were added."""
    if sum(fh) < min_samples:
        return False
    for p in range(2):
        for q in range(12):
            row[p * 12 + q] += fh[p * 12 + q]
        if sum(row[p * 12:p * 12 + 12]) > AGE_LIMIT:
            for q in range(12):
                row[p * 12 + q] //= 2
    return True


def label(row, part):
    """(name, share_pm, second, second_pm, samples) of a part of a row of 24 counts."""
    v = [row[q] + row[12 + q] for q in range(12)] if part == WHOLE else list(row[part * 12:part * 12 + 12])
    tot = sum(v)
    if tot == 0:
        return (-1, 0, -1, 0, 0)
    a = max(range(12), key=lambda q: (v[q], -q))
    rest = [q for q in range(12) if q != a and v[q] > 0]
    if not rest:
        return (a, v[a] * 1000 // tot, -1, 0, tot)
    s = max(rest, key=lambda q: (v[q], -q))
    return (a, v[a] * 1000 // tot, s, v[s] * 1000 // tot, tot)


@dataclasses.dataclass
class Row:
    track_id: int
    first: int
    last: int
    hist: list
    cls: int
    used: int
    flags: int

    def out(self, track=-1, frame_samples=0, flags=None):
        """The row as the library hands it out, ready for ``==``."""
        return (self.track_id, self.first, self.last, list(self.hist), self.cls, self.used, self.flags if flags is None else flags, track, frame_samples,
                [label(self.hist, p) for p in range(3)])


class Stream:
    """One stream's ledger.  ``process`` -> (code, updated, retired); code 0, or -4 from the overflowing call on (sticky)."""

    def __init__(self, cfg: Cfg, max_tracks: int):
        self.k, self.cap = cfg, 2 * max_tracks
        self.rows = {}
        self.err = 0

    def process(self, ids, xyxy, cls, frame, frame_id, selected=None, list_order="id", defect=None):
        """``ids`` / ``xyxy`` / ``cls`` in the caller's order (``updated`` follows it); ``selected``: the entries a tracker passes
        (None: all).  list_order "id": the occluders are taken in ascending id (a caller's list); "given": in the order given (a
        tracker's own list)."""
        k = self.k
        h, w = frame.shape[:2]
        n = len(ids)
        sel = [True] * n if selected is None else [bool(v) for v in selected]
        plans = [plan(k, xyxy[i], h, w, cls[i], defect) if sel[i] else None for i in range(n)]
        walk = sorted(range(n), key=lambda i: int(ids[i])) if list_order == "id" else list(range(n))
        lp, li = [plans[i] for i in walk], [int(ids[i]) for i in walk]
        retired = []
        for t in sorted(self.rows):
            if frame_id - self.rows[t].last > k.retire_after:
                row = self.rows.pop(t)
                retired.append(row.out(flags=row.flags & ~F_NEW))
        members = [i for i in range(n) if plans[i] is not None]
        idle = [t for t in self.rows if t not in {int(ids[i]) for i in members}]
        if len(members) + len(idle) > self.cap:
            for t in idle:
                del self.rows[t]
            self.err = 1
        for t in self.rows:
            self.rows[t].flags &= ~F_NEW
        updated = []
        for i in members:
            fh, fl = frame_hist(k, frame, lp, li, walk.index(i), defect)
            t = int(ids[i])
            old = self.rows.get(t)
            row = Row(t, frame_id, frame_id, [0] * 24, int(cls[i]), 0, 0) if old is None else old
            added = accumulate(row.hist, fh, k.min_samples)
            row.last, row.cls, row.used = frame_id, int(cls[i]), row.used + (1 if added else 0)
            row.flags = fl | (F_NEW if old is None else 0) | (0 if added else F_THIN)
            self.rows[t] = row
            updated.append(row.out(track=i, frame_samples=sum(fh)))
        return (-4 if self.err else 0), updated, retired

    def state(self):
        return [self.rows[t].out() for t in sorted(self.rows)]

    def label(self, track_id):
        r = self.rows[track_id]
        return tuple(NAMES[label(r.hist, p)[0]] if label(r.hist, p)[0] >= 0 else None for p in (UPPER, LOWER))
