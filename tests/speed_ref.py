"""The speed estimator's rules (csrc/ground_plane.h, csrc/speed.hip, include/rtmodt.h), restated: plain Python integers with
``math.isqrt`` for everything after the rounding, NumPy float32 for the anchor and NumPy float64 -- one rounded operation per
line, in the header's order -- for the projection.  The kernels are held equal to this, exactly; ``HAND_CASES`` are worked on
paper and ``tests/test_speed_cpu.py`` holds this file to them.

A fixed camera, one plane per stream.  Per call and sampled track, in this order: ring, odometer (dead band), speed (chord of the
ring over its time span, floor), histogram, SPEEDING, STOPPED, WRONG_WAY; events leave in list order, kinds in that order; pairs in
(i, j) order of the sampled list."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
FOOT, CENTRE = 0, 1
LIMIT = 1 << 29
F_TIMER, F_NEW = 8, 16
KINDS = ("speeding", "stopped", "wrong_way")
INT32_MAX = 2 ** 31 - 1

# the largest reprojection residual of fit_plane against the constructed truth over FIT_CASES (4 exact correspondences, 8 and 16
# over-determined), in mm, measured with this file and with tests/native/ground_plane_check.cpp (the larger of the two); the tests
# assert 8 x this (host compilers may order float64 sums differently); recorded in DESIGN.md section 30
FIT_RESIDUAL_MEASURED_MM = 7.4e-12
FIT_RESIDUAL_BOUND_MM = 8 * FIT_RESIDUAL_MEASURED_MM


def anchor(kind, box):
    """The float32 anchor of a box, or None when a coordinate (or the float32 sum) is not finite."""
    b = np.asarray(box, F32)
    if not np.all(np.isfinite(b)):
        return None
    with np.errstate(over="ignore"):
        u = F32(F32(b[0] + b[2]) / F32(2))
        v = F32(F32(b[1] + b[3]) / F32(2)) if kind == CENTRE else b[3]
    if not (np.isfinite(u) and np.isfinite(v)):
        return None
    return u, v


def project(H, u, v):
    """(X, Y) in integer mm, or None off the plane: ground_plane.h, operation by operation."""
    H = np.asarray(H, F64).reshape(9)
    u, v = F64(u), F64(v)
    with np.errstate(all="ignore"):
        w = F64(F64(F64(H[6] * u) + F64(H[7] * v)) + H[8])
        xn = F64(F64(F64(H[0] * u) + F64(H[1] * v)) + H[2])
        yn = F64(F64(F64(H[3] * u) + F64(H[4] * v)) + H[5])
        if not w > 0:
            return None
        fx = np.floor(F64(F64(xn / w) + F64(0.5)))
        fy = np.floor(F64(F64(yn / w) + F64(0.5)))
    if not (fx >= -LIMIT and fx <= LIMIT and fy >= -LIMIT and fy <= LIMIT):
        return None
    return int(fx), int(fy)


def dist2(a, b):
    return (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2


def speed_of(d_mm, dt_us):
    return min(d_mm * 1_000_000 // dt_us, INT32_MAX)


def percentile_of(hist, bin_mm_s, p):
    """Nearest rank: the upper edge of the first bin whose cumulative count reaches ceil(p / 100 * total) (at least 1); None when empty,
    inf for the open-ended last bin."""
    h = [int(v) for v in hist]
    total = sum(h)
    if total == 0:
        return None
    need = max(1, -(-int(round(p * 1000)) * total // 100000))
    run = 0
    for b, v in enumerate(h):
        run += v
        if run >= need:
            return math.inf if b == len(h) - 1 else (b + 1) * bin_mm_s
    return math.inf


class SpeedRef:
    """One stream.  ``process(rows, t_us)`` with rows = [(track id, xyxy, class), ...] in the caller's order returns
    ``(rows_out, events, pairs, total_pairs)`` as plain dicts / tuples; ``snapshot()`` is the ledger's canonical form."""

    def __init__(self, plane=None, *, mm_per_pixel=None, anchor=FOOT, window=8, min_samples=2, hold=3, max_gap_us=1_000_000, min_step_mm=50,
                 limit_mm_s=0, stop_mm_s=0, stop_us=2_000_000, wrong_way_min_mm_s=500, allowed_dir=(0, 0), bins=0, bin_mm_s=1000, proximity_mm=0,
                 max_pairs=256, max_events=256, classes=None, max_tracks=1024):
        self.H = None if plane is None and mm_per_pixel is None else (
            np.asarray(plane, F64).reshape(9) if plane is not None else np.array([mm_per_pixel, 0, 0, 0, mm_per_pixel, 0, 0, 0, 1], F64))
        self.anchor, self.window, self.min_samples, self.hold = anchor, window, min_samples, hold
        self.max_gap_us, self.min_step_mm, self.limit, self.stop, self.stop_us = max_gap_us, min_step_mm, limit_mm_s, stop_mm_s, stop_us
        self.ww_min, self.dir, self.bins, self.bin_w, self.prox = wrong_way_min_mm_s, tuple(allowed_dir), bins, bin_mm_s, proximity_mm
        self.max_pairs, self.max_events, self.classes, self.cap = max_pairs, max_events, None if classes is None else set(classes), 2 * max_tracks
        self.rows = {}                       # id -> dict
        self.hist = [0] * bins
        self.last_t = None
        self.ledger_overflow = self.events_truncated = self.pairs_truncated = False

    def sample(self, box, cls):
        if self.classes is not None and cls not in self.classes:
            return None
        uv = anchor(self.anchor, box)
        return None if uv is None else project(self.H, *uv)

    def process(self, rows, t_us):
        assert self.H is not None, "no plane"
        assert self.last_t is None or t_us > self.last_t, "t_us must increase"
        self.last_t = t_us
        sampled = []
        for idx, (tid, box, cls) in enumerate(rows):
            P = self.sample(box, cls)
            if P is not None:
                sampled.append((idx, int(tid), np.asarray(box, F32), int(cls), P))
        # rows older than max_gap_us are dropped (also the row of an id that returns now: it starts fresh)
        self.rows = {i: r for i, r in self.rows.items() if t_us - r["last"] <= self.max_gap_us}
        ids_now = {s[1] for s in sampled}
        for r in self.rows.values():
            r["flags"] &= ~F_NEW
        if len(ids_now | set(self.rows)) > self.cap:                          # the idle rows go, the stream is in error for good
            self.ledger_overflow = True
            self.rows = {i: r for i, r in self.rows.items() if i in ids_now}
        out_rows, events = [], []
        for idx, tid, box, cls, P in sampled:
            r = self.rows.get(tid)
            if r is None:
                r = self.rows[tid] = dict(ring=[], odo=0, anchor=P, peak=-1, flags=F_NEW, run_s=0, run_w=0, since=None)
            else:
                step = math.isqrt(dist2(r["anchor"], P))
                if step >= self.min_step_mm:
                    r["odo"] += step
                    r["anchor"] = P
            r["ring"] = (r["ring"] + [(P[0], P[1], t_us)])[-self.window:]
            r["last"], r["cls"] = t_us, cls
            speed, chord = -1, (0, 0)
            if len(r["ring"]) >= self.min_samples:
                q = r["ring"][0]
                chord = (P[0] - q[0], P[1] - q[1])
                speed = speed_of(math.isqrt(dist2(q, P)), t_us - q[2])
                if self.bins:
                    self.hist[min(speed // self.bin_w, self.bins - 1)] += 1
            r["speed"], r["chord"], r["peak"] = speed, chord, max(r["peak"], speed)
            fired = []
            if self.limit > 0:
                if speed > self.limit:
                    r["run_s"] = min(r["run_s"] + 1, self.hold)
                    if r["run_s"] >= self.hold and not r["flags"] & 1:
                        r["flags"] |= 1
                        fired.append(0)
                else:
                    r["run_s"] = 0
                    r["flags"] &= ~1
            if self.stop > 0:
                if 0 <= speed < self.stop:
                    if not r["flags"] & F_TIMER:
                        r["flags"] |= F_TIMER
                        r["since"] = t_us
                    if t_us - r["since"] >= self.stop_us and not r["flags"] & 2:
                        r["flags"] |= 2
                        fired.append(1)
                else:
                    r["flags"] &= ~(F_TIMER | 2)
                    r["since"] = None
            if self.dir != (0, 0):
                if speed >= 0 and speed >= self.ww_min and chord[0] * self.dir[0] + chord[1] * self.dir[1] < 0:
                    r["run_w"] = min(r["run_w"] + 1, self.hold)
                    if r["run_w"] >= self.hold and not r["flags"] & 4:
                        r["flags"] |= 4
                        fired.append(2)
                else:
                    r["run_w"] = 0
                    r["flags"] &= ~4
            out_rows.append(dict(track_id=tid, track=idx, world=list(P), speed_mm_s=speed, peak_mm_s=r["peak"], heading=list(chord), odometer_mm=r["odo"],
                                 class_id=cls, flags=r["flags"], n_samples=len(r["ring"])))
            for k in fired:
                events.append(dict(kind=KINDS[k], track_id=tid, speed_mm_s=speed, t_us=t_us, bbox_xyxy=[float(v) for v in box], world_mm=list(P),
                                   class_id=cls, track=idx))
        pairs = []
        if self.prox > 0:
            for i in range(len(sampled)):
                for j in range(i + 1, len(sampled)):
                    d2 = dist2(sampled[i][4], sampled[j][4])
                    if d2 < self.prox * self.prox:
                        pairs.append((sampled[i][1], sampled[j][1], math.isqrt(d2)))
        self.events_truncated = len(events) > self.max_events
        self.pairs_truncated = len(pairs) > self.max_pairs
        return out_rows, events, pairs[:self.max_pairs], len(pairs)

    def snapshot(self):
        return [[i, r["last"], [list(s) for s in r["ring"]], r["odo"], list(r["anchor"]), r["speed"], r["peak"], list(r["chord"]), r["cls"], r["flags"],
                 r["run_s"], r["run_w"], r["since"] if r["flags"] & F_TIMER else None] for i, r in sorted(self.rows.items())]


# ---------------------------------------------------------------------------------------------------------------------------------
# fit_plane: normalised DLT, h8 = 1 in the normalised frames, 8 x 8 normal equations, Gaussian elimination with partial pivoting
# ---------------------------------------------------------------------------------------------------------------------------------
def _normaliser(xy, normalise):
    if not normalise:
        return 0.0, 0.0, 1.0
    c = xy.mean(axis=0)
    m = np.sqrt(((xy - c) ** 2).sum(axis=1)).mean()
    if not m > 0:
        return None
    return float(c[0]), float(c[1]), float(np.sqrt(2.0) / m)


def _solve(A, b, tol):
    A, b, n = A.copy(), b.copy(), len(b)
    big = np.abs(A).max()
    if not big > 0:
        return None
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if not abs(A[p, c]) > tol * big:
            return None
        if p != c:
            A[[c, p]] = A[[p, c]]
            b[[c, p]] = b[[p, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    for r in range(n - 1, -1, -1):
        b[r] = (b[r] - A[r, r + 1:] @ b[r + 1:]) / A[r, r]
    return b


def project64(H, uv):
    """The continuous projection of points [n, 2] (no rounding)."""
    H = np.asarray(H, F64).reshape(3, 3)
    p = np.c_[np.asarray(uv, F64), np.ones(len(uv))] @ H.T
    return p[:, :2] / p[:, 2:3]


def fit_plane(img_xy, world_xy, normalise=True):
    """(H [3, 3] scaled to w = 1 at the image centroid, max residual in mm), or None for degenerate input.  ``normalise=False`` is the
    deliberate defect of tests/test_speed_cpu.py."""
    a, b = np.asarray(img_xy, F64).reshape(-1, 2), np.asarray(world_xy, F64).reshape(-1, 2)
    n = len(a)
    if n < 4 or len(b) != n or not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return None
    ni, nw = _normaliser(a, normalise), _normaliser(b, normalise)
    if ni is None or nw is None:
        return None
    (icx, icy, isc), (wcx, wcy, wsc) = ni, nw
    M, r = np.zeros((8, 8)), np.zeros(8)
    for i in range(n):
        u, v = isc * (a[i, 0] - icx), isc * (a[i, 1] - icy)
        x, y = wsc * (b[i, 0] - wcx), wsc * (b[i, 1] - wcy)
        for row, rhs in ((np.array([u, v, 1, 0, 0, 0, -u * x, -v * x]), x), (np.array([0, 0, 0, u, v, 1, -u * y, -v * y]), y)):
            M += np.outer(row, row)
            r += row * rhs
    h = _solve(M, r, 1e-12 if normalise else 0.0)            # (in normalised frames a pivot below 1e-12 means collinear points)
    if h is None:
        return None
    Hn = np.append(h, 1.0).reshape(3, 3)
    if normalise and not abs(np.linalg.det(Hn)) > 1e-10 * max(1.0, np.abs(Hn).max()) ** 3:      # collinear world points: the plane collapses onto a line
        return None
    Ti = np.array([[isc, 0, -isc * icx], [0, isc, -isc * icy], [0, 0, 1]])
    Twi = np.array([[1 / wsc, 0, wcx], [0, 1 / wsc, wcy], [0, 0, 1]])
    H = Twi @ Hn @ Ti
    wc = H[2] @ np.array([a[:, 0].mean(), a[:, 1].mean(), 1.0])
    if not np.isfinite(wc) or wc == 0:
        return None
    H = H / wc
    if not np.all(np.isfinite(H)) or np.linalg.det(H) == 0:
        return None
    p = np.c_[a, np.ones(n)] @ H.T
    if not np.all(p[:, 2] > 0):
        return None
    res = np.sqrt(((p[:, :2] / p[:, 2:3] - b) ** 2).sum(axis=1)).max()
    return H, float(res)


# a surveyed road seen from a pole: image 1920 x 1080, world in mm; perspective (H6, H7 != 0)
ROAD_H = np.array([[12.5, -3.25, -4000.0], [1.5, 55.0, -20000.0], [0.0, 0.0015625, 1.0]], F64)


def _inverse_project(H, world):
    Hi = np.linalg.inv(np.asarray(H, F64).reshape(3, 3))
    p = np.c_[np.asarray(world, F64), np.ones(len(world))] @ Hi.T
    return p[:, :2] / p[:, 2:3]


def fit_cases():
    """[(name, image points, world points = ROAD_H of them, the constructed truth)]: 4 exact correspondences, 8 and 16 over-determined."""
    rng = np.random.default_rng(30)
    out = []
    for n in (4, 8, 16):
        if n == 4:
            img = np.array([[200.0, 400.0], [1700.0, 420.0], [1850.0, 1000.0], [100.0, 1040.0]])
        else:
            img = np.c_[rng.uniform(50, 1870, n), rng.uniform(350, 1060, n)]
        out.append((f"n{n}", img, project64(ROAD_H, img)))
    return out


# the defect case: the correspondences crowd around (1900, 1000); without the normalisation the normal equations lose the fit
def defect_case():
    rng = np.random.default_rng(31)
    img = np.c_[1900 + rng.uniform(-15, 15, 8), 1000 + rng.uniform(-15, 15, 8)]
    return img, project64(ROAD_H, img)


# ---------------------------------------------------------------------------------------------------------------------------------
# hand cases
# ---------------------------------------------------------------------------------------------------------------------------------
def box(u, v, w=20.0, h=40.0):
    """A box whose FOOT anchor is exactly (u, v) (u, v multiples of 0.5, small)."""
    return [u - w / 2, v - h, u + w / 2, v]


# AFFINE: 20 mm per pixel plus an offset, half-integer anchors: every world coordinate is an exact integer.
AFFINE_H = [20.0, 0.0, 100.0, 0.0, 20.0, -40.0, 0.0, 0.0, 1.0]
SEC = 1_000_000
# track 7 walks +x at 2.5 px = 50 mm per 100 ms call = 500 mm/s, six calls; then stands (speed of the 4-window decays to 0).
# window 4, min_samples 2, min_step 30 mm, limit 400 mm/s hold 2, stop below 100 mm/s for 200 ms.
#   call t(ms) X      ring (oldest X)  speed                odo   events
#   0    0     300    -                -1                   0
#   1    100   350    300              50*1e6/1e5 = 500     50    (run_s 1)
#   2    200   400    300              100/0.2 = 500        100   SPEEDING (run_s 2 = hold)
#   3    300   450    300              150/0.3 = 500        150
#   4    400   500    350              150/0.3 = 500        200
#   5    500   550    400              500                  250
#   6    600   550    450              100/0.3 = 333        250   (<= limit: re-arms)
#   7    700   550    500              50/0.3 = 166         250
#   8    800   550    550              0                    250   timer starts at 800
#   9    900   550    550              0                    250
#   10   1000  550    550              0                    250   STOPPED (1000 - 800 >= 200)
#   11   1100  570    550              20/0.3 = 66          250   step 20 < 30: dead band, odometer and its anchor stay
#   12   1200  590    550              40/0.3 = 133         290   step from the anchor 550 -> 590 = 40: gained; 133 >= 100: timer off, re-armed
HAND_WALK_X = [10.0, 12.5, 15.0, 17.5, 20.0, 22.5, 22.5, 22.5, 22.5, 22.5, 22.5, 23.5, 24.5]
HAND_CASES = {
    "affine_walk": dict(
        plane=AFFINE_H,
        kwargs=dict(window=4, min_samples=2, hold=2, min_step_mm=30, limit_mm_s=400, stop_mm_s=100, stop_us=200_000, max_gap_us=SEC, bins=4, bin_mm_s=200),
        calls=[(k * 100_000, [(7, box(x, 52.0), 2)]) for k, x in enumerate(HAND_WALK_X)],
        world=[[int(20 * x + 100), 1000] for x in HAND_WALK_X],
        speeds=[-1, 500, 500, 500, 500, 500, 333, 166, 0, 0, 0, 66, 133],
        odometer=[0, 50, 100, 150, 200, 250, 250, 250, 250, 250, 250, 250, 290],
        events=[(2, "speeding", 500), (10, "stopped", 0)],
        hist=[6, 1, 5, 0],                   # bins of 200: [0,200): 166 0 0 0 66 133; [200,400): 333; [400,600): five 500s; last: none
    ),
    # two tracks head-on along y, allowed direction +y: track 2 goes the wrong way.  3-4-5 triangles give exact diagonal speeds.
    #   track 1: (0, 0) -> steps of (+30, +40) px * 20 mm = (600, 800) mm = 1000 mm per 500 ms = 2000 mm/s, heading . (0, 1) > 0
    #   track 2: steps of (0, -25) px = -500 mm per 500 ms = 1000 mm/s, heading . (0, 1) < 0: WRONG_WAY on its 3rd known speed (hold 3) = call 3
    #   world: track 1 at (600 k + 100, 800 k), track 2 at (1300, 3960 - 500 k).  proximity 1500 mm: call 2 (1300, 1600) and (1300, 2960): 1360 apart;
    #   call 3 (1900, 2400) and (1300, 2460): isqrt(600^2 + 60^2 = 363600) = 602 (603^2 = 363609); call 4: 1725 apart, no pair
    "head_on": dict(
        plane=AFFINE_H,
        kwargs=dict(window=8, min_samples=2, hold=3, min_step_mm=0, allowed_dir=(0, 1), wrong_way_min_mm_s=500, proximity_mm=1500, max_gap_us=SEC),
        calls=[(k * 500_000, [(1, box(0.0 + 30 * k, 2.0 + 40 * k), 0), (2, box(60.0, 200.0 - 25 * k), 0)]) for k in range(5)],
        world=None,
        speeds=None,
        events=[(3, "wrong_way", 1000)],
        pairs={2: [(1, 2, 1360)], 3: [(1, 2, 602)]},
    ),
}

# PERSPECTIVE: w = 0.001 v + 0.5, x = 1000 u, y = 1000 v; the anchors below are exact in float32 unless said otherwise.
#   v = -600: w = -0.1 <= 0; v = -500: w = 0                  -> off the plane
#   (1.0e6, 500): w = 1, x = 1e9 > 2^29                        -> off the plane
#   (0.75, 500): w = 1, x = 750, y = 500000                    -> (750, 500000)
#   (1.25, 1500): w = 2, x / w + 0.5 = 625.5                   -> (625, 750000)
#   (0.625, 1500): w = 2, x / w + 0.5 = 312.5 + 0.5 = 313, an exact integer   -> (313, 750000): the half rounds up
#   (-0.625, 1500): x / w + 0.5 = -312.5 + 0.5 = -312          -> (-312, 750000): the half rounds toward +inf
#   (536870.912, 500): float32 holds 536870.9375, x + 0.5 = 536870938 > 2^29 = 536870912   -> off the plane
#   (536870.5, 500): x = 536870500 <= 2^29                     -> (536870500, 500000)
PERSP_H = [1000.0, 0.0, 0.0, 0.0, 1000.0, 0.0, 0.0, 0.001, 0.5]
PERSP_POINTS = [
    ((0.0, -600.0), None),
    ((0.0, -500.0), None),
    ((1.0e6, 500.0), None),
    ((0.75, 500.0), (750, 500000)),
    ((1.25, 1500.0), (625, 750000)),
    ((0.625, 1500.0), (313, 750000)),
    ((-0.625, 1500.0), (-312, 750000)),
    ((536870.912, 500.0), None),
    ((536870.5, 500.0), (536870500, 500000)),
]

# the perspective family as a hand case: one call, one box per point above (its FOOT anchor is that point), then a box with a NaN;
# the points off the plane and the NaN box are not sampled (not clamped), the others land where the table says
HAND_CASES["perspective"] = dict(
    plane=PERSP_H, kwargs={},
    calls=[(0, [(k + 1, box(u, v), 0) for k, ((u, v), _) in enumerate(PERSP_POINTS)] + [(99, [float("nan"), 0.0, 1.0, 1.0], 0)])],
    events=[],
    first_call_ids=[k + 1 for k, (_, w) in enumerate(PERSP_POINTS) if w is not None],
    first_call_world=[list(w) for _, w in PERSP_POINTS if w is not None],
)


def track_rows(n, t, seed=0, lattice=200):
    """n tracks at pseudo-random half-integer anchors that drift with t: the large-shape scenes of the GPU test."""
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, 2 * lattice, n) / 2.0, rng.integers(0, 2 * lattice, n) / 2.0
    vx, vy = rng.integers(-4, 5, n) / 2.0, rng.integers(-4, 5, n) / 2.0
    return [(i + 1, box(float(x0[i] + vx[i] * t), float(y0[i] + vy[i] * t)), int(i % 3)) for i in range(n)]
