"""NumPy restatement of the DeepSORT tracker of ``csrc/deepsort.hip`` and of the appearance descriptor and gallery distance of
``csrc/appearance.hip`` -- TEST INFRASTRUCTURE, written rule by rule as the kernels' header comments read.  Slow by design.

The algorithm is the published one (Wojke et al.; deep_sort's ``tracker.py``, ``linear_assignment.py``, ``nn_matching.py``,
``kalman_filter.py``).  PARITY UNPINNED: ``deep_sort_realtime`` is not installed anywhere this runs, so nothing here is checked
against that library; ``tests/test_deepsort_cpu.py`` checks the pieces against independent forms instead (the 8x8 float64 Kalman
filter, SciPy's Hungarian run the way ``min_cost_matching`` runs it, a per-pixel histogram loop).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import kalman_oracle as K
from oracle.tracker_oracle import F32, batch_iou

DIM = 192
DOT_ONE = 127 * 127                        # 16129: the dot product of a unit descriptor with itself
GATE = F32(9.4877)                         # chi2inv95[4]
COORD_MAX = 1 << 20
INT32_MIN = -(1 << 31)
TENTATIVE, CONFIRMED = 1, 2


# ---- appearance descriptor ------------------------------------------------------------------------------------------
def coord(v) -> int:
    f = float(np.float32(v))
    return int(max(-COORD_MAX, min(COORD_MAX, f)))


def box_region(box, h, w):
    """(x0, y0, x1, y1) pixel region (half-open) or None for the all-zero descriptor."""
    b = [float(np.float32(v)) for v in box]
    if any(v != v for v in b):
        return None
    x0, y0, x1, y1 = (coord(v) for v in b)
    x0, x1 = min(max(x0, 0), w), min(max(x1, 0), w)
    y0, y1 = min(max(y0, 0), h), min(max(y1, 0), h)
    if x1 - x0 <= 0 or y1 - y0 <= 0:
        return None
    return x0, y0, x1, y1


def describe_counts(frame: np.ndarray, box) -> np.ndarray:
    """int32[192] bin counts of one box: 4 stripes x (B, G, R) x 16 bins."""
    h, w = frame.shape[:2]
    out = np.zeros(DIM, np.int32)
    reg = box_region(box, h, w)
    if reg is None:
        return out
    x0, y0, x1, y1 = reg
    H = y1 - y0
    for s in range(4):
        r0, r1 = y0 + (s * H) // 4, y0 + ((s + 1) * H) // 4
        patch = frame[r0:r1, x0:x1]
        for c in range(3):
            out[s * 48 + c * 16:s * 48 + c * 16 + 16] = np.bincount((patch[:, :, c] >> 4).reshape(-1), minlength=16)
    return out


def quantize_counts(counts) -> np.ndarray:
    """int32 counts -> int8: r = isqrt(sum count^2), q = min(127, (127 * count + r // 2) // r); r == 0 gives zeros."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    r = math.isqrt(sum(v * v for v in c))
    if r == 0:
        return np.zeros(len(c), np.int8)
    return np.asarray([min(127, (127 * v + r // 2) // r) for v in c], np.int8)


def describe(frame, boxes):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    counts = np.stack([describe_counts(frame, b) for b in boxes]) if len(boxes) else np.zeros((0, DIM), np.int32)
    desc = np.stack([quantize_counts(c) for c in counts]) if len(boxes) else np.zeros((0, DIM), np.int8)
    return desc, counts


def quantize_rows(x) -> np.ndarray:
    """Float embedding rows -> int8: float64, sequential summation, rint(127 * x / ||x||); a zero row gives zeros."""
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape, np.int8)
    for i, row in enumerate(x.astype(np.float64)):
        n2 = 0.0
        for v in row:
            n2 += float(v) * float(v)
        norm = math.sqrt(n2)
        if norm > 0.0 and math.isfinite(norm):
            out[i] = np.clip(np.rint(127.0 * row / norm), -127, 127).astype(np.int8)
    return out


def dotmax(gallery, counts, dets) -> np.ndarray:
    """gallery (T, budget, dim) int8, counts[T], dets (N, dim) int8 -> (T, N) int32, INT32_MIN for an empty gallery."""
    g = np.asarray(gallery, np.int64)
    d = np.asarray(dets, np.int64)
    out = np.full((g.shape[0], d.shape[0]), INT32_MIN, np.int64)
    for t in range(g.shape[0]):
        if counts[t] > 0:
            out[t] = (g[t, :counts[t]] @ d.T).max(axis=0)
    return out.astype(np.int32)


# ---- gating ------------------------------------------------------------------------------------------------------------
def projected_var(mean, cov):
    """(n, 4) float32: a_k + r_k, r as kalman_oracle.kf_update computes it."""
    mean = np.asarray(mean, F32).reshape(-1, 8)
    cov = np.asarray(cov, F32).reshape(-1, 4, 3)
    sp = K.WP * mean[:, 3]
    r = (sp * sp).astype(F32)
    S = np.empty((mean.shape[0], 4), F32)
    for k in range(4):
        S[:, k] = cov[:, k, 0] + (r if k != 2 else K.A_PROJ * K.A_PROJ)
    return S


def gating_d2(mean, cov, z) -> np.ndarray:
    """(n_tracks, n_dets) float32 squared Mahalanobis distance in measurement space, one rounding per operation, k = 0..3."""
    mean = np.asarray(mean, F32).reshape(-1, 8)
    z = np.asarray(z, F32).reshape(-1, 4)
    S = projected_var(mean, cov)
    d2 = None
    for k in range(4):
        y = (z[None, :, k] - mean[:, None, k]).astype(F32)
        term = ((y * y).astype(F32) / S[:, None, k]).astype(F32)
        d2 = term if d2 is None else (d2 + term).astype(F32)
    return d2 if d2 is not None else np.zeros((mean.shape[0], z.shape[0]), F32)


# ---- exact maximum-gain matching -----------------------------------------------------------------------------------------
def max_gain_matching(gain):
    """gain[r][c]: a number > 0 for an admissible pair, None otherwise.  Returns (pairs, total): a matching of maximum total gain,
    found exactly (Fractions are fine; ints and floats are used here) by the Hungarian method on the matrix padded with zero-gain
    dummies.  Written independently of csrc/lap.h (dense, O(n^3))."""
    m = len(gain)
    n = len(gain[0]) if m else 0
    if m == 0 or n == 0:
        return [], 0
    size = m + n                                           # row r's private dummy column n + r, column c's dummy row m + c
    zero = 0 * next((g for row in gain for g in row if g is not None), 0)
    big = None
    cost = [[None] * size for _ in range(size)]
    for r in range(size):
        for c in range(size):
            if r < m and c < n:
                cost[r][c] = None if gain[r][c] is None else -gain[r][c]
            elif r < m:
                cost[r][c] = zero if c - n == r else None
            elif c < n:
                cost[r][c] = zero if r - m == c else None
            else:
                cost[r][c] = zero
    # Hungarian (e-maxx form) with None = forbidden
    INF = float("inf")
    u = [zero] * (size + 1)
    v = [zero] * (size + 1)
    p = [0] * (size + 1)
    way = [0] * (size + 1)
    for i in range(1, size + 1):
        p[0] = i
        j0 = 0
        minv = [INF] * (size + 1)
        used = [False] * (size + 1)
        while True:
            used[j0] = True
            i0 = p[j0]
            delta, j1 = INF, -1
            for j in range(1, size + 1):
                if used[j]:
                    continue
                cij = cost[i0 - 1][j - 1]
                if cij is not None:
                    cur = cij - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j] = cur
                        way[j] = j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            for j in range(size + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                elif minv[j] != INF:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    del big
    pairs = sorted((p[j] - 1, j - 1) for j in range(1, n + 1) if 1 <= p[j] <= m)
    return pairs, sum(gain[r][c] for r, c in pairs)


def unique_optimum(gain, pairs, total) -> bool:
    """The optimum is unique iff forbidding each matched pair in turn makes the best total gain drop."""
    for r, c in pairs:
        g = [list(row) for row in gain]
        g[r][c] = None
        if not max_gain_matching(g)[1] < total:
            return False
    return True


# ---- the tracker ---------------------------------------------------------------------------------------------------------
class DeepSortRef:
    """One stream.  ``update(xyxy, conf, cls, desc)`` advances a frame; ``snapshot()`` is the parity surface
    (= rtmodt_deepsort_state).  ``record`` (a list) receives, per matching problem solved, a dict with the gain matrix, the
    pairs and the raw costs -- what the CPU tests re-check with SciPy and for uniqueness."""

    def __init__(self, max_dist=0.2, min_confidence=0.3, max_iou_distance=0.7, max_age=70, n_init=3, nn_budget=100, dim=DIM, record=None):
        self.max_dist, self.min_confidence, self.max_iou_distance = float(max_dist), float(min_confidence), float(max_iou_distance)
        self.max_age, self.n_init, self.nn_budget, self.dim = int(max_age), int(n_init), int(nn_budget), int(dim)
        self.thr = math.floor(self.max_dist * DOT_ONE)
        self.record = record
        self.next_id = 1
        self.ids, self.state, self.hits, self.age, self.tsu = [], [], [], [], []
        self.box, self.conf, self.cls = [], [], []
        self.mean = np.zeros((0, 8), F32)
        self.cov = np.zeros((0, 12), F32)
        self.gallery = []                                  # per track: list of int8 rows, oldest first, at most nn_budget

    # the two cost rules
    def appearance_gain(self, rows, cols, d2, dm):
        gain = [[None] * len(cols) for _ in rows]
        cost = np.full((len(rows), len(cols)), -1, np.int64)
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                c = max(0, DOT_ONE - int(dm[i, j]))
                cost[a, b] = c
                if not (d2[i, j] > GATE) and c <= self.thr:
                    gain[a][b] = self.thr + 1 - c
        return gain, cost

    def iou_gain(self, rows, cols, iou):
        limit = self.max_iou_distance + 1e-5
        gain = [[None] * len(cols) for _ in rows]
        cost = np.zeros((len(rows), len(cols)), np.float64)
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                cd = float(F32(1) - iou[i, j])
                cost[a, b] = cd
                if cd <= self.max_iou_distance:
                    gain[a][b] = limit - cd
        return gain, cost

    def _solve(self, kind, gain, cost, rows, cols):
        pairs, total = max_gain_matching(gain)
        if self.record is not None:
            self.record.append({"kind": kind, "gain": gain, "cost": cost, "pairs": pairs, "total": total})
        return [(rows[r], cols[c]) for r, c in pairs]

    def update(self, xyxy, conf, cls, desc):
        xyxy = np.asarray(xyxy, F32).reshape(-1, 4)
        conf = np.asarray(conf, F32).reshape(-1)
        cls = np.asarray(cls, np.int32).reshape(-1)
        desc = np.asarray(desc, np.int8).reshape(-1, self.dim)
        M = len(self.ids)
        # predict
        if M:
            self.mean, self.cov = K.kf_predict(self.mean, self.cov)
        self.age = [a + 1 for a in self.age]
        self.tsu = [t + 1 for t in self.tsu]
        # filter
        keep = np.nonzero(conf >= F32(self.min_confidence))[0]
        xyxy, conf, cls, desc = xyxy[keep], conf[keep], cls[keep], desc[keep]
        nd = len(keep)
        z = K.xyxy_to_xyah(xyxy) if nd else np.zeros((0, 4), F32)
        t_match = [-1] * M
        d_match = [-1] * nd
        if M and nd:
            d2 = gating_d2(self.mean, self.cov, z)
            g = np.zeros((M, self.nn_budget, self.dim), np.int8)
            for i in range(M):
                g[i, :len(self.gallery[i])] = np.stack(self.gallery[i])
            dm = dotmax(g, [len(x) for x in self.gallery], desc)
            for level in range(1, self.max_age + 1):
                rows = [i for i in range(M) if self.state[i] == CONFIRMED and self.tsu[i] == level]
                cols = [j for j in range(nd) if d_match[j] < 0]
                if not rows:
                    continue
                if not cols:
                    break
                gain, cost = self.appearance_gain(rows, cols, d2, dm)
                for i, j in self._solve("appearance", gain, cost, rows, cols):
                    t_match[i], d_match[j] = j, i
            rows = [i for i in range(M) if t_match[i] < 0 and (self.state[i] == TENTATIVE or self.tsu[i] == 1)]
            cols = [j for j in range(nd) if d_match[j] < 0]
            if rows and cols:
                iou = batch_iou(K.xyah_to_xyxy(self.mean[:, :4]), xyxy)
                gain, cost = self.iou_gain(rows, cols, iou)
                for i, j in self._solve("iou", gain, cost, rows, cols):
                    t_match[i], d_match[j] = j, i
        # life cycle
        alive = []
        for i in range(M):
            j = t_match[i]
            if j >= 0:
                m, c = K.kf_update(self.mean[i:i + 1], self.cov[i:i + 1], z[j:j + 1])
                self.mean[i], self.cov[i] = m[0], c[0]
                self.gallery[i] = (self.gallery[i] + [desc[j].copy()])[-self.nn_budget:]
                self.hits[i] += 1
                self.tsu[i] = 0
                if self.state[i] == TENTATIVE and self.hits[i] >= self.n_init:
                    self.state[i] = CONFIRMED
                self.box[i], self.conf[i], self.cls[i] = xyxy[j].copy(), conf[j], int(cls[j])
                alive.append(i)
            elif self.state[i] == CONFIRMED and self.tsu[i] <= self.max_age:
                alive.append(i)
        for name in ("ids", "state", "hits", "age", "tsu", "box", "conf", "cls", "gallery"):
            setattr(self, name, [getattr(self, name)[i] for i in alive])
        self.mean, self.cov = self.mean[alive], self.cov[alive]
        for j in range(nd):
            if d_match[j] >= 0:
                continue
            m, c = K.kf_initiate(z[j:j + 1])
            self.mean, self.cov = np.concatenate([self.mean, m]), np.concatenate([self.cov, c])
            self.ids.append(self.next_id)
            self.next_id += 1
            self.state.append(TENTATIVE)
            self.hits.append(1)
            self.age.append(1)
            self.tsu.append(0)
            self.box.append(xyxy[j].copy())
            self.conf.append(conf[j])
            self.cls.append(int(cls[j]))
            self.gallery.append([desc[j].copy()])
        return [i for i in range(len(self.ids)) if self.state[i] == CONFIRMED and self.tsu[i] == 0]

    def snapshot(self) -> dict:
        n = len(self.ids)
        gal = np.zeros((n, self.nn_budget, self.dim), np.int8)
        for i in range(n):
            gal[i, :len(self.gallery[i])] = np.stack(self.gallery[i])
        return {"ids": np.asarray(self.ids, np.int64), "state": np.asarray(self.state, np.int32), "hits": np.asarray(self.hits, np.int32),
                "age": np.asarray(self.age, np.int32), "tsu": np.asarray(self.tsu, np.int32),
                "xyxy": np.asarray(self.box, F32).reshape(n, 4), "conf": np.asarray(self.conf, F32), "cls": np.asarray(self.cls, np.int32),
                "mean": self.mean.copy(), "cov": self.cov.copy(), "gallery_count": np.asarray([len(g) for g in self.gallery], np.int32),
                "gallery": gal, "next_id": self.next_id}

    def tracks_out(self, idx):
        """What DeepSortTracker.update returns for these indices: (track id, posterior mean box)."""
        boxes = K.xyah_to_xyxy(self.mean[:, :4]) if len(self.ids) else np.zeros((0, 4), F32)
        return [(self.ids[i], boxes[i]) for i in idx]


def snapshots_equal(a: dict, b: dict):
    """None when two snapshots agree bit for bit, else the name of the first field that differs."""
    if a["next_id"] != b["next_id"]:
        return "next_id"
    for k in ("ids", "state", "hits", "age", "tsu", "cls", "gallery_count", "gallery"):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            return k
    for k in ("xyxy", "conf", "mean", "cov"):
        x, y = np.ascontiguousarray(a[k], F32), np.ascontiguousarray(b[k], F32)
        if x.shape != y.shape or not np.array_equal(x.view(np.int32), y.view(np.int32)):
            return k
    return None


# ---- scenes ----------------------------------------------------------------------------------------------------------------
PALETTE = np.asarray([[230, 40, 40], [40, 230, 40], [40, 40, 230], [230, 230, 40], [230, 40, 230], [40, 230, 230], [250, 250, 250], [120, 20, 200],
                      [20, 120, 200], [200, 120, 20], [90, 200, 90], [200, 90, 90]], np.uint8)


def render_scene(boxes, colours, h, w, seed=0):
    """A noisy grey frame with every box filled by its colour (two-tone: top half lighter) -- later boxes paint over earlier ones."""
    rng = np.random.default_rng(seed)
    frame = rng.integers(96, 112, size=(h, w, 3), dtype=np.uint8)
    for b, c in zip(boxes, colours):
        reg = box_region(b, h, w)
        if reg is None:
            continue
        x0, y0, x1, y1 = reg
        ym = (y0 + y1) // 2
        frame[y0:ym, x0:x1] = c
        frame[ym:y1, x0:x1] = c // 2
    return frame


def crossing_scene(n_pairs=3, frames=60, h=360, w=640, size=(40, 80), seed=0):
    """Pairs of differently coloured boxes of equal size that cross at equal and opposite speed along a row: at the crossing the
    two boxes coincide (one detection hides the other for a few frames), then they separate again.  Returns per frame
    (xyxy (n, 4) float32, conf, cls, object ids, colours)."""
    rng = np.random.default_rng(seed)
    bw, bh = size
    out = []
    for f in range(frames):
        boxes, ids, cols = [], [], []
        for p in range(n_pairs):
            y = 30 + p * (bh + 25)
            span = w - bw - 40
            t = f / (frames - 1)
            xa = 20 + span * t
            xb = 20 + span * (1 - t)
            ja, jb = rng.uniform(-0.4, 0.4, 2)
            hidden = abs(xa - xb) < 0.35 * bw                  # the far box is occluded while they overlap this much
            boxes.append([xa + ja, y, xa + ja + bw, y + bh]); ids.append(2 * p); cols.append(PALETTE[(2 * p) % len(PALETTE)])
            if not hidden:
                boxes.append([xb + jb, y, xb + jb + bw, y + bh]); ids.append(2 * p + 1); cols.append(PALETTE[(2 * p + 1) % len(PALETTE)])
        xy = np.asarray(boxes, F32).reshape(-1, 4)
        out.append((xy, np.full(len(xy), 0.9, F32), np.zeros(len(xy), np.int32), np.asarray(ids), np.asarray(cols, np.uint8).reshape(-1, 3)))
    return out, h, w


def random_scene(seed, frames=40, n_obj=5, h=240, w=320, gaps=(), spurious=0.0, lowconf=0.0, speed=2.0, size=(24, 48)):
    """n_obj coloured boxes in constant-velocity motion (with jitter); ``gaps`` = (object, first frame, length) detection drop-outs;
    ``spurious`` = per-frame probability of a one-off detection; ``lowconf`` = probability that a detection's confidence falls
    below 0.3 (some exactly at float32(0.3)).  Same return as crossing_scene."""
    rng = np.random.default_rng(seed)
    bw, bh = size
    pos = np.stack([rng.uniform(10, w - bw - 10, n_obj), rng.uniform(10, h - bh - 10, n_obj)], 1)
    vel = rng.uniform(-speed, speed, (n_obj, 2))
    colours = np.asarray([PALETTE[k % len(PALETTE)] for k in range(n_obj)], np.uint8)
    out = []
    for f in range(frames):
        boxes, ids, cols, confs = [], [], [], []
        for k in range(n_obj):
            p = pos[k] + vel[k] * f + rng.uniform(-0.5, 0.5, 2)
            if any(o == k and a <= f < a + n for o, a, n in gaps):
                continue
            boxes.append([p[0], p[1], p[0] + bw, p[1] + bh]); ids.append(k); cols.append(colours[k])
            u = rng.uniform()
            confs.append(0.9 if u >= lowconf else (0.3 if u < lowconf / 3 else rng.uniform(0.05, 0.29)))
        if rng.uniform() < spurious:
            p = [rng.uniform(0, w - bw), rng.uniform(0, h - bh)]
            boxes.append([p[0], p[1], p[0] + bw * 0.8, p[1] + bh * 0.8]); ids.append(100 + f)
            cols.append(rng.integers(0, 255, 3).astype(np.uint8)); confs.append(0.8)
        xy = np.asarray(boxes, F32).reshape(-1, 4)
        out.append((xy, np.asarray(confs, F32), (np.asarray(ids, np.int32) % 3).astype(np.int32), np.asarray(ids),
                    np.asarray(cols, np.uint8).reshape(-1, 3)))
    return out, h, w


# The sequences of the GPU suite (tests/test_gpu_deepsort.py): SEQUENCES (described on rendered frames) and EMBEDDED (caller
# descriptors of another dimension).  tests/test_deepsort_cpu.py proves every assignment optimum on every frame of each of them
# unique, so that "the" optimum the kernel must find is well defined.  Two GPU tests are outside that proof because their
# detections exist only on a GPU (they come out of the detector: update_from_detector, pipeline.run); one of them compares the two
# ways of feeding one handle's kernels with each other and with the restatement, the other checks the loop's plumbing.
#   name -> (tracker parameters, scene factory)
SEQUENCES = {
    "crossing": (dict(max_age=30, n_init=3, nn_budget=100), lambda: crossing_scene(3, 110, seed=3)),
    "occlusion": (dict(max_age=5, n_init=2, nn_budget=100),
                  lambda: random_scene(11, 44, 5, gaps=((0, 8, 3), (1, 10, 4), (2, 12, 5), (3, 14, 9), (4, 6, 30)))),
    "lifecycle": (dict(max_age=8, n_init=3, nn_budget=100), lambda: random_scene(21, 36, 4, gaps=((0, 1, 4), (1, 2, 3)), spurious=0.5)),
    "budget": (dict(max_age=10, n_init=2, nn_budget=4), lambda: random_scene(31, 30, 3)),
    "min_confidence": (dict(max_age=6, n_init=2, nn_budget=16), lambda: random_scene(42, 36, 6, lowconf=0.3)),
}
SEQUENCES["tiny"] = (dict(max_age=3, n_init=1, nn_budget=3), lambda: random_scene(61, 8, 3))      # run at odd capacities (5 tracks, 3 detections)
for _k in range(8):                                      # the 8 streams of one call: ragged object counts
    SEQUENCES[f"stream{_k}"] = (dict(max_age=6, n_init=2, nn_budget=8),
                                lambda _k=_k: random_scene(50 + _k, 24, 1 + (_k * 3) % 7, gaps=((0, 5 + _k, 2 + _k),), spurious=0.2, lowconf=0.1))


def sequence_inputs(name):
    """(parameters, list of per-frame (frame image, xyxy, conf, cls, object ids))."""
    params, factory = SEQUENCES[name]
    scene, h, w = factory()
    return params, [(render_scene(xy, col, h, w, seed=1000 + f), xy, cf, cl, ids) for f, (xy, cf, cl, ids, col) in enumerate(scene)]


def embedded_scene(seed=77, frames=30, n_obj=5, dim=64, gaps=((1, 6, 3), (2, 9, 7)), noise=0.05):
    """random_scene with a float embedding per detection instead of pixels: each object has its own direction plus noise."""
    rng = np.random.default_rng(seed + 1000)
    scene, h, w = random_scene(seed, frames, n_obj, gaps=gaps)
    base = rng.normal(0, 1, (200, dim)).astype(np.float32)
    return [(xy, cf, cl, ids, (base[ids % 200] + rng.normal(0, noise, (len(ids), dim))).astype(np.float32)) for xy, cf, cl, ids, _ in scene], h, w


#   name -> (tracker parameters, descriptor dimension, scene factory)
EMBEDDED = {
    "embed64": (dict(max_age=5, n_init=2, nn_budget=6), 64, lambda: embedded_scene()),
}


def embedded_inputs(name):
    """(parameters, dim, list of per-frame (float embeddings, xyxy, conf, cls, object ids))."""
    params, dim, factory = EMBEDDED[name]
    scene, _, _ = factory()
    return params, dim, [(x, xy, cf, cl, ids) for xy, cf, cl, ids, x in scene]


def pair_limit_frames(extra: bool, seed=2048):
    """Two frames that put the IoU stage at the contested-pair limit of csrc/lap.h: frame 1 has 32 detections (33 with ``extra``)
    that become tentative tracks, frame 2 has 64 detections.  Every box is the 40 x 40 box at (10, 10) moved by less than 1 px,
    except the last detection of frame 2, 16 px to the right (IoU 0.35 or more with the 32 tracks: admissible, IoU >= 0.3), so all
    32 x 64 = 2048 pairs are admissible and none is isolated.  The extra track sits 32 px to the right: admissible with that last
    detection alone (IoU 0.37 or more; 0.15 or less with the others), the 2049th pair.  Caller descriptors (no track is confirmed:
    the appearance cascade has no rows).  Returns (tracker parameters, [(xyxy, conf, cls, int8 descriptors) per frame])."""
    rng = np.random.default_rng(seed)

    def boxes(n, dx=0.0):
        j = rng.uniform(-1, 1, (n, 2)) + np.asarray([dx, 0.0])
        return np.concatenate([10 + j, 50 + j], axis=1).astype(F32)

    f1 = boxes(32)
    if extra:
        f1 = np.concatenate([f1, boxes(1, 32.0)])
    f2 = np.concatenate([boxes(63), boxes(1, 16.0)])
    out = []
    for b in (f1, f2):
        out.append((b, np.full(len(b), 0.9, F32), np.zeros(len(b), np.int32), rng.integers(-127, 128, (len(b), DIM)).astype(np.int8)))
    return dict(max_age=3, n_init=3, nn_budget=4), out
