"""Plain-Python restatement of the OC-SORT tracker of ``csrc/ocsort.hip`` -- TEST INFRASTRUCTURE, written rule by rule as the kernel's
header comment reads.  Slow by design: one float32 operation per line where the rounding matters.

The algorithm is the published one (Cao et al., "Observation-Centric SORT", CVPR 2023; its ``ocsort.py`` / ``association.py`` /
``kalmanfilter.py``) as this project reads it.  PARITY UNPINNED: ``ocsort``, ``boxmot`` and ``filterpy`` are installed nowhere this
runs, so nothing here is checked against those libraries; ``tests/test_ocsort_cpu.py`` checks the pieces against independent forms
instead (a dense 7x7 float64 Kalman filter, SciPy's Hungarian method on the dense gain matrix, ``math.acos``).  Known differences
from the published code, all deliberate: pairs are gated by IoU before the assignment (the published code runs the Hungarian method
on the dense matrix and drops pairs below the threshold afterwards); the covariance update is ``P - K H P`` (filterpy's Joseph form
rounds differently); everything is float32 with one rounding per operation except the gain, which is float64.

The switches ``ocm`` / ``ocr`` / ``oru`` exist only here: ``tests/test_ocsort_cpu.py`` turns each off on a scene built for it and
shows that the final identities change, so the GPU test on the same scene is known to exercise that component.
"""
from __future__ import annotations

import numpy as np

from oracle.tracker_oracle import batch_iou

F32 = np.float32
PI = float.fromhex("0x1.921fb54442d18p+1")
HALF_PI = float.fromhex("0x1.921fb54442d18p+0")
# asin(x) = x + x * z * P(z), z = x^2: the Taylor coefficients (2k)! / (4^k k!^2 (2k + 1)), k = 1..22, each rounded once to float64
ASIN_C = tuple(float.fromhex(h) for h in (
    "0x1.5555555555555p-3", "0x1.3333333333333p-4", "0x1.6db6db6db6db7p-5", "0x1.f1c71c71c71c7p-6", "0x1.6e8ba2e8ba2e9p-6",
    "0x1.1c4ec4ec4ec4fp-6", "0x1.c99999999999ap-7", "0x1.7a87878787878p-7", "0x1.3fde50d79435ep-7", "0x1.12ef3cf3cf3cfp-7",
    "0x1.df3bd37a6f4dfp-8", "0x1.a6863d70a3d71p-8", "0x1.782dda12f684cp-8", "0x1.51ba308d3dcb1p-8", "0x1.31683bdef7bdfp-8",
    "0x1.15ee9d45d1746p-8", "0x1.fcaf8fb6db6dbp-9", "0x1.d3d2a8e0dd67dp-9", "0x1.b026f57b13b14p-9", "0x1.90cb77f60c7cep-9",
    "0x1.750de64d7d05fp-9", "0x1.5c5f56efaaaabp-9"))
RING = 8                                   # observation ring slots = the largest delta_t
P0_POS, P0_VEL = F32(10), F32(1e4)
Q_POS = F32(1)
Q_VEL = (F32(1e-2), F32(1e-2), F32(1e-4), F32(0))
R_MEAS = (F32(1), F32(1), F32(10), F32(10))
EPS = F32(1e-6)
HALF = F32(0.5)


# ---- the fixed-sequence acos (csrc/track_dev.h: acos_fixed) -------------------------------------------------------------
def _asin_poly(z: float) -> float:
    p = ASIN_C[-1]
    for c in ASIN_C[-2::-1]:
        p = c + z * p
    return p


def acos_fixed(c) -> float:
    """acos of a float32 in [-1, 1], in float64 additions, multiplications and divisions only (each correctly rounded by any IEEE
    build, no libm call, no float64 square root):
      |x| <= 0.5   pi/2 - (x + x * (z * P(z))), z = x * x
      |x| >  0.5   t = (1 - |x|) * 0.5 (exact); s = sqrt(t) by two Newton steps y = 0.5 * (y + t / y) from the float32 square root
                   of float32(t); 2 * (s + s * (t * P(t))), reflected to pi - that for x < 0."""
    x = float(c)
    a = abs(x)
    if a <= 0.5:
        z = x * x
        return HALF_PI - (x + x * (z * _asin_poly(z)))
    t = (1.0 - a) * 0.5
    if t == 0.0:
        s = 0.0
    else:
        y = float(np.sqrt(F32(t)))
        y = 0.5 * (y + t / y)
        y = 0.5 * (y + t / y)
        s = y
    r = s + s * (t * _asin_poly(t))
    ac = 2.0 * r
    return PI - ac if x < 0.0 else ac


# ---- float32 pieces -----------------------------------------------------------------------------------------------------
def box_to_z(b):
    """xyxy -> (x, y, s, r) with r = w / (h + 1e-6)."""
    w, h = F32(b[2] - b[0]), F32(b[3] - b[1])
    return np.asarray([F32(b[0] + F32(w * HALF)), F32(b[1] + F32(h * HALF)), F32(w * h), F32(w / F32(h + EPS))], F32)


def state_to_box(m):
    """(x, y, s, r) -> xyxy: w = sqrt(s * r), h = s / w."""
    w = F32(np.sqrt(F32(m[2] * m[3])))
    h = F32(m[2] / w)
    hw, hh = F32(w * HALF), F32(h * HALF)
    return np.asarray([F32(m[0] - hw), F32(m[1] - hh), F32(m[0] + hw), F32(m[1] + hh)], F32)


def direction(b1, b2):
    """Unit direction (dy, dx) from the centre of b1 to the centre of b2."""
    cx1, cy1 = F32(F32(b1[0] + b1[2]) * HALF), F32(F32(b1[1] + b1[3]) * HALF)
    cx2, cy2 = F32(F32(b2[0] + b2[2]) * HALF), F32(F32(b2[1] + b2[3]) * HALF)
    dx, dy = F32(cx2 - cx1), F32(cy2 - cy1)
    norm = F32(F32(np.sqrt(F32(F32(dx * dx) + F32(dy * dy)))) + EPS)
    return np.asarray([F32(dy / norm), F32(dx / norm)], F32)


def kf_init(z):
    mean = np.zeros(8, F32)
    mean[:4] = z
    cov = np.zeros(12, F32)                 # per lane (a, b, c): [[a, b], [b, c]] of (position, velocity); lane 3 (r) has no velocity
    for k in range(4):
        cov[3 * k] = P0_POS
        cov[3 * k + 2] = P0_VEL if k < 3 else F32(0)
    return mean, cov


def kf_predict(mean, cov):
    """F P F' + Q per (position, velocity) pair: csrc/track_dev.h kf_predict1 with the constant noises of SORT."""
    mean, cov = mean.copy(), cov.copy()
    for k in range(4):
        a0, b0, c0 = cov[3 * k], cov[3 * k + 1], cov[3 * k + 2]
        mean[k] = F32(mean[k] + mean[4 + k])
        cov[3 * k] = F32(F32(F32(a0 + F32(b0 + b0)) + c0) + Q_POS)
        cov[3 * k + 1] = F32(b0 + c0)
        cov[3 * k + 2] = F32(c0 + Q_VEL[k])
    return mean, cov


def kf_update(mean, cov, z):
    """csrc/track_dev.h kf_update1 with R = diag(1, 1, 10, 10): the P - K H P form."""
    mean, cov = mean.copy(), cov.copy()
    for k in range(4):
        a0, b0, c0 = cov[3 * k], cov[3 * k + 1], cov[3 * k + 2]
        s = F32(a0 + R_MEAS[k])
        k0, k1 = F32(a0 / s), F32(b0 / s)
        y = F32(z[k] - mean[k])
        mean[k] = F32(mean[k] + F32(k0 * y))
        mean[4 + k] = F32(mean[4 + k] + F32(k1 * y))
        cov[3 * k] = F32(a0 - F32(k0 * a0))
        cov[3 * k + 1] = F32(b0 - F32(k0 * b0))
        cov[3 * k + 2] = F32(c0 - F32(k1 * b0))
    return mean, cov


# ---- exact maximum-gain matching -----------------------------------------------------------------------------------------
def _hungarian(gain):
    """deepsort_ref.max_gain_matching restated for float gains: the Hungarian method on the matrix padded with zero-gain dummies."""
    m, n = len(gain), len(gain[0])
    size = m + n
    INF = float("inf")
    cost = [[None] * size for _ in range(size)]
    for r in range(size):
        for c in range(size):
            if r < m and c < n:
                cost[r][c] = None if gain[r][c] is None else -gain[r][c]
            elif r < m:
                cost[r][c] = 0.0 if c - n == r else None
            elif c < n:
                cost[r][c] = 0.0 if r - m == c else None
            else:
                cost[r][c] = 0.0
    u, v, p, way = [0.0] * (size + 1), [0.0] * (size + 1), [0] * (size + 1), [0] * (size + 1)
    for i in range(1, size + 1):
        p[0] = i
        j0 = 0
        minv, used = [INF] * (size + 1), [False] * (size + 1)
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
                        minv[j], way[j] = cur, j0
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
    return sorted((p[j] - 1, j - 1) for j in range(1, n + 1) if 1 <= p[j] <= m)


def components(gain):
    """Connected components of the admissible-pair graph: [(rows, cols)] with at least one pair each."""
    m = len(gain)
    n = len(gain[0]) if m else 0
    parent = list(range(m + n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for r in range(m):
        for c in range(n):
            if gain[r][c] is not None:
                parent[find(r)] = find(m + c)
    groups = {}
    for r in range(m):
        if any(g is not None for g in gain[r]):
            groups.setdefault(find(r), ([], []))[0].append(r)
    for c in range(n):
        root = find(m + c)
        if root in groups and any(gain[r][c] is not None for r in groups[root][0]):
            groups[root][1].append(c)
    return list(groups.values())


def max_gain_matching(gain):
    """gain[r][c]: a float > 0 for an admissible pair, None otherwise.  (pairs, total) of a matching of maximum total gain, solved
    component by component (an isolated pair is matched outright)."""
    pairs = []
    for rows, cols in components(gain):
        if len(rows) == 1 and len(cols) == 1:
            pairs.append((rows[0], cols[0]))
            continue
        sub = [[gain[r][c] for c in cols] for r in rows]
        pairs += [(rows[a], cols[b]) for a, b in _hungarian(sub)]
    pairs.sort()
    return pairs, sum(gain[r][c] for r, c in pairs)


def optimum_margin(gain, pairs):
    """Total gain of the optimum minus that of the best matching that lacks one of its pairs (inf when nothing is matched): every
    other matching lacks at least one pair of a unique optimum, so a positive margin is uniqueness and its size is what summation
    order would have to overcome to change a match."""
    margin = float("inf")
    matched = dict(pairs)
    for rows, cols in components(gain):
        sub = [[gain[r][c] for c in cols] for r in rows]
        best = sum(gain[r][matched[r]] for r in rows if r in matched)
        for a, r in enumerate(rows):
            if r not in matched:
                continue
            b = cols.index(matched[r])
            keep = sub[a][b]
            sub[a][b] = None
            alt = sum(sub[x][y] for x, y in _hungarian(sub)) if len(rows) * len(cols) > 1 else 0.0
            sub[a][b] = keep
            margin = min(margin, best - alt)
    return margin


# ---- the tracker ---------------------------------------------------------------------------------------------------------
class _Trk:
    __slots__ = ("id", "hits", "streak", "age", "tsu", "box", "conf", "cls", "mean", "cov", "dir", "obs", "saved", "pbox")


class OcSortRef:
    """One stream.  ``update(xyxy, conf, cls)`` advances a frame and returns the indices of the returned tracks; ``snapshot()`` is
    the parity surface (= rtmodt_ocsort_state).  ``record`` (a list) receives, per matching problem solved, a dict with the stage,
    the frame, the gain matrix and the pairs -- what the CPU tests re-check with SciPy and for a unique optimum."""

    def __init__(self, det_thresh=0.6, low_thresh=0.1, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3, inertia=0.2, use_byte=False,
                 ocm=True, ocr=True, oru=True, record=None):
        if not 1 <= int(delta_t) <= RING:
            raise ValueError("delta_t 1..8")
        if not float(F32(iou_threshold)) > float(inertia) / 2:
            raise ValueError("iou_threshold must exceed inertia / 2")
        self.det_thresh, self.low_thresh, self.iou_threshold = F32(det_thresh), F32(low_thresh), F32(iou_threshold)
        self.max_age, self.min_hits, self.delta_t, self.inertia, self.use_byte = int(max_age), int(min_hits), int(delta_t), float(inertia), bool(use_byte)
        self.ocm, self.ocr, self.oru, self.record = ocm, ocr, oru, record
        self.next_id, self.frame_count = 1, 0
        self.tracks = []

    # the reference observation of steps 4 and 7: age - delta_t, else the nearest later stored age below age, else the newest
    def _reference(self, t):
        for dt in range(self.delta_t, 0, -1):
            if t.age - dt in t.obs:
                return t.obs[t.age - dt]
        return t.box

    def _solve(self, stage, gain, rows, cols):
        pairs, total = max_gain_matching(gain) if rows and cols else ([], 0.0)
        if self.record is not None and rows and cols:
            self.record.append({"stage": stage, "frame": self.frame_count, "gain": gain, "pairs": pairs, "total": total})
        return [(rows[r], cols[c]) for r, c in pairs]

    def _iou_gain(self, boxes, rows, cols, dets):
        gain = [[None] * len(cols) for _ in rows]
        if rows and cols:
            iou = batch_iou(np.asarray([boxes[i] for i in rows], F32), dets[cols])
            for a, b in zip(*np.nonzero(iou >= self.iou_threshold)):
                gain[a][b] = float(iou[a, b])
        return gain

    def update(self, xyxy, conf, cls):
        with np.errstate(all="ignore"):
            return self._update(np.asarray(xyxy, F32).reshape(-1, 4), np.asarray(conf, F32).reshape(-1), np.asarray(cls, np.int32).reshape(-1))

    def _update(self, xyxy, conf, cls):
        self.frame_count += 1
        # 1. split
        high = [j for j in range(len(conf)) if conf[j] > self.det_thresh]
        low = [j for j in range(len(conf)) if conf[j] > self.low_thresh and conf[j] < self.det_thresh] if self.use_byte else []
        # 2./3. predict
        T = self.tracks
        alive = []
        for i, t in enumerate(T):
            if F32(t.mean[2] + t.mean[6]) <= F32(0):
                t.mean[6] = F32(0)
            t.mean, t.cov = kf_predict(t.mean, t.cov)
            t.age += 1
            if t.tsu > 0:
                t.streak = 0
            t.tsu += 1
            t.pbox = state_to_box(t.mean)
            if np.isfinite(t.pbox).all():
                alive.append(i)
        t_match = {}
        d_used = set()
        pbox = {i: T[i].pbox for i in alive}
        ref = {i: self._reference(T[i]) for i in alive if T[i].hits > 0}
        # 4. observation-centric momentum
        rows, cols = list(alive), list(high)
        gain = [[None] * len(cols) for _ in rows]
        iou = batch_iou(np.asarray([pbox[i] for i in rows], F32), xyxy[cols]) if rows and cols else np.zeros((0, 0), F32)
        for a, b in zip(*np.nonzero(iou >= self.iou_threshold)):
            i, j = rows[a], cols[b]
            angle = 0.0
            if self.ocm and i in ref:
                d = direction(ref[i], xyxy[j])
                c = F32(F32(T[i].dir[1] * d[1]) + F32(T[i].dir[0] * d[0]))
                c = min(max(c, F32(-1)), F32(1))
                angle = ((HALF_PI - acos_fixed(c)) / PI) * self.inertia * float(conf[j])
            if float(iou[a, b]) + angle > 0.0:               # (always, for conf <= 1: iou_threshold > inertia / 2)
                gain[a][b] = float(iou[a, b]) + angle
        for i, j in self._solve("ocm", gain, rows, cols):
            t_match[i] = j
            d_used.add(j)
        # 5. BYTE
        if self.use_byte:
            rows, cols = [i for i in alive if i not in t_match], list(low)
            for i, j in self._solve("byte", self._iou_gain(pbox, rows, cols, xyxy), rows, cols):
                t_match[i] = j
                d_used.add(j)
        # 6. observation-centric recovery
        if self.ocr:
            rows, cols = [i for i in alive if i not in t_match and T[i].hits > 0], [j for j in high if j not in d_used]
            last = {i: T[i].box for i in rows}
            for i, j in self._solve("ocr", self._iou_gain(last, rows, cols, xyxy), rows, cols):
                t_match[i] = j
                d_used.add(j)
        # 7. update
        kept = []
        for i in alive:
            t = T[i]
            if i in t_match:
                z = xyxy[t_match[i]]
                if t.hits > 0:
                    t.dir = direction(ref[i], z)
                    if t.tsu >= 2 and self.oru:
                        self._reupdate(t, z)
                t.mean, t.cov = kf_update(t.mean, t.cov, box_to_z(z))
                t.box, t.conf, t.cls = z.copy(), conf[t_match[i]], int(cls[t_match[i]])
                t.obs = {a: b for a, b in t.obs.items() if a > t.age - RING}
                t.obs[t.age] = z.copy()
                t.tsu = 0
                t.hits += 1
                t.streak += 1
            elif t.tsu == 1:
                t.saved = (t.mean.copy(), t.cov.copy())
            if t.tsu <= self.max_age:
                kept.append(t)
        # 8. births
        for j in high:
            if j in d_used:
                continue
            t = _Trk()
            t.id = self.next_id
            self.next_id += 1
            t.hits = t.streak = t.age = t.tsu = 0
            t.box, t.conf, t.cls = xyxy[j].copy(), conf[j], int(cls[j])
            t.mean, t.cov = kf_init(box_to_z(xyxy[j]))
            t.dir = np.zeros(2, F32)
            t.obs, t.saved, t.pbox = {}, None, None
            kept.append(t)
        self.tracks = kept
        # 9. returned
        return [i for i, t in enumerate(kept) if t.tsu == 0 and (t.streak >= self.min_hits or self.frame_count <= self.min_hits)]

    def _reupdate(self, t, z):
        """ORU: from the filter state saved at the first missed frame, walk tsu virtual observations on the line from the last
        observation to z (update, then predict; the last step is update only)."""
        mean, cov = t.saved[0].copy(), t.saved[1].copy()
        b = t.box
        w1, h1 = F32(b[2] - b[0]), F32(b[3] - b[1])
        x1, y1 = F32(b[0] + F32(w1 * HALF)), F32(b[1] + F32(h1 * HALF))
        w2, h2 = F32(z[2] - z[0]), F32(z[3] - z[1])
        x2, y2 = F32(z[0] + F32(w2 * HALF)), F32(z[1] + F32(h2 * HALF))
        g = F32(t.tsu)
        dx, dy, dw, dh = F32(F32(x2 - x1) / g), F32(F32(y2 - y1) / g), F32(F32(w2 - w1) / g), F32(F32(h2 - h1) / g)
        for i in range(1, t.tsu + 1):
            fi = F32(i)
            x, y = F32(x1 + F32(fi * dx)), F32(y1 + F32(fi * dy))
            w, h = F32(w1 + F32(fi * dw)), F32(h1 + F32(fi * dh))
            mean, cov = kf_update(mean, cov, np.asarray([x, y, F32(w * h), F32(w / h)], F32))
            if i < t.tsu:
                mean, cov = kf_predict(mean, cov)
        t.mean, t.cov = mean, cov

    def snapshot(self) -> dict:
        T = self.tracks
        n = len(T)
        return {"ids": np.asarray([t.id for t in T], np.int64), "hits": np.asarray([t.hits for t in T], np.int32),
                "hit_streak": np.asarray([t.streak for t in T], np.int32), "age": np.asarray([t.age for t in T], np.int32),
                "tsu": np.asarray([t.tsu for t in T], np.int32), "xyxy": np.asarray([t.box for t in T], F32).reshape(n, 4),
                "conf": np.asarray([t.conf for t in T], F32), "cls": np.asarray([t.cls for t in T], np.int32),
                "mean": np.asarray([t.mean for t in T], F32).reshape(n, 8), "cov": np.asarray([t.cov for t in T], F32).reshape(n, 12),
                "dir": np.asarray([t.dir for t in T], F32).reshape(n, 2), "next_id": self.next_id, "frame_count": self.frame_count}

    def tracks_out(self, idx):
        """What OcSortTracker.update returns for these indices: (track id, box of the last matched detection)."""
        return [(self.tracks[i].id, self.tracks[i].box) for i in idx]


def snapshots_equal(a: dict, b: dict):
    """None when two snapshots agree bit for bit, else the name of the first field that differs."""
    for k in ("next_id", "frame_count"):
        if a[k] != b[k]:
            return k
    for k in ("ids", "hits", "hit_streak", "age", "tsu", "cls"):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            return k
    for k in ("xyxy", "conf", "mean", "cov", "dir"):
        x, y = np.ascontiguousarray(a[k], F32), np.ascontiguousarray(b[k], F32)
        if x.shape != y.shape or not np.array_equal(x.view(np.int32), y.view(np.int32)):
            return k
    return None


# ---- scenes: every coordinate a multiple of 1/4 px (tests/tracker_cases.py), so shifts and sums of them are exact in float32 -----
def _quarter(a):
    return (np.round(np.asarray(a, np.float64) * 4) / 4).astype(F32)


def _frame(boxes, conf=0.9, cls=0):
    b = _quarter(np.asarray(boxes, np.float64).reshape(-1, 4))
    c = np.full(len(b), conf, F32) if np.isscalar(conf) else np.asarray(conf, F32)
    k = np.full(len(b), cls, np.int32) if np.isscalar(cls) else np.asarray(cls, np.int32)
    return b, c, k


def ocm_scene(va=4, vb=4, w=24, n=12, jit=6):
    """Object A moves right along y = 100, object B moves down the column A reaches at frame n / 2: there both detections sit on
    one another but for `jit` px (A's along x, B's along y), so the IoU with the two predictions is ambiguous and alone prefers the
    exchange; the directions from the reference observations (right for A, down for B) separate them."""
    out = []
    for f in range(n):
        ax, ay = 10 + va * f, 100.0
        bx, by = 10 + va * (n // 2), 100 - vb * (n // 2) + vb * f
        j = jit if f == n // 2 else 0
        out.append(_frame([[ax + j, ay, ax + j + w, ay + w], [bx, by + j, bx + w, by + j + w]]))
    return out


def ocr_scene(speeds=(4, 8, 12, 16, 16, 16, 16), w=24, halt=3):
    """An object that accelerates to 16 px a frame (box 24 px wide) and then halts: the prediction runs on by about its width, so its
    IoU with the detection is below 0.3, while the last observation is the detection itself."""
    out, x = [], 10.0
    for v in speeds:
        x += v
        out.append(_frame([[x, 50, x + w, 50 + 2 * w]]))
    for _ in range(halt):
        out.append(_frame([[x, 50, x + w, 50 + 2 * w]]))
    return out


def oru_scene(v=8, w=32, gap=2, decoy=16, n=8, tail=3):
    """An object moves right at v px a frame, is lost for `gap` frames in which it halts, and is found again where it was last seen
    (by the recovery stage).  From the next frame on a second object appears ahead of it, where the velocity from before the gap
    points: the re-update has replaced that velocity by the one of the virtual path (none), and the track stays on its object."""
    out, x, y = [], 10.0, 50.0
    for f in range(n):
        out.append(_frame([[x + v * f, y, x + v * f + w, y + w]]))
    xs = x + v * (n - 1)
    out += [_frame([])] * gap
    out.append(_frame([[xs, y, xs + w, y + w]]))
    for f in range(tail):
        xd = xs + decoy * (f + 1)
        out.append(_frame([[xs, y, xs + w, y + w], [xd, y, xd + w, y + w]]))
    return out


def motion_scene(seed, frames=30, n_obj=5, gaps=(), spurious=0.0, lowconf=0.0, speed=3.0, size=(24, 48), pitch=120, empty=()):
    """n_obj boxes in constant-velocity motion, each starting in its own cell of a `pitch`-px grid; ``gaps`` = (object, first frame,
    length) detection drop-outs; ``spurious`` = per-frame probability of a one-off detection; ``lowconf`` = probability that a
    detection's confidence is not high (a third of those exactly at float32(0.6) or float32(0.1), the rest in between);
    ``empty`` = frames without any detection."""
    rng = np.random.default_rng(seed)
    bw, bh = size
    side = int(np.ceil(np.sqrt(n_obj)))
    cell = rng.permutation(side * side)[:n_obj]
    pos = np.stack([(cell % side) * pitch + rng.uniform(20, 40, n_obj), (cell // side) * pitch + rng.uniform(20, 40, n_obj)], 1)
    vel = rng.uniform(-speed, speed, (n_obj, 2))
    wh = np.stack([bw + rng.uniform(-4, 4, n_obj), bh + rng.uniform(-4, 4, n_obj)], 1)
    out = []
    for f in range(frames):
        boxes, confs, cls = [], [], []
        for k in range(n_obj):
            p = pos[k] + vel[k] * f + rng.uniform(-0.75, 0.75, 2)
            u = rng.uniform()
            if f in empty or any(o == k and a <= f < a + n for o, a, n in gaps):
                continue
            boxes.append([p[0], p[1], p[0] + wh[k, 0], p[1] + wh[k, 1]])
            cls.append(k % 3)
            confs.append(0.9 if u >= lowconf else (0.6 if u < lowconf / 6 else 0.1 if u < lowconf / 3 else rng.uniform(0.15, 0.55)))
        if rng.uniform() < spurious and f not in empty:
            p = [rng.uniform(0, side * pitch), rng.uniform(0, side * pitch)]
            boxes.append([p[0], p[1], p[0] + bw * 0.75, p[1] + bh * 0.75])
            cls.append(3)
            confs.append(0.8)
        out.append(_frame(boxes, confs, cls))
    return out


def big_scene(n_obj=250, n_low=700, frames=3, seed=5):
    """250 objects (no multiple of 64) one per cell of a 96-px grid, each drifting by whole quarter pixels, plus `n_low` detections
    of confidence 0.05 (below low_thresh: they fill detection slots and belong to neither set) and a few pairs of objects in one
    cell close enough to contest one another's detections."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_obj)))
    cell = rng.permutation(side * side)[:n_obj]
    pos = np.stack([(cell % side) * 96.0 + rng.uniform(4, 8, n_obj), (cell // side) * 96.0 + rng.uniform(4, 8, n_obj)], 1)
    pos[1::50] = pos[0::50] + np.asarray([10.0, 6.0])        # five contested neighbours
    wh = rng.uniform(28, 40, (n_obj, 2))
    vel = _quarter(rng.uniform(-1.5, 1.5, (n_obj, 2)))
    out = []
    for f in range(frames):
        p = pos + vel * f
        boxes = np.concatenate([p, p + wh], 1)
        lows = rng.uniform(0, side * 96.0, (n_low, 2))
        boxes = np.concatenate([boxes, np.concatenate([lows, lows + 20], 1)])
        conf = np.concatenate([np.full(n_obj, 0.9), np.full(n_low, 0.05)])
        order = rng.permutation(len(boxes))
        out.append(_frame(boxes[order], conf[order], (order % 5).astype(np.int32)))
    return out


def pair_limit_frames(extra: bool, seed=2048):
    """Two frames that put the first association at the contested-pair limit of csrc/lap.h: frame 1 has 32 detections (33 with
    ``extra``) that become tracks, frame 2 has 64 detections.  Every box is (10, 10, 50, 50) with each corner moved by at most 2 px (no two
    alike), except the last detection of frame 2, 14 px to the right (IoU 0.37 or more with the 32 tracks), so all 32 x 64 = 2048
    pairs are admissible and none is isolated.  The extra track sits 34 px to the right: admissible with that last detection alone
    (IoU 1/3; below 0.1 with the others), the 2049th pair."""
    rng = np.random.default_rng(seed)
    spots, ends = rng.permutation(17 * 17), rng.permutation(17 * 17)

    def boxes(n, first):                                     # both corners move on their own, so sizes differ too: 36 .. 44 px
        k, e = spots[first:first + n], ends[first:first + n]
        return np.concatenate([10 + np.stack([k % 17, k // 17], 1) * 0.25 - 2.0, 50 + np.stack([e % 17, e // 17], 1) * 0.25 - 2.0], axis=1)

    f1 = boxes(32, 0)
    if extra:
        f1 = np.concatenate([f1, [[44.0, 10.0, 84.0, 50.0]]])
    f2 = np.concatenate([boxes(63, 32), [[24.0, 10.0, 64.0, 50.0]]])
    return [_frame(f1), _frame(f2)]


# The sequences of the GPU suite (tests/test_gpu_ocsort.py): name -> (tracker parameters, scene factory).  tests/test_ocsort_cpu.py
# shows on the restatement that every assignment optimum in every frame of each of them is unique with a margin above 1e-9.
_OCC = dict(gaps=((0, 8, 3), (1, 9, 5), (2, 10, 6), (3, 12, 9)))
SEQUENCES = {
    "ocm": (dict(), ocm_scene),
    "ocr": (dict(), ocr_scene),
    "oru": (dict(), oru_scene),
    "occlusion": (dict(max_age=5, min_hits=2), lambda: motion_scene(11, 30, 5, speed=1.5, **_OCC)),
    "lifecycle": (dict(max_age=4, min_hits=3), lambda: motion_scene(21, 30, 4, gaps=((0, 1, 4), (1, 2, 3)), spurious=0.6)),
    "byte_on": (dict(max_age=6, min_hits=2, use_byte=True), lambda: motion_scene(42, 30, 6, lowconf=0.4)),
    "byte_off": (dict(max_age=6, min_hits=2, use_byte=False), lambda: motion_scene(42, 30, 6, lowconf=0.4)),
    "inertia0": (dict(max_age=6, inertia=0.0), lambda: motion_scene(43, 24, 5, gaps=((1, 6, 3),), pitch=60, speed=4.0)),
    "delta_t1": (dict(max_age=6, delta_t=1), lambda: motion_scene(44, 24, 5, gaps=((1, 6, 3),), pitch=60, speed=4.0)),
    "delta_t8": (dict(max_age=12, delta_t=8), lambda: motion_scene(45, 30, 5, gaps=((1, 6, 3), (2, 10, 9)), pitch=60, speed=4.0)),
    "empty": (dict(max_age=3, min_hits=1), lambda: [_frame([])] * 2 + motion_scene(46, 16, 3, empty=(5, 6, 9, 10, 11, 12, 13))),
    "big": (dict(max_age=5), big_scene),
    "limit": (dict(max_age=3), lambda: pair_limit_frames(False)),
}
for _k in range(8):                                      # the 8 streams of one call: ragged object counts and lengths
    SEQUENCES[f"stream{_k}"] = (dict(max_age=6, min_hits=2, use_byte=True),
                                lambda _k=_k: motion_scene(50 + _k, 14 + _k, 1 + (_k * 3) % 7, gaps=((0, 4 + _k, 2 + _k % 3),), spurious=0.3,
                                                           lowconf=0.2))


def sequence_inputs(name):
    """(parameters, list of per-frame (xyxy, conf, cls))."""
    params, factory = SEQUENCES[name]
    return params, factory()
