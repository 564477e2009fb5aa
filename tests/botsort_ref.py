"""Plain-Python restatement of the BoT-SORT tracker of ``csrc/botsort.hip`` -- TEST INFRASTRUCTURE, written rule by rule as the kernel's
header comment reads.  Slow by design: one float32 operation per line where the rounding matters, Python ints for the feature.

The algorithm is the published one (Aharon et al., "BoT-SORT: Robust Associations Multi-Pedestrian Tracking", 2022; its
``bot_sort.py`` / ``kalman_filter.py`` / ``matching.py``) as this project reads it.  PARITY UNPINNED: ``BoT-SORT`` and ``boxmot`` are
installed nowhere this runs, so nothing here is checked against them; ``tests/test_botsort_cpu.py`` checks the pieces against
independent forms instead (a dense 8x8 float64 Kalman filter, SciPy's Hungarian method on the dense gain matrix, hand-worked cases).
Known differences from the published code, all deliberate: one list with a flag instead of three lists; the smoothed feature is an
integer EMA (int16 state at norm 16256, int8 row for the matrix cores); pairs are gated by their cost before the assignment (the
published code solves the dense problem with a cost limit); the covariance update is ``P - K H P``; everything is float32 with one
rounding per operation except the association costs, which are float64.

The switches ``gmc`` / ``reid`` exist only here (``fuse_score`` is a parameter of the tracker itself): ``tests/test_botsort_cpu.py``
turns each off on a scene built for it and shows that the final identities change.
"""
from __future__ import annotations

import math

import numpy as np

import deepsort_ref as DS
import ocsort_ref as OC
from oracle.tracker_oracle import batch_iou

F32 = np.float32
WP, WV = F32(1.0 / 20), F32(1.0 / 160)
W2P, W10V = F32(F32(2) * WP), F32(F32(10) * WV)
HALF = F32(0.5)
DOT_ONE = 127 * 127                        # 16129
FEAT_NORM = 127 * 128                      # 16256: the norm of the int16 feature state
NEW, TRACKED, LOST = 1, 2, 3
SECOND_THRESH, NEW_MATCH_THRESH, DUP_DIST = 0.5, 0.7, 0.15

max_gain_matching = OC.max_gain_matching
optimum_margin = OC.optimum_margin
components = OC.components

# upper triangle of a symmetric 4x4 block, row-major: the order of cov[0:10] (block (cx, cy, vx, vy)) and cov[10:20] ((w, h, vw, vh))
UT = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
UT_INDEX = {rc: k for k, rc in enumerate(UT)}
BLOCK_MEAN = ((0, 1, 4, 5), (2, 3, 6, 7))    # a block's (p0, p1, v0, v1) in the mean (cx, cy, w, h, vx, vy, vw, vh)


def _p(P, r, c):
    return P[UT_INDEX[(r, c) if r <= c else (c, r)]]


# ---- the two-block filter --------------------------------------------------------------------------------------------------
def box_to_xywh(b):
    w, h = F32(b[2] - b[0]), F32(b[3] - b[1])
    return np.asarray([F32(b[0] + F32(w * HALF)), F32(b[1] + F32(h * HALF)), w, h], F32)


def mean_to_box(m):
    x1, y1 = F32(m[0] - F32(m[2] * HALF)), F32(m[1] - F32(m[3] * HALF))
    return np.asarray([x1, y1, F32(x1 + m[2]), F32(y1 + m[3])], F32)


def kf_init(z):
    mean = np.zeros(8, F32)
    mean[:4] = z
    w, h = z[2], z[3]
    sp = (F32(W2P * w), F32(W2P * h))
    sv = (F32(W10V * w), F32(W10V * h))
    blk = np.zeros(10, F32)
    blk[UT_INDEX[(0, 0)]], blk[UT_INDEX[(1, 1)]] = F32(sp[0] * sp[0]), F32(sp[1] * sp[1])
    blk[UT_INDEX[(2, 2)]], blk[UT_INDEX[(3, 3)]] = F32(sv[0] * sv[0]), F32(sv[1] * sv[1])
    return mean, np.concatenate([blk, blk]).astype(F32)


def _blk_predict(x, P, qp, qv):
    """F P F' + Q of one block, F = [[I, I], [0, I]]: A + (B + B') + C, B + C, C in 2x2 parts, each sum left to right as written."""
    x = [F32(x[0] + x[2]), F32(x[1] + x[3]), x[2], x[3]]
    g = lambda r, c: _p(P, r, c)                           # noqa: E731
    out = np.zeros(10, F32)
    out[0] = F32(F32(F32(g(0, 0) + F32(g(0, 2) + g(0, 2))) + g(2, 2)) + qp[0])
    out[1] = F32(F32(g(0, 1) + F32(g(0, 3) + g(1, 2))) + g(2, 3))
    out[4] = F32(F32(F32(g(1, 1) + F32(g(1, 3) + g(1, 3))) + g(3, 3)) + qp[1])
    out[2] = F32(g(0, 2) + g(2, 2))
    out[3] = F32(g(0, 3) + g(2, 3))
    out[5] = F32(g(1, 2) + g(2, 3))
    out[6] = F32(g(1, 3) + g(3, 3))
    out[7] = F32(g(2, 2) + qv[0])
    out[8] = g(2, 3)
    out[9] = F32(g(3, 3) + qv[1])
    return x, out


def kf_predict(mean, cov):
    mean, cov = mean.copy(), cov.copy()
    w, h = mean[2], mean[3]
    sp = (F32(WP * w), F32(WP * h))
    sv = (F32(WV * w), F32(WV * h))
    qp = (F32(sp[0] * sp[0]), F32(sp[1] * sp[1]))
    qv = (F32(sv[0] * sv[0]), F32(sv[1] * sv[1]))
    for b in range(2):
        idx = BLOCK_MEAN[b]
        x, P = _blk_predict([mean[i] for i in idx], cov[10 * b:10 * b + 10], qp, qv)
        for i, v in zip(idx, x):
            mean[i] = v
        cov[10 * b:10 * b + 10] = P
    return mean, cov


def _blk_update(x, P, z, r):
    """One block's update with its 2-vector measurement: S = A + diag(r), the 2x2 inverse by the adjugate (s11 / det, -s01 / det,
    s00 / det, det = s00 s11 - s01 s01), K = P H' S^-1, x + K y, P - K H P on the upper triangle."""
    g = lambda a, b: _p(P, a, b)                           # noqa: E731
    s00, s01, s11 = F32(g(0, 0) + r[0]), g(0, 1), F32(g(1, 1) + r[1])
    det = F32(F32(s00 * s11) - F32(s01 * s01))
    i00, i01, i11 = F32(s11 / det), F32(F32(-s01) / det), F32(s00 / det)
    K = []
    for k in range(4):
        a, b = g(k, 0), g(k, 1)
        K.append((F32(F32(a * i00) + F32(b * i01)), F32(F32(a * i01) + F32(b * i11))))
    y0, y1 = F32(z[0] - x[0]), F32(z[1] - x[1])
    xn = [F32(x[k] + F32(F32(K[k][0] * y0) + F32(K[k][1] * y1))) for k in range(4)]
    out = np.zeros(10, F32)
    for n, (k, l) in enumerate(UT):
        out[n] = F32(g(k, l) - F32(F32(K[k][0] * g(0, l)) + F32(K[k][1] * g(1, l))))
    return xn, out


def kf_update(mean, cov, z):
    mean, cov = mean.copy(), cov.copy()
    sp = (F32(WP * mean[2]), F32(WP * mean[3]))
    r = (F32(sp[0] * sp[0]), F32(sp[1] * sp[1]))
    for b in range(2):
        idx = BLOCK_MEAN[b]
        x, P = _blk_update([mean[i] for i in idx], cov[10 * b:10 * b + 10], (z[2 * b], z[2 * b + 1]), r)
        for i, v in zip(idx, x):
            mean[i] = v
        cov[10 * b:10 * b + 10] = P
    return mean, cov


def warp_is_identity(warp) -> bool:
    w = np.asarray(warp, F32).reshape(6)
    return bool(w[0] == 1 and w[1] == 0 and w[2] == 0 and w[3] == 0 and w[4] == 1 and w[5] == 0)


def _rxr(R, x00, x01, x10, x11):
    """R X R' of a 2x2 X: T = R X, then T R', each entry a sum of two products."""
    r00, r01, r10, r11 = R
    t00, t01 = F32(F32(r00 * x00) + F32(r01 * x10)), F32(F32(r00 * x01) + F32(r01 * x11))
    t10, t11 = F32(F32(r10 * x00) + F32(r11 * x10)), F32(F32(r10 * x01) + F32(r11 * x11))
    return (F32(F32(t00 * r00) + F32(t01 * r01)), F32(F32(t00 * r10) + F32(t01 * r11)),
            F32(F32(t10 * r00) + F32(t11 * r01)), F32(F32(t10 * r10) + F32(t11 * r11)))


def kf_warp(mean, cov, warp):
    """The camera-motion warp [R | t] (row-major 2x3): every pair of the mean times R, t added to (cx, cy), each block M P M' with
    M = diag(R, R).  The identity warp is skipped (the state keeps its bits)."""
    if warp is None or warp_is_identity(warp):
        return mean, cov
    w = np.asarray(warp, F32).reshape(6)
    R, t = (w[0], w[1], w[3], w[4]), (w[2], w[5])
    mean, cov = mean.copy(), cov.copy()
    for a, b in ((0, 1), (2, 3), (4, 5), (6, 7)):
        p, q = mean[a], mean[b]
        mean[a] = F32(F32(R[0] * p) + F32(R[1] * q))
        mean[b] = F32(F32(R[2] * p) + F32(R[3] * q))
    mean[0], mean[1] = F32(mean[0] + t[0]), F32(mean[1] + t[1])
    for blk in range(2):
        P = cov[10 * blk:10 * blk + 10]
        g = lambda r, c: _p(P, r, c)                       # noqa: E731
        a = _rxr(R, g(0, 0), g(0, 1), g(0, 1), g(1, 1))
        b = _rxr(R, g(0, 2), g(0, 3), g(1, 2), g(1, 3))
        c = _rxr(R, g(2, 2), g(2, 3), g(2, 3), g(3, 3))
        cov[10 * blk:10 * blk + 10] = np.asarray([a[0], a[1], b[0], b[1], a[3], b[2], b[3], c[0], c[1], c[3]], F32)
    return mean, cov


def dense_cov(cov):
    """cov[20] -> the 8x8 matrix in the mean's order."""
    out = np.zeros((8, 8), np.float64)
    for b in range(2):
        idx = BLOCK_MEAN[b]
        for n, (r, c) in enumerate(UT):
            out[idx[r], idx[c]] = out[idx[c], idx[r]] = float(cov[10 * b + n])
    return out


# ---- the integer feature -----------------------------------------------------------------------------------------------------
def feat_step(s16, f):
    """One step of the smoothed feature: v = 9 s16 + 128 f (a birth: 128 f), r = isqrt(sum v^2); the int16 state at norm 16256 and
    the int8 row at norm 127, both rounded half up in magnitude; r == 0 gives zeros.  Returns (s16, s8) as lists of ints."""
    f = [int(v) for v in f]
    v = [128 * b for b in f] if s16 is None else [9 * int(a) + 128 * b for a, b in zip(s16, f)]
    r = math.isqrt(sum(x * x for x in v))
    if r == 0:
        return [0] * len(v), [0] * len(v)
    sign = lambda x: -1 if x < 0 else 1                    # noqa: E731
    n16 = [sign(x) * ((FEAT_NORM * abs(x) + r // 2) // r) for x in v]
    n8 = [sign(x) * min(127, (127 * abs(x) + r // 2) // r) for x in v]
    return n16, n8


# ---- the tracker ---------------------------------------------------------------------------------------------------------
class _Trk:
    __slots__ = ("id", "flag", "age", "tsu", "start", "last", "box", "conf", "cls", "mean", "cov", "f16", "f8", "pbox")


class BotSortRef:
    """One stream.  ``update(xyxy, conf, cls, desc=None, warp=None)`` advances a frame and returns the indices of the returned
    tracks (flag == 2); ``snapshot()`` is the parity surface (= rtmodt_botsort_state).  ``dim`` = 0 is motion only.  ``record`` (a
    list) receives, per matching problem solved, a dict with the stage, the frame, the gain matrix and the pairs."""

    def __init__(self, track_high_thresh=0.6, track_low_thresh=0.1, new_track_thresh=0.7, track_buffer=30, match_thresh=0.8,
                 proximity_thresh=0.5, appearance_thresh=0.25, fuse_score=True, dim=0, gmc=True, reid=True, record=None):
        self.high, self.low, self.new = F32(track_high_thresh), F32(track_low_thresh), F32(new_track_thresh)
        self.track_buffer, self.match_thresh = int(track_buffer), float(match_thresh)
        self.proximity, self.appearance, self.fuse_score = float(proximity_thresh), float(appearance_thresh), bool(fuse_score)
        self.dim, self.gmc, self.reid, self.record = int(dim), gmc, reid, record
        self.next_id, self.frame_count = 1, 0
        self.tracks = []

    def _solve(self, stage, gain, rows, cols):
        pairs, total = max_gain_matching(gain) if rows and cols else ([], 0.0)
        if self.record is not None and rows and cols:
            self.record.append({"stage": stage, "frame": self.frame_count, "gain": gain, "pairs": pairs, "total": total})
        return [(rows[r], cols[c]) for r, c in pairs]

    def _fused_gain(self, rows, cols, xyxy, conf, desc, thr):
        T = self.tracks
        gain = [[None] * len(cols) for _ in rows]
        if not rows or not cols:
            return gain
        iou = batch_iou(np.asarray([T[i].pbox for i in rows], F32), xyxy[cols])
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                d = 1.0 - float(iou[a, b])
                far = d > self.proximity
                if self.fuse_score:
                    d = 1.0 - float(iou[a, b]) * float(conf[j])
                cost = d
                if self.dim and self.reid:
                    dot = sum(int(x) * int(y) for x, y in zip(T[i].f8, desc[j]))
                    emb = max(0, DOT_ONE - dot) / 32258.0
                    if emb > self.appearance or far:
                        emb = 1.0
                    cost = min(d, emb)
                if cost <= thr:
                    gain[a][b] = (thr + 1e-5) - cost
        return gain

    def _iou_gain(self, rows, cols, xyxy, thr):
        gain = [[None] * len(cols) for _ in rows]
        if not rows or not cols:
            return gain
        iou = batch_iou(np.asarray([self.tracks[i].pbox for i in rows], F32), xyxy[cols])
        for a in range(len(rows)):
            for b in range(len(cols)):
                d = 1.0 - float(iou[a, b])
                if d <= thr:
                    gain[a][b] = (thr + 1e-5) - d
        return gain

    def update(self, xyxy, conf, cls, desc=None, warp=None):
        xyxy = np.asarray(xyxy, F32).reshape(-1, 4)
        conf, cls = np.asarray(conf, F32).reshape(-1), np.asarray(cls, np.int32).reshape(-1)
        if self.dim:
            desc = np.asarray(desc, np.int8).reshape(-1, self.dim) if len(conf) else np.zeros((0, self.dim), np.int8)
        with np.errstate(all="ignore"):
            return self._update(xyxy, conf, cls, desc, warp if self.gmc else None)

    def _update(self, xyxy, conf, cls, desc, warp):
        self.frame_count += 1
        fc = self.frame_count
        T = self.tracks
        # predict (tracked and lost; a lost track's vw, vh are zeroed first), then the warp on every track
        for t in T:
            t.age += 1
            t.tsu += 1
            if t.flag != NEW:
                if t.flag == LOST:
                    t.mean[6] = t.mean[7] = F32(0)
                t.mean, t.cov = kf_predict(t.mean, t.cov)
            t.mean, t.cov = kf_warp(t.mean, t.cov, warp)
            t.pbox = mean_to_box(t.mean)
        high = [j for j in range(len(conf)) if conf[j] > self.high]
        low = [j for j in range(len(conf)) if conf[j] > self.low and conf[j] < self.high]
        t_match, d_used = {}, set()

        def matched(i, j, feature):
            t = T[i]
            t.mean, t.cov = kf_update(t.mean, t.cov, box_to_xywh(xyxy[j]))
            if feature and self.dim:
                t.f16, t.f8 = feat_step(t.f16, desc[j])
            t.flag, t.tsu, t.last = TRACKED, 0, fc
            t.box, t.conf, t.cls = xyxy[j].copy(), conf[j], int(cls[j])
            t_match[i] = j
            d_used.add(j)

        # first association: tracked + lost x high
        rows, cols = [i for i, t in enumerate(T) if t.flag != NEW], list(high)
        pairs1 = self._solve("first", self._fused_gain(rows, cols, xyxy, conf, desc, self.match_thresh), rows, cols)
        # second association: still unmatched tracked x low, plain IoU
        m1 = {i for i, _ in pairs1}
        rows, cols = [i for i, t in enumerate(T) if t.flag == TRACKED and i not in m1], list(low)
        pairs2 = self._solve("second", self._iou_gain(rows, cols, xyxy, SECOND_THRESH), rows, cols)
        # new tracks x remaining high
        u1 = {j for _, j in pairs1}
        rows, cols = [i for i, t in enumerate(T) if t.flag == NEW], [j for j in high if j not in u1]
        pairs3 = self._solve("new", self._fused_gain(rows, cols, xyxy, conf, desc, NEW_MATCH_THRESH), rows, cols)
        for i, j in pairs1 + pairs3:
            matched(i, j, True)
        for i, j in pairs2:
            matched(i, j, False)
        kept = []
        for i, t in enumerate(T):
            if i not in t_match:
                if t.flag == NEW:
                    continue
                if t.flag == TRACKED:
                    t.flag = LOST
                if fc - t.last > self.track_buffer:
                    continue
            kept.append(t)
        for j in high:
            if j in d_used or not conf[j] >= self.new:
                continue
            t = _Trk()
            t.id = self.next_id
            self.next_id += 1
            t.flag = TRACKED if fc == 1 else NEW
            t.age = t.tsu = 0
            t.start = t.last = fc
            t.box, t.conf, t.cls = xyxy[j].copy(), conf[j], int(cls[j])
            t.mean, t.cov = kf_init(box_to_xywh(xyxy[j]))
            t.f16, t.f8 = feat_step(None, desc[j]) if self.dim else (None, None)
            t.pbox = None
            kept.append(t)
        # duplicates: every (not lost, lost) pair judged on the list before any removal
        boxes = [mean_to_box(t.mean) for t in kept]
        lost = [q for q, t in enumerate(kept) if t.flag == LOST]
        rest = [p for p, t in enumerate(kept) if t.flag != LOST]
        kill = set()
        if lost and rest:
            iou = batch_iou(np.asarray([boxes[p] for p in rest], F32), np.asarray([boxes[q] for q in lost], F32))
            for a, p in enumerate(rest):
                for b, q in enumerate(lost):
                    if 1.0 - float(iou[a, b]) < DUP_DIST:
                        kill.add(q if fc - kept[p].start > fc - kept[q].start else p)
        self.tracks = [t for k, t in enumerate(kept) if k not in kill]
        return [i for i, t in enumerate(self.tracks) if t.flag == TRACKED]

    def snapshot(self) -> dict:
        T = self.tracks
        n, D = len(T), self.dim
        out = {"ids": np.asarray([t.id for t in T], np.int64), "flag": np.asarray([t.flag for t in T], np.int32),
               "age": np.asarray([t.age for t in T], np.int32), "tsu": np.asarray([t.tsu for t in T], np.int32),
               "start_frame": np.asarray([t.start for t in T], np.int32), "last_frame": np.asarray([t.last for t in T], np.int32),
               "xyxy": np.asarray([t.box for t in T], F32).reshape(n, 4), "conf": np.asarray([t.conf for t in T], F32),
               "cls": np.asarray([t.cls for t in T], np.int32), "mean": np.asarray([t.mean for t in T], F32).reshape(n, 8),
               "cov": np.asarray([t.cov for t in T], F32).reshape(n, 20), "next_id": self.next_id, "frame_count": self.frame_count}
        out["feat16"] = np.asarray([t.f16 for t in T], np.int16).reshape(n, D) if D else np.zeros((n, 0), np.int16)
        out["feat8"] = np.asarray([t.f8 for t in T], np.int8).reshape(n, D) if D else np.zeros((n, 0), np.int8)
        return out

    def tracks_out(self, idx):
        """What BotSortTracker.update returns for these indices: (track id, box of the filter's mean)."""
        return [(self.tracks[i].id, mean_to_box(self.tracks[i].mean)) for i in idx]


def snapshots_equal(a: dict, b: dict):
    """None when two snapshots agree bit for bit, else the name of the first field that differs."""
    for k in ("next_id", "frame_count"):
        if a[k] != b[k]:
            return k
    for k in ("ids", "flag", "age", "tsu", "start_frame", "last_frame", "cls", "feat16", "feat8"):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            return k
    for k in ("xyxy", "conf", "mean", "cov"):
        x, y = np.ascontiguousarray(a[k], F32), np.ascontiguousarray(b[k], F32)
        if x.shape != y.shape or not np.array_equal(x.view(np.int32), y.view(np.int32)):
            return k
    return None


# ---- scenes: a frame is (xyxy, conf, cls, object ids, warp or None) ------------------------------------------------------------
_frame = OC._frame


def affine(deg=0.0, scale=1.0, tx=0.0, ty=0.0):
    """Row-major 2x3 [R | t] as float32."""
    c, s = math.cos(math.radians(deg)) * scale, math.sin(math.radians(deg)) * scale
    return np.asarray([c, -s, tx, s, c, ty], F32)


def gmc_scene(n=12, step=(12.0, 16.0), turn=6):
    """Two standing objects (24 x 48 boxes) seen by a camera that pans half a box width a frame and a third of its height, out and
    back: every detection moves by `step` at once (IoU 0.2 with the standing prediction: fused cost 0.82 > match_thresh).  The warp
    handed in is the true image motion of the frame."""
    out, off = [], np.zeros(2)
    world = np.asarray([[200.0, 200.0, 224.0, 248.0], [300.0, 230.0, 324.0, 278.0]])
    for f in range(n):
        d = np.zeros(2) if f == 0 else np.asarray(step) * (1 if f < turn else -1)
        off = off + d
        b, c, k = _frame(world - np.tile(off, 2))
        out.append((b, c, k, np.arange(2), affine(tx=-d[0], ty=-d[1])))
    return out


def reid_scene(n_in=9, n_out=7, v=6.0, w=40.0, h=80.0, gap=10.0):
    """Two objects walk towards one another along a row, overlap (`gap` px apart) and turn back: the constant-velocity predictions
    run on, so IoU alone exchanges them at the turn (0.6 + 0.6 against 0.54 + 0.54); their appearance keeps them apart."""
    out = []
    for f in range(n_in + n_out):
        k = n_in - 1 - f if f < n_in else f - n_in + 1      # frames away from the meeting
        xa, xb = 100.0 - v * k, 100.0 + gap + v * k
        b, c, cl = _frame([[xa, 50, xa + w, 50 + h], [xb, 50, xb + w, 50 + h]])
        out.append((b, c, cl, np.arange(2), None))
    return out


def fuse_scene(n=4, tail=4):
    """A standing object; then two detections beside it: the nearer one (IoU 0.6) with confidence 0.65, the other (IoU 0.54) with
    0.95.  IoU alone takes the nearer; fused with the score, 0.6 x 0.65 < 0.54 x 0.95."""
    out = []
    for f in range(n):
        b, c, k = _frame([[100, 50, 140, 130]])
        out.append((b, c, k, np.arange(1), None))
    for f in range(tail):
        b, c, k = _frame([[90, 50, 130, 130], [112, 50, 152, 130]], [0.65, 0.95])
        out.append((b, c, k, np.arange(2), None))
    return out


def _from_oc(frames, warps=None):
    return [(b, c, k, None, None if warps is None else warps[f % len(warps)]) for f, (b, c, k) in enumerate(frames)]


def _from_ds(scene, warps=None):
    frames, h, w = scene
    return [(b, c, k, ids, None if warps is None else warps[f % len(warps)]) for f, (b, c, k, ids, _) in enumerate(frames)], h, w


def object_descriptors(frames, dim, seed, noise=0.08):
    """int8 rows per detection: each object id has its own random direction, plus per-frame noise (so the EMA moves)."""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 1, (256, dim)).astype(np.float32)
    out = []
    for f in frames:
        ids = np.asarray(f[3], np.int64) if f[3] is not None else np.arange(len(f[0]))
        x = base[ids % 256] + rng.normal(0, noise, (len(ids), dim)).astype(np.float32)
        out.append(DS.quantize_rows(x) if len(ids) else np.zeros((0, dim), np.int8))
    return out


def object_colours(frames):
    return [DS.PALETTE[(np.asarray(f[3]) if f[3] is not None else np.arange(len(f[0]))) % len(DS.PALETTE)].reshape(-1, 3) for f in frames]


def render_frames(frames, h, w, seed=2000):
    """BGR frames for the built-in descriptor: every box filled with its object's colour (deepsort_ref.render_scene)."""
    return [DS.render_scene(f[0], col, h, w, seed=seed + k) for k, (f, col) in enumerate(zip(frames, object_colours(frames)))]


_STREAM_WARPS = [None, [affine()], [affine(2.0, 1.0, 3.0, -2.0)], [affine(-3.0, 1.02, -4.0, 1.5), affine(1.0, 0.99, 2.0, 2.0)],
                 [affine(0.0, 1.0, 5.25, -3.5)], [affine(4.0, 0.97, 0.0, 0.0)], None, [affine(-1.5, 1.01, -2.25, 4.0)]]


def _stream(k):
    """Stream k of the eight-stream call: ragged counts, its own warp; stream 1 gets the identity row, stream 5 has detections only
    in its first frames (tracks, no detections), stream 6 only in its last (detections, no tracks)."""
    frames, _, _ = _from_ds(DS.random_scene(50 + k, 12 + k, 1 + (k * 3) % 7, gaps=((0, 4 + k % 3, 2 + k % 3),), spurious=0.3, lowconf=0.25),
                            _STREAM_WARPS[k])
    empty = (np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32), np.zeros(0, np.int64))
    if k == 5:
        frames = [f if n < 5 else empty + (f[4],) for n, f in enumerate(frames)]
    if k == 6:
        frames = [f if n >= 6 else empty + (f[4],) for n, f in enumerate(frames)]
    return frames


# The sequences of the GPU suite (tests/test_gpu_botsort.py): name -> (tracker parameters, descriptor dimension (0 = motion only),
# scene factory).  tests/test_botsort_cpu.py shows on the restatement that every assignment optimum in every frame of each of them is
# unique with a margin above 1e-9.
_OCC = dict(gaps=((0, 8, 3), (1, 9, 5), (2, 10, 6), (3, 12, 9)))
SEQUENCES = {
    "gmc": (dict(), 0, gmc_scene),
    "reid64": (dict(), 64, reid_scene),
    "reid512": (dict(), 512, reid_scene),
    "fuse": (dict(), 0, fuse_scene),
    "fuse_off": (dict(fuse_score=False), 0, fuse_scene),
    "occlusion": (dict(track_buffer=5), 0, lambda: _from_oc(OC.motion_scene(11, 30, 5, speed=1.5, **_OCC))),
    "lifecycle": (dict(track_buffer=4), 0, lambda: _from_oc(OC.motion_scene(21, 30, 4, gaps=((0, 1, 4), (1, 2, 3)), spurious=0.6))),
    "thresholds": (dict(track_buffer=6), 0, lambda: _from_oc(OC.motion_scene(42, 30, 6, lowconf=0.4))),
    "warped": (dict(track_buffer=6), 0, lambda: _from_oc(OC.motion_scene(43, 24, 5, gaps=((1, 6, 3),), speed=3.0),
                                                         [affine(1.5, 1.01, 2.0, -1.0), affine(-2.0, 0.99, -1.5, 2.5), affine()])),
    "empty": (dict(track_buffer=3), 0, lambda: _from_oc([OC._frame([])] * 2 + OC.motion_scene(46, 16, 3, empty=(5, 6, 9, 10, 11, 12, 13)))),
    "rendered": (dict(track_buffer=5), 192, lambda: _from_ds(DS.random_scene(11, 14, 4, h=48, w=64, gaps=((0, 5, 3),), speed=1.0, size=(10, 20)))),
    "big": (dict(track_buffer=5), 0, lambda: _from_oc(OC.big_scene())),
    "limit": (dict(track_buffer=3), 0, lambda: _from_oc(OC.pair_limit_frames(False))),
}
for _k in range(8):
    SEQUENCES[f"stream{_k}"] = (dict(track_buffer=4), 64, lambda _k=_k: _stream(_k))


def sequence_inputs(name):
    """(parameters, dim, list of per-frame (xyxy, conf, cls, int8 descriptors or None, warp or None, BGR frame or None)).  The
    descriptors of a 192-dimensional sequence are the built-in ones of its rendered frames."""
    params, dim, factory = SEQUENCES[name]
    scene = factory()
    images = [None] * len(scene) if not isinstance(scene, tuple) else None
    if isinstance(scene, tuple):
        scene, h, w = scene
        images = render_frames(scene, h, w)
    if dim == 192:
        desc = [DS.describe(img, f[0])[0] for img, f in zip(images, scene)]
    elif dim:
        desc = object_descriptors(scene, dim, seed=len(name) + dim)
    else:
        desc = [None] * len(scene)
    return params, dim, [(f[0], f[1], f[2], d, f[4], img) for f, d, img in zip(scene, desc, images)]


def run(name, record=None, **switch):
    """The restatement over a named sequence; returns it after the last frame."""
    params, dim, frames = sequence_inputs(name)
    ref = BotSortRef(dim=dim, record=record, **params, **switch)
    for xy, cf, cl, desc, warp, _ in frames:
        ref.update(xy, cf, cl, desc, warp)
    return ref
