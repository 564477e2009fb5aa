"""Plain NumPy / Python restatement of the snapshot gallery (``csrc/snapshot_rule.h``, ``csrc/snapshot.hip``): the crop rectangle,
the never-enlarging fit, the exact area average, the score, the replacement rule, the id-sorted ledger with retirement, and the
slot assignment.  Written from the rules, not from the kernels: matrices of integer weights instead of tiled sums, dictionaries
and sorted lists instead of prefix sums.  The kernels must equal it exactly: every thumbnail byte, every ``updated`` / ``retired``
entry, the whole ledger and the slot bitmap after every call."""
from __future__ import annotations

import dataclasses

import numpy as np

COORD_MAX = 1 << 20
F_NEW, F_REWRITTEN, F_CUT, F_OCCLUDED = 1, 2, 4, 8
OK, E_INVALID, E_CAPACITY = 0, -1, -4


@dataclasses.dataclass
class Cfg:
    thumb_h: int = 96
    thumb_w: int = 96
    margin_pm: int = 100
    min_side: int = 8
    area_cap: int = 1 << 16
    occl_iou_pm: int = 300
    min_gain_pm: int = 100
    retire_after: int = 30
    pad_bgr: tuple = (114, 114, 114)
    max_updated: int = 1024
    max_retired: int = 1024
    classes: tuple | None = None


@dataclasses.dataclass
class Plan:
    raw: tuple
    box: tuple
    crop: tuple
    sw: int
    sh: int
    dw: int
    dh: int
    ox: int
    oy: int
    cut: int
    area: int


def coord(v) -> int:
    """privacy_regions.h: the float32 value clamped to +-2^20, truncated toward zero."""
    v = np.float32(v)
    lim = np.float32(COORD_MAX)
    return int(min(max(v, -lim), lim))


def plan(cfg: Cfg, xyxy, h: int, w: int, cls: int = 0, use_filter: bool = True):
    """The plan of one box, or ``None`` when the box is not sampled."""
    if use_filter and cfg.classes is not None and int(cls) not in [int(c) for c in cfg.classes]:
        return None
    b = np.asarray(xyxy, np.float32)
    if not np.isfinite(b).all():
        return None
    x0, y0, x1, y1 = (coord(v) for v in b)
    if x1 < x0 or y1 < y0:
        return None
    W, H = x1 - x0 + 1, y1 - y0 + 1
    mx, my = W * cfg.margin_pm // 1000, H * cfg.margin_pm // 1000
    box = (max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1))
    crop = (max(x0 - mx, 0), max(y0 - my, 0), min(x1 + mx, w - 1), min(y1 + my, h - 1))
    sw, sh = crop[2] - crop[0] + 1, crop[3] - crop[1] + 1
    if sw < max(cfg.min_side, 1) or sh < max(cfg.min_side, 1):
        return None
    tw, th = cfg.thumb_w, cfg.thumb_h
    if sw <= tw and sh <= th:
        dw, dh = sw, sh
    elif sw * th >= sh * tw:
        dw, dh = tw, max(1, (sh * tw + sw // 2) // sw)
    else:
        dw, dh = max(1, (sw * th + sh // 2) // sh), th
    cut = int(x0 <= 0 or y0 <= 0 or x1 >= w - 1 or y1 >= h - 1)
    bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
    area = min(bw * bh, cfg.area_cap) if bw > 0 and bh > 0 else 0
    return Plan((x0, y0, x1, y1), box, crop, sw, sh, dw, dh, (tw - dw) // 2, (th - dh) // 2, cut, area)


def axis_weights(S: int, D: int) -> np.ndarray:
    """[D][S] int64: row j holds the overlap of [j S, (j + 1) S) with every source pixel's [i D, (i + 1) D); each row sums to S."""
    assert 1 <= D <= S
    j = np.arange(D, dtype=np.int64)[:, None]
    i = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((j + 1) * S, (i + 1) * D) - np.maximum(j * S, i * D))


def resample(crop: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """The exact area average of ``crop`` (sh x sw x 3, uint8) at dh x dw: one rounding per value."""
    sh, sw = crop.shape[:2]
    wy, wx = axis_weights(sh, dh), axis_weights(sw, dw)
    tot = sh * sw
    out = np.empty((dh, dw, crop.shape[2]), np.uint8)
    for c in range(crop.shape[2]):
        acc = wy @ crop[..., c].astype(np.int64) @ wx.T
        out[..., c] = ((acc + tot // 2) // tot).astype(np.uint8)
    return out


def thumbnail(cfg: Cfg, frame: np.ndarray, p: Plan) -> np.ndarray:
    t = np.empty((cfg.thumb_h, cfg.thumb_w, 3), np.uint8)
    t[:] = np.asarray(cfg.pad_bgr[:3], np.uint8)
    x0, y0, x1, y1 = p.crop
    t[p.oy:p.oy + p.dh, p.ox:p.ox + p.dw] = resample(frame[y0:y1 + 1, x0:x1 + 1, :3], p.dh, p.dw)
    return t


def conf_milli(conf) -> int:
    if conf is None:
        return 1000
    with np.errstate(all="ignore"):
        m = np.float32(conf) * np.float32(1000.0)
    if not m > 0:
        return 0
    if m >= 1000:
        return 1000
    return int(m)


def occludes(a, b, pm: int) -> bool:
    if pm <= 0 or a[2] < a[0] or a[3] < a[1] or b[2] < b[0] or b[3] < b[1]:
        return False
    iw = min(a[2], b[2]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[1], b[1]) + 1
    if iw <= 0 or ih <= 0:
        return False
    inter = iw * ih
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return inter * 1000 > pm * union


def score(cm: int, area: int, cut: bool, occluded: bool) -> int:
    s = cm * area
    if cut:
        s >>= 1
    if occluded:
        s >>= 1
    return s


def replaces(new: int, best: int, min_gain_pm: int) -> bool:
    return new * 1000 > best * (1000 + min_gain_pm)


@dataclasses.dataclass
class Row:
    track_id: int
    slot: int
    best_score: int
    best_frame: int
    xyxy: np.ndarray
    conf: np.float32
    cls: int
    first_seen: int
    last_seen: int
    n_rewrites: int
    flags: int


class Stream:
    """One stream's ledger and atlas."""

    def __init__(self, cfg: Cfg, max_tracks: int):
        self.cfg, self.max_tracks, self.cap = cfg, max_tracks, 2 * max_tracks
        self.rows: dict[int, Row] = {}
        self.atlas = np.zeros((self.cap, cfg.thumb_h, cfg.thumb_w, 3), np.uint8)
        self.last_frame = None
        self.err = 0

    def bitmap(self) -> np.ndarray:
        bm = np.zeros((self.cap + 31) // 32, np.uint32)
        for r in self.rows.values():
            bm[r.slot // 32] |= np.uint32(1 << (r.slot % 32))
        return bm

    def ledger(self):
        return [self.rows[k] for k in sorted(self.rows)]

    def process(self, ids, xyxy, conf, cls, frame, frame_id, selected=None):
        """One call.  Returns (code, updated, retired, n_rewritten): ``updated`` = (track_id, score, slot, flags, list index) in list
        order, ``retired`` = the retired rows in id order -- both whole; the C ABI delivers the first max_updated / max_retired."""
        cfg = self.cfg
        if self.last_frame is not None and frame_id <= self.last_frame:
            return E_INVALID, [], [], 0
        self.last_frame = frame_id
        h, w = frame.shape[:2]
        n = len(ids)
        plans = [plan(cfg, xyxy[i], h, w, cls[i]) if (selected is None or selected[i]) else None for i in range(n)]
        sampled = [i for i in range(n) if plans[i] is not None]
        start_slots = {r.slot for r in self.rows.values()}
        n_old = len(self.rows)
        retired = [r for r in self.ledger() if frame_id - r.last_seen > cfg.retire_after]
        for r in retired:
            del self.rows[r.track_id]
        decisions = []
        for i in sampled:
            p = plans[i]
            occl = any(occludes(p.box, plans[u].box, cfg.occl_iou_pm) for u in sampled if u != i)
            s = score(conf_milli(None if conf is None else conf[i]), p.area, bool(p.cut), occl)
            fl = (F_CUT if p.cut else 0) | (F_OCCLUDED if occl else 0)
            row = self.rows.get(int(ids[i]))
            if row is None:
                fl |= F_NEW
            elif replaces(s, row.best_score, cfg.min_gain_pm):
                fl |= F_REWRITTEN
            decisions.append((i, s, fl))
        sampled_ids = {int(ids[i]) for i in sampled}
        idle = [k for k in self.rows if k not in sampled_ids]
        n_new = sum(1 for _, _, fl in decisions if fl & F_NEW)
        overflow = len(sampled) + len(idle) > self.cap or n_new > self.cap - n_old
        if overflow:
            for k in idle:
                del self.rows[k]
            self.err = 1
            start_slots = {r.slot for r in self.rows.values()}
        free = [s for s in range(self.cap) if s not in start_slots]
        for r in self.rows.values():
            r.flags &= F_CUT | F_OCCLUDED
        updated, k_new, n_rew = [], 0, 0
        for i, s, fl in decisions:
            tid = int(ids[i])
            c = np.float32(1.0) if conf is None else np.float32(conf[i])
            if fl & F_NEW:
                row = Row(tid, free[k_new], s, frame_id, np.array(xyxy[i], np.float32), c, int(cls[i]), frame_id, frame_id, 0, fl)
                k_new += 1
                self.rows[tid] = row
            else:
                row = self.rows[tid]
                row.last_seen = frame_id
                if fl & F_REWRITTEN:
                    row.best_score, row.best_frame, row.xyxy, row.conf, row.cls = s, frame_id, np.array(xyxy[i], np.float32), c, int(cls[i])
                    row.n_rewrites += 1
                    row.flags = fl
                    n_rew += 1
            if fl & (F_NEW | F_REWRITTEN):
                self.atlas[row.slot] = thumbnail(cfg, frame, plans[i])
                updated.append((tid, s, row.slot, fl, i))
        code = OK
        if self.err:
            code = E_CAPACITY
        elif len(updated) > cfg.max_updated or len(retired) > cfg.max_retired:
            code = E_CAPACITY
        return code, updated, retired, n_rew


def crop(cfg: Cfg, frames, boxes, frame_idx):
    """Stateless crops: (thumbnails [n][th][tw][3] with untouched entries left zero, sampled [n])."""
    out = np.zeros((len(boxes), cfg.thumb_h, cfg.thumb_w, 3), np.uint8)
    ok = np.zeros(len(boxes), np.int32)
    for i, b in enumerate(boxes):
        f = frames[int(frame_idx[i])]
        p = plan(cfg, b, f.shape[0], f.shape[1], use_filter=False)
        if p is not None:
            out[i] = thumbnail(cfg, f, p)
            ok[i] = 1
    return out, ok
