"""The left / removed object detector's rules restated in NumPy and plain Python: the definition ``csrc/leftobj.hip`` and
``csrc/leftobj_rule.h`` are pinned to with ``==`` (every rule is integer arithmetic).  PARITY UNPINNED: the reference has no
counterpart and no default has been validated on real footage.

Grid, cell luma and pixel boxes are the motion detector's (``tests/motion_ref.py``).

Rules.
  1. Cell: ``bg``, ``cand`` (8.8 fixed point), ``age`` (16 bits), ``miss`` (8 bits), ``flags`` (bit 0: ignore).  ``t = Yc << 8``.
     ``frames_seen == 0``: ``bg = cand = t``, ``age = miss = 0``.  ``frames_seen < warmup``: ``bg += (t - bg) >> warm_shift``.
     Else ``fg = |t - bg| > threshold << 8``.  Not fg: ``bg += (t - bg) >> learn_shift``; with ``age > 0``, ``miss += 1`` and a miss
     above ``occlusion`` sets ``age = miss = 0``.  fg and ``|t - cand| <= stable << 8``: ``cand += (t - cand) >> cand_shift``,
     ``age = min(age + 1, 65535)``, ``miss = 0``.  fg, not stable: ``age > 0 and miss < occlusion``: ``miss += 1``; else
     ``cand = t, age = 1, miss = 0``.  ``static = age >= static_frames and not ignore``.
  2. Mask: ``static and n3 >= min_neighbors`` (3 x 3 count, the cell included).
  3. Regions: 8-connected components with ``min_area <= area <= max_area`` in raster order of their first cell; the first
     ``max_regions`` are stored.  ``cur`` / ``bgc``: over mask cells ``c`` and 4-neighbours ``n`` in the grid and outside the mask,
     ``|cand[c] >> 8 - Y[n]|`` / ``|bg[c] >> 8 - bg[n] >> 8|``; ABANDONED if ``cur > bgc``, REMOVED if ``bgc > cur``, else UNKNOWN.
  4. Status: WARMUP, else SCENE_CHANGE if ``1000 * n_fg >= scene_pm * cells`` (``frames_seen = 0``, every entry retires RESET, nothing
     is matched or born), else STATIC with a region, else CLEAR.
  5. Tracks: box = floor / ceil of the float32 coordinates clamped to +-2^20; not finite or empty: skipped.  covered:
     ``1000 * overlap >= covered_pm * region box area``; attended: an owner class and the box grown by ``attend_margin`` overlaps.
  6. Match: regions in raster order take the free entry sharing most cells of the (inclusive) cell boxes, lowest oid on a tie.
     Matched or born: attended -> ``idle = 0``, owner = largest attending id; else ``idle += 1`` unless covered by no report class.
     Until the alarm ``kind`` = TRACKED_STATIC if a report-class track covers, else the region's.  ``idle >= alarm_frames``: one
     event, latched.  Then ``frame_id - first_frame >= absorb_frames`` (> 0): ABSORBED, the region's cells take ``bg = cand``,
     ``age = miss = 0``.  Unmatched: ``unmatched += 1``; above ``miss_frames``: CLEARED.  Births follow the kept rows in raster
     order with the next oids; beyond ``max_objects`` they are dropped and counted.
"""
import numpy as np

import motion_ref as MR

WARMUP, CLEAR, STATIC, SCENE_CHANGE = 0, 1, 2, 3
UNKNOWN, ABANDONED, REMOVED, TRACKED_STATIC = 0, 1, 2, 3
CLEARED, ABSORBED, RESET = 1, 2, 3
MAX_SEEN = 2 ** 30
BOX_LIMIT = 2 ** 20
DEFAULTS = dict(scale=4, warmup=8, warm_shift=2, learn_shift=6, threshold=16, stable=10, cand_shift=3, occlusion=50, static_frames=100,
                min_neighbors=4, min_area=4, max_area=2 ** 24, max_regions=32, scene_pm=600, max_objects=64, miss_frames=50, alarm_frames=250,
                absorb_frames=0, covered_pm=500, attend_margin=32, max_tracks=256)
RULE_FIELDS = ("warmup", "warm_shift", "learn_shift", "threshold", "stable", "cand_shift", "occlusion", "static_frames")


def config(**kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise TypeError(k)
        c[k] = int(v)
    return c


# ---- 1. the cell ---------------------------------------------------------------------------------------------------------
def cell_loop(yc, cell, seen, c):
    """One cell ``(bg, cand, age, miss, flags)`` in plain Python integers -> (cell, fg, static)."""
    bg, cand, age, miss, flags = (int(v) for v in cell)
    t = int(yc) * 256
    fg = False
    if seen == 0:
        bg = cand = t
        age = miss = 0
    elif seen < c["warmup"]:
        bg += (t - bg) >> c["warm_shift"]
    elif abs(t - bg) <= c["threshold"] * 256:
        bg += (t - bg) >> c["learn_shift"]
        if age > 0:
            miss += 1
            if miss > c["occlusion"]:
                age = miss = 0
    else:
        fg = True
        if abs(t - cand) <= c["stable"] * 256:
            cand += (t - cand) >> c["cand_shift"]
            age = min(age + 1, 65535)
            miss = 0
        elif age > 0 and miss < c["occlusion"]:
            miss += 1
        else:
            cand, age, miss = t, 1, 0
    return (bg, cand, age, miss, flags), fg, age >= c["static_frames"] and not flags & 1


def update(yc, bg, cand, age, miss, seen, c):
    """The vectorised form -> (fg, bg, cand, age, miss) as new int64 arrays."""
    yc, bg, cand, age, miss = (np.asarray(v, np.int64) for v in (yc, bg, cand, age, miss))
    t = yc << 8
    none = np.zeros(yc.shape, bool)
    if seen == 0:
        return none, t.copy(), t.copy(), np.zeros_like(t), np.zeros_like(t)
    d = t - bg
    if seen < c["warmup"]:
        return none, bg + (d >> c["warm_shift"]), cand.copy(), age.copy(), miss.copy()
    fg = np.abs(d) > c["threshold"] << 8
    e = t - cand
    stable = fg & (np.abs(e) <= c["stable"] << 8)
    walk = fg & ~stable & (age > 0) & (miss < c["occlusion"])
    fresh = fg & ~stable & ~walk
    nbg = np.where(fg, bg, bg + (d >> c["learn_shift"]))
    ncand = np.where(stable, cand + (e >> c["cand_shift"]), np.where(fresh, t, cand))
    nmiss = np.where(~fg & (age > 0), miss + 1, miss)
    lost = ~fg & (age > 0) & (nmiss > c["occlusion"])
    nage = np.where(lost, 0, age)
    nmiss = np.where(lost, 0, nmiss)
    nage = np.where(stable, np.minimum(age + 1, 65535), np.where(fresh, 1, nage))
    nmiss = np.where(stable | fresh, 0, np.where(walk, miss + 1, nmiss))
    return fg, nbg, ncand, nage, nmiss


# ---- 2. / 3. mask, regions, kind -------------------------------------------------------------------------------------------
def mask_of(static, min_neighbors):
    s = np.asarray(static).astype(np.int64)
    return ((s > 0) & (MR._window_sum(s, 1) >= min_neighbors)).astype(np.uint8)


def labels_of(mask):
    """-> (labels int64 (gh, gw), -1 outside the mask, else the component's first cell index; MR.components' list)."""
    mask = np.asarray(mask) != 0
    gh, gw = mask.shape
    comps = MR.components(mask)
    if len(comps) == 1:
        return np.where(mask, comps[0][0], -1).astype(np.int64), comps
    lab = np.full((gh, gw), -1, np.int64)
    # a flood from each first cell: plain, and independent of MR.components' own union-find
    for first, area, *_ in comps:
        stack = [(first // gw, first % gw)]
        lab[stack[0]] = first
        n = 0
        while stack:
            y, x = stack.pop()
            n += 1
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if 0 <= ny < gh and 0 <= nx < gw and mask[ny, nx] and lab[ny, nx] < 0:
                        lab[ny, nx] = first
                        stack.append((ny, nx))
        assert n == area
    return lab, comps


def edge_sums(lab, root, cand, bg, luma):
    """cur and bgc of the component labelled ``root`` (vectorised; ``edge_sums_loop`` is the plain form)."""
    gh, gw = lab.shape
    sel = lab == root
    c8, b8, y = np.asarray(cand, np.int64) >> 8, np.asarray(bg, np.int64) >> 8, np.asarray(luma, np.int64)
    out = np.zeros((gh + 2, gw + 2), bool)
    out[1:-1, 1:-1] = lab < 0                                # cells outside the grid are no neighbours
    yp, bp = np.zeros((gh + 2, gw + 2), np.int64), np.zeros((gh + 2, gw + 2), np.int64)
    yp[1:-1, 1:-1], bp[1:-1, 1:-1] = y, b8
    cur = bgc = 0
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        win = (slice(1 + dy, 1 + dy + gh), slice(1 + dx, 1 + dx + gw))
        use = sel & out[win]
        cur += int(np.abs(c8 - yp[win])[use].sum())
        bgc += int(np.abs(b8 - bp[win])[use].sum())
    return cur, bgc


def edge_sums_loop(lab, root, cand, bg, luma):
    gh, gw = lab.shape
    cur = bgc = 0
    for y, x in zip(*np.nonzero(lab == root)):
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            ny, nx = y + dy, x + dx
            if 0 <= ny < gh and 0 <= nx < gw and lab[ny, nx] < 0:
                cur += abs((int(cand[y, x]) >> 8) - int(luma[ny, nx]))
                bgc += abs((int(bg[y, x]) >> 8) - (int(bg[ny, nx]) >> 8))
    return cur, bgc


def kind_of(cur, bgc):
    return ABANDONED if cur > bgc else (REMOVED if bgc > cur else UNKNOWN)


def status_of(seen, n_fg, cells, n_regions_total, c):
    if seen < c["warmup"]:
        return WARMUP
    if 1000 * n_fg >= c["scene_pm"] * cells:
        return SCENE_CHANGE
    return STATIC if n_regions_total >= 1 else CLEAR


def next_seen(seen, status):
    return 0 if status == SCENE_CHANGE else min(seen + 1, MAX_SEEN)


# ---- 5. tracks ---------------------------------------------------------------------------------------------------------------
def track_box(xyxy):
    """float32 (x0, y0, x1, y1) -> the integer box, or None when it takes no part."""
    v = np.asarray(xyxy, np.float32)
    if not np.isfinite(v).all():
        return None
    v = np.clip(v.astype(np.float64), -BOX_LIMIT, BOX_LIMIT)
    b = (int(np.floor(v[0])), int(np.floor(v[1])), int(np.ceil(v[2])), int(np.ceil(v[3])))
    return b if b[0] < b[2] and b[1] < b[3] else None


def overlap(a, b):
    x0, y0, x1, y1 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    return (x1 - x0) * (y1 - y0) if x0 < x1 and y0 < y1 else 0


def covered(track, region, covered_pm):
    return 1000 * overlap(track, region) >= covered_pm * (region[2] - region[0]) * (region[3] - region[1])


def attended(track, region, margin):
    return overlap((track[0] - margin, track[1] - margin, track[2] + margin, track[3] + margin), region) > 0


def shared_cells(a, b):
    x0, y0, x1, y1 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    return (x1 - x0 + 1) * (y1 - y0 + 1) if x0 <= x1 and y0 <= y1 else 0


def track_tests(regions, tracks, c, owner_classes, report_classes):
    """Fills covered (bit 0: any, bit 1: a report class), attended and the owner (largest attending id, else None) of each region."""
    for g in regions:
        g["covered"], g["attended"], g["_owner"] = 0, 0, None
    if tracks is None:
        return
    ids, xyxy, cls = tracks
    for i in range(len(ids)):
        tb = track_box(xyxy[i])
        if tb is None:
            continue
        for g in regions:
            if covered(tb, g["box"], c["covered_pm"]):
                g["covered"] |= 3 if int(cls[i]) in report_classes else 1
            if int(cls[i]) in owner_classes and attended(tb, g["box"], c["attend_margin"]):
                g["attended"] = 1
                g["_owner"] = int(ids[i]) if g["_owner"] is None else max(g["_owner"], int(ids[i]))


# ---- 6. the ledger ---------------------------------------------------------------------------------------------------------
def timer(e, g, c):
    """One matched (or born) entry ``e`` against its region ``g``; -> whether the alarm fires."""
    if g["attended"]:
        e["idle"], e["owner"] = 0, g["_owner"]
    elif not g["covered"] & 1 or g["covered"] & 2:
        e["idle"] = min(e["idle"] + 1, MAX_SEEN)
    if not e["alarmed"]:
        e["kind"] = TRACKED_STATIC if g["covered"] & 2 else g["kind"]
    if not e["alarmed"] and e["idle"] >= c["alarm_frames"]:
        e["alarmed"] = 1
        return True
    return False


def event_of(e, frame_id):
    return dict(oid=e["oid"], kind=e["kind"], box=e["box"], area=e["area"], first_frame=e["first_frame"], frame_id=frame_id, owner=e["owner"])


def ledger_step(ledger, next_oid, regions, frame_id, c):
    """-> (new ledger, next_oid, events, retired, dropped, absorbed roots).  ``regions`` carry covered / attended / _owner."""
    free = [True] * len(ledger)
    match = {}
    for r, g in enumerate(regions):
        best, bj = 0, -1
        for j, e in enumerate(ledger):
            s = shared_cells(e["cells"], g["cells"]) if free[j] else 0
            if s > best:
                best, bj = s, j
        g["_match"] = bj
        if bj >= 0:
            free[bj] = False
            match[bj] = r
    kept, events, retired, absorbed = [], [], [], []
    for j, e in enumerate(ledger):
        e = dict(e)
        if j in match:
            g = regions[match[j]]
            fired = timer(e, g, c)
            e.update(unmatched=0, area=g["area"], cells=g["cells"], box=g["box"])
            g["oid"] = e["oid"]
            if fired:
                events.append(event_of(e, frame_id))
            if c["absorb_frames"] > 0 and frame_id - e["first_frame"] >= c["absorb_frames"]:
                retired.append((e["oid"], ABSORBED, e["alarmed"]))
                absorbed.append(g["root"])
                continue
        else:
            e["unmatched"] += 1
            if e["unmatched"] > c["miss_frames"]:
                retired.append((e["oid"], CLEARED, e["alarmed"]))
                continue
        kept.append(e)
    room = c["max_objects"] - len(kept)
    dropped = 0
    births = []
    for g in regions:
        if g["_match"] >= 0:
            continue
        if len(births) >= room:
            dropped += 1
            continue
        e = dict(oid=next_oid + len(births), kind=UNKNOWN, area=g["area"], idle=0, unmatched=0, alarmed=0, first_frame=frame_id, owner=-1,
                 cells=g["cells"], box=g["box"])
        if timer(e, g, c):
            events.append(event_of(e, frame_id))
        g["oid"] = e["oid"]
        births.append(e)
    return kept + births, next_oid + len(births), events, retired, dropped, absorbed


class Ref:
    """``streams`` models and ledgers; ``process`` answers what ``LeftObjectDetector.process`` answers, as dicts."""

    def __init__(self, streams, h, w, owner_classes=(0,), report_tracked=(), **cfg):
        self.c = config(**cfg)
        self.S, self.h, self.w = streams, h, w
        self.gh, self.gw = MR.grid_shape(h, w, self.c["scale"])
        self.owner, self.report = set(int(k) for k in owner_classes), set(int(k) for k in report_tracked)
        z = lambda: [np.zeros((self.gh, self.gw), np.int64) for _ in range(streams)]     # noqa: E731
        self.bg, self.cand, self.age, self.miss, self.flags, self.luma = z(), z(), z(), z(), z(), z()
        self.masks = [np.zeros((self.gh, self.gw), np.uint8) for _ in range(streams)]
        self.seen = [0] * streams
        self.ledgers = [[] for _ in range(streams)]
        self.next_oid = [1] * streams
        self.next_frame = [0] * streams

    def step(self, s, frame, frame_id=None, tracks=None):
        c = self.c
        frame_id = self.next_frame[s] if frame_id is None else int(frame_id)
        self.next_frame[s] = frame_id + 1
        yc = MR.cell_luma(frame, c["scale"])
        seen = self.seen[s]
        fg, self.bg[s], self.cand[s], self.age[s], self.miss[s] = update(yc, self.bg[s], self.cand[s], self.age[s], self.miss[s], seen, c)
        self.luma[s] = yc
        static = (self.age[s] >= c["static_frames"]) & (self.flags[s] & 1 == 0)
        mask = mask_of(static, c["min_neighbors"])
        self.masks[s] = mask
        lab, comps = labels_of(mask)
        comps = [k for k in comps if c["min_area"] <= k[1] <= c["max_area"]]
        regions = []
        for first, area, cx0, cy0, cx1, cy1 in comps[:c["max_regions"]]:
            sel = lab == first
            cur, bgc = edge_sums(lab, first, self.cand[s], self.bg[s], yc)
            regions.append(dict(box=MR.px_box(cx0, cy0, cx1, cy1, c["scale"], self.h, self.w), cells=(cx0, cy0, cx1, cy1), area=area, kind=kind_of(cur, bgc),
                                age_min=int(self.age[s][sel].min()), age_max=int(self.age[s][sel].max()), covered=0, attended=0, oid=0, root=first))
        n_fg = int(fg.sum())
        status = status_of(seen, n_fg, self.gh * self.gw, len(comps), c)
        self.seen[s] = next_seen(seen, status)
        events, dropped = [], 0
        if status == SCENE_CHANGE:
            retired = [(e["oid"], RESET, e["alarmed"]) for e in self.ledgers[s]]
            self.ledgers[s] = []
        else:
            track_tests(regions, tracks, c, self.owner, self.report)
            self.ledgers[s], self.next_oid[s], events, retired, dropped, absorbed = ledger_step(self.ledgers[s], self.next_oid[s], regions, frame_id, c)
            for root in absorbed:
                sel = lab == root
                self.bg[s] = np.where(sel, self.cand[s], self.bg[s])
                self.age[s] = np.where(sel, 0, self.age[s])
                self.miss[s] = np.where(sel, 0, self.miss[s])
        for g in regions:
            g.pop("_owner", None); g.pop("_match", None)
        return dict(stream=s, status=status, frames_seen=self.seen[s], n_fg=n_fg, n_static=int(mask.sum()), n_regions_total=len(comps),
                    n_objects=len(self.ledgers[s]), dropped=dropped, next_oid=self.next_oid[s], regions=regions, events=events, retired=retired,
                    objects=[dict(e) for e in self.ledgers[s]])

    def process(self, frames, streams=None, frame_id=None, tracks=None):
        names = range(self.S) if streams is None else streams
        out = []
        for i, s in enumerate(names):
            fid = None if frame_id is None else (frame_id if np.isscalar(frame_id) else frame_id[i])
            out.append(self.step(s, frames[i], fid, None if tracks is None else tracks[i]))
        return out

    def state(self, s):
        """-> (bg, cand, age, miss, flags, luma, frames_seen)"""
        return self.bg[s], self.cand[s], self.age[s], self.miss[s], self.flags[s], self.luma[s], self.seen[s]

    def set_ignore(self, grid, s=0):
        self.flags[s] = (np.asarray(grid) != 0).astype(np.int64)

    def reset(self, s):
        for a in (self.bg, self.cand, self.age, self.miss, self.luma):
            a[s] = np.zeros((self.gh, self.gw), np.int64)
        self.masks[s] = np.zeros((self.gh, self.gw), np.uint8)
        self.seen[s], self.ledgers[s], self.next_oid[s], self.next_frame[s] = 0, [], 1, 0
