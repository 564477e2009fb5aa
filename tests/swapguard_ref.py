"""Plain-Python restatement of the ID-swap guard of ``csrc/swapguard.hip`` -- TEST INFRASTRUCTURE, written rule by rule as
DESIGN.md section 19 reads.  Slow by design.

The guard is the online cure the reference's design document asks for three times and never builds (B.4 "Re-Identification
Considerations": keep the average colour histogram of a track's last 5 frames, and when two tracks swap within 3 frames compare
histograms and revert if similarity > 0.85; B.4's failure table: "add appearance verification"; G.1 row 1: "add lightweight
appearance hash verification").  PARITY UNPINNED: there is no reference implementation.  Everything is integer arithmetic except
the IoU, which is ``oracle.tracker_oracle.batch_iou`` (float32, operation by operation what ``track_dev.h``'s ``iou_ref`` does).

Also the scene builders of the two test files (S1 .. S7) and the runner that plays a scene through any guard.
"""
from __future__ import annotations

import math

import numpy as np

from deepsort_ref import DIM, PALETTE, describe, render_scene
from oracle.tracker_oracle import F32, TrackerOracle, batch_iou

DEFAULTS = dict(history=5, min_history=3, window=3, min_similarity_pm=850, min_gain_pm=1, contact_iou=0.0, max_gap_frames=30)


def similarity(q, ref) -> int:
    """Per-mille cosine of two non-negative integer vectors: (1000 * dot) // max(1, isqrt(n2(q) * n2(ref)))."""
    q = [int(v) for v in q]
    ref = [int(v) for v in ref]
    dot = sum(a * b for a, b in zip(q, ref))
    n2q, n2r = sum(a * a for a in q), sum(b * b for b in ref)
    return (1000 * dot) // max(1, math.isqrt(n2q * n2r))


def partners(boxes, contact_iou):
    """Per track (partner index or -1, in contact): the other track with the largest IoU, ties to the lowest index; a NaN IoU is
    never the largest.  In contact iff that maximum is > contact_iou (float32)."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    n = len(boxes)
    with np.errstate(all="ignore"):
        iou = batch_iou(boxes, boxes) if n else np.zeros((0, 0), F32)
    thr = F32(contact_iou)
    out = []
    for i in range(n):
        best, bj = F32(-np.inf), -1
        for j in range(n):
            if j != i and iou[i, j] > best:
                best, bj = iou[i, j], j
        out.append((bj, bool(bj >= 0 and best > thr)))
    return out


class SwapGuardRef:
    """One stream.  ``process(ids, boxes, descs, frame_id)`` -> (ids after the reverts, events); ``snapshot()`` is the parity
    surface (= rtmodt_swapguard_state).  ``refused`` counts the candidate pairs (mutual contact ids, both rows present, neither
    track in contact) that were not reverted."""

    def __init__(self, max_tracks=1024, **kw):
        p = dict(DEFAULTS, **kw)
        self.history, self.min_history, self.window = int(p["history"]), int(p["min_history"]), int(p["window"])
        self.min_similarity_pm, self.min_gain_pm = int(p["min_similarity_pm"]), int(p["min_gain_pm"])
        self.contact_iou, self.max_gap_frames = float(p["contact_iou"]), int(p["max_gap_frames"])
        assert 1 <= self.history <= 8 and 1 <= self.min_history <= self.history
        self.max_tracks, self.cap = int(max_tracks), 2 * int(max_tracks)
        self.rows = {}                                     # id -> dict(last, ring [int8[192] oldest first], contact_frame, contact_id)
        self.n_reverted = 0
        self.refused = 0
        self.ledger_overflow = False

    def process(self, ids, boxes, descs, frame_id):
        ids = [int(i) for i in ids]
        n = len(ids)
        if len(set(ids)) != n:
            raise ValueError("duplicate track id")
        if n > self.max_tracks:
            raise OverflowError("more tracks than max_tracks")
        boxes = np.asarray(boxes, F32).reshape(n, 4)
        descs = np.asarray(descs, np.int8).reshape(n, DIM)
        frame_id = int(frame_id)
        # 0. expiry
        for k in [k for k, r in self.rows.items() if frame_id - r["last"] > self.max_gap_frames]:
            del self.rows[k]
        # 1. / 2. blind tracks, partners, contact
        blind = [not descs[i].any() for i in range(n)]
        pc = partners(boxes, self.contact_iou)
        # 3. decisions, on the rows as they stand
        where = {tid: i for i, tid in enumerate(ids)}
        reverts = []
        for i in range(n):
            A = ids[i]
            ra = self.rows.get(A)
            if ra is None or ra["contact_id"] < 0:
                continue
            B = ra["contact_id"]
            j = where.get(B, -1)
            rb = self.rows.get(B)
            if j <= i or rb is None or rb["contact_id"] != A or pc[i][1] or pc[j][1]:
                continue
            ok = not blind[i] and not blind[j]
            ok = ok and frame_id - ra["contact_frame"] <= self.window and frame_id - rb["contact_frame"] <= self.window
            ok = ok and len(ra["ring"]) >= self.min_history and len(rb["ring"]) >= self.min_history
            sims = None
            if ok:
                refa = np.sum(np.asarray(ra["ring"], np.int32), axis=0)
                refb = np.sum(np.asarray(rb["ring"], np.int32), axis=0)
                sims = [similarity(descs[i], refa), similarity(descs[i], refb), similarity(descs[j], refb), similarity(descs[j], refa)]
                sAA, sAB, sBB, sBA = sims
                ok = sAB >= self.min_similarity_pm and sBA >= self.min_similarity_pm and sAB >= sAA + self.min_gain_pm and sBA >= sBB + self.min_gain_pm
            if ok:
                reverts.append((i, j, A, B, sims))
            else:
                self.refused += 1
        # 4. effects
        out = list(ids)
        events = []
        for i, j, A, B, sims in reverts:
            out[i], out[j] = B, A
            self.rows[A]["contact_id"] = self.rows[B]["contact_id"] = -1
            events.append(dict(frame_id=frame_id, track_a=i, track_b=j, id_a=A, id_b=B, sims=sims))
            self.n_reverted += 1
        # 5. update with the final ids; a ledger that would pass 2 x max_tracks rows drops its idle rows and stays in error
        idle = [k for k in self.rows if k not in where]
        if n + len(idle) > self.cap:
            self.ledger_overflow = True
            for k in idle:
                del self.rows[k]
        for i in range(n):
            r = self.rows.setdefault(out[i], dict(last=frame_id, ring=[], contact_frame=0, contact_id=-1))
            r["last"] = frame_id
            if pc[i][1]:
                r["contact_frame"], r["contact_id"] = frame_id, out[pc[i][0]]
            elif not blind[i]:
                r["ring"] = (r["ring"] + [descs[i].copy()])[-self.history:]
        return out, events

    def process_frame(self, ids, boxes, frame, frame_id):
        """The same with the descriptors taken from the frame (csrc/appearance.hip's rules, tests/deepsort_ref.py: describe)."""
        return self.process(ids, boxes, describe(frame, boxes)[0], frame_id)

    def snapshot(self):
        """Rows in ascending id: [id, last frame, count, contact frame, contact id, the ring's bytes oldest first]."""
        return [[k, r["last"], len(r["ring"]), r["contact_frame"], r["contact_id"],
                 np.asarray(r["ring"], np.int8).reshape(-1, DIM).tobytes()] for k, r in sorted(self.rows.items())]


# ---- scenes ------------------------------------------------------------------------------------------------------------------
# A scene is (h, w, frames); a frame is dict(frame_id, tracks=[(object key, box)], colours={key: bgr}, swaps=[(key, key)]).
# An object key names one physical object (one colour); ids0 maps it to the id it starts under.  `swaps` exchanges the ids of
# two objects before the frame is handed over: the tracker's mistake.  The caller adopts the ids the guard returns.
COL_A, COL_B = (40, 60, 220), (220, 120, 30)


def _frame(frame_id, tracks, colours, h, w, swaps=()):
    boxes = [b for _, b in tracks]
    img = render_scene(boxes, [np.asarray(colours[k], np.uint8) for k, _ in tracks], h, w, seed=1000 + frame_id)
    return dict(frame_id=frame_id, tracks=[(k, np.asarray(b, F32)) for k, b in tracks], img=img, swaps=list(swaps))


def pair_boxes(f, y=30, x0=60, gap=48, bw=40, bh=60):
    """S1's geometry: two boxes that cross along a row, 2 px a frame each; they touch while |4f - gap| < bw."""
    xa, xb = x0 + 2 * f, x0 + gap - 2 * f
    return [xa, y, xa + bw, y + bh], [xb, y, xb + bw, y + bh]


def s1_detections(frames=40):
    """S1 as the tracker sees it: per frame (xyxy, conf, cls, colours) with the detection order A, B for f <= 12 and B, A after."""
    out = []
    for f in range(frames):
        a, b = pair_boxes(f)
        order = [(a, COL_A), (b, COL_B)] if f <= 12 else [(b, COL_B), (a, COL_A)]
        xy = np.asarray([o[0] for o in order], F32)
        out.append((xy, np.full(2, 0.9, F32), np.zeros(2, np.int32), [o[1] for o in order]))
    return out, 120, 320


def s1_frames(frames=40):
    dets, h, w = s1_detections(frames)
    return [(render_scene(xy, [np.asarray(c, np.uint8) for c in col], h, w, seed=1000 + f), xy, cf, cl) for f, (xy, cf, cl, col) in enumerate(dets)], h, w


def scene_pair(colours=(COL_A, COL_B), first=0, frames=40, swap_at=13, mutate=None, h=120, w=320):
    """S1's two objects as a scripted scene: ids exchanged at `swap_at`; `mutate(f, tracks)` edits a frame's list."""
    col = {"a": colours[0], "b": colours[1]}
    out = []
    for f in range(first, frames):
        a, b = pair_boxes(f)
        tracks = [("a", a), ("b", b)]
        if mutate is not None:
            tracks = mutate(f, tracks)
        out.append(_frame(f, tracks, col, h, w, swaps=[("a", "b")] if f == swap_at else ()))
    return dict(h=h, w=w, frames=out, ids0={"a": 1, "b": 2})


def scene_s2():
    """S2: a chain.  B sits between A and C; A's partner is B, B's partner is C (the larger overlap), C's partner is B.  A and B
    exchange ids while they touch; afterwards row[A] names B but row[B] names C: not mutual, no revert."""
    col = {"a": COL_A, "b": COL_B, "c": (30, 200, 60)}
    out = []
    for f in range(16):
        d = 0 if f < 4 else (f - 3 if f < 8 else 4)            # A and C close in on B during frames 4..7 ...
        if f >= 10:
            d = 0                                              # ... and are apart again from frame 10
        xb = 130
        xa, xc = 70 + 6 * d, 190 - 8 * d                       # at d = 4: A overlaps B by 4 px, C overlaps B by 12 px
        tracks = [("a", [xa, 30, xa + 40, 90]), ("b", [xb, 30, xb + 40, 90]), ("c", [xc, 30, xc + 40, 90])]
        out.append(_frame(f, tracks, col, 120, 320, swaps=[("a", "b")] if f == 8 else ()))
    return dict(h=120, w=320, frames=out, ids0={"a": 1, "b": 2, "c": 3})


def scene_s3():
    """S3: same-colour twins.  The cross and the own similarity are equal, so min_gain_pm blocks the revert."""
    return scene_pair(colours=(COL_A, COL_A))


def scene_s4_nan_corner():
    """A blind track: at frame 22, the first contact-free frame, A's box has a NaN corner; the revert waits for frame 23."""
    def mutate(f, tracks):
        if f == 22:
            b = list(tracks[0][1]); b[2] = float("nan")
            tracks[0] = ("a", b)
        return tracks
    return scene_pair(mutate=mutate)


def scene_s4_outside():
    """A blind track: B's box lies outside the frame from frame 22 to 25; the window passes and nothing is reverted."""
    def mutate(f, tracks):
        if 22 <= f <= 25:
            tracks[1] = ("b", [400, 30, 440, 90])
        return tracks
    return scene_pair(mutate=mutate)


def scene_s4_gap(absent):
    """One track seen on frames 0..3, absent for `absent` frames, then seen again twice (max_gap_frames = 4)."""
    col = {"a": COL_A}
    fr = list(range(4)) + [4 + absent - 1 + k for k in (1, 2)]
    return dict(h=120, w=320, frames=[_frame(f, [("a", [60, 30, 100, 90])], col, 120, 320) for f in fr], ids0={"a": 7})


def scene_s4_short_history():
    """The pair starts at frame 1: two contact-free frames before the contact, count = 2 < min_history at frame 22 (window = 1)."""
    return scene_pair(first=1)


def scene_s4_window(returns_at):
    """Neither track is passed from frame 22 until `returns_at`: 24 is inside the window (24 - 21 = 3), 25 is one frame too late."""
    def mutate(f, tracks):
        return [] if 22 <= f < returns_at else tracks
    return scene_pair(mutate=mutate)


def scene_s5(frames=26, swap_at=14):
    """S5: 64 tracks as 32 crossing pairs in one 360 x 640 frame (4 columns x 8 rows of cells); the even pairs exchange ids."""
    h, w = 360, 640
    col, ids0 = {}, {}
    for p in range(32):
        col[2 * p], col[2 * p + 1] = PALETTE[p % 12], PALETTE[(p + 5) % 12]
        ids0[2 * p], ids0[2 * p + 1] = 2 * p + 1, 2 * p + 2
    out = []
    for f in range(frames):
        tracks = []
        for p in range(32):
            cx, cy = 160 * (p % 4) + 10 + 2 * (p % 3), 45 * (p // 4) + 5
            a, b = pair_boxes(f, y=cy, x0=cx, gap=56, bw=20, bh=30)
            tracks += [(2 * p, a), (2 * p + 1, b)]
        out.append(_frame(f, tracks, col, h, w, swaps=[(2 * p, 2 * p + 1) for p in range(0, 32, 2)] if f == swap_at else ()))
    return dict(h=h, w=w, frames=out, ids0=ids0)


def scene_s6(frames=4):
    """S6: max_tracks = 4 and four fresh ids on every frame with a long max_gap_frames: the third frame needs 12 rows of 8."""
    col = {k: PALETTE[k % 12] for k in range(4 * frames)}
    out = []
    for f in range(frames):
        tracks = [(4 * f + k, [20 + 70 * k, 30, 60 + 70 * k, 90]) for k in range(4)]
        out.append(_frame(f, tracks, col, 120, 320))
    return dict(h=120, w=320, frames=out, ids0={k: 100 + k for k in range(4 * frames)})


FUZZ_SEEDS = (2, 49, 54)


def scene_s7(seed, n_obj=8, frames=140, h=180, w=320, bw=22, bh=30):
    """S7: random walks (reflected at the border) of coloured boxes; when two boxes begin to overlap (each the other's partner)
    their ids are exchanged with probability 0.8; now and then a box drops out for a few frames or leaves the frame."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0, w - bw, n_obj), rng.uniform(0, h - bh, n_obj)], 1)
    vel = rng.uniform(-3.0, 3.0, (n_obj, 2))
    col = {k: (PALETTE[k % 12] if k != 4 else PALETTE[0]) for k in range(n_obj)}       # objects 0 and 4 are twins
    hidden = np.zeros(n_obj, np.int64)
    touching_before = set()
    out = []
    for f in range(frames):
        pos += vel
        for d, lim in ((0, w - bw), (1, h - bh)):
            low, high = pos[:, d] < 0, pos[:, d] > lim
            pos[low, d], pos[high, d] = -pos[low, d], 2 * lim - pos[high, d]
            vel[low | high, d] *= -1
        boxes = {k: [float(F32(pos[k, 0])), float(F32(pos[k, 1])), float(F32(pos[k, 0] + bw)), float(F32(pos[k, 1] + bh))] for k in range(n_obj)}
        for k in range(n_obj):
            if hidden[k] == 0 and rng.uniform() < 0.01:
                hidden[k] = rng.integers(1, 5)
        tracks = [(k, boxes[k]) for k in range(n_obj) if hidden[k] == 0]
        hidden[hidden > 0] -= 1
        if rng.uniform() < 0.03 and tracks:
            k = int(rng.integers(len(tracks)))
            tracks[k] = (tracks[k][0], [w + 5, 10, w + 5 + bw, 10 + bh])                 # outside the frame: blind
        tracks = [tracks[i] for i in rng.permutation(len(tracks))]
        keys = [k for k, _ in tracks]
        pc = partners([b for _, b in tracks], 0.0)
        touching = {(min(keys[i], keys[j]), max(keys[i], keys[j])) for i, (j, t) in enumerate(pc) if t and pc[j][0] == i}
        swaps = [pair for pair in sorted(touching - touching_before) if rng.uniform() < 0.8]
        touching_before = touching
        out.append(_frame(f, tracks, col, h, w, swaps=swaps))
    return dict(h=h, w=w, frames=out, ids0={k: k + 1 for k in range(n_obj)})


def play(scene, process):
    """Plays a scene: process(ids, boxes (n, 4) float32, frame image, frame_id) -> (ids out, events).  The caller adopts the ids
    that come back.  Yields (frame_id, keys, ids handed over, ids returned, events) per frame."""
    idmap = dict(scene["ids0"])
    for fr in scene["frames"]:
        for ka, kb in fr["swaps"]:
            idmap[ka], idmap[kb] = idmap[kb], idmap[ka]
        keys = [k for k, _ in fr["tracks"]]
        ids = [idmap[k] for k in keys]
        boxes = np.asarray([b for _, b in fr["tracks"]], F32).reshape(len(keys), 4)
        ids_out, events = process(ids, boxes, fr["img"], fr["frame_id"])
        for k, i in zip(keys, ids_out):
            idmap[k] = int(i)
        yield fr["frame_id"], keys, ids, [int(i) for i in ids_out], events, dict(idmap)


def play_ref(scene, **kw):
    """The restatement alone: (the guard, every event, the final object -> id map)."""
    ref = SwapGuardRef(**kw)
    events, idmap = [], dict(scene["ids0"])
    for _, _, _, _, ev, idmap in play(scene, ref.process_frame):
        events += ev
    return ref, events, idmap


def run_tracker_s1(assign, guard: SwapGuardRef | None):
    """S1 through the tracker oracle (TrackerOracle(0.5, 30, 0.8, assign)); with a guard the oracle adopts the corrected ids, as
    rtmodt_swapguard_process_tracker writes them into the tracker's state.  Returns (per frame {colour: id}, events)."""
    frames, _, _ = s1_frames()
    dets, _, _ = s1_detections()
    trk = TrackerOracle(0.5, 30, 0.8, assign)
    seen, events = [], []
    for f, (img, xy, cf, cl) in enumerate(frames):
        trk.update(xy, cf, cl)
        passed = np.nonzero(trk.tsu == 1)[0]
        if guard is not None:
            out, ev = guard.process_frame(trk.ids[passed], trk.xyxy[passed], img, f)
            trk.ids[passed] = out
            events += [dict(e, track_a=int(passed[e["track_a"]]), track_b=int(passed[e["track_b"]])) for e in ev]
        who = {}
        for i in passed:
            for (box, colour) in zip(dets[f][0], dets[f][3]):
                if np.array_equal(box, trk.xyxy[i]):
                    who[colour] = int(trk.ids[i])
        seen.append(who)
    return seen, events
