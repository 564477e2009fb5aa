"""The reference's tracker comparison (TECHNICAL_DESIGN_DOCUMENT.md H.2) on this project's four trackers: ByteTrack
(MultiObjectTracker), DeepSORT with the colour-histogram descriptor (DeepSortTracker), OC-SORT (OcSortTracker) and BoT-SORT
(BotSortTracker, once with the colour-histogram descriptor and once on motion only) run over the same seeded synthetic sequences (tests/deepsort_ref.py: crossing pairs that occlude one another, and constant-velocity objects with
detection drop-outs and one-off detections, rendered so that the appearance descriptor has pixels to read).  Prints H.2's columns
-- IDF1, MOTA, MOTP, ID switches, per-frame tracker time, whether a Re-ID model is needed -- plus HOTA / DetA / AssA, all from
rtmodt_mot_eval / rtmodt_hota_eval on the GPU.  Synthetic scenes, so the figures rank the trackers on these scenes only: they are not
the design document's MOT17 figures.  A second table repeats one scene under a panning camera (every box moves by the camera's offset,
half a box width a frame, out and back): the synthetic scene's true camera motion is handed to BoT-SORT as its warp; the other three
trackers get none, since they cannot use one.  Nothing is asserted.

    python tools/compare_trackers.py [--out profiles/botsort/compare_trackers.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rtmodt_amd as pkg  # noqa: E402


def sequences():
    import deepsort_ref as D
    scenes = {
        "crossing": D.crossing_scene(3, 110, seed=3),
        "occlusion": D.random_scene(11, 60, 5, gaps=((0, 8, 3), (1, 10, 4), (2, 12, 5), (3, 14, 9), (4, 20, 12))),
        "clutter": D.random_scene(21, 60, 6, gaps=((0, 5, 4), (1, 20, 6)), spurious=0.4),
        "fast": D.random_scene(31, 60, 6, gaps=((2, 15, 5), (3, 30, 8)), speed=6.0),
    }
    out = {}
    for name, (scene, h, w) in scenes.items():
        out[name] = [(D.render_scene(xy, col, h, w, seed=1000 + f), xy, cf, cl, ids) for f, (xy, cf, cl, ids, col) in enumerate(scene)]
    return out


def panning(scene, h, w, step=12.0, leg=6):
    """The scene seen by a camera that pans `step` px a frame, `leg` frames out and `leg` back: boxes in image coordinates, plus the
    image motion of every frame as a 2x3 warp (a translation)."""
    out, warps, off = [], [], 0.0
    for f, (xy, cf, cl, ids, col) in enumerate(scene):
        d = 0.0 if f == 0 else step * (1 if (f - 1) // leg % 2 == 0 else -1)
        off += d
        moved = (xy - np.asarray([off, 0, off, 0], np.float32)).astype(np.float32)
        warps.append(np.asarray([[1, 0, -d], [0, 1, 0]], np.float32))
        out.append((moved, cf, cl, ids, col))
    return out, warps


def panning_sequence():
    import deepsort_ref as D
    scene, h, w = D.random_scene(11, 60, 5, w=480, gaps=((0, 8, 3), (1, 10, 4), (2, 12, 5)))
    scene = [(xy + np.asarray([80, 0, 80, 0], np.float32), cf, cl, ids, col) for xy, cf, cl, ids, col in scene]
    moved, warps = panning(scene, h, w)
    return [(D.render_scene(xy, col, h, w, seed=3000 + f), xy, cf, cl, ids) for f, (xy, cf, cl, ids, col) in enumerate(moved)], warps


def make(kind):
    if kind == "bytetrack":
        trk = pkg.MultiObjectTracker("bytetrack")
        trk.report = "matched"                              # the tracks matched or spawned this frame (the default mirrors the reference and returns none)
        return trk, False
    if kind == "deepsort":
        return pkg.DeepSortTracker(max_tracks=64, max_dets=32), True
    if kind == "botsort":
        return pkg.BotSortTracker(embedder="colorhist", max_tracks=64, max_dets=32), True
    if kind == "botsort-motion":
        return pkg.BotSortTracker(max_tracks=64, max_dets=32), False
    return pkg.OcSortTracker(max_tracks=64, max_dets=32), False


def run(kind, frames, warps=None):
    trk, needs_frame = make(kind)
    warped = warps is not None and kind.startswith("botsort")
    hyp, ms = [], []
    for f, (img, xy, cf, cl, _) in enumerate(frames):
        det = pkg.Detections(xy, cf, cl)
        t0 = time.perf_counter()
        kw = dict(warp=warps[f]) if warped else {}
        tracks = trk.update(det, frame=img, **kw) if needs_frame else trk.update(det, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
        hyp += [[f + 1, t.track_id, t.xyxy[0], t.xyxy[1], t.xyxy[2] - t.xyxy[0], t.xyxy[3] - t.xyxy[1]] for t in tracks]
    if hasattr(trk, "close"):
        trk.close()
    return np.asarray(hyp, np.float64).reshape(-1, 6), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "botsort", "compare_trackers.json"))
    a = ap.parse_args()
    from importlib import import_module
    M = import_module(pkg.__name__ + ".evaluation.metrics")
    seqs = sequences()
    gts = {n: np.asarray([[f + 1, int(o), b[0], b[1], b[2] - b[0], b[3] - b[1]] for f, (_, xy, _, _, ids) in enumerate(fr) for o, b in zip(ids, xy)],
                         np.float64).reshape(-1, 6) for n, fr in seqs.items()}
    pan, pan_warps = panning_sequence()
    seqs_pan = {"occlusion under a pan": pan}
    gts.update({n: np.asarray([[f + 1, int(o), b[0], b[1], b[2] - b[0], b[3] - b[1]] for f, (_, xy, _, _, ids) in enumerate(fr) for o, b in zip(ids, xy)],
                              np.float64).reshape(-1, 6) for n, fr in seqs_pan.items()})
    kinds = (("bytetrack", "No"), ("deepsort", "Yes (colour histogram here)"), ("botsort", "Yes (colour histogram here)"), ("botsort-motion", "No"),
             ("ocsort", "No"))
    tables = {"rows": table(M, kinds, seqs, gts, None), "rows_panning": table(M, kinds, seqs_pan, gts, pan_warps)}
    for title, rows in tables.items():
        cols = list(next(iter(rows.values())))
        print(f"\n{title}\n| Tracker | " + " | ".join(cols) + " |")
        print("|" + "---|" * (len(cols) + 1))
        for kind, r in rows.items():
            print(f"| {kind} | " + " | ".join(f"{r[c]:.3f}" if isinstance(r[c], float) else str(r[c]) for c in cols) + " |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"sequences": {n: len(fr) for n, fr in {**seqs, **seqs_pan}.items()}, **tables,
                   "panning": "12 px a frame, 6 frames out and 6 back; BoT-SORT is handed the true image motion as its warp, the others none",
                   "command": "python tools/compare_trackers.py"}, f, indent=1)
        f.write("\n")


def table(M, kinds, seqs, gts, warps):
    rows = {}
    for kind, reid in kinds:
        pairs, ms = [], []
        for n, fr in seqs.items():
            hyp, t = run(kind, fr, warps)
            pairs.append((gts[n], hyp))
            ms.append(t)
        mot = M.mot_eval(pairs)
        tot = {k: sum(r[k] for r in mot) for k in ("num_objects", "num_predictions", "num_matches", "num_switches", "num_misses", "num_false_positives",
                                                   "idtp", "dist_sum")}
        hota = M.hota_eval(pairs)["combined"]["mean"]
        rows[kind] = {"IDF1": 2 * tot["idtp"] / max(1, tot["num_objects"] + tot["num_predictions"]),
                      "MOTA": 1 - (tot["num_misses"] + tot["num_switches"] + tot["num_false_positives"]) / max(1, tot["num_objects"]),
                      "MOTP": tot["dist_sum"] / max(1, tot["num_matches"] + tot["num_switches"]), "ID switches": tot["num_switches"],
                      "update wall ms (median per frame)": float(np.mean(ms)), "Req. Re-ID model": reid,
                      "HOTA": hota["HOTA"], "DetA": hota["DetA"], "AssA": hota["AssA"]}
    return rows


if __name__ == "__main__":
    main()
