"""The reference's tracker comparison (TECHNICAL_DESIGN_DOCUMENT.md H.2) on this project's three trackers: ByteTrack
(MultiObjectTracker), DeepSORT with the colour-histogram descriptor (DeepSortTracker) and OC-SORT (OcSortTracker) run over the same
seeded synthetic sequences (tests/deepsort_ref.py: crossing pairs that occlude one another, and constant-velocity objects with
detection drop-outs and one-off detections, rendered so that the appearance descriptor has pixels to read).  Prints H.2's columns
-- IDF1, MOTA, MOTP, ID switches, per-frame tracker time, whether a Re-ID model is needed -- plus HOTA / DetA / AssA, all from
rtmodt_mot_eval / rtmodt_hota_eval on the GPU.  Synthetic scenes, so the figures rank the trackers on these scenes only: they are not
the design document's MOT17 figures.  Nothing is asserted.

    python tools/compare_trackers.py [--out profiles/ocsort/compare_trackers.json]
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


def make(kind):
    if kind == "bytetrack":
        trk = pkg.MultiObjectTracker("bytetrack")
        trk.report = "matched"                              # the tracks matched or spawned this frame (the default mirrors the reference and returns none)
        return trk, False
    if kind == "deepsort":
        return pkg.DeepSortTracker(max_tracks=64, max_dets=32), True
    return pkg.OcSortTracker(max_tracks=64, max_dets=32), False


def run(kind, frames):
    trk, needs_frame = make(kind)
    hyp, ms = [], []
    for f, (img, xy, cf, cl, _) in enumerate(frames):
        det = pkg.Detections(xy, cf, cl)
        t0 = time.perf_counter()
        tracks = trk.update(det, frame=img) if needs_frame else trk.update(det)
        ms.append((time.perf_counter() - t0) * 1e3)
        hyp += [[f + 1, t.track_id, t.xyxy[0], t.xyxy[1], t.xyxy[2] - t.xyxy[0], t.xyxy[3] - t.xyxy[1]] for t in tracks]
    if hasattr(trk, "close"):
        trk.close()
    return np.asarray(hyp, np.float64).reshape(-1, 6), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocsort", "compare_trackers.json"))
    a = ap.parse_args()
    from importlib import import_module
    M = import_module(pkg.__name__ + ".evaluation.metrics")
    seqs = sequences()
    gts = {n: np.asarray([[f + 1, int(o), b[0], b[1], b[2] - b[0], b[3] - b[1]] for f, (_, xy, _, _, ids) in enumerate(fr) for o, b in zip(ids, xy)],
                         np.float64).reshape(-1, 6) for n, fr in seqs.items()}
    rows = {}
    for kind, reid in (("bytetrack", "No"), ("deepsort", "Yes (colour histogram here)"), ("ocsort", "No")):
        pairs, ms = [], []
        for n, fr in seqs.items():
            hyp, t = run(kind, fr)
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
    cols = list(next(iter(rows.values())))
    print("| Tracker | " + " | ".join(cols) + " |")
    print("|" + "---|" * (len(cols) + 1))
    for kind, r in rows.items():
        print(f"| {kind} | " + " | ".join(f"{r[c]:.3f}" if isinstance(r[c], float) else str(r[c]) for c in cols) + " |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"sequences": {n: len(fr) for n, fr in seqs.items()}, "rows": rows, "command": "python tools/compare_trackers.py"}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
