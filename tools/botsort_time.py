"""Times the BoT-SORT tracker per call: device time (HIP events) of the launches of one rtmodt_botsort_update_batch at 8 and 64 streams
x 32 and 256 tracks per stream, with Re-ID (caller descriptors of 192 values: distance + update) and without (the update launch
alone, with a warp), beside OC-SORT and DeepSORT at the same load in the same run.  Nothing is asserted: the numbers are reported, not
gated.  Writes one JSON document.

    python tools/botsort_time.py [--repeat 30] [--out profiles/botsort/botsort_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rtmodt_amd  # noqa: E402

DIM = 192


def boxes_at(n, t, seed=0):
    """n boxes on a 96-px grid, drifting a quarter pixel per frame; every eighth box skips every fifth frame."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    base = np.stack([(np.arange(n) % side) * 96.0 + 8, (np.arange(n) // side) * 96.0 + 8], 1)
    wh = np.round(rng.uniform(28, 40, (n, 2)) * 4) / 4
    p = base + 0.25 * t
    xy = np.concatenate([p, p + wh], 1).astype(np.float32)
    keep = np.nonzero(~((np.arange(n) % 8 == 0) & (t % 5 == 4)))[0]
    return xy[keep], keep


def measure(S, n, repeat, warm=5):
    T = import_module(rtmodt_amd.__name__ + ".tracking")
    N = n
    kw = dict(n_streams=S, max_tracks=256, max_dets=N)
    bot_m = T.botsort._BotSortCore(**kw)
    bot_r = T.botsort._BotSortCore(embedder="colorhist", dim=DIM, **kw)
    oc = T.ocsort._OcSortCore(**kw)
    ds = T.deepsort._DeepSortCore(dim=DIM, **kw)
    rng = np.random.default_rng(1)
    rows = rng.integers(-127, 128, (n, DIM)).astype(np.int8)       # one descriptor per object
    warp = np.tile(np.asarray([1, 0, 0.25, 0, 1, 0.25], np.float32), (S, 1))   # the grid's own drift, as a camera would report it
    times = []
    for t in range(warm + repeat):
        b, keep = boxes_at(n, t)
        xy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32)
        emb = np.zeros((S, N, DIM), np.int8)
        xy[:, :len(b)], conf[:, :len(b)], emb[:, :len(b)] = b, 0.9, rows[keep]
        cnt = np.full(S, len(b), np.int32)
        bot_m.update_batch(xy, conf, cls, cnt, warp=warp)
        bot_r.update_batch(xy, conf, cls, cnt, embeddings=emb)
        oc.update_batch(xy, conf, cls, cnt)
        ds.update_batch(xy, conf, cls, cnt, embeddings=emb)
        if t >= warm:
            times.append((bot_m.last_ms()[2],) + bot_r.last_ms()[1:] + (oc.last_ms(),) + ds.last_ms()[1:])
    tm = np.median(np.asarray(times), axis=0)
    tracks = int(len(bot_r.snapshot(0, features=False)["ids"]))
    for c in (bot_m, bot_r, oc, ds):
        c.close()
    return {"streams": S, "detections_per_stream": n, "tracks_per_stream": tracks,
            "botsort_motion_only_update_ms": float(tm[0]),
            "botsort_reid_distance_ms": float(tm[1]), "botsort_reid_update_ms": float(tm[2]), "botsort_reid_total_ms": float(tm[1] + tm[2]),
            "ocsort_update_ms": float(tm[3]),
            "deepsort_distance_ms": float(tm[4]), "deepsort_update_ms": float(tm[5]), "deepsort_total_ms": float(tm[4] + tm[5])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "botsort", "botsort_time.json"))
    a = ap.parse_args()
    out = {
        "loads": [measure(S, n, a.repeat) for S in (8, 64) for n in (32, 256)],
        "how": "median over the repeats of the HIP-event times between the launches of one synchronous update_batch call "
               "(rtmodt_botsort_last_ms / rtmodt_ocsort_last_ms / rtmodt_deepsort_last_ms), all streams together; caller descriptors of 192 values, "
               "so no describe launch is in any figure; boxes on a grid (one admissible detection per track: the shortcut path of the assignment); "
               "DeepSORT at its default nn_budget of 100 rows per track, BoT-SORT at its one row per track",
        "command": "python tools/botsort_time.py --repeat %d" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
