"""Times the zone engine's kernel (zones_update: 200 tracks x 16 zones per stream) in its four call shapes, in the same run on the same
box: on the device-resident state of a ByteTrack handle of 8 streams and of 1 stream (one launch per frame each), and on track lists
the host hands over, stream by stream through an engine of 8 streams (8 launches per frame) and through an engine of 1 stream.
Nothing is asserted: the numbers are reported, not gated.

The launch is not bracketed by HIP events inside the library, so its device time is taken as tools/crossing_time.py takes it, from
the profiler's kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/zones_time.py --repeat 120
    python tools/zones_time.py --summarize OUT [--out profiles/track_ledger/zones_time.json]

The first form runs the workload (and prints the wall clock of the synchronous calls, list staging included); the second reads the
trace and writes the median device time per call shape over the frames after the warm-up.  Per frame the workload launches
zones_update 11 times, in this order: tracker 8 streams, tracker 1 stream, lists stream 0..7 of the 8-stream engine, list of the
1-stream engine; the summary tells the series apart by that order.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time
from importlib import import_module
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from crossing_time import items  # noqa: E402

WARMUP = 10
S = 8
SHAPES = ("tracker_8_streams", "tracker_1_stream", "lists_8_streams", "list_1_stream")
PER_FRAME = 1 + 1 + S + 1


def workload(repeat, n=200):
    import rtmodt_amd
    bt_cls = import_module(rtmodt_amd.__name__ + ".tracking.tracker")._ByteTrackCore
    zones = items()[0]
    with tempfile.TemporaryDirectory(prefix="zones_time_") as tmp:              # the engines' alert logs go with the run
        mk = lambda k, streams: rtmodt_amd.events.ZoneEventEngine(zones, log_path=os.path.join(tmp, f"e{k}.jsonl"), n_streams=streams, max_tracks=256,
                                                                 max_events=4096)
        engines = [mk(0, S), mk(1, 1), mk(2, S), mk(3, 1)]
        bts = [bt_cls(n_streams=S, max_tracks=256, max_dets=256), bt_cls(n_streams=1, max_tracks=256, max_dets=256)]
        _workload(engines, bts, repeat, n)
        for h in engines + bts:
            h.close()


def _workload(engines, bts, repeat, n):
    trks = [SimpleNamespace(_core=bt, report="matched") for bt in bts]
    base = np.asarray([[(k % 20) * 90 + 10, (k // 20) * 100 + 10] for k in range(n)], np.float32)
    conf = np.zeros((S, 256), np.float32); conf[:, :n] = 0.9
    cls = np.zeros((S, 256), np.int32); cls[:, :n] = np.arange(n) % 80
    cnt = np.full(S, n, np.int32)
    xy = np.zeros((S, 256, 4), np.float32)
    order = np.random.default_rng(3).permutation(n)                             # the lists arrive shuffled: the staging sorts them
    wall = {k: [] for k in SHAPES}
    n_ev = {k: 0 for k in SHAPES}
    for t in range(WARMUP + repeat):
        phase = t % 60
        dx = 4 * (phase if phase < 30 else 60 - phase)         # every box drifts 120 px to the right and back: matched on every frame
        for s in range(S):
            xy[s, :n, 0] = base[:, 0] + dx + s; xy[s, :n, 1] = base[:, 1]
            xy[s, :n, 2] = xy[s, :n, 0] + 60; xy[s, :n, 3] = xy[s, :n, 1] + 60
        bts[0].update_batch(xy, conf, cls, cnt)
        bts[1].update_batch(xy[:1], conf[:1], cls[:1], cnt[:1])
        lists = [[SimpleNamespace(track_id=int(k) + 1, xyxy=xy[s, k].copy(), class_id=int(cls[s, k]), class_name="") for k in order] for s in range(S)]
        now = 100.0 + 0.04 * t
        t0 = time.perf_counter()
        ev = [engines[0].process_tracker(trks[0], t, now=now)]
        t1 = time.perf_counter()
        ev.append(engines[1].process_tracker(trks[1], t, now=now))
        t2 = time.perf_counter()
        ev.append([engines[2].process(lists[s], t, stream=s, now=now) for s in range(S)])
        t3 = time.perf_counter()
        ev.append([engines[3].process(lists[0], t, now=now)])
        t4 = time.perf_counter()
        if t >= WARMUP:
            for k, dt, e in zip(SHAPES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3), ev):
                wall[k].append(dt * 1e3)
                n_ev[k] += sum(map(len, e))
    out = {"load": {"tracks_per_stream": n, "zones": 16, "frames": repeat, "warmup": WARMUP, "zones_update_launches_per_frame": PER_FRAME},
           "wall_ms_median_per_frame": {k: float(np.median(v)) for k, v in wall.items()},
           "note": "lists_8_streams is eight synchronous calls (sort, six copies, launch, fetch each)", "events": n_ev}
    print(json.dumps(out))


def summarize(directory, out_path):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    dur = []
    for path in files:
        with open(path, newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        dur += [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "zones_update" in r["Kernel_Name"]]
    if len(dur) % PER_FRAME or len(dur) < PER_FRAME * (WARMUP + 100):
        raise SystemExit(f"{len(dur)} zones_update launches: not {PER_FRAME} per frame of at least {WARMUP + 100} frames")
    frames = np.asarray(dur).reshape(-1, PER_FRAME)[WARMUP:]
    series = {"tracker_8_streams": frames[:, 0], "tracker_1_stream": frames[:, 1], "lists_8_streams": frames[:, 2:2 + S].ravel(), "list_1_stream": frames[:, 2 + S]}
    out = {"kernel_device_time_us": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90)), "launches": int(v.size)}
                                     for k, v in series.items()},
           "how": "rocprofv3 --kernel-trace device timestamps of every zones_update launch in one run of tools/zones_time.py; the first "
                  f"{WARMUP} frames are dropped; lists_8_streams is per launch (one stream)", "files": [os.path.relpath(p, directory) for p in files]}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=120)
    ap.add_argument("--summarize", metavar="DIR", help="read the kernel trace a profiled run left under DIR")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.out)
    else:
        workload(a.repeat)


if __name__ == "__main__":
    main()
