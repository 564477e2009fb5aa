"""Times the speed estimator's kernels (speed_update, speed_pairs: 8 streams x 200 sampled tracks, proximity off and on) beside the
crossing counter's (crossing_update: the same tracks, 8 lines + 8 gates), all on the device-resident state of one ByteTrack handle,
in the same run on the same box.  Nothing is asserted: the numbers are reported, not gated.

The launches are not bracketed by HIP events inside the library, so the device time of every kernel is taken the same way, from the
profiler's kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/speed_time.py --repeat 120
    python tools/speed_time.py --summarize OUT [--out profiles/speed/speed_time.json]

The first form runs the workload (and prints the wall clock of the synchronous calls); the second reads the trace and writes the
median device time per kernel over the launches after the warm-up.  Per frame the workload launches, in this order: crossing_update,
speed_update (estimator without proximity), speed_update + speed_pairs (estimator with proximity); the summary tells the two
speed_update series apart by that order.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time
from importlib import import_module
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

WARMUP = 10
PROXIMITY_MM = 2500


def workload(repeat, S=8, n=200):
    import rtmodt_amd
    bt = import_module(rtmodt_amd.__name__ + ".tracking.tracker")._ByteTrackCore(n_streams=S, max_tracks=256, max_dets=256)
    from crossing_time import items
    _, lines, gates = items()
    counter = rtmodt_amd.events.CrossingCounter(lines, gates, n_streams=S, max_tracks=256, max_events=4096)
    kw = dict(mm_per_pixel=25, window=8, hold=3, limit_mm_s=13_000, stop_mm_s=300, stop_us=500_000, wrong_way_min_mm_s=1000, allowed_dir=(1, 0), bins=64,
              bin_mm_s=500, n_streams=S, max_tracks=256, max_events=1024, max_pairs=4096)
    plain = rtmodt_amd.events.SpeedEstimator(**kw)
    prox = rtmodt_amd.events.SpeedEstimator(proximity_mm=PROXIMITY_MM, **kw)
    trk = SimpleNamespace(_core=bt, report="matched")
    base = np.asarray([[(k % 20) * 90 + 10, (k // 20) * 100 + 10] for k in range(n)], np.float32)
    conf = np.zeros((S, 256), np.float32); conf[:, :n] = 0.9
    cls = np.zeros((S, 256), np.int32); cls[:, :n] = np.arange(n) % 80
    cnt = np.full(S, n, np.int32)
    xy = np.zeros((S, 256, 4), np.float32)
    wall = {"crossing": [], "speed": [], "speed_proximity": [], "speed_no_outputs": []}
    n_ev, n_pairs = [0, 0], 0
    quiet = rtmodt_amd.events.SpeedEstimator(**kw)
    for t in range(WARMUP + repeat):
        phase = t % 60
        dx = 4 * (phase if phase < 30 else 60 - phase)         # every box drifts 120 px to the right and back: matched on every frame
        for s in range(S):
            xy[s, :n, 0] = base[:, 0] + dx + s; xy[s, :n, 1] = base[:, 1]
            xy[s, :n, 2] = xy[s, :n, 0] + 60; xy[s, :n, 3] = xy[s, :n, 1] + 60
        bt.update_batch(xy, conf, cls, cnt)
        t0 = time.perf_counter()
        ec = counter.process_tracker(trk, t)
        t1 = time.perf_counter()
        es = plain.process_tracker(trk, t * 40_000)
        t2 = time.perf_counter()
        prox.process_tracker(trk, t * 40_000)
        t3 = time.perf_counter()
        if t >= WARMUP:
            wall["crossing"].append((t1 - t0) * 1e3); wall["speed"].append((t2 - t1) * 1e3); wall["speed_proximity"].append((t3 - t2) * 1e3)
            n_ev[0] += sum(map(len, ec)); n_ev[1] += sum(map(len, es)); n_pairs += sum(prox.last_total_pairs)
    # the call without outputs returns without waiting for the device: its wall clock is the enqueue (timed apart: it adds launches to the trace)
    for t in range(WARMUP + repeat, WARMUP + repeat + 20):
        bt.update_batch(xy, conf, cls, cnt)
        t0 = time.perf_counter()
        quiet.process_tracker(trk, t * 40_000, outputs=False)
        wall["speed_no_outputs"].append((time.perf_counter() - t0) * 1e3)
    quiet.snapshot()
    sampled = len(plain.last_rows[0])
    out = {"load": {"streams": S, "sampled_tracks_per_stream": sampled, "lines": len(lines), "gates": len(gates), "window": kw["window"], "bins": kw["bins"],
                    "proximity_mm": PROXIMITY_MM, "launches": repeat, "warmup": WARMUP},
           "wall_ms_median_of_the_call": {k: float(np.median(v)) for k, v in wall.items()},
           "events": {"crossing": n_ev[0], "speed": n_ev[1]}, "pairs_per_frame_all_streams": n_pairs / repeat,
           "p85_mm_s_stream0": plain.percentile(85)}
    print(json.dumps(out))
    for x in (counter, plain, prox, quiet, bt):
        x.close()


def summarize(directory, out_path):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    rows = []
    for path in files:
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = {"crossing_update": [], "speed_update": [], "speed_update_before_pairs": [], "speed_pairs": []}
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    names = [r["Kernel_Name"] for r in rows]
    for i, r in enumerate(rows):
        if "crossing_update" in names[i]:
            dur["crossing_update"].append(us(r))
        elif "speed_pairs" in names[i]:
            dur["speed_pairs"].append(us(r))
        elif "speed_update" in names[i]:
            nxt = next((n for n in names[i + 1:i + 2]), "")
            dur["speed_update_before_pairs" if "speed_pairs" in nxt else "speed_update"].append(us(r))
    n_timed = len(dur["crossing_update"]) - WARMUP
    out = {"kernel_device_time_us": {}, "how": "rocprofv3 --kernel-trace device timestamps of every launch in one run of tools/speed_time.py; the first "
                                               f"{WARMUP} launches of each kernel are dropped; speed_update_before_pairs is the update launch of the estimator "
                                               "with proximity on (the same kernel, followed by speed_pairs)",
           "files": [os.path.relpath(p, directory) for p in files]}
    for k, v in dur.items():
        v = v[WARMUP:WARMUP + n_timed]                      # (the no-output launches at the end of the workload are left out)
        if len(v) < 100:
            raise SystemExit(f"{k}: {len(v)} launches after the warm-up, need at least 100")
        out["kernel_device_time_us"][k] = {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90)), "launches": len(v)}
    m = {k: v["median"] for k, v in out["kernel_device_time_us"].items()}
    out["speed_over_crossing"] = m["speed_update"] / m["crossing_update"]
    out["speed_with_pairs_over_crossing"] = (m["speed_update_before_pairs"] + m["speed_pairs"]) / m["crossing_update"]
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
