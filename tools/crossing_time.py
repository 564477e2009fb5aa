"""Times the crossing counter's kernel (crossing_update: 8 streams x 200 passed tracks, 8 lines + 8 gates) beside the zone engine's
(zones_update: 8 streams x 200 tracks x 16 zones), both on the device-resident state of one ByteTrack handle, in the same run on the
same box.  Nothing is asserted: the numbers are reported, not gated.

Neither launch is bracketed by HIP events inside the library (the zone engine has none, and csrc/zones.hip is the yardstick: it is
not touched), so the device time of both kernels is taken the same way, from the profiler's kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/crossing_time.py --repeat 120
    python tools/crossing_time.py --summarize OUT [--out profiles/crossing/crossing_time.json]

The first form runs the workload (and prints the wall clock of the two synchronous calls); the second reads the trace and writes the
median device time per kernel over the launches after the warm-up.
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

WARMUP = 10
KERNELS = ("zones_update", "crossing_update")


def items():
    zones = [{"name": f"z{i}", "polygon": [[120 * i, 60 * (i % 4)], [120 * i + 300, 60 * (i % 4)], [120 * i + 300, 60 * (i % 4) + 500], [120 * i, 60 * (i % 4) + 500]],
              "dwell_time_sec": 0.5, "cooldown_sec": 1.0} for i in range(16)]
    lines = [{"name": f"l{i}", "a": [200 + 200 * i, 0], "b": [230 + 200 * i, 1080], "direction": ("both", "pos", "neg")[i % 3]} for i in range(8)]
    gates = [{"name": f"g{i}", "polygon": z["polygon"], "direction": (None, "left_to_right", "right_to_left", "top_to_bottom")[i % 4]}
             for i, z in enumerate(zones[:8])]
    return zones, lines, gates


def workload(repeat, S=8, n=200):
    import rtmodt_amd
    bt_cls = import_module(rtmodt_amd.__name__ + ".tracking.tracker")._ByteTrackCore
    zones, lines, gates = items()
    with tempfile.TemporaryDirectory(prefix="crossing_time_") as tmp:          # the zone engine's alert log goes with the run
        _workload(rtmodt_amd, bt_cls, zones, lines, gates, os.path.join(tmp, "events.jsonl"), repeat, S, n)


def _workload(rtmodt_amd, bt_cls, zones, lines, gates, log_path, repeat, S, n):
    bt = bt_cls(n_streams=S, max_tracks=256, max_dets=256)
    eng = rtmodt_amd.events.ZoneEventEngine(zones, log_path=log_path, n_streams=S, max_tracks=256, max_events=4096)
    counter = rtmodt_amd.events.CrossingCounter(lines, gates, n_streams=S, max_tracks=256, max_events=4096)
    trk = SimpleNamespace(_core=bt, report="matched")
    base = np.asarray([[(k % 20) * 90 + 10, (k // 20) * 100 + 10] for k in range(n)], np.float32)
    conf = np.zeros((S, 256), np.float32); conf[:, :n] = 0.9
    cls = np.zeros((S, 256), np.int32); cls[:, :n] = np.arange(n) % 80
    cnt = np.full(S, n, np.int32)
    xy = np.zeros((S, 256, 4), np.float32)
    wall = {"zones": [], "crossing": []}
    n_ev = [0, 0]
    for t in range(WARMUP + repeat):
        phase = t % 60
        dx = 4 * (phase if phase < 30 else 60 - phase)         # every box drifts 120 px to the right and back: matched on every frame
        for s in range(S):
            xy[s, :n, 0] = base[:, 0] + dx + s; xy[s, :n, 1] = base[:, 1]
            xy[s, :n, 2] = xy[s, :n, 0] + 60; xy[s, :n, 3] = xy[s, :n, 1] + 60
        bt.update_batch(xy, conf, cls, cnt)
        t0 = time.perf_counter()
        ez = eng.process_tracker(trk, t, now=100.0 + 0.04 * t)
        t1 = time.perf_counter()
        ec = counter.process_tracker(trk, t)
        t2 = time.perf_counter()
        if t >= WARMUP:
            wall["zones"].append((t1 - t0) * 1e3); wall["crossing"].append((t2 - t1) * 1e3)
            n_ev[0] += sum(map(len, ez)); n_ev[1] += sum(map(len, ec))
    passed = int((bt.snapshot(0)["tsu"] == 1).sum())
    out = {"load": {"streams": S, "passed_tracks_per_stream": passed, "zones": len(zones), "lines": len(lines), "gates": len(gates), "launches": repeat,
                    "warmup": WARMUP},
           "wall_ms_median_of_the_synchronous_call": {"zones_process_tracker": float(np.median(wall["zones"])),
                                                      "crossing_process_tracker": float(np.median(wall["crossing"]))},
           "events": {"zones": n_ev[0], "crossing": n_ev[1]}}
    print(json.dumps(out))
    eng.close(); counter.close(); bt.close()


def summarize(directory, out_path):
    dur = {k: [] for k in KERNELS}
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    for path in files:
        with open(path, newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"kernel_device_time_us": {}, "how": "rocprofv3 --kernel-trace device timestamps of every launch in one run of tools/crossing_time.py; the first "
                                               f"{WARMUP} launches of each kernel are dropped", "files": [os.path.relpath(p, directory) for p in files]}
    for k, v in dur.items():
        v = v[WARMUP:]
        if len(v) < 100:
            raise SystemExit(f"{k}: {len(v)} launches after the warm-up, need at least 100")
        out["kernel_device_time_us"][k] = {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90)), "launches": len(v)}
    z, c = out["kernel_device_time_us"]["zones_update"]["median"], out["kernel_device_time_us"]["crossing_update"]["median"]
    out["crossing_over_zones"] = c / z
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
