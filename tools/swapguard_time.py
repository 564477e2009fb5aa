"""Times the ID-swap guard on the device-resident state of one ByteTrack handle: the device time of rtmodt_swapguard_process_tracker
(HIP events inside the library, read through rtmodt_swapguard_last_ms: the descriptor launches, and gather + step) beside the
ByteTrack update alone in the same run on the same box, for 8 streams x 50 and x 200 tracks on 1080p frames.  Medians of 5 after a
warm-up.  Nothing is asserted: the numbers are reported, not gated.

The tracker's update is not bracketed by HIP events inside the library (csrc/tracker.hip is not touched), so its figure is the wall
clock of the synchronous rtmodt_tracker_update_batch call; the guard's wall clock is reported next to it for a like-for-like pair.

    python tools/swapguard_time.py [--out profiles/swapguard/swapguard_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from importlib import import_module
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

WARMUP, REPEAT = 5, 5
H, W = 1080, 1920


def measure(pkg, S, n):
    ffi = pkg._ffi
    bt = import_module(pkg.__name__ + ".tracking.tracker")._ByteTrackCore(n_streams=S, max_tracks=256, max_dets=256)
    guard = pkg.tracking.IdSwapGuard(n_streams=S, max_tracks=256)
    trk = SimpleNamespace(_core=bt, report="matched")
    rng = np.random.default_rng(7)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bufs = [ffi.DeviceBuffer(frame.nbytes) for _ in range(S)]                  # device frames, as the detector holds them
    for b in bufs:
        b.upload(frame)
    base = np.asarray([[(k % 20) * 92 + 10, (k // 20) * 104 + 10] for k in range(n)], np.float32)
    conf = np.zeros((S, 256), np.float32); conf[:, :n] = 0.9
    cls = np.zeros((S, 256), np.int32)
    cnt = np.full(S, n, np.int32)
    xy = np.zeros((S, 256, 4), np.float32)
    rows = []
    for t in range(WARMUP + REPEAT):
        dx = 3 * (t % 20)                                   # every box drifts right: matched on every frame; neighbours 92 px apart, 70 px wide
        for s in range(S):
            xy[s, :n, 0] = base[:, 0] + dx + s; xy[s, :n, 1] = base[:, 1]
            xy[s, :n, 2] = xy[s, :n, 0] + 70; xy[s, :n, 3] = xy[s, :n, 1] + 96
        t0 = time.perf_counter()
        bt.update_batch(xy, conf, cls, cnt)
        t1 = time.perf_counter()
        guard.process_tracker(trk, [b.ptr for b in bufs], t, height=H, width=W, stride=3 * W, mem_kind=ffi.MEM_DEVICE)
        t2 = time.perf_counter()
        ms = guard.last_ms()
        if t >= WARMUP:
            rows.append((ms["describe"], ms["step"], (t2 - t1) * 1e3, (t1 - t0) * 1e3))
    passed = int((bt.snapshot(0)["tsu"] == 1).sum())
    stored = sum(r[2] for r in guard.state(0))
    a = np.median(np.asarray(rows), axis=0)
    for b in bufs:
        b.free()
    guard.close(); bt.close()
    return {"streams": S, "tracks_per_stream": n, "passed_tracks_stream0": passed, "descriptors_stored_stream0": int(stored),
            "guard_device_ms": {"describe": float(a[0]), "gather_and_step": float(a[1]), "total": float(a[0] + a[1])},
            "guard_wall_ms_of_the_synchronous_call": float(a[2]), "bytetrack_update_wall_ms_of_the_synchronous_call": float(a[3])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rtmodt_amd
    out = {"how": f"medians of {REPEAT} calls after {WARMUP}; the guard's device time from HIP events inside the library (rtmodt_swapguard_last_ms), "
                  "wall clocks from time.perf_counter around the synchronous calls; 1080p device frames; launches per call: 1 gather + 2 descriptor + 1 step, "
                  "whatever the track count; nothing was measured before this feature existed",
           "loads": [measure(rtmodt_amd, 8, n) for n in (50, 200)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
