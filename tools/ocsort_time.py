"""Times the OC-SORT tracker at 8 streams x 100 detections x 100 tracks: kernel time (HIP events) of the single launch of one call,
beside the ByteTrack call at the same load (wall clock of both synchronous calls, like for like) and the CPU time of the restatement
(tests/ocsort_ref.py) for one stream's frame.  Nothing is asserted: the numbers are reported, not gated.  Writes one JSON document.

    python tools/ocsort_time.py [--repeat 50] [--out profiles/ocsort/ocsort_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rtmodt_amd  # noqa: E402


def boxes_at(S, n, t, seed=0):
    """n boxes per stream on a 96-px grid, drifting a quarter pixel per frame; every eighth box of a stream skips every fifth frame."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    base = np.stack([(np.arange(n) % side) * 96.0 + 8, (np.arange(n) // side) * 96.0 + 8], 1)
    wh = np.round(rng.uniform(28, 40, (n, 2)) * 4) / 4
    p = base + 0.25 * t
    xy = np.concatenate([p, p + wh], 1).astype(np.float32)
    keep = ~((np.arange(n) % 8 == 0) & (t % 5 == 4))
    return [xy[keep] for _ in range(S)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocsort", "ocsort_time.json"))
    a = ap.parse_args()
    S, n, N = a.streams, a.dets, 128
    core = import_module(rtmodt_amd.__name__ + ".tracking.ocsort")._OcSortCore(n_streams=S, max_tracks=256, max_dets=N)
    bt = import_module(rtmodt_amd.__name__ + ".tracking.tracker")._ByteTrackCore(n_streams=S, max_tracks=256, max_dets=N)
    import ocsort_ref as R
    ref = R.OcSortRef()
    warm, times, ref_ms = 10, [], []
    for t in range(warm + a.repeat):
        per = boxes_at(S, n, t)
        xy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32)
        cnt = np.zeros(S, np.int32)
        for s, b in enumerate(per):
            xy[s, :len(b)], conf[s, :len(b)], cnt[s] = b, 0.9, len(b)
        t0 = time.perf_counter()
        core.update_batch(xy, conf, cls, cnt)
        oc_wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        bt.update_batch(xy, conf, cls, cnt)
        bt_wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref.update(per[0], conf[0, :cnt[0]], cls[0, :cnt[0]])
        r_ms = (time.perf_counter() - t0) * 1e3
        if t >= warm:
            times.append((core.last_ms(), oc_wall, bt_wall))
            ref_ms.append(r_ms)
    st = core.snapshot(0)
    tm = np.asarray(times)
    out = {
        "load": {"streams": S, "detections_per_stream": n, "tracks_per_stream": int(len(st["ids"])), "max_tracks": 256, "max_dets": N, "repeat": a.repeat},
        "measured_kernel_ms_median": float(np.median(tm[:, 0])), "measured_kernel_ms_min": float(tm[:, 0].min()),
        "measured_ocsort_update_batch_wall_ms_median": float(np.median(tm[:, 1])),
        "measured_bytetrack_update_batch_wall_ms_median": float(np.median(tm[:, 2])),
        "measured_restatement_cpu_ms_per_stream_frame_median": float(np.median(ref_ms)),
        "how": "HIP events around the one launch of rtmodt_ocsort_update_batch (rtmodt_ocsort_last_ms); the two wall-clock figures are taken the same way, "
               "around the synchronous rtmodt_ocsort_update_batch / rtmodt_tracker_update_batch (host copies of the detections and the Python marshalling "
               "included) -- compare those two with each other, not with the kernel time",
        "command": "python tools/ocsort_time.py --repeat %d" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
