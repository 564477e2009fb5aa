"""Times the DeepSORT tracker at 8 streams x 1080p x 100 detections x 100 confirmed tracks x full galleries: kernel time (HIP
events) of the descriptor, distance and update parts of one call, beside the floor of reading the boxes' pixels once from HBM,
the ByteTrack call at the same load (wall clock of both synchronous calls, like for like), and the CPU time of the restatement (tests/deepsort_ref.py) for one stream's frame.
Nothing is asserted: the numbers are reported, not gated.  Writes one JSON document.

    python tools/deepsort_time.py [--repeat 20] [--out profiles/deepsort/deepsort_time.json]
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

_ffi = rtmodt_amd._ffi
HBM_BYTES_PER_S = 8.0e12                                    # MI355X data sheet: 8 TB/s


def scene(S, n, h, w, seed=0):
    """n boxes per stream on a grid (no overlap), each with its own colour; the boxes drift by a pixel per frame."""
    rng = np.random.default_rng(seed)
    cols, rows = 20, (n + 19) // 20
    bw, bh = w // cols - 16, h // rows - 16
    base = np.asarray([[(k % cols) * (w // cols) + 8, (k // cols) * (h // rows) + 8] for k in range(n)], np.float32)
    colours = rng.integers(0, 256, (S, n, 3), dtype=np.uint8)
    return base, bw, bh, colours


def frames_at(S, n, h, w, base, bw, bh, colours, t):
    out, boxes = [], np.zeros((S, n, 4), np.float32)
    for s in range(S):
        f = np.full((h, w, 3), 100, np.uint8)
        for k in range(n):
            x0, y0 = int(base[k, 0]) + (t % 4), int(base[k, 1]) + (t % 3)
            f[y0:y0 + bh, x0:x0 + bw] = colours[s, k]
            f[y0:y0 + bh // 2, x0:x0 + bw // 2] = colours[s, k] // 2 + (t * 7 + k) % 16           # the descriptor changes a little per frame
            boxes[s, k] = (x0, y0, x0 + bw, y0 + bh)
        out.append(f)
    return out, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--budget", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepsort", "deepsort_time.json"))
    a = ap.parse_args()
    S, n, h, w, B = a.streams, a.dets, 1080, 1920, a.budget
    core_cls = import_module(rtmodt_amd.__name__ + ".tracking.deepsort")._DeepSortCore
    bt_cls = import_module(rtmodt_amd.__name__ + ".tracking.tracker")._ByteTrackCore
    core = core_cls(n_streams=S, max_tracks=256, max_dets=128, nn_budget=B, n_init=3, max_age=70)
    bt = bt_cls(n_streams=S, max_tracks=256, max_dets=128)
    base, bw, bh, colours = scene(S, n, h, w)
    dev = [_ffi.DeviceBuffer(h * w * 3) for _ in range(S)]
    conf = np.zeros((S, 128), np.float32); conf[:, :n] = 0.9
    cls = np.zeros((S, 128), np.int32)
    cnt = np.full(S, n, np.int32)
    xy = np.zeros((S, 128, 4), np.float32)
    times = []
    fill = B + 3                                             # frames until every gallery is full and every track confirmed
    import deepsort_ref as R
    ref = R.DeepSortRef(nn_budget=B, n_init=3, max_age=70)
    ref_ms = []
    for t in range(fill + a.repeat):
        frames, boxes = frames_at(S, n, h, w, base, bw, bh, colours, t)
        for d, f in zip(dev, frames):
            d.upload(f)
        xy[:, :n] = boxes
        t0 = time.perf_counter()
        core.update_batch(xy, conf, cls, cnt, frames=[d.ptr for d in dev], mem_kind=_ffi.MEM_DEVICE, height=h, width=w, stride=3 * w)
        ds_wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        bt.update_batch(xy, conf, cls, cnt)
        bt_wall = (time.perf_counter() - t0) * 1e3
        if t >= fill:
            times.append(core.last_ms() + (bt_wall, ds_wall))
        if t < fill or t - fill < 3:                         # the restatement: one stream, same load
            desc = R.describe(frames[0], boxes[0])[0]
            t0 = time.perf_counter()
            ref.update(boxes[0], conf[0, :n], cls[0, :n], desc)
            if t >= fill:
                ref_ms.append((time.perf_counter() - t0) * 1e3)
    st = core.snapshot(0, gallery=False)
    tm = np.asarray(times)
    pixels = float(S * n * bw * bh * 3)
    out = {
        "load": {"streams": S, "frame": [h, w], "detections_per_stream": n, "box": [bw, bh], "confirmed_tracks_per_stream": int((st["state"] == 2).sum()),
                 "gallery_rows_per_track": int(st["gallery_count"].min()), "nn_budget": B, "repeat": a.repeat},
        "measured_kernel_ms_median": {"descriptor": float(np.median(tm[:, 0])), "distance": float(np.median(tm[:, 1])), "update": float(np.median(tm[:, 2]))},
        "measured_kernel_ms_min": {"descriptor": float(tm[:, 0].min()), "distance": float(tm[:, 1].min()), "update": float(tm[:, 2].min())},
        "floor_read_box_pixels_once_ms": pixels / HBM_BYTES_PER_S * 1e3,
        "box_pixel_bytes": pixels,
        "measured_bytetrack_update_batch_wall_ms_median": float(np.median(tm[:, 3])),
        "measured_deepsort_update_batch_wall_ms_median": float(np.median(tm[:, 4])),
        "measured_restatement_cpu_ms_per_stream_frame_median": float(np.median(ref_ms)) if ref_ms else None,
        "how": "HIP events around the three parts of rtmodt_deepsort_update_batch (rtmodt_deepsort_last_ms); the two wall-clock figures are taken the same way, around "
               "the synchronous rtmodt_tracker_update_batch / rtmodt_deepsort_update_batch (host copies of the detections and the Python marshalling "
               "included, frames already in HBM) -- compare those two with each other, not with the kernel times; the floor assumes 8 TB/s",
        "command": "python tools/deepsort_time.py --repeat %d" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
