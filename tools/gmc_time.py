"""Times the camera-motion estimator: 8 x 1080p BGR24 frames resident in HBM, downscale 4 and 2.  Per configuration: the host-timed
median of 5 synchronous rtmodt_gmc_estimate_batch calls, the device time (HIP events) of the six launches, the floor of reading the
frames once from HBM, and the device time of BoT-SORT's own update (rtmodt_botsort_last_ms, motion only, 32 tracks per stream) fed
the estimated warps in the same run.  Nothing is asserted: the numbers are reported, not gated.  Writes one JSON document.

    python tools/gmc_time.py [--repeat 5] [--out profiles/gmc/gmc_time.json]
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
import gmc_ref as G  # noqa: E402

HBM_BYTES_PER_S = 8.0e12                                    # MI355X data sheet: 8 TB/s
S, H, W = 8, 1080, 1920
STEPS = [(12, -8), (-20, 16), (0, 28), (24, 24), (-16, -4)]


def measure(d, repeat, warm=2):
    T = import_module(rtmodt_amd.__name__ + ".tracking")
    ffi = rtmodt_amd._ffi
    est = T.gmc.CameraMotionEstimator(downscale=d, n_streams=S)
    bot = T.botsort._BotSortCore(n_streams=S, max_tracks=256, max_dets=32)
    cv = G.canvas(H + 160, W + 160, 9)
    views = [G.crop(cv, 80 + x, 80 + y, H, W) for x, y in [(0, 0)] + STEPS]
    fbytes = H * W * 3
    bufs = []                                                # two sets of 8 frames in HBM, every stream with its own phase of the pan
    for k in range(2):
        b = ffi.DeviceBuffer(S * fbytes)
        for s in range(S):
            b.upload(views[(k + s) % len(views)], s * fbytes)
        bufs.append(b)
    rng = np.random.default_rng(0)
    p = rng.uniform(100, 900, (32, 2))
    xy = np.tile(np.concatenate([p, p + 40], 1).astype(np.float32), (S, 1, 1))
    conf, cls, cnt = np.full((S, 32), 0.9, np.float32), np.zeros((S, 32), np.int32), np.full(S, 32, np.int32)
    host, dev, upd, ok = [], [], [], 0
    for t in range(warm + repeat):
        ptrs = [bufs[t % 2].ptr + s * fbytes for s in range(S)]
        t0 = time.perf_counter()
        warp, status = est.estimate(ptrs, mem_kind=ffi.MEM_DEVICE, height=H, width=W, stride=3 * W)
        t1 = time.perf_counter()
        bot.update_batch(xy, conf, cls, cnt, warp=warp)
        if t >= warm:
            host.append((t1 - t0) * 1e3)
            dev.append(est.last_ms())
            upd.append(bot.last_ms()[2])
            ok += int((status == 0).sum())
    g = est.geometry()
    est.close(); bot.close()
    for b in bufs:
        b.free()
    floor = S * fbytes / HBM_BYTES_PER_S * 1e3
    return {"downscale": d, "streams": S, "frame": [W, H], "blocks_per_stream": g["nb"], "estimated_ok": ok, "of": repeat * S,
            "host_call_ms": float(np.median(host)), "kernels_ms": float(np.median(dev)), "hbm_read_floor_ms": floor,
            "kernels_over_floor": float(np.median(dev) / floor), "botsort_update_ms": float(np.median(upd))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmc", "gmc_time.json"))
    a = ap.parse_args()
    out = {
        "loads": [measure(d, a.repeat) for d in (4, 2)],
        "how": "medians over the repeats; host_call_ms: time.perf_counter around one synchronous estimate_batch on frames already in HBM (checks, "
               "six launches, copy of 8 warps and statuses); kernels_ms: HIP events around the six launches (rtmodt_gmc_last_ms); the floor assumes "
               "8 TB/s; botsort_update_ms: rtmodt_botsort_last_ms's update part, motion only, 32 detections per stream, fed the estimated warps",
        "command": "python tools/gmc_time.py --repeat %d" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
