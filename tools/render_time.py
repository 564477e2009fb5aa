"""Times one FrameRenderer.render_batch of 8 x 1080p BGR24 frames, 200 tracks each (30-point trails) and 2 zones:
device-resident frames (drawn in place: wall time per batch and the kernel's HIP-event time), host frames (upload, draw,
download) and the NumPy restatement tests/render_ref.py on the CPU for comparison.  Prints one JSON line.

    python tools/render_time.py [--iters 50] [--out profiles/render/render_time.json]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rtmodt_amd  # noqa: E402,F401
import render_ref  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W, TRACKS, TRAIL = 8, 1080, 1920, 200, 30
ZONES = [("entrance", np.array([[200, 300], [900, 250], [1000, 800], [300, 900]], np.int32)),
         ("loading bay", np.array([[1100, 200], [1800, 300], [1700, 1000], [1200, 900], [1400, 600]], np.int32))]


def scene(rng):
    out = []
    for i in range(TRACKS):
        x1, y1 = rng.uniform(0, W - 120), rng.uniform(0, H - 200)
        bw, bh = rng.uniform(20, 120), rng.uniform(40, 200)
        cx, cy = int(x1 + bw / 2), int(y1 + bh / 2)
        trail = [(cx - 3 * (TRAIL - k), cy - 2 * (TRAIL - k)) for k in range(TRAIL)]
        out.append(SimpleNamespace(track_id=i, xyxy=np.array([x1, y1, x1 + bw, y1 + bh], np.float32), confidence=np.float32(rng.uniform(0.3, 1)),
                                   class_name="person", trail=trail))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [scene(rng) for _ in range(N)]
    r = pkg.FrameRenderer()
    dev = pkg._ffi.DeviceBuffer(frames.nbytes)
    dev.upload(frames)

    def device_batch():
        r.render_batch(dev, lists, zones=ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)

    for _ in range(5):
        device_batch()
    wall, kern = [], []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        device_batch()
        wall.append((time.perf_counter() - t0) * 1e6)
        kern.append(r.last_kernel_ms() * 1e3)

    host = [f.copy() for f in frames]
    r.render_batch(host, lists, zones=ZONES, fps=30.0, latency_ms=5.0)
    host_t = []
    for _ in range(max(args.iters // 5, 3)):
        t0 = time.perf_counter()
        r.render_batch(host, lists, zones=ZONES, fps=30.0, latency_ms=5.0)
        host_t.append((time.perf_counter() - t0) * 1e6)
    host_kern = r.last_kernel_ms() * 1e3

    # the device result of one fresh batch against the CPU restatement (frame 0), and its time
    dev.upload(frames)
    device_batch()
    got = dev.download(H * W * 3).reshape(H, W, 3)
    t0 = time.perf_counter()
    want = render_ref.render(frames[0], lists[0], ZONES, 30.0, 5.0)
    ref_us = (time.perf_counter() - t0) * 1e6 * N
    dev.free()

    # bytes a kernel that read and wrote every pixel would move (the estimate of the issue); the tiled kernel touches less
    full_rw = 2 * N * H * W * 3
    res = {"frames": N, "size": f"{W}x{H}", "tracks_per_frame": TRACKS, "trail_points": TRAIL, "zones": len(ZONES),
           "device_wall_us_p50": float(np.median(wall)), "device_wall_us_min": float(np.min(wall)),
           "kernel_us_p50": float(np.median(kern)), "kernel_us_min": float(np.min(kern)),
           "host_path_us_p50": float(np.median(host_t)), "host_path_kernel_us": host_kern,
           "cpu_ref_us_per_batch": ref_us, "full_frame_rw_bytes": full_rw,
           "full_frame_rw_equiv_GBps_at_kernel_p50": full_rw / (np.median(kern) * 1e-6) / 1e9,
           "bit_exact_frame0": bool(np.array_equal(got, want))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["bit_exact_frame0"] else 1


if __name__ == "__main__":
    sys.exit(main())
