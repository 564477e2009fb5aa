"""Times JpegEncoder.encode_batch on 8 x 1080p BGR24 frames as FrameRenderer.render_batch leaves them in device memory (structured
synthetic background with +-6 levels of sensor noise, 200 tracks with 30-point trails, 2 zones, HUD), at quality 95 and 85:
the kernels' HIP-event time, the whole call for device-resident frames and for host frames, the bytes per file, and on the same
frames Pillow's (libjpeg-turbo) encode time on one CPU thread and the time of the raw 50 MB device-to-host copy the JPEG path
replaces.  Frame 0 of every batch is compared with tests/jpeg_ref.py.  Prints one JSON line.

    python tools/jpeg_time.py [--iters 50] [--out profiles/jpeg/jpeg_time.json]
"""
import argparse
import io
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
import jpeg_ref  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W, TRACKS, TRAIL = 8, 1080, 1920, 200, 30
ZONES = [("entrance", np.array([[200, 300], [900, 250], [1000, 800], [300, 900]], np.int32)),
         ("loading bay", np.array([[1100, 200], [1800, 300], [1700, 1000], [1200, 900], [1400, 600]], np.int32))]
HBM_GBPS = 8000.0            # MI355X peak HBM3E rate: the floor of reading the 50 MB once


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


def stats(us):
    return {"p50": float(np.median(us)), "min": float(np.min(us))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    base = pkg.synth.structured_frames(N, H, W).astype(np.int16) + rng.integers(-6, 7, (N, H, W, 3), dtype=np.int16)
    frames = np.clip(base, 0, 255).astype(np.uint8)
    dev = pkg._ffi.DeviceBuffer(frames.nbytes)
    dev.upload(frames)
    pkg.FrameRenderer().render_batch(dev, [scene(rng) for _ in range(N)], zones=ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
    drawn = dev.download().reshape(N, H, W, 3)
    host = [drawn[i] for i in range(N)]

    raw = []
    for _ in range(5 + args.iters):
        t0 = time.perf_counter()
        dev.download()
        raw.append((time.perf_counter() - t0) * 1e6)
    res = {"frames": N, "size": f"{W}x{H}", "tracks_per_frame": TRACKS, "zones": len(ZONES), "iters": args.iters,
           "raw_bytes": int(frames.nbytes), "raw_d2h_copy_us": stats(raw[5:]), "hbm_read_floor_us": frames.nbytes / (HBM_GBPS * 1e3)}
    ok = True
    for q in (95, 85):
        enc = pkg.JpegEncoder(q, max_height=H, max_width=W, max_batch=N)
        for _ in range(5):
            out = enc.encode_batch(dev, height=H, width=W)
        wall, kern = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            out = enc.encode_batch(dev, height=H, width=W)
            wall.append((time.perf_counter() - t0) * 1e6)
            kern.append(enc.last_kernel_ms() * 1e3)
        enc.encode_batch(host)
        host_t = []
        for _ in range(max(args.iters // 5, 3)):
            t0 = time.perf_counter()
            enc.encode_batch(host)
            host_t.append((time.perf_counter() - t0) * 1e6)
        exact = out[0] == jpeg_ref.encode(drawn[0], q)
        ok &= exact
        from PIL import Image
        pil = []
        for _ in range(3):
            t0 = time.perf_counter()
            for f in host:
                Image.fromarray(f[..., ::-1]).save(io.BytesIO(), "JPEG", quality=q, subsampling=2, optimize=False, restart_marker_rows=1)
            pil.append((time.perf_counter() - t0) * 1e6)
        nbytes = [len(o) for o in out]
        # the JPEG bytes alone over the link: a device buffer of that size, copied like the raw frames above
        small = pkg._ffi.DeviceBuffer(sum(nbytes))
        cp = []
        for _ in range(5 + args.iters):
            t0 = time.perf_counter()
            small.download()
            cp.append((time.perf_counter() - t0) * 1e6)
        small.free()
        k50 = float(np.median(kern))
        res[f"q{q}"] = {"kernel_us": stats(kern), "device_call_us": stats(wall), "host_call_us": stats(host_t),
                        "jpeg_bytes_per_frame_mean": float(np.mean(nbytes)), "jpeg_bytes_per_frame_max": int(max(nbytes)),
                        "jpeg_bytes_d2h_copy_us": stats(cp[5:]), "pillow_1thread_us_per_batch": stats(pil),
                        "kernel_plus_jpeg_copy_us_p50": k50 + float(np.median(cp[5:])),
                        "kernel_over_hbm_floor": k50 / res["hbm_read_floor_us"], "bit_exact_frame0": bool(exact)}
        enc.close()
    dev.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
