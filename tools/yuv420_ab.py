"""A/B of the 4:2:0 input path against BGR24 on one detector (profiles/yuv420/README.md).

  python tools/yuv420_ab.py --leg host     host-fed detect + track, 8 streams x 4 frames, 1080p page-locked frames: BGR24 vs NV12
  python tools/yuv420_ab.py --leg hbm      HBM-resident 640 x 640 frames, same engine shape: BGR24 vs NV12 (the cost of losing the
                                           fused byte-source front end: NV12 always goes letterbox kernel -> image tensor -> stem)
  python tools/yuv420_ab.py --leg kernel --src 1080x1920    batches of 32 through the plain engine, for
      rocprofv3 --kernel-trace --stats (letterbox_yuv420_kernel vs letterbox_kernel; RTMODT_STEM_FUSE=0 is set so that 640 x 640
      BGR frames take letterbox_kernel too)

One process, one detector (YOLOv8s @ 640, batch 32, the staged engine bench.py runs: two stages for host frames, three for HBM-resident
ones); the two forms alternate per repeat (--reps), each repeat = --warmup untimed + --steps timed steps with --depth batches in flight.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["host", "hbm", "kernel"], required=True)
    ap.add_argument("--src", default="", help="HxW of the source frames (default: 1080x1920 for host / kernel, 640x640 for hbm)")
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--frames-per-stream", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ring", type=int, default=2, help="distinct steps of frames kept (host: page-locked, hbm: device)")
    return ap.parse_args()


def main():
    a = parse()
    if a.leg == "kernel":
        os.environ["RTMODT_STEM_FUSE"] = "0"
    import rtmodt_amd  # noqa: F401
    pkg = sys.modules["rtmodt_amd"]
    from importlib import import_module
    core_cls = import_module(pkg.__name__ + ".tracking.tracker")._ByteTrackCore
    h, w = (int(v) for v in (a.src or ("640x640" if a.leg == "hbm" else "1080x1920")).split("x"))
    S, F = a.streams, a.frames_per_stream
    B = S * F
    size = 640
    wpath = os.path.join(tempfile.gettempdir(), f"rtmodt_yuv_ab_yolov8s_{size}.rtw")
    pkg.weights.save(wpath, pkg.weights.synthetic("s", input_size=size), "s")
    if "RTMODT_TUNE_CACHE" not in os.environ:             # the bench's seeded tile choices: the same launches as bench.py
        os.environ["RTMODT_TUNE_CACHE"] = os.path.join(tempfile.gettempdir(), f"rtmodt_yuv_ab_tune_{os.getpid()}.txt")
        shutil.copy(os.path.join(ROOT, "profiles", "bench_tune_cache.txt"), os.environ["RTMODT_TUNE_CACHE"])
    stages = 2 if a.leg == "host" else 3
    chains = 1 if a.leg == "kernel" else 1 - stages
    # (the kernel leg runs eagerly: no captured graph replayed hundreds of times under the kernel tracer)
    det = pkg.Detector(wpath, input_size=(size, size), batch=B, warmup=False, chains=chains, autotune=a.leg != "kernel",
                       use_graph=a.leg != "kernel", max_source_size=(max(w, size), max(h, size)))
    trk = core_cls(n_streams=S, max_dets=128, max_tracks=2048)

    # frames: 8 distinct noise frames (as bench.py feeds), tiled over the ring; NV12 = the same frames converted
    base = pkg.synth.frames(8, h, w, seed=1234)
    nv = pkg.synth.bgr_to_yuv420(base, "nv12")
    R = a.ring
    forms = {}
    for name, src in (("bgr24", base), ("nv12", nv)):
        if a.leg == "host":
            ring = pkg.pipeline.PinnedFrameRing(R * B, h, w, pixel_format=name)
            for k in range(R * B):
                ring.write(k, src[k % 8])
            steps = [[ring.frame(r * B + i) for i in range(B)] for r in range(R)]
            forms[name] = (ring, steps, src[0].nbytes)
        else:
            per = src[0].nbytes
            buf = pkg._ffi.DeviceBuffer(R * B * per)
            for k in range(R * B):
                buf.upload(src[k % 8], offset=k * per)
            steps = [[buf.ptr + (r * B + i) * per for i in range(B)] for r in range(R)]
            forms[name] = (buf, steps, per)

    depth = (det.model.stages + 1) if det.model.stages > 1 else 2

    def run(name, n_steps):
        _, steps, _ = forms[name]
        kw = {} if a.leg == "host" else dict(height=h, width=w)
        t = 0
        for _ in range(depth - 1):
            det.enqueue(steps[t % R], pixel_format=name, **kw); trk.update_from_detector(det, 0, S, frames_per_stream=F); t += 1
        det.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            det.enqueue(steps[t % R], pixel_format=name, **kw); trk.update_from_detector(det, 0, S, frames_per_stream=F); t += 1
            det.fetch()
        dt = time.perf_counter() - t0
        for _ in range(depth - 1):
            det.fetch()
        det.synchronize()
        return n_steps * B / dt

    out = {"leg": a.leg, "src": f"{h}x{w}", "batch": B, "streams": S, "frames_per_stream": F, "engine_stages": det.model.stages,
           "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "frames_s": {"bgr24": [], "nv12": []},
           "bytes_per_frame": {k: int(v[2]) for k, v in forms.items()}}
    for rep in range(a.reps):
        for name in (("bgr24", "nv12") if rep % 2 == 0 else ("nv12", "bgr24")):
            run(name, a.warmup)
            out["frames_s"][name].append(round(run(name, a.steps), 1))
    for name, v in out["frames_s"].items():
        out[f"{name}_median"] = float(np.median(v))
        out[f"{name}_spread_pct"] = round(100 * (max(v) - min(v)) / np.median(v), 2)
    out["nv12_over_bgr24"] = round(out["nv12_median"] / out["bgr24_median"], 4)
    if a.leg == "host":
        out["h2d_GB_s"] = {k: round(out[f"{k}_median"] * forms[k][2] / 1e9, 2) for k in forms}
    print(json.dumps(out), flush=True)
    for v in forms.values():
        v[0].free() if hasattr(v[0], "free") else v[0].close()
    det.close()


if __name__ == "__main__":
    main()
