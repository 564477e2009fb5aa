"""Times MotionDetector.process (csrc/motion.hip) on 8 x 1080p BGR24 frames in device memory -- the frames tools/render_time.py times
the renderer on -- at scale 1, 2 and 4: a still scene (the same frames call after call) and a busy scene (200 filled boxes per
stream, render_time.py's boxes, that move from call to call), beside each call's floor -- the bytes it must move, each once, at the
best copy rate of profiles/r01/bandwidth_probe.txt -- and, in the same run, render_batch's kernel time on the same frames and the
device time of one detector pass (synthetic YOLOv8n at 640) over the same 8 frames: the pass a still frame saves.  Device times are
HIP-event times around the launches of one call (rtmodt_motion_last_ms), medians after a warm-up.  Writes motion_time.json and
README.md into --out-dir and prints the JSON line.

    python tools/motion_time.py [--iters 30] [--out-dir profiles/motion]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import rtmodt_amd  # noqa: E402,F401
import motion_ref  # noqa: E402
import render_time  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
SCALES = (1, 2, 4)
VARIANTS = 4                    # frame sets the busy scene cycles through

README = """# Motion detection: timings (`tools/motion_time.py`)

What is measured: one `MotionDetector.process` call on {n} streams of 1080p, BGR24 frames already in device memory ({frames_mb:.1f} MB:
the frames `tools/render_time.py` times the renderer on), at scale 1 ({cells1:.2f} M cells per stream), 2 ({cells2:.2f} M) and 4
({cells4:.2f} M), with the default configuration.  Still scene: the same frames call after call, so nothing is foreground.  Busy scene:
{tracks} filled boxes per stream (`render_time.py`'s boxes) that move by 8 pixels from call to call, {variants} frame sets in rotation.
Everything below comes from ONE process on one MI355X.

How: device times are HIP-event times around the memset and the seven launches of one call (`rtmodt_motion_last_ms`), medians of
{iters} calls after {warmup} warm-up calls (and after the model's own warm-up frames).  `render_batch`'s kernel time is its own
HIP-event time on the same frames, and the detector pass is the sum of the engine's HIP-event stage times (letterbox, forward, NMS) of
one batch of the same {n} frames through a synthetic YOLOv8n at 640, both in the same run.  No profiler was attached, nothing was
fixed in advance and nothing is gated on these numbers.

    python tools/motion_time.py --out-dir profiles/motion

## Figures (`motion_time.json`)

| scene | scale 1 | floor | x floor | scale 2 | floor | x floor | scale 4 | floor | x floor |
|---|---|---|---|---|---|---|---|---|---|
{rows}

A floor is the bytes the call must move, each once, at the {hbm:.2f} TB/s of the best `copy` line of
`profiles/r01/bandwidth_probe.txt` ({probe_line}): {frames_mb:.1f} MB of pixels plus 4 B read and 4 B written per cell.  It leaves out
what the call moves besides: the raw and mask bytes (1 B per cell written, read back by the next kernels) and, for mask cells, the
union-find arrays (24 B per mask cell).

`render_batch`'s kernel on the same frames: {render_ms:.3f} ms.  One detector pass over the same {n} frames: {det_ms:.3f} ms
(letterbox {pre_ms:.3f} + forward {fwd_ms:.3f} + NMS {nms_ms:.3f}).

{verdict}

## Parity

PINNED, exactly: the kernels against `tests/motion_ref.py` (stream 0's result, mask and model after the first busy call were compared
again in this run at every scale: {exact}).  UNPINNED: parity with OpenCV's `BackgroundSubtractorMOG2` and with Frigate's motion
detector (neither is installed where this runs), and every default: none has been validated on real footage.  NV12 / I420 input,
whose Y plane could be read directly at a third of the bytes, is the obvious next step and is not implemented.
"""


def timed(call, ms_of, warmup, iters):
    ms = []
    for k in range(warmup + iters):
        call(k)
        if k >= warmup:
            ms.append(ms_of())
    return {"ms": float(np.median(ms)), "minmax_ms": [float(min(ms)), float(max(ms))]}


def busy_frames(base, lists, shift):
    """The base frames with every stream's boxes filled white, moved right and down by `shift` pixels."""
    out = base.copy()
    for s, tracks in enumerate(lists):
        for t in tracks:
            x0, y0, x1, y1 = (int(v) for v in t.xyxy)
            out[s, min(y0 + shift, H - 1):min(y1 + shift, H), min(x0 + shift, W - 1):min(x1 + shift, W)] = 255
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    still = pkg._ffi.DeviceBuffer(frames.nbytes)
    still.upload(frames)
    busy_host = [busy_frames(frames, lists, 8 * v) for v in range(VARIANTS)]
    busy = [pkg._ffi.DeviceBuffer(frames.nbytes) for _ in range(VARIANTS)]
    for b, f in zip(busy, busy_host):
        b.upload(f)
    tbs, probe_line = hbm_rate()
    res = {"tool": "tools/motion_time.py", "streams": N, "size": f"{W}x{H}", "boxes_per_stream": render_time.TRACKS, "variants": VARIANTS,
           "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs, "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "scales": {}}
    exact = True
    for scale in SCALES:
        gh, gw = motion_ref.grid_shape(H, W, scale)
        det = pkg.MotionDetector(N, H, W, scale=scale)
        ref = motion_ref.Ref(1, H, W, scale=scale)
        for _ in range(det._cfg.warmup):
            det.process(still)
        row = {"grid": f"{gw}x{gh}", "cells_per_stream": gh * gw, "floor_bytes": frames.nbytes + 8 * N * gh * gw}
        row["floor_us"] = row["floor_bytes"] / (tbs * 1e12) * 1e6
        row["still"] = timed(lambda k: det.process(still), det.last_kernel_ms, a.warmup, a.iters)
        # the first busy call against the restatement, which starts from the device's own model
        bg, dev, seen = det.state(0)
        ref.load_state(bg, dev, seen)
        got = det.process(busy[0])
        want = ref.step(0, busy_host[0][0])
        g = got[0]
        ok = (g.status, g.n_raw, g.n_fg, g.luma_sum, tuple(g.bbox), list(g.regions), g.n_regions_total, g.frames_seen) == \
            (want["status"], want["n_raw"], want["n_fg"], want["luma_sum"], want["bbox"], want["regions"], want["n_regions_total"], want["frames_seen"])
        ok = ok and bool(np.array_equal(det.mask(0), ref.masks[0])) and bool(np.array_equal(det.state(0)[0], ref.state(0)[0]))
        row["bit_exact"] = bool(ok)
        exact &= bool(ok)
        last = {}

        def busy_call(k):
            last["r"] = det.process(busy[(k + 1) % VARIANTS])
        row["busy"] = timed(busy_call, det.last_kernel_ms, a.warmup, a.iters)
        r = last["r"]
        row["busy_last_call"] = {"statuses": [x.status_name for x in r], "n_fg_share": float(np.mean([x.n_fg for x in r]) / (gh * gw)),
                                 "regions_total": [x.n_regions_total for x in r]}
        for k in ("still", "busy"):
            row[k]["over_floor"] = row[k]["ms"] * 1e3 / row["floor_us"]
        res["scales"][str(scale)] = row
        det.close()
    r = pkg.FrameRenderer()
    rk = []
    for k in range(a.warmup + a.iters):
        r.render_batch(still, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if k >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    still.upload(frames)
    # one detector pass over the same 8 frames
    path = os.path.join(tempfile.mkdtemp(prefix="rtmodt_motion_time_"), "yolov8n_640.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=640), "n")
    d = pkg.Detector(path, input_size=(640, 640), batch=N, max_source_size=(W, H))
    ptrs = [still.ptr + i * H * W * 3 for i in range(N)]
    st = []
    for k in range(a.warmup + a.iters):
        d.enqueue(ptrs, H, W, 3 * W)
        d.fetch()
        if k >= a.warmup:
            st.append(d.stage_times())
    pre, fwd, nms = (float(np.median([s[i] for s in st])) for i in range(3))
    res["detector_pass"] = {"model": "synthetic YOLOv8n @ 640", "frames": N, "preprocess_ms": pre, "forward_ms": fwd, "nms_ms": nms, "ms": pre + fwd + nms}
    d.close()
    res["bit_exact"] = exact
    for b in busy + [still]:
        b.free()

    rows, notes = [], []
    for k, label in (("still", "still scene"), ("busy", f"busy scene, {render_time.TRACKS} moving boxes")):
        cols = []
        for scale in SCALES:
            e, row = res["scales"][str(scale)][k], res["scales"][str(scale)]
            e["over_detector_pass"] = e["ms"] / res["detector_pass"]["ms"]
            cols += [f"{e['ms']:.3f} ms", f"{row['floor_us']:.1f} us", f"{e['over_floor']:.1f} x"]
        rows.append(f"| {label} | " + " | ".join(cols) + " |")
    s4, b4, b1 = res["scales"]["4"]["still"], res["scales"]["4"]["busy"], res["scales"]["1"]["busy"]
    notes.append(f"At the default scale 4 the motion call takes {s4['ms']:.3f} ms on a still scene and {b4['ms']:.3f} ms on the busy one: "
                 f"{100 * s4['over_detector_pass']:.1f} % and {100 * b4['over_detector_pass']:.1f} % of the {res['detector_pass']['ms']:.3f} ms detector pass it can "
                 f"save, and {s4['ms'] / res['render_kernel_ms']:.2f} x / {b4['ms'] / res['render_kernel_ms']:.2f} x the render kernel's time.")
    notes.append(f"The busy scene at scale 1 ({b1['ms']:.3f} ms, {b1['over_floor']:.1f} x its floor) pays for the labelling: "
                 f"{100 * res['scales']['1']['busy_last_call']['n_fg_share']:.0f} % of the cells are in the mask, each is a union-find node, and the area and box "
                 f"of a component are added at its root with integer atomics.")
    notes.append("The call is seven launches and a memset whatever the frames show, so the still scene pays the launches of the labelling kernels, "
                 "whose workgroups find an empty mask and return.  Which kernel bounds each figure was not profiled: no per-kernel trace was taken.")
    notes.append("Reported as measured, not tuned.")
    res["verdict"] = " ".join(notes)
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "motion_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        sc = res["scales"]
        dp = res["detector_pass"]
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=frames.nbytes / 1e6, cells1=sc["1"]["cells_per_stream"] / 1e6, cells2=sc["2"]["cells_per_stream"] / 1e6,
                                  cells4=sc["4"]["cells_per_stream"] / 1e6, tracks=render_time.TRACKS, variants=VARIANTS, iters=a.iters, warmup=a.warmup,
                                  rows="\n".join(rows), hbm=tbs, probe_line=probe_line, render_ms=res["render_kernel_ms"], det_ms=dp["ms"],
                                  pre_ms=dp["preprocess_ms"], fwd_ms=dp["forward_ms"], nms_ms=dp["nms_ms"], verdict=res["verdict"],
                                  exact="equal" if exact else "NOT EQUAL"))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
