"""Times LeftObjectDetector.process (csrc/leftobj.hip) on 8 x 1080p BGR24 frames in device memory -- the frames tools/motion_time.py
times the motion detector on -- with 200 tracks per stream read from one ByteTrack handle's device-resident state, at scale 4, 2 and
1: a still scene (the same frames call after call: no static cell) and a scene with 20 left objects per stream (static blocks the
ledger follows), beside each call's byte floor.  Yardsticks from the same run: MotionDetector.process on the same frames at the same
scale (its model kernel reads the same pixels with the same mapping) and render_batch's kernel.  Device times are HIP-event times
around the launches of one call (rtmodt_leftobj_last_ms / rtmodt_motion_last_ms), medians after a warm-up.

Every GPU step (one per scale, one for the renderer) runs in a child process of its own under its own time limit; the first step
that fails or runs out of time ends the run.  Writes leftobj_time.json and README.md into --out-dir (a leftobj_time_run1.json found
there is quoted as the earlier run) and prints the JSON line.

    python tools/leftobj_time.py [--iters 30] [--out-dir profiles/leftobj]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

N, H, W, TRACKS, OBJECTS, BLOCK = 8, 1080, 1920, 200, 20, 64
SCALES = (4, 2, 1)
STEP_SECONDS = 240
CFG = dict(static_frames=5, alarm_frames=1000, max_objects=64, max_regions=64)      # the defaults but for a short wait for static

README = """# Left / removed objects: timings (`tools/leftobj_time.py`)

What is measured: one `LeftObjectDetector.process` call on {n} streams of 1080p, BGR24 frames already in device memory
({frames_mb:.1f} MB), with {tracks} tracks per stream read from one ByteTrack handle's device-resident state, at scale 4, 2 and 1.
The configuration is the default but for `static_frames` {static_frames} (so that the tool need not run 100 frames before anything
is static), `alarm_frames` {alarm_frames}, `max_objects` and `max_regions` {max_objects}.  Still scene: the same frames call after
call, so no cell is foreground and none static.  Left objects: {objects} blocks of {block} x {block} pixels per stream, static, each
followed by a ledger entry.  Every GPU step ran in a process of its own under a {step_s} s limit, all on one MI355X, one after the
other.

How: device times are HIP-event times around the memset and the nine launches of one call (`rtmodt_leftobj_last_ms`), medians of
{iters} calls after {warmup} warm-up calls; every timed call returns its outputs (one copy), as the motion detector's does.  The
yardsticks come from the same processes: `MotionDetector.process` (default configuration, seven launches) on the same frames at the
same scale -- its model kernel reads the same pixels with the same thread-to-run mapping -- and `render_batch`'s kernel.  No profiler was attached, nothing was fixed in advance and nothing is gated on
these numbers.

    python tools/leftobj_time.py --out-dir profiles/leftobj

## Figures (`leftobj_time.json`)

| scale | cells / stream | floor | still | x floor | x motion still | 20 left objects | x floor | motion still | motion on the objects |
|---|---|---|---|---|---|---|---|---|---|
{rows}

A floor is the bytes the call must move, each once, at the {hbm:.2f} TB/s of the best `copy` line of
`profiles/r01/bandwidth_probe.txt` ({probe_line}): {frames_mb:.1f} MB of pixels, 8 B read and 8 B written per cell, 1 B of luma per
cell.  It leaves out the second read of the cells by the filter, the mask, and for mask cells the union-find parent and the 48 B of
accumulators at a root.

`render_batch`'s kernel on the same frames: {render_ms:.3f} ms.

{verdict}

The detector reads the frame itself; a pipeline that also runs `MotionDetector` pays for the pixels twice (the `motion still` column
is that second pass).  Sharing one pixel pass is out of scope here.

## Spread

{spread}

## Parity

PINNED, exactly: the kernels against `tests/leftobj_ref.py` (tests/test_gpu_leftobj.py).  UNPINNED: parity with any vendor's
left-object rule, and every default: none has been validated on real footage.  Deliberate limits: a fixed camera (no camera-motion
compensation), one luma channel.
"""


def timed(call, ms_of, warmup, iters):
    ms = []
    for k in range(warmup + iters):
        call()
        if k >= warmup:
            ms.append(ms_of())
    return {"ms": float(np.median(ms)), "minmax_ms": [float(min(ms)), float(max(ms))]}


def scenes():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    left = frames.copy()
    for s in range(N):
        for k in range(OBJECTS):                                     # a 5 x 4 raster of blocks, well apart
            x0, y0 = 100 + (k % 5) * 360 + 8 * s, 90 + (k // 5) * 250
            left[s, y0:y0 + BLOCK, x0:x0 + BLOCK] = 255
    boxes = np.zeros((N, 256, 4), np.float32)
    for s in range(N):
        x1, y1 = rng.uniform(0, W - 120, TRACKS), rng.uniform(0, H - 200, TRACKS)
        boxes[s, :TRACKS] = np.stack([x1, y1, x1 + rng.uniform(40, 120, TRACKS), y1 + rng.uniform(80, 200, TRACKS)], 1)
    return frames, left, boxes


def step_scale(scale, iters, warmup):
    import rtmodt_amd  # noqa: F401
    pkg = sys.modules["rtmodt_amd"]
    frames, left, boxes = scenes()
    still, objs = pkg._ffi.DeviceBuffer(frames.nbytes), pkg._ffi.DeviceBuffer(frames.nbytes)
    still.upload(frames); objs.upload(left)
    core = pkg.tracking.tracker._ByteTrackCore(0.5, 30, 0.8, n_streams=N, max_tracks=256, max_dets=256)
    conf, cls, cnt = np.full((N, 256), 0.9, np.float32), np.zeros((N, 256), np.int32), np.full(N, TRACKS, np.int32)
    cls[:, ::3] = 2
    for _ in range(2):
        core.update_batch(boxes, conf, cls, cnt)
    n_sel = [int((core.snapshot(s)["tsu"] == 1).sum()) for s in range(N)]
    from types import SimpleNamespace
    tracker = SimpleNamespace(_core=core, report="matched")
    gh, gw = -(-H // scale), -(-W // scale)
    row = {"grid": f"{gw}x{gh}", "cells_per_stream": gh * gw, "floor_bytes": int(frames.nbytes + 17 * N * gh * gw), "tracks_selected": n_sel}
    det = pkg.LeftObjectDetector(N, H, W, scale=scale, **CFG)
    for _ in range(det._cfg.warmup + 1):
        det.process(still, tracker=tracker, outputs=False)
    row["still"] = timed(lambda: det.process(still, tracker=tracker), det.last_kernel_ms, warmup, iters)      # with its outputs, as motion below
    r = det.process(still, tracker=tracker)
    row["still_last_call"] = {"statuses": [x.status_name for x in r], "n_fg": [x.n_fg for x in r], "n_static": [x.n_static for x in r]}
    for _ in range(CFG["static_frames"] + 2):
        det.process(objs, tracker=tracker, outputs=False)
    row["objects"] = timed(lambda: det.process(objs, tracker=tracker), det.last_kernel_ms, warmup, iters)
    r = det.process(objs, tracker=tracker)
    row["objects_last_call"] = {"statuses": [x.status_name for x in r], "n_static": [x.n_static for x in r], "n_regions_total": [x.n_regions_total for x in r],
                                "n_objects": [x.n_objects for x in r]}
    det.close()
    mo = pkg.MotionDetector(N, H, W, scale=scale)
    for _ in range(mo._cfg.warmup + 1):
        mo.process(still)
    row["motion_still"] = timed(lambda: mo.process(still), mo.last_kernel_ms, warmup, iters)
    row["motion_objects"] = timed(lambda: mo.process(objs), mo.last_kernel_ms, warmup, iters)     # (the blocks fade into its background)
    mo.close(); core.close(); still.free(); objs.free()
    return row


def step_render(iters, warmup):
    import rtmodt_amd  # noqa: F401
    import render_time
    pkg = sys.modules["rtmodt_amd"]
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    buf = pkg._ffi.DeviceBuffer(frames.nbytes)
    buf.upload(frames)
    r = pkg.FrameRenderer()
    out = timed(lambda: r.render_batch(buf, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W), r.last_kernel_ms, warmup, iters)
    buf.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        res = step_render(a.iters, a.warmup) if a.step == "render" else step_scale(int(a.step), a.iters, a.warmup)
        print("STEP " + json.dumps(res))
        return 0
    from heatmap_time import hbm_rate
    tbs, probe_line = hbm_rate()
    res = {"tool": "tools/leftobj_time.py", "streams": N, "size": f"{W}x{H}", "tracks_per_stream": TRACKS, "objects_per_stream": OBJECTS, "cfg": CFG,
           "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs, "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "scales": {}}
    for step in [str(s) for s in SCALES] + ["render"]:
        # one GPU step: a fresh child under its own time limit; a failure or a timeout ends the run (nothing more is started)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            sys.stderr.write(f"step {step} ran past {STEP_SECONDS} s\n")
            return 1
        lines = [l for l in p.stdout.splitlines() if l.startswith("STEP ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            return 1
        out = json.loads(lines[-1][5:])
        if step == "render":
            res["render_kernel_ms"] = out["ms"]
        else:
            out["floor_us"] = out["floor_bytes"] / (tbs * 1e12) * 1e6
            for k in ("still", "objects"):
                out[k]["over_floor"] = out[k]["ms"] * 1e3 / out["floor_us"]
            out["still"]["over_motion_still"] = out["still"]["ms"] / out["motion_still"]["ms"]
            res["scales"][step] = out
    rows = []
    for s in SCALES:
        r = res["scales"][str(s)]
        rows.append(f"| {s} | {r['cells_per_stream']} | {r['floor_us']:.1f} us | {r['still']['ms']:.3f} ms | {r['still']['over_floor']:.1f} x | "
                    f"{r['still']['over_motion_still']:.2f} x | {r['objects']['ms']:.3f} ms | {r['objects']['over_floor']:.1f} x | {r['motion_still']['ms']:.3f} ms | "
                    f"{r['motion_objects']['ms']:.3f} ms |")
    worst = max(res["scales"][str(s)]["still"]["over_motion_still"] for s in SCALES)
    d = res["scales"]["4"]
    notes = [f"At the default scale 4 a call takes {d['still']['ms']:.3f} ms on the still scene ({d['still']['over_motion_still']:.2f} x the motion detector's "
             f"{d['motion_still']['ms']:.3f} ms on the same frames) and {d['objects']['ms']:.3f} ms with {OBJECTS} left objects per stream; "
             f"{d['still']['ms'] / res['render_kernel_ms']:.2f} x / {d['objects']['ms'] / res['render_kernel_ms']:.2f} x the render kernel's time.",
             f"The largest still ratio over the three scales is {worst:.2f} x motion's still figure."]
    if worst > 1.5:
        notes.append("That is above 1.5 x.  Which launch carries it is not known from this run: no kernel trace is taken here.  Take one in a run of its "
                     "own, with no counters: `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/leftobj_time.py --step <scale>`, and read the "
                     "`leftobj_*` rows beside the `motion_*` rows of the same process.")
    elif worst < 1.0:
        notes.append("The still call is below the motion detector's at every scale although it moves more bytes per cell.  Why was not profiled: no "
                     "kernel trace was taken, so the split between the kernels of either call is not known.")
    else:
        notes.append("The still call lies between 1 x and 1.5 x the motion detector's; no kernel trace was taken.")
    notes += ["The call is nine launches and a memset whatever the frames show; on the still scene the labelling, ledger and absorb kernels find an empty "
              "mask and return.", "Reported as measured, not tuned."]
    res["verdict"] = " ".join(notes)
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        prev_path = os.path.join(a.out_dir, "leftobj_time_run1.json")
        spread = "Only one run was made."
        if os.path.exists(prev_path):
            prev = json.load(open(prev_path))
            parts = []
            for s in SCALES:
                p_, c_ = prev["scales"][str(s)], res["scales"][str(s)]
                parts.append(f"scale {s}: still {p_['still']['ms']:.3f} ms, objects {p_['objects']['ms']:.3f} ms, motion still {p_['motion_still']['ms']:.3f} ms "
                             f"(this run: {c_['still']['ms']:.3f} / {c_['objects']['ms']:.3f} / {c_['motion_still']['ms']:.3f})")
            spread = ("The same command was run twice on this code, one run after the other; the figures above are the second run, "
                      "`leftobj_time_run1.json` the first: " + "; ".join(parts) + f"; render kernel {prev['render_kernel_ms']:.3f} ms "
                      f"(this run {res['render_kernel_ms']:.3f}).  Within a run the extremes of each figure are in `minmax_ms`.")
        with open(os.path.join(a.out_dir, "leftobj_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=N * H * W * 3 / 1e6, tracks=TRACKS, objects=OBJECTS, block=BLOCK, step_s=STEP_SECONDS, iters=a.iters,
                                  warmup=a.warmup, rows="\n".join(rows), hbm=tbs, probe_line=probe_line, render_ms=res["render_kernel_ms"],
                                  verdict=res["verdict"], spread=spread, **{k: CFG[k] for k in ("static_frames", "alarm_frames", "max_objects")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
