"""Times the colour attributes (csrc/colour.hip: cl_sample + cl_merge) on 8 x 1080p device frames with 200 tracks per stream,
straight on the device-resident state of one ByteTrack handle, beside the snapshot gallery's process_tracker on the same state and
render_batch's kernel on the same frames in the same run.  Nothing is asserted: the numbers are reported, not gated.

  default            inset 200, rows 150 / 500 / 900, max_side 48, occluders skipped;
  skip_occluded = 0  the same without the occluder sweep;
  max_side 16 / 96   a coarser and a finer grid.

Device times are HIP events around the two launches (rtmodt_colour_last_ms), medians after a warm-up; the raw series are kept in the
JSON.  The floor is 3 bytes per sample taken over the measured copy bandwidth of the chip.  Writes colour_time<tag>.json (and, without a
tag, README.md) into --out-dir and prints the JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from importlib import import_module
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import render_time  # noqa: E402

S, H, W, N_TRACKS, THUMB = 8, 1080, 1920, 200, (96, 96)
HBM_COPY_BYTES_PER_S = 6.29e12            # measured float4 copy on the MI355X (8.0e12 on the datasheet)

README = """# Colour attributes: device time of a call

`tools/colour_time.py`, {S} x {W}x{H} BGR24 device frames, {n} tracks per stream on one ByteTrack handle (boxes of {bw}x{bh} px on a
grid, drifting, neighbours overlapping).  HIP events around the two launches of a call (`cl_sample`, `cl_merge`), medians of {repeat}
calls after {warmup} warm-up calls, outputs fetched (the device time is the launches, not the copy of the results).  The snapshot
gallery's `process_tracker` on the same tracker state and `render_batch`'s kernel on the same frames are timed the same way in the
same run.  Two runs of the tool: `colour_time.json` (the table) and `colour_time_run1.json`; raw series in both (`*_ms_raw`).

| configuration | samples taken per call | device time | run 1 | / render kernel | / floor |
|---|---|---|---|---|---|
{rows}

Beside them, in the same run:

| | device time |
|---|---|
| `SnapshotGallery.process_tracker`, first call (every track takes its shot) | {snap_first_ms:.3f} ms |
| `SnapshotGallery.process_tracker`, every thumbnail kept | {snap_kept_ms:.3f} ms |
| `render_batch`'s kernel ({n} tracks per frame, trails and zones as `tools/render_time.py`) | {render_ms:.3f} ms |

The floor -- 3 bytes per sample taken, read once, at the {bw_tb:.2f} TB/s a float4 copy reaches on this chip -- is {floor_us:.3f} us for
the default configuration: a call is far from it.  It reads three single bytes per sample from rows {sy} lines apart, one workgroup per
track, and a {n}-track stream launches {mc} workgroups of which {idle} leave at once.  Reported as measured, not tuned.

Not profiled: no kernel trace and no counters were collected (the split between the two kernels, the share of the occluder sweep,
LDS atomic conflicts of the per-wave counters, occupancy), no host-side cost of the call or of the result copy
({block_kb:.0f} kB per stream), host frames, the other three trackers, and no real footage -- the overlap of the boxes is the tool's own
choice.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--tag", default="", help="suffix of the JSON file of a further run (no README is written)")
    a = ap.parse_args()
    import rtmodt_amd as pkg
    F = pkg._ffi
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8)
    dev = F.DeviceBuffer(frames.nbytes)
    dev.upload(frames)
    new_core = lambda: import_module(pkg.__name__ + ".tracking.tracker")._ByteTrackCore(n_streams=S, max_tracks=256, max_dets=256)
    bw, bh = 100, 220                                     # on a 90 x 100 grid: every box overlaps its neighbours
    base = np.asarray([[(k % 20) * 90 + 10, (k // 20) * 80 + 10] for k in range(N_TRACKS)], np.float32)
    cls = np.zeros((S, 256), np.int32)
    cnt = np.full(S, N_TRACKS, np.int32)
    fid = [0]

    def update(bt, t):
        phase = t % 60
        dx = 2 * (phase if phase < 30 else 60 - phase)
        xy = np.zeros((S, 256, 4), np.float32)
        conf = np.zeros((S, 256), np.float32)
        for s in range(S):
            xy[s, :N_TRACKS, 0] = base[:, 0] + dx + s; xy[s, :N_TRACKS, 1] = base[:, 1]
            xy[s, :N_TRACKS, 2] = xy[s, :N_TRACKS, 0] + bw; xy[s, :N_TRACKS, 3] = xy[s, :N_TRACKS, 1] + bh
            conf[s, :N_TRACKS] = 0.6
        bt.update_batch(xy, conf, cls, cnt)

    def call(obj, bt):
        fid[0] += 1
        obj.process_tracker(SimpleNamespace(_core=bt, report="matched"), dev, fid[0], height=H, width=W)
        return obj.last_kernel_ms()

    res = {"tool": "tools/colour_time.py", "streams": S, "size": f"{W}x{H}", "tracks_per_stream": N_TRACKS, "box": [bw, bh], "warmup": a.warmup, "repeat": a.repeat}
    configs = [("default", {}), ("skip_occluded_0", {"skip_occluded": 0}), ("max_side_16", {"max_side": 16}), ("max_side_96", {"max_side": 96})]
    for name, kw in configs:
        bt = new_core()
        ca = pkg.ColourAttributes(n_streams=S, max_tracks=256, **kw)
        ms, samples = [], []
        for t in range(a.warmup + a.repeat):
            update(bt, t)
            v = call(ca, bt)
            if t >= a.warmup:
                ms.append(v)
                samples.append(int(ca.updated["frame_samples"].sum()))
        res[name + "_ms_raw"] = ms
        res[name + "_ms"] = float(np.median(ms))
        res[name + "_samples"] = float(np.mean(samples))
        res[name + "_members"] = int(len(ca.updated))
        res[name + "_floor_us"] = 3.0 * res[name + "_samples"] / HBM_COPY_BYTES_PER_S * 1e6
        if name == "default":
            plan = F.ColourPlan()
            import ctypes as C
            box = np.float32([10, 10, 10 + bw, 10 + bh])
            F.check(F.lib().rtmodt_colour_plan(C.byref(ca.cfg), F.ptr(box), H, W, C.byref(plan)))
            res["default_stride"] = [plan.sx, plan.sy]
            res["block_bytes_per_stream"] = int(16 + 208 * 3 * ca.max_tracks)
        ca.close(); bt.close()
    # ---- the snapshot gallery on the same state: its first call, then calls in which every thumbnail is kept ----
    bt = new_core()
    g = pkg.visualization.SnapshotGallery(THUMB, n_streams=S, max_tracks=256, max_updated=256, max_retired=512, retire_after=30)
    update(bt, 0)
    first = []
    for _ in range(8):
        g.reset()
        first.append(call(g, bt))
    kept = []
    for t in range(1, a.warmup + 30):
        update(bt, t)
        v = call(g, bt)
        if t > a.warmup:
            kept.append(v)
    res["snapshot_first_ms"], res["snapshot_kept_ms"] = float(np.median(first[2:])), float(np.median(kept))
    res["snapshot_kept_rewritten"] = int(g.n_rewritten)
    g.close(); bt.close()
    # ---- the render kernel on the same frames ----
    lists = [render_time.scene(rng) for _ in range(S)]
    r = pkg.FrameRenderer()
    rk = []
    for i in range(a.warmup + 20):
        r.render_batch(dev, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if i >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    for name, _ in configs:
        res[name + "_over_render"] = res[name + "_ms"] / res["render_kernel_ms"]
        res[name + "_over_floor"] = res[name + "_ms"] * 1e3 / max(res[name + "_floor_us"], 1e-9)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_raw")}))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"colour_time{a.tag}.json"), "w") as f:
            json.dump(res, f, indent=1)
        if not a.tag:
            run1 = {}
            p1 = os.path.join(a.out_dir, "colour_time_run1.json")
            if os.path.exists(p1):
                run1 = json.load(open(p1))
            label = {"default": "default", "skip_occluded_0": "`skip_occluded = 0`", "max_side_16": "`max_side = 16`", "max_side_96": "`max_side = 96`"}
            rows = "\n".join(f"| {label[k]} | {res[k + '_samples']:.0f} | {res[k + '_ms']:.3f} ms | " + (f"{run1[k + '_ms']:.3f} ms" if k + "_ms" in run1 else "-") +
                             f" | {res[k + '_over_render']:.2f} x | {res[k + '_over_floor']:.0f} x |" for k, _ in configs)
            with open(os.path.join(a.out_dir, "README.md"), "w") as f:
                f.write(README.format(S=S, W=W, H=H, n=N_TRACKS, bw=bw, bh=bh, repeat=a.repeat, warmup=a.warmup, rows=rows, snap_first_ms=res["snapshot_first_ms"],
                                      snap_kept_ms=res["snapshot_kept_ms"], render_ms=res["render_kernel_ms"], bw_tb=HBM_COPY_BYTES_PER_S / 1e12,
                                      floor_us=res["default_floor_us"], sy=res["default_stride"][1], mc=256, idle=256 - N_TRACKS,
                                      block_kb=res["block_bytes_per_stream"] / 1e3))
    r.close(); dev.free()


if __name__ == "__main__":
    main()
