"""Times Heatmap (csrc/heatmap.hip) on 8 x 1080p streams, 200 tracks per stream -- the scene tools/render_time.py times the renderer
on -- with the DISC footprint at cell 1 and cell 4: accumulate without decay, accumulate on a decay tick, accumulate with empty
track lists, and the overlay onto BGR24 frames in device memory (scaled to the grid's own maximum: two launches; and to a fixed
scale_max: one), beside render_batch's kernel time on the same frames and each step's floor -- the bytes it must move, once, at the
best copy rate of profiles/r01/bandwidth_probe.txt -- all in one run.  Device times are the handle's HIP-event times around its
launches (rtmodt_heatmap_last_ms), medians after a warm-up.  Writes heatmap_time.json and README.md into --out-dir and prints the
JSON line.

    python tools/heatmap_time.py [--iters 30] [--out-dir profiles/heatmap]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import rtmodt_amd  # noqa: E402,F401
import heatmap_ref  # noqa: E402
import render_time  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
CELLS = (1, 4)
PROBE = os.path.join(ROOT, "profiles", "r01", "bandwidth_probe.txt")

README = """# Occupancy heatmap: timings (`tools/heatmap_time.py`)

What is measured: {n} streams of 1080p, {tracks} track boxes per stream and frame (the scene `tools/render_time.py` times the renderer
on), the DISC footprint, grids of cell 1 ({cells1:.1f} M cells, {grid1:.1f} MB in all) and cell 4 ({cells4:.2f} M cells, {grid4:.1f} MB);
the overlay blends onto {n} BGR24 frames already in device memory ({frames_mb:.1f} MB).  Everything below comes from ONE process on
one MI355X.

How: device times are HIP-event times around the launches of one call (`rtmodt_heatmap_last_ms`), medians of {iters} calls after
{warmup} warm-up calls.  The grid keeps accumulating from call to call (its values do not change the work); the frames are uploaded
afresh before the timed overlay calls.  `render_batch`'s kernel time is its own HIP-event time on the same frames and tracks, in the
same run.  No profiler was attached, nothing was fixed in advance and nothing is gated on these numbers.

    python tools/heatmap_time.py --out-dir profiles/heatmap

## Figures (`heatmap_time.json`)

| step | cell 1 | floor | x floor | cell 4 | floor | x floor |
|---|---|---|---|---|---|---|
{rows}

`render_batch`'s kernel on the same frames: {render_ms:.3f} ms.  A floor is the bytes the step must move, each once, at the
{hbm:.2f} TB/s of the best `copy` line of `profiles/r01/bandwidth_probe.txt` ({probe_line}): accumulate reads and writes the covered
cells (4 + 4 B each; {cov1:.1%} of the cells at cell 1, {cov4:.1%} at cell 4), a decay tick every cell; the empty call moves nothing,
so its time is the cost of the launch and of {tiles1} (cell 1) or {tiles4} (cell 4) workgroups that return at once; the overlay reads
the grid once (twice when it first finds the maximum) and reads and writes the blended pixels (3 + 3 B each, {blend1:.1%} of them at
cell 1 with min_level 1).

{verdict}

## Parity

PINNED, exactly: the kernels against `tests/heatmap_ref.py` (stream 0's grid after the first accumulate call and frame 0 after
one overlay were compared again in this run, at both cell sizes: {exact}).  UNPINNED: parity with Ultralytics' `Heatmap`
solution, with cv2's colormaps (the default jet is closed-form; its parity with `cv2.COLORMAP_JET` is unpinned) and `addWeighted`,
and any default tuned on real footage.
"""


def hbm_rate():
    """(TB/s, the line it came from): the best ``copy`` rate of the bandwidth probe."""
    best = (0.0, "")
    for line in open(PROBE):
        m = re.search(r"copy\s+([0-9.]+) TB/s", line)
        if m and float(m.group(1)) > best[0]:
            best = (float(m.group(1)), " ".join(line.split()[:2]))
    if best[0] <= 0:
        raise RuntimeError(f"no copy rate in {PROBE}")
    return best


def timed(call, ms_of, warmup, iters, before_timed=None):
    ms = []
    for k in range(warmup + iters):
        if k == warmup and before_timed:
            before_timed()
        call()
        if k >= warmup:
            ms.append(ms_of())
    return {"ms": float(np.median(ms)), "minmax_ms": [float(min(ms)), float(max(ms))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    boxes = [(np.stack([t.xyxy for t in l]).astype(np.float32), np.zeros(len(l), np.int32)) for l in lists]
    empty = [np.zeros((0, 4), np.float32)] * N
    dev = pkg._ffi.DeviceBuffer(frames.nbytes)
    tbs, probe_line = hbm_rate()
    res = {"tool": "tools/heatmap_time.py", "streams": N, "size": f"{W}x{H}", "tracks_per_stream": render_time.TRACKS, "footprint": "disc",
           "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs, "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "cells": {}}
    exact = True
    for cell in CELLS:
        gh, gw = heatmap_ref.grid_shape(H, W, cell)
        row = {"grid": f"{gw}x{gh}", "cells_per_stream": gh * gw, "workgroups": N * (-(-gw // 64)) * (-(-gh // 16))}
        hm = pkg.visualization.Heatmap(N, H, W, cell=cell, footprint="disc")
        hm.accumulate(boxes)
        g0 = hm.grid(0)
        ok = bool(np.array_equal(g0, heatmap_ref.stamp(np.zeros((gh, gw), np.uint32), heatmap_ref.counts(*boxes[0], H, W, cell, kind=heatmap_ref.DISC))))
        covered = sum(int(np.count_nonzero(hm.grid(s))) for s in range(N))
        row["covered_cells"] = covered
        row["covered_share"] = covered / (N * gh * gw)
        row["accumulate"] = timed(lambda: hm.accumulate(boxes), hm.last_kernel_ms, a.warmup, a.iters)
        row["accumulate"]["floor_bytes"] = 8 * covered
        row["accumulate_empty"] = timed(lambda: hm.accumulate(empty), hm.last_kernel_ms, a.warmup, a.iters)
        row["accumulate_empty"]["floor_bytes"] = 0
        # the overlay, on the grid as the calls above left it
        grid0 = hm.grid(0)
        m = int(grid0.max())
        blended = 0
        for s in range(N):
            g = hm.grid(s)
            lv = heatmap_ref.levels(g, int(g.max())) >= 1
            blended += int(np.repeat(np.repeat(lv, cell, 0), cell, 1)[:H, :W].sum())
        row["blended_pixels"] = blended
        row["blended_share"] = blended / (N * H * W)
        dev.upload(frames)
        hm.overlay(dev)
        ok &= bool(np.array_equal(dev.download(H * W * 3).reshape(H, W, 3), heatmap_ref.overlay(frames[0], grid0, cell)))
        row["overlay"] = timed(lambda: hm.overlay(dev), hm.last_kernel_ms, a.warmup, a.iters, lambda: dev.upload(frames))
        row["overlay"]["floor_bytes"] = 6 * blended + 2 * 4 * N * gh * gw
        row["overlay_fixed_scale"] = timed(lambda: hm.overlay(dev, scale_max=m), hm.last_kernel_ms, a.warmup, a.iters, lambda: dev.upload(frames))
        row["overlay_fixed_scale"]["floor_bytes"] = 6 * blended + 4 * N * gh * gw
        hm.close()
        dec = pkg.visualization.Heatmap(N, H, W, cell=cell, footprint="disc", decay_shift=4, decay_every=1)
        row["accumulate_decay_tick"] = timed(lambda: dec.accumulate(boxes), dec.last_kernel_ms, a.warmup, a.iters)
        row["accumulate_decay_tick"]["floor_bytes"] = 8 * N * gh * gw
        dec.close()
        row["bit_exact"] = ok
        exact &= ok
        for k in ("accumulate", "accumulate_decay_tick", "accumulate_empty", "overlay", "overlay_fixed_scale"):
            fl = row[k]["floor_bytes"] / (tbs * 1e12) * 1e6
            row[k]["floor_us"] = fl
            row[k]["over_floor"] = row[k]["ms"] * 1e3 / fl if fl > 0 else None
        res["cells"][str(cell)] = row
    r = pkg.FrameRenderer()
    dev.upload(frames)
    rk = []
    for k in range(a.warmup + a.iters):
        r.render_batch(dev, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if k >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    res["bit_exact"] = exact
    dev.free()
    names = [("accumulate", "accumulate, no decay"), ("accumulate_decay_tick", "accumulate, decay tick"), ("accumulate_empty", "accumulate, empty lists"),
             ("overlay", "overlay, own maximum"), ("overlay_fixed_scale", "overlay, fixed scale_max")]
    rows, notes = [], []
    for k, label in names:
        cols = []
        for cell in CELLS:
            e = res["cells"][str(cell)][k]
            e["over_render_kernel"] = e["ms"] / res["render_kernel_ms"]
            cols += [f"{e['ms']:.3f} ms", f"{e['floor_us']:.1f} us" if e["floor_us"] else "launch only", f"{e['over_floor']:.1f} x" if e["over_floor"] else "-"]
            if e["over_render_kernel"] > 2.0:
                notes.append(f"{label} at cell {cell} takes {e['over_render_kernel']:.1f} x the render kernel's time.")
        rows.append(f"| {label} | " + " | ".join(cols) + " |")
    e1, e4 = res["cells"]["1"]["accumulate_empty"]["ms"], res["cells"]["4"]["accumulate_empty"]["ms"]
    notes.append(f"The empty call takes {e1 * 1e3:.1f} us at cell 1 and {e4 * 1e3:.1f} us at cell 4: no tile touches the grid, and what remains is "
                 f"the launch and the dispatch of {res['cells']['1']['workgroups']} and {res['cells']['4']['workgroups']} workgroups.")
    notes.append(f"Accumulate sits well above its byte floor ({res['cells']['1']['accumulate']['over_floor']:.0f} x at cell 1, "
                 f"{res['cells']['4']['accumulate']['over_floor']:.0f} x at cell 4): the floor counts bytes only, while every workgroup walks its stream's "
                 f"{render_time.TRACKS} stamps through the LDS cull and tests its candidate cells in int64; at cell 4 the whole call is "
                 f"{res['cells']['4']['workgroups']} workgroups, about four per CU.  Which of these bounds the time was not profiled.")
    notes.append("Reported as measured, not tuned.")
    res["verdict"] = " ".join(notes)
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "heatmap_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        c1, c4 = res["cells"]["1"], res["cells"]["4"]
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, tracks=render_time.TRACKS, cells1=c1["cells_per_stream"] / 1e6, grid1=4 * N * c1["cells_per_stream"] / 1e6,
                                  cells4=c4["cells_per_stream"] / 1e6, grid4=4 * N * c4["cells_per_stream"] / 1e6, frames_mb=frames.nbytes / 1e6,
                                  iters=a.iters, warmup=a.warmup, rows="\n".join(rows), render_ms=res["render_kernel_ms"], hbm=tbs,
                                  probe_line=probe_line, cov1=c1["covered_share"], cov4=c4["covered_share"], tiles1=c1["workgroups"],
                                  tiles4=c4["workgroups"], blend1=c1["blended_share"], verdict=res["verdict"], exact="equal" if exact else "NOT EQUAL"))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
