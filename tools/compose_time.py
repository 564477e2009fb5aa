"""Times Compositor.run (csrc/compose.hip) on 1080p BGR24 frames in device memory -- the frames tools/render_time.py times the
renderer on -- into the compositor's own device buffers: 8 frames into a 2 x 4 wall of 1920 x 1080 (BGR24 and NV12), the same 8
frames into 8 sub-streams of 640 x 360, and one frame shown whole with a 2 x inset on top; beside each call's floor -- the bytes of
the cells' crops and of the outputs, each moved once, at the best copy rate of profiles/r01/bandwidth_probe.txt -- and, in the same
run, render_batch's kernel time on the same frames.  Device times are HIP-event times around the one launch of a run
(rtmodt_compose_last_ms), medians after a warm-up.  Writes compose_time.json and README.md into --out-dir and prints the JSON line.
--first-run: the JSON of an earlier run of the same command, quoted in the README's spread.

    python tools/compose_time.py [--iters 200] [--out-dir profiles/compose] [--first-run first.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import rtmodt_amd  # noqa: E402,F401
import compose_ref  # noqa: E402
import render_time  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W

README = """# Compositor: timings (`tools/compose_time.py`)

What is measured: one `Compositor.run` call on 1080p BGR24 frames already in device memory (the frames `tools/render_time.py` times
the renderer on), into the compositor's own device buffers:

- `wall_bgr24` / `wall_nv12`: {n} frames into a 2 x 4 wall of 1920 x 1080, each cell 480 x 540 with the picture fitted (480 x 270,
  a 4 : 1 shrink per axis, bars above and below);
- `substreams`: the same {n} frames into {n} outputs of 640 x 360 (3 : 1 per axis), one launch;
- `inset`: one frame shown whole (a copy) in a 1920 x 1080 output with a 2 x inset (a 480 x 270 crop enlarged to 960 x 540) on top.

Everything below comes from ONE process on one MI355X.

How: device times are HIP-event times around the one launch of a run (`rtmodt_compose_last_ms`), medians of {iters} runs after
{warmup} warm-up runs.  `render_batch`'s kernel time is its own HIP-event time on the same {n} frames in the same process.  No
profiler was attached, nothing was fixed in advance and nothing is gated on these numbers.

    python tools/compose_time.py --out-dir profiles/compose

## Figures (`compose_time.json`)

| case | run | floor | x floor | x render kernel |
|---|---|---|---|---|
{rows}

The floor is the bytes the call must move, each once, at the {hbm:.2f} TB/s of the best `copy` line of
`profiles/r01/bandwidth_probe.txt` ({probe_line}): the bytes of every cell's crop plus the bytes of every output.  The inset case
counts the whole frame and the inset's crop although the part of the frame under the inset is never read.
The {n} source frames ({frames_mb:.1f} MB) fit the 256 MiB Infinity Cache and every run reads the same frames, so the source may come from that cache
rather than from HBM; the floor is priced at the HBM copy rate all the same.

`render_batch`'s kernel on the {n} frames: {render_ms:.3f} ms.

{verdict}

## What bounds the call

NOT profiled: no counter run was taken, so which of source loads, LDS traffic, the per-tap weight arithmetic and the stores bounds
a run is not known.  From the code: a tile of 32 x 8 output pixels stages its source footprint in LDS once, so a source byte is
fetched once per cell but for the rows and columns two neighbouring tiles share -- at most one row and one column of a footprint of
(32 r + 1) x (8 r + 1) pixels at ratio r, 16 % at r = 1 down to 4 % at r = 4 -- and an output byte is written once.  The distance
to the floor is therefore not a byte count; the 64-bit weight arithmetic per tap and the byte-wide LDS reads are the first
suspects.  Reported as measured, not tuned.

## Parity

PINNED, exactly: every output byte against `tests/compose_ref.py` (the wall, sub-stream 0 and the inset picture were compared again
in this run: {exact}); the restatement equals the snapshot resampler on shrinks and Pillow's `Image.reduce` on factors whose product
is a power of two.  KNOWN DIFFERENCE: for other integer factors ((3, 3), (2, 3), ...) Pillow multiplies by a truncated reciprocal
and is off by one in places; this compositor divides exactly.  UNPINNED: `cv2.resize` (INTER_AREA / INTER_LINEAR),
`cv2.cvtColor(..., COLOR_BGR2YUV_I420)` (its chroma comes from one pixel of the block) and any encoder's reading of the NV12: none
of them runs where this is tested.
{spread}"""

SPREAD = """
## Spread

The same command was run twice on this code, one run after the other; the figures above are the second run.  The first gave
{first} ms (second: {second} ms) for {names}, render kernel {r1:.3f} / {r2:.3f} ms: the largest difference between the runs is
{diff:.1f} %.  Within the second run a case's extremes lie within {within:.0f} % of its median (`minmax_ms` in `compose_time.json`).
"""


def timed(call, ms_of, warmup, iters):
    ms = []
    for k in range(warmup + iters):
        call()
        if k >= warmup:
            ms.append(ms_of())
    return {"ms": float(np.median(ms)), "minmax_ms": [float(min(ms)), float(max(ms))]}


def out_bytes(o):
    h, w = o.size
    return h * w * 3 if pkg._ffi.pixel_format_id(o.fmt) == pkg._ffi.PIX_BGR24 else h * w * 3 // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--first-run", default=None)
    a = ap.parse_args()
    V = pkg.visualization
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    src = pkg._ffi.DeviceBuffer(frames.nbytes)
    src.upload(frames)
    dev = [(src, i * H * W * 3, None) for i in range(N)]
    tbs, probe_line = hbm_rate()
    inset_cells = [V.Cell(0, 0, (0, 0, W, H), fit="stretch"), V.Cell(0, 0, (900, 60, 960, 540), (700, 400, 480, 270), "stretch")]
    cases = {
        "wall_bgr24": (V.Compositor.grid(N, (H, W), (H, W), cols=4), dev),
        "wall_nv12": (V.Compositor.grid(N, (H, W), (H, W), cols=4, fmt="nv12"), dev),
        "substreams": (V.Compositor([(H, W)] * N, [V.Output((360, 640)) for _ in range(N)], [V.Cell(i, i, (0, 0, 640, 360), fit="stretch") for i in range(N)]), dev),
        "inset": (V.Compositor([(H, W)], [V.Output((H, W))], inset_cells), dev[:1]),
    }
    res = {"tool": "tools/compose_time.py", "streams": N, "size": f"{W}x{H}", "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs,
           "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "cases": {}}
    exact = True
    for name, (comp, fr) in cases.items():
        crop_bytes = sum(p.crop[2] * p.crop[3] * 3 for p in comp.plans)
        floor_bytes = crop_bytes + sum(out_bytes(o) for o in comp.outputs)
        row = {"cells": len(comp.cells), "outputs": len(comp.outputs), "crop_bytes": crop_bytes, "floor_bytes": floor_bytes,
               "floor_us": floor_bytes / (tbs * 1e12) * 1e6}
        row.update(timed(lambda: comp.run(fr, "device"), comp.last_ms, a.warmup, a.iters))
        row["over_floor"] = row["ms"] * 1e3 / row["floor_us"]
        res["cases"][name] = row
    # parity again, on the timed inputs: the BGR wall, sub-stream 0, the inset picture
    rc = lambda c: compose_ref.Cell(0, c.source, tuple(c.rect), tuple(c.crop), V.compose._fit_id(c.fit), tuple(c.pad), tuple(c.offline))
    for name, k, n_src in (("wall_bgr24", 0, N), ("substreams", 0, N), ("inset", 0, 1)):
        comp = cases[name][0]
        cells = [rc(c) for c in comp.cells if c.output == k]
        want = compose_ref.compose([(H, W)] * n_src, [compose_ref.Output(*comp.outputs[k].size)], cells, list(frames[:n_src]))[0]
        view, pitch = comp.output(k)
        oh, ow = comp.outputs[k].size
        got = view.download(pitch * oh).reshape(oh, pitch)[:, :3 * ow].reshape(oh, ow, 3)
        ok = bool(np.array_equal(got, want))
        res["cases"][name]["bit_exact"] = ok
        exact &= ok
    r = pkg.FrameRenderer()
    rk = []
    for k in range(a.warmup + a.iters):
        r.render_batch(src, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if k >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    res["bit_exact"] = exact
    for comp, _ in cases.values():
        comp.close()
    src.free()

    rows = []
    for name, row in res["cases"].items():
        row["over_render_kernel"] = row["ms"] / res["render_kernel_ms"]
        rows.append(f"| {name} | {row['ms']:.3f} ms | {row['floor_us']:.1f} us | {row['over_floor']:.1f} x | {row['over_render_kernel']:.2f} x |")
    c = res["cases"]
    res["verdict"] = (f"Composing {N} 1080p frames into the wall takes {c['wall_bgr24']['ms']:.3f} ms as BGR24 ({c['wall_bgr24']['over_floor']:.1f} x its byte "
                      f"floor) and {c['wall_nv12']['ms']:.3f} ms as NV12 ({c['wall_nv12']['over_floor']:.1f} x); the {N} sub-streams take "
                      f"{c['substreams']['ms']:.3f} ms ({c['substreams']['over_floor']:.1f} x) and the frame with its inset {c['inset']['ms']:.3f} ms "
                      f"({c['inset']['over_floor']:.1f} x).  Reported as measured, not tuned.")
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "compose_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        spread = ""
        if a.first_run:
            first = json.load(open(a.first_run))
            names = list(c)
            pairs = [(first["cases"][k]["ms"], c[k]["ms"]) for k in names] + [(first["render_kernel_ms"], res["render_kernel_ms"])]
            within = max(max(abs(m - row["ms"]) for m in row["minmax_ms"]) / row["ms"] for row in c.values())
            spread = SPREAD.format(first=" / ".join(f"{x:.3f}" for x, _ in pairs[:-1]), second=" / ".join(f"{y:.3f}" for _, y in pairs[:-1]),
                                   names=" / ".join(names), r1=pairs[-1][0], r2=pairs[-1][1], diff=100 * max(abs(x - y) / y for x, y in pairs),
                                   within=100 * within)
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=frames.nbytes / 1e6, iters=a.iters, warmup=a.warmup, rows="\n".join(rows), hbm=tbs, probe_line=probe_line,
                                  render_ms=res["render_kernel_ms"], verdict=res["verdict"], exact="equal" if exact else "NOT EQUAL", spread=spread))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
