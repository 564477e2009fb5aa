"""Times LensCorrector.process (csrc/lens.hip) on 8 x 1080p BGR24 frames in device memory -- the frames tools/render_time.py times
the renderer on -- device to device, same size out: a moderate barrel lens (k1 = -0.30, k2 = 0.10) and an identity lens, the pure
copy through the table; beside the call's floor -- table, source and destination bytes, each moved once, at the best copy rate of
profiles/r01/bandwidth_probe.txt -- and, in the same run, render_batch's kernel time on the same frames.  Device times are HIP-event
times around the one launch of a call (rtmodt_lens_last_ms), medians after a warm-up.  Writes lens_time.json and README.md into
--out-dir and prints the JSON line.  --first-run: the JSON of an earlier run of the same command, quoted in the README's spread.

    python tools/lens_time.py [--iters 200] [--out-dir profiles/lens] [--first-run first.json]
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
import lens_ref  # noqa: E402
import render_time  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
K = (1100.0, 1100.0, (W - 1) / 2, (H - 1) / 2)
LENSES = {"barrel": (-0.30, 0.10, 0.0, 0.0), "identity": (0.0, 0.0, 0.0, 0.0)}

README = """# Lens correction: timings (`tools/lens_time.py`)

What is measured: one `LensCorrector.process` call on {n} streams of 1080p, BGR24 frames already in device memory ({frames_mb:.1f} MB:
the frames `tools/render_time.py` times the renderer on), device to device, the rectified frames the same size.  Barrel: a moderate
lens, k1 = -0.30, k2 = 0.10 at f = 1100 px, output intrinsics = source intrinsics ({barrel_out} of {px} output pixels per stream are
border).  Identity: all coefficients zero, the pure copy through the table.  Every stream has its own table.  Everything below comes
from ONE process on one MI355X.

How: device times are HIP-event times around the one launch of a call (`rtmodt_lens_last_ms`), medians of {iters} calls after
{warmup} warm-up calls.  `render_batch`'s kernel time is its own HIP-event time on the same frames in the same run.  No profiler was
attached, nothing was fixed in advance and nothing is gated on these numbers.

    python tools/lens_time.py --out-dir profiles/lens

## Figures (`lens_time.json`)

| lens | process | floor | x floor | x render kernel |
|---|---|---|---|---|
{rows}

The floor is the bytes the call must move, each once, at the {hbm:.2f} TB/s of the best `copy` line of
`profiles/r01/bandwidth_probe.txt` ({probe_line}): {table_mb:.1f} MB of table (8 B per output pixel), {frames_mb:.1f} MB of source and
{frames_mb:.1f} MB of destination.  It counts every source byte once although the barrel lens does not read the source's rim.

`render_batch`'s kernel on the same frames: {render_ms:.3f} ms.

{verdict}

## What was and was not tried

The kernel gathers the four taps of each channel with byte loads straight from the source at the caller's pitch, for any base
address and pitch.  Staging an output tile's source footprint in LDS was NOT tried, and wider source loads (dwords where base and
pitch allow) were NOT tried either: correctness was this module's acceptance criterion.  Computing the map per pixel on the device
instead of reading the 8 B table entry is the follow-up these figures are the yardstick for.  Which of table reads, tap loads and
stores bounds the call was not profiled: no counter run was taken.

## Parity

PINNED, exactly: table and output bytes against `tests/lens_ref.py` (stream 0's table and rectified frame were compared again in
this run for both lenses: {exact}).  UNPINNED: parity with `cv2.undistort` / `initUndistortRectifyMap` / `remap` (cv2's table rounds
differently and is not installed where this runs), the `fisheye_map` helper, and any calibration on real footage.
{spread}"""

SPREAD = """
## Spread

The same command was run twice on this code, one run after the other on one machine; the figures above are the second run.  The
first gave barrel {b1:.3f} ms, identity {i1:.3f} ms, render kernel {r1:.3f} ms (second: {b2:.3f} / {i2:.3f} / {r2:.3f} ms): the largest
difference between the runs is {diff:.1f} %.  Within the second run a call's extremes lie within {within:.0f} % of its median
(`minmax_ms` in `lens_time.json`).
"""


def timed(call, ms_of, warmup, iters):
    ms = []
    for k in range(warmup + iters):
        call()
        if k >= warmup:
            ms.append(ms_of())
    return {"ms": float(np.median(ms)), "minmax_ms": [float(min(ms)), float(max(ms))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--first-run", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    src, dst = pkg._ffi.DeviceBuffer(frames.nbytes), pkg._ffi.DeviceBuffer(frames.nbytes)
    src.upload(frames)
    tbs, probe_line = hbm_rate()
    table_bytes = 8 * N * H * W
    floor_bytes = table_bytes + 2 * frames.nbytes
    res = {"tool": "tools/lens_time.py", "streams": N, "size": f"{W}x{H}", "K": list(K), "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs,
           "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "floor_bytes": floor_bytes, "floor_us": floor_bytes / (tbs * 1e12) * 1e6,
           "lenses": {}}
    exact = True
    for name, dist in LENSES.items():
        lc = pkg.ingestion.LensCorrector(N, (H, W))
        n_out = [lc.set_model(s, K, dist) for s in range(N)][0]
        row = {"dist": list(dist), "n_outside": n_out}
        row.update(timed(lambda: lc.process(src, out=dst), lc.last_ms, a.warmup, a.iters))
        row["over_floor"] = row["ms"] * 1e3 / res["floor_us"]
        table = lens_ref.build_model(lens_ref.Lens(*K, dist), (H, W))
        ok = all(np.array_equal(g, w) for g, w in zip(lc.map(0), table))
        ok = ok and np.array_equal(dst.download(H * W * 3).reshape(H, W, 3), lens_ref.sample(frames[0], table))
        if name == "identity":
            ok = ok and np.array_equal(dst.download(), frames.ravel())
        row["bit_exact"] = bool(ok)
        exact &= bool(ok)
        res["lenses"][name] = row
        lc.close()
    r = pkg.FrameRenderer()
    rk = []
    for k in range(a.warmup + a.iters):
        r.render_batch(src, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if k >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    res["bit_exact"] = exact
    src.free(); dst.free()

    rows = []
    for name, row in res["lenses"].items():
        row["over_render_kernel"] = row["ms"] / res["render_kernel_ms"]
        rows.append(f"| {name} | {row['ms']:.3f} ms | {res['floor_us']:.1f} us | {row['over_floor']:.1f} x | {row['over_render_kernel']:.2f} x |")
    b, i = res["lenses"]["barrel"], res["lenses"]["identity"]
    res["verdict"] = (f"Rectifying {N} 1080p frames takes {b['ms']:.3f} ms through the barrel lens ({b['over_floor']:.1f} x its byte floor) and {i['ms']:.3f} ms "
                      f"through the identity lens ({i['over_floor']:.1f} x): {b['ms'] / N * 1e3:.0f} us per frame, {b['over_render_kernel']:.2f} x the render "
                      f"kernel's time on the same frames.  Reported as measured, not tuned.")
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "lens_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        spread = ""
        if a.first_run:
            first = json.load(open(a.first_run))
            pairs = [(first["lenses"]["barrel"]["ms"], b["ms"]), (first["lenses"]["identity"]["ms"], i["ms"]), (first["render_kernel_ms"], res["render_kernel_ms"])]
            within = max(max(abs(m - row["ms"]) for m in row["minmax_ms"]) / row["ms"] for row in (b, i))
            spread = SPREAD.format(b1=pairs[0][0], i1=pairs[1][0], r1=pairs[2][0], b2=pairs[0][1], i2=pairs[1][1], r2=pairs[2][1],
                                   diff=100 * max(abs(x - y) / y for x, y in pairs), within=100 * within)
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=frames.nbytes / 1e6, barrel_out=b["n_outside"], px=H * W, iters=a.iters, warmup=a.warmup,
                                  rows="\n".join(rows), hbm=tbs, probe_line=probe_line, table_mb=table_bytes / 1e6, render_ms=res["render_kernel_ms"],
                                  verdict=res["verdict"], exact="equal" if exact else "NOT EQUAL", spread=spread))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
