"""Times FrameEnhancer.process (csrc/enhance.hip) on 8 x 1080p BGR24 frames in device memory -- the frames tools/render_time.py times
the renderer on -- at the defaults: (a) uniform-noise frames, (b) night frames with every pixel inside 16 levels (the worst case for
the LDS atomics of the histogram pass), (c) tile grids (1, 1) and (16, 16), (d) in place against separate destinations.  Beside each,
in the same run: LensCorrector.process through the identity lens, CameraHealth.process at scale 1 and render_batch's kernel on the
same frames; and the call's byte floor -- the source read twice, the destination written once, the histograms and curves once, at
the best copy rate of profiles/r01/bandwidth_probe.txt.  Device times are HIP-event times around the memset and the three launches
of one call (rtmodt_enhance_last_ms), medians after a warm-up.  Nothing is gated on these numbers.  Writes enhance_time.json and
README.md into --out-dir (an enhance_time_run1.json found there is quoted as the first of two runs; an enhance_kernel_stats.csv found
there -- `rocprofv3 --kernel-trace --stats`, a run of its own with --only default -- gives the split between the launches) and
prints the JSON line.

    python tools/enhance_time.py [--iters 30] [--out-dir profiles/enhance]
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import rtmodt_amd  # noqa: E402,F401
import enhance_ref  # noqa: E402
import render_time  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402
from motion_time import timed  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
#: name -> (content, tiles, in place)
CASES = {"default": ("uniform", (8, 8), False), "night16": ("night16", (8, 8), False), "tiles_1x1": ("uniform", (1, 1), False),
         "tiles_16x16": ("uniform", (16, 16), False), "in_place": ("uniform", (8, 8), True)}

README = """# Frame enhancement: timings (`tools/enhance_time.py`)

What is measured: one `FrameEnhancer.process` call on {n} streams of 1080p, BGR24 frames already in device memory ({frames_mb:.1f} MB:
the frames `tools/render_time.py` times the renderer on), at the defaults (8 x 8 tiles, clip limit 2.0, strength 256, smooth_shift 2,
SHIFT), on the same frames call after call.  Beside it, in the same process, `LensCorrector.process` through the identity lens,
`CameraHealth.process` at scale 1 and `render_batch`'s kernel on the same frames.  Everything below comes from ONE process on one
MI355X.

How: device times are HIP-event times around the memset and all three launches of one call together (`rtmodt_enhance_last_ms`), medians
of {iters} calls after {warmup} warm-up calls.  No profiler was attached, nothing was fixed in advance and nothing is gated on these
numbers.

    python tools/enhance_time.py --out-dir profiles/enhance

## Figures (`enhance_time.json`)

| case | frames | tiles | destination | call | floor | x floor |
|---|---|---|---|---|---|---|
{rows}

The floor is the bytes the call must move, each once, at the {hbm:.2f} TB/s of the best `copy` line of
`profiles/r01/bandwidth_probe.txt` ({probe_line}): the source read twice (the histogram pass and the apply pass) and the destination
written once ({frames_mb:.1f} MB each), plus per frame and tile the histogram written and read (2 x 1 KB), s read and written (2 x 512 B)
and lut8 written (256 B).  It leaves out the memset of the histograms, the lut8 every apply workgroup stages again and the axis tables.

In the same run: `LensCorrector.process`, identity lens, {lens_ms:.3f} ms; `CameraHealth.process`, scale 1, {health_ms:.3f} ms;
`render_batch`'s kernel, {render_ms:.3f} ms.

{verdict}

{split}

{spread}

## Parity

PINNED, exactly: the kernels against `tests/enhance_ref.py` (stream 0's output, histograms, state and result row of the first call were
compared again in this run in every case: {exact}).  UNPINNED: parity with `cv2.createCLAHE` (installed nowhere this runs; its tiles
are padded by reflection and its interpolation is float), every default (`tiles`, `clip_limit`, `smooth_shift`: validated on no real
footage) and any gain in detector recall (there is no trained checkpoint offline).  Only ONE form of histogram privatisation was
built (copies per lane group, runs of equal neighbours added once): no second form was timed against it, so night16 over default
says how far this form is from indifferent to the content, not that another form would be slower.  Occupancy, LDS bank conflicts
and the atomic rate were not profiled: no counters were collected.
"""


def content(kind, rng):
    if kind == "uniform":
        return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    return np.broadcast_to(rng.integers(24, 40, (N, H, W, 1), dtype=np.uint8), (N, H, W, 3)).copy()       # every pixel inside 16 levels


def floor_bytes(frames_bytes, tiles):
    return 3 * frames_bytes + N * tiles[0] * tiles[1] * (2 * 1024 + 2 * 512 + 256)


def kernel_split(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        for k in ("en_hist", "en_curve", "en_apply"):
            if k in r["Name"]:
                rows.setdefault(k, [0, 0.0])
                rows[k][0] += int(r["Calls"])
                rows[k][1] += float(r["TotalDurationNs"])
    return {k: {"calls": c, "mean_us": t / c / 1e3} for k, (c, t) in rows.items() if c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case alone, nothing beside it (for a kernel trace)")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    data = {k: content(k, rng) for k in ("uniform", "night16")}
    nbytes = data["uniform"].nbytes
    src, dst = pkg._ffi.DeviceBuffer(nbytes), pkg._ffi.DeviceBuffer(nbytes)
    tbs, probe_line = hbm_rate()
    res = {"tool": "tools/enhance_time.py", "streams": N, "size": f"{W}x{H}", "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs,
           "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "cases": {}}
    exact = True
    for name, (kind, tiles, in_place) in CASES.items():
        if a.only and name != a.only:
            continue
        frames = data[kind]
        src.upload(frames)
        en = pkg.ingestion.FrameEnhancer(N, H, W, tiles=tiles)
        ref = enhance_ref.Ref(1, H, W, tiles_y=tiles[0], tiles_x=tiles[1])
        want, wrow = ref.step(0, frames[0])
        got = en.process(src, None if in_place else dst)[0]
        out = (src if in_place else dst).download(H * W * 3).reshape(H, W, 3)
        ok = bool(np.array_equal(out, want)) and got._asdict() == wrow and bool(np.array_equal(en.histograms(0), ref.hist[0]))
        ok = ok and bool(np.array_equal(en.state(0)[0], ref.state(0)[0]))
        row = {"frames": kind, "tiles": list(tiles), "in_place": in_place, "bit_exact": ok, "floor_bytes": floor_bytes(nbytes, tiles)}
        exact &= ok
        row["floor_us"] = row["floor_bytes"] / (tbs * 1e12) * 1e6

        def one(k):
            if in_place:
                src.upload(frames)                                      # (outside the events: every call enhances the same frames)
            en.process(src, None if in_place else dst, want_results=False)

        row.update(timed(one, en.kernel_ms, a.warmup, a.iters))
        row["over_floor"] = row["ms"] * 1e3 / row["floor_us"]
        res["cases"][name] = row
        en.close()
    res["bit_exact"] = exact
    if a.only:
        print(json.dumps(res))
        return 0 if exact else 1
    src.upload(data["uniform"])
    lc = pkg.ingestion.LensCorrector(N, (H, W))
    for s in range(N):
        lc.set_model(s, (1000.0, 1000.0, (W - 1) / 2, (H - 1) / 2), (0.0, 0.0, 0.0, 0.0))
    res["lens_identity"] = timed(lambda k: lc.process(src, out=dst), lc.last_ms, a.warmup, a.iters)
    lc.close()
    mon = pkg.ingestion.CameraHealth(N, H, W, scale=1)
    res["health_scale1"] = timed(lambda k: mon.process(src), mon.last_kernel_ms, a.warmup, a.iters)
    mon.close()
    r = pkg.FrameRenderer()
    lists = [render_time.scene(rng) for _ in range(N)]
    res["render_kernel"] = timed(lambda k: r.render_batch(src, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W), r.last_kernel_ms,
                                 a.warmup, a.iters)
    src.free(); dst.free()

    c = res["cases"]
    rows = [f"| {name} | {row['frames']} | {row['tiles'][0]} x {row['tiles'][1]} | {'in place' if row['in_place'] else 'separate'} | {row['ms']:.3f} ms | "
            f"{row['floor_us']:.1f} us | {row['over_floor']:.1f} x |" for name, row in c.items()]
    res["night_over_uniform"] = c["night16"]["ms"] / c["default"]["ms"]
    res["verdict"] = (f"At the defaults the call takes {c['default']['ms']:.3f} ms for {N} streams on uniform noise ({c['default']['ms'] / N * 1e3:.0f} us per frame, "
                      f"{c['default']['over_floor']:.1f} x its byte floor), {c['default']['ms'] / res['lens_identity']['ms']:.2f} x the identity lens call, "
                      f"{c['default']['ms'] / res['health_scale1']['ms']:.2f} x the health call at scale 1 and {c['default']['ms'] / res['render_kernel']['ms']:.2f} x the render "
                      f"kernel.  Night frames with every pixel inside 16 levels take {c['night16']['ms']:.3f} ms: {res['night_over_uniform']:.2f} x the uniform-noise "
                      f"call -- the figure that says whether the histogram privatisation is enough.  One tile takes {c['tiles_1x1']['ms']:.3f} ms, 16 x 16 tiles "
                      f"{c['tiles_16x16']['ms']:.3f} ms; in place {c['in_place']['ms']:.3f} ms against {c['default']['ms']:.3f} ms into separate destinations.  "
                      f"Reported as measured, not tuned.")
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        split = "The split between the three launches was not measured: no kernel trace was taken."
        stats = os.path.join(a.out_dir, "enhance_kernel_stats.csv")
        if os.path.exists(stats):
            ks = kernel_split(stats)
            res["kernel_split"] = ks
            total = sum(v["mean_us"] for v in ks.values())
            split = ("The split between the launches, from a kernel trace in a run of its own (`rocprofv3 --kernel-trace --stats -- python "
                     "tools/enhance_time.py --only default`, `enhance_kernel_stats.csv`; mean device time per launch, uniform noise, defaults): "
                     + ", ".join(f"`{k}` {v['mean_us']:.1f} us ({100 * v['mean_us'] / total:.0f} %)" for k, v in ks.items()) + ".")
        prev_path = os.path.join(a.out_dir, "enhance_time_run1.json")
        spread = "Only one run was made."
        if os.path.exists(prev_path):
            prev = json.load(open(prev_path))
            parts = [f"{k} {prev['cases'][k]['ms']:.3f} ms (this run {c[k]['ms']:.3f})" for k in c]
            spread = ("The same command was run twice on this code, one run after the other; the figures above are the second run, "
                      "`enhance_time_run1.json` the first: " + "; ".join(parts) + f"; identity lens {prev['lens_identity']['ms']:.3f} ({res['lens_identity']['ms']:.3f}), "
                      f"health at scale 1 {prev['health_scale1']['ms']:.3f} ({res['health_scale1']['ms']:.3f}), render kernel {prev['render_kernel']['ms']:.3f} "
                      f"({res['render_kernel']['ms']:.3f}).  Within a run the extremes of each figure are in `minmax_ms`.")
        with open(os.path.join(a.out_dir, "enhance_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=nbytes / 1e6, iters=a.iters, warmup=a.warmup, rows="\n".join(rows), hbm=tbs, probe_line=probe_line,
                                  lens_ms=res["lens_identity"]["ms"], health_ms=res["health_scale1"]["ms"], render_ms=res["render_kernel"]["ms"],
                                  verdict=res["verdict"], split=split, spread=spread, exact="equal" if exact else "NOT EQUAL"))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
