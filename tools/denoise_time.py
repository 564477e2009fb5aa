"""Times FrameDenoiser.process (csrc/denoise.hip) on 8 x 1080p BGR24 frames in device memory -- the frames' size tools/render_time.py
times the renderer on -- at the defaults: (a) a still scene under fresh sensor noise of +-4 in every call, (b) the same with 200 boxes
per stream that move between the calls.  Four frame sets are uploaded once and taken in turn, so every call sees new noise and moved
boxes.  Beside each, in the same run: FrameEnhancer.process at its defaults, LensCorrector.process through the identity lens and
render_batch's kernel on the same frames; and the call's byte floor -- per pixel 3 bytes of the frame, 6 of acc and 1 of the Y(prev)
plane read, and as many written: 20 bytes -- at 6.3 TB/s, the achievable HBM streaming rate tools/layer_roofline.py uses (8 TB/s is the
peak; the best copy line of profiles/r01/bandwidth_probe.txt, a copy that the 256 MB last-level cache holds, is quoted beside it).
Device times are HIP-event times around the memset and the two launches of one call (rtmodt_denoise_last_ms), medians after a
warm-up.  Nothing is gated on these numbers.  Writes denoise_time.json and README.md into --out-dir (a denoise_time_run1.json found there is quoted as the first of two
runs; a denoise_kernel_stats.csv found there -- `rocprofv3 --kernel-trace --stats`, a run of its own with --only still -- gives the
split between the launches) and prints the JSON line.

    python tools/denoise_time.py [--iters 30] [--out-dir profiles/denoise]
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
import denoise_ref  # noqa: E402
import render_time  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402
from motion_time import timed  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
SETS, NOISE, BOXES, BOX, LIFT, STEP = 4, 4, 200, 24, 60, 8
CASES = {"still": 0, "boxes200": BOXES}
BYTES_PER_PIXEL = 20
HBM_TBS = 6.3                                               # achievable streaming rate (tools/layer_roofline.py); the peak is 8 TB/s

README = """# Frame noise reduction: timings (`tools/denoise_time.py`) and what the filter gains

## What the filter gains, on the restatements alone (`tests/test_denoise_cpu.py`)

`enhance_cases.night_scene()` at 320 x 240 under uniform noise of +-4 / +-8 levels on every channel, 30 still frames and then 20 in
which a box moves 8 px a frame, through `tests/denoise_ref.py` at the defaults.  No GPU is involved; the kernel equals the restatement
byte for byte (`tests/test_gpu_denoise.py`).

| noise | PSNR raw -> filtered, frame 29 | gain at temporal_shift 3 (derived 11.76 dB) | gain at temporal_shift 2 (derived 8.45 dB) | JPEG bytes filtered / raw, quality 85 |
|---|---|---|---|---|
| +-4 | 39.88 -> 50.88 dB | 10.99 dB | 8.11 dB | 0.91 |
| +-8 | 34.33 -> 45.40 dB | 11.07 dB | 8.20 dB | 0.77 |

The derived figure is the steady state of a first-order filter of weight w = 2^-temporal_shift on white noise, `10 log10((2 - w) / w)`;
the measured gains fall 0.25 to 0.8 dB short of it (quantisation, the clip at 0); the test allows 2 dB.  Every frame from the tenth on
is a smaller JPEG.  Behind a box 60 levels brighter, in the 40 columns it has just left, the mean absolute error against the clean
frame is 1.43 (raw 2.22) at +-4 and 2.13 (raw 4.24) at +-8, inside the box 1.58 (2.17) and 2.33 (4.14): no trail; a filter that holds
every pixel as static leaves 16.9 and 43.4 there.  `enhance_ref` -> `motion_ref` gives the same status on all 50 frames of the lift-8
sequence with and without the filter, MOTION on all 20 moving frames.  No gain in detector recall is claimed: there is no trained
checkpoint offline.

## Timings

What is measured: one `FrameDenoiser.process` call on {n} streams of 1080p, BGR24 frames already in device memory ({frames_mb:.1f} MB),
into a second device buffer, at the defaults (motion 18 / 54, temporal_shift 3, spatial 256, spatial_thr 6).  {sets} frame sets are
uploaded once and taken in turn: every call sees fresh noise of +-{noise} and, in `boxes200`, {boxes} boxes of {box} x {box} pixels per
stream, {lift} levels brighter, each moved {step} px since the call before.  Beside it, in the same process, `FrameEnhancer.process` at
its defaults, `LensCorrector.process` through the identity lens and `render_batch`'s kernel on the same frames.  Everything below comes
from ONE process on one MI355X.

How: device times are HIP-event times around the memset and both launches of one call together (`rtmodt_denoise_last_ms`), medians of
{iters} calls after {warmup} warm-up calls.  No profiler was attached, nothing was fixed in advance and nothing is gated on these
numbers.

    python tools/denoise_time.py --out-dir profiles/denoise

| case | call | moving pixels per frame | floor | x floor |
|---|---|---|---|---|
{rows}

The floor is the bytes the call must move, each once -- per pixel 3 bytes of the frame, 6 of `acc` and 1 of the Y(prev) plane read and
as many written, {bpp} bytes, {floor_mb:.1f} MB for this batch -- at {hbm:.1f} TB/s, the achievable HBM streaming rate
`tools/layer_roofline.py` uses (the peak is 8 TB/s; the best `copy` line of `profiles/r01/bandwidth_probe.txt`, {probe_tbs:.2f} TB/s at
{probe_line}, is a copy the 256 MB last-level cache holds, and at it the floor would be {floor_probe_us:.1f} us).  The state of this batch,
{state_mb:.0f} MB of `acc` and planes, does not fit that cache beside the frames.  The floor leaves out the halo rows a tile reads again
(2 of 18), the counters and the result rows.

In the same run: `FrameEnhancer.process`, defaults, {enhance_ms:.3f} ms; `LensCorrector.process`, identity lens, {lens_ms:.3f} ms;
`render_batch`'s kernel, {render_ms:.3f} ms.

{verdict}

{split}

{spread}

## Parity

PINNED, exactly: the kernel against `tests/denoise_ref.py` (stream 0's outputs, state and result rows of the first two calls were
compared again in this run in every case: {exact}).  UNPINNED: parity with any camera's 3DNR, `cv2.fastNlMeansDenoising` or ffmpeg's
`hqdn3d` (none is installed where this runs), every default (validated on no real footage) and any gain in detector recall.  Only ONE
form of the kernel was built (a 256 x 16 tile, the Y(prev) plane double-buffered): no second form was timed against it.  Occupancy,
LDS bank conflicts and the share of the integer divisions were not profiled: no counters were collected.
"""


def frame_sets(rng, boxes):
    """-> uint8 (SETS, N, H, W, 3): one still scene per stream under fresh noise per set, with `boxes` boxes that move STEP px a set"""
    base = rng.integers(40, 120, (N, H // 8, W // 8, 1)).repeat(8, 1).repeat(8, 2) + rng.integers(-4, 5, (N, H, W, 1))
    at = rng.integers(0, [H - BOX - STEP * SETS, W - BOX - STEP * SETS], (N, boxes, 2)) if boxes else None
    out = np.empty((SETS, N, H, W, 3), np.uint8)
    for k in range(SETS):
        img = base + np.zeros((1, 1, 1, 3), np.int64)
        for s in range(N):
            for b in range(boxes):
                y, x = at[s, b] + STEP * k
                img[s, y:y + BOX, x:x + BOX] += LIFT
        out[k] = np.clip(img + rng.integers(-NOISE, NOISE + 1, img.shape), 0, 255)
    return out


def kernel_split(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        for k in ("dn_filter", "dn_finish"):
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
    nbytes = N * H * W * 3
    srcs, dst = [pkg._ffi.DeviceBuffer(nbytes) for _ in range(SETS)], pkg._ffi.DeviceBuffer(nbytes)
    tbs = HBM_TBS
    probe_tbs, probe_line = hbm_rate()
    floor_bytes = N * H * W * BYTES_PER_PIXEL
    res = {"tool": "tools/denoise_time.py", "streams": N, "size": f"{W}x{H}", "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs,
           "hbm_source": "achievable HBM streaming rate, as in tools/layer_roofline.py (peak 8 TB/s)", "probe_copy_tbs": probe_tbs, "floor_bytes": floor_bytes, "floor_us": floor_bytes / (tbs * 1e12) * 1e6, "cases": {}}
    exact = True
    for name, boxes in CASES.items():
        if a.only and name != a.only:
            continue
        data = frame_sets(rng, boxes)
        for k in range(SETS):
            srcs[k].upload(data[k])
        dn = pkg.ingestion.FrameDenoiser(N, H, W)
        ref = denoise_ref.Ref(1, H, W)
        ok, moving = True, 0
        for k in range(2):
            want, wrow = ref.step(0, data[k, 0])
            got = dn.process(srcs[k], dst)
            ok = ok and bool(np.array_equal(dst.download(H * W * 3).reshape(H, W, 3), want)) and got[0]._asdict() == wrow
            ok = ok and bool(np.array_equal(dn.state(0)[0], ref.state(0)[0]))
        exact &= ok
        seen = []

        def one(k):
            seen.append(dn.process(srcs[k % SETS], dst, want_results=k % 8 == 7))

        row = {"boxes": boxes, "bit_exact": ok}
        row.update(timed(one, dn.kernel_ms, a.warmup, a.iters))
        rows_back = [r for res_ in seen if res_ for r in res_]
        row["moving_per_frame"] = sum(r.n_moving for r in rows_back) / max(len(rows_back), 1)
        row["noise_q8"] = sum(r.noise_q8 for r in rows_back) / max(len(rows_back), 1)
        row["over_floor"] = row["ms"] * 1e3 / res["floor_us"]
        row["tbs"] = floor_bytes / (row["ms"] * 1e-3) / 1e12
        res["cases"][name] = row
        dn.close()
    res["bit_exact"] = exact
    if a.only:
        print(json.dumps(res))
        return 0 if exact else 1
    src = srcs[0]
    en = pkg.ingestion.FrameEnhancer(N, H, W)
    res["enhance_default"] = timed(lambda k: en.process(src, dst, want_results=False), en.kernel_ms, a.warmup, a.iters)
    en.close()
    lc = pkg.ingestion.LensCorrector(N, (H, W))
    for s in range(N):
        lc.set_model(s, (1000.0, 1000.0, (W - 1) / 2, (H - 1) / 2), (0.0, 0.0, 0.0, 0.0))
    res["lens_identity"] = timed(lambda k: lc.process(src, out=dst), lc.last_ms, a.warmup, a.iters)
    lc.close()
    r = pkg.FrameRenderer()
    lists = [render_time.scene(rng) for _ in range(N)]
    res["render_kernel"] = timed(lambda k: r.render_batch(src, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W), r.last_kernel_ms,
                                 a.warmup, a.iters)
    for b in srcs + [dst]:
        b.free()

    c = res["cases"]
    rows = [f"| {name} | {row['ms']:.3f} ms | {row['moving_per_frame']:.0f} | {res['floor_us']:.1f} us | {row['over_floor']:.1f} x |" for name, row in c.items()]
    res["boxes_over_still"] = c["boxes200"]["ms"] / c["still"]["ms"]
    res["verdict"] = (f"On the still scene the call takes {c['still']['ms']:.3f} ms for {N} streams ({c['still']['ms'] / N * 1e3:.0f} us per frame, "
                      f"{c['still']['over_floor']:.1f} x its byte floor, {c['still']['tbs']:.2f} TB/s of the floor's bytes), {c['still']['ms'] / res['enhance_default']['ms']:.2f} x "
                      f"the enhancer's call, {c['still']['ms'] / res['lens_identity']['ms']:.2f} x the identity lens call and {c['still']['ms'] / res['render_kernel']['ms']:.2f} x "
                      f"the render kernel.  With {BOXES} moving boxes per stream it takes {c['boxes200']['ms']:.3f} ms: {res['boxes_over_still']:.2f} x the still call.  Every "
                      f"pixel runs both filters whatever it shows; where a difference between the two cases comes from was not looked into.  The noise figure reported on the still scene is "
                      f"{c['still']['noise_q8'] / 256:.2f} levels.  Reported as measured, not tuned.")
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        split = "The split between the two launches was not measured: no kernel trace was taken."
        stats = os.path.join(a.out_dir, "denoise_kernel_stats.csv")
        if os.path.exists(stats):
            ks = kernel_split(stats)
            res["kernel_split"] = ks
            total = sum(v["mean_us"] for v in ks.values())
            split = ("The split between the launches, from a kernel trace in a run of its own (`rocprofv3 --kernel-trace --stats -- python "
                     "tools/denoise_time.py --only still`, `denoise_kernel_stats.csv`; mean device time per launch, still scene, defaults): "
                     + ", ".join(f"`{k}` {v['mean_us']:.1f} us ({100 * v['mean_us'] / total:.0f} %)" for k, v in ks.items()) + ".")
        prev_path = os.path.join(a.out_dir, "denoise_time_run1.json")
        spread = "Only one run was made."
        if os.path.exists(prev_path):
            prev = json.load(open(prev_path))
            parts = [f"{k} {prev['cases'][k]['ms']:.3f} ms (this run {c[k]['ms']:.3f})" for k in c]
            spread = ("The same command was run twice on this code, one run after the other; the figures above are the second run, "
                      "`denoise_time_run1.json` the first: " + "; ".join(parts) + f"; enhancer {prev['enhance_default']['ms']:.3f} ({res['enhance_default']['ms']:.3f}), "
                      f"identity lens {prev['lens_identity']['ms']:.3f} ({res['lens_identity']['ms']:.3f}), render kernel {prev['render_kernel']['ms']:.3f} "
                      f"({res['render_kernel']['ms']:.3f}).  Within a run the extremes of each figure are in `minmax_ms`.")
        with open(os.path.join(a.out_dir, "denoise_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=nbytes / 1e6, sets=SETS, noise=NOISE, boxes=BOXES, box=BOX, lift=LIFT, step=STEP, iters=a.iters, warmup=a.warmup,
                                  rows="\n".join(rows), bpp=BYTES_PER_PIXEL, floor_mb=floor_bytes / 1e6, hbm=tbs, probe_line=probe_line, probe_tbs=probe_tbs,
                                  floor_probe_us=floor_bytes / (probe_tbs * 1e12) * 1e6, state_mb=N * H * W * 8 / 1e6,
                                  enhance_ms=res["enhance_default"]["ms"], lens_ms=res["lens_identity"]["ms"], render_ms=res["render_kernel"]["ms"],
                                  verdict=res["verdict"], split=split, spread=spread, exact="equal" if exact else "NOT EQUAL"))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
