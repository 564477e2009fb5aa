"""Times PrivacyMask.apply_batch (csrc/privacy.hip) on 8 x 1080p BGR24 frames in device memory, 200 tracks and 2 privacy
polygons per frame -- the scene tools/render_time.py times the renderer on -- per mode (FILL, PIXELATE 16, BLUR (8, 2),
BLUR (16, 3)), in place and out of place, beside render_batch's kernel time on the same frames and the floor of reading and
writing the masked bytes once from HBM, all in one run.  Device times are the handle's HIP-event times around its launches
(rtmodt_privacy_last_ms), medians after a warm-up.  Writes privacy_time.json and README.md into --out-dir and prints the JSON line.

    python tools/privacy_time.py [--iters 30] [--out-dir profiles/privacy]
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
import privacy_ref  # noqa: E402
import render_time  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
POLYGONS = [p for _, p in render_time.ZONES]
HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0          # float4 copy as measured on this chip / data sheet
MODES = [("FILL", dict(mode="fill", color=(0, 0, 0))), ("PIXELATE 16", dict(mode="pixelate", cell=16)),
         ("BLUR (8, 2)", dict(mode="blur", radius=8, passes=2)), ("BLUR (16, 3)", dict(mode="blur", radius=16, passes=3))]

README = """# Privacy masking: timings (`tools/privacy_time.py`)

What is measured: {n} x 1080p BGR24 frames already in device memory, {tracks} track boxes and 2 privacy polygons per frame (the
scene `tools/render_time.py` times the renderer on); {masked_share:.1%} of the pixels are masked ({masked_mb:.1f} MB of {total_mb:.1f} MB).
Everything below comes from ONE process on one MI355X.

How: device times are HIP-event times around the launches of one `apply_batch` call (`rtmodt_privacy_last_ms`: paint or blur,
plus the commit launch of in-place BLUR; the copy that makes `dst` a copy of `src` out of place is outside the events), medians
of {iters} calls after {warmup} warm-up calls; the frames are uploaded afresh before each mode.  `render_batch`'s kernel time is its
own HIP-event time on the same frames and tracks, in the same run.  No profiler was attached, nothing was fixed in advance and
nothing is gated on these numbers.

    python tools/privacy_time.py --out-dir profiles/privacy

## Figures (`privacy_time.json`)

| mode | in place | out of place | in place / render kernel | in place / HBM floor |
|---|---|---|---|---|
{rows}

`render_batch`'s kernel on the same frames: {render_ms:.3f} ms.  The floor -- the masked bytes read once and written once,
{floor_mb:.1f} MB -- is {floor_us:.1f} us at the {hbm} TB/s a float4 copy reaches on this chip ({floor_spec_us:.1f} us at the data
sheet's 8.0 TB/s).  FILL reads nothing, so its floor is half of that.
FILL and PIXELATE sit an order of magnitude above that floor: at this coverage almost every tile tests all of its frame's 200
rectangles per pixel group, and a masked pixel is written as three single-byte stores (the frame's pitch and alignment are
the caller's); neither is tuned here, both stay below half of the render kernel's time.

{verdict}

## Parity

PINNED, byte for byte: the kernels against `tests/privacy_ref.py` (regions, mask, FILL, PIXELATE, BLUR; frame 0 of every mode
was compared again in this run: {exact}).  UNPINNED: parity with cv2's `blur` / `GaussianBlur` (iterated box passes stand in for
Gaussian weights, and no OpenCV is installed where this ran) and with any camera's privacy mask.
"""

REASONS = {
    "FILL": "",
    "PIXELATE 16": "",
    "BLUR (8, 2)": ("each 64 x 16 tile loads a (64 + 32) x (16 + 32) region per channel -- {amp:.1f} x its own pixels -- and runs two horizontal and two "
                    "vertical running-sum passes over it in LDS, one channel at a time, byte loads; in place a second launch commits the scratch image"),
    "BLUR (16, 3)": ("each 64 x 16 tile loads a (64 + 96) x (16 + 96) region per channel -- {amp:.1f} x its own pixels -- and runs three horizontal and "
                     "three vertical running-sum passes over it in LDS (54.9 KB per workgroup: two workgroups per CU), one channel at a time, byte loads"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    boxes = [(np.stack([t.xyxy for t in l]), np.zeros(len(l), np.int32)) for l in lists]
    src = pkg._ffi.DeviceBuffer(frames.nbytes)
    dst = pkg._ffi.DeviceBuffer(frames.nbytes)
    masked = sum(int(privacy_ref.mask_of(privacy_ref.regions(b, c, H, W), POLYGONS, H, W).sum()) for b, c in boxes)
    res = {"tool": "tools/privacy_time.py", "frames": N, "size": f"{W}x{H}", "tracks_per_frame": render_time.TRACKS, "polygons": len(POLYGONS),
           "iters": a.iters, "warmup": a.warmup, "masked_pixels": masked, "masked_share": masked / (N * H * W), "modes": {}}
    exact = True
    for name, kw in MODES:
        mask = pkg.visualization.PrivacyMask(polygons=POLYGONS, **kw)
        row = {}
        for where, out in (("in_place", None), ("out_of_place", dst)):
            src.upload(frames)
            ms = []
            for k in range(a.warmup + a.iters):
                if out is None and kw["mode"] != "fill" and k == a.warmup:
                    src.upload(frames)                    # in place the input changes from call to call: start the timed calls from the clean frames
                mask.apply_batch(src, boxes, out=out, height=H, width=W)
                if k >= a.warmup:
                    ms.append(mask.last_kernel_ms())
            row[where + "_ms"] = float(np.median(ms))
            row[where + "_minmax_ms"] = [float(min(ms)), float(max(ms))]
        got = dst.download(H * W * 3).reshape(H, W, 3)       # out of place: frame 0 of the clean frames, masked once
        ok = bool(np.array_equal(got, privacy_ref.apply(frames[0], *boxes[0], polygons=POLYGONS, **kw)))
        row["bit_exact_frame0"] = ok
        exact &= ok
        res["modes"][name] = row
        mask.close()
    r = pkg.FrameRenderer()
    src.upload(frames)
    rk = []
    for k in range(a.warmup + a.iters):
        r.render_batch(src, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if k >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    floor_bytes = 2 * 3 * masked
    res["floor_bytes"] = floor_bytes
    res["floor_us"] = {"measured_hbm": floor_bytes / (HBM_MEASURED_TBS * 1e12) * 1e6, "spec_hbm": floor_bytes / (HBM_SPEC_TBS * 1e12) * 1e6}
    res["bit_exact_frame0"] = exact
    rows, slow = [], []
    for name, kw in MODES:
        m = res["modes"][name]
        m["over_render_kernel"] = m["in_place_ms"] / res["render_kernel_ms"]
        m["over_floor"] = m["in_place_ms"] * 1e3 / res["floor_us"]["measured_hbm"]
        rows.append(f"| {name} | {m['in_place_ms']:.3f} ms | {m['out_of_place_ms']:.3f} ms | {m['over_render_kernel']:.2f} x | {m['over_floor']:.1f} x |")
        if m["over_render_kernel"] > 2.0:
            R = kw.get("radius", 0) * kw.get("passes", 0)
            why = REASONS[name].format(amp=(64 + 2 * R) * (16 + 2 * R) / 1024.0) or "see the kernel's header"
            slow.append(f"{name} takes {m['over_render_kernel']:.1f} x the render kernel's time: {why}.  Reported as measured, not tuned.")
    res["verdict"] = " ".join(slow) if slow else "No mode takes more than 2 x the render kernel's time."
    src.free(); dst.free()
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "privacy_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, tracks=render_time.TRACKS, masked_share=res["masked_share"], masked_mb=3 * masked / 1e6,
                                  total_mb=frames.nbytes / 1e6, iters=a.iters, warmup=a.warmup, rows="\n".join(rows),
                                  render_ms=res["render_kernel_ms"], floor_mb=floor_bytes / 1e6, floor_us=res["floor_us"]["measured_hbm"],
                                  floor_spec_us=res["floor_us"]["spec_hbm"], hbm=HBM_MEASURED_TBS, verdict=res["verdict"],
                                  exact="equal" if exact else "NOT EQUAL"))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
