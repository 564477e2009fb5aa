"""Times sliced inference (csrc/slice.hip) on 1080p device frames, tile 640, overlap 128, overview on -- 9 images per frame --
beside the detector's own time for the same image batch and the unsliced path on the same frames, in one run.  Device times come
from HIP events (the slicer's and the detector's own), end-to-end rates from a host clock around a pipelined loop that ends in a
fetch.  Writes slice_time.json and README.md into --out-dir and prints the JSON line.

    python tools/slice_time.py [--frames 7] [--repeat 30] [--steps 60] [--out-dir profiles/slice]

A detector batch holds at most 64 images, so at 9 images per frame a sliced batch holds at most 7 frames (63 images).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import rtmodt_amd  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
S = pkg.detection.sliced
W, H, TILE, OVERLAP = 1920, 1080, 640, 128
HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0          # float4 copy as measured on this chip / data sheet

README = """# Sliced inference: timings (`tools/slice_time.py`)

What is measured: {frames} x 1080p BGR frames already in device memory, tile 640, overlap 128, overview on: {images} images of
640 x 640 per sliced batch (a detector batch holds at most 64 images, so 7 frames is the largest 1080p batch: 8 frames would be
72 images).  YOLOv8s with synthetic weights, confidence {conf}, max_det {max_det}, merge NMM / IoS / {match}.
Everything below comes from ONE process on one MI355X.

How: device times are HIP-event times -- `slice_gather` and `slice_merge` from the slicer's own events around each launch, the
detector's from its events around the whole pass of the same batch (letterbox-free stem .. NMS) -- medians of {repeat} synchronous
batches after {warmup} warm-up batches.  Rates are a host clock around {steps} pipelined batches (two in flight, the loop ends
in a fetch), after the same warm-up.  No profiler was attached, nothing was fixed in advance, nothing is gated on these numbers.

    python tools/slice_time.py --out-dir profiles/slice

## Figures (`slice_time.json`)

| per sliced batch of {frames} frames ({images} images) | device time | share of the detector's pass |
|---|---|---|
| `slice_gather` | {gather_ms:.3f} ms | {gather_share:.1%} |
| `slice_merge`, {cand_mean:.0f} candidates per frame (measured counts) | {merge_ms:.3f} ms | {merge_share:.1%} |
| `slice_merge`, 100 candidates per image ({cand_full} per frame), kernel alone | {merge_full_ms:.3f} ms | {merge_full_share:.1%} |
| detector, whole pass of the {images}-image batch | {det_ms:.3f} ms | 1 |
| detector, forward part of it | {fwd_ms:.3f} ms | |

`slice_gather` reads {frames} frames and writes {images} tiles: {gather_mb:.1f} MB if every byte moved once, which takes
{gather_floor_us:.1f} us at the {hbm} TB/s a float4 copy reaches on this chip ({gather_floor_spec_us:.1f} us at the 8.0 TB/s of the data
sheet); the kernel took {gather_x:.1f} x that.  (The tiles overlap, so the frames' bytes are read about {reread:.2f} times, mostly from
L2, and the overview reads four taps per pixel.)

| end to end, {frames} frames per batch, two batches in flight | frames/s | images/s |
|---|---|---|
| sliced ({images} images of 640 x 640 per batch) | {sliced_fps:.0f} | {sliced_ips:.0f} |
| unsliced (the same frames letterboxed to 640 x 640) | {plain_fps:.0f} | {plain_fps:.0f} |

The sliced path delivers {ratio:.2f} x fewer frames per second than the unsliced one on the same frames ({inv_images} would be the
image count alone).  Beside the forward pass: {verdict}

Merged detections per frame: {merged_mean:.0f} from {cand_mean:.0f} candidates.  The weights are synthetic, so the counts say nothing about
accuracy.  PARITY UNPINNED: `sahi` is installed nowhere this ran.  UNPINNED: any accuracy gain on real footage.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--conf", type=float, default=0.05)
    ap.add_argument("--match", type=float, default=0.5)
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    n, max_det = a.frames, 100
    path = os.path.join(tempfile.mkdtemp(prefix="rtmodt_slice_"), "yolov8s_640_noise.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("s", input_size=TILE), "s")
    frames = pkg.synth.structured_frames(n, H, W, seed=11)
    buf = pkg._ffi.DeviceBuffer(frames.nbytes)
    buf.upload(frames)
    ptrs = [buf.ptr + i * frames[0].nbytes for i in range(n)]
    tune = not a.no_autotune
    sd = pkg.SlicedDetector(path, frame_size=(W, H), streams=n, tile=(TILE, TILE), overlap=(OVERLAP, OVERLAP), match_threshold=a.match,
                            confidence=a.conf, max_det=max_det, autotune=tune, warmup=False)
    I = sd.images_per_frame
    res = {"tool": "tools/slice_time.py", "frames": n, "images": n * I, "tile": TILE, "overlap": OVERLAP, "conf": a.conf, "match": a.match,
           "max_det": max_det, "autotune": tune, "repeat": a.repeat, "warmup": a.warmup, "steps": a.steps,
           "stages": sd.detector.model.stages, "chains": sd.detector.model.chains}

    # ---- device times per synchronous batch
    g_ms, m_ms, d_ms, f_ms, cand, merged = [], [], [], [], [], []
    for k in range(a.warmup + a.repeat):
        sd.enqueue(ptrs)
        dets = sd.fetch()
        if k < a.warmup:
            continue
        g, m = sd.last_ms()
        tot, fwd = sd.detector.last_timing()
        g_ms.append(g); m_ms.append(m); d_ms.append(tot); f_ms.append(fwd)
        cand.append(np.mean([sum(len(d) for d in t) for t in sd.last_tiles]))
        merged.append(np.mean([len(d) for d in dets]))
    res["device_ms"] = {"slice_gather": float(np.median(g_ms)), "slice_merge": float(np.median(m_ms)), "detector_pass": float(np.median(d_ms)),
                        "detector_forward": float(np.median(f_ms)), "slice_gather_minmax": [float(min(g_ms)), float(max(g_ms))],
                        "slice_merge_minmax": [float(min(m_ms)), float(max(m_ms))], "detector_pass_minmax": [float(min(d_ms)), float(max(d_ms))]}
    res["candidates_per_frame"] = float(np.mean(cand))
    res["merged_per_frame"] = float(np.mean(merged))

    # ---- the merge kernel alone at 100 candidates per image: the last batch's boxes, every slot of every image taken
    rng = np.random.default_rng(3)
    xy = rng.uniform(0, TILE - 80, (n * I, max_det, 2)).astype(np.float32)
    xy = np.concatenate([xy, xy + rng.uniform(8, 80, (n * I, max_det, 2)).astype(np.float32)], axis=2)
    cf = rng.uniform(0.05, 0.95, (n * I, max_det)).astype(np.float32)
    cl = rng.integers(0, 8, (n * I, max_det)).astype(np.int32)
    cnt = np.full(n * I, max_det, np.int32)
    full = []
    for k in range(3 + 10):
        out, ms = S.slice_merge(sd._cfg, xy, cf, cl, cnt, want_ms=True)
        if k >= 3:
            full.append(ms)
    res["device_ms"]["slice_merge_full"] = float(np.median(full))
    res["merged_per_frame_full"] = float(np.mean([len(o[1]) for o in out]))

    # ---- end to end, two batches in flight
    def rate(enqueue, fetch):
        for _ in range(a.warmup):
            enqueue(); fetch()
        enqueue()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            enqueue()
            fetch()
        dt = time.perf_counter() - t0
        fetch()
        return n * a.steps / dt

    sliced_fps = rate(lambda: sd.enqueue(ptrs), sd.fetch)
    plain = pkg.Detector(path, input_size=(TILE, TILE), confidence=a.conf, max_det=max_det, batch=n, autotune=tune, warmup=False)
    plain_fps = rate(lambda: plain.enqueue(ptrs, height=H, width=W), plain.fetch)
    sliced_fps2 = rate(lambda: sd.enqueue(ptrs), sd.fetch)             # again, after the other: the spread of the same measurement
    res["frames_per_s"] = {"sliced": float(sliced_fps), "sliced_again": float(sliced_fps2), "unsliced": float(plain_fps),
                           "unsliced_over_sliced": float(plain_fps / sliced_fps)}
    nbytes = frames.nbytes + n * I * TILE * TILE * 3
    tiles, _ = sd.grid()
    res["gather_bytes_once"] = int(nbytes)
    res["gather_floor_us"] = {"measured_hbm": nbytes / (HBM_MEASURED_TBS * 1e12) * 1e6, "spec_hbm": nbytes / (HBM_SPEC_TBS * 1e12) * 1e6}
    plain.close(); sd.close(); buf.free()

    d = res["device_ms"]
    gshare, mshare = d["slice_gather"] / d["detector_pass"], d["slice_merge"] / d["detector_pass"]
    res["share_of_detector_pass"] = {"slice_gather": gshare, "slice_merge": mshare, "slice_merge_full": d["slice_merge_full"] / d["detector_pass"]}
    seen = [k for k, v in (("`slice_gather`", gshare), ("`slice_merge`", mshare)) if v >= 0.05]
    verdict = ("neither new kernel reaches 5 % of the detector's pass." if not seen else
               " and ".join(seen) + (" is" if len(seen) == 1 else " are") + " visible (5 % of the detector's pass or more).")
    res["verdict"] = verdict
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "slice_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(frames=n, images=n * I, conf=a.conf, max_det=max_det, match=a.match, repeat=a.repeat, warmup=a.warmup, steps=a.steps,
                                  gather_ms=d["slice_gather"], merge_ms=d["slice_merge"], merge_full_ms=d["slice_merge_full"], det_ms=d["detector_pass"],
                                  fwd_ms=d["detector_forward"], gather_share=gshare, merge_share=mshare,
                                  merge_full_share=d["slice_merge_full"] / d["detector_pass"], cand_mean=res["candidates_per_frame"],
                                  cand_full=I * max_det, gather_mb=nbytes / 1e6, gather_floor_us=res["gather_floor_us"]["measured_hbm"],
                                  gather_floor_spec_us=res["gather_floor_us"]["spec_hbm"], hbm=HBM_MEASURED_TBS,
                                  gather_x=d["slice_gather"] * 1e3 / res["gather_floor_us"]["measured_hbm"],
                                  reread=len(tiles) * TILE * TILE / (W * H), sliced_fps=sliced_fps, sliced_ips=sliced_fps * I, plain_fps=plain_fps,
                                  ratio=plain_fps / sliced_fps, inv_images=I, verdict=verdict, merged_mean=res["merged_per_frame"]))


if __name__ == "__main__":
    main()
