"""Times the re-identification embedder (csrc/reid.hip) at 8 streams x 1080p x {10, 50, 100} boxes: kernel time (HIP events) of
the crop and of the network + quantiser, per call and per crop, beside two floors per crop -- the network's FLOPs at the fp16
matrix-core peak, and its compulsory bytes (the box's pixels in, 512 bytes out; the weights are shared by every crop) at the HBM
peak -- beside the bytes this implementation really moves (every tap and scratch tensor written once and read by its consumers),
and beside the colour-histogram descriptor of the same boxes on the same frames in the same run (profiles/deepsort/).
Nothing is asserted: the numbers are reported, not gated.  Writes one JSON document.

    python tools/reid_time.py [--repeat 10] [--out profiles/reid/reid_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import rtmodt_amd  # noqa: E402

_ffi = rtmodt_amd._ffi
HBM_BYTES_PER_S = 8.0e12                                    # MI355X data sheet: 8 TB/s
FP16_FLOPS = 2.5e15                                         # MI355X data sheet: 2.5 PFLOP/s dense fp16 on the matrix cores


def network_cost():
    """(MACs per crop, bytes of activations this implementation writes + reads per crop), from the layer table."""
    macs = 128 * 64 * 147 * 16
    moved = 256 * 128 * 3 * 2 + 128 * 64 * 16 * 2 * 2 + 64 * 32 * 16 * 2 * 2           # crop w + r, conv1 w + r, maxpool w + r
    for P, cin, mid, midp, cout, first in ((2048, 16, 16, 16, 64, 1), (2048, 64, 16, 16, 64, 0), (512, 64, 24, 32, 96, 1), (512, 96, 24, 32, 96, 0),
                                           (128, 96, 32, 32, 128, 1), (128, 128, 32, 32, 128, 0)):
        macs += P * (cin * mid + 10 * (mid * mid + 9 * mid) + mid * cout + (cin * cout if first else 0))
        m = P * midp * 2
        moved += P * cin * 2 * (2 if first else 1) + m                                  # input read by conv1 (+ downsample), x1 written
        moved += 10 * 4 * m + 4 * m                                                     # every LightConv: 1x1 r + w, depthwise r + w; x1 re-read per stream
        moved += 2 * 4 * m + m + m                                                      # gate: two passes over four maps, x2 written, read by conv3
        moved += P * cout * 2 * (3 if first else 2)                                     # [downsample w], residual r, output w
    for P, c in ((2048, 64), (512, 96)):
        macs += P * c * c
        moved += P * c * 2 * 3 + P * c * 2 // 4 * 2
    macs += 128 * 128 * 128 + 128 * 512
    moved += 128 * 128 * 2 * 3 + 512 * 4 * 2 + 512
    return macs, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reid", "reid_time.json"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="rtmodt_reid_")
    try:
        run(a, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run(a, tmp):
    S, h, w = a.streams, 1080, 1920
    RW = rtmodt_amd.reid_weights
    path = os.path.join(tmp, "osnet_synth.rtreid")
    RW.save(path, RW.synthetic(0))
    frames = rtmodt_amd.synth.structured_frames(S, h, w, 11)
    dev = [_ffi.DeviceBuffer(h * w * 3) for _ in range(S)]
    for d, f in zip(dev, frames):
        d.upload(np.ascontiguousarray(f))
    ptrs = [d.ptr for d in dev]
    core_cls = import_module(rtmodt_amd.__name__ + ".tracking.deepsort")._DeepSortCore
    macs, moved = network_cost()
    rows = []
    for n in (10, 50, 100):
        eng = rtmodt_amd.tracking.ReidEmbedder(path, max_boxes=n, max_frames=S)
        hist = core_cls(n_streams=S, max_tracks=256, max_dets=n)
        rng = np.random.default_rng(n)
        bw, bh = 80, 200                                                                # a pedestrian at 1080p
        x0, y0 = rng.uniform(0, w - bw, (S, n)), rng.uniform(0, h - bh, (S, n))
        xy = np.stack([x0, y0, x0 + bw, y0 + bh], -1).astype(np.float32)
        cnt = np.full(S, n, np.int32)
        conf, cls = np.full((S, n), 0.9, np.float32), np.zeros((S, n), np.int32)
        crop_ms, net_ms, hist_ms = [], [], []
        for t in range(a.repeat + 2):
            eng.embed(ptrs, xy, cnt, mem_kind=_ffi.MEM_DEVICE, height=h, width=w, stride=3 * w)
            hist.reset()
            hist.update_batch(xy, conf, cls, cnt, frames=ptrs, mem_kind=_ffi.MEM_DEVICE, height=h, width=w, stride=3 * w)
            if t >= 2:
                c, m = eng.last_ms()
                crop_ms.append(c); net_ms.append(m); hist_ms.append(hist.last_ms()[0])
        crops = S * n
        box_bytes = bw * bh * 3
        rows.append({
            "boxes_per_stream": n, "crops": crops,
            "measured_kernel_ms_median": {"crop": float(np.median(crop_ms)), "network_and_quantiser": float(np.median(net_ms))},
            "measured_kernel_ms_min": {"crop": float(np.min(crop_ms)), "network_and_quantiser": float(np.min(net_ms))},
            "measured_us_per_crop_median": float((np.median(crop_ms) + np.median(net_ms)) * 1e3 / crops),
            "measured_colorhist_descriptor_kernel_ms_median": float(np.median(hist_ms)),
            "measured_colorhist_us_per_box_median": float(np.median(hist_ms) * 1e3 / crops),
            "floor_flops_us_per_crop": 2.0 * macs / FP16_FLOPS * 1e6,
            "floor_compulsory_bytes_us_per_crop": (box_bytes + 512) / HBM_BYTES_PER_S * 1e6,
            "floor_bytes_this_implementation_moves_us_per_crop": moved / HBM_BYTES_PER_S * 1e6,
        })
        eng.close(); hist.close()
    out = {
        "load": {"streams": S, "frame": [h, w], "box": [80, 200], "repeat": a.repeat},
        "per_crop": {"macs": macs, "flops": 2 * macs, "compulsory_bytes": 80 * 200 * 3 + 512, "weight_bytes_shared_by_all_crops": os.path.getsize(path),
                     "activation_bytes_this_implementation_moves": moved},
        "runs": rows,
        "how": "HIP events around the crop kernel and around everything after it (rtmodt_reid_last_ms), frames already in HBM; the colour histogram is "
               "rtmodt_deepsort_last_ms's descriptor part on a colorhist tracker fed the same boxes on the same frames in the same process; floors assume "
               "2.5 PFLOP/s fp16 and 8 TB/s",
        "command": "python tools/reid_time.py --repeat %d" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
