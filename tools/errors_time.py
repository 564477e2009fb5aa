"""Times rtmodt_amd.evaluation.detection_errors on a COCO-val-shaped synthetic set (tools/eval_time.py's: 5 000 images, 80 categories,
about 7 GTs and 100 results per image, of which those at or above conf_thr are kept), beside coco_eval on the same arrays (existing
code, the yardstick) and the NumPy restatement (tests/errors_ref.py) on a 100-image slice.  As in tools/eval_time.py every figure is
split into host preparation (the Python marshalling before the C call) and the C call itself (host checks + upload + the kernel +
download); the synchronous call is timed on the host, median of --repeat calls after one untimed call.  Nothing is asserted: the
numbers are reported, not gated.  Prints one JSON line.

    python tools/errors_time.py [--repeat 5] [--out profiles/errors/errors_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from eval_time import EV, run, synth_coco  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gt, dt, img, cat = synth_coco()
    wh = np.tile([640.0, 480.0], (len(img), 1))
    res = {"tool": "tools/errors_time.py",
           "set": {"images": len(img), "categories": len(cat), "gts": len(gt["area"]), "results": len(dt["score"]),
                   "kept_at_conf_0.25": int((dt["score"] >= 0.25).sum())}}
    errors = lambda: EV.detection_errors(gt, dt, img_wh=wh, img_ids=img, cat_ids=cat)            # noqa: E731
    coco = lambda: EV.coco_eval(gt, dt, img_ids=img, cat_ids=cat)                               # noqa: E731
    errors(); coco()                                                                             # untimed: module load, LDS attribute, first allocations
    out, res["detection_errors"] = run(errors, "rtmodt_detection_errors", a.repeat)
    res["detection_errors"]["columns_total"] = out["by_class"].sum(axis=0).tolist()
    _, res["coco_eval_T10"] = run(coco, "rtmodt_coco_eval", a.repeat)
    res["call_ratio_errors_over_coco_eval"] = res["detection_errors"]["call_ms"] / res["coco_eval_T10"]["call_ms"]
    if a.ref_images:
        import errors_ref as XR
        n = a.ref_images
        gs = {k: v[gt["image_id"] < n] for k, v in gt.items()}
        ds = {k: v[dt["image_id"] < n] for k, v in dt.items()}
        whd = {int(i): (640.0, 480.0) for i in img[:n]}
        t = time.perf_counter()
        ref = XR.errors_ref(gs, ds, whd, img[:n], cat)
        res["numpy_restatement_slice"] = {"images": n, "ms": (time.perf_counter() - t) * 1e3}
        got = EV.detection_errors(gs, ds, img_wh=whd, img_ids=img[:n], cat_ids=cat)
        res["numpy_restatement_slice"]["equal"] = bool(all(np.array_equal(got[k], ref[k]) for k in XR.OUTPUTS))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
