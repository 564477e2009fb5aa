"""Times rtmodt_amd.evaluation's array API on COCO-val-sized and MOT17-train-sized synthetic sets, in two parts:
host preparation (the Python marshalling before the C call) and the C call itself (host checks + upload + kernels +
download).  --ref also times the NumPy restatement (tests/eval_ref.py) on a 1/10 subset.  Prints one JSON line.

    python tools/eval_time.py [--repeat 3] [--ref] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rtmodt_amd  # noqa: E402

EV = rtmodt_amd.evaluation
_ffi = rtmodt_amd._ffi


def synth_coco(n_img=5000, n_cat=80, gt_per_img=7, dt_per_img=100, seed=0):
    rng = np.random.default_rng(seed)
    ng = rng.poisson(gt_per_img, n_img)
    gimg = np.repeat(np.arange(n_img), ng)
    G = len(gimg)
    gw, gh = rng.integers(4, 300, G).astype(np.float64), rng.integers(4, 300, G).astype(np.float64)
    gx, gy = rng.integers(0, 600, G).astype(np.float64), rng.integers(0, 400, G).astype(np.float64)
    gcat = rng.integers(1, n_cat + 1, G)
    gt = {"id": np.arange(1, G + 1), "image_id": gimg, "category_id": gcat, "bbox": np.stack([gx, gy, gw, gh], 1),
          "area": gw * gh * 0.8, "iscrowd": (rng.random(G) < 0.01).astype(np.int64)}
    D = n_img * dt_per_img
    dimg = np.repeat(np.arange(n_img), dt_per_img)
    src = rng.integers(0, max(G, 1), D)
    near = (rng.random(D) < 0.3) & (gimg[src] == dimg)                  # a third of the detections sit near a GT of their image
    jit = rng.normal(0, 6, (D, 4))
    box = np.where(near[:, None], gt["bbox"][src] + jit, np.stack([rng.uniform(0, 600, D), rng.uniform(0, 400, D),
                                                                  rng.uniform(4, 200, D), rng.uniform(4, 200, D)], 1))
    box[:, 2:] = np.maximum(box[:, 2:], 1.0)
    dcat = np.where(near, gcat[src], rng.integers(1, n_cat + 1, D))
    dt = {"image_id": dimg, "category_id": dcat, "bbox": box, "score": np.round(rng.random(D), 3)}
    return gt, dt, np.arange(n_img), np.arange(1, n_cat + 1)


def synth_mot(n_seq=7, frames_total=5300, per_frame=30, seed=0):
    rng = np.random.default_rng(seed)
    seqs = []
    for s in range(n_seq):
        F = frames_total // n_seq
        life = 120
        n_obj = per_frame * F // life
        gt, hyp = [], []
        hid_next = 1
        for o in range(n_obj):
            t0 = int(rng.integers(-life // 2, F)); t1 = min(F, t0 + life); t0 = max(0, t0)
            if t1 - t0 < 2:
                continue
            f = np.arange(t0, t1)
            x0, y0 = rng.uniform(0, 1800, 2); vx, vy = rng.uniform(-2, 2, 2); w, h = rng.uniform(20, 120, 2)
            b = np.stack([f + 1.0, np.full(len(f), o + 1.0), x0 + vx * f, y0 + vy * f, np.full(len(f), w), np.full(len(f), h)], 1)
            gt.append(b)
            keep = rng.random(len(f)) > 0.1
            hb = b[keep].copy()
            sw = np.cumsum(rng.random(len(hb)) < 0.01)
            hb[:, 1] = hid_next + sw
            hid_next += int(sw[-1]) + 1 if len(sw) else 1
            hb[:, 2:6] += rng.normal(0, 2.0, (len(hb), 4))
            hyp.append(hb)
        seqs.append((np.concatenate(gt), np.concatenate(hyp)))
    return seqs


class _Timed:
    """Wraps one C entry point of the library to time the call alone."""

    def __init__(self, name):
        self.L, self.name = _ffi.lib(), name
        self.fn = getattr(self.L, name)
        self.ms = []

    def __call__(self, *a):
        t = time.perf_counter()
        rc = self.fn(*a)
        self.ms.append((time.perf_counter() - t) * 1e3)
        return rc

    def __enter__(self):
        setattr(self.L, self.name, self)
        return self

    def __exit__(self, *exc):
        setattr(self.L, self.name, self.fn)


def run(fn, entry, repeat):
    tot = []
    with _Timed(entry) as t:
        for _ in range(repeat):
            s = time.perf_counter()
            out = fn()
            tot.append((time.perf_counter() - s) * 1e3)
    c = np.array(t.ms)
    return out, {"host_prep_ms": float(np.median(np.array(tot) - c)), "call_ms": float(np.median(c)), "total_ms": float(np.median(tot)),
                 "repeat": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--ref", action="store_true", help="also time the NumPy restatement on a 1/10 subset")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "tools/eval_time.py"}
    gt, dt, img, cat = synth_coco()
    res["coco_set"] = {"images": len(img), "categories": len(cat), "gts": len(gt["id"]), "dets": len(dt["score"]), "T": 10}
    out, res["coco"] = run(lambda: EV.coco_eval(gt, dt, img_ids=img, cat_ids=cat), "rtmodt_coco_eval", a.repeat)
    res["coco"]["stats0"] = float(out["stats"][0])
    seqs = synth_mot()
    res["mot_set"] = {"sequences": len(seqs), "frames": int(sum(len(np.union1d(g[:, 0], h[:, 0])) for g, h in seqs)),
                      "gt_rows": int(sum(len(g) for g, _ in seqs)), "hyp_rows": int(sum(len(h) for _, h in seqs))}
    out, res["mot"] = run(lambda: EV.mot_eval(seqs), "rtmodt_mot_eval", a.repeat)
    res["mot"]["mota0"] = out[0]["mota"]
    if a.ref:
        import eval_ref as ER
        gs, ds, im, ct = synth_coco(n_img=500, seed=1)
        t = time.perf_counter()
        ER.coco_ref(gs, ds, im, ct)
        res["ref_coco_subset"] = {"images": 500, "ms": (time.perf_counter() - t) * 1e3}
        t = time.perf_counter()
        for g, h in synth_mot(n_seq=1, frames_total=530, seed=1):
            ER.mot_ref(g, h)
        res["ref_mot_subset"] = {"frames": 530, "ms": (time.perf_counter() - t) * 1e3}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
