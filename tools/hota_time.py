"""Times rtmodt_amd.evaluation.hota_eval beside mot_eval on the same rows in the same run: the MOT17-train-sized synthetic
set of tools/eval_time.py.  Host-timed medians of 5 (after one warm-up call each) for the C call alone and for the whole Python
call with its NumPy marshalling.  Writes hota_time.json and README.md into --out-dir and prints the JSON line.

    python tools/hota_time.py [--repeat 5] [--out-dir profiles/hota]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import rtmodt_amd  # noqa: E402
from eval_time import _Timed, synth_mot  # noqa: E402

EV = rtmodt_amd.evaluation

README = """# HOTA: timings (`tools/hota_time.py`)

What is measured: `hota_eval` and `mot_eval` on the same rows in the same process on the same MI355X: the evaluator's own
timing workload (`tools/eval_time.py`), {sequences} sequences, {frames} frames, {gt_rows:,} ground-truth and {hyp_rows:,} hypothesis
rows.  `hota_eval` stores every pair with IoU > 0 ({tp0:,} matches count at the first alpha), `mot_eval` the pairs with IoU >= 0.5.

How: a host clock around the synchronous call, median of {repeat} after one warm-up call; the C call is timed alone by wrapping the
entry point (argument checks, uploads, kernels, the host finish, downloads), the Python call around it adds the NumPy marshalling
and the records.  No profiler was attached and no time was fixed in advance: the number to read HOTA's against is `mot_eval`'s
from the same run.  Nothing is gated on these numbers.

    python tools/hota_time.py --out-dir profiles/hota

## Figures (`hota_time.json`)

| call, {sequences} sequences | C call | whole Python call |
|---|---|---|
| `hota_eval` (19 alphas) | {hota_call:.1f} ms | {hota_total:.0f} ms |
| `mot_eval` on the same rows | {mot_call:.1f} ms | {mot_total:.0f} ms |

The {repeat} C calls of `hota_eval` took {hota_calls} ms, those of `mot_eval` {mot_calls} ms.  On this workload HOTA is {hota:.4f}
(DetA {deta:.4f}, AssA {assa:.4f}, LocA {loca:.4f}, means over alpha, all sequences combined) beside MOTA {mota:.4f} and IDF1 {idf1:.4f}
of the first sequence.  Per-kernel device times were not taken (no profiler run): not measured.

PARITY UNPINNED: TrackEval is installed nowhere this ran; the values are the restated rules' (INTEGRATION.md section 17).
"""


def timed(fn, entry, repeat):
    """-> (the last result, medians of the C call alone and of the whole Python call, every C call's time)."""
    tot = []
    with _Timed(entry) as t:
        for _ in range(repeat):
            s = time.perf_counter()
            out = fn()
            tot.append((time.perf_counter() - s) * 1e3)
    return out, {"call_ms": float(np.median(t.ms)), "total_ms": float(np.median(tot)), "repeat": repeat,
                 "call_ms_each": [round(x, 3) for x in t.ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    seqs = synth_mot()
    res = {"tool": "tools/hota_time.py",
           "set": {"sequences": len(seqs), "frames": int(sum(len(np.union1d(g[:, 0], h[:, 0])) for g, h in seqs)),
                   "gt_rows": int(sum(len(g) for g, _ in seqs)), "hyp_rows": int(sum(len(h) for _, h in seqs))}}
    EV.hota_eval(seqs)                                         # warm-up: module load, LDS attribute, allocator
    EV.mot_eval(seqs)
    hota, res["hota"] = timed(lambda: EV.hota_eval(seqs), "rtmodt_hota_eval", a.repeat)
    mot, res["mot"] = timed(lambda: EV.mot_eval(seqs), "rtmodt_mot_eval", a.repeat)
    c = hota["combined"]
    res["hota"].update({k: c["mean"][k] for k in ("HOTA", "DetA", "AssA", "LocA")})
    res["hota"]["n_alpha"] = len(hota["alphas"])
    res["hota"]["tp_alpha0"] = int(c["HOTA_TP"][0])
    res["mot"].update({"mota0": mot[0]["mota"], "idf10": mot[0]["idf1"]})
    line = json.dumps(res)
    print(line)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "hota_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)       # noqa: E731
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(repeat=a.repeat, tp0=res["hota"]["tp_alpha0"],
                                  hota_call=res["hota"]["call_ms"], hota_total=res["hota"]["total_ms"], mot_call=res["mot"]["call_ms"],
                                  mot_total=res["mot"]["total_ms"], hota_calls=fmt(res["hota"]["call_ms_each"]),
                                  mot_calls=fmt(res["mot"]["call_ms_each"]), hota=c["mean"]["HOTA"], deta=c["mean"]["DetA"],
                                  assa=c["mean"]["AssA"], loca=c["mean"]["LocA"], mota=mot[0]["mota"], idf1=mot[0]["idf1"], **res["set"]))


if __name__ == "__main__":
    main()
