"""Times track stitching (rtmodt_amd.evaluation.stitch_tracks, csrc/stitch.hip) on a batch shaped like the evaluator's own
timing workload (tools/eval_time.py: synth_mot): tens of sequences, thousands of tracklets each.  Host-timed medians of 5 for
the C call (host checks + sort + upload + kernels + download) and for the whole Python call; beside them, in the same run,
`mot_eval` on the same rows and the plain-Python restatement (tests/stitch_ref.py) on one sequence.  Nothing is asserted: the
numbers are reported, not gated.

    python tools/stitch_time.py [--repeat 5] [--sequences 24] [--out profiles/stitch/stitch_time.json]
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


def synth(n_seq, frames=3000, per_frame=30, life=120, seed=0):
    """(gt, hyp) per sequence: objects on linear paths; a hypothesis loses a tenth of its rows and changes its id with
    probability 0.03 a row, so an object comes as about four tracklets with gaps of a frame or more between them."""
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(n_seq):
        gt, hyp, hid = [], [], 1
        for o in range(per_frame * frames // life):
            t0 = int(rng.integers(-life // 2, frames)); t1 = min(frames, t0 + life); t0 = max(0, t0)
            if t1 - t0 < 2:
                continue
            f = np.arange(t0, t1)
            x0, y0 = rng.uniform(0, 1800, 2); vx, vy = rng.uniform(-2, 2, 2); w, h = rng.uniform(20, 120, 2)
            b = np.stack([f + 1.0, np.full(len(f), o + 1.0), x0 + vx * f, y0 + vy * f, np.full(len(f), w), np.full(len(f), h)], 1)
            gt.append(b)
            hb = b[rng.random(len(f)) > 0.1].copy()
            if len(hb) == 0:
                continue
            sw = np.cumsum(rng.random(len(hb)) < 0.03)
            hb[:, 1] = hid + sw
            hid += int(sw[-1]) + 1
            hb[:, 2:4] += rng.normal(0, 1.0, (len(hb), 2))
            hyp.append(hb)
        seqs.append((np.concatenate(gt), np.concatenate(hyp)))
    return seqs


def median_ms(fn, repeat):
    ms, out = [], None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return out, float(np.median(ms)), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=24)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rtmodt_amd
    from tools.eval_time import _Timed
    import stitch_ref as SR
    EV = rtmodt_amd.evaluation
    seqs = synth(a.sequences, a.frames)
    hyps = [h for _, h in seqs]
    res = {"tool": "tools/stitch_time.py", "repeat": a.repeat,
           "load": {"sequences": len(seqs), "frames_per_sequence": a.frames, "hyp_rows": int(sum(len(h) for h in hyps)),
                    "gt_rows": int(sum(len(g) for g, _ in seqs)), "tracklets": int(sum(len(np.unique(h[:, 1])) for h in hyps)),
                    "params": {"max_gap": 30, "max_dist": 20.0, "velocity_window": 3, "interpolate": True}}}
    kw = dict(max_gap=30, max_dist=20.0, velocity_window=3, interpolate=True)
    EV.stitch_tracks(hyps[:1], **kw)                                     # library load, first-launch costs
    with _Timed("rtmodt_stitch_tracks") as t:
        recs, total, totals = median_ms(lambda: EV.stitch_tracks(hyps, **kw), a.repeat)
    res["stitch"] = {"c_call_ms_median": float(np.median(t.ms)), "c_call_ms": [round(m, 3) for m in t.ms], "python_call_ms_median": total,
                     "python_call_ms": totals, "links": int(sum(len(r["links"]) for r in recs)),
                     "tracks_after": int(sum(r["n_tracks_after"] for r in recs)), "fill_rows": int(sum(len(r["fill"]) for r in recs))}
    with _Timed("rtmodt_mot_eval") as t:
        before, total, totals = median_ms(lambda: EV.mot_eval(seqs), a.repeat)
    res["mot_eval_same_rows"] = {"c_call_ms_median": float(np.median(t.ms)), "python_call_ms_median": total, "python_call_ms": totals}
    after = EV.mot_eval([(g, r["rows"]) for (g, _), r in zip(seqs, recs)])
    agg = lambda rs, k: int(sum(r[k] for r in rs))                        # noqa: E731
    for name, rs in (("before", before), ("after", after)):
        res["idf1_" + name] = 2 * agg(rs, "idtp") / (agg(rs, "num_objects") + agg(rs, "num_predictions"))
        res["switches_" + name] = agg(rs, "num_switches")
    t0 = time.perf_counter()
    ref = SR.stitch(hyps[0], 30, 20.0, 3, True)
    res["restatement_one_sequence"] = {"ms": (time.perf_counter() - t0) * 1e3, "tracklets": ref["n_tracks_before"],
                                       "same_link_count_as_gpu": len(ref["links"]) == len(recs[0]["links"])}
    line = json.dumps(res, indent=1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
