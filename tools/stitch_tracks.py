#!/usr/bin/env python3
"""Stitch the fragmented tracks of a MOTChallenge file on the GPU.

    python tools/stitch_tracks.py IN.txt OUT.txt [--gt GT.txt] [--max-gap 30] [--max-dist 20] [--velocity-window 0] [--interpolate]

IN.txt is read with ``load_mot``; OUT.txt is written in ``mot_rows``' line format (``frame,id,bb_left,bb_top,w,h,conf,-1,-1,-1``,
1-based corner, conf = 1).  With --gt, IDF1, ID switches and MOTA are printed before and after, from ``mot_eval``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_mot(path, rows):
    from rtmodt_amd.evaluation.metrics import _num
    with open(path, "w") as f:
        for r in rows:
            f.write(f"{int(r[0])},{int(r[1])},{_num(r[2] + 1.0)},{_num(r[3] + 1.0)},{_num(r[4])},{_num(r[5])},1,-1,-1,-1\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--gt", default=None, help="MOTChallenge ground truth: print IDF1 / ID switches / MOTA before and after")
    ap.add_argument("--max-gap", type=int, default=30)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--velocity-window", type=int, default=0)
    ap.add_argument("--interpolate", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    import rtmodt_amd  # noqa: F401
    EV = sys.modules["rtmodt_amd"].evaluation
    hyp = EV.load_mot(a.input)
    rec = EV.stitch_tracks([hyp], max_gap=a.max_gap, max_dist=a.max_dist, velocity_window=a.velocity_window, interpolate=a.interpolate,
                           device=a.device)[0]
    write_mot(a.output, rec["rows"])
    out = {"tracks_before": rec["n_tracks_before"], "tracks_after": rec["n_tracks_after"], "links": len(rec["links"]),
           "fill_rows": int(len(rec["fill"])), "rows_out": int(len(rec["rows"]))}
    if a.gt:
        gt = EV.load_mot(a.gt)
        before, after = EV.mot_eval([(gt, hyp), (gt, rec["rows"])], device=a.device)
        for name, r in (("before", before), ("after", after)):
            out[name] = {"idf1": r["idf1"], "num_switches": r["num_switches"], "mota": r["mota"], "idfp": r["idfp"], "idfn": r["idfn"]}
            print(f"{name:>6}: IDF1 {r['idf1']:.4f}  ID switches {r['num_switches']}  MOTA {r['mota']:.4f}")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
