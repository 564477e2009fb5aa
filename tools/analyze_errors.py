"""What the detector gets wrong: types every detection and ground truth of a COCO ground-truth file and a COCO results file on the
GPU (rtmodt_amd.evaluation.analyze_detection_errors; the rules are INTEGRATION.md section 14) and writes

    DIR/errors.json            parameters, the histograms, the per-row types
    DIR/confusion_matrix.csv   rows ground truth, columns prediction, the last row / column background
    DIR/by_cell.csv            one line per grid cell: iy, ix and the seven counts

and prints the error table and the confusion matrix.  This is the tool the reference's design document calls in D.6 step 4
(tools/plot_confusion_matrix.py --gt annotations.json --pred predictions.json) and never ships; the output is text, no plotting
library is assumed.

    python tools/analyze_errors.py --gt annotations.json --pred predictions.json --out DIR
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def category_names(gt_path, cat_ids):
    with open(gt_path) as f:
        cats = {int(c["id"]): str(c.get("name", c["id"])) for c in json.load(f).get("categories", [])}
    return [cats.get(int(c), str(int(c))) for c in cat_ids]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt", required=True)
    ap.add_argument("--pred", required=True)
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--conf-thr", type=float, default=0.25)
    ap.add_argument("--max-det", type=int, default=100)
    ap.add_argument("--iou-fg", type=float, default=0.5)
    ap.add_argument("--iou-bg", type=float, default=0.1)
    ap.add_argument("--cm-iou", type=float, default=0.45)
    ap.add_argument("--grid", type=int, nargs=2, default=(8, 8), metavar=("GX", "GY"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import rtmodt_amd
    from rtmodt_amd.evaluation import errors as E
    res = rtmodt_amd.evaluation.analyze_detection_errors(a.gt, a.pred, conf_thr=a.conf_thr, max_det=a.max_det, iou_fg=a.iou_fg, iou_bg=a.iou_bg,
                                                         cm_iou=a.cm_iou, grid=tuple(a.grid), device=a.device)
    names = category_names(a.gt, res["cat_ids"])
    os.makedirs(a.out, exist_ok=True)
    doc = {"parity": "unpinned: neither tidecv nor ultralytics is installed where this runs; the rules are INTEGRATION.md section 14",
           "params": {**res["params"], "grid": list(res["params"]["grid"])}, "columns": list(E.ERROR_COLUMNS), "dt_type_names": list(E.DT_TYPE_NAMES),
           "gt_state_names": list(E.GT_STATE_NAMES), "cat_ids": res["cat_ids"].tolist(), "cat_names": names, "img_ids": res["img_ids"].tolist()}
    for k in ("by_class", "by_size", "by_cell", "missed_uncovered", "cm", "cm_dropped", "dt_type", "dt_gt", "gt_state", "gt_dt"):
        doc[k] = res[k].tolist()
    with open(os.path.join(a.out, "errors.json"), "w") as f:
        json.dump(doc, f)
        f.write("\n")
    with open(os.path.join(a.out, "confusion_matrix.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["gt \\ pred"] + names + ["background"])
        for name, row in zip(names + ["background"], res["cm"].tolist()):
            w.writerow([name] + row)
    with open(os.path.join(a.out, "by_cell.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["iy", "ix"] + list(E.ERROR_COLUMNS))
        for iy, line in enumerate(res["by_cell"].tolist()):
            for ix, counts in enumerate(line):
                w.writerow([iy, ix] + counts)
    sys.stdout.write(E.format_error_table(res, names) + "\n" + E.format_confusion_matrix(res["cm"], names))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
