"""NumPy restatement of the detection-error rules, written loop by loop as the rules read, for
the tests of ``rtmodt_amd.evaluation.detection_errors``.  Plain Python / NumPy only; slow by design.  The IoU is
``eval_ref.iou_rows`` (the COCO one: the union of a crowd GT is the detection's area).
"""
from __future__ import annotations

import math

import numpy as np

from eval_ref import iou_rows

# detection types (0..5 are histogram columns as well), histogram column 6, GT states
TP, LOCALIZATION, CLASSIFICATION, BOTH, DUPLICATE, BACKGROUND = range(6)
MISSED_COL, IGNORED, NOT_EVALUATED = 6, 6, 7
GT_CROWD, GT_MATCHED, GT_MISSED_COVERED, GT_MISSED, GT_NOT_EVALUATED = 0, 1, 2, 3, 4


def size_bin(area):
    return 0 if area < 32 ** 2 else (1 if area < 96 ** 2 else 2)


def cell_index(x, w, n, W):
    """clamp((int)floor(((x + 0.5 * w) * n) / W), 0, n - 1) in float64, the operations in the order written."""
    f = math.floor((np.float64(x) + np.float64(0.5) * np.float64(w)) * np.float64(n) / np.float64(W))
    return int(min(max(f, 0), n - 1))


def first_max(values, members):
    """(maximum of values over members, the first member attaining it); (0.0, -1) for an empty set."""
    best, at = 0.0, -1
    for g in members:
        if at < 0 or values[g] > best:
            best, at = values[g], g
    return best, at


def errors_ref(gt, dt, img_wh, img_ids=None, cat_ids=None, conf_thr=0.25, max_det=100, iou_fg=0.5, iou_bg=0.1, cm_iou=0.45, grid=(8, 8)):
    """Arrays in ``detection_errors``'s form -> the same dict.  ``img_wh``: ``{image id: (width, height)}``."""
    gimg, gcat = np.asarray(gt["image_id"]).reshape(-1), np.asarray(gt["category_id"]).reshape(-1)
    dimg, dcat = np.asarray(dt["image_id"]).reshape(-1), np.asarray(dt["category_id"]).reshape(-1)
    gbox = np.asarray(gt["bbox"], np.float64).reshape(-1, 4)
    garea = np.asarray(gt["area"], np.float64).reshape(-1)
    gcrowd = np.asarray(gt["iscrowd"]).reshape(-1) != 0
    dbox = np.asarray(dt["bbox"], np.float64).reshape(-1, 4)
    dscore = np.asarray(dt["score"], np.float64).reshape(-1) + 0.0           # -0.0 -> 0.0
    imgs = np.unique(gimg if img_ids is None else np.asarray(img_ids))
    cats = np.unique(gcat if cat_ids is None else np.asarray(cat_ids))
    cat_index = {int(c): k for k, c in enumerate(cats)}
    K = len(cats)
    gx, gy = grid
    fg, bg, cmt = (min(t, 1 - 1e-10) for t in (iou_fg, iou_bg, cm_iou))
    dt_type = np.full(len(dimg), NOT_EVALUATED, np.int32)
    dt_gt = np.full(len(dimg), -1, np.int32)
    gt_state = np.full(len(gimg), GT_NOT_EVALUATED, np.int32)
    gt_dt = np.full(len(gimg), -1, np.int32)
    by_class = np.zeros((K, 7), np.int64)
    by_size = np.zeros((3, 7), np.int64)
    by_cell = np.zeros((gy, gx, 7), np.int64)
    missed_uncovered = np.zeros(K, np.int64)
    cm = np.zeros((K + 1, K + 1), np.int64)
    cm_dropped = np.zeros(K, np.int64)

    def count(col, k, area, box, W, H):
        by_class[k, col] += 1
        by_size[size_bin(area), col] += 1
        by_cell[cell_index(box[1], box[3], gy, H), cell_index(box[0], box[2], gx, W), col] += 1

    for im in imgs:
        W, H = img_wh[int(im)]
        grow = np.nonzero((gimg == im) & np.isin(gcat, cats))[0].tolist()      # file order
        drow = np.nonzero((dimg == im) & np.isin(dcat, cats))[0].tolist()
        gk = [cat_index[int(gcat[i])] for i in grow]
        # ---- kept detections: score >= conf_thr, ranked by (-score, file index), the first max_det ----
        elig = [i for i in drow if dscore[i] >= conf_thr]
        kept = sorted(elig, key=lambda i: (-dscore[i], i))[:max_det]
        dk = [cat_index[int(dcat[i])] for i in kept]
        crowd = [bool(gcrowd[i]) for i in grow]
        iou = iou_rows(dbox[kept], gbox[grow], crowd).reshape(len(kept), len(grow))    # crowd columns in the crowd form
        G, D = len(grow), len(kept)
        # ---- step 1: class-aware matching in rank order ----
        matched_by = [-1] * G
        types, points = [None] * D, [-1] * D
        for r in range(D):
            cand = [g for g in range(G) if gk[g] == dk[r] and iou[r, g] >= fg and (crowd[g] or matched_by[g] < 0)]
            pick = -1
            for group in ([g for g in cand if not crowd[g]], [g for g in cand if crowd[g]]):
                if group:
                    best = max(iou[r, g] for g in group)
                    pick = [g for g in group if iou[r, g] == best][-1]           # the last GT on equal IoU
                    break
            if pick >= 0:
                points[r] = pick
                if crowd[pick]:
                    types[r] = IGNORED
                else:
                    types[r] = TP
                    matched_by[pick] = r
        # ---- step 2: every unmatched detection by itself ----
        for r in range(D):
            if types[r] is not None:
                continue
            s, s_at = first_max(iou[r], [g for g in range(G) if not crowd[g] and gk[g] == dk[r]])
            o, o_at = first_max(iou[r], [g for g in range(G) if not crowd[g] and gk[g] != dk[r]])
            if s >= fg:
                types[r], points[r] = DUPLICATE, s_at
            elif o >= fg:
                types[r], points[r] = CLASSIFICATION, o_at
            elif s >= bg:
                types[r], points[r] = LOCALIZATION, s_at
            elif o >= bg:
                types[r], points[r] = BOTH, o_at
            else:
                types[r], points[r] = BACKGROUND, -1
        # ---- step 3: GT states ----
        covered = {points[r] for r in range(D) if types[r] in (LOCALIZATION, CLASSIFICATION) and points[r] >= 0}
        for g in range(G):
            if crowd[g]:
                st = GT_CROWD
            elif matched_by[g] >= 0:
                st = GT_MATCHED
            else:
                st = GT_MISSED_COVERED if g in covered else GT_MISSED
            gt_state[grow[g]] = st
            gt_dt[grow[g]] = kept[matched_by[g]] if matched_by[g] >= 0 else -1
            if st in (GT_MISSED_COVERED, GT_MISSED):
                count(MISSED_COL, gk[g], garea[grow[g]], gbox[grow[g]], W, H)
                if st == GT_MISSED:
                    missed_uncovered[gk[g]] += 1
        for r in range(D):
            dt_type[kept[r]] = types[r]
            dt_gt[kept[r]] = grow[points[r]] if points[r] >= 0 else -1
            if types[r] <= BACKGROUND:
                b = dbox[kept[r]]
                count(types[r], dk[r], b[2] * b[3], b, W, H)
        # ---- confusion matrix: class-agnostic, one to one, pairs in the total order (IoU desc, rank asc, GT asc) ----
        pairs = [(-iou[r, g], r, g) for r in range(D) for g in range(G) if not crowd[g] and iou[r, g] >= cmt]
        pairs.sort()
        det_free, gt_free = [True] * D, [True] * G
        for _, r, g in pairs:
            if det_free[r] and gt_free[g]:
                det_free[r] = gt_free[g] = False
                cm[gk[g], dk[r]] += 1
        for g in range(G):
            if gt_free[g] and not crowd[g]:
                cm[gk[g], K] += 1
        for r in range(D):
            if det_free[r]:
                if any(crowd[g] and gk[g] == dk[r] and iou[r, g] >= cmt for g in range(G)):
                    cm_dropped[dk[r]] += 1
                else:
                    cm[K, dk[r]] += 1
    return {"dt_type": dt_type, "dt_gt": dt_gt, "gt_state": gt_state, "gt_dt": gt_dt, "by_class": by_class, "by_size": by_size,
            "by_cell": by_cell, "missed_uncovered": missed_uncovered, "cm": cm, "cm_dropped": cm_dropped}


OUTPUTS = ("dt_type", "dt_gt", "gt_state", "gt_dt", "by_class", "by_size", "by_cell", "missed_uncovered", "cm", "cm_dropped")
