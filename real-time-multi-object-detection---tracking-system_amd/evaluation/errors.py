"""Detection error analysis on the GPU: what the detector gets wrong.

The reference's design document defines five error types (localization, classification, duplicate, background false positive,
missed; TECHNICAL_DESIGN_DOCUMENT.md D.5), wants them clustered by image region and object size, and plots a confusion matrix
from a GT and a predictions file (D.6 step 4) with a tool that does not exist; its code has only ``build_confusion_matrix`` on
label pairs that nothing produces.  ``detection_errors`` types every detection and every ground truth of an image set in one
launch of ``csrc/errors.hip`` (``rtmodt_detection_errors``) and returns the per-row types, the three histograms and the
confusion matrix.

PARITY UNPINNED: neither tidecv (TIDE) nor ultralytics is installed anywhere this runs.  INTEGRATION.md section 14 states the
rules and how they differ from both; tests/errors_ref.py restates them in NumPy loops.
"""
from __future__ import annotations

import json

import numpy as np

from .. import _ffi
from .metrics import load_coco

# detection types; 0..5 are the histogram columns as well, column 6 counts the missed ground truths
TP, LOCALIZATION, CLASSIFICATION, BOTH, DUPLICATE, BACKGROUND = range(6)
MISSED_COLUMN, IGNORED, NOT_EVALUATED = 6, 6, 7
ERROR_COLUMNS = ("TP", "LOCALIZATION", "CLASSIFICATION", "BOTH", "DUPLICATE", "BACKGROUND", "MISSED")
DT_TYPE_NAMES = ("TP", "LOCALIZATION", "CLASSIFICATION", "BOTH", "DUPLICATE", "BACKGROUND", "IGNORED", "NOT_EVALUATED")
# ground-truth states; GT_NOT_EVALUATED marks a row outside the evaluated images / categories (set here, not by the library)
GT_CROWD, GT_MATCHED, GT_MISSED_COVERED, GT_MISSED, GT_NOT_EVALUATED = range(5)
GT_STATE_NAMES = ("CROWD", "MATCHED", "MISSED_COVERED", "MISSED", "NOT_EVALUATED")
SIZE_NAMES = ("small", "medium", "large")


def _image_sizes(img_wh, img_ids_given, img_ids: np.ndarray) -> np.ndarray:
    """``img_wh`` -> float64 ``[I][2]`` in the order of the sorted ``img_ids``: a ``{image id: (w, h)}`` mapping, or an array with
    one row per entry of the caller's ``img_ids``."""
    if isinstance(img_wh, dict):
        missing = [int(i) for i in img_ids if int(i) not in img_wh]
        if missing:
            raise ValueError(f"img_wh lacks images {missing[:10]}")
        return np.ascontiguousarray([img_wh[int(i)] for i in img_ids], np.float64).reshape(-1, 2)
    if img_ids_given is None:
        raise ValueError("img_wh as an array needs img_ids (one row per image id); or pass a {image id: (w, h)} dict")
    given = np.asarray(img_ids_given, np.int64).reshape(-1)
    wh = np.asarray(img_wh, np.float64).reshape(-1, 2)
    if len(wh) != len(given) or len(np.unique(given)) != len(given):
        raise ValueError(f"img_wh has {len(wh)} rows for {len(given)} image ids (which must be distinct)")
    return np.ascontiguousarray(wh[np.argsort(given, kind="stable")])


def detection_errors(gt: dict, dt: dict, *, img_wh, img_ids=None, cat_ids=None, conf_thr=0.25, max_det=100, iou_fg=0.5, iou_bg=0.1,
                     cm_iou=0.45, grid=(8, 8), device="cuda:0") -> dict:
    """Types every detection and ground truth on the GPU.

    ``gt``: arrays ``image_id, category_id, bbox (x, y, w, h), area, iscrowd``; ``dt``: ``image_id, category_id, bbox, score``
    (file order), as ``coco_eval`` takes them.  ``img_wh``: ``{image id: (width, height)}``, or an array with one row per entry
    of ``img_ids``.  ``img_ids`` / ``cat_ids`` default to the GT's own, sorted; rows outside them take no part
    (``NOT_EVALUATED`` / ``GT_NOT_EVALUATED``).  Returns, in the caller's row order, ``dt_type``, ``dt_gt`` (GT row, -1 none),
    ``gt_state``, ``gt_dt`` (detection row, -1 none), and the int64 counts ``by_class[K, 7]``, ``by_size[3, 7]``,
    ``by_cell[gy, gx, 7]`` (columns ``ERROR_COLUMNS``), ``missed_uncovered[K]``, ``cm[K + 1, K + 1]`` (rows ground truth,
    columns prediction, index K background) and ``cm_dropped[K]``."""
    gimg = np.asarray(gt["image_id"], np.int64).reshape(-1)
    gcat = np.asarray(gt["category_id"], np.int64).reshape(-1)
    dimg = np.asarray(dt["image_id"], np.int64).reshape(-1)
    dcat = np.asarray(dt["category_id"], np.int64).reshape(-1)
    ids = np.unique(gimg) if img_ids is None else np.unique(np.asarray(img_ids, np.int64))
    cats = np.unique(gcat) if cat_ids is None else np.unique(np.asarray(cat_ids, np.int64))
    if len(cats) == 0:
        raise ValueError("detection_errors needs at least one category")
    wh = _image_sizes(img_wh, img_ids, ids)
    gx, gy = (int(v) for v in grid)
    K, I = len(cats), len(ids)
    gsel = np.nonzero(np.isin(gimg, ids) & np.isin(gcat, cats))[0]
    dsel = np.nonzero(np.isin(dimg, ids) & np.isin(dcat, cats))[0]
    gi = np.searchsorted(ids, gimg[gsel])
    di = np.searchsorted(ids, dimg[dsel])
    grow = gsel[np.argsort(gi, kind="stable")]             # the library's GT rows -> the caller's, file order inside an image
    drow = dsel[np.argsort(di, kind="stable")]
    edges = np.arange(I + 1)
    gt_start = np.searchsorted(np.sort(gi), edges, "left").astype(np.int32)
    dt_start = np.searchsorted(np.sort(di), edges, "left").astype(np.int32)
    c32 = lambda a: np.ascontiguousarray(a, np.int32)     # noqa: E731
    f64 = lambda a: np.ascontiguousarray(a, np.float64)   # noqa: E731
    g_cat = c32(np.searchsorted(cats, gcat[grow]))
    g_box = f64(np.asarray(gt["bbox"], np.float64).reshape(-1, 4)[grow])
    g_area = f64(np.asarray(gt["area"], np.float64).reshape(-1)[grow])
    g_crowd = c32(np.asarray(gt["iscrowd"]).reshape(-1)[grow] != 0)
    d_cat = c32(np.searchsorted(cats, dcat[drow]))
    d_box = f64(np.asarray(dt["bbox"], np.float64).reshape(-1, 4)[drow])
    d_sc = f64(np.asarray(dt["score"], np.float64).reshape(-1)[drow])
    o_type, o_dgt = np.empty(len(drow), np.int32), np.empty(len(drow), np.int32)
    o_state, o_gdt = np.empty(len(grow), np.int32), np.empty(len(grow), np.int32)
    by_class, by_size, by_cell = np.zeros((K, 7), np.int64), np.zeros((3, 7), np.int64), np.zeros((max(gy, 0), max(gx, 0), 7), np.int64)
    missed_unc, cm, cm_drop = np.zeros(K, np.int64), np.zeros((K + 1, K + 1), np.int64), np.zeros(K, np.int64)
    params = _ffi.ErrorParams(float(conf_thr), float(iou_fg), float(iou_bg), float(cm_iou), int(max_det), gx, gy, 0)
    P = _ffi.ptr
    import ctypes
    _ffi.check(_ffi.lib().rtmodt_detection_errors(_ffi.device_ordinal(device), ctypes.byref(params), K, I, P(wh), P(gt_start), P(g_cat), P(g_box),
                                                  P(g_area), P(g_crowd), P(dt_start), P(d_cat), P(d_box), P(d_sc), P(o_type), P(o_dgt),
                                                  P(o_state), P(o_gdt), P(by_class), P(by_size), P(by_cell), P(missed_unc), P(cm), P(cm_drop)))
    dt_type = np.full(len(dimg), NOT_EVALUATED, np.int32)
    dt_gt = np.full(len(dimg), -1, np.int32)
    gt_state = np.full(len(gimg), GT_NOT_EVALUATED, np.int32)
    gt_dt = np.full(len(gimg), -1, np.int32)
    dt_type[drow] = o_type
    dt_gt[drow] = np.where(o_dgt >= 0, grow[np.maximum(o_dgt, 0)] if len(grow) else -1, -1)
    gt_state[grow] = o_state
    gt_dt[grow] = np.where(o_gdt >= 0, drow[np.maximum(o_gdt, 0)] if len(drow) else -1, -1)
    return {"dt_type": dt_type, "dt_gt": dt_gt, "gt_state": gt_state, "gt_dt": gt_dt, "by_class": by_class, "by_size": by_size,
            "by_cell": by_cell, "missed_uncovered": missed_unc, "cm": cm, "cm_dropped": cm_drop, "img_ids": ids, "cat_ids": cats,
            "params": {"conf_thr": float(conf_thr), "max_det": int(max_det), "iou_fg": float(iou_fg), "iou_bg": float(iou_bg),
                       "cm_iou": float(cm_iou), "grid": (gx, gy)}}


def analyze_detection_errors(gt_coco_json: str, pred_coco_json: str, **kw) -> dict:
    """``detection_errors`` of a COCO ground-truth file and a COCO results file; the image sizes are the GT file's
    ``images[].width`` / ``height``."""
    gt, dt, img_ids, cat_ids = load_coco(gt_coco_json, pred_coco_json)
    with open(gt_coco_json) as f:
        images = json.load(f).get("images", [])
    try:
        wh = {int(im["id"]): (float(im["width"]), float(im["height"])) for im in images}
    except KeyError as e:
        raise ValueError(f"{gt_coco_json}: an image lacks {e}") from None
    return detection_errors(gt, dt, img_wh=wh, img_ids=img_ids, cat_ids=cat_ids, **kw)


def _table(header, rows) -> str:
    width = [max(len(str(r[c])) for r in [header] + rows) for c in range(len(header))]
    line = lambda r: "  ".join(str(v).ljust(width[c]) if c == 0 else str(v).rjust(width[c]) for c, v in enumerate(r)).rstrip()   # noqa: E731
    return "\n".join(line(r) for r in [header] + rows) + "\n"


def format_confusion_matrix(cm, names) -> str:
    """Plain text: rows ground truth, columns prediction, the last row / column background."""
    cm = np.asarray(cm)
    names = [str(n) for n in names] + ["background"]
    if cm.shape != (len(names), len(names)):
        raise ValueError(f"a {cm.shape} matrix for {len(names) - 1} names")
    return _table(["gt \\ pred"] + names, [[names[i]] + [int(v) for v in cm[i]] for i in range(len(names))])


def format_error_table(result: dict, names) -> str:
    """Plain text: the error counts per class with a total row, then per size, then how many of the missed were uncovered."""
    by_class, by_size = np.asarray(result["by_class"]), np.asarray(result["by_size"])
    names = [str(n) for n in names]
    if len(names) != len(by_class):
        raise ValueError(f"{len(by_class)} classes, {len(names)} names")
    rows = [[names[k]] + [int(v) for v in by_class[k]] for k in range(len(names))]
    rows.append(["all"] + [int(v) for v in by_class.sum(axis=0)])
    rows += [[SIZE_NAMES[s]] + [int(v) for v in by_size[s]] for s in range(3)]
    return _table(["class / size"] + list(ERROR_COLUMNS), rows) + f"missed and not covered by any detection: {int(np.sum(result['missed_uncovered']))}\n"
