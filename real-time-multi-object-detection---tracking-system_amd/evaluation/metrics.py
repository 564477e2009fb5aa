"""Offline evaluation on the GPU (reference: src/evaluation/metrics.py).

* ``evaluate_detection`` -- COCO bbox AP.  The reference calls pycocotools' ``COCOeval``; here ``evaluate`` and
  ``accumulate`` run in ``csrc/eval.hip`` (``rtmodt_coco_eval``) and ``summarize``'s 12 ``stats`` are built in NumPy.
* ``evaluate_tracking``  -- CLEAR MOT and IDF1.  The reference calls motmetrics; here ``rtmodt_mot_eval`` does the
  per-frame matching and the identity pairing.
* ``build_confusion_matrix`` / ``measure_tracking_drift`` -- the reference's NumPy helpers, unchanged in behaviour.
* ``coco_eval`` / ``mot_eval`` -- array-level entry points (custom IoU thresholds, many sequences per launch).
* ``hota_eval`` / ``evaluate_tracking_hota`` -- HOTA (TrackEval's hota.py) on ``mot_eval``'s input: ``rtmodt_hota_eval`` in
  ``csrc/hota.hip``, the final formulae in NumPy.
* ``coco_results`` / ``mot_rows`` -- write the project's detections / tracks in COCO results / MOTChallenge form.

PARITY UNPINNED: neither pycocotools nor motmetrics is installed anywhere this runs.  INTEGRATION.md section 9 states the
rules and the known divergences; tests/eval_ref.py restates them in NumPy.
"""
from __future__ import annotations

import json
import re

import numpy as np

from .. import _ffi

# the evaluation parameters: thresholds built on the host exactly as written, so that e.g.
# IOU_THRS[8] is 0.8999999999999999
IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
AREA_LBL = ("all", "small", "medium", "large")

# the 80 contiguous class ids of a COCO-trained detector -> COCO's 91-id category ids
COCO80_TO_91 = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34, 35, 36,
                37, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 70, 72,
                73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90)


# ---------------------------------------------------------------------------------------------------------------------
# COCO
# ---------------------------------------------------------------------------------------------------------------------
def load_coco(gt_coco_json: str, pred_coco_json: str):
    """The two files -> ``(gt, dt, img_ids, cat_ids)`` in ``coco_eval``'s array form (COCO() + loadRes() rules)."""
    with open(gt_coco_json) as f:
        g = json.load(f)
    with open(pred_coco_json) as f:
        r = json.load(f)
    img_ids = np.unique(np.array([im["id"] for im in g.get("images", [])], np.int64))
    cat_ids = np.unique(np.array([c["id"] for c in g.get("categories", [])], np.int64))
    anns = g.get("annotations", [])
    try:
        gt = {
            "id": np.array([a["id"] for a in anns], np.int64),
            "image_id": np.array([a["image_id"] for a in anns], np.int64),
            "category_id": np.array([a["category_id"] for a in anns], np.int64),
            "bbox": np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4),
            "area": np.array([a["area"] for a in anns], np.float64),
            "iscrowd": np.array([int(a.get("iscrowd", 0)) for a in anns], np.int32),    # missing -> 0 (pycocotools raises)
        }
    except KeyError as e:
        raise ValueError(f"{gt_coco_json}: an annotation lacks {e}") from None
    if not isinstance(r, list) or len(r) == 0:
        raise ValueError(f"{pred_coco_json}: the results list is empty")
    try:
        dt = {
            "image_id": np.array([d["image_id"] for d in r], np.int64),
            "category_id": np.array([d["category_id"] for d in r], np.int64),
            "bbox": np.array([d["bbox"] for d in r], np.float64).reshape(-1, 4),
            "score": np.array([d["score"] for d in r], np.float64),
        }
    except KeyError as e:
        raise ValueError(f"{pred_coco_json}: a result lacks {e}") from None
    return gt, dt, img_ids, cat_ids


def coco_eval(gt: dict, dt: dict, *, img_ids=None, cat_ids=None, iou_thrs=None, device="cuda:0") -> dict:
    """COCOeval(bbox).evaluate() + accumulate() on the GPU, summarize() in NumPy.

    ``gt``: arrays ``id, image_id, category_id, bbox (x, y, w, h), area, iscrowd``; ``dt``: ``image_id, category_id, bbox,
    score`` (file order).  ``img_ids`` / ``cat_ids`` default to the GT's own, sorted.  ``iou_thrs`` defaults to
    ``np.linspace(.5, .95, 10)``.  Returns ``precision[T, R, K, A, M]``, ``recall[T, K, A, M]``, ``stats[12]`` and the
    parameters used."""
    iou = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, np.float64).reshape(-1)
    gimg = np.asarray(gt["image_id"], np.int64).reshape(-1)
    gcat = np.asarray(gt["category_id"], np.int64).reshape(-1)
    img_ids = np.unique(gimg) if img_ids is None else np.unique(np.asarray(img_ids, np.int64))
    cat_ids = np.unique(gcat) if cat_ids is None else np.unique(np.asarray(cat_ids, np.int64))
    if len(cat_ids) == 0 or len(iou) == 0:
        raise ValueError("coco_eval needs at least one category and one IoU threshold")
    dimg = np.asarray(dt["image_id"], np.int64).reshape(-1)
    dcat = np.asarray(dt["category_id"], np.int64).reshape(-1)
    dbox = np.asarray(dt["bbox"], np.float64).reshape(-1, 4)
    dsc = np.asarray(dt["score"], np.float64).reshape(-1)
    if len(dimg) == 0:
        raise ValueError("the results list is empty")
    if not np.isin(dimg, img_ids).all():
        raise ValueError("results do not correspond to the ground truth: image ids "
                         f"{sorted(set(dimg[~np.isin(dimg, img_ids)].tolist()))[:10]} are not GT images")
    if np.isnan(dsc).any() or np.isnan(dbox).any():
        raise ValueError("a result has a NaN score or box")
    gbox = np.asarray(gt["bbox"], np.float64).reshape(-1, 4)
    garea = np.asarray(gt["area"], np.float64).reshape(-1)
    gcrowd = (np.asarray(gt["iscrowd"]).reshape(-1) != 0).astype(np.int32)
    gid = np.asarray(gt["id"], np.int64).reshape(-1)
    # GTs / results outside the evaluated images and categories take no part (getAnnIds(imgIds, catIds))
    gsel = np.isin(gimg, img_ids) & np.isin(gcat, cat_ids)
    dsel = np.isin(dcat, cat_ids)
    K, I = len(cat_ids), len(img_ids)
    gkey = np.searchsorted(cat_ids, gcat[gsel]) * I + np.searchsorted(img_ids, gimg[gsel])
    dkey = np.searchsorted(cat_ids, dcat[dsel]) * I + np.searchsorted(img_ids, dimg[dsel])
    go = np.argsort(gkey, kind="stable")
    do = np.argsort(dkey, kind="stable")
    gkey, dkey = gkey[go], dkey[do]
    cells = np.union1d(gkey, dkey)
    gt_start = np.searchsorted(gkey, cells, "left").astype(np.int32)
    gt_start = np.append(gt_start, len(gkey)).astype(np.int32)
    dt_start = np.append(np.searchsorted(dkey, cells, "left"), len(dkey)).astype(np.int32)
    cell_cat = (cells // I).astype(np.int32)
    g_box = np.ascontiguousarray(gbox[gsel][go])
    g_area = np.ascontiguousarray(garea[gsel][go])
    g_crowd = np.ascontiguousarray(gcrowd[gsel][go])
    g_id = np.ascontiguousarray(gid[gsel][go])
    d_box = np.ascontiguousarray(dbox[dsel][do])
    d_sc = np.ascontiguousarray(dsc[dsel][do]) + 0.0                      # -0.0 -> 0.0
    T, R, A, M = len(iou), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    iou_c = np.ascontiguousarray(iou)
    md = np.array(MAX_DETS, np.int32)
    prec = np.empty((T, R, K, A, M), np.float64)
    rec = np.empty((T, K, A, M), np.float64)
    P = _ffi.ptr
    _ffi.check(_ffi.lib().rtmodt_coco_eval(_ffi.device_ordinal(device), P(iou_c), T, P(REC_THRS), R, P(md), M, P(AREA_RNG), A, K,
                                           len(cells), P(cell_cat), P(gt_start), P(g_box), P(g_area), P(g_crowd), P(g_id), P(dt_start),
                                           P(d_box), P(d_sc), P(prec), P(rec)))
    return {"precision": prec, "recall": rec, "stats": coco_stats(prec, rec, iou), "iou_thrs": iou, "rec_thrs": REC_THRS,
            "max_dets": MAX_DETS, "area_rng": AREA_RNG, "img_ids": img_ids, "cat_ids": cat_ids}


def coco_stats(precision: np.ndarray, recall: np.ndarray, iou_thrs) -> np.ndarray:
    """COCOeval.summarize()'s 12 numbers: mean(s[s > -1]) over the selected slice, -1 when nothing qualifies."""
    iou = np.asarray(iou_thrs, np.float64)

    def summ(ap, thr=None, area="all", mdet=100):
        a = AREA_LBL.index(area)
        m = MAX_DETS.index(mdet)
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == iou)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        s = s[s > -1]
        return -1.0 if len(s) == 0 else float(np.mean(s))

    return np.array([summ(1), summ(1, .5), summ(1, .75), summ(1, area="small"), summ(1, area="medium"), summ(1, area="large"),
                     summ(0, mdet=1), summ(0, mdet=10), summ(0), summ(0, area="small"), summ(0, area="medium"),
                     summ(0, area="large")], np.float64)


def evaluate_detection(gt_coco_json: str, pred_coco_json: str, iou_thresh: float = 0.5, *, device="cuda:0") -> dict:
    """COCO bbox mAP at ``iou_thresh`` (the reference's mapping of ``stats``, quirks included: ``mAP``, ``mAP_50`` and
    ``precision`` are all ``stats[0]``, ``recall`` is ``stats[8]``)."""
    gt, dt, img_ids, cat_ids = load_coco(gt_coco_json, pred_coco_json)
    st = coco_eval(gt, dt, img_ids=img_ids, cat_ids=cat_ids, iou_thrs=[iou_thresh], device=device)["stats"]
    return {"mAP": float(st[0]), "mAP_50": float(st[0]), "precision": float(st[0]), "recall": float(st[8])}


def coco_results(image_id: int, detections, category_ids=COCO80_TO_91) -> list:
    """One frame's ``Detections`` -> COCO results entries: xyxy -> x, y, w, h (float64 of the float32 corners), class
    ``c`` -> ``category_ids[c]`` (default: the standard 80 -> 91 map)."""
    xy = np.asarray(detections.xyxy, np.float32).reshape(-1, 4).astype(np.float64)
    out = []
    for b, s, c in zip(xy, np.asarray(detections.confidence).reshape(-1), np.asarray(detections.class_id).reshape(-1)):
        out.append({"image_id": int(image_id), "category_id": int(category_ids[int(c)]),
                    "bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])], "score": float(s)})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# MOT
# ---------------------------------------------------------------------------------------------------------------------
_SEP = re.compile(r"[,\s]+")


def load_mot(path: str) -> np.ndarray:
    """A MOTChallenge file -> ``(n, 6)`` float64 rows ``frame, id, x, y, w, h`` with x, y moved to 0-based (minus 1),
    every row kept (motmetrics' ``loadtxt(fmt="mot15-2D")``).  A duplicate (frame, id) raises ``ValueError``."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            fields = [t for t in _SEP.split(line) if t]
            if len(fields) < 6:
                raise ValueError(f"{path}:{ln}: {len(fields)} fields, at least 6 needed (frame, id, x, y, w, h)")
            try:
                v = [float(t) for t in fields[:6]]
            except ValueError:
                raise ValueError(f"{path}:{ln}: not a number in {line!r}") from None
            rows.append(v)
    a = np.array(rows, np.float64).reshape(-1, 6)
    a[:, 2] -= 1.0
    a[:, 3] -= 1.0
    if len(a):
        key = a[:, :2]
        if len(np.unique(key, axis=0)) != len(key):
            raise ValueError(f"{path}: a (frame, id) pair occurs twice")
    return a


def _quiet_div(a, b) -> float:
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mot_arrays(seqs):
    """``(gt, hyp)`` pairs -> the CSR arrays ``rtmodt_mot_eval`` and ``rtmodt_hota_eval`` share (``seqs`` is not empty)."""
    fstart, fids, gstart, hstart = [0], [], [0], [0]
    goid, gbox, hhid, hbox, n_oid, n_hid = [], [], [], [], [], []
    for gt, hyp in seqs:
        gt = np.asarray(gt, np.float64).reshape(-1, 6)
        hyp = np.asarray(hyp, np.float64).reshape(-1, 6)
        for name, a in (("GT", gt), ("hypothesis", hyp)):
            if len(a) and len(np.unique(a[:, :2], axis=0)) != len(a):
                raise ValueError(f"{name} rows: a (frame, id) pair occurs twice")
        gt = gt[np.lexsort((gt[:, 1], gt[:, 0]))]
        hyp = hyp[np.lexsort((hyp[:, 1], hyp[:, 0]))]
        frames = np.union1d(gt[:, 0], hyp[:, 0])
        g_ids, g_inv = np.unique(gt[:, 1], return_inverse=True)
        h_ids, h_inv = np.unique(hyp[:, 1], return_inverse=True)
        gs = np.searchsorted(gt[:, 0], frames, "left")
        hs = np.searchsorted(hyp[:, 0], frames, "left")
        gstart.extend((gstart[-1] + np.append(gs[1:], len(gt))).tolist())
        hstart.extend((hstart[-1] + np.append(hs[1:], len(hyp))).tolist())
        fids.extend(frames.astype(np.int64).tolist())
        fstart.append(fstart[-1] + len(frames))
        goid.append(g_inv.reshape(-1)); gbox.append(gt[:, 2:6]); hhid.append(h_inv.reshape(-1)); hbox.append(hyp[:, 2:6])
        n_oid.append(len(g_ids)); n_hid.append(len(h_ids))
    i32 = lambda x: np.ascontiguousarray(np.asarray(x), np.int32)       # noqa: E731
    f64 = lambda x: np.ascontiguousarray(np.concatenate(x).reshape(-1, 4), np.float64)   # noqa: E731
    fstart, gstart, hstart = i32(fstart), i32(gstart), i32(hstart)
    fids = np.ascontiguousarray(fids, np.int64)
    goid, hhid = i32(np.concatenate(goid)), i32(np.concatenate(hhid))
    gbox, hbox = f64(gbox), f64(hbox)
    n_oid, n_hid = i32(n_oid), i32(n_hid)
    return fstart, fids, gstart, hstart, goid, gbox, hhid, hbox, n_oid, n_hid


def mot_eval(sequences, *, device="cuda:0") -> list:
    """CLEAR MOT + IDF1 of many sequences in one launch.  ``sequences``: ``(gt, hyp)`` pairs of ``(n, 6)`` arrays
    ``frame, id, x, y, w, h`` (0-based boxes, as ``load_mot`` returns them).  Returns one record per sequence: every
    count plus ``mota``, ``motp`` (1 - IoU) and ``idf1``."""
    seqs = list(sequences)
    if not seqs:
        return []
    fstart, fids, gstart, hstart, goid, gbox, hhid, hbox, n_oid, n_hid = _mot_arrays(seqs)
    out = (_ffi.MotCounts * len(seqs))()
    P = _ffi.ptr
    _ffi.check(_ffi.lib().rtmodt_mot_eval(_ffi.device_ordinal(device), len(seqs), P(fstart), P(fids), P(gstart), P(hstart), P(goid),
                                          P(gbox), P(hhid), P(hbox), P(n_oid), P(n_hid), out))
    recs = []
    for c in out:
        r = {n: int(getattr(c, n)) for n, _ in _ffi.MotCounts._fields_ if n != "dist_sum"}
        r["dist_sum"] = float(c.dist_sum)
        r["mota"] = 1.0 - _quiet_div(r["num_misses"] + r["num_switches"] + r["num_false_positives"], r["num_objects"])
        r["motp"] = _quiet_div(r["dist_sum"], r["num_matches"] + r["num_switches"])
        r["idf1"] = _quiet_div(2 * r["idtp"], r["num_objects"] + r["num_predictions"])
        recs.append(r)
    return recs


def evaluate_tracking(gt_mot_file: str, pred_mot_file: str, *, device="cuda:0") -> dict:
    """IDF1, MOTA, MOTP (1 - IoU), ID switches, mostly tracked / lost of one MOTChallenge sequence."""
    r = mot_eval([(load_mot(gt_mot_file), load_mot(pred_mot_file))], device=device)[0]
    return {"idf1": r["idf1"], "mota": r["mota"], "motp": r["motp"], "num_switches": r["num_switches"],
            "mostly_tracked": r["mostly_tracked"], "mostly_lost": r["mostly_lost"]}


# ---------------------------------------------------------------------------------------------------------------------
# HOTA (TrackEval's trackeval/metrics/hota.py)
# ---------------------------------------------------------------------------------------------------------------------
HOTA_ALPHAS = np.arange(0.05, 0.99, 0.05)                  # TrackEval's array_labels: 19 values, used as built
HOTA_FLOAT_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
HOTA_COUNT_FIELDS = ("HOTA_TP", "HOTA_FN", "HOTA_FP")
HOTA_SUM_FIELDS = ("loc_sum", "ass_a_sum", "ass_re_sum", "ass_pr_sum")


def hota_record(tp, fn, fp, loc_sum, ass_a_sum, ass_re_sum, ass_pr_sum, alphas=None, *, combined=False) -> dict:
    """The sums per alpha -> one HOTA record with TrackEval's formulae and guards.  Per alpha: the integer counts
    ``HOTA_TP / HOTA_FN / HOTA_FP``, the four sums, and ``DetRe = TP / max(1, TP + FN)``, ``DetPr = TP / max(1, TP + FP)``,
    ``DetA = TP / max(1, TP + FN + FP)``, ``AssA / AssRe / AssPr = sum / max(1, TP)``, ``HOTA = sqrt(DetA * AssA)``,
    ``LocA = max(1e-10, loc_sum) / max(1e-10, TP)`` (1 where nothing matched).  ``combined``: TrackEval's
    ``combine_sequences`` weights LocA by TP instead, ``loc_sum / max(1e-10, TP)`` (0 where nothing matched); every other
    field of a combination is the same formula on the added sums.  ``mean``: each float field's mean over alpha;
    ``HOTA(0)``, ``LocA(0)``, ``HOTALocA(0)``: the first alpha's values and their product."""
    tp, fn, fp = (np.asarray(v, np.int64).reshape(-1) for v in (tp, fn, fp))
    loc, aa, ar, ap = (np.asarray(v, np.float64).reshape(-1) for v in (loc_sum, ass_a_sum, ass_re_sum, ass_pr_sum))
    r = {"alphas": HOTA_ALPHAS.copy() if alphas is None else np.asarray(alphas, np.float64).reshape(-1).copy(),
         "HOTA_TP": tp, "HOTA_FN": fn, "HOTA_FP": fp, "loc_sum": loc, "ass_a_sum": aa, "ass_re_sum": ar, "ass_pr_sum": ap}
    tpf = tp.astype(np.float64)
    r["DetRe"] = tpf / np.maximum(1, tp + fn)
    r["DetPr"] = tpf / np.maximum(1, tp + fp)
    r["DetA"] = tpf / np.maximum(1, tp + fn + fp)
    r["AssA"] = aa / np.maximum(1, tp)
    r["AssRe"] = ar / np.maximum(1, tp)
    r["AssPr"] = ap / np.maximum(1, tp)
    r["HOTA"] = np.sqrt(r["DetA"] * r["AssA"])
    r["LocA"] = loc / np.maximum(1e-10, tpf) if combined else np.maximum(1e-10, loc) / np.maximum(1e-10, tpf)
    r["mean"] = {k: float(np.mean(r[k])) for k in HOTA_FLOAT_FIELDS}
    r["HOTA(0)"] = float(r["HOTA"][0])
    r["LocA(0)"] = float(r["LocA"][0])
    r["HOTALocA(0)"] = r["HOTA(0)"] * r["LocA(0)"]
    return r


def hota_combine(records, alphas=None) -> dict:
    """TrackEval's ``combine_sequences``: the counts summed and the association / localisation terms weighted by TP, which
    with the sums kept in every record is adding the sums."""
    records = list(records)
    n = len(HOTA_ALPHAS if alphas is None else np.asarray(alphas).reshape(-1))
    tot = {k: np.zeros(n, np.int64) for k in HOTA_COUNT_FIELDS}
    tot.update({k: np.zeros(n, np.float64) for k in HOTA_SUM_FIELDS})
    for r in records:
        for k in tot:
            tot[k] = tot[k] + r[k]
    return hota_record(tot["HOTA_TP"], tot["HOTA_FN"], tot["HOTA_FP"], tot["loc_sum"], tot["ass_a_sum"], tot["ass_re_sum"],
                       tot["ass_pr_sum"], alphas, combined=True)


def hota_eval(sequences, *, alphas=None, device="cuda:0") -> dict:
    """HOTA of many sequences in one call (``rtmodt_hota_eval``).  ``sequences``: ``mot_eval``'s input.  ``alphas``: an
    ascending array of at most 32 thresholds, default ``np.arange(0.05, 0.99, 0.05)``.  Returns ``{"sequences": [one record
    per sequence], "combined": the record of all of them, "alphas": the thresholds}``; a record is ``hota_record``'s.
    PARITY UNPINNED against TrackEval."""
    al = np.ascontiguousarray(HOTA_ALPHAS if alphas is None else np.asarray(alphas, np.float64).reshape(-1), np.float64)
    if len(al) == 0:
        raise ValueError("hota_eval needs at least one alpha")
    seqs = list(sequences)
    out = (_ffi.HotaCounts * (len(seqs) * len(al)))()
    P = _ffi.ptr
    if seqs:
        fstart, fids, gstart, hstart, goid, gbox, hhid, hbox, n_oid, n_hid = _mot_arrays(seqs)
        _ffi.check(_ffi.lib().rtmodt_hota_eval(_ffi.device_ordinal(device), len(seqs), P(fstart), P(fids), P(gstart), P(hstart), P(goid),
                                               P(gbox), P(hhid), P(hbox), P(n_oid), P(n_hid), P(al), len(al), out))
    else:
        _ffi.check(_ffi.lib().rtmodt_hota_eval(_ffi.device_ordinal(device), 0, None, None, None, None, None, None, None, None, None, None,
                                               P(al), len(al), out))
    recs = []
    for s in range(len(seqs)):
        c = out[s * len(al):(s + 1) * len(al)]
        recs.append(hota_record(*[[getattr(x, n) for x in c] for n, _ in _ffi.HotaCounts._fields_], al))
    return {"sequences": recs, "combined": hota_combine(recs, al), "alphas": al.copy()}


def evaluate_tracking_hota(gt_mot_file: str, pred_mot_file: str, *, device="cuda:0") -> dict:
    """The HOTA record of one MOTChallenge sequence (``hota_eval`` on the two files)."""
    return hota_eval([(load_mot(gt_mot_file), load_mot(pred_mot_file))], device=device)["sequences"][0]


def _num(v: float) -> str:
    v = float(v)
    return str(int(v)) if v.is_integer() and abs(v) < 2 ** 53 else repr(v)


def mot_rows(frame_id: int, tracks) -> list:
    """MOTChallenge lines ``frame,id,bb_left,bb_top,w,h,conf,-1,-1,-1`` for one frame's tracks (1-based corner:
    ``bb_left = x1 + 1``, so that a reader's minus 1 gives the track's box back)."""
    out = []
    for t in tracks:
        x1, y1, x2, y2 = (float(v) for v in np.asarray(t.xyxy, np.float32).reshape(4))
        out.append(f"{int(frame_id)},{int(t.track_id)},{_num(x1 + 1.0)},{_num(y1 + 1.0)},{_num(x2 - x1)},{_num(y2 - y1)},"
                   f"{_num(float(t.confidence))},-1,-1,-1")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# NumPy helpers (the reference's, same values)
# ---------------------------------------------------------------------------------------------------------------------
def build_confusion_matrix(gt_labels, pred_labels, num_classes: int) -> np.ndarray:
    """(num_classes x num_classes) int64 counts, rows = ground truth, columns = prediction; pairs with a label outside
    0..num_classes-1 are skipped, and the longer list is cut to the shorter (zip)."""
    cm = np.zeros((num_classes, num_classes), dtype=np.int64)
    n = min(len(gt_labels), len(pred_labels))
    g = np.asarray(list(gt_labels)[:n], dtype=np.int64).reshape(-1)
    p = np.asarray(list(pred_labels)[:n], dtype=np.int64).reshape(-1)
    ok = (g >= 0) & (g < num_classes) & (p >= 0) & (p < num_classes)
    np.add.at(cm, (g[ok], p[ok]), 1)
    return cm


def measure_tracking_drift(gt_centroids: dict, pred_centroids: dict) -> dict:
    """Per track id present in both dicts: the mean float32 Euclidean distance between its GT and predicted centroids,
    frame by frame over the shorter of the two trails.  ``mean_drift_px`` is the mean over all those distances (0.0 when
    there are none)."""
    ids = set(gt_centroids) & set(pred_centroids)
    dist = {}
    for tid in ids:
        a = np.asarray(gt_centroids[tid], np.float32).reshape(-1, 2)
        b = np.asarray(pred_centroids[tid], np.float32).reshape(-1, 2)
        k = min(len(a), len(b))
        dist[tid] = np.sqrt(((a[:k] - b[:k]) ** 2).sum(axis=1))
    allv = np.concatenate([v.astype(np.float64) for v in dist.values()]) if dist else np.empty(0)
    return {"mean_drift_px": float(allv.mean()) if allv.size else 0.0, "per_track": {t: float(v.mean()) for t, v in dist.items()}}
