"""The detection-error rules on hand-worked cases with literal expected values, through the NumPy
restatement (tests/errors_ref.py) -- so that the restatement does not certify itself -- plus what the library does without a GPU:
every argument check of rtmodt_detection_errors (they run before the first HIP call) and the two text formatters."""
import ctypes

import numpy as np
import pytest

import errors_ref as XR
from rtmodt_amd import _ffi
from rtmodt_amd import evaluation as EV

TP, LOC, CLS, BOTH, DUP, BKG, MISSED_COL, IGNORED, NOT_EVALUATED = 0, 1, 2, 3, 4, 5, 6, 6, 7
CROWD, MATCHED, MISSED_COVERED, MISSED = 0, 1, 2, 3
A = [0, 0, 10, 10]
FAR = [50, 50, 10, 10]
CATS = [1, 2]                                              # K = 2: cm is 3 x 3, index 2 is background
WH = (100.0, 100.0)

# name -> (gts, dts, parameters, expected).  gts: (category, [x, y, w, h], area, crowd); dts: (category, [x, y, w, h], score);
# one image of 100 x 100 each.  IoU of A with [0, 0, 10, h] is h / 10.  tests/test_gpu_errors.py runs every case on the GPU.
CASES = {
    "tp": ([(1, A, 100, 0)], [(1, A, .9)], {},
           dict(dt_type=[TP], dt_gt=[0], gt_state=[MATCHED], gt_dt=[0], by_class={(0, TP): 1}, missed_uncovered=[0, 0],
                cm=[[1, 0, 0], [0, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # IoU 0.3 with the GT of its own class: a localization error; the GT is missed but covered; 0.3 < cm_iou, so no cm pair
    "localization": ([(1, A, 100, 0)], [(1, [0, 0, 10, 3], .9)], {},
                     dict(dt_type=[LOC], dt_gt=[0], gt_state=[MISSED_COVERED], gt_dt=[-1], by_class={(0, LOC): 1, (0, MISSED_COL): 1},
                          missed_uncovered=[0, 0], cm=[[0, 0, 1], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    "classification": ([(1, A, 100, 0)], [(2, A, .9)], {},
                       dict(dt_type=[CLS], dt_gt=[0], gt_state=[MISSED_COVERED], gt_dt=[-1], by_class={(1, CLS): 1, (0, MISSED_COL): 1},
                            missed_uncovered=[0, 0], cm=[[0, 1, 0], [0, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # wrong class AND a poor box: BOTH does not cover the GT
    "both": ([(1, A, 100, 0)], [(2, [0, 0, 10, 3], .9)], {},
             dict(dt_type=[BOTH], dt_gt=[0], gt_state=[MISSED], gt_dt=[-1], by_class={(1, BOTH): 1, (0, MISSED_COL): 1},
                  missed_uncovered=[1, 0], cm=[[0, 0, 1], [0, 0, 0], [0, 1, 0]], cm_dropped=[0, 0])),
    "duplicate": ([(1, A, 100, 0)], [(1, A, .9), (1, [0, 0, 10, 8], .8)], {},
                  dict(dt_type=[TP, DUP], dt_gt=[0, 0], gt_state=[MATCHED], gt_dt=[0], by_class={(0, TP): 1, (0, DUP): 1},
                       missed_uncovered=[0, 0], cm=[[1, 0, 0], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    "background": ([(1, A, 100, 0)], [(1, FAR, .9)], {},
                   dict(dt_type=[BKG], dt_gt=[-1], gt_state=[MISSED], gt_dt=[-1], by_class={(0, BKG): 1, (0, MISSED_COL): 1},
                        missed_uncovered=[1, 0], cm=[[0, 0, 1], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    "missed": ([(2, A, 100, 0)], [], {},
               dict(dt_type=[], dt_gt=[], gt_state=[MISSED], gt_dt=[-1], by_class={(1, MISSED_COL): 1}, missed_uncovered=[0, 1],
                    cm=[[0, 0, 0], [0, 0, 1], [0, 0, 0]], cm_dropped=[0, 0])),
    # below conf_thr: the row takes no part at all
    "below_conf": ([], [(1, A, .2)], {},
                   dict(dt_type=[NOT_EVALUATED], dt_gt=[-1], gt_state=[], gt_dt=[], by_class={}, missed_uncovered=[0, 0],
                        cm=[[0, 0, 0], [0, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # ---- priority conflicts ----
    # s >= fg and o >= fg: the second detection finds its own-class GT taken -> DUPLICATE, not CLASSIFICATION.  cm: four pairs of IoU 1
    # in the order (r0, g0), (r0, g1), (r1, g0), (r1, g1): the first and the last are taken
    "duplicate_before_classification": ([(1, A, 100, 0), (2, A, 100, 0)], [(1, A, .9), (1, A, .8)], {},
                                        dict(dt_type=[TP, DUP], dt_gt=[0, 0], gt_state=[MATCHED, MISSED], gt_dt=[0, -1],
                                             by_class={(0, TP): 1, (0, DUP): 1, (1, MISSED_COL): 1}, missed_uncovered=[0, 1],
                                             cm=[[1, 0, 0], [1, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # o >= fg with bg <= s < fg: CLASSIFICATION, pointing at the other-class GT
    "classification_before_localization": ([(1, [0, 0, 10, 3], 30, 0), (2, A, 100, 0)], [(1, A, .9)], {},
                                           dict(dt_type=[CLS], dt_gt=[1], gt_state=[MISSED, MISSED_COVERED], gt_dt=[-1, -1],
                                                by_class={(0, CLS): 1, (0, MISSED_COL): 1, (1, MISSED_COL): 1}, missed_uncovered=[1, 0],
                                                cm=[[0, 0, 1], [1, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # bg <= s and bg <= o, both below fg (s = 0.3, o = 0.4): LOCALIZATION, pointing at the own-class GT
    "localization_before_both": ([(1, [0, 0, 10, 3], 30, 0), (2, [0, 0, 10, 4], 40, 0)], [(1, A, .9)], {},
                                 dict(dt_type=[LOC], dt_gt=[0], gt_state=[MISSED_COVERED, MISSED], gt_dt=[-1, -1],
                                      by_class={(0, LOC): 1, (0, MISSED_COL): 1, (1, MISSED_COL): 1}, missed_uncovered=[0, 1],
                                      cm=[[0, 0, 1], [0, 0, 1], [1, 0, 0]], cm_dropped=[0, 0])),
    # ---- IoU exactly at a threshold counts as reached ----
    "iou_exactly_fg": ([(1, [0, 0, 10, 5], 50, 0)], [(1, A, .9)], {},
                       dict(dt_type=[TP], dt_gt=[0], gt_state=[MATCHED], gt_dt=[0], by_class={(0, TP): 1}, missed_uncovered=[0, 0],
                            cm=[[1, 0, 0], [0, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    "iou_exactly_bg": ([(1, [0, 0, 10, 1], 10, 0)], [(1, A, .9)], {},
                       dict(dt_type=[LOC], dt_gt=[0], gt_state=[MISSED_COVERED], gt_dt=[-1], by_class={(0, LOC): 1, (0, MISSED_COL): 1},
                            missed_uncovered=[0, 0], cm=[[0, 0, 1], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    "iou_exactly_cm": ([(1, [0, 0, 10, 5], 50, 0)], [(2, A, .9)], {"cm_iou": 0.5},
                       dict(dt_type=[CLS], dt_gt=[0], gt_state=[MISSED_COVERED], gt_dt=[-1], by_class={(1, CLS): 1, (0, MISSED_COL): 1},
                            missed_uncovered=[0, 0], cm=[[0, 1, 0], [0, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # ---- crowd: the non-crowd GT is preferred although the crowd's IoU (intersection / detection area = 1) is as high; the second
    # detection falls to the crowd -> IGNORED, counted nowhere, and dropped from the confusion matrix ----
    "crowd": ([(1, [0, 0, 100, 100], 10000, 1), (1, [10, 10, 10, 10], 100, 0)], [(1, [10, 10, 10, 10], .9), (1, [10, 10, 10, 10], .8)], {},
              dict(dt_type=[TP, IGNORED], dt_gt=[1, 0], gt_state=[CROWD, MATCHED], gt_dt=[-1, 0], by_class={(0, TP): 1}, missed_uncovered=[0, 0],
                   cm=[[1, 0, 0], [0, 0, 0], [0, 0, 0]], cm_dropped=[1, 0])),
    "crowd_only": ([(1, [0, 0, 100, 100], 10000, 1)], [(1, [10, 10, 10, 10], .9), (2, [10, 10, 10, 10], .8)], {},
                   dict(dt_type=[IGNORED, BKG], dt_gt=[0, -1], gt_state=[CROWD], gt_dt=[-1], by_class={(1, BKG): 1}, missed_uncovered=[0, 0],
                        cm=[[0, 0, 0], [0, 0, 0], [0, 1, 0]], cm_dropped=[1, 0])),
    # ---- ties ----
    # equal scores: the file order ranks, so max_det = 1 keeps the first row (a miss) and never looks at the second
    "equal_scores": ([(1, A, 100, 0)], [(1, FAR, .5), (1, A, .5)], {"max_det": 1},
                     dict(dt_type=[BKG, NOT_EVALUATED], dt_gt=[-1, -1], gt_state=[MISSED], gt_dt=[-1], by_class={(0, BKG): 1, (0, MISSED_COL): 1},
                          missed_uncovered=[1, 0], cm=[[0, 0, 1], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    # equal IoU in step 1: the LAST GT is matched; in the cm order the FIRST GT pairs
    "step1_last_gt_wins": ([(1, A, 100, 0), (1, A, 100, 0)], [(1, A, .9)], {},
                           dict(dt_type=[TP], dt_gt=[1], gt_state=[MISSED, MATCHED], gt_dt=[-1, 0], by_class={(0, TP): 1, (0, MISSED_COL): 1},
                                missed_uncovered=[1, 0], cm=[[1, 0, 1], [0, 0, 0], [0, 0, 0]], cm_dropped=[0, 0])),
    # equal IoU in step 2: the FIRST GT is pointed at
    "step2_first_gt_wins": ([(2, A, 100, 0), (2, A, 100, 0)], [(1, A, .9)], {},
                            dict(dt_type=[CLS], dt_gt=[0], gt_state=[MISSED_COVERED, MISSED], gt_dt=[-1, -1],
                                 by_class={(0, CLS): 1, (1, MISSED_COL): 2}, missed_uncovered=[0, 1],
                                 cm=[[0, 0, 0], [1, 0, 1], [0, 0, 0]], cm_dropped=[0, 0])),
    # cm order, IoU first: r0 (class 1) has IoU 0.8 with g0, r1 (class 2) has IoU 1.0 with g0 -> g0 pairs with r1 although r0 ranks first
    "cm_iou_before_rank": ([(1, A, 100, 0)], [(1, [0, 0, 10, 8], .9), (2, A, .8)], {},
                           dict(dt_type=[TP, CLS], dt_gt=[0, 0], gt_state=[MATCHED], gt_dt=[0], by_class={(0, TP): 1, (1, CLS): 1},
                                missed_uncovered=[0, 0], cm=[[0, 1, 0], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    # ---- grid: the centre (25, 50) lies exactly on the lines x = 2 * 12.5 and y = 4 * 12.5 -> cell (ix 2, iy 4) ----
    "centre_on_grid_line": ([], [(1, [20, 45, 10, 10], .9)], {},
                            dict(dt_type=[BKG], dt_gt=[-1], gt_state=[], gt_dt=[], by_class={(0, BKG): 1}, by_cell={(4, 2, BKG): 1},
                                 missed_uncovered=[0, 0], cm=[[0, 0, 0], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    # the centre x = 100 = W gives 8.0 -> clamped to the last column; a centre left of and above the image -> cell (0, 0)
    "centre_at_image_edge": ([(1, [-40, -40, 10, 10], 100, 0)], [(1, [95, 0, 10, 10], .9)], {},
                             dict(dt_type=[BKG], dt_gt=[-1], gt_state=[MISSED], gt_dt=[-1], by_class={(0, BKG): 1, (0, MISSED_COL): 1},
                                  by_cell={(0, 7, BKG): 1, (0, 0, MISSED_COL): 1}, missed_uncovered=[1, 0],
                                  cm=[[0, 0, 1], [0, 0, 0], [1, 0, 0]], cm_dropped=[0, 0])),
    # sizes: areas 1023 / 1024 / 9215 / 9216 of missed GTs (the `area` field, not w * h), and a 32 x 32 background detection
    "size_boundaries": ([(1, [0, 0, 5, 5], 1023, 0), (1, [20, 0, 5, 5], 1024, 0), (1, [40, 0, 5, 5], 9215, 0), (1, [60, 0, 5, 5], 9216, 0)],
                        [(2, [0, 50, 32, 32], .9)], {},
                        dict(dt_type=[BKG], dt_gt=[-1], gt_state=[MISSED] * 4, gt_dt=[-1] * 4, by_class={(1, BKG): 1, (0, MISSED_COL): 4},
                             by_size={(0, MISSED_COL): 1, (1, MISSED_COL): 2, (2, MISSED_COL): 1, (1, BKG): 1}, missed_uncovered=[4, 0],
                             cm=[[0, 0, 4], [0, 0, 0], [0, 1, 0]], cm_dropped=[0, 0])),
}


def arrays(cases, first_image=1):
    """The named cases as one input set, one image each -> (gt, dt, img_wh, img_ids, row slices per case)."""
    gt = {k: [] for k in ("image_id", "category_id", "bbox", "area", "iscrowd")}
    dt = {k: [] for k in ("image_id", "category_id", "bbox", "score")}
    where = {}
    for n, name in enumerate(cases):
        gts, dts = CASES[name][:2]
        img = first_image + n
        where[name] = (img, slice(len(gt["area"]), len(gt["area"]) + len(gts)), slice(len(dt["score"]), len(dt["score"]) + len(dts)))
        for c, b, area, crowd in gts:
            gt["image_id"].append(img); gt["category_id"].append(c); gt["bbox"].append(b); gt["area"].append(area); gt["iscrowd"].append(crowd)
        for c, b, s in dts:
            dt["image_id"].append(img); dt["category_id"].append(c); dt["bbox"].append(b); dt["score"].append(s)
    gt = {k: np.array(v, np.float64 if k in ("bbox", "area") else np.int64) for k, v in gt.items()}
    dt = {k: np.array(v, np.float64 if k in ("bbox", "score") else np.int64) for k, v in dt.items()}
    gt["bbox"] = gt["bbox"].reshape(-1, 4)
    dt["bbox"] = dt["bbox"].reshape(-1, 4)
    ids = [first_image + n for n in range(len(cases))]
    return gt, dt, {i: WH for i in ids}, ids, where


def sparse(shape, entries):
    out = np.zeros(shape, np.int64)
    for k, v in entries.items():
        out[k] = v
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_hand_case(name):
    gt, dt, wh, ids, _ = arrays([name])
    want = CASES[name][3]
    out = XR.errors_ref(gt, dt, wh, ids, CATS, **CASES[name][2])
    for k in ("dt_type", "dt_gt", "gt_state", "gt_dt", "missed_uncovered", "cm", "cm_dropped"):
        assert out[k].tolist() == want[k], (k, out[k].tolist())
    assert np.array_equal(out["by_class"], sparse((2, 7), want["by_class"])), out["by_class"]
    if "by_cell" in want:
        assert np.array_equal(out["by_cell"], sparse((8, 8, 7), want["by_cell"])), np.argwhere(out["by_cell"])
    if "by_size" in want:
        assert np.array_equal(out["by_size"], sparse((3, 7), want["by_size"])), out["by_size"]
    assert out["by_class"].sum() == out["by_size"].sum() == out["by_cell"].sum()
    assert out["by_class"].dtype == out["cm"].dtype == np.int64


def test_totals_and_confusion_matrix_identities():
    """All cases in one call (default parameters): the three histograms count the same events column by column; the cm rows of the real
    classes sum to the non-crowd GTs per class, its columns plus the dropped detections to the kept detections per class."""
    gt, dt, wh, ids, _ = arrays(list(CASES))
    out = XR.errors_ref(gt, dt, wh, ids, CATS)
    assert np.array_equal(out["by_class"].sum(axis=0), out["by_size"].sum(axis=0))
    assert np.array_equal(out["by_class"].sum(axis=0), out["by_cell"].sum(axis=(0, 1)))
    assert out["by_class"].sum() > 30
    kept = out["dt_type"] != NOT_EVALUATED
    for k, c in enumerate(CATS):
        assert out["cm"][k].sum() == ((gt["category_id"] == c) & (gt["iscrowd"] == 0)).sum()
        assert out["cm"][:, k].sum() + out["cm_dropped"][k] == (kept & (dt["category_id"] == c)).sum()
        assert out["by_class"][k, MISSED_COL] == ((gt["category_id"] == c) & np.isin(out["gt_state"], (MISSED, MISSED_COVERED))).sum()
        assert out["missed_uncovered"][k] == ((gt["category_id"] == c) & (out["gt_state"] == MISSED)).sum()
    assert out["cm"][2, 2] == 0
    # every matched GT and its detection point at each other
    for g in np.nonzero(out["gt_state"] == MATCHED)[0]:
        assert out["dt_type"][out["gt_dt"][g]] == TP and out["dt_gt"][out["gt_dt"][g]] == g


def test_rows_outside_the_evaluated_sets_take_no_part():
    gt, dt, wh, ids, _ = arrays(["tp", "classification"])
    out = XR.errors_ref(gt, dt, wh, [1], [1])              # image 2 and category 2 are not evaluated
    assert out["dt_type"].tolist() == [TP, NOT_EVALUATED] and out["gt_state"].tolist() == [MATCHED, XR.GT_NOT_EVALUATED]
    assert out["cm"].tolist() == [[1, 0], [0, 0]] and out["by_class"].tolist() == [[1, 0, 0, 0, 0, 0, 0]]


# ---- the library without a GPU: argument checks come before the first HIP call -------------------------------------------------------
def call(params=None, K=2, n_img=1, null=(), **over):
    """rtmodt_detection_errors on one 100 x 100 image with one GT and one detection, with some arguments replaced -> (code, message)."""
    a = {"img_wh": np.array([[100.0, 100.0]]), "gt_start": np.array([0, 1], np.int32), "gt_cat": np.array([0], np.int32),
         "gt_box": np.array([[0.0, 0, 10, 10]]), "gt_area": np.array([100.0]), "gt_crowd": np.array([0], np.int32),
         "dt_start": np.array([0, 1], np.int32), "dt_cat": np.array([1], np.int32), "dt_box": np.array([[0.0, 0, 10, 10]]),
         "dt_score": np.array([0.9])}
    a.update({k: np.ascontiguousarray(v) for k, v in over.items()})
    n_gt, n_dt = int(a["gt_start"][-1]), int(a["dt_start"][-1])
    p = dict(conf_thr=0.25, iou_fg=0.5, iou_bg=0.1, cm_iou=0.45, max_det=100, grid_x=8, grid_y=8)
    p.update(params or {})
    a.update({"dt_type": np.zeros(n_dt, np.int32), "dt_gt": np.zeros(n_dt, np.int32), "gt_state": np.zeros(n_gt, np.int32),
              "gt_dt": np.zeros(n_gt, np.int32), "by_class": np.zeros((K, 7), np.int64), "by_size": np.zeros((3, 7), np.int64),
              "by_cell": np.zeros((64, 64, 7), np.int64), "missed_uncovered": np.zeros(K, np.int64), "cm": np.zeros((K + 1, K + 1), np.int64),
              "cm_dropped": np.zeros(K, np.int64)})
    P = lambda k: None if k in null else _ffi.ptr(a[k])    # noqa: E731
    ps = _ffi.ErrorParams(p["conf_thr"], p["iou_fg"], p["iou_bg"], p["cm_iou"], p["max_det"], p["grid_x"], p["grid_y"], 0)
    L = _ffi.lib()
    rc = L.rtmodt_detection_errors(0, None if "params" in null else ctypes.byref(ps), K, n_img, P("img_wh"), P("gt_start"), P("gt_cat"), P("gt_box"),
                                   P("gt_area"), P("gt_crowd"), P("dt_start"), P("dt_cat"), P("dt_box"), P("dt_score"), P("dt_type"), P("dt_gt"),
                                   P("gt_state"), P("gt_dt"), P("by_class"), P("by_size"), P("by_cell"), P("missed_uncovered"), P("cm"),
                                   P("cm_dropped"))
    return rc, L.rtmodt_last_error().decode()


NAN = float("nan")
BAD = [  # (what, keyword arguments of call(), code, text the message must hold)
    ("null params", dict(null=("params",)), _ffi.E_INVALID, "null params"),
    ("null histogram", dict(null=("cm",)), _ffi.E_INVALID, "null histogram"),
    ("null image sizes", dict(null=("img_wh",)), _ffi.E_INVALID, "null image arrays"),
    ("null CSR", dict(null=("dt_start",)), _ffi.E_INVALID, "null image arrays"),
    ("null GT array", dict(null=("gt_area",)), _ffi.E_INVALID, "null GT arrays"),
    ("null GT output", dict(null=("gt_state",)), _ffi.E_INVALID, "null GT arrays"),
    ("null detection array", dict(null=("dt_score",)), _ffi.E_INVALID, "null detection arrays"),
    ("null detection output", dict(null=("dt_gt",)), _ffi.E_INVALID, "null detection arrays"),
    ("NaN conf_thr", dict(params={"conf_thr": NAN}), _ffi.E_INVALID, "conf_thr is NaN"),
    ("NaN iou_fg", dict(params={"iou_fg": NAN}), _ffi.E_INVALID, "iou_fg is NaN"),
    ("NaN iou_bg", dict(params={"iou_bg": NAN}), _ffi.E_INVALID, "iou_bg is NaN"),
    ("NaN cm_iou", dict(params={"cm_iou": NAN}), _ffi.E_INVALID, "cm_iou is NaN"),
    ("iou_bg above iou_fg", dict(params={"iou_bg": 0.6}), _ffi.E_INVALID, "iou_bg 0.6 > iou_fg 0.5"),
    ("max_det 0", dict(params={"max_det": 0}), _ffi.E_INVALID, "max_det 0 outside 1..1024"),
    ("max_det 1025", dict(params={"max_det": 1025}), _ffi.E_INVALID, "max_det 1025 outside 1..1024"),
    ("grid_x 0", dict(params={"grid_x": 0}), _ffi.E_INVALID, "grid 0 x 8 outside 1..64"),
    ("grid_y 65", dict(params={"grid_y": 65}), _ffi.E_INVALID, "grid 8 x 65 outside 1..64"),
    ("K 0", dict(K=0), _ffi.E_INVALID, "K 0"),
    ("zero width", dict(img_wh=[[0.0, 100.0]]), _ffi.E_INVALID, "image 0: width 0, height 100"),
    ("negative height", dict(img_wh=[[100.0, -1.0]]), _ffi.E_INVALID, "image 0: width 100, height -1"),
    ("NaN width", dict(img_wh=[[NAN, 100.0]]), _ffi.E_INVALID, "image 0: width nan"),
    ("CSR not from 0", dict(gt_start=np.array([1, 1], np.int32)), _ffi.E_INVALID, "CSR must start at 0"),
    ("CSR descending", dict(n_img=2, img_wh=[[100.0, 100.0]] * 2, gt_start=np.array([0, 1, 0], np.int32), dt_start=np.array([0, 1, 1], np.int32)),
     _ffi.E_INVALID, "image 1: malformed CSR"),
    ("GT category", dict(gt_cat=np.array([2], np.int32)), _ffi.E_INVALID, "GT row 0: category index 2 outside 0..1"),
    ("detection category", dict(dt_cat=np.array([-1], np.int32)), _ffi.E_INVALID, "detection row 0: category index -1 outside 0..1"),
    ("NaN GT box", dict(gt_box=[[0.0, NAN, 10, 10]]), _ffi.E_INVALID, "GT row 0 has a NaN or infinite box"),
    ("NaN GT area", dict(gt_area=[NAN]), _ffi.E_INVALID, "GT row 0 has a NaN area"),
    ("NaN detection box", dict(dt_box=[[0.0, 0, NAN, 10]]), _ffi.E_INVALID, "detection row 0 has a NaN or infinite box"),
    ("NaN score", dict(dt_score=[NAN]), _ffi.E_INVALID, "detection row 0 has a NaN score"),
    ("1025 GTs", dict(n_img=2, img_wh=[[100.0, 100.0]] * 2, gt_start=np.array([0, 0, 1025], np.int32), dt_start=np.array([0, 1, 1], np.int32),
                      gt_cat=np.zeros(1025, np.int32), gt_box=np.ones((1025, 4)), gt_area=np.ones(1025), gt_crowd=np.zeros(1025, np.int32)),
     _ffi.E_CAPACITY, "image 1 holds 1025 GTs > 1024"),
    ("4097 detections", dict(dt_start=np.array([0, 4097], np.int32), dt_cat=np.zeros(4097, np.int32), dt_box=np.ones((4097, 4)),
                             dt_score=np.ones(4097)), _ffi.E_CAPACITY, "image 0 holds 4097 detections > 4096"),
]


@pytest.mark.parametrize("what,kw,code,text", BAD, ids=[b[0] for b in BAD])
def test_argument_checks_need_no_gpu(what, kw, code, text):
    rc, msg = call(**kw)
    assert rc == code and text in msg and msg.startswith("detection_errors:"), (rc, msg)


def test_python_wrapper_raises_the_library_error_and_its_own():
    gt, dt, wh, ids, _ = arrays(["tp"])
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.detection_errors(gt, dt, img_wh=wh, img_ids=ids, cat_ids=CATS, iou_bg=0.7)
    assert e.value.code == _ffi.E_INVALID and "iou_bg 0.7 > iou_fg 0.5" in e.value.msg
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.detection_errors(gt, dt, img_wh={1: (100.0, 0.0)}, img_ids=ids, cat_ids=CATS)
    assert e.value.code == _ffi.E_INVALID and "height 0" in e.value.msg
    with pytest.raises(ValueError, match=r"lacks images \[1\]"):
        EV.detection_errors(gt, dt, img_wh={}, img_ids=ids, cat_ids=CATS)
    with pytest.raises(ValueError, match="needs img_ids"):
        EV.detection_errors(gt, dt, img_wh=[[100, 100]], cat_ids=CATS)
    with pytest.raises(ValueError, match="2 rows for 1 image ids"):
        EV.detection_errors(gt, dt, img_wh=[[100, 100], [5, 5]], img_ids=ids, cat_ids=CATS)


def test_exports_and_struct_layout():
    for n in ("detection_errors", "analyze_detection_errors", "format_confusion_matrix", "format_error_table", "build_confusion_matrix"):
        assert n in EV.__all__ and callable(getattr(EV, n))
    assert ctypes.sizeof(_ffi.ErrorParams) == 48
    assert [getattr(_ffi.ErrorParams, n).offset for n, _ in _ffi.ErrorParams._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert "rtmodt_detection_errors" in _ffi.header_symbols()


# ---- formatters ------------------------------------------------------------------------------------------------------------------------
def test_format_confusion_matrix_fixed_text():
    cm = np.array([[50, 2, 0, 7], [1, 120, 3, 10], [0, 0, 9, 1], [4, 11, 0, 0]])
    assert EV.format_confusion_matrix(cm, ["person", "car", "dog"]) == (
        "gt \\ pred   person  car  dog  background\n"
        "person          50    2    0           7\n"
        "car              1  120    3          10\n"
        "dog              0    0    9           1\n"
        "background       4   11    0           0\n")
    with pytest.raises(ValueError, match="3 names"):
        EV.format_confusion_matrix(cm[:3, :3], ["person", "car", "dog"])


def test_format_error_table_fixed_text():
    res = {"by_class": np.array([[50, 3, 1, 0, 2, 4, 9], [120, 0, 2, 1, 0, 11, 14], [9, 1, 0, 0, 0, 0, 1]]),
           "by_size": np.array([[20, 3, 2, 1, 1, 9, 15], [100, 1, 1, 0, 1, 5, 8], [59, 0, 0, 0, 0, 1, 1]]),
           "missed_uncovered": np.array([6, 12, 1])}
    assert EV.format_error_table(res, ["person", "car", "dog"]) == (
        "class / size   TP  LOCALIZATION  CLASSIFICATION  BOTH  DUPLICATE  BACKGROUND  MISSED\n"
        "person         50             3               1     0          2           4       9\n"
        "car           120             0               2     1          0          11      14\n"
        "dog             9             1               0     0          0           0       1\n"
        "all           179             4               3     1          2          15      24\n"
        "small          20             3               2     1          1           9      15\n"
        "medium        100             1               1     0          1           5       8\n"
        "large          59             0               0     0          0           1       1\n"
        "missed and not covered by any detection: 19\n")
