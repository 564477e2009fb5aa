"""rtmodt_amd.evaluation.detection_errors on the GPU against the NumPy restatement (tests/errors_ref.py): every output equal, no
tolerances -- the four per-row arrays, the three histograms, missed_uncovered, cm and cm_dropped."""
import numpy as np
import pytest

import errors_ref as XR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def EV():
    import rtmodt_amd
    return rtmodt_amd.evaluation


def same(out, ref):
    for k in XR.OUTPUTS:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (k, out[k].dtype, out[k].shape, ref[k].shape)
        assert np.array_equal(out[k], ref[k]), (k, np.argwhere(out[k] != ref[k])[:5])


def test_hand_cases_single_and_in_one_call(EV):
    """The hand-worked cases of tests/test_errors_cpu.py: each as a single image with its own parameters (their literal expectations are
    checked against the restatement there), then all in one call."""
    import test_errors_cpu as TC
    for name in TC.CASES:
        gt, dt, wh, ids, _ = TC.arrays([name])
        kw = TC.CASES[name][2]
        same(EV.detection_errors(gt, dt, img_wh=wh, img_ids=ids, cat_ids=TC.CATS, **kw), XR.errors_ref(gt, dt, wh, ids, TC.CATS, **kw))
    gt, dt, wh, ids, where = TC.arrays(list(TC.CASES), first_image=5)
    out = EV.detection_errors(gt, dt, img_wh=wh, img_ids=ids, cat_ids=TC.CATS)
    same(out, XR.errors_ref(gt, dt, wh, ids, TC.CATS))
    _, gs, ds = where["crowd"]                               # one answer stated outright
    assert out["dt_type"][ds].tolist() == [TC.TP, TC.IGNORED] and out["gt_state"][gs].tolist() == [TC.CROWD, TC.MATCHED]
    # img_wh as an array in the caller's image order
    rev = ids[::-1]
    same(EV.detection_errors(gt, dt, img_wh=[wh[i] for i in rev], img_ids=rev, cat_ids=TC.CATS), XR.errors_ref(gt, dt, wh, ids, TC.CATS))


def synth(seed, n_img=40, n_cat=5, nonzero_ids=False):
    """tests/test_gpu_eval.py's synth_coco (integer-grid boxes, scores on a 0.01 grid, 6 % crowd GTs, category 998 with detections
    but no GT, detections of the unknown category 999) plus image sizes; some images have no GT, no detection, or neither."""
    from test_gpu_eval import synth_coco
    gt, dt, img_ids, cats = synth_coco(seed, n_img=n_img, n_cat=n_cat)
    if nonzero_ids:
        gt["id"] = gt["id"] + 1
    rng = np.random.default_rng(seed + 1000)
    wh = {int(i): (float(rng.integers(300, 460)), float(rng.integers(280, 460))) for i in img_ids}
    return gt, dt, wh, img_ids, cats


def test_random_data_equals_restatement(EV):
    gt, dt, wh, img_ids, cats = synth(12)
    has_g, has_d = np.isin(img_ids, gt["image_id"]), np.isin(img_ids, dt["image_id"])
    assert (~has_g & has_d).any() and (has_g & ~has_d).any() and (~has_g & ~has_d).any()    # no GT / no detection / neither
    kw = dict(conf_thr=0.3, max_det=6, iou_fg=0.6, iou_bg=0.2, cm_iou=0.5, grid=(5, 3))
    out = EV.detection_errors(gt, dt, img_wh=wh, img_ids=img_ids, cat_ids=cats, **kw)
    ref = XR.errors_ref(gt, dt, wh, img_ids, cats, **kw)
    same(out, ref)
    assert out["by_cell"].shape == (3, 5, 7)
    assert (ref["by_class"].sum(axis=0) > 0).all(), ref["by_class"].sum(axis=0)            # every column occurs
    assert ref["cm_dropped"].sum() > 0 and (ref["dt_type"] == XR.IGNORED).any() and (ref["dt_type"] == XR.NOT_EVALUATED).sum() > len(dt["score"]) // 4
    assert (ref["gt_state"] == XR.GT_MISSED_COVERED).any() and ref["by_class"][-1, :6].sum() > 0 and ref["by_class"][-1, 6] == 0   # 998: no GT
    # default parameters as well, and twice: integer counts do not depend on the arrival order of the atomics
    a = EV.detection_errors(gt, dt, img_wh=wh, img_ids=img_ids, cat_ids=cats)
    same(a, XR.errors_ref(gt, dt, wh, img_ids, cats))
    same(EV.detection_errors(gt, dt, img_wh=wh, img_ids=img_ids, cat_ids=cats), a)


def dense_image(seed, n_gt, n_dt, n_cat=3):
    """One image: GTs on a 40-pixel lattice (4 % crowd), detections on or near them with scores on a 0.01 grid."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_gt)))
    gb = np.array([[40 * (j % side), 40 * (j // side), rng.integers(8, 36), rng.integers(8, 36)] for j in range(n_gt)], np.float64)
    gt = {"image_id": np.ones(n_gt, np.int64), "category_id": rng.integers(1, n_cat + 1, n_gt), "bbox": gb, "area": gb[:, 2] * gb[:, 3],
          "iscrowd": (rng.random(n_gt) < 0.04).astype(np.int64)}
    on = rng.integers(0, n_gt, n_dt)
    db = gb[on] + np.where(rng.random((n_dt, 1)) < 0.5, rng.integers(-1, 2, (n_dt, 4)), rng.integers(-6, 7, (n_dt, 4)))
    db[:, 2:] = np.maximum(db[:, 2:], 1)
    dc = np.where(rng.random(n_dt) < 0.8, gt["category_id"][on], rng.integers(1, n_cat + 1, n_dt))
    dt = {"image_id": np.ones(n_dt, np.int64), "category_id": dc, "bbox": db, "score": np.round(rng.random(n_dt), 2)}
    return gt, dt, {1: (40.0 * side, 40.0 * side)}


def test_stride_crossings_and_max_det_cut(EV):
    """300 GTs (five 64-lane passes of step 1, two workgroup strides) and 130 detections at or above conf_thr out of 200 (the
    max_det = 100 cut applies; two strides of the rank sort)."""
    gt, dt, wh = dense_image(3, 300, 200)
    dt["score"][:130] = np.maximum(dt["score"][:130], 0.25)
    dt["score"][130:] = np.minimum(dt["score"][130:], 0.24)
    out = EV.detection_errors(gt, dt, img_wh=wh)
    ref = XR.errors_ref(gt, dt, wh)
    same(out, ref)
    assert (ref["dt_type"] != XR.NOT_EVALUATED).sum() == 100 and (ref["dt_type"][130:] == XR.NOT_EVALUATED).all()
    assert (ref["dt_type"] == XR.TP).sum() > 20 and (ref["dt_type"] == XR.DUPLICATE).sum() > 0


def test_capacity_exact_and_one_beyond(EV):
    """Exactly 1024 GTs and 4096 raw detections in one image (max_det = 1024: the largest LDS carve) runs and equals the restatement;
    one GT or one detection more is a capacity error naming the image, before anything is launched (the outputs stay untouched is
    the library's contract; here: the error code and text)."""
    from rtmodt_amd import _ffi
    gt, dt, wh = dense_image(8, 1024, 4096)
    kw = dict(conf_thr=0.8, max_det=1024)                  # about 800 detections are kept
    same(EV.detection_errors(gt, dt, img_wh=wh, **kw), XR.errors_ref(gt, dt, wh, **kw))
    more_gt = {k: np.concatenate([v, v[:1]]) for k, v in gt.items()}
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.detection_errors(more_gt, dt, img_wh=wh, **kw)
    assert e.value.code == _ffi.E_CAPACITY and "image 0 holds 1025 GTs" in e.value.msg
    more_dt = {k: np.concatenate([v, v[:1]]) for k, v in dt.items()}
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.detection_errors(gt, more_dt, img_wh=wh, **kw)
    assert e.value.code == _ffi.E_CAPACITY and "image 0 holds 4097 detections" in e.value.msg


def test_true_positives_agree_with_coco_eval_recall(EV):
    """A cross-check against code that exists: with every detection kept (conf_thr = -inf) and iou_fg = 0.5, step 1 is COCOeval's
    matcher at IoU 0.5 over all areas (no image of this set has more than 100 detections, so the per-image cut equals the per-cell
    one; annotation ids are all nonzero), hence TP_k / (non-crowd GT_k) is coco_eval's recall[t = 0.5, k, all, 100] bit for bit."""
    gt, dt, wh, img_ids, cats = synth(5, n_img=120, n_cat=8, nonzero_ids=True)
    assert max(np.bincount(np.searchsorted(img_ids, dt["image_id"]))) <= 100 and (gt["id"] != 0).all()
    out = EV.detection_errors(gt, dt, img_wh=wh, img_ids=img_ids, cat_ids=cats, conf_thr=-np.inf, iou_fg=0.5)
    rec = EV.coco_eval(gt, dt, img_ids=img_ids, cat_ids=cats, iou_thrs=[0.5])["recall"][0, :, 0, 2]
    for k, c in enumerate(cats):
        n = int(((gt["category_id"] == c) & (gt["iscrowd"] == 0)).sum())
        tp = int(out["by_class"][k, 0])
        if n == 0:
            assert rec[k] == -1 and tp == 0
        else:
            assert np.float64(tp) / np.float64(n) == rec[k], (c, tp, n, rec[k])
    assert out["by_class"][:, 0].sum() > 100


def test_file_level_entry_point(EV, tmp_path):
    import json
    gt, dt, wh, img_ids, cats = synth(9, n_img=12, n_cat=3)
    gj = {"images": [{"id": int(i), "width": wh[int(i)][0], "height": wh[int(i)][1]} for i in img_ids], "categories": [{"id": int(c)} for c in cats],
          "annotations": [{"id": int(gt["id"][i]) + 1, "image_id": int(gt["image_id"][i]), "category_id": int(gt["category_id"][i]),
                           "bbox": gt["bbox"][i].tolist(), "area": float(gt["area"][i]), "iscrowd": int(gt["iscrowd"][i])} for i in range(len(gt["id"]))]}
    rj = [{"image_id": int(dt["image_id"][i]), "category_id": int(dt["category_id"][i]), "bbox": dt["bbox"][i].tolist(), "score": float(dt["score"][i])}
          for i in range(len(dt["score"]))]
    (tmp_path / "gt.json").write_text(json.dumps(gj))
    (tmp_path / "res.json").write_text(json.dumps(rj))
    out = EV.analyze_detection_errors(str(tmp_path / "gt.json"), str(tmp_path / "res.json"), grid=(4, 4))
    same(out, XR.errors_ref(gt, dt, wh, img_ids, cats, grid=(4, 4)))
    text = EV.format_error_table(out, [str(c) for c in cats]) + EV.format_confusion_matrix(out["cm"], [str(c) for c in cats])
    assert text.count("\n") == 1 + len(cats) + 1 + 3 + 1 + 1 + len(cats) + 1
