"""rtmodt_amd.evaluation on the GPU against the NumPy restatement (tests/eval_ref.py): COCO precision / recall bit for
bit, CLEAR MOT / IDF1 counts exactly, on seeded synthetic data."""
import json

import numpy as np
import pytest

import eval_ref as ER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def EV():
    import rtmodt_amd
    return rtmodt_amd.evaluation


def synth_coco(seed, n_img=300, n_cat=12):
    """Integer-grid boxes spanning every area range, crowd GTs, a GT with id 0, scores on a 0.01 grid (many ties), a
    category with detections but no GT (-1), detections of an unknown category (dropped)."""
    rng = np.random.default_rng(seed)
    cats = np.arange(1, n_cat + 1) * 3
    gt = {k: [] for k in ("id", "image_id", "category_id", "bbox", "area", "iscrowd")}
    dt = {k: [] for k in ("image_id", "category_id", "bbox", "score")}
    nid = 0
    for im in range(n_img):
        img = 1000 + 7 * im
        for _ in range(rng.integers(0, 9)):
            w, h = int(rng.integers(2, 150)), int(rng.integers(2, 150))
            x, y = int(rng.integers(0, 300)), int(rng.integers(0, 300))
            c = int(rng.choice(cats))
            gt["id"].append(nid); nid += 1
            gt["image_id"].append(img); gt["category_id"].append(c)
            gt["bbox"].append([x, y, w, h]); gt["area"].append(float(w * h) * float(rng.choice([1.0, 0.7])))
            gt["iscrowd"].append(int(rng.random() < 0.06))
            for _ in range(rng.integers(0, 4)):            # detections near this GT
                jx, jy, jw, jh = (int(v) for v in rng.integers(-6, 7, 4))
                dt["image_id"].append(img)
                dt["category_id"].append(c if rng.random() < 0.85 else int(rng.choice(cats)))
                dt["bbox"].append([x + jx, y + jy, max(1, w + jw), max(1, h + jh)])
                dt["score"].append(round(float(rng.random()), 2))
        for _ in range(rng.integers(0, 5)):                # background detections
            dt["image_id"].append(img)
            u = rng.random()
            dt["category_id"].append(int(rng.choice(cats)) if u < 0.9 else (998 if u < 0.95 else 999))
            dt["bbox"].append([int(rng.integers(0, 300)), int(rng.integers(0, 300)), int(rng.integers(1, 120)), int(rng.integers(1, 120))])
            dt["score"].append(round(float(rng.random()), 2))
    gt = {k: np.array(v) for k, v in gt.items()}
    dt = {k: np.array(v) for k, v in dt.items()}
    gt["bbox"] = gt["bbox"].astype(np.float64).reshape(-1, 4)
    dt["bbox"] = dt["bbox"].astype(np.float64).reshape(-1, 4)
    return gt, dt, np.array([1000 + 7 * i for i in range(n_img)]), np.append(cats, 998)     # 998: detections only; 999: dropped


def _ref_on(gt, dt, img_ids, cats, iou_thrs):
    keep = np.isin(dt["category_id"], cats)                # results of an unknown category are dropped
    return ER.coco_ref(gt, {k: v[keep] for k, v in dt.items()}, img_ids, cats, iou_thrs)


@pytest.mark.parametrize("T", [1, 10])
def test_coco_bit_identical(EV, T):
    gt, dt, img_ids, cats = synth_coco(11 + T)
    iou = [0.5] if T == 1 else None
    out = EV.coco_eval(gt, dt, img_ids=img_ids, cat_ids=cats, iou_thrs=iou)
    p, r = _ref_on(gt, dt, img_ids, cats, iou)
    assert out["precision"].shape == p.shape and out["recall"].shape == r.shape
    assert np.array_equal(out["precision"].view(np.int64), p.view(np.int64)), np.argwhere(out["precision"] != p)[:5]
    assert np.array_equal(out["recall"].view(np.int64), r.view(np.int64))
    assert np.array_equal(out["stats"], EV.coco_stats(p, r, out["iou_thrs"]))
    assert (p > 0).any() and (p == -1).any()
    if T == 1:
        assert out["stats"][2] == -1


def dense_coco(seed):
    """A few dense cells: 300 GTs on a grid (more than one 64-lane pass of the matcher, hundreds of true positives per
    category: several chunks of the suffix max) and 600 detections per cell (the rank sort's 256-thread stride, the
    maxDets 10 / 100 cuts), scores on a 0.01 grid."""
    rng = np.random.default_rng(seed)
    gt = {k: [] for k in ("id", "image_id", "category_id", "bbox", "area", "iscrowd")}
    dt = {k: [] for k in ("image_id", "category_id", "bbox", "score")}
    nid = 1
    for img in range(1, 11):
        for c in (1, 2):
            boxes = []
            for j in range(300):
                x, y = 40 * (j % 20), 40 * (j // 20)
                w, h = int(rng.integers(3, 35)), int(rng.integers(3, 35))
                boxes.append((x, y, w, h))
                gt["id"].append(nid); nid += 1
                gt["image_id"].append(img); gt["category_id"].append(c); gt["bbox"].append([x, y, w, h])
                gt["area"].append(float(w * h)); gt["iscrowd"].append(int(rng.random() < 0.03))
            for q in range(600):
                x, y, w, h = boxes[int(rng.integers(0, 300))]
                if q % 2:                                      # on a GT, a pixel or two off
                    b = [x + int(rng.integers(-1, 2)), y + int(rng.integers(-1, 2)), w + int(rng.integers(-1, 2)), h]
                else:
                    b = [x + int(rng.integers(-3, 4)), y + int(rng.integers(-3, 4)), int(rng.integers(3, 35)), int(rng.integers(3, 35))]
                dt["image_id"].append(img); dt["category_id"].append(c); dt["bbox"].append(b)
                dt["score"].append(round(float(rng.random()), 2))
    gt = {k: np.array(v) for k, v in gt.items()}
    dt = {k: np.array(v) for k, v in dt.items()}
    gt["bbox"] = gt["bbox"].astype(np.float64)
    dt["bbox"] = dt["bbox"].astype(np.float64)
    return gt, dt


def test_coco_dense_cells_bit_identical(EV):
    gt, dt = dense_coco(4)
    out = EV.coco_eval(gt, dt, iou_thrs=[0.3, 0.5])
    p, r = ER.coco_ref(gt, dt, iou_thrs=[0.3, 0.5])
    assert np.array_equal(out["precision"].view(np.int64), p.view(np.int64)), np.argwhere(out["precision"] != p)[:5]
    assert np.array_equal(out["recall"].view(np.int64), r.view(np.int64))
    npig = int(((gt["category_id"] == 1) & (gt["iscrowd"] == 0)).sum())
    assert round(r[0, 0, 0, 2] * npig) > 256 and r[0, 0, 0, 1] < r[0, 0, 0, 2]   # > 256 true positives; maxDets 10 cuts


def test_coco_hand_derived_cases(EV):
    """Every hand-derived case of tests/test_eval_cpu.py, on the GPU, against the restatement bit for bit."""
    import test_eval_cpu as TC
    for name, (gts, dts, cat_ids) in TC.CASES.items():
        gt = {"image_id": np.array([g[0] for g in gts]), "category_id": np.array([g[1] for g in gts]),
              "bbox": np.array([g[2] for g in gts], np.float64), "area": np.array([g[3] for g in gts], np.float64),
              "iscrowd": np.array([g[4] for g in gts]), "id": np.array([g[5] for g in gts])}
        dt = {"image_id": np.array([d[0] for d in dts]), "category_id": np.array([d[1] for d in dts]),
              "bbox": np.array([d[2] for d in dts], np.float64), "score": np.array([d[3] for d in dts], np.float64)}
        out = EV.coco_eval(gt, dt, cat_ids=cat_ids, iou_thrs=[0.5])
        p, r = ER.coco_ref(gt, dt, cat_ids=cat_ids, iou_thrs=[0.5])
        assert np.array_equal(out["precision"].view(np.int64), p.view(np.int64)), name
        assert np.array_equal(out["recall"].view(np.int64), r.view(np.int64)), name
    # two of the answers, stated outright
    assert out["stats"][0] == 0.0                                            # gt_id_zero: the only hit counts as a false positive


def test_coco_known_answer(EV):
    gt = {"id": np.array([1, 2]), "image_id": np.array([1, 1]), "category_id": np.array([1, 1]),
          "bbox": np.array([[0, 0, 10, 10], [20, 0, 10, 10]], np.float64), "area": np.array([100.0, 100.0]), "iscrowd": np.array([0, 0])}
    dt = {"image_id": np.array([1, 1, 1]), "category_id": np.array([1, 1, 1]),
          "bbox": np.array([[0, 0, 10, 10], [50, 50, 10, 10], [20, 0, 10, 10]], np.float64), "score": np.array([.9, .8, .7])}
    out = EV.coco_eval(gt, dt, iou_thrs=[0.5])
    assert out["stats"][0] == 0.834983498349835


def _mot_sequence(rng, n_frames=60, n_obj=12):
    """Continuous random boxes (tie-free), linear motion, births / deaths, gaps, hypotheses with noise, id switches and
    false positives."""
    gt, hyp = [], []
    hid_next = 100
    for o in range(n_obj):
        t0 = int(rng.integers(0, n_frames // 2)); t1 = int(rng.integers(t0 + 3, n_frames + 1))
        x, y = rng.uniform(0, 400, 2); vx, vy = rng.uniform(-3, 3, 2); w, h = rng.uniform(20, 60, 2)
        hid = hid_next; hid_next += 1
        for f in range(t0, t1):
            bx, by = x + vx * f, y + vy * f
            if rng.random() < 0.05:                        # GT gap
                continue
            gt.append([f + 1, o + 1, bx, by, w, h])
            if rng.random() < 0.1:                         # missed by the tracker
                continue
            if rng.random() < 0.04:                        # identity switch
                hid = hid_next; hid_next += 1
            n = rng.normal(0, 2.5, 4)
            hyp.append([f + 1, hid, bx + n[0], by + n[1], w + n[2], h + n[3]])
    for _ in range(n_frames // 3):                         # false positives
        f = int(rng.integers(1, n_frames + 1))
        hyp.append([f, hid_next, *rng.uniform(0, 400, 2), *rng.uniform(20, 60, 2)]); hid_next += 1
    hyp.append([n_frames + 3, 7, 1.5, 2.5, 10.25, 10.5])  # a frame present in one file only
    return np.array(gt, np.float64), np.array(hyp, np.float64)


KEYS = ("num_frames", "num_objects", "num_predictions", "num_matches", "num_switches", "num_misses", "num_false_positives",
        "mostly_tracked", "mostly_lost", "num_unique_objects", "idtp", "idfp", "idfn")


def test_mot_counts_equal_batched_and_single(EV):
    rng = np.random.default_rng(7)
    seqs = [_mot_sequence(rng, n_frames=40 + 10 * i, n_obj=8 + 3 * i) for i in range(5)]
    got = EV.mot_eval(seqs)
    for (g, h), r in zip(seqs, got):
        ref = ER.mot_ref(g, h)
        for k in KEYS:
            assert r[k] == ref[k], (k, r[k], ref[k])
        assert abs(r["motp"] - ref["motp"]) <= 1e-12 * abs(ref["motp"])
        assert r["mota"] == ref["mota"] and r["idf1"] == ref["idf1"]
    assert sum(r["num_switches"] for r in got) > 0
    for s, r in zip(seqs, got):
        one = EV.mot_eval([s])[0]
        assert one == r


def test_mot_assignment_optimal_on_ties(EV):
    """Integer-grid boxes with many equal distances: one frame per sequence, so the counts are exactly the optimal
    (cardinality, sum of d) of that frame's assignment."""
    rng = np.random.default_rng(3)
    seqs, opt = [], []
    for _ in range(40):
        no, nh = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        g = np.array([[1, i + 1, *rng.integers(0, 40, 2), 10, 10] for i in range(no)], np.float64)
        h = np.array([[1, i + 1, *rng.integers(0, 40, 2), 10, 10] for i in range(nh)], np.float64)
        D = np.array([[1 - ER.box_iou(a[2:], b[2:]) for b in h] for a in g])
        pairs = ER.assign_lex(D, D <= 0.5)
        seqs.append((g, h))
        opt.append((len(pairs), sum(D[i, j] for i, j in pairs)))
    got = EV.mot_eval(seqs)
    for r, (card, dsum) in zip(got, opt):
        assert r["num_matches"] + r["num_switches"] == card
        assert abs(r["dist_sum"] - dsum) <= 1e-12 * max(1.0, dsum)


def test_file_level_entry_points(EV, tmp_path):
    gt, dt, img_ids, cats = synth_coco(5, n_img=40, n_cat=5)
    gj = {"images": [{"id": int(i)} for i in img_ids], "categories": [{"id": int(c)} for c in cats],
          "annotations": [{"id": int(gt["id"][i]), "image_id": int(gt["image_id"][i]), "category_id": int(gt["category_id"][i]),
                           "bbox": gt["bbox"][i].tolist(), "area": float(gt["area"][i]), "iscrowd": int(gt["iscrowd"][i])}
                          for i in range(len(gt["id"]))]}
    rj = [{"image_id": int(dt["image_id"][i]), "category_id": int(dt["category_id"][i]), "bbox": dt["bbox"][i].tolist(),
           "score": float(dt["score"][i])} for i in range(len(dt["score"]))]
    (tmp_path / "gt.json").write_text(json.dumps(gj))
    (tmp_path / "res.json").write_text(json.dumps(rj))
    res = EV.evaluate_detection(str(tmp_path / "gt.json"), str(tmp_path / "res.json"), 0.5)
    p, r = _ref_on(gt, dt, img_ids, cats, [0.5])
    st = EV.coco_stats(p, r, [0.5])
    assert res == {"mAP": st[0], "mAP_50": st[0], "precision": st[0], "recall": st[8]}

    g, h = _mot_sequence(np.random.default_rng(9))
    for name, a in (("gt.txt", g), ("res.txt", h)):
        (tmp_path / name).write_text("".join(f"{int(r[0])},{int(r[1])},{float(r[2] + 1)!r},{float(r[3] + 1)!r},{float(r[4])!r},{float(r[5])!r},1,-1,-1,-1\n" for r in a))
    out = EV.evaluate_tracking(str(tmp_path / "gt.txt"), str(tmp_path / "res.txt"))
    ref = ER.mot_ref(EV.load_mot(str(tmp_path / "gt.txt")), EV.load_mot(str(tmp_path / "res.txt")))
    assert set(out) == {"idf1", "mota", "motp", "num_switches", "mostly_tracked", "mostly_lost"}
    for k in ("num_switches", "mostly_tracked", "mostly_lost", "mota", "idf1"):
        assert out[k] == ref[k], k
    assert abs(out["motp"] - ref["motp"]) <= 1e-12 * ref["motp"]


def test_capacity_errors_before_launch(EV):
    from rtmodt_amd import _ffi
    n = 1025
    gt = {"id": np.arange(1, n + 1), "image_id": np.ones(n, np.int64), "category_id": np.ones(n, np.int64),
          "bbox": np.tile([0.0, 0.0, 5.0, 5.0], (n, 1)), "area": np.full(n, 25.0), "iscrowd": np.zeros(n, np.int64)}
    dt = {"image_id": np.array([1]), "category_id": np.array([1]), "bbox": np.array([[0.0, 0.0, 5.0, 5.0]]), "score": np.array([0.5])}
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.coco_eval(gt, dt)
    assert e.value.code == _ffi.E_CAPACITY and "1025 GTs" in e.value.msg
    rows = np.array([[1, i, 0, 0, 5, 5] for i in range(n)], np.float64)
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.mot_eval([(rows, rows[:3])])
    assert e.value.code == _ffi.E_CAPACITY and "frame 1" in e.value.msg
