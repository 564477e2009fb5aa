"""The evaluation rules on hand-derived cases, through the NumPy restatement (tests/eval_ref.py),
plus the host-only parts of rtmodt_amd.evaluation: file parsing, writers, summarize, the NumPy helpers."""
import itertools
import json
from types import SimpleNamespace

import numpy as np
import pytest

import eval_ref as ER
from rtmodt_amd import evaluation as EV


def coco(gts, dts, iou_thrs=(0.5,), img_ids=None, cat_ids=None):
    """gts: (image, cat, [x, y, w, h], area, crowd, id); dts: (image, cat, [x, y, w, h], score)."""
    gt = {"image_id": np.array([g[0] for g in gts], np.int64), "category_id": np.array([g[1] for g in gts], np.int64),
          "bbox": np.array([g[2] for g in gts], np.float64).reshape(-1, 4), "area": np.array([g[3] for g in gts], np.float64),
          "iscrowd": np.array([g[4] for g in gts], np.int64), "id": np.array([g[5] for g in gts], np.int64)}
    dt = {"image_id": np.array([d[0] for d in dts], np.int64), "category_id": np.array([d[1] for d in dts], np.int64),
          "bbox": np.array([d[2] for d in dts], np.float64).reshape(-1, 4), "score": np.array([d[3] for d in dts], np.float64)}
    p, r = ER.coco_ref(gt, dt, img_ids, cat_ids, list(iou_thrs))
    return p, r, EV.coco_stats(p, r, list(iou_thrs))


B0, B1, FAR = [0, 0, 10, 10], [20, 0, 10, 10], [50, 50, 10, 10]
# hand-derived COCO cases: (gts, dts, cat_ids); tests/test_gpu_eval.py runs every one through the GPU as well
CASES = {
    "ap_known_answer": ([(1, 1, B0, 100, 0, 1), (1, 1, B1, 100, 0, 2)], [(1, 1, B0, .9), (1, 1, FAR, .8), (1, 1, B1, .7)], None),
    "single": ([(1, 1, B0, 100, 0, 1)], [(1, 1, B0, .9)], None),
    "crowd": ([(1, 1, [0, 0, 100, 100], 10000, 1, 1), (1, 1, [200, 200, 10, 10], 100, 0, 2)],
              [(1, 1, [0, 0, 10, 10], .9), (1, 1, [50, 50, 10, 10], .8), (1, 1, [200, 200, 10, 10], .7)], None),
    "area_ignore": ([(1, 1, [0, 0, 100, 100], 10000, 0, 1), (1, 1, [200, 200, 10, 10], 100, 0, 2)],
                    [(1, 1, [0, 0, 100, 100], .95), (1, 1, [300, 300, 90, 90], .9), (1, 1, [200, 200, 10, 10], .5)], None),
    "max_dets": ([(1, 1, [30 * i, 0, 10, 10], 100, 0, i + 1) for i in range(3)], [(1, 1, [30 * i, 0, 10, 10], .9 - .1 * i) for i in range(3)],
                 None),
    "ties_in_cell": ([(1, 1, B0, 100, 0, 1)], [(1, 1, FAR, .5), (1, 1, B0, .5)], None),
    "ties_across_images": ([(1, 1, B0, 100, 0, 1), (2, 1, B0, 100, 0, 2)], [(2, 1, B0, .5), (1, 1, FAR, .5)], None),
    "equal_iou_last_wins": ([(1, 1, B0, 100, 0, 7), (1, 1, B0, 100, 0, 0)], [(1, 1, B0, .9), (1, 1, B0, .8)], None),
    "category_without_gt": ([(1, 1, B0, 100, 0, 1)], [(1, 1, B0, .9), (1, 2, B0, .9)], [1, 2]),
    "gt_id_zero": ([(1, 1, B0, 100, 0, 0)], [(1, 1, B0, .9), (1, 1, [1, 0, 10, 10], .8)], None),
}
TP1 = 0.9999999999999998                                  # 1 / (1 + eps): the precision of a lone true positive
AP1 = float(np.mean(np.full(101, TP1)))                   # ... averaged over the 101 recall thresholds (0.9999999999999999)


# ---- COCO ------------------------------------------------------------------------------------------------------------
def test_ap_known_answer():
    """Dets .9 hit, .8 miss, .7 hit the other GT: tp = 1,1,2; fp = 0,1,1; rc = .5,.5,1; pr = 1/(1+eps), .5, 2/3, then
    the running max from the right gives 1/(1+eps), 2/3, 2/3.  Recall thresholds 0..0.5 (51 of them) take 0.9999999999999998,
    0.51..1 (50) take 2/3: AP = (51 * 0.9999999999999998 + 50 * 2/3) / 101 = 0.834983498349835."""
    p, r, st = coco(*CASES["ap_known_answer"][:2])
    assert st[0] == 0.834983498349835
    assert p[0, 0, 0, 0, 2] == 0.9999999999999998 and p[0, 100, 0, 0, 2] == 2 / 3
    assert r[0, 0, 0, 2] == 1.0


def test_single_threshold_stats_layout():
    """iouThrs = [0.5]: stats[1] (IoU .5) is the same slice as stats[0]; stats[2] (IoU .75) selects nothing -> -1."""
    _, _, st = coco([(1, 1, B0, 100, 0, 1)], [(1, 1, B0, .9)])
    assert st[0] == st[1] == AP1
    assert st[2] == -1
    assert st[8] == 1.0


def test_crowd_gt_matched_by_several_dets():
    """A crowd GT stays eligible after a match, its IoU uses the det's area as the union, and the dets it takes are
    ignored: only the non-crowd GT counts, one tp -> precision 1/(1+eps) everywhere up to recall 1."""
    crowd = [0, 0, 100, 100]
    p, r, _ = coco([(1, 1, crowd, 10000, 1, 1), (1, 1, [200, 200, 10, 10], 100, 0, 2)],
                   [(1, 1, [0, 0, 10, 10], .9), (1, 1, [50, 50, 10, 10], .8), (1, 1, [200, 200, 10, 10], .7)])
    assert r[0, 0, 0, 2] == 1.0
    assert (p[0, :, 0, 0, 2] == 0.9999999999999998).all()


def test_area_range_ignore_both_sides():
    """'small' (area < 32^2): the large GT is ignored, the det that matches it is ignored through the GT; an unmatched large
    det is ignored by its own w*h.  The small GT + its det give AP 1/(1+eps); recall 1."""
    big, small = [0, 0, 100, 100], [200, 200, 10, 10]
    p, r, st = coco([(1, 1, big, 10000, 0, 1), (1, 1, small, 100, 0, 2)],
                    [(1, 1, big, .95), (1, 1, [300, 300, 90, 90], .9), (1, 1, small, .5)])
    assert r[0, 0, 1, 2] == 1.0 and st[3] == AP1
    # 'all': the unmatched large det is a false positive there
    assert st[0] < AP1


def test_max_dets_truncation():
    """Three GTs, three hits with scores .9 > .8 > .7: maxDets 1 sees one det (recall 1/3), 10 and 100 see all three."""
    gts = [(1, 1, [30 * i, 0, 10, 10], 100, 0, i + 1) for i in range(3)]
    dts = [(1, 1, [30 * i, 0, 10, 10], .9 - .1 * i) for i in range(3)]
    _, r, st = coco(gts, dts)
    assert r[0, 0, 0, 0] == 1 / 3 and r[0, 0, 0, 1] == 1.0 and r[0, 0, 0, 2] == 1.0
    assert st[6] == 1 / 3 and st[7] == st[8] == 1.0


def test_score_ties_broken_by_file_then_image_order():
    """Equal scores: inside a cell the file order decides which det is kept by maxDets=1 (the first, a miss here); across
    images the image order decides the accumulation order (image 1's miss before image 2's hit: pr = 0, 1/2)."""
    _, r, _ = coco([(1, 1, B0, 100, 0, 1)], [(1, 1, FAR, .5), (1, 1, B0, .5)])
    assert r[0, 0, 0, 0] == 0.0 and r[0, 0, 0, 2] == 1.0
    p, _, _ = coco([(1, 1, B0, 100, 0, 1), (2, 1, B0, 100, 0, 2)], [(2, 1, B0, .5), (1, 1, FAR, .5)])
    # order: image 1's miss, image 2's hit -> rc = 0, .5; pr = 0, .5 -> precision .5 up to recall .5, 0 after
    assert p[0, 0, 0, 0, 2] == 0.5 and p[0, 50, 0, 0, 2] == 0.5 and p[0, 51, 0, 0, 2] == 0.0


def test_equal_iou_last_gt_wins():
    """Two identical GTs, the LAST with annotation id 0, and two detections on them.  The .9 detection takes the last GT
    with the maximum IoU -- id 0, so it counts as a false positive -- and the .8 detection takes the first: pr = 0, 1/2.
    Were the first GT taken first, the curve would start at 1/(1+eps)."""
    p, r, _ = coco(*CASES["equal_iou_last_wins"][:2])
    assert p[0, 0, 0, 0, 2] == 0.5 and r[0, 0, 0, 2] == 0.5


def test_category_without_gt_is_minus_one():
    """Category 2 has a det but no GT: npig = 0 -> precision / recall stay -1 and do not enter the means."""
    p, r, st = coco([(1, 1, B0, 100, 0, 1)], [(1, 1, B0, .9), (1, 2, B0, .9)], cat_ids=[1, 2])
    assert (p[:, :, 1] == -1).all() and (r[:, 1] == -1).all()
    assert st[0] == AP1


def test_gt_id_zero_counts_as_unmatched():
    """A det matched to an annotation with id 0 records dtm = 0: it is neither a tp nor ignored (inside the area range),
    so it is a false positive; the GT is still consumed."""
    p, r, _ = coco([(1, 1, B0, 100, 0, 0)], [(1, 1, B0, .9), (1, 1, [1, 0, 10, 10], .8)])
    assert r[0, 0, 0, 2] == 0.0 and (p[0, :, 0, 0, 2] == 0).all()


def test_load_coco_rules(tmp_path):
    g = {"images": [{"id": 3}, {"id": 1}], "categories": [{"id": 5}],
         "annotations": [{"id": 1, "image_id": 1, "category_id": 5, "bbox": [0, 0, 2, 2], "area": 4}]}
    (tmp_path / "g.json").write_text(json.dumps(g))
    (tmp_path / "r.json").write_text(json.dumps([{"image_id": 3, "category_id": 5, "bbox": [0, 0, 1, 1], "score": .5}]))
    gt, dt, img, cat = EV.load_coco(str(tmp_path / "g.json"), str(tmp_path / "r.json"))
    assert img.tolist() == [1, 3] and cat.tolist() == [5] and gt["iscrowd"].tolist() == [0]     # missing iscrowd -> 0
    (tmp_path / "e.json").write_text("[]")
    with pytest.raises(ValueError, match="empty"):
        EV.load_coco(str(tmp_path / "g.json"), str(tmp_path / "e.json"))
    with pytest.raises(ValueError, match="not GT images"):
        dt["image_id"][:] = 99
        EV.coco_eval(gt, dt, img_ids=img, cat_ids=cat)


def test_coco_results_writer():
    d = SimpleNamespace(xyxy=np.array([[1.5, 2.0, 11.5, 22.0]], np.float32), confidence=np.array([.25], np.float32),
                        class_id=np.array([11], np.int32))
    out = EV.coco_results(42, d)
    assert out == [{"image_id": 42, "category_id": 13, "bbox": [1.5, 2.0, 10.0, 20.0], "score": 0.25}]
    assert sorted(set(range(1, 91)) - set(EV.COCO80_TO_91)) == [12, 26, 29, 30, 45, 66, 68, 69, 71, 83]


# ---- exact assignment ------------------------------------------------------------------------------------------------
def _brute(D, V):
    r, c = V.shape
    best = (0, 0.0)
    for perm in itertools.product(*[[-1] + [j for j in range(c) if V[i, j]] for i in range(r)]):
        cols = [j for j in perm if j >= 0]
        if len(cols) != len(set(cols)):
            continue
        key = (len(cols), sum(D[i, j] for i, j in enumerate(perm) if j >= 0))
        if key[0] > best[0] or (key[0] == best[0] and key[1] < best[1]):
            best = key
    return best


@pytest.mark.parametrize("seed", range(12))
def test_assign_lex_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    r, c = int(rng.integers(1, 8)), int(rng.integers(1, 8))
    D = rng.integers(0, 6, (r, c)) / 10.0                 # many ties
    V = rng.random((r, c)) < 0.45
    pairs = ER.assign_lex(D, V)
    card, dsum = _brute(D, V)
    assert len(pairs) == card and abs(sum(D[i, j] for i, j in pairs) - dsum) < 1e-12


def test_assign_lex_matches_scipy_embedding():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(1)
    for _ in range(20):
        r, c = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        D = rng.random((r, c)) * 0.5
        V = rng.random((r, c)) < 0.3
        big = 1e3                                          # motmetrics' expensive-edge embedding
        C = np.where(V, D - big, 0.0)
        ri, ci = opt.linear_sum_assignment(C)
        ref = [(i, j) for i, j in zip(ri, ci) if V[i, j]]
        pairs = ER.assign_lex(D, V)
        assert len(pairs) == len(ref)
        assert abs(sum(D[i, j] for i, j in pairs) - sum(D[i, j] for i, j in ref)) < 1e-9


def test_max_weight_exact():
    W = np.array([[5, 4, 0], [4, 0, 0], [0, 0, 1]])
    assert ER.max_weight(W) == 4 + 4 + 1               # not the greedy 5 + 1


# ---- MOT -------------------------------------------------------------------------------------------------------------
def row(f, i, x, y=0.0, w=10.0, h=10.0):
    return [f, i, x, y, w, h]


def test_switch_counted():
    """GT 1 is followed by hyp 10 then hyp 11: one match, one switch."""
    c = ER.mot_ref([row(1, 1, 0), row(2, 1, 0)], [row(1, 10, 0), row(2, 11, 0)])
    assert (c["num_matches"], c["num_switches"], c["num_misses"], c["num_false_positives"]) == (1, 1, 0, 0)


def test_no_continuation_after_gap():
    """Frame 1: o1-h1.  Frame 2: o1 absent (last_update = 2).  Frame 3: o1 and h1 again, h2 is closer: last_match(o1) = 1
    != last_update = 2, so no continuation; the assignment picks the closer h2 -> a switch."""
    g = [row(1, 1, 0), row(2, 2, 500), row(3, 1, 0)]
    h = [row(1, 1, 0), row(2, 9, 500), row(3, 1, 3), row(3, 2, 0)]
    c = ER.mot_ref(g, h)
    assert c["events"][2] == [("SWITCH", 1.0, 2.0), ("FP", None, 1.0)]
    # without the gap the continuation keeps h1 although h2 is closer
    c2 = ER.mot_ref([row(1, 1, 0), row(2, 1, 0)], [row(1, 1, 0), row(2, 1, 3), row(2, 2, 0)])
    assert c2["events"][1][0] == ("MATCH", 1.0, 1.0)


def test_cardinality_before_distance():
    """o1 is close to h1 (d small) and valid with h2; o2 is valid only with h1.  Minimum sum alone would take (o1, h1);
    maximum cardinality takes (o1, h2) + (o2, h1)."""
    D = np.array([[0.0, 0.4], [0.45, 1.0]])
    V = D <= 0.5
    assert sorted(ER.assign_lex(D, V)) == [(0, 1), (1, 0)]


def test_mostly_tracked_and_lost_at_the_boundaries():
    """o1 tracked 4 of 5 frames (0.8 -> mostly tracked); o2 tracked 1 of 5 (0.2 -> not mostly lost); o3 never (lost)."""
    g, h = [], []
    for f in range(1, 6):
        g += [row(f, 1, 0), row(f, 2, 100), row(f, 3, 200)]
        if f != 5:
            h.append(row(f, 1, 0))
        if f == 1:
            h.append(row(f, 2, 100))
    c = ER.mot_ref(g, h)
    assert (c["mostly_tracked"], c["mostly_lost"]) == (1, 1)


def test_idf1_global_pairing_differs_from_matches():
    """o1 is matched to h1 in frames 1-2; from frame 3 on h2 overlaps o1 as well as h1 does not: the per-frame matches give
    2 (h1) + 3 (h2) but one id can pair with one id only: IDTP = 3 (o1-h2), IDF1 = 6 / 10."""
    g = [row(f, 1, 0) for f in range(1, 6)]
    h = [row(f, 1, 0) for f in (1, 2)] + [row(f, 2, 0) for f in (3, 4, 5)]
    c = ER.mot_ref(g, h)
    assert c["num_matches"] + c["num_switches"] == 5 and c["idtp"] == 3 and c["idf1"] == 0.6


def test_frames_in_one_file_only():
    """Frame 2 has only a hypothesis, frame 3 only a GT: they count as frames, an FP and a miss."""
    c = ER.mot_ref([row(1, 1, 0), row(3, 1, 0)], [row(1, 1, 0), row(2, 1, 0)])
    assert (c["num_frames"], c["num_false_positives"], c["num_misses"], c["num_matches"]) == (3, 1, 1, 1)


def test_load_mot_and_writer_round_trip(tmp_path):
    t = SimpleNamespace(track_id=4, xyxy=np.array([10.5, 20.0, 30.5, 60.0], np.float32), confidence=0.75)
    lines = EV.mot_rows(7, [t])
    assert lines == ["7,4,11.5,21,20,40,0.75,-1,-1,-1"]
    p = tmp_path / "a.txt"
    p.write_text("\n".join(lines + ["8 5 1.5 2.5 3 4", "9,6, 1,1,2,2"]) + "\n")
    a = EV.load_mot(str(p))
    assert a.tolist() == [[7, 4, 10.5, 20.0, 20.0, 40.0], [8, 5, 0.5, 1.5, 3, 4], [9, 6, 0, 0, 2, 2]]
    p.write_text("1,1,0,0,5\n")
    with pytest.raises(ValueError, match="at least 6"):
        EV.load_mot(str(p))
    p.write_text("1,1,0,0,5,5\n1,1,3,3,5,5\n")
    with pytest.raises(ValueError, match="twice"):
        EV.load_mot(str(p))
    p.write_text("1,1,0,x,5,5\n")
    with pytest.raises(ValueError, match="not a number"):
        EV.load_mot(str(p))


# ---- NumPy helpers ---------------------------------------------------------------------------------------------------
def test_confusion_matrix_skips_out_of_range_and_truncates():
    cm = EV.build_confusion_matrix([0, 1, 2, 5, -1, 1], [0, 2, 2, 1, 0], 3)
    assert cm.tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 1]] and cm.dtype == np.int64


def test_tracking_drift():
    out = EV.measure_tracking_drift({1: [(0, 0), (3, 4), (9, 9)], 2: [(0, 0)], 5: [(1, 1)]}, {1: [(0, 0), (0, 0)], 2: [(6, 8)]})
    assert out["per_track"] == {1: 2.5, 2: 10.0}
    assert out["mean_drift_px"] == pytest.approx(5.0)
    assert EV.measure_tracking_drift({}, {1: [(0, 0)]}) == {"mean_drift_px": 0.0, "per_track": {}}
