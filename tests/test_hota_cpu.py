"""CPU: the HOTA restatement (tests/hota_ref.py) against the truth -- hand-worked literals, scipy's
linear_sum_assignment (the solver TrackEval calls) for the per-frame matching, and the invariants that hold by construction.
The GPU tests (tests/test_gpu_hota.py) then require the kernels to be bit-identical with the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hota_ref as HR  # noqa: E402

BOX = [10.0, 20.0, 50.0, 80.0]


def rows(spec):
    """[(frame, id, box)] -> (n, 6)"""
    return np.array([[f, i, *b] for f, i, b in spec], np.float64).reshape(-1, 6)


def test_alphas_are_trackevals_nineteen():
    assert len(HR.ALPHAS) == 19 and HR.ALPHAS[0] == 0.05 and HR.EPS == 2.0 ** -52


def test_perfect_tracking_scores_one_everywhere():
    gt = rows([(f, i, [100.0 * i + 3 * f, 5.0 * f, 40, 60]) for f in range(1, 7) for i in (1, 2, 3)])
    r = HR.record(HR.hota_ref(gt, gt.copy()))
    for k in HR.FLOAT_FIELDS:
        assert np.array_equal(r[k], np.ones(19)), k
    assert r["HOTA_TP"].tolist() == [18] * 19 and not r["HOTA_FN"].any() and not r["HOTA_FP"].any()
    assert r["HOTA(0)"] == 1.0 and r["LocA(0)"] == 1.0 and r["HOTALocA(0)"] == 1.0 and r["mean"]["HOTA"] == 1.0


def test_one_id_change_halves_the_association():
    """One GT track of 4 frames with exact boxes, the hypothesis id changing after frame 2: TP = 4 and DetA = 1; every TP has
    TPA 2, FNA 2, FPA 0, so AssA = 0.5 and HOTA = sqrt(0.5)."""
    gt = rows([(f, 1, BOX) for f in (1, 2, 3, 4)])
    hyp = rows([(1, 7, BOX), (2, 7, BOX), (3, 9, BOX), (4, 9, BOX)])
    c = HR.hota_ref(gt, hyp)
    assert c["pmc"] == {(1.0, 7.0): 2.0, (1.0, 9.0): 2.0}
    r = HR.record(c)
    assert r["HOTA_TP"].tolist() == [4] * 19 and np.array_equal(r["DetA"], np.ones(19))
    assert np.array_equal(r["AssA"], np.full(19, 0.5)) and np.array_equal(r["HOTA"], np.full(19, np.sqrt(0.5)))
    assert np.array_equal(r["AssRe"], np.full(19, 0.5)) and np.array_equal(r["AssPr"], np.ones(19)) and np.array_equal(r["LocA"], np.ones(19))


def test_no_hypotheses_and_no_ground_truth():
    """No hypotheses: FN = the GT rows and every score 0; no GT is the mirror case.  (LocA alone is 1 there: TrackEval's
    max(1e-10, 0) / max(1e-10, 0) guard; a combination weights it by TP and gives 0.)"""
    gt = rows([(f, i, BOX) for f in (1, 2, 3) for i in (1, 2)])
    none = np.zeros((0, 6))
    for g, h, miss, extra in ((gt, none, 6, 0), (none, gt, 0, 6)):
        c = HR.hota_ref(g, h)
        r = HR.record(c)
        assert r["HOTA_TP"].tolist() == [0] * 19 and r["HOTA_FN"].tolist() == [miss] * 19 and r["HOTA_FP"].tolist() == [extra] * 19
        for k in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr"):
            assert not r[k].any(), k
        assert np.array_equal(r["LocA"], np.ones(19)) and r["HOTA(0)"] == 0.0
        assert not HR.combine([c])["LocA"].any()


@pytest.mark.parametrize("iou,height", [(0.5, 5.0), (0.25, 2.5), (0.75, 7.5)])
def test_threshold_that_equals_the_iou_counts(iou, height):
    """A pair of boxes with IoU exactly 0.5 / 0.25 / 0.75 is a TP up to the alpha that equals it and an FN + FP above:
    np.arange(0.05, 0.99, 0.05) rounds 0.75 to 0.7500000000000001, which the `- eps` rule absorbs."""
    gt = rows([(1, 1, [0, 0, 10, 10])])
    hyp = rows([(1, 1, [0, 0, 10, height])])
    assert HR.box_iou(gt[0, 2:], hyp[0, 2:]) == iou
    idx = int(np.argmin(np.abs(HR.ALPHAS - iou)))
    assert abs(HR.ALPHAS[idx] - iou) < 1e-15
    c = HR.hota_ref(gt, hyp)
    want = (np.arange(19) <= idx).astype(np.int64)
    assert np.array_equal(c["HOTA_TP"], want) and np.array_equal(c["HOTA_FN"], 1 - want) and np.array_equal(c["HOTA_FP"], 1 - want)
    assert np.array_equal(c["loc_sum"], want * iou)
    if iou == 0.75:
        assert HR.ALPHAS[idx] > iou                             # the case the rule exists for


def scipy_pairs(fr):
    from scipy.optimize import linear_sum_assignment
    score = np.zeros((fr["nO"], fr["nH"]))
    for i, j, sc in fr["edges"]:
        score[i, j] = sc
    r, c = linear_sum_assignment(-score)
    return sorted((int(i), int(j)) for i, j in zip(r, c) if score[i, j] > 0), score


def test_matching_equals_scipy_pair_for_pair():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(11)
    contested = 0
    for k in range(4):
        gt, hyp = HR.synth_sequence(rng, 24, 10, jitter=6.0, fp=0.3)
        hyp = np.concatenate([hyp, hyp[::3] + np.array([0, 1000, 4.0, -3.0, 2.0, 1.0])])      # near duplicates: contested frames
        c = HR.hota_ref(gt, hyp)
        for fr in c["frames"]:
            want, _ = scipy_pairs(fr)
            assert fr["pairs"] == want, (k, fr["frame"])
            contested += len(HR.split_edges(fr["edges"])[1])
    assert contested > 200                                      # the solver, not only the isolated-edge rule, was compared


def test_tie_heavy_total_score_equals_scipy():
    """Integer-grid boxes: many equal scores, so the optimum is not unique and the pairs may differ; the total may not.
    1e-9 is far above the rounding of a sum of at most 256 scores <= 1 and far below any real gap."""
    pytest.importorskip("scipy")
    rng = np.random.default_rng(12)
    ties = 0
    for k in range(3):
        gt, hyp = HR.synth_sequence(rng, 20, 12, jitter=8.0, fp=0.4, grid=20.0)
        hyp = np.concatenate([hyp, hyp[::2] + np.array([0, 1000, 20.0, 0, 0, 0])])
        tg, th = HR.tie_sequence(rng, 20, 3, 2 + k, first_id=5000)      # clusters in which every score is the same
        tg[:, 2] += 2000.0
        th[:, 2] += 2000.0
        gt, hyp = np.concatenate([gt, tg]), np.concatenate([hyp, th])
        c = HR.hota_ref(gt, hyp)
        for fr in c["frames"]:
            want, score = scipy_pairs(fr)
            got = sum(score[i, j] for i, j in fr["pairs"])
            assert abs(got - sum(score[i, j] for i, j in want)) <= 1e-9, (k, fr["frame"])
            assert len(set(i for i, _ in fr["pairs"])) == len(fr["pairs"]) == len(set(j for _, j in fr["pairs"]))
            sc = [e[2] for e in fr["edges"]]
            ties += len(sc) - len(set(sc))
    assert ties > 500


def test_invariants_hold_by_construction():
    rng = np.random.default_rng(13)
    cs = [HR.hota_ref(*HR.synth_sequence(rng, 20, 6)) for _ in range(3)]
    for c in cs:
        r = HR.record(c)
        # sqrt rounds once (2^-53 relative), squaring doubles that and rounds again: 3 * 2^-53 of the product at most
        assert np.all(np.abs(r["HOTA"] ** 2 - r["DetA"] * r["AssA"]) <= 4 * 2.0 ** -53 * r["DetA"] * r["AssA"])
        assert np.array_equal(r["HOTA_TP"] + r["HOTA_FN"], np.full(19, r["HOTA_TP"][0] + r["HOTA_FN"][0]))
        assert np.all(np.diff(r["HOTA_TP"]) <= 0)
    both = HR.combine(cs)
    summed = HR.record({k: cs[0][k] + cs[1][k] + cs[2][k] for k in HR.SUM_FIELDS}, combined=True)
    for k in HR.SUM_FIELDS + HR.FLOAT_FIELDS:
        assert np.array_equal(both[k], summed[k]), k
    assert both["HOTA_TP"].tolist() == sum(c["HOTA_TP"] for c in cs).tolist()


def test_package_formulae_equal_the_restatement(pkg):
    """rtmodt_amd.evaluation.hota_record / hota_combine (NumPy, no GPU) on the restatement's sums."""
    EV = pkg.evaluation
    rng = np.random.default_rng(14)
    cs = [HR.hota_ref(*HR.synth_sequence(rng, 16, 5)) for _ in range(2)] + [HR.hota_ref(np.zeros((0, 6)), rows([(1, 1, BOX)]))]
    recs = [EV.hota_record(*[c[k] for k in HR.SUM_FIELDS]) for c in cs]
    for got, want in list(zip(recs, [HR.record(c) for c in cs])) + [(EV.hota_combine(recs), HR.combine(cs))]:
        for k in HR.SUM_FIELDS + HR.FLOAT_FIELDS:
            assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
        assert got["mean"] == want["mean"] and all(got[k] == want[k] for k in ("HOTA(0)", "LocA(0)", "HOTALocA(0)"))
    assert np.array_equal(EV.HOTA_ALPHAS, HR.ALPHAS)
