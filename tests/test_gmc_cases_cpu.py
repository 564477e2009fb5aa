"""CPU: every case of tests/gmc_cases.py reaches, on the restatement (tests/gmc_ref.py), the condition it exists for, so that
tests/test_gpu_gmc_limits.py cannot pass by not exercising its target.  Conditions, not measurements."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmc_cases as K  # noqa: E402
import gmc_ref as G  # noqa: E402


def _estimates(name, masked=True):
    """[(frame, stream, status, debug)] of the frames after the first."""
    return [(f, s, st, dbg) for f, row in enumerate(K.reference(name, masked)) for s, (_, st, dbg) in enumerate(row) if f]


def _statuses(name):
    return [[st for _, st, _ in row] for row in K.reference(name)]


def _reasons(dbg):
    return np.bincount(dbg["blk"]["reason"], minlength=6)


@pytest.mark.parametrize("name", K.NAMES)
def test_first_frame_then_estimates_and_round_0_counts_the_best_score(name):
    """Every case has a FIRST frame and at least one estimate per stream.  Wherever the fit reaches refit round 0, its N is the best
    score: the reason gmc_fit's FEW_INLIERS exit in round 0 has no case."""
    seen = _statuses(name)
    assert len(seen) >= 2 and all(st == G.FIRST for st in seen[0]) and all(st != G.FIRST for row in seen[1:] for st in row)
    for f, s, st, dbg in _estimates(name):
        if st != G.FEW_BLOCKS and dbg["scores"].max() >= K.case(name).cfg.get("min_inliers", G.DEFAULTS["min_inliers"]):
            assert int(dbg["sums"][0][0]) == int(dbg["scores"].max()), (name, f, s)
            assert G.sums_model([int(v) for v in dbg["sums"][0]]) is not None            # D > 0


@pytest.mark.parametrize("name", K.D4_NAMES)
def test_d4_cases_take_the_default_downscale_and_the_row_alignments_they_claim(name):
    c = K.case(name)
    assert c.cfg["downscale"] == G.DEFAULTS["downscale"] == 4
    assert all(st == G.OK for row in _statuses(name)[1:] for st in row)
    res = [K.row_residues(c.streams[s][0], 4, base) for s, base in enumerate(K.staged_bases(c))]
    if name == "d4":
        assert c.streams[0][0].strides[0] == 3 * 384 and res == [{0}] and K.geometry(c)["nb"] == 30      # tight: every row as dwords
        return
    g = K.geometry(c)
    assert (g["h"], g["w"]) == (331, 389) and g["w"] % 4 and g["h"] % 4                   # partial cells right and below
    assert all(sx % 4 and sy % 4 for sx, sy in K.D4_ODD_STEPS)
    pitch = c.streams[0][0].strides[0]
    assert pitch > 3 * g["w"] and pitch % 4 == (1 if name == "d4-streams" else int(name[-1]))
    for r in res:
        assert 0 in r and r - {0}, (name, r)                                              # both paths
    # inside one cell: its four rows are not all of one kind
    for s, base in enumerate(K.staged_bases(c)):
        kinds = [(base + r * pitch) % 4 == 0 for r in range(g["H0"] * 4)]
        assert all(0 < sum(kinds[4 * y:4 * y + 4]) < 4 for y in range(g["H0"])), name
    if name == "d4-streams":
        assert len(c.streams) == 3 and g["h"] % 2 and pitch % 2
        assert len({b % 4 for b in K.staged_bases(c)}) == 3                               # three frame bases, three alignments


def test_d8():
    c = K.case("d8")
    assert c.cfg["downscale"] == 8 and c.cfg["coarse_search"] == 2 and K.geometry(c)["nb"] == 48
    assert _statuses("d8")[1:] == [[G.OK], [G.OK]]


def test_widest_fills_the_coarse_stage():
    c, g = K.case("widest"), K.geometry(K.case("widest"))
    cs = c.cfg["coarse_search"]
    assert cs == 16 and g["W1"] == 960 == G.MAX_W // 4 and g["w"] == G.MAX_W and g["nb"] == 2400
    assert (g["H1"] - 2 * cs) % 4 == 0 and g["H1"] - 2 * cs >= 4                          # whole workgroups of four interior rows: 4 + 2 x 16 = 36 rows in LDS
    for _, _, st, dbg in _estimates("widest"):
        assert st == G.OK and max(abs(v) for v in dbg["coarse"]) > 8 and len(dbg["order"]) > 1024     # beyond the default search; more blocks than threads


@pytest.mark.parametrize("name", ["blocks-4096-d1", "blocks-4096-d2"])
def test_blocks_4096_gives_every_fit_thread_four_blocks(name):
    assert K.geometry(K.case(name))["nb"] == 4096 == G.MAX_BLOCKS and K.geometry(K.case(name))["BX"] == 64
    est = _estimates(name)
    assert len(est) == 2
    for _, _, st, dbg in est:
        assert st == G.OK and len(dbg["order"]) > 3072                                    # so every thread's fourth pass over the points has work
    assert any(dbg["blk"]["reason"][4095] == G.R_VALID for _, _, _, dbg in est)           # the last thread's last block is a valid one, once


@pytest.mark.parametrize("name", ["masks-200", "masks-1024", "masks-edges"])
def test_masks_hit_exactly_the_blocks_of_the_named_boxes(name):
    c = K.case(name)
    m = c.masks[0]
    named = {i: b for i, b in c.extra.items() if isinstance(i, int)}
    union = set().union(*named.values())
    for (f, s, st, dbg), (_, _, _, bare) in zip(_estimates(name), _estimates(name, masked=False)):
        assert st == G.OK
        want = {i for i in union if bare["blk"]["reason"][i] == G.R_VALID}
        assert set(np.nonzero(dbg["blk"]["reason"] == G.R_MASK)[0].tolist()) == want, (name, f)
        other = dbg["blk"]["reason"] != G.R_MASK
        assert np.array_equal(dbg["blk"]["reason"][other], bare["blk"]["reason"][other])
        for i, blocks in named.items():
            assert not blocks or blocks & want, (name, i)                                 # every named box masks a block of its own
    if name == "masks-200":
        assert len(m.xyxy) == 200 and sorted(i for i, b in named.items() if b) == [130, 199]          # the third and the fourth pass of the lane loop
    if name == "masks-1024":
        assert len(m.xyxy) == 1024 and sorted(named) == [1023]                            # the limit; the sixteenth pass, lane 63
    if name == "masks-edges":
        at = np.float32(G.DEFAULTS["mask_conf"])
        assert m.confidence[0] == at and m.confidence[1] < at and m.confidence[1] == np.nextafter(at, np.float32(0))
        dbg = _estimates(name)[0][3]
        assert all(dbg["blk"]["reason"][i] == G.R_VALID for i in c.extra["below"])       # valid blocks under the box just below mask_conf
        assert all(dbg["blk"]["reason"][i] == G.R_VALID for i in c.extra["touched"])     # and next to the two boxes that only touch them
        assert np.isnan(m.xyxy[4:]).any(1).all()


def test_reasons_has_every_block_reason_and_offsets_of_both_signs():
    _, _, st, dbg = _estimates("reasons")[0]
    assert st == G.OK and (_reasons(dbg)[:5] >= 1).all(), _reasons(dbg)
    for k in ("offx", "offy"):
        assert dbg["blk"][k].min() < 0 < dbg["blk"][k].max()
    assert dbg["sums"][1][0] < dbg["sums"][0][0]                                          # what few-inliers-refit-1 stands on


@pytest.mark.parametrize("name,exit_", [("few-inliers-after-hypotheses", "after-hypotheses"), ("few-inliers-refit-1", "refit-1")])
def test_few_inliers_exits(name, exit_):
    c = K.case(name)
    best = K.reasons_best_score()
    assert c.cfg["min_inliers"] == best + (exit_ == "after-hypotheses")
    (_, _, st, dbg), = _estimates(name)
    assert st == G.FEW_INLIERS and K.fit_exit(dbg, c.cfg["min_inliers"]) == exit_ and dbg["scores"].max() == best


def test_mixed_statuses_in_one_call():
    assert _statuses("mixed") == [[G.FIRST] * 3, [G.FEW_INLIERS, G.OK, G.FEW_BLOCKS]]
    assert [K.fit_exit(dbg, K.case("mixed").cfg["min_inliers"]) for _, _, _, dbg in _estimates("mixed")] == ["after-hypotheses", "end", "few-blocks"]


def test_crop_view_ends_on_its_buffer_and_holds_the_copy_s_pixels():
    v, c = K.case("crop-view"), K.case("crop-copy")
    for a, b in zip(v.streams[0], c.streams[0]):
        big = a.base
        assert a.strides[0] == 3 * 165 > 3 * 160 and b.strides[0] == 3 * 160 and np.array_equal(a, b)
        end = a.ctypes.data + (a.shape[0] - 1) * a.strides[0] + 3 * a.shape[1]
        assert end == big.ctypes.data + big.nbytes                                        # h * pitch from its first byte would run 15 bytes past
    assert all(st == G.OK for row in _statuses("crop-view")[1:] for st in row)
