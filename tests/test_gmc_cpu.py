"""CPU: the camera-motion restatement (tests/gmc_ref.py, the rules of csrc/gmc.hip) checked against warps that are known by
construction, hand-worked literal cases, and BoT-SORT's restatement fed the estimated warps.  PARITY UNPINNED: OpenCV and BoT-SORT's
GMC are installed nowhere this runs."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import botsort_ref as B  # noqa: E402
import gmc_ref as G  # noqa: E402

H, W, D = 360, 640, 2
CENTRE = ((W - 1) / 2, (H - 1) / 2)
#: the rotation at which the frame's corner moves by (search - 1) level-0 pixels, the farthest a valid block may go (defaults, 640x360, d = 2)
ROT_LIMIT = math.degrees((G.DEFAULTS["search"] - 1) * D / math.hypot(*CENTRE))
#: twice the largest corner error measured at seed 0 of test_accuracy_within_the_coarse_range (0.064 px); DESIGN.md section 23
BOUND = 0.128
#: the same for test_accuracy_at_translations_up_to_100_px (seed 0: 0.05966 px)
BOUND_100 = 0.1193


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32).tolist()


# ------------------------------------------------------------------------------------------------------------ literal cases
@pytest.mark.parametrize("d,h,w", [(1, 96, 160), (2, 192, 320), (4, 384, 640), (8, 768, 1280)])
def test_exact_translation_gives_the_exact_warp(d, h, w):
    cv = G.canvas(h + 32 * d, w + 32 * d, 3)
    ref = G.GmcRef(downscale=d)
    assert ref.estimate(G.crop(cv, 16 * d, 16 * d, h, w))[1] == G.FIRST
    warp, status, dbg = ref.estimate(G.crop(cv, 16 * d - 4 * d, 16 * d + 8 * d, h, w))       # the content moves by (4d, -8d)
    G.assert_textured(dbg, ref.cfg["min_texture"])
    assert status == G.OK and dbg["coarse"] == (1, -2) and len(dbg["order"]) >= 20
    assert _bits(warp) == _bits([1, 0, 4 * d, 0, 1, -8 * d])
    assert (dbg["blk"]["sad"] == 0).all() and (dbg["blk"]["offx"] == 0).all() and (dbg["blk"]["offy"] == 0).all()
    assert dbg["inl"].all() and dbg["model"][2].tolist() == [1.0, 0.0, 64.0 * d, -128.0 * d]


def test_hand_worked_integer_sums():
    """Q = [[1, -1], [1, 1]] P + (10, 20): N 4, SP (200, 200), SQ (40, 480), S(P.Q) 0 + 11000 + 12000 + 23000, S(PxQ) 0 + 12000 + 9000
    + 21000, S|P|^2 0 + 10000 + 10000 + 20000; A = 4 x 46000 - (8000 + 96000), B = 4 x 42000 - (96000 - 8000), D = 4 x 40000 - 80000."""
    P = np.asarray([[0, 0], [100, 0], [0, 100], [100, 100]], np.int64)
    Q = np.asarray([[10, 20], [110, 120], [-90, 120], [10, 220]], np.int64)
    s = G.int_sums(P, Q, np.ones(4, bool))
    assert s == [4, 200, 200, 40, 480, 46000, 42000, 40000]
    assert G.sums_model(s) == (1.0, 1.0, 10.0, 20.0)
    assert G.two_point_model(P[1], P[2], Q[1], Q[2]) == (1.0, 1.0, 10.0, 20.0)
    assert G.sums_model([3, 30, 30, 0, 0, 0, 0, 600]) is None                    # three times the same point: D = 3 x 600 - 1800 = 0
    assert G.inliers((1.0, 1.0, 10.0, 20.0), P, Q + np.asarray([[0, 0], [3, 4], [3, 5], [0, 0]]), 25.0).tolist() == [True, True, False, True]


def test_subpixel_division_literals():
    assert G.subpixel(10, 4, 6) == 4 and G.subpixel(6, 4, 10) == -4              # 32 / 8
    assert G.subpixel(9, 4, 8) == 1                                              # 8 / 9 rounds up
    assert G.subpixel(20, 3, 18) == 1 and G.subpixel(18, 3, 20) == -1            # 16 / 32: half goes away from zero
    assert G.subpixel(5, 5, 5) == 0 and G.subpixel(3, 5, 4) == 0                  # the denominator is not positive
    assert G.subpixel(20, 5, 0) == 8 and G.subpixel(0, 5, 20) == -8              # 160 / 10 clamped
    assert G.subpixel(10, 0, 6) == 0                                             # an exact match has no sub-pixel part


def test_tie_rule_literals():
    def table(r, zeros):
        t = np.full((2 * r + 1, 2 * r + 1), 9, np.int64)
        for dx, dy in zeros:
            t[dy + r, dx + r] = 0
        return t
    assert G.argmin_shift(np.full((5, 5), 7), 2) == (0, 0)                       # all equal: the smallest dx^2 + dy^2
    assert G.argmin_shift(table(2, [(2, 0), (1, 1)]), 2) == (1, 1)               # 4 against 2
    assert G.argmin_shift(table(2, [(1, 0), (0, 1)]), 2) == (1, 0)               # same radius: the smaller dy
    assert G.argmin_shift(table(2, [(1, 0), (-1, 0)]), 2) == (-1, 0)             # same dy: the smaller dx
    assert G.argmin_shift(table(2, [(0, -1), (1, 0)]), 2) == (0, -1)


def test_generator_first_pairs():
    """seed 1, k 0: x = 1664525 + 1013904223 = 1015568748, >> 16 = 15496, % 100 = 96; x = 1586005467, >> 16 = 24200, % 99 = 44."""
    assert [G.lcg_pair(1, k, 100) for k in range(4)] == [(96, 44), (30, 95), (64, 43), (98, 93)]
    assert G.lcg_pair(0xFFFFFFFF, 255, 4096) == (2008, 1055)
    for n in (2, 3, 17):
        for k in range(64):
            i, j = G.lcg_pair(5, k, n)
            assert 0 <= i < n and 0 <= j < n and i != j


# ------------------------------------------------------------------------------------------------------------ known warps
def _known_warp_errors(seed, t_max, n=3, **cfg):
    rng = np.random.default_rng(seed)
    cv = G.canvas(H + 260, W + 260, 100 + seed)
    out = []
    for _ in range(n):
        deg, scale = rng.uniform(-ROT_LIMIT, ROT_LIMIT), rng.uniform(0.98, 1.02)
        tx, ty = rng.uniform(-t_max, t_max, 2)
        truth = G.similarity(deg, scale, tx, ty, centre=CENTRE)
        ref = G.GmcRef(downscale=D, **cfg)
        ref.estimate(G.crop(cv, 130, 130, H, W))
        warp, status, dbg = ref.estimate(G.sample(cv, truth, H, W, (130, 130)))
        G.assert_textured(dbg, ref.cfg["min_texture"])
        out.append((G.corner_error(warp, truth, H, W), status, (round(tx), round(ty))))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_accuracy_within_the_coarse_range(seed):
    """Rotation up to the derived limit (0.94 degrees here), scale 0.98..1.02, translation up to +-60 px: inside the 64 px the coarse
    stage reaches at d = 2 (8 level-1 pixels = 32 level-0 pixels).  Largest corner error per seed, measured: 0.064, 0.069, 0.061,
    0.079, 0.094, 0.045 px; the bound is twice seed 0's, and far below d / 2 = 1 px: the sub-pixel step pays for itself."""
    errs = _known_warp_errors(seed, 60.0)
    print("corner errors", errs)
    assert all(st == G.OK for _, st, _ in errs)
    assert max(e for e, _, _ in errs) <= BOUND and BOUND < D / 2


@pytest.mark.parametrize("seed", range(6))
def test_accuracy_at_translations_up_to_100_px(seed):
    """The cases the issue sets: rotation up to the derived limit, scale 0.98..1.02, translation up to +-100 px at 640x360, d = 2.
    100 px are 12.5 level-1 pixels, beyond the default coarse_search of 8 (64 px at d = 2), so the estimator runs with coarse_search
    = 16, the widest (128 px).  Largest corner error per seed, measured: 0.0597, 0.1075, 0.0355, 0.0593, 0.0882, 0.0704 px; the bound
    is twice seed 0's, and below d / 2 = 1 px."""
    errs = _known_warp_errors(seed, 100.0, coarse_search=16)
    print("corner errors", errs)
    assert all(st == G.OK for _, st, _ in errs)
    assert max(e for e, _, _ in errs) <= BOUND_100 and BOUND_100 < D / 2


def test_default_coarse_search_falls_back_beyond_its_reach():
    """coarse_search = 8 reaches 64 px at d = 2: a pan of 90 px gives the identity and says so, not a wrong warp."""
    cv = G.canvas(H + 200, W + 200, 4)
    ref = G.GmcRef(downscale=D)
    ref.estimate(G.crop(cv, 100, 100, H, W))
    warp, status, _ = ref.estimate(G.crop(cv, 10, 100, H, W))
    assert status in (G.FEW_BLOCKS, G.FEW_INLIERS) and _bits(warp) == _bits(G.IDENTITY)
    wide = G.GmcRef(downscale=D, coarse_search=16)
    wide.estimate(G.crop(cv, 100, 100, H, W))
    warp, status, _ = wide.estimate(G.crop(cv, 10, 100, H, W))
    assert status == G.OK and _bits(warp) == _bits([1, 0, 90, 0, 1, 0])


# ------------------------------------------------------------------------------------------------------------ foreground
def _foreground_pair(seed=11):
    """Background moving by (+10, -6), two 240 x 144 rectangles (30 % of the frame) with their own texture moving by (+14, -10): (+4, -4) against
    the background, inside the block search, so their blocks are measured and it is the fit that has to leave them out."""
    bg, fg = G.canvas(H + 80, W + 80, seed), G.canvas(H + 80, W + 80, seed + 1, smooth=5)
    rects = np.asarray([[40, 30, 280, 174], [350, 190, 590, 334]], np.float32)
    f0, f1 = G.crop(bg, 40, 40, H, W), G.crop(bg, 30, 46, H, W)
    moved = rects + np.asarray([14, -10, 14, -10], np.float32)
    for r, m in zip(rects.astype(int), moved.astype(int)):
        f0[r[1]:r[3], r[0]:r[2]] = fg[r[1]:r[3], r[0]:r[2]]
        f1[m[1]:m[3], m[0]:m[2]] = fg[r[1]:r[3], r[0]:r[2]]
    return f0, f1, rects, moved, G.similarity(tx=10.0, ty=-6.0)


def _blocks_inside(rects, bx_n, by_n, d):
    out = []
    for by in range(by_n):
        for bx in range(bx_n):
            x0, y0 = 16 * d * bx, 16 * d * by
            if any(r[0] <= x0 and r[1] <= y0 and x0 + 16 * d <= r[2] and y0 + 16 * d <= r[3] for r in rects):
                out.append(by * bx_n + bx)
    return out


@pytest.mark.parametrize("masked", [True, False])
def test_foreground_objects_do_not_move_the_warp(masked):
    f0, f1, rects, moved, truth = _foreground_pair()
    assert (rects[:, 2] - rects[:, 0]).dot(rects[:, 3] - rects[:, 1]) / (H * W) == pytest.approx(0.30)
    ref = G.GmcRef(downscale=D)
    ref.estimate(f0)
    boxes = np.concatenate([rects, moved])                   # where the objects were and where they are
    warp, status, dbg = ref.estimate(f1, boxes if masked else None, np.ones(4, np.float32) if masked else None)
    on = _blocks_inside(rects, W // D // 16, H // D // 16, D)
    assert status == G.OK and len(on) >= 20
    assert G.corner_error(warp, truth, H, W) <= BOUND
    if masked:
        assert (dbg["blk"]["reason"][on] != G.R_VALID).all() and (dbg["blk"]["reason"][on] == G.R_MASK).sum() >= 10
    else:
        assert (dbg["blk"]["reason"][on] == G.R_VALID).sum() >= 10           # they were measured, and they moved consistently ...
        inl = set(dbg["order"][dbg["inl"][1].astype(bool)].tolist())
        assert not inl & set(on)                                              # ... yet no hypothesis kept one


# ------------------------------------------------------------------------------------------------------------ fallbacks
def test_fallbacks_give_the_identity_with_their_status(pkg):
    cv = G.canvas(H + 40, W + 40, 5)
    f0, f1 = G.crop(cv, 20, 20, H, W), G.crop(cv, 14, 24, H, W)
    got = {}
    ref = G.GmcRef(downscale=D)
    got["first"] = ref.estimate(f0)
    flat = G.GmcRef(downscale=D)
    flat.estimate(np.full((H, W, 3), 128, np.uint8))
    got["flat"] = flat.estimate(np.full((H, W, 3), 128, np.uint8))
    got["masked"] = ref.estimate(f1, np.asarray([[0, 0, W, H]], np.float32), np.ones(1, np.float32))
    halves = G.GmcRef(downscale=D, min_inliers=100)
    halves.estimate(f0)
    apart = f0.copy()
    apart[:, :W // 2 - 4], apart[:, W // 2 + 4:] = f0[:, 4:W // 2], f0[:, W // 2:W - 4]      # the left half goes left, the right half right
    got["halves"] = halves.estimate(apart)
    assert [got[k][1] for k in ("first", "flat", "masked", "halves")] == [G.FIRST, G.FEW_BLOCKS, G.FEW_BLOCKS, G.FEW_INLIERS]
    assert set(got["flat"][2]["blk"]["reason"].tolist()) <= {G.R_WINDOW, G.R_TEXTURE}
    assert set(got["masked"][2]["blk"]["reason"].tolist()) <= {G.R_WINDOW, G.R_MASK}
    assert 12 <= got["halves"][2]["scores"].max() < 100 and len(got["halves"][2]["order"]) >= 100
    check = pkg._ffi.lib().rtmodt_botsort_check_warp
    for k, (warp, _, _) in got.items():
        assert _bits(warp) == _bits(G.IDENTITY), k
        assert check(pkg._ffi.ptr(np.ascontiguousarray(warp)), 1) == 0


def test_scale_outside_the_range_falls_back():
    P = np.asarray([[x, y] for y in range(0, 4096, 512) for x in range(0, 4096, 512)], np.int64)
    for scale, status in ((3, G.BAD_SCALE), (2, G.OK)):
        f = G.fit(P, scale * P + 7, 16, 1, 8.0, 1.5, 16, 12)
        assert f["status"] == status and (_bits(f["warp"]) == _bits(G.IDENTITY)) == (status != G.OK)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_gmc_scene_keeps_two_identities_with_the_estimated_warps():
    """botsort_ref.gmc_scene rendered as frames: BoT-SORT's restatement fed the warps estimated from the pixels (the objects masked
    by the frame's detections) holds the two identities through the pan, as it does with the true warps; without a warp it
    fragments, asserted as tests/test_botsort_cpu.py asserts it."""
    scene = B.gmc_scene()
    frames = G.gmc_scene_frames(scene)
    est, with_warp, without = G.GmcRef(downscale=D), B.BotSortRef(), B.BotSortRef()
    for img, (xy, cf, cl, _, truth) in zip(frames, scene):
        warp, status, dbg = est.estimate(img, xy, cf)
        if status != G.FIRST:
            G.assert_textured(dbg, est.cfg["min_texture"])
            assert status == G.OK and G.corner_error(warp, truth, *img.shape[:2]) <= BOUND
        with_warp.update(xy, cf, cl, None, warp)
        without.update(xy, cf, cl, None, None)
    assert [t.id for t in with_warp.tracks] == [1, 2] and with_warp.next_id == 3
    assert without.next_id > 10 and all(t.flag != B.TRACKED for t in without.tracks)
