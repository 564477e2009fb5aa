"""CPU: the BoT-SORT restatement (tests/botsort_ref.py) checked against independent forms -- hand-worked literal cases, a dense 8x8
float64 Kalman filter, SciPy's Hungarian method on the dense gain matrix -- and the scenes of the GPU suite
(tests/test_gpu_botsort.py) shown to have a unique optimum in every frame and to exercise camera-motion compensation, appearance
and score fusion.  PARITY UNPINNED: BoT-SORT and boxmot are installed nowhere this runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import botsort_ref as R  # noqa: E402

F32 = np.float32
BOX = np.asarray([[10, 10, 40, 70]], F32)
FAR = np.asarray([[200, 10, 230, 70], [300, 10, 330, 70], [400, 10, 430, 70]], F32)


def _one(conf, box=BOX):
    return box, np.asarray([conf], F32), np.zeros(1, np.int32)


def _none():
    return np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32)


def _state(r):
    return [(t.id, t.flag, t.tsu) for t in r.tracks]


# ------------------------------------------------------------------------------------------------------------ literal cases
def test_split_is_strict_at_both_thresholds():
    up = lambda v: np.nextafter(F32(v), F32(1))            # noqa: E731
    r = R.BotSortRef(new_track_thresh=0.0)
    r.update(FAR, np.asarray([F32(0.6), up(0.6), F32(0.9)], F32), np.zeros(3, np.int32))
    assert [tuple(t.box) for t in r.tracks] == [tuple(FAR[1]), tuple(FAR[2])]         # conf == track_high_thresh: not high, no birth
    r = R.BotSortRef()
    r.update(*_one(0.9))
    seen = []
    for conf in (F32(0.1), F32(0.6), up(0.1), np.nextafter(F32(0.6), F32(0))):
        r.update(*_one(conf))
        seen.append((r.tracks[0].flag, r.tracks[0].tsu))
        if r.tracks[0].flag == R.LOST:                       # bring it back for the next probe
            r.update(*_one(0.9))
    # at track_low_thresh: in neither set; at track_high_thresh: in neither set; just above low / just below high: low, second association
    assert seen == [(R.LOST, 1), (R.LOST, 1), (R.TRACKED, 0), (R.TRACKED, 0)] and r.next_id == 2


def test_new_track_thresh_is_greater_or_equal():
    r = R.BotSortRef()
    conf = np.asarray([F32(0.7), np.nextafter(F32(0.7), F32(0)), F32(0.65)], F32)
    r.update(FAR, conf, np.zeros(3, np.int32))
    assert [tuple(t.box) for t in r.tracks] == [tuple(FAR[0])] and r.next_id == 2     # high (> 0.6) all three; only conf >= 0.7 is born


def test_first_frame_activation_and_deletion_of_an_unmatched_new_track():
    r = R.BotSortRef()
    assert r.update(*_one(0.9)) == [0] and _state(r) == [(1, R.TRACKED, 0)]             # the stream's first frame: activated at once
    both = np.concatenate([BOX, FAR[:1]])
    assert r.update(both, np.full(2, 0.9, F32), np.zeros(2, np.int32)) == [0]            # frame 2: a birth is new, not returned
    assert _state(r) == [(1, R.TRACKED, 0), (2, R.NEW, 0)]
    assert r.update(*_one(0.9)) == [0] and _state(r) == [(1, R.TRACKED, 0)]             # unmatched on its second frame: deleted
    r.update(both, np.full(2, 0.9, F32), np.zeros(2, np.int32))
    assert r.update(both, np.full(2, 0.9, F32), np.zeros(2, np.int32)) == [0, 1]         # matched on its second frame: tracked
    assert _state(r) == [(1, R.TRACKED, 0), (3, R.TRACKED, 0)] and r.tracks[1].start == 4 and r.tracks[1].age == 1


def test_lost_track_dies_at_track_buffer_plus_one():
    for buf in (1, 4):
        r = R.BotSortRef(track_buffer=buf)
        r.update(*_one(0.9))
        alive = []
        for _ in range(buf + 2):
            assert r.update(*_none()) == []                 # a lost track is not returned
            alive.append([t.flag for t in r.tracks])
        assert alive == [[R.LOST]] * buf + [[], []] and r.next_id == 2 and r.frame_count == buf + 3


def test_lost_track_is_reactivated_with_its_id():
    r = R.BotSortRef(track_buffer=5)
    r.update(*_one(0.9))
    r.update(*_none())
    r.update(*_none())
    assert _state(r) == [(1, R.LOST, 2)]
    assert r.update(*_one(0.9)) == [0] and _state(r) == [(1, R.TRACKED, 0)] and r.tracks[0].last == 4 and r.tracks[0].start == 1


def _duplicate_case(start_of_second):
    """Track 1 stands at x = 100 and is lost from frame 3 on; track 2 is born far away in frame 2, tracked from frame 3.  Then track 2
    is put 2 px beside track 1 by hand and matched there in frame 5: IoU 38 / 42 = 0.905, distance 0.095 < 0.15."""
    r = R.BotSortRef()
    a, b = np.asarray([[100, 50, 140, 130]], F32), np.asarray([[300, 50, 340, 130]], F32)
    r.update(*_one(0.9, a))
    r.update(np.concatenate([a, b]), np.full(2, 0.9, F32), np.zeros(2, np.int32))
    r.update(*_one(0.9, b))
    r.update(*_one(0.9, b))
    assert _state(r) == [(1, R.LOST, 2), (2, R.TRACKED, 0)] and [t.start for t in r.tracks] == [1, 2]
    t2 = r.tracks[1]
    t2.mean[0] = r.tracks[0].mean[0] + F32(2)
    t2.mean[4:] = 0
    t2.start = start_of_second
    near = np.asarray([[102, 50, 142, 130]], F32)
    r.update(*_one(0.9, near))
    return [(t.id, t.flag) for t in r.tracks]


def test_duplicate_rule_keeps_the_older_and_drops_the_tracked_one_on_a_tie():
    assert _duplicate_case(2) == [(1, R.LOST)]             # lost since frame 1 is older than tracked since frame 2: the tracked one goes
    assert _duplicate_case(1) == [(1, R.LOST)]             # a tie: the tracked one goes, as published
    assert _duplicate_case(0) == [(2, R.TRACKED)]          # the tracked one is older: the lost one goes


def test_integer_feature_step_by_hand():
    # birth: v = 128 f = (384, -512, 0, 0), r = isqrt(147456 + 262144) = 640
    #   s16 = (16256 * 384 + 320) // 640 = 9754, -((16256 * 512 + 320) // 640) = -13005; s8 = (127 * 384 + 320) // 640 = 76, -((127 * 512 + 320) // 640) = -102
    s16, s8 = R.feat_step(None, [3, -4, 0, 0])
    assert (s16, s8) == ([9754, -13005, 0, 0], [76, -102, 0, 0])
    # match: v = 9 s16 + 128 f = (87786, -117045 + 640, 0, -1536), sum v^2 = 21258865117, r = 145804 (145804^2 = 21258806416 <= n2 < 145805^2)
    #   s16 = (16256 * 87786 + 72902) // 145804 = 9787, -((16256 * 116405 + 72902) // 145804) = -12978, -((16256 * 1536 + 72902) // 145804) = -171
    s16, s8 = R.feat_step(s16, [0, 5, 0, -12])
    assert 145804 ** 2 <= 87786 ** 2 + 116405 ** 2 + 1536 ** 2 < 145805 ** 2
    assert (s16, s8) == ([9787, -12978, 0, -171], [76, -101, 0, -1])
    assert R.feat_step(None, [0, 0, 0, 0]) == ([0] * 4, [0] * 4) and R.feat_step([0] * 4, [0] * 4) == ([0] * 4, [0] * 4)   # r == 0
    # the 16-bit state moves where an 8-bit one would stand still: 9 * 76 + 5 = 689 -> 127 * 689 / ... rounds back to 76
    n16, n8 = R.feat_step([9754, -13005, 0, 0], [4, -4, 0, 0])
    assert n16[0] > 9754 and n8[0] in (76, 77)
    s16, s8 = R.feat_step(None, [127] + [0] * 63)
    assert s16[0] == R.FEAT_NORM and s8[0] == 127


# ------------------------------------------------------------------------------------------------------------------ filter
MEASURED_MEAN, MEASURED_COV = 1.82e-7, 7.91e-7


def test_two_block_filter_equals_dense_float64_filter():
    """The published 8-state filter as dense float64 8x8 matrices (F, H, Q, R as published, P - K H P, the warp as kron(I4, R) with t
    on the centre) against the float32 two-block form, over 300 steps of predict, warp (a rotation of up to 4 degrees, a scale of
    0.97 .. 1.03 and a translation of up to 6 px, new every step) and update (every fifth step is a miss).  No tolerance was fixed in
    advance.  Measured, seed 0: the largest |difference| relative to the largest magnitude of the float64 quantity is 1.82e-7 for the
    mean and 7.91e-7 for the covariance (seeds 1..5: at most 2.1e-7 and 9.5e-7).  Asserted: four times the measured values; the
    margin covers the seeds not tried.  The dense filter's entries outside the two blocks stay below 1e-9 (they are exactly 0)."""
    rng = np.random.default_rng(0)
    Fm = np.eye(8)
    for k in range(4):
        Fm[k, 4 + k] = 1.0
    H = np.eye(4, 8)
    mean, cov = R.kf_init(R.box_to_xywh(np.asarray([100, 50, 140, 130], F32)))
    x, P = mean.astype(np.float64), R.dense_cov(cov)
    wp, wv = float(R.WP), float(R.WV)
    inblock = np.zeros((8, 8), bool)
    for blk in R.BLOCK_MEAN:
        inblock[np.ix_(blk, blk)] = True
    pos, wh = np.asarray([120.0, 90.0]), np.asarray([40.0, 80.0])
    worst_m = worst_c = 0.0
    for n in range(1, 301):
        w, h = x[2], x[3]
        Q = np.diag([(wp * w) ** 2, (wp * h) ** 2, (wp * w) ** 2, (wp * h) ** 2, (wv * w) ** 2, (wv * h) ** 2, (wv * w) ** 2, (wv * h) ** 2])
        x, P = Fm @ x, Fm @ P @ Fm.T + Q
        mean, cov = R.kf_predict(mean, cov)
        wa = R.affine(rng.uniform(-4, 4), rng.uniform(0.97, 1.03), rng.uniform(-6, 6), rng.uniform(-6, 6))
        Rm, t = np.asarray([[wa[0], wa[1]], [wa[3], wa[4]]], np.float64), np.asarray([wa[2], wa[5]], np.float64)
        M = np.kron(np.eye(4), Rm)
        x = M @ x
        x[:2] += t
        P = M @ P @ M.T
        mean, cov = R.kf_warp(mean, cov, wa)
        pos, wh = Rm @ pos + t + rng.uniform(-2, 2, 2), wh * rng.uniform(0.98, 1.02)
        if n % 5 != 0:
            z = np.asarray([pos[0], pos[1], wh[0], wh[1]], F32)
            w, h = x[2], x[3]
            S = H @ P @ H.T + np.diag([(wp * w) ** 2, (wp * h) ** 2, (wp * w) ** 2, (wp * h) ** 2])
            K = P @ H.T @ np.linalg.inv(S)
            x, P = x + K @ (z.astype(np.float64) - H @ x), P - K @ H @ P
            mean, cov = R.kf_update(mean, cov, z)
        assert np.abs(P[~inblock]).max() < 1e-9
        worst_m = max(worst_m, np.abs(mean.astype(np.float64) - x).max() / np.abs(x).max())
        worst_c = max(worst_c, np.abs(R.dense_cov(cov) - P).max() / np.abs(P).max())
    print(f"two-block filter: largest relative difference mean {worst_m:.3e}, covariance {worst_c:.3e}")
    assert worst_m <= 4 * MEASURED_MEAN and worst_c <= 4 * MEASURED_COV, (worst_m, worst_c)


def test_identity_warp_leaves_the_state_bit_identical():
    params, dim, frames = R.sequence_inputs("thresholds")
    a, b = R.BotSortRef(dim=dim, **params), R.BotSortRef(dim=dim, **params)
    ident = R.affine()
    assert R.warp_is_identity(ident) and not R.warp_is_identity(R.affine(tx=0.25))
    for f, (xy, cf, cl, desc, _, _) in enumerate(frames):
        assert a.update(xy, cf, cl, desc, None) == b.update(xy, cf, cl, desc, ident)
        assert R.snapshots_equal(a.snapshot(), b.snapshot()) is None, f
    mean, cov = R.kf_init(R.box_to_xywh(BOX[0]))
    mean[4:] = F32(-0.0)                                     # (a product with the identity would turn -0 into +0)
    m2, c2 = R.kf_warp(mean, cov, ident)
    assert np.array_equal(m2.view(np.int32), mean.view(np.int32)) and np.array_equal(c2.view(np.int32), cov.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- matching
@pytest.fixture(scope="module")
def records():
    """Every sequence of the GPU suite run once on the restatement: name -> (restatement, recorded matching problems)."""
    out = {}
    for name in R.SEQUENCES:
        rec = []
        out[name] = (R.run(name, record=rec), rec)
    return out


def _dense(gain):
    return np.asarray([[0.0 if g is None else g for g in row] for row in gain], np.float64)


def test_every_stage_matching_equals_scipy_on_the_dense_gain_matrix(records):
    from scipy.optimize import linear_sum_assignment
    stages = set()
    for name, (_, rec) in records.items():
        for d in rec:
            G = _dense(d["gain"])
            assert (G[G != 0] > 0).all()
            rows, cols = linear_sum_assignment(G, maximize=True)
            want = sorted((int(r), int(c)) for r, c in zip(rows, cols) if G[r, c] > 0)
            assert want == d["pairs"], (name, d["stage"], d["frame"])
            stages.add(d["stage"])
    assert stages == {"first", "second", "new"}


def test_every_optimum_of_the_gpu_suite_is_unique_with_a_margin(records):
    """The kernel sums gains in another order than the restatement; a runner-up more than 1e-9 below the optimum (float64 sums of
    at most 256 gains below 2 differ by far less) means summation order cannot decide a match."""
    worst = {}
    for name, (_, rec) in records.items():
        margins = [R.optimum_margin(d["gain"], d["pairs"]) for d in rec]
        worst[name] = min(margins) if margins else float("inf")
        assert worst[name] > 1e-9, (name, worst[name])
    print("smallest margin per sequence:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    ref, rec = records["limit"]
    last = rec[-1]
    assert len(last["gain"]) == 32 and len(last["gain"][0]) == 64 and sum(g is not None for row in last["gain"] for g in row) == 2048
    assert len(last["pairs"]) == 32 and len(ref.tracks) == 64


def test_pair_limit_scene_with_the_extra_track_has_one_more_contested_pair():
    rec = []
    ref = R.BotSortRef(record=rec, **R.SEQUENCES["limit"][0])
    for xy, cf, cl in R.OC.pair_limit_frames(True):
        ref.update(xy, cf, cl)
    g = rec[-1]["gain"]
    assert len(g) == 33 and sum(x is not None for row in g for x in row) == 2049 and sum(x is not None for x in g[32]) == 1
    assert g[32][63] is not None and sum(row[63] is not None for row in g) == 33


def test_big_scene_is_near_the_capacity_and_has_few_contested_pairs(records):
    ref, rec = records["big"]
    frames = R.sequence_inputs("big")[2]
    assert len(ref.tracks) == 250 and 250 % 64 != 0 and all(len(f[0]) == 950 for f in frames)
    contested = [sum(1 for rows, cols in R.components(d["gain"]) if len(rows) * len(cols) > 1) for d in rec]
    assert all(0 < c <= 8 for c in contested), contested


def test_the_sequences_reach_every_path(records):
    """Re-activation of a lost track, expiry, births that are deleted, the second association, warps with rotation, and the streams
    of the eight-stream call that have tracks but no detections, detections but no tracks, and an identity warp row."""
    ref, rec = records["occlusion"]
    assert ref.next_id - 1 == 5 + 2                        # track_buffer = 5: gaps of 3 and 5 frames are bridged, gaps of 6 and 9 are not
    assert records["lifecycle"][0].next_id - 1 > len(records["lifecycle"][0].tracks) + 5
    assert sum(len(d["pairs"]) for d in records["thresholds"][1] if d["stage"] == "second") > 5
    assert any(w is not None and not R.warp_is_identity(w) and w[1] != 0 for *_, w, _ in R.sequence_inputs("warped")[2])
    s5, s6 = R.sequence_inputs("stream5")[2], R.sequence_inputs("stream6")[2]
    assert len(s5[0][0]) > 0 and len(s5[5][0]) == 0 and len(s6[0][0]) == 0 and len(s6[6][0]) > 0
    assert all(R.warp_is_identity(f[4]) for f in R.sequence_inputs("stream1")[2]) and R.sequence_inputs("stream0")[2][0][4] is None


# ------------------------------------------------------------------------------------------------------- the three components
def _final(name, **switch):
    ref = R.run(name, **switch)
    return [(t.id, tuple(float(v) for v in t.box)) for t in ref.tracks], ref


def test_gmc_scene_fragments_without_the_warp():
    on, ref = _final("gmc")
    off, ref_off = _final("gmc", gmc=False)
    assert [i for i, _ in on] == [1, 2] and ref.next_id == 3                 # the ids are held through the pan, out and back
    assert ref_off.next_id > 10 and all(t.flag != R.TRACKED for t in ref_off.tracks)       # every frame's detections start over
    assert [b for _, b in on] == [tuple(float(v) for v in b) for b in R.sequence_inputs("gmc")[2][-1][0]]


@pytest.mark.parametrize("name", ["reid64", "reid512"])
def test_reid_scene_swaps_identities_on_motion_alone(name):
    on, _ = _final(name)
    off, _ = _final(name, reid=False)
    a, b = (tuple(float(v) for v in box) for box in R.sequence_inputs(name)[2][-1][0])
    assert on == [(1, a), (2, b)]                          # each walks back with its own id
    assert off == [(1, b), (2, a)]                         # IoU alone exchanges them at the turn


def test_fuse_scene_is_decided_by_the_score():
    on, _ = _final("fuse")
    off, _ = _final("fuse_off")
    near, far = (tuple(float(v) for v in box) for box in R.sequence_inputs("fuse")[2][-1][0])
    assert on == [(1, far)]                                # 0.54 x 0.95 beats 0.6 x 0.65; the other detection (0.65 < 0.7) starts no track
    assert off[0] == (1, near) and [i for i, _ in off] == [1, 2]


# ------------------------------------------------------------------------------------------------------------- the library
def test_library_refuses_bad_warps_and_bad_configurations_without_a_device(pkg):
    """rtmodt_botsort_check_warp is what both update calls apply before anything is launched; it and the refusals of create need no
    device.  (frames together with descriptors, and either on a motion-only handle, need a handle: tests/test_gpu_botsort.py.)"""
    ffi = pkg._ffi
    L = ffi.lib()
    good = np.stack([R.affine(3.0, 1.01, 2.0, -1.0), R.affine()]).astype(F32)
    assert L.rtmodt_botsort_check_warp(ffi.ptr(good), 2) == ffi.OK and L.rtmodt_botsort_check_warp(None, 2) == ffi.OK
    for bad in (np.asarray([1, 2, 0, 2, 4, 0], F32), np.asarray([0, 0, 5, 0, 0, 5], F32), np.asarray([1e-4, 0, 0, 0, 1e-3, 0], F32)):
        w = good.copy()
        w[1] = bad
        assert L.rtmodt_botsort_check_warp(ffi.ptr(w), 2) == ffi.E_INVALID and b"singular" in L.rtmodt_last_error()
        assert L.rtmodt_botsort_check_warp(ffi.ptr(w), 1) == ffi.OK              # only the streams of the call are judged
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            w = good.copy()
            w[0, k] = v
            assert L.rtmodt_botsort_check_warp(ffi.ptr(w), 2) == ffi.E_INVALID and b"not finite" in L.rtmodt_last_error()
    assert L.rtmodt_botsort_check_warp(ffi.ptr(good), 0) == ffi.E_INVALID and L.rtmodt_botsort_check_warp(ffi.ptr(good), 65) == ffi.E_INVALID
    bot = pkg.tracking.botsort
    with pytest.raises(ffi.RtmodtError):
        bot.check_warp(np.zeros((2, 3), F32))
    assert bot.check_warp(None) is None and bot.check_warp(R.affine(2.0)).shape == (1, 6)

    def create(**kw):
        p = dict(track_high_thresh=0.6, track_low_thresh=0.1, new_track_thresh=0.7, track_buffer=30, match_thresh=0.8, proximity_thresh=0.5,
                 appearance_thresh=0.25, fuse_score=1, embedder=None, dim=0, max_tracks=32, max_dets=16, n_streams=1, device=0)
        p.update(kw)
        h = C.c_void_p()
        rc = L.rtmodt_botsort_create(C.byref(ffi.BotSortCfg(*p.values())), C.byref(h))
        assert rc != ffi.OK and not h.value                # (every call here is refused before the device is touched)
        return rc
    assert create(embedder=b"osnet_x0_25.onnx") == ffi.E_UNSUPPORTED and b"only the built-in \"colorhist\" descriptor" in L.rtmodt_last_error()
    assert create(embedder=b"none", dim=64) == ffi.E_INVALID and create(embedder=b"colorhist", dim=100) == ffi.E_INVALID
    assert create(embedder=b"colorhist", dim=576) == ffi.E_INVALID and create(embedder=b"missing.rtreid", dim=64) == ffi.E_INVALID
    assert create(embedder=b"missing.rtreid") != ffi.OK
    assert create(track_buffer=0) == ffi.E_INVALID and create(match_thresh=float("nan")) == ffi.E_INVALID and create(match_thresh=1.5) == ffi.E_INVALID
    assert create(track_high_thresh=float("inf")) == ffi.E_INVALID and create(max_tracks=0) == ffi.E_INVALID and create(n_streams=0) == ffi.E_INVALID
    assert create(max_tracks=257) == ffi.E_CAPACITY and create(max_dets=1025) == ffi.E_CAPACITY and create(n_streams=65) == ffi.E_CAPACITY
    assert L.rtmodt_botsort_create(None, None) == ffi.E_INVALID
    assert L.rtmodt_botsort_update_batch(None, None, None, None, None, None, 0, 0, 0, 0, None, None, None) == ffi.E_INVALID
    assert L.rtmodt_botsort_state(None, 0, *([None] * 16)) == ffi.E_INVALID and L.rtmodt_botsort_reset(None, 0) == ffi.E_INVALID
    assert L.rtmodt_crossing_process_botsort(None, None, 0, None, None) == ffi.E_INVALID
    assert pkg.BotSortTracker is pkg.tracking.BotSortTracker and pkg.BotSortTracker.zone_events_on_device is False
    with pytest.raises(NotImplementedError, match="no embedding network runs here"):
        pkg.BotSortTracker(embedder="osnet_x0_25.onnx")
    with pytest.raises(FileNotFoundError):
        pkg.BotSortTracker(embedder="missing.rtreid")
    with pytest.raises(ValueError, match="Unknown tracker: botsort"):
        pkg.MultiObjectTracker("botsort")                  # MultiObjectTracker stays as it is: the class is the way in
