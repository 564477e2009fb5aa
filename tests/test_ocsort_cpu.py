"""CPU: the OC-SORT restatement (tests/ocsort_ref.py) checked against independent forms -- hand-worked literal cases, a dense 7x7
float64 Kalman filter, SciPy's Hungarian method on the dense gain matrix, math.acos -- and the scenes of the GPU suite
(tests/test_gpu_ocsort.py) shown to have a unique optimum in every frame and to exercise each observation-centric component.
PARITY UNPINNED: ocsort, boxmot and filterpy are installed nowhere this runs."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ocsort_ref as R  # noqa: E402

F32 = np.float32
BOX = np.asarray([[10, 10, 40, 70]], F32)


def _one(conf, box=BOX):
    return box, np.asarray([conf], F32), np.zeros(1, np.int32)


def _none():
    return np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32)


# ------------------------------------------------------------------------------------------------------------ literal cases
def test_split_is_strict_at_both_thresholds():
    up = lambda v: np.nextafter(F32(v), F32(1))            # noqa: E731
    r = R.OcSortRef(use_byte=True)
    far = np.asarray([[200, 10, 230, 70], [300, 10, 330, 70], [400, 10, 430, 70]], F32)
    r.update(far, np.asarray([F32(0.6), up(0.6), F32(0.9)], F32), np.zeros(3, np.int32))
    assert [t.id for t in r.tracks] == [1, 2] and [tuple(t.box) for t in r.tracks] == [tuple(far[1]), tuple(far[2])]   # conf == det_thresh: no birth
    for use_byte, want in ((True, [1, 2, 0]), (False, [1, 2, 3])):
        r = R.OcSortRef(use_byte=use_byte)
        r.update(*_one(0.9))
        seen = []
        for conf in (F32(0.1), F32(0.6), up(0.1)):         # at low_thresh: in neither set; at det_thresh: in neither set; just above low_thresh: low
            r.update(*_one(conf))
            seen.append(r.tracks[0].tsu)
        assert seen == want and len(r.tracks) == 1 and r.next_id == 2
    r = R.OcSortRef(use_byte=True)
    r.update(*_one(0.9))
    r.update(*_one(np.nextafter(F32(0.6), F32(0))))        # just below det_thresh: low, matched by the BYTE stage
    assert r.tracks[0].tsu == 0 and r.tracks[0].hits == 1


def test_life_cycle_and_returned_set_over_min_hits():
    r = R.OcSortRef(min_hits=3, max_age=2)
    second = np.asarray([[200, 10, 230, 70]], F32)
    returned, counts = [], []
    for f in range(1, 13):
        boxes = [BOX] if f <= 12 else []
        if 5 <= f <= 9:
            boxes = boxes + [second]
        xy = np.concatenate(boxes) if boxes else np.zeros((0, 4), F32)
        idx = r.update(xy, np.full(len(xy), 0.9, F32), np.zeros(len(xy), np.int32))
        returned.append([r.tracks[i].id for i in idx])
        counts.append([(t.id, t.hits, t.streak, t.age, t.tsu) for t in r.tracks])
    # track 1: born in frame 1 and returned at once (frame_count <= min_hits), then streak 1, 2, 3, ...: never missing from the list
    # track 2: born in frame 5 (hits 0), matched in 6, 7, 8 -> streak 3 in frame 8: returned in frames 8 and 9 only
    assert returned == [[1], [1], [1], [1], [1], [1], [1], [1, 2], [1, 2], [1], [1], [1]]
    assert counts[0] == [(1, 0, 0, 0, 0)] and counts[1] == [(1, 1, 1, 1, 0)] and counts[4] == [(1, 4, 4, 4, 0), (2, 0, 0, 0, 0)]
    assert counts[8] == [(1, 8, 8, 8, 0), (2, 4, 4, 4, 0)]
    # frames 10, 11: track 2 is missed (tsu 1, 2 <= max_age, streak reset by the second predict); frame 12: tsu 3 > max_age: deleted
    assert counts[9][1] == (2, 4, 4, 5, 1) and counts[10][1] == (2, 4, 0, 6, 2) and counts[11] == [(1, 11, 11, 11, 0)]


def test_death_at_max_age_plus_one():
    for max_age in (1, 4):
        r = R.OcSortRef(max_age=max_age)
        r.update(*_one(0.9))
        r.update(*_one(0.9))
        alive = []
        for _ in range(max_age + 2):
            r.update(*_none())
            alive.append(len(r.tracks))
        assert alive == [1] * max_age + [0, 0]
        assert r.next_id == 2 and r.frame_count == max_age + 4


def test_restatement_and_library_refuse_iou_threshold_not_above_half_inertia(pkg):
    with pytest.raises(ValueError):
        R.OcSortRef(iou_threshold=0.05, inertia=0.2)
    with pytest.raises(ValueError):
        R.OcSortRef(delta_t=9)
    ffi = pkg._ffi
    L = ffi.lib()

    def create(**kw):
        p = dict(det_thresh=0.6, low_thresh=0.1, iou_threshold=0.3, inertia=0.2, max_age=30, min_hits=3, delta_t=3, use_byte=0, max_tracks=32,
                 max_dets=16, n_streams=1, device=0)
        p.update(kw)
        h = C.c_void_p()
        rc = L.rtmodt_ocsort_create(C.byref(ffi.OcSortCfg(*p.values())), C.byref(h))
        assert rc != ffi.OK and not h.value                # (every call here is refused before the device is touched)
        return rc
    assert create(iou_threshold=0.05) == ffi.E_INVALID and b"inertia / 2" in L.rtmodt_last_error()
    assert create(iou_threshold=0.3, inertia=0.7) == ffi.E_INVALID
    assert create(inertia=-0.1) == ffi.E_INVALID and create(inertia=float("nan")) == ffi.E_INVALID
    assert create(delta_t=0) == ffi.E_INVALID and create(max_age=0) == ffi.E_INVALID and create(min_hits=-1) == ffi.E_INVALID
    assert create(max_tracks=0) == ffi.E_INVALID and create(n_streams=0) == ffi.E_INVALID
    assert create(delta_t=9) == ffi.E_CAPACITY and create(max_tracks=257) == ffi.E_CAPACITY and create(max_dets=1025) == ffi.E_CAPACITY
    assert create(n_streams=65) == ffi.E_CAPACITY
    assert L.rtmodt_ocsort_create(None, None) == ffi.E_INVALID
    assert pkg.OcSortTracker.needs_frame is False and pkg.tracking.OcSortTracker is pkg.OcSortTracker
    with pytest.raises(ValueError, match="Unknown tracker: ocsort"):
        pkg.MultiObjectTracker("ocsort")                   # MultiObjectTracker stays as it is: the class is the way in


# ------------------------------------------------------------------------------------------------------------------ filter
def test_block_diagonal_filter_equals_dense_float64_filter():
    """SORT's 7-state filter as dense float64 matrices (F, H, Q, R, P0 as published; P - K H P) against the block-diagonal float32
    lanes, over 25 predict / update steps.  Every float32 operation rounds by at most 2^-24 relative to its operands, and a step
    has fewer than 16 operations per value, so after n steps the two differ by less than 16 n 2^-24 of the largest magnitude that
    entered the computation (x 4 for the gains, which carry the covariance's error into the mean).  For the covariance that
    magnitude is P0's 1e4, not the result: P - K H P cancels (the first update takes a variance of 1e4 down to 1), which is the
    price of this form and why the comparison is not relative to the entry.  For the mean it is the largest state value."""
    rng = np.random.default_rng(3)
    Fm = np.eye(7)
    Fm[0, 4] = Fm[1, 5] = Fm[2, 6] = 1.0
    H = np.eye(4, 7)
    Q = np.diag([1, 1, 1, 1, 1e-2, 1e-2, 1e-4])
    Rm = np.diag([1.0, 1.0, 10.0, 10.0])
    z0 = R.box_to_z(np.asarray([100, 50, 140, 130], F32))
    x = np.concatenate([z0.astype(np.float64), np.zeros(3)])
    P = np.diag([10, 10, 10, 10, 1e4, 1e4, 1e4]).astype(np.float64)
    mean, cov = R.kf_init(z0)
    steps = 25
    worst, peak = 0.0, 0.0
    for n in range(1, steps + 1):
        x, P = Fm @ x, Fm @ P @ Fm.T + Q
        mean, cov = R.kf_predict(mean, cov)
        if n % 4 != 0:                                     # every fourth step is a miss: predict only
            z = R.box_to_z(np.asarray([100 + 3 * n, 50 + 2 * n, 140 + 3 * n + n % 3, 130 + 2 * n], F32) + rng.integers(-4, 5, 4).astype(F32) / 4)
            S = H @ P @ H.T + Rm
            K = P @ H.T @ np.linalg.inv(S)
            x, P = x + K @ (z.astype(np.float64) - H @ x), P - K @ H @ P
            mean, cov = R.kf_update(mean, cov, z)
        dense = np.zeros((7, 7))
        for k in range(4):
            dense[k, k] = cov[3 * k]
            if k < 3:
                dense[k, 4 + k] = dense[4 + k, k] = cov[3 * k + 1]
                dense[4 + k, 4 + k] = cov[3 * k + 2]
        assert mean[7] == 0 and cov[10] == 0 and cov[11] == 0
        bound = 4 * 16 * n * 2.0 ** -24
        peak = max(peak, np.abs(x).max())
        for got, want, scale in ((mean[:7].astype(np.float64), x, peak), (dense, P, 1e4)):
            err = np.abs(got - want).max() / scale
            worst = max(worst, err / bound)
            assert err <= bound, (n, err, bound)
        assert np.abs(P[dense == 0]).max() < 1e-9          # the dense filter stays block-diagonal too
    print(f"block-diagonal filter: worst error / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- matching
@pytest.fixture(scope="module")
def records():
    """Every sequence of the GPU suite run once on the restatement: name -> (restatement, recorded matching problems)."""
    out = {}
    for name in R.SEQUENCES:
        params, frames = R.sequence_inputs(name)
        rec = []
        ref = R.OcSortRef(record=rec, **params)
        for xy, cf, cl in frames:
            ref.update(xy, cf, cl)
        out[name] = (ref, rec)
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
    assert stages == {"ocm", "byte", "ocr"}


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
    ref = R.OcSortRef(record=rec, **R.SEQUENCES["limit"][0])
    for xy, cf, cl in R.pair_limit_frames(True):
        ref.update(xy, cf, cl)
    g = rec[-1]["gain"]
    assert len(g) == 33 and sum(x is not None for row in g for x in row) == 2049 and sum(x is not None for x in g[32]) == 1
    assert g[32][63] is not None and sum(row[63] is not None for row in g) == 33


def test_big_scene_is_near_the_capacity_and_has_few_contested_pairs(records):
    ref, rec = records["big"]
    params, frames = R.sequence_inputs("big")
    assert len(ref.tracks) == 250 and 250 % 64 != 0 and all(len(xy) == 950 for xy, _, _ in frames)
    contested = [sum(1 for rows, cols in R.components(d["gain"]) if len(rows) * len(cols) > 1) for d in rec]
    assert all(0 < c <= 8 for c in contested), contested


# ------------------------------------------------------------------------------------------------------- the three components
def _final(name, **switch):
    params, frames = R.sequence_inputs(name)
    ref = R.OcSortRef(**params, **switch)
    for xy, cf, cl in frames:
        ref.update(xy, cf, cl)
    return [(t.id, tuple(float(v) for v in t.box)) for t in ref.tracks], frames


def test_ocm_scene_changes_identities_without_direction_consistency():
    on, frames = _final("ocm")
    off, _ = _final("ocm", ocm=False)
    a, b = (tuple(float(v) for v in box) for box in frames[-1][0])
    assert on == [(1, a), (2, b)]                          # A keeps id 1, B keeps id 2
    assert off == [(1, b), (2, a)]                         # IoU alone exchanges them where they meet


def test_ocr_scene_changes_identities_without_recovery(records):
    on, frames = _final("ocr")
    off, _ = _final("ocr", ocr=False)
    assert [i for i, _ in on] == [1] and [i for i, _ in off] == [1, 2]
    rec = records["ocr"][1]
    assert sum(len(d["pairs"]) for d in rec if d["stage"] == "ocr") >= 1
    first_halt = [d for d in rec if d["stage"] == "ocm" and d["frame"] == 8]
    assert first_halt and first_halt[0]["pairs"] == []     # the prediction ran on: no admissible pair in the first association


def test_oru_scene_changes_identities_without_re_update(records):
    on, frames = _final("oru")
    off, _ = _final("oru", oru=False)
    obj, decoy = (tuple(float(v) for v in box) for box in frames[-1][0])
    assert on == [(1, obj), (2, decoy)]                    # the track stays on its halted object
    assert off[0] == (1, decoy) and off != on              # the stale velocity carries id 1 to the object ahead
    assert sum(len(d["pairs"]) for d in records["oru"][1] if d["stage"] == "ocr") == 1     # re-found by the recovery stage, tsu 3


# -------------------------------------------------------------------------------------------------------------------- acos
def test_fixed_sequence_acos_is_below_the_step_a_float32_cosine_resolves():
    """Largest error against math.acos over a dense grid of [-1, 1] (every float32 within 4096 ulps of -1, -0.5, 0, 0.5 and 1, and
    400001 evenly spaced points).  Bound: the cosine is a float32 in [-1, 1] whose spacing at unit scale is 2^-24, and |d acos / dc|
    >= 1, so one step of the cosine there moves acos by at least 2^-24 = 5.96e-8; an error below that cannot be told from the
    rounding of the cosine itself.  Measured: 4.5e-16."""
    pts = [np.linspace(-1, 1, 400001).astype(F32)]
    for centre in (-1.0, -0.5, 0.0, 0.5, 1.0):
        x = F32(centre)
        up, down = [x], [x]
        for _ in range(4096):
            up.append(np.nextafter(up[-1], F32(2)))
            down.append(np.nextafter(down[-1], F32(-2)))
        pts.append(np.asarray(up + down, F32))
    grid = np.unique(np.concatenate(pts))
    grid = grid[(grid >= -1) & (grid <= 1)]
    assert grid[0] == -1 and grid[-1] == 1
    err = max(abs(R.acos_fixed(c) - math.acos(float(c))) for c in grid)
    print(f"acos_fixed: largest error {err:.3e} over {len(grid)} points")
    assert err < 2.0 ** -24
    assert R.acos_fixed(F32(1)) == 0.0 and R.acos_fixed(F32(-1)) == R.PI and R.acos_fixed(F32(0)) == R.HALF_PI
