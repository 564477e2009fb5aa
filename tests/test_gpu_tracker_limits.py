"""GPU: the single-launch ByteTrack kernel where the fixture sequences never take it -- more than 1024 tracks or detections (the
second trip of every scan loop), ties at every lane width of the association pass, edge parameters, exactly-full capacity, reset,
per-stream addressing and the LDS budget.  Every comparison is bit for bit against the NumPy oracle fed the same arrays;
tests/test_tracker_cases_cpu.py proves that the scenes (tests/tracker_cases.py) reach the paths they are meant for."""
import functools

import numpy as np
import pytest

import tracker_cases as TC
from oracle import kalman_oracle as K
from oracle import tracker_oracle as T

pytestmark = pytest.mark.gpu
KEYS = ("ids", "xyxy", "conf", "cls", "age", "tsu")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_state(core, orc, stream=0, tag=""):
    s, o = core.snapshot(stream), orc.snapshot()
    for key in KEYS:
        assert np.array_equal(bits(s[key]), bits(o[key])), (tag, key)
    assert s["next_id"] == o["next_id"], tag
    if "mean" in o:
        k = core.kalman_snapshot(stream)
        assert np.array_equal(k["mean"].view(np.int32), o["mean"].view(np.int32)), (tag, "mean")
        assert np.array_equal(k["cov"].view(np.int32), o["cov"].view(np.int32)), (tag, "cov")
    return s


def make_core(pkg, **kw):
    return pkg.tracking.tracker._ByteTrackCore(**kw)


def oracle_for(kalman=False, **kw):
    return (K.TrackerOracleKalman if kalman else T.TrackerOracle)(**kw)


def spawn_then(pkg, tracks, dets, conf, tag):
    """frame 1 spawns ``tracks`` (all confident), frame 2 feeds the tie detections; compared after each"""
    core, orc = make_core(pkg, max_tracks=2048, max_dets=2048), T.TrackerOracle()     # 2048 * 28 + 2048 * 40 + 132 = 139 396 B of LDS
    try:
        cls = (np.arange(len(tracks)) % 80).astype(np.int32)
        for f, (b, c, k) in enumerate([(tracks, np.full(len(tracks), 0.9, np.float32), cls),
                                       (dets, conf, (np.arange(len(dets)) % 7).astype(np.int32))]):
            core.update(b, c, k)
            orc.update(b, c, k)
            s = same_state(core, orc, tag=(tag, f))
        assert len(s["ids"]) >= len(tracks) and (s["age"] == 2).any() and (s["tsu"] == 2).any()      # matched rows and losers of a contest
    finally:
        core.close()


# ------------------------------------------------------------------ A / B: ties and contested columns at every lane width
@pytest.mark.parametrize("m", TC.TIE_SIZES)
def test_ties_first_pass(pkg, m):
    spawn_then(pkg, *TC.tie_scene(m, TC.tie_rng(m)), tag=m)


@pytest.mark.parametrize("rows,cols,width", TC.COLUMN_BOUND)
def test_ties_column_bound(pkg, rows, cols, width):
    spawn_then(pkg, *TC.column_bound_scene(rows, cols, np.random.default_rng(rows)), tag=(rows, cols))


@pytest.mark.parametrize("m", TC.TIE_SIZES_PASS2)
def test_ties_second_pass(pkg, m):
    """half of the detections are low-confidence: rows go through the unmatched-track list, columns through the low list"""
    spawn_then(pkg, *TC.tie_scene(m, TC.tie_rng(m, 0.5), low_share=0.5), tag=m)


# ------------------------------------------------------------------ C / D / F / G: more than 1024 live tracks
@functools.lru_cache(maxsize=None)
def population_frames():
    return tuple(TC.two_populations(900, np.random.default_rng(3)))


@functools.lru_cache(maxsize=None)
def churn_frames():
    return tuple(TC.churn_frames(900, np.random.default_rng(4)))


@pytest.mark.parametrize("kalman", [False, True])
def test_1800_live_tracks_default_capacities(pkg, kalman):
    """the tracker as every tool constructs it (2048 tracks, 1024 detections): two trips of the predict, unmatched-list and
    compaction loops and of the association rows; pass 2 sees more than 1024 unmatched tracks"""
    core, orc = make_core(pkg, kalman=kalman), oracle_for(kalman)
    assert (core.max_tracks, core.max_dets) == (2048, 1024)
    try:
        for f, (b, c, k) in enumerate(population_frames()):
            core.update(b, c, k)
            orc.update(b, c, k)
            s = same_state(core, orc, tag=f)
            assert len(s["ids"]) == (900 if f == 0 else 1800), f
    finally:
        core.close()


@pytest.mark.parametrize("kalman", [False, True])
def test_mixed_expiry_across_both_trips(pkg, kalman):
    core, orc = make_core(pkg, track_buffer=2, max_tracks=2048, max_dets=1024, kalman=kalman), oracle_for(kalman, track_buffer=2)
    try:
        frames = churn_frames()
        for f, (b, c, k) in enumerate(frames):
            core.update(b, c, k)
            orc.update(b, c, k)
            s = same_state(core, orc, tag=f)
            assert (np.diff(s["ids"]) > 0).all(), f                     # stable compaction: ids stay in list order
        assert s["next_id"] - 1 > 1800 and len(s["ids"]) > 1024
    finally:
        core.close()


def test_1800_live_tracks_lapjv(pkg):
    """isolated edges only: the degree count and the shortcut of the sparse solver past one trip (the solver has its own tests)"""
    core = make_core(pkg, max_tracks=2048, max_dets=1024, assign_mode=pkg._ffi.ASSIGN_LAPJV)
    orc = T.TrackerOracle(assign="lapjv")
    try:
        for f, (b, c, k) in enumerate(population_frames()[:4]):
            core.update(b, c, k)
            orc.update(b, c, k)
            s = same_state(core, orc, tag=f)
        assert len(s["ids"]) == 1800
    finally:
        core.close()


# ------------------------------------------------------------------ E: more than 1024 highs and more than 1024 lows in one frame
def test_more_than_1024_highs_and_lows(pkg):
    """second trip of the hi / lo split, of the spawn list and of the low-detection list.  2048 tracks leave room for 2397
    detections under the kernel's LDS limit ((153 600 - 132 - 2048 * 28) / 40); 2304 holds the 2080 of the scene."""
    core, orc = make_core(pkg, max_tracks=2048, max_dets=2304), T.TrackerOracle()
    try:
        for f, (b, c, k) in enumerate(TC.big_frames(np.random.default_rng(5))):
            core.update(b, c, k)
            orc.update(b, c, k)
            s = same_state(core, orc, tag=f)
        assert len(s["ids"]) > 1024
    finally:
        core.close()


# ------------------------------------------------------------------ H: edge parameters
def run_small(pkg, frames, max_tracks=512, max_dets=512, **params):
    core, orc = make_core(pkg, max_tracks=max_tracks, max_dets=max_dets, **params), T.TrackerOracle(**params)
    snaps = []
    try:
        for f, (b, c, k) in enumerate(frames):
            core.update(b, c, k)
            orc.update(b, c, k)
            snaps.append(same_state(core, orc, tag=f))
    finally:
        core.close()
    return snaps


def test_track_buffer_0_and_1(pkg):
    frames = TC.drift_frames(64, 10, np.random.default_rng(6))
    snaps = run_small(pkg, frames, track_buffer=0)
    assert all(len(s["ids"]) == 0 for s in snaps)                       # every track expires in the frame that spawned it
    highs = np.cumsum([int((c >= np.float32(0.5)).sum()) for _, c, _ in frames])
    assert [s["next_id"] for s in snaps] == (highs + 1).tolist()        # ... and the ids advance all the same
    snaps = run_small(pkg, frames, track_buffer=1)
    assert all((s["tsu"] == 1).all() for s in snaps) and max(int(s["age"].max(initial=0)) for s in snaps) >= 3


def test_match_thresh_zero(pkg):
    """every row passes with its arg-max; the rows whose IoU is 0 everywhere all pick column 0 and the smallest one wins it"""
    rng = np.random.default_rng(7)
    tracks = TC.grid_boxes(300, rng)
    cls = np.zeros(300, np.int32)
    frames = [(tracks, np.full(300, 0.9, np.float32), cls)]
    for f in range(1, 9):
        pick = rng.permutation(300)[:40]
        frames.append(((tracks[pick] + np.float32(0.5 * f)).astype(np.float32), TC._confidences(40, rng, 0.3), cls[:40] + f))
    snaps = run_small(pkg, frames, match_thresh=0.0)
    moved = np.diag(T.batch_iou(snaps[0]["xyxy"], snaps[1]["xyxy"][:300])) == 0
    assert moved.any() and (snaps[1]["age"][:300][moved] == 2).all()    # a track took a detection it does not overlap at all


def test_match_thresh_above_one(pkg):
    frames = TC.drift_frames(48, 10, np.random.default_rng(8), low_share=0.3, drop=0.0)
    snaps = run_small(pkg, frames, match_thresh=1.5)
    highs = np.cumsum([int((c >= np.float32(0.5)).sum()) for _, c, _ in frames])
    assert [len(s["ids"]) for s in snaps] == highs.tolist()             # nothing ever matches: every high detection spawns
    assert (snaps[-1]["age"] == 1).all()


def test_all_high_all_low_and_empty_frames(pkg):
    rng = np.random.default_rng(9)
    base = TC.drift_frames(60, 12, rng, low_share=0.0, drop=0.1)
    frames = []
    for f, (b, c, k) in enumerate(base):
        if f % 3 == 1:
            c = rng.uniform(0.1, 0.45, len(c)).astype(np.float32)       # all low: pass 1 is skipped, nothing can spawn
        elif f % 3 == 2:
            b, c, k = b[:0], c[:0], k[:0]
        frames.append((b, c, k))
    snaps = run_small(pkg, frames)
    assert snaps[1]["next_id"] == snaps[0]["next_id"] and (snaps[1]["tsu"] == 1).any()


# ------------------------------------------------------------------ I: exactly full
def full_frames():
    boxes = TC.grid_boxes(65, np.random.default_rng(10))
    conf, cls = np.full(65, 0.9, np.float32), np.arange(65, dtype=np.int32)
    return [(boxes[:n], conf[:n], cls[:n]) for n in (60, 64, 65)]


def test_exactly_full_then_one_too_many(pkg):
    core, orc = make_core(pkg, max_tracks=64, max_dets=128), T.TrackerOracle()
    try:
        for b, c, k in full_frames()[:2]:
            core.update(b, c, k)
            orc.update(b, c, k)
        s = same_state(core, orc)
        assert len(s["ids"]) == 64 and s["next_id"] == 65               # M + spawned == max_tracks is not an error
        calls = [lambda: core.update(*full_frames()[2]), core.snapshot, lambda: core.update(*full_frames()[0])]
        for call in calls:                                              # one more raises, and the error is sticky
            with pytest.raises(pkg._ffi.RtmodtError) as e:
                call()
            assert e.value.code == pkg._ffi.E_CAPACITY
    finally:
        core.close()


# ------------------------------------------------------------------ J: reset
@pytest.mark.parametrize("kalman", [False, True])
def test_reset_one_stream_and_all(pkg, kalman):
    S = 3
    core = make_core(pkg, n_streams=S, max_tracks=64, max_dets=128, kalman=kalman)
    orcs = [oracle_for(kalman) for _ in range(S)]
    seqs = [TC.drift_frames(30 + 5 * s, 12, np.random.default_rng(20 + s)) for s in range(S)]
    try:
        for f in range(3):
            for s in (0, 2):
                core.update(*seqs[s][f], stream=s)
                orcs[s].update(*seqs[s][f])
        for b, c, k in full_frames()[:2]:
            core.update(b, c, k, stream=1)
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            core.update(*full_frames()[2], stream=1)
        assert e.value.code == pkg._ffi.E_CAPACITY
        with pytest.raises(pkg._ffi.RtmodtError):
            core.snapshot(1)
        core.reset(1)
        orcs[1] = oracle_for(kalman)
        assert len(same_state(core, orcs[1], stream=1)["ids"]) == 0
        for f in range(3, 8):                                           # the reset stream starts again at id 1, the others go on
            for s in range(S):
                core.update(*seqs[s][f], stream=s)
                orcs[s].update(*seqs[s][f])
                same_state(core, orcs[s], stream=s, tag=(f, s))
        assert core.snapshot(1)["ids"][0] == 1 and core.snapshot(0)["ids"][0] == 1
        core.reset(-1)
        orcs = [oracle_for(kalman) for _ in range(S)]
        for f in range(8, 11):
            for s in range(S):
                core.update(*seqs[s][f], stream=s)
                orcs[s].update(*seqs[s][f])
                same_state(core, orcs[s], stream=s, tag=("after reset(-1)", f, s))
    finally:
        core.close()


# ------------------------------------------------------------------ K: stream addressing
def test_ragged_streams_batch_and_single_updates_interleaved(pkg):
    """streams of 0, 5, 300 and 1500 live tracks in one handle, advanced alternately by update_batch (one launch, one
    workgroup per stream) and by update(..., stream=s) (one launch per stream, addressed through stream_base)"""
    S, N, frames = 4, 1024, 6
    rng = np.random.default_rng(11)
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    seqs = [[empty] * frames, TC.drift_frames(5, frames, rng, drop=0.0), TC.drift_frames(300, frames, rng, drop=0.0),
            TC.two_populations(750, rng, frames)]
    core = make_core(pkg, n_streams=S, max_tracks=2048, max_dets=N)
    orcs = [T.TrackerOracle() for _ in range(S)]
    try:
        for f in range(frames):
            if f % 2 == 0:
                xy, cf, cl = np.zeros((S, N, 4), np.float32), np.zeros((S, N), np.float32), np.zeros((S, N), np.int32)
                cnt = np.zeros(S, np.int32)
                for s in range(S):
                    b, c, k = seqs[s][f]
                    cnt[s] = len(c)
                    xy[s, :len(c)], cf[s, :len(c)], cl[s, :len(c)] = b, c, k
                assert core.update_batch(xy, cf, cl, cnt).tolist() == [0] * S
            else:
                for s in (2, 0, 3, 1):
                    core.update(*seqs[s][f], stream=s)
            for s in range(S):
                orcs[s].update(*seqs[s][f])
                same_state(core, orcs[s], stream=s, tag=(f, s))
        assert [len(o.ids) for o in orcs] == [0, 5, 300, 1500]
    finally:
        core.close()


# ------------------------------------------------------------------ K: the smallest handle, odd capacities
@pytest.mark.parametrize("assign", ["greedy", "lapjv"])
@pytest.mark.parametrize("kalman", [False, True], ids=["plain", "kalman"])
def test_small_odd_handle_equals_oracle_every_frame(pkg, kalman, assign):
    """7 tracks x 5 detections x 3 streams: no state array's size is a multiple of 16 bytes, so every array after the first
    depends on the pool's alignment rule.  Births, misses, a second-pass match and expiries (track_buffer = 2) in every stream; the
    full state -- with the Kalman model on, the filter state too -- equals the oracle's bit for bit after every frame."""
    S, N = TC.SMALL_STREAMS, TC.SMALL_DETS
    mode = pkg._ffi.ASSIGN_LAPJV if assign == "lapjv" else pkg._ffi.ASSIGN_GREEDY
    core = make_core(pkg, track_buffer=TC.SMALL_BUFFER, n_streams=S, max_tracks=TC.SMALL_TRACKS, max_dets=N, assign_mode=mode, kalman=kalman)
    orcs = [oracle_for(kalman, track_buffer=TC.SMALL_BUFFER, assign=assign) for _ in range(S)]
    seqs = [TC.small_handle_frames(s) for s in range(S)]
    try:
        for f in range(TC.SMALL_FRAMES):
            xy, cf, cl, cnt = np.zeros((S, N, 4), np.float32), np.zeros((S, N), np.float32), np.zeros((S, N), np.int32), np.zeros(S, np.int32)
            for s in range(S):
                b, c, k = seqs[s][f]
                xy[s, :len(b)], cf[s, :len(b)], cl[s, :len(b)], cnt[s] = b, c, k, len(b)
                orcs[s].update(b, c, k)
            core.update_batch(xy, cf, cl, cnt)
            for s in range(S):
                same_state(core, orcs[s], stream=s, tag=(f, s))
        assert all(o.next_id - 1 > len(o.ids) for o in orcs)              # tracks expired in every stream
    finally:
        core.close()


# ------------------------------------------------------------------ L: LDS budget
# The kernel carves max_tracks * 28 + max_dets * 40 + 132 bytes (boxes 16 + three int lists 12 per track; box 16 + confidence,
# class, three index lists and the column winners 24 per detection; 17 scan words + 64) and launch_tracker_update accepts at
# most 150 KiB = 153 600 B.  With 4096 tracks: 4096 * 28 + 969 * 40 + 132 = 153 580 fits, 970 detections need 153 620.
LDS_TRACKS, LDS_DETS_FIT = 4096, 969


def test_lds_budget_largest_fit_and_first_refusal(pkg):
    assert LDS_TRACKS * 28 + LDS_DETS_FIT * 40 + 132 <= 150 * 1024 < LDS_TRACKS * 28 + (LDS_DETS_FIT + 1) * 40 + 132
    frames = TC.drift_frames(50, 2, np.random.default_rng(12), drop=0.0)
    snaps = run_small(pkg, frames, max_tracks=LDS_TRACKS, max_dets=LDS_DETS_FIT)
    assert len(snaps[-1]["ids"]) > 0
    core = make_core(pkg, max_tracks=LDS_TRACKS, max_dets=LDS_DETS_FIT + 1)      # creation accepts up to 4096 x 4096
    try:
        for _ in range(2):                                              # refused before any launch, every time
            with pytest.raises(pkg._ffi.RtmodtError) as e:
                core.update(*frames[0])
            assert e.value.code == pkg._ffi.E_INVALID
            assert "150 KiB" in str(e.value) and "153620" in str(e.value)
        s = core.snapshot()                                             # nothing ran: the state is still the initial one
        assert len(s["ids"]) == 0 and s["next_id"] == 1
    finally:
        core.close()
    assert core._h is None
