"""CPU, oracle only: the scenes of tests/tracker_cases.py reach the conditions that tests/test_gpu_tracker_limits.py relies on.
Without these a GPU test could pass on a scene that never takes the path it was written for."""
import numpy as np
import pytest

import tracker_cases as TC
from oracle import kalman_oracle as K
from oracle import tracker_oracle as T


def pass_matrices(tracks, dets, conf, match_thresh=0.8):
    """The IoU matrices the two association passes see when the tracks were spawned from ``tracks`` one frame earlier."""
    hi = conf >= np.float32(TC.TRACK_THRESH)
    iou1 = T.batch_iou(tracks, dets[hi])
    _, _, um, _ = T.assign_greedy(iou1, match_thresh)
    iou2 = T.batch_iou(tracks[np.asarray(um, np.int64)], dets[~hi]) if um and (~hi).any() else None
    return iou1, iou2


def tie_stats(iou, thresh=0.8):
    """tie rows (row maximum >= thresh attained in >= 2 columns) as (row, those columns), and the columns
    that are the first arg-max of >= 2 passing rows."""
    thr = np.float32(thresh)
    best = iou.max(axis=1)
    ties = []
    for r in np.nonzero(best >= thr)[0]:
        c = np.nonzero(iou[r] == best[r])[0]
        if len(c) >= 2:
            ties.append((int(r), c))
    first = iou.argmax(axis=1)[best >= thr]
    cols, cnt = np.unique(first, return_counts=True)
    return ties, cols[cnt >= 2]


def check_ties(iou, width, min_ties, min_contested):
    assert TC.lane_width(*iou.shape) == width, (iou.shape, TC.lane_width(*iou.shape))
    ties, contested = tie_stats(iou)
    assert len(ties) >= min_ties and len(contested) >= min_contested, (len(ties), len(contested))
    if width >= 2:
        assert any(len(set(c % width)) > 1 for _, c in ties)               # the tie is settled by the butterfly
        # ... and one inside a single lane's loop -- which needs two columns that are `width` apart
        if iou.shape[1] > width:
            assert any(len(set(c % width)) < len(c) for _, c in ties)
        else:
            assert width >= iou.shape[1]
    assert T.assign_greedy_parallel(iou, 0.8) == T.assign_greedy(iou, 0.8)
    return len(ties), len(contested)


@pytest.mark.parametrize("m,width", list(zip(TC.TIE_SIZES, TC.TIE_WIDTHS)))
def test_tie_scenes_first_pass(m, width):
    tracks, dets, conf = TC.tie_scene(m, TC.tie_rng(m))
    assert len(tracks) == m and (conf >= np.float32(TC.TRACK_THRESH)).all()
    iou1, iou2 = pass_matrices(tracks, dets, conf)
    assert iou2 is None
    assert T.batch_iou(tracks[:m - m // 6], tracks[:m - m // 6])[~np.eye(m - m // 6, dtype=bool)].max() == 0      # distinct tracks never overlap
    check_ties(iou1, width, m // 6, m // 8)
    assert (m > 1024) == (m == 1500)                                    # R = 1 with one trip over the rows (1000) and with two (1500)


def test_tie_scenes_cover_every_lane_width():
    widths = [TC.lane_width(m, len(TC.tie_scene(m, TC.tie_rng(m))[1])) for m in TC.TIE_SIZES]
    assert tuple(widths) == TC.TIE_WIDTHS == (16, 32, 16, 8, 4, 2, 1, 1)
    assert [TC.lane_width(r, c) for r, c, _ in TC.COLUMN_BOUND] == [w for _, _, w in TC.COLUMN_BOUND] == [64, 2]
    assert set(widths) | {64, 2} == {64, 32, 16, 8, 4, 2, 1}


@pytest.mark.parametrize("rows,cols,width", TC.COLUMN_BOUND)
def test_column_bound_scenes(rows, cols, width):
    tracks, dets, conf = TC.column_bound_scene(rows, cols, np.random.default_rng(rows))
    assert tracks.shape == (rows, 4) and dets.shape == (cols, 4)
    iou1, _ = pass_matrices(tracks, dets, conf)
    check_ties(iou1, width, 1, 1)


@pytest.mark.parametrize("m", TC.TIE_SIZES_PASS2)
def test_tie_scenes_second_pass(m):
    """low_share = 0.5: both passes hold tie rows and contested columns; the second one's rows go through the unmatched-track list."""
    tracks, dets, conf = TC.tie_scene(m, TC.tie_rng(m, 0.5), low_share=0.5)
    iou1, iou2 = pass_matrices(tracks, dets, conf)
    assert iou2 is not None and iou2.shape[0] < m                       # some tracks left in pass 1: the row list is a true indirection
    for iou in (iou1, iou2):
        ties, contested = tie_stats(iou)
        assert len(ties) >= 1 and len(contested) >= 1, (m, len(ties), len(contested))
        assert T.assign_greedy_parallel(iou, 0.8) == T.assign_greedy(iou, 0.8)
    if m == 1500:
        assert iou2.shape[0] > 1024 or iou1.shape[0] > 1024


def run(oracle, frames):
    counts = []
    for b, c, k in frames:
        oracle.update(b, c, k)
        counts.append(len(oracle.ids))
    return counts


@pytest.mark.parametrize("make", [T.TrackerOracle, K.TrackerOracleKalman])
def test_two_populations_reach_1800_tracks(make):
    frames = TC.two_populations(900, np.random.default_rng(3))
    assert max(len(c) for _, c, _ in frames) == 900
    orc = make()
    assert run(orc, frames) == [900] + [1800] * 7
    assert orc.next_id == 1801                                          # nothing was lost and respawned on the way
    assert (orc.age > 1).all()                                          # every track was matched again, in pass 1 or 2


@pytest.mark.parametrize("make", [T.TrackerOracle, K.TrackerOracleKalman])
def test_churn_expires_on_both_sides_of_1024(make):
    frames = TC.churn_frames(900, np.random.default_rng(4))
    orc = make(track_buffer=2)
    mixed = 0
    for b, c, k in frames:
        before = orc.ids.copy()
        n_before = len(before)
        orc.update(b, c, k)
        gone = ~np.isin(before, orc.ids)                               # by position in the list before the frame
        if n_before > 1024 and gone[:1024].any() and gone[1024:].any() and (~gone[:1024]).any() and (~gone[1024:]).any():
            mixed += 1
        assert (np.diff(orc.ids) > 0).all()                             # stable compaction keeps ids in list order
    assert mixed >= 1
    assert orc.next_id - 1 > 1800                                       # expired tracks came back under new ids


def test_big_frames_exceed_1024_highs_and_lows():
    frames = TC.big_frames(np.random.default_rng(5))
    for b, c, _ in frames:
        hi = int((c >= np.float32(TC.TRACK_THRESH)).sum())
        assert len(c) > 2048 and hi > 1024 and len(c) - hi > 1024
    orc = T.TrackerOracle()
    counts = run(orc, frames)
    assert counts[0] > 1024 and max(counts) <= 2048 and counts[-1] > counts[0]      # later frames spawn too, and all of it fits
    assert (orc.age[:counts[0]] > 1).any()


@pytest.mark.parametrize("make", [T.TrackerOracle, K.TrackerOracleKalman])
@pytest.mark.parametrize("assign", ["greedy", "lapjv"])
def test_small_handle_frames_have_births_misses_and_an_expiry(make, assign):
    for s in range(TC.SMALL_STREAMS):
        frames = TC.small_handle_frames(s)
        assert len(frames) == TC.SMALL_FRAMES and max(len(c) for _, c, _ in frames) <= TC.SMALL_DETS
        assert any((c < np.float32(TC.TRACK_THRESH)).any() for _, c, _ in frames)         # the second pass has a detection
        orc = make(track_buffer=TC.SMALL_BUFFER, assign=assign)
        births = misses = expired = 0
        for f, (b, c, k) in enumerate(frames):
            before, next_before = orc.ids.copy(), orc.next_id
            orc.update(b, c, k)
            births += f > 0 and orc.next_id > next_before
            misses += int((orc.tsu > 1).sum())
            expired += int((~np.isin(before, orc.ids)).sum())
            assert len(orc.ids) <= TC.SMALL_TRACKS
        assert births >= 2 and misses >= 2 and expired >= 2, (s, births, misses, expired)
