"""GPU: the calls directly behind a zeroing write.  A create, a reset or a load zeroes its buffers on the handle's own stream and waits
for that stream once before it returns (csrc/handle_host.h: handle_zero, handle_created), so whatever the caller does next finds the
zeroes in place and nothing zeroes again behind it.  One run of each cannot prove a race absent; these pin what the sequence
guarantees, with == on integers, at one stream and the modules' smallest sizes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossing_ref as CR  # noqa: E402
import gmc_cases as K  # noqa: E402
import snapshot_ref as SR  # noqa: E402
from gmc_run import _est, _same  # noqa: E402
from test_gpu_crossing import check, counts_of, tracks_of  # noqa: E402
from test_gpu_snapshot import Dev, Frame  # noqa: E402

pytestmark = pytest.mark.gpu


def test_crossing_counts_from_zero_right_after_the_reset(pkg):
    line = {"name": "l", "a": [50, 0], "b": [50, 100], "direction": "both"}
    counter = pkg.events.CrossingCounter([line], (), max_tracks=8)
    ref = CR.CrossingRef([line], (), max_tracks=8)
    left, right = lambda i: CR.box(40, 10 + 20 * i), lambda i: CR.box(60, 10 + 20 * i)
    calls = [(0, [(1, left(0), 0), (2, left(1), 0), (3, right(2), 0)]), (1, [(1, right(0), 0), (2, right(1), 0), (3, left(2), 0)])]
    for frame_id, rows in calls:
        check(counter, ref, counter.process(tracks_of(rows), frame_id), ref.process(rows, frame_id), f"frame {frame_id}")
    assert np.sum(ref.counts()["line_total"]) == 3                                  # a few crossings ...
    counter.reset_counts()                                                          # ... the counts go back to zero ...
    ref.reset_counts()
    rows = [(1, left(0), 0), (2, right(1), 0), (3, left(2), 0)]                     # ... and at once one more crossing: track 1 walks back
    check(counter, ref, counter.process(tracks_of(rows), 2), ref.process(rows, 2), "frame 2")
    assert counts_of(counter) == ref.counts() and np.sum(ref.counts()["line_total"]) == 1
    counter.close()


def test_snapshot_stream_is_fresh_right_after_its_reset(pkg):
    box = lambda i: [4 + 6 * (i % 12), 4 + 8 * (i // 12), 12 + 6 * (i % 12), 14 + 8 * (i // 12)]
    fr = Frame(pkg, 61, 97, 3 * 97, 30, False, 0)
    cfg = SR.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=2, occl_iou_pm=0, retire_after=1000)
    d = Dev(pkg, cfg, 1, 4)                                                         # 8 rows
    for call in range(2):                                                           # the stream fills up
        ids = [4 * call + i for i in range(4)]
        assert d.process(0, ids, [box(i) for i in ids], None, [0] * 4, fr, call)[0] == 0
    d.F.check(d.L.rtmodt_snapshot_reset(d.h, 0))
    d.ref[0] = SR.Stream(cfg, 4)                                                    # a fresh stream ...
    d.ref[0].atlas[:] = d.atlas(0)                                                  # (... whose atlas bytes stay as they are)
    code, u, r = d.process(0, [9], [box(9)], None, [0], fr, 0)                      # results, atlas, ledger and bitmap against the restatement
    assert code == 0 and len(u) == 1 and r == []
    rc, rows, bm = d.state(0)
    assert rc == 0 and [x[0] for x in rows] == [9] and int(np.unpackbits(bm.view(np.uint8)).sum()) == 1
    d.close()
    fr.free()


def test_gmc_first_estimates_right_after_create(pkg):
    c, ref = K.case("d4"), K.reference("d4")
    est = _est(pkg, n_streams=len(c.streams), **c.cfg)
    for f in range(2):                                                              # the first pair: FIRST, then a full estimate
        warp, status = est.estimate([st[f] for st in c.streams], c.masks)
        for s in range(len(c.streams)):
            _same(est, s, warp[s], status[s], ref[f][s], ("d4", f, s))
    est.close()


def _core(pkg, name, **kw):
    T = pkg.tracking
    return {"bytetrack": T.tracker._ByteTrackCore, "deepsort": T.deepsort._DeepSortCore, "ocsort": T.ocsort._OcSortCore, "botsort": T.botsort._BotSortCore}[name](**kw)


@pytest.mark.parametrize("name", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_tracker_empty_update_right_after_create(pkg, name):
    S, N = 3, 4
    core = _core(pkg, name, max_tracks=4, max_dets=N, n_streams=S)
    got = core.update_batch(np.zeros((S, N, 4), np.float32), np.zeros((S, N), np.float32), np.zeros((S, N), np.int32), np.zeros(S, np.int32))
    assert np.asarray(got).tolist() == [0] * S
    for s in range(S):
        st = core.snapshot(s)
        assert len(st["ids"]) == 0, (name, s, st["ids"])
    core.close()
