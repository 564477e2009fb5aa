"""GPU: the speed estimator (csrc/speed.hip) against its restatement (tests/speed_ref.py): rows, events, pairs, histogram and the
ledger snapshot compared after every call, with exact equality; everything through the C ABI."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ledger_boundary as B
import speed_ref as R
import swapguard_ref as SG

pytestmark = pytest.mark.gpu

SEC = 1_000_000


def tracks_of(rows):
    return [SimpleNamespace(track_id=i, xyxy=np.asarray(b, np.float32), class_id=k, class_name=f"c{k}") for i, b, k in rows]


def ev_dict(e):
    return dict(kind=e.event_type, track_id=e.track_id, speed_mm_s=e.speed_mm_s, t_us=e.t_us, bbox_xyxy=e.bbox_xyxy, world_mm=e.world_mm,
                class_id=e.class_id, track=e.track)


def check(est, ref, want, where, k=0, stream=0, remap=None):
    """The call's outputs (slot k of the last_* lists) and the stream's ledger and histogram against the restatement.  ``remap``: the
    tracker-list index of each entry of the list the restatement was fed."""
    rows, events, pairs, total = want
    if remap is not None:
        rows = [dict(r, track=int(remap[r["track"]])) for r in rows]
        events = [dict(e, track=int(remap[e["track"]])) for e in events]
    assert est.last_rows[k] == rows, where
    assert [ev_dict(e) for e in est.last_events[k]] == events[:est.max_events], where
    assert est.last_pairs[k] == pairs and est.last_total_pairs[k] == total, where
    assert est.snapshot(stream) == ref.snapshot(), where
    assert est.histogram(stream).tolist() == ref.hist, where


def run_host(pkg, plane, calls, **kw):
    est = pkg.events.SpeedEstimator(plane=plane, **kw)
    ref = R.SpeedRef(plane, **kw)
    out = []
    for t, rows in calls:
        want = ref.process(rows, t)
        got = est.process(tracks_of(rows), t)
        assert got is est.last_events[0]
        check(est, ref, want, f"t {t}")
        out.append(want)
    est.close()
    return ref, out


def test_hand_cases(pkg):
    """1. The CPU test's paper cases, one stream, max_tracks = 64; the literals are the ones worked out by hand."""
    for name, case in sorted(R.HAND_CASES.items()):
        ref, out = run_host(pkg, case["plane"], case["calls"], max_tracks=64, **case["kwargs"])
        assert [(k, e["kind"], e["speed_mm_s"]) for k, o in enumerate(out) for e in o[1]] == case["events"], name
        if case.get("speeds"):
            assert [o[0][0]["speed_mm_s"] for o in out] == case["speeds"] and [o[0][0]["odometer_mm"] for o in out] == case["odometer"]
            assert ref.hist == case["hist"]
        if case.get("pairs"):
            assert {k: o[2] for k, o in enumerate(out) if o[2]} == case["pairs"], name
        if "first_call_world" in case:
            assert [r["world"] for r in out[0][0]] == case["first_call_world"] and [r["track_id"] for r in out[0][0]] == case["first_call_ids"], name
    est = pkg.events.SpeedEstimator(mm_per_pixel=20, anchor="centre", max_tracks=8)      # the scale shorthand, the other anchor
    ref = R.SpeedRef(mm_per_pixel=20, anchor=R.CENTRE, max_tracks=8)
    for t, rows in [(5, [(1, [1, 2, 4, 9], 0)]), (9, [(1, [2, 2, 5, 9.5], 0)])]:
        want = ref.process(rows, t)
        est.process(tracks_of(rows), t)
        check(est, ref, want, f"t {t}")
    assert est.last_rows[0][0]["world"] == [70, 115] and est.label(1) == f"{(est.last_rows[0][0]['speed_mm_s'] * 36 + 5000) // 10000} km/h"
    assert est.label(2) == ""
    est.close()


def test_three_streams_different_planes(pkg):
    """2. Three streams of different lengths through one handle -- one of them empty -- each with its own plane and its own clock, all
    in one call; then one stream alone."""
    kw = dict(window=4, hold=2, limit_mm_s=300, stop_mm_s=120, stop_us=150_000, min_step_mm=10, proximity_mm=900, bins=6, bin_mm_s=400, classes=(0, 2), max_tracks=64)
    planes = [R.AFFINE_H, R.ROAD_H.reshape(9).tolist(), [7.0, 0, 0, 0, 7.0, 0, 0, 0, 1]]
    est = pkg.events.SpeedEstimator(n_streams=3, **kw)
    refs = [R.SpeedRef(p, **kw) for p in planes]
    for s, p in enumerate(planes):
        est.set_plane(p, stream=s)
    n_ev = 0
    for f in range(10):
        lists = [R.track_rows(9, f, seed=1, lattice=40), [] if f % 3 else R.track_rows(3, f, seed=2, lattice=40), R.track_rows(33, f, seed=3, lattice=40)[::-1]]
        lists[0] = [(i, [b[0] + 700, b[1] + 500, b[2] + 700, b[3] + 500], c) for i, b, c in lists[0]]
        t = [f * 100_000, f * 100_000 + 7, f * 50_000 + 1]
        want = [refs[s].process(lists[s], t[s]) for s in range(3)]
        got = est.process_batch([tracks_of(l) for l in lists], t)
        for s in range(3):
            check(est, refs[s], want[s], f"frame {f} stream {s}", k=s, stream=s)
            assert all(e.stream == s and e.class_name == f"c{e.class_id}" for e in got[s])
            n_ev += len(want[s][1])
    assert n_ev > 5 and sum(sum(r.hist) for r in refs) > 100
    rows = R.track_rows(5, 11, seed=1, lattice=40)
    want = refs[2].process(rows, 10 * SEC)
    est.process(tracks_of(rows), 10 * SEC, stream=2)
    check(est, refs[2], want, "stream 2 alone", stream=2)
    for s in (0, 1):
        assert est.snapshot(s) == refs[s].snapshot()
    est.close()


# ---- 3. the four trackers -------------------------------------------------------------------------------------------
S, N, FH, FW = 2, 32, 400, 400


def scene(f, s):
    """~12 objects in lanes 30 px apart moving right at 2..7 px a frame (stream 1: a different set); births, misses and deaths."""
    bx = []
    for k in range(12):
        born, dies, v = (k * 3) % 14, 40 - (k * 5) % 17, 2 + (k + 3 * s) % 6
        missed = (f + k) % 9 == 4 and k % 2 == s
        if born <= f < dies and not missed:
            x, y = 10.0 + v * f + (0.5 if k % 3 == 0 else 0.0), 12.0 + 30 * k + (f % 2) * 0.5
            bx.append([x, y, x + 20, y + 20])
    xy = np.float32(bx).reshape(-1, 4)
    return xy, np.full(len(xy), 0.9, np.float32), (np.arange(len(xy)) % 3).astype(np.int32)


def _trackers(pkg):
    T = pkg.tracking                     # (ByteTrack: match_thresh 0.3, so that a 20 px box moving 7 px a frame still matches)
    return {
        "bytetrack": (lambda: T.tracker._ByteTrackCore(0.5, 5, 0.3, n_streams=S, max_tracks=64, max_dets=N), False, lambda core, st: np.nonzero(st["tsu"] == 1)[0]),
        "deepsort": (lambda: T.deepsort._DeepSortCore(n_init=2, max_age=5, nn_budget=4, n_streams=S, max_tracks=64, max_dets=N), True,
                     lambda core, st: np.nonzero((st["state"] == 2) & (st["tsu"] == 0))[0]),
        "ocsort": (lambda: T.ocsort._OcSortCore(min_hits=2, n_streams=S, max_tracks=64, max_dets=N), False, lambda core, st: core.returned(st)),
        "botsort": (lambda: T.botsort._BotSortCore(n_streams=S, max_tracks=64, max_dets=N), False,
                    lambda core, st: np.nonzero((st["flag"] == 2) & (st["tsu"] == 0))[0]),
    }


@pytest.mark.parametrize("which", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_process_tracker_equals_process_on_the_passed_tracks(pkg, which):
    make, with_frames, passed = _trackers(pkg)[which]
    core = make()
    kw = dict(window=4, hold=2, limit_mm_s=2400, min_step_mm=0, proximity_mm=700, bins=8, bin_mm_s=500, max_gap_us=200_000, max_tracks=64)
    planes = [R.AFFINE_H, R.ROAD_H.reshape(9).tolist()]
    dev, host = (pkg.events.SpeedEstimator(n_streams=S, **kw) for _ in range(2))
    refs = [R.SpeedRef(p, **kw) for p in planes]
    for s, p in enumerate(planes):
        dev.set_plane(p, stream=s); host.set_plane(p, stream=s)
    frames = [np.random.default_rng(s).integers(0, 256, (FH, FW, 3), dtype=np.uint8) for s in range(S)]
    tracker = SimpleNamespace(_core=core, report="matched") if which == "bytetrack" else core
    n_state = n_pass = n_ev = n_pairs = 0
    for f in range(40):
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32); cnt = np.zeros(S, np.int32)
        for s in range(S):
            xy, cf, cl = scene(f, s)
            xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf, cl, len(cf)
        if with_frames:
            core.update_batch(xyxy, conf, cls, cnt, frames=frames)
        else:
            core.update_batch(xyxy, conf, cls, cnt)
        t = f * 40_000
        dev.process_tracker(tracker, t, class_names={0: "a", 1: "b", 2: "c"})
        for s in range(S):
            st = core.snapshot(s)
            idx = passed(core, st)
            n_state += len(st["ids"]); n_pass += len(idx)
            rows = [(int(st["ids"][i]), st["xyxy"][i], int(st["cls"][i])) for i in idx]
            want = refs[s].process(rows, t)
            check(dev, refs[s], want, f"{which} frame {f} stream {s} (device state)", k=s, stream=s, remap=idx)
            assert all(e.class_name == "abc"[e.class_id] for e in dev.last_events[s])
            host.process(tracks_of(rows), t, stream=s)
            check(host, refs[s], want, f"{which} frame {f} stream {s} (list)", stream=s)
            n_ev += len(want[1]); n_pairs += want[3]
    assert 0 < n_pass < n_state and n_ev > 0 and n_pairs > 0, (n_pass, n_state, n_ev, n_pairs)
    with pytest.raises(TypeError, match="process\\(tracks, t_us\\)"):
        dev.process_tracker(object(), 0)
    dev.close(); host.close(); core.close()


# ---- 4 .. 9 ----------------------------------------------------------------------------------------------------------
def test_300_tracks_and_a_few_hundred_pairs(pkg):
    """4. 300 tracks in one stream, max_tracks = 320: every loop runs past the workgroup's 256 threads, the ledger's binary searches see
    600 rows after the ids change, and the pair search delivers a few hundred pairs in (i, j) order; the lists arrive shuffled."""
    kw = dict(window=3, hold=2, limit_mm_s=300, stop_mm_s=40, stop_us=100_000, min_step_mm=15, proximity_mm=200, max_pairs=2048, max_events=1024,
              bins=16, bin_mm_s=50, max_gap_us=150_000, max_tracks=320)
    est, ref = pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    rng = np.random.default_rng(4)
    totals, n_ev = [], 0
    for f in range(7):
        rows = R.track_rows(300, f, seed=4)
        if f >= 4:                                                                 # new ids: the old 300 rows idle beside 300 new ones
            rows = [(i + 1000, b, c) for i, b, c in rows]
        rows = [rows[i] for i in rng.permutation(len(rows))]
        want = ref.process(rows, f * 100_000)
        est.process(tracks_of(rows), f * 100_000)
        check(est, ref, want, f"frame {f}")
        totals.append(want[3]); n_ev += len(want[1])
        if f == 4:
            assert len(ref.rows) == 600
    assert all(100 < t < 1500 for t in totals) and n_ev > 50 and not ref.pairs_truncated and not ref.events_truncated, (totals, n_ev)
    assert len(ref.rows) == 300                                                    # the first 300 have expired
    est.close()


def test_both_scans_end_at_a_workgroup_pass_then_one_row_too_many(pkg):
    """ledger_boundary.py: 255, 256 and 257 list entries beside 255, 256 and 257 idle rows (max_tracks = 600), ids that return inside
    max_gap_us and after it, a ledger exactly full and then over by one row: every call equals the restatement, the last one is
    E_CAPACITY with its own rows complete."""
    seq = B.calls()
    B.guards(seq)
    tick = 100_000
    kw = dict(window=3, hold=2, limit_mm_s=300, stop_mm_s=40, stop_us=tick, min_step_mm=15, max_events=2048, bins=16, bin_mm_s=50,
              max_gap_us=B.GAP * tick, max_tracks=B.MAX_TRACKS)
    est, ref = pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    n_ev = 0
    for step, ids, idle in seq:
        rows = [(i, R.box(20.0 + (i % 40) * 10 + ((step * (i % 5)) % 7), 52.0 + (i // 40 % 30) * 10), i % 3) for i in ids]
        before = set(ref.rows)
        want = ref.process(rows, step * tick)
        if step < B.LAST_STEP:
            assert not ref.ledger_overflow and len(ref.rows) - len(ids) == idle, step    # the restatement keeps the idle rows the sequence plans
            est.process(tracks_of(rows), step * tick)
            check(est, ref, want, f"step {step}")
            n_ev += len(want[1])
            continue
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            est.process(tracks_of(rows), step * tick)
        assert ref.ledger_overflow and len(before) == idle == 2 * B.MAX_TRACKS and not before & set(ids)      # 1200 idle rows + 1: they go
        assert e.value.code == pkg._ffi.E_CAPACITY and "ledger full" in str(e.value)
        assert est.last_rows[0] == want[0] and len(want[0]) == 1 and sorted(ref.rows) == ids       # this call's rows are complete all the same
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            est.snapshot()
        assert e.value.code == pkg._ffi.E_CAPACITY
        assert est.histogram().tolist() == ref.hist
    assert n_ev > 50 and not ref.events_truncated
    est.close()


def test_pairs_and_events_overflow(pkg):
    """5. max_pairs and max_events exceeded: E_CAPACITY, the first ones delivered, the totals reported, the ledger complete; the stream
    works on the next call."""
    kw = dict(window=2, hold=1, limit_mm_s=100, min_step_mm=0, proximity_mm=10_000, max_pairs=5, max_events=3, max_tracks=16)
    est, ref = pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    rows0 = [(i, R.box(10.0 * i, 52.0), 0) for i in range(1, 7)]
    rows1 = [(i, R.box(10.0 * i + 5, 52.0), 0) for i in range(1, 7)]               # all six speed: 6 events > 3; 15 pairs > 5
    want = ref.process(rows0[:3], 0)
    est.process(tracks_of(rows0[:3]), 0)
    check(est, ref, want, "three tracks: three pairs")
    want = ref.process(rows0, 50_000)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        est.process(tracks_of(rows0), 50_000)
    assert e.value.code == pkg._ffi.E_CAPACITY and "pairs" in str(e.value) and ref.pairs_truncated and not ref.events_truncated
    check(est, ref, want, "pairs overflow")
    assert want[3] == 15 and len(est.last_pairs[0]) == 5
    want = ref.process(rows1, 100_000)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        est.process(tracks_of(rows1), 100_000)
    assert e.value.code == pkg._ffi.E_CAPACITY and "events" in str(e.value) and ref.events_truncated and len(want[1]) == 6
    check(est, ref, want, "events and pairs overflow")
    assert [e.track_id for e in est.last_events[0]] == [1, 2, 3]
    want = ref.process(rows0[:2], 150_000)                                          # an ordinary call
    est.process(tracks_of(rows0[:2]), 150_000)
    check(est, ref, want, "after the overflow")
    est.close()


def test_ledger_full_is_an_error_code_and_sticks(pkg):
    """6. A ledger pushed past 2 x max_tracks rows: E_CAPACITY on that call and on every later call and snapshot of the stream; the
    histogram stays readable; another stream of the same handle is not affected."""
    kw = dict(window=2, min_step_mm=0, bins=2, bin_mm_s=100, max_gap_us=100 * SEC, max_tracks=4)
    est, ref = pkg.events.SpeedEstimator(plane=R.AFFINE_H, n_streams=2, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    for k, ids in enumerate(([1, 2, 3, 4], [5, 6, 7, 8], [5, 6, 7, 8], [9, 5], [5])):
        rows = [(i, R.box(10.0 + k, 52.0), 0) for i in ids]
        want = ref.process(rows, k * SEC)
        if not ref.ledger_overflow:
            est.process(tracks_of(rows), k * SEC)
            check(est, ref, want, f"call {k}")
            continue
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            est.process(tracks_of(rows), k * SEC)
        assert e.value.code == pkg._ffi.E_CAPACITY and "ledger full" in str(e.value), k
        assert est.last_rows[0] == want[0]                                          # this call's rows are complete all the same
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            est.snapshot()
        assert e.value.code == pkg._ffi.E_CAPACITY
    assert ref.ledger_overflow and est.histogram().tolist() == ref.hist and sum(ref.hist) == 6
    est.process(tracks_of([(1, R.box(5, 52), 0)]), 0, stream=1)
    assert len(est.snapshot(1)) == 1
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        est.process(tracks_of([(i, R.box(5, 52), 0) for i in range(5)]), 1, stream=1)      # 5 tracks > max_tracks: refused before any launch
    assert e.value.code == pkg._ffi.E_CAPACITY and len(est.snapshot(1)) == 1
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        est.process(tracks_of([(1, R.box(5, 52), 0), (1, R.box(6, 52), 0)]), 2, stream=1)    # duplicate id
    assert e.value.code == pkg._ffi.E_INVALID
    est.close()


def test_id_churn_and_refusals(pkg):
    """7. Ids that leave and return inside and outside max_gap_us; a timestamp that does not increase and a stream without a plane are
    refused and change nothing."""
    kw = dict(window=4, min_step_mm=0, stop_mm_s=30, stop_us=200_000, max_gap_us=300_000, max_tracks=16)
    est, ref = pkg.events.SpeedEstimator(n_streams=2, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        est.process(tracks_of([(1, R.box(1, 52), 0)]), 0)
    assert e.value.code == pkg._ffi.E_INVALID and "plane" in str(e.value)
    est.set_plane(R.AFFINE_H, stream=0)
    rng = np.random.default_rng(7)
    gone = {}
    for f in range(40):
        rows = []
        for i in range(1, 13):
            if gone.get(i, 0) > 0:
                gone[i] -= 1
                continue
            if rng.random() < 0.2:
                gone[i] = int(rng.integers(1, 6))                                  # away for 100 .. 500 ms: within and beyond the gap
                continue
            rows.append((i, R.box(10.0 * i + (f if i % 2 else 0) * 0.5, 52.0), i % 3))
        want = ref.process(rows, f * 100_000)
        est.process(tracks_of(rows), f * 100_000)
        check(est, ref, want, f"frame {f}")
    before = est.snapshot()
    for t in (39 * 100_000, 0):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            est.process(tracks_of([(1, R.box(1, 52), 0)]), t)
        assert e.value.code == pkg._ffi.E_INVALID and "not later" in str(e.value)
    assert est.snapshot() == before
    for bad in ([[1, 0, 0], [0, 1, 0], [1, 1, 0]], [[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]]):     # singular; non-finite
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            est.set_plane(bad, stream=1)
        assert e.value.code == pkg._ffi.E_INVALID
    with pytest.raises(pkg._ffi.RtmodtError):
        est.process(tracks_of([]), 0, stream=1)                                      # still no plane
    for kwargs in (dict(window=1), dict(window=33), dict(min_samples=1), dict(window=4, min_samples=5), dict(hold=0), dict(bins=257), dict(bins=4, bin_mm_s=0),
                   dict(proximity_mm=-1), dict(max_gap_us=-1), dict(allowed_dir=(1 << 21, 0))):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            pkg.events.SpeedEstimator(**kwargs)
        assert e.value.code == pkg._ffi.E_INVALID, kwargs
    est.close()


def test_ledger_follows_ids_the_swap_guard_exchanged(pkg):
    """8. ByteTrack exchanges the ids of two objects that pass each other, the swap guard exchanges them back inside the tracker's state,
    which leaves the tracker's list out of id order: the ledger rows are then placed by counting, and stay with their ids."""
    frames, h, w = SG.s1_frames()
    core = pkg.tracking.tracker._ByteTrackCore(0.5, 30, 0.8, n_streams=1, max_tracks=32, max_dets=16)
    guard = pkg.tracking.IdSwapGuard(n_streams=1, max_tracks=32)
    kw = dict(window=4, min_step_mm=0, proximity_mm=1500, max_tracks=32)
    dev, host, ref = pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    tracker = SimpleNamespace(_core=core, report="matched")
    reverted, out_of_order = 0, False
    for f, (img, xy, cf, cl) in enumerate(frames):
        xyxy = np.zeros((1, 16, 4), np.float32); conf = np.zeros((1, 16), np.float32); cls = np.zeros((1, 16), np.int32)
        xyxy[0, :len(xy)], conf[0, :len(xy)], cls[0, :len(xy)] = xy, cf, cl
        core.update_batch(xyxy, conf, cls, np.array([len(xy)], np.int32))
        reverted += len(guard.process_tracker(tracker, [img], f)[0])
        st = core.snapshot(0)
        out_of_order |= bool(np.any(np.diff(st["ids"]) <= 0))
        idx = np.nonzero(st["tsu"] == 1)[0]
        rows = [(int(st["ids"][i]), st["xyxy"][i], int(st["cls"][i])) for i in idx]
        want = ref.process(rows, f * 40_000)
        dev.process_tracker(tracker, f * 40_000)
        check(dev, ref, want, f"frame {f} (device state)", remap=idx)
        host.process(tracks_of(rows), f * 40_000)
        check(host, ref, want, f"frame {f} (list)")
    assert reverted == 1 and out_of_order
    assert [r[0] for r in ref.snapshot()] == [1, 2] and all(len(r[2]) == 4 for r in ref.snapshot())
    for x in (dev, host, guard, core):
        x.close()


def test_no_outputs_then_state(pkg):
    """9. Every output pointer null: nothing comes back, and the ledger and histogram are what a handle that fetched everything holds."""
    kw = dict(window=4, hold=2, limit_mm_s=300, min_step_mm=15, proximity_mm=300, bins=8, bin_mm_s=100, max_tracks=64)
    quiet, loud, ref = pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), pkg.events.SpeedEstimator(plane=R.AFFINE_H, **kw), R.SpeedRef(R.AFFINE_H, **kw)
    for f in range(6):
        rows = R.track_rows(40, f, seed=9, lattice=60)
        ref.process(rows, f * 100_000)
        assert quiet.process(tracks_of(rows), f * 100_000, outputs=False) == []
        loud.process(tracks_of(rows), f * 100_000)
    assert quiet.snapshot() == loud.snapshot() == ref.snapshot() and quiet.histogram().tolist() == loud.histogram().tolist() == ref.hist
    assert sum(ref.hist) > 0 and quiet.last_rows == [[]]
    assert quiet.histogram(reset=True).tolist() == ref.hist and quiet.histogram().tolist() == [0] * 8
    assert quiet.percentile(85) is None and loud.percentile(85) == R.percentile_of(ref.hist, 100, 85)
    quiet.close(); loud.close()


# ---- 10. the pipeline ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_speed")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    yield det
    det.close()


def test_pipeline_speed_stage(pkg, detector):
    """pipeline.run(speed=...) on the synthetic source: the same frame over and over, so every track stands still and fires STOPPED once;
    the device path (the tracker's device-resident state) and the host-list path report the same alarms.  Without an estimator the
    stage is absent."""
    src = pkg.synth.frames(1, 320, 320, seed=11)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    kw = dict(mm_per_pixel=10, window=4, stop_mm_s=50, stop_us=100_000, max_tracks=2048, fps=25.0)
    outs, snaps = [], []
    for handoff in (True, False):
        trk = pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
        trk.report = "matched"
        est = pkg.events.SpeedEstimator(**kw)
        p = prof()
        out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(src), detector, trk, p, max_frames=8, device_handoff=handoff, speed=est)
        assert "speed_mean_ms" in out and list(p.STAGE_ORDER).index("speed") == list(p.STAGE_ORDER).index("events") + 1
        outs.append(out); snaps.append(est.snapshot())
        n_tracks = int((trk._core.snapshot(0)["tsu"] == 1).sum())
        assert out["speed_events"] == n_tracks > 0, (out["speed_events"], n_tracks)
        est.close()
    assert outs[0]["speed_events"] == outs[1]["speed_events"] and snaps[0] == snaps[1]
    trk = pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(src), detector, trk, prof(), max_frames=2)
    assert "speed_events" not in base and "speed_mean_ms" not in base
    assert pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events", "visualization", "total"]
