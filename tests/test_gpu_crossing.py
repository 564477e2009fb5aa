"""GPU: the crossing counter (csrc/crossing.hip) against its plain-Python restatement (tests/crossing_ref.py): events, counts
and the ledger snapshot compared after every frame, with exact equality; everything through the C ABI."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import tracker_oracle as T
import crossing_ref as R
import ledger_boundary as B
import deepsort_ref as D

pytestmark = pytest.mark.gpu


def tracks_of(rows):
    return [SimpleNamespace(track_id=i, xyxy=np.asarray(b, np.float32), class_id=k, class_name=f"c{k}") for i, b, k in rows]


def as_dict(e):
    return dict(track_id=e.track_id, kind=e.event_type.split("_")[0], index=e.index, direction=e.direction, class_id=e.class_id, bbox_xyxy=e.bbox_xyxy,
                centroid=e.centroid, prev=e.previous, frames=e.frames)


def want_dict(e):
    return {k: v for k, v in e.items() if k != "track"}


def counts_of(counter, stream=0):
    c = counter.counts(stream)
    return {k: c[k].tolist() for k in ("line_total", "line_class", "gate_total", "gate_class")}


def check(counter, ref, got, want, where, stream=0):
    assert [as_dict(e) for e in got] == [want_dict(e) for e in want], where
    assert counter.snapshot(stream) == ref.snapshot(), where
    assert counts_of(counter, stream) == ref.counts(), where


def run_host(pkg, lines, gates, calls, **kw):
    """One stream: every call through CrossingCounter.process and the restatement, compared after every frame."""
    counter = pkg.events.CrossingCounter(lines, gates, **kw)
    ref = R.CrossingRef(lines, gates, **kw)
    n = 0
    for frame_id, rows in calls:
        want = ref.process(rows, frame_id)
        got = counter.process(tracks_of(rows), frame_id)
        check(counter, ref, got, want, f"frame {frame_id}")
        n += len(want)
    counter.close()
    return ref, n


def test_hand_cases(pkg):
    """The CPU test's paper cases, one stream, max_tracks = 64; the totals are the ones worked out by hand."""
    for name, case in sorted(R.HAND_CASES.items()):
        ref, _ = run_host(pkg, case.get("lines", ()), case.get("gates", ()), case["calls"], max_tracks=64, **case.get("kwargs", {}))
        if "line_total" in case:
            assert ref.line_total == case["line_total"], name
        if "gate_total" in case:
            assert ref.gate_total == case["gate_total"], name


def test_centroid_corner_cases(pkg):
    """A non-finite box is not passed (its row stays, a new id gets none), the clamp to +-2^20, truncation toward zero, a float32 sum
    that overflows, and class ids outside [0, C)."""
    far = {"name": "far", "a": [R.LIMIT - 10, -R.LIMIT], "b": [R.LIMIT - 10, R.LIMIT], "direction": "both"}
    gate = {"name": "g", "polygon": [[-6, -6], [-4, -6], [-4, 6], [-6, 6]], "direction": None}
    nan, inf = float("nan"), float("inf")
    calls = [
        (0, [(1, R.box(5, 10), 0), (2, [0, 0, 20, 20], 7), (3, [-7.5, -1, -2.25, 1], -1), (4, [3e38, 0, 3e38, 2], 3)]),
        (1, [(1, [nan, 0, 1, 1], 0), (5, [0, 0, inf, 1], 0), (2, [4e6, 0, 4e6, 20], 7), (3, [-7.5, -1, -4.25, 1], 3), (4, [0, 0, 2, 2], 3)]),
        (2, [(1, R.box(15, 10), 0), (5, [0, 0, 2, -inf], 0), (3, [-2.5, -1, -4.25, 1], 3)]),
    ]
    ref, n = run_host(pkg, [R.LINE_V, far], [gate], calls, max_tracks=64, n_classes=3)
    assert n == 5 and ref.line_total == [[1, 1], [1, 1]] and ref.gate_total == [1] and sorted(ref.rows) == [1, 2, 3, 4]
    assert ref.line_class[0] == [[0, 0, 0], [1, 0, 0]]                                   # track 1, class 0; track 4's class 3 is outside [0, 3)
    assert sum(map(sum, ref.line_class[1])) == 0 and sum(ref.gate_class[0]) == 0           # classes 7 and 3: totals only


def test_random_walk_three_streams(pkg):
    """3 streams through one handle, 150 ids each on a 96 x 96 lattice, 6 lines, 4 gates, 120 frames, ids that vanish for up to
    max_gap_frames + 3 frames and return, lists in shuffled order.  tests/test_crossing_cpu.py holds the guards that make this run
    meaningful; they are asserted here again on the very models the kernel was compared with."""
    kw = dict(n_classes=R.WALK["n_classes"], max_tracks=R.WALK["max_tracks"], max_events=R.WALK["max_events"], max_gap_frames=R.WALK["max_gap_frames"])
    counter = pkg.events.CrossingCounter(R.WALK_LINES, R.WALK_GATES, n_streams=R.WALK["n_streams"], **kw)
    models = R.walk_models()
    for s, frame_id, rows in R.walk_scenario():
        want = models[s].process(rows, frame_id)
        got = counter.process(tracks_of(rows), frame_id, stream=s)
        check(counter, models[s], got, want, f"stream {s} frame {frame_id}", stream=s)
    R.walk_guards(models)
    counter.close()


def test_more_than_one_pass_then_mostly_idle_rows(pkg):
    """max_tracks = 300 with 257, 300, 1 and 300 tracks passed: two passes of the 256-thread loops, then 299 idle rows around one passed."""
    ref, n = run_host(pkg, R.BOUNDARY_LINES, R.BOUNDARY_GATES, R.boundary_calls(), max_tracks=300, max_events=2048, max_gap_frames=10)
    assert n > 300 and len(ref.rows) == 300


def test_both_scans_end_at_a_workgroup_pass_then_one_row_too_many(pkg):
    """ledger_boundary.py: 255, 256 and 257 list entries beside 255, 256 and 257 idle rows (max_tracks = 600), ids that return inside
    max_gap_frames and after it, a ledger exactly full and then over by one row: every call equals the restatement, the last one is
    E_CAPACITY with the counts of the overflowing frame complete."""
    seq = B.calls()
    B.guards(seq)
    kw = dict(max_tracks=B.MAX_TRACKS, max_events=4096, max_gap_frames=B.GAP)
    counter = pkg.events.CrossingCounter(R.BOUNDARY_LINES, R.BOUNDARY_GATES, **kw)
    ref = R.CrossingRef(R.BOUNDARY_LINES, R.BOUNDARY_GATES, **kw)
    n_ev = 0
    for step, ids, idle in seq:
        rows = [(i, R.box(80 + 12 * ((step + i) % 4), 10 * (i % 300)), i % 90) for i in ids]
        want = ref.process(rows, step)
        assert len(ref.rows) - len(ids) == idle, step                                  # the restatement keeps the idle rows the sequence plans
        if step < B.LAST_STEP:
            assert not ref.ledger_overflow
            check(counter, ref, counter.process(tracks_of(rows), step), want, f"step {step}")
            n_ev += len(want)
            continue
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            counter.process(tracks_of(rows), step)
        assert ref.ledger_overflow and e.value.code == pkg._ffi.E_CAPACITY and "ledger full" in str(e.value)
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            counter.snapshot()
        assert e.value.code == pkg._ffi.E_CAPACITY
        assert counts_of(counter) == ref.counts()
    assert n_ev > 300 and len(ref.rows) == 2 * B.MAX_TRACKS + 1
    counter.close()


def test_event_overflow_truncates_events_not_counts(pkg):
    """max_events = 4, nine crossings in one frame: E_CAPACITY, the first four events in list order, all nine in the counts; the stream
    goes on working."""
    counter = pkg.events.CrossingCounter([R.NINE_LINE], max_tracks=64, max_events=4)
    ref = R.CrossingRef([R.NINE_LINE], max_tracks=64, max_events=4)
    (f0, rows0), (f1, rows1) = R.nine_crossings_calls()
    assert counter.last_events == [[]]                                                  # readable before the first call
    assert counter.process(tracks_of(rows0), f0) == ref.process(rows0, f0) == []
    want = ref.process(rows1, f1)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        counter.process(tracks_of(rows1), f1)
    assert e.value.code == pkg._ffi.E_CAPACITY and len(want) == 9 and ref.events_truncated
    check(counter, ref, counter.last_events[0], want[:4], "overflow frame")
    assert counts_of(counter)["line_total"] == [[0, 9]]
    rows2 = [(i, R.box(5, 10 * i), 1) for i in (2, 1)]                                  # two come back: an ordinary frame
    check(counter, ref, counter.process(tracks_of(rows2), f1 + 1), ref.process(rows2, f1 + 1), "after the overflow")
    assert counts_of(counter)["line_total"] == [[2, 9]]
    counter.close()


def test_ledger_full_is_an_error_code_and_sticks(pkg):
    """A ledger pushed past 2 x max_tracks rows: E_CAPACITY on that frame and on every later call and snapshot of the stream (the documented
    contract of rtmodt_crossing_create); the counts stay readable; another stream of the same handle is not affected."""
    counter = pkg.events.CrossingCounter([R.LINE_V], max_tracks=8, max_gap_frames=1000, n_streams=2)
    ref = R.CrossingRef([R.LINE_V], max_tracks=8, max_gap_frames=1000)
    for frame_id, ids in R.LEDGER_FULL_CALLS:
        rows = [(i, R.box(5 if frame_id < 3 else 15, 5), 0) for i in ids]
        want = ref.process(rows, frame_id)
        if not ref.ledger_overflow:
            check(counter, ref, counter.process(tracks_of(rows), frame_id), want, f"frame {frame_id}")
            continue
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            counter.process(tracks_of(rows), frame_id)
        assert e.value.code == pkg._ffi.E_CAPACITY and "ledger full" in str(e.value)
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            counter.snapshot()
        assert e.value.code == pkg._ffi.E_CAPACITY
    assert ref.ledger_overflow and counts_of(counter)["line_total"] == [[0, 1]]            # id 3 crossed at frame 3, before the ledger filled
    assert counter.process(tracks_of([(1, R.box(5, 5), 0)]), 0, stream=1) == [] and len(counter.snapshot(1)) == 1
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        counter.process(tracks_of([(i, R.box(5, 5), 0) for i in range(9)]), 9, stream=1)     # 9 tracks > max_tracks: refused before any launch
    assert e.value.code == pkg._ffi.E_CAPACITY and len(counter.snapshot(1)) == 1
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        counter.process(tracks_of([(1, R.box(5, 5), 0), (1, R.box(6, 5), 0)]), 10, stream=1)  # duplicate id
    assert e.value.code == pkg._ffi.E_INVALID
    counter.close()


def test_bytetrack_device_state(pkg):
    """process_tracker on a ByteTrack handle, 2 streams in one launch: boxes march over a line and through a gate (stream 1 the other way),
    one detection drops out for four frames; the restatement is fed from the tracker oracle's state (matched or spawned tracks)."""
    S, N = 2, 32
    core = pkg.tracking.tracker._ByteTrackCore(n_streams=S, max_tracks=64, max_dets=N)
    counter = pkg.events.CrossingCounter(R.MARCH_LINES, R.MARCH_GATES, n_streams=S, max_tracks=64, max_gap_frames=8)
    refs = [R.CrossingRef(R.MARCH_LINES, R.MARCH_GATES, max_tracks=64, max_gap_frames=8) for _ in range(S)]
    oras = [T.TrackerOracle() for _ in range(S)]
    scenes = [R.march_scene(), R.march_scene(reverse=True)]
    for f in range(len(scenes[0])):
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32); cnt = np.zeros(S, np.int32)
        for s in range(S):
            xy, cf, cl, _ = scenes[s][f]
            xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf, cl, len(cf)
        core.update_batch(xyxy, conf, cls, cnt)
        got = counter.process_tracker(SimpleNamespace(_core=core, report="matched"), f, class_names={0: "a", 1: "b", 2: "c"})
        for s in range(S):
            oras[s].update(*scenes[s][f][:3])
            st = oras[s].snapshot()
            passed = [(int(i), st["xyxy"][j], int(st["cls"][j])) for j, i in enumerate(st["ids"]) if st["tsu"][j] == 1]
            check(counter, refs[s], got[s], refs[s].process(passed, f), f"frame {f} stream {s}", stream=s)
            assert all(e.class_name == "abc"[e.class_id] and e.stream == s for e in got[s])
    # stream 0: the box that was not detected while it passed the line comes back under a new id (this tracker does not re-associate it), past
    # the line already: four "neg" crossings, and all five leave the gate left to right
    assert refs[0].line_total == [[0, 4]] and refs[0].gate_total == [5] and refs[0].gate_exits == [[5, 0]]
    assert refs[1].line_total == [[5, 0]] and refs[1].gate_total == [0] and refs[1].gate_exits == [[0, 5]]      # the other way: "pos", gate silent
    assert counter.process_tracker(SimpleNamespace(_core=core, report="reference"), 99) == [[], []]               # the reference's filter passes none
    core.close(); counter.close()


def test_deepsort_device_state(pkg):
    """The same scene through DeepSortTracker with caller descriptors; the restatement is fed from tests/deepsort_ref.py's state (confirmed
    tracks with time_since_update == 0).  One more box is over the line on its second frame, while its track is tentative: not counted."""
    dim, params = 64, dict(max_age=10, n_init=3, nn_budget=8)
    trk = pkg.DeepSortTracker(embedding_dim=dim, max_tracks=32, max_dets=16, **params)
    dref = D.DeepSortRef(dim=dim, **params)
    counter = pkg.events.CrossingCounter(R.MARCH_LINES, R.MARCH_GATES, max_tracks=32, max_gap_frames=8)
    ref = R.CrossingRef(R.MARCH_LINES, R.MARCH_GATES, max_tracks=32, max_gap_frames=8)
    with_tentative = R.CrossingRef(R.MARCH_LINES, R.MARCH_GATES, max_tracks=32, max_gap_frames=8)
    rng = np.random.default_rng(5)
    base = rng.normal(0, 1, (8, dim)).astype(np.float32)
    for f, (xy, cf, cl, obj) in enumerate(R.march_scene(early=True)):
        q = pkg._ffi.appearance_quantize((base[obj] + rng.normal(0, 0.05, (len(obj), dim))).astype(np.float32))
        trk.update(pkg.Detections(xy, cf, cl), embeddings=q)
        dref.update(xy, cf, cl, q)
        st = dref.snapshot()
        assert D.snapshots_equal(trk._core.snapshot(0), st) is None, f
        got = counter.process_tracker(trk, f)
        passed = [(int(i), st["xyxy"][j], int(st["cls"][j])) for j, i in enumerate(st["ids"]) if st["state"][j] == 2 and st["tsu"][j] == 0]
        check(counter, ref, got[0], ref.process(passed, f), f"frame {f}")
        with_tentative.process([(int(i), st["xyxy"][j], int(st["cls"][j])) for j, i in enumerate(st["ids"]) if st["tsu"][j] == 0], f)
    assert ref.line_total == [[0, 5]] and with_tentative.line_total == [[0, 6]] and ref.gate_total == [6]
    with pytest.raises(TypeError, match="process\\(tracks, frame_id\\)"):
        counter.process_tracker(object(), 0)
    trk.close(); counter.close()


def test_counts_are_cumulative_and_resettable(pkg, tmp_path):
    """reset_counts() zeroes the counts and leaves the ledger alone: a track halfway through a gate still fires on exit.  Also the
    JSON-lines log, and the reference's own zone list: one left_to_right crossing of exit_gate, none for the opposite walk."""
    default_zones = [
        {"name": "restricted_area", "polygon": [[100, 200], [400, 200], [400, 500], [100, 500]], "trigger": "intrusion", "dwell_time_sec": 2.0, "cooldown_sec": 10.0},
        {"name": "exit_gate", "polygon": [[500, 100], [700, 100], [700, 300], [500, 300]], "trigger": "crossing", "direction": "left_to_right"},
    ]
    log = tmp_path / "logs" / "crossings.jsonl"
    counter = pkg.events.CrossingCounter.from_zone_configs(default_zones, max_tracks=16, log_path=str(log))
    assert [(g["name"], g["direction"]) for g in counter.gates] == [("exit_gate", "left_to_right")] and counter.lines == []
    ref = R.CrossingRef([], R.gates_from_zone_configs(default_zones), max_tracks=16)
    path = [(450, 200), (520, 200), (600, 210), (690, 190), (750, 200)]
    frame = 0
    for tid, pts in ((1, path), (2, path[::-1]), (3, path)):                               # 1 and 3 walk left to right, 2 the opposite way
        for k, p in enumerate(pts):
            rows = [(tid, R.box(*p), 2)]
            check(counter, ref, counter.process(tracks_of(rows), frame), ref.process(rows, frame), f"frame {frame}")
            if tid == 3 and k == 2:                                                        # halfway through the gate
                before = counter.snapshot()
                counter.reset_counts(); ref.reset_counts()
                assert counts_of(counter)["gate_total"] == [0] and counter.snapshot() == before and before[-1][4] == [[0, 520, 200, frame - 1]]
            frame += 1
        assert counts_of(counter)["gate_total"] == [{1: 1, 2: 1, 3: 1}[tid]]               # cumulative: 1, still 1 after the opposite walk; 1 again after the reset
    lines = [json.loads(x) for x in open(log)]
    assert [(e["track_id"], e["name"], e["direction"], e["event_type"], e["class_name"]) for e in lines] == [
        (1, "exit_gate", "left_to_right", "gate_crossing", "c2"), (3, "exit_gate", "left_to_right", "gate_crossing", "c2")]
    assert lines[0]["previous"] == [520, 200] and lines[0]["centroid"] == [750, 200] and lines[0]["frames"] == 3
    counter.close()
