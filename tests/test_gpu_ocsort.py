"""GPU: the OC-SORT tracker (csrc/ocsort.hip) against its restatement (tests/ocsort_ref.py).  After every frame rtmodt_ocsort_state
equals the restatement's snapshot exactly -- integers as integers, float32 state as bit patterns -- and the returned count matches.
tests/test_ocsort_cpu.py shows every assignment optimum of these sequences unique with a margin, and that the three component scenes
change their identities when OCM / OCR / ORU is switched off.  PARITY UNPINNED: ocsort, boxmot and filterpy are not installed; the
restatement is the published algorithm as this project reads it."""
import ctypes as C
import os
import sys
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossing_ref  # noqa: E402
import ocsort_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def core_cls(pkg):
    return import_module(pkg.__name__ + ".tracking.ocsort")._OcSortCore


def _run_streams(pkg, names, max_tracks=32, max_dets=16):
    """Advance len(names) streams in one call per frame; compare the state with the restatement after every frame."""
    inputs = [R.sequence_inputs(n) for n in names]
    params = inputs[0][0]
    assert all(p == params for p, _ in inputs)
    S = len(names)
    core = core_cls(pkg)(n_streams=S, max_tracks=max_tracks, max_dets=max_dets, **params)
    refs = [R.OcSortRef(**params) for _ in names]
    for f in range(max(len(fr) for _, fr in inputs)):
        xy = np.zeros((S, max_dets, 4), np.float32); cf = np.zeros((S, max_dets), np.float32); cl = np.zeros((S, max_dets), np.int32)
        cnt, want = np.zeros(S, np.int32), []
        for s, (_, fr) in enumerate(inputs):
            b, c, k = fr[f] if f < len(fr) else (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
            n = len(b)
            xy[s, :n], cf[s, :n], cl[s, :n], cnt[s] = b, c, k, n
            want.append(len(refs[s].update(b, c, k)))
        ret = core.update_batch(xy, cf, cl, cnt)
        for s in range(S):
            got = core.snapshot(s)
            diff = R.snapshots_equal(got, refs[s].snapshot())
            assert diff is None, (names[s], f, diff)
            assert ret[s] == want[s] == len(core.returned(got)), (names[s], f)
    core.close()
    return refs


@pytest.mark.parametrize("name", ["ocm", "ocr", "oru"])
def test_component_scene_state_equals_restatement_bit_for_bit(pkg, name):
    """The scenes whose final identities change when the component is switched off in the restatement (tests/test_ocsort_cpu.py)."""
    ref = _run_streams(pkg, [name])[0]
    assert [t.id for t in ref.tracks] == ([1] if name == "ocr" else [1, 2])


@pytest.mark.parametrize("name", ["occlusion", "lifecycle", "byte_on", "byte_off", "inertia0", "delta_t1", "delta_t8", "empty"])
def test_sequence_state_equals_restatement_bit_for_bit(pkg, name):
    """Gaps below, at and past max_age; births and deaths of one-off detections; use_byte on and off with low-confidence detections
    (some exactly at a threshold); inertia = 0; delta_t 1 and 8; frames with no detection, and with no track."""
    ref = _run_streams(pkg, [name])[0]
    frames = R.sequence_inputs(name)[1]
    if name == "occlusion":       # max_age = 5: gaps of 3 and 5 frames are bridged, gaps of 6 and 9 are not: two new ids
        assert ref.next_id - 1 == 5 + 2
    if name == "lifecycle":
        assert ref.next_id - 1 > len(ref.tracks) + 5              # one-off detections were born and died
    if name in ("byte_on", "byte_off"):
        assert sum(int(((cf > np.float32(0.1)) & (cf < np.float32(0.6))).sum()) for _, cf, _ in frames) > 20
        assert sum(int((cf == np.float32(0.6)).sum() + (cf == np.float32(0.1)).sum()) for _, cf, _ in frames) > 3
    if name == "empty":
        assert len(frames[0][0]) == 0 and sum(len(xy) == 0 for xy, _, _ in frames) >= 7 and ref.next_id > 4


def test_eight_streams_with_ragged_counts_in_one_call(pkg):
    _run_streams(pkg, [f"stream{k}" for k in range(8)])


def test_250_tracks_against_950_detections(pkg):
    """A track count that is no multiple of 64 near the 256 x 1024 capacity, few contested pairs (tests/test_ocsort_cpu.py)."""
    ref = _run_streams(pkg, ["big"], max_tracks=256, max_dets=1024)[0]
    assert len(ref.tracks) == 250


def test_first_association_at_the_contested_pair_limit_and_past_it(pkg):
    """32 tracks against 64 detections that all overlap them: exactly 2048 admissible pairs, none isolated -- the most lap.h's edge
    array holds -- and the state equals the restatement.  One more track with a single pair into a contested column, 2049, is refused
    with E_CAPACITY: nothing faults, the state stays readable, and the handle answers again after a reset."""
    ffi = pkg._ffi
    ref = _run_streams(pkg, ["limit"], max_tracks=128, max_dets=64)[0]
    assert len(ref.tracks) == 64 and sum(t.hits == 1 for t in ref.tracks) == 32
    params = R.SEQUENCES["limit"][0]
    core = core_cls(pkg)(n_streams=1, max_tracks=128, max_dets=64, **params)
    frames = R.pair_limit_frames(True)
    assert core.update(*frames[0]) == 33 and len(core.snapshot(0)["ids"]) == 33
    with pytest.raises(ffi.RtmodtError) as e:
        core.update(*frames[1])
    assert e.value.code == ffi.E_CAPACITY and "contested" in e.value.msg
    with pytest.raises(ffi.RtmodtError) as e:                                     # sticky
        core.snapshot(0)
    assert e.value.code == ffi.E_CAPACITY
    st = core.snapshot(0, allow_capacity=True)                                    # ... and readable: a well-formed list
    assert st["error"] == ffi.E_CAPACITY and st["frame_count"] == 2 and 33 <= len(st["ids"]) <= 97 and (np.diff(st["ids"]) > 0).all()
    assert np.isfinite(st["mean"]).all() and st["next_id"] == st["ids"].max() + 1
    core.reset()
    assert len(core.snapshot(0)["ids"]) == 0 and core.snapshot(0)["frame_count"] == 0
    xy, cf, cl = frames[0]
    assert core.update(xy[:3], cf[:3], cl[:3]) == 3 and len(core.snapshot(0)["ids"]) == 3
    core.close()


def test_limits_and_bad_arguments_return_codes(pkg):
    ffi = pkg._ffi
    L = ffi.lib()
    core = core_cls(pkg)(n_streams=2, max_tracks=4, max_dets=8, max_age=3, min_hits=1)
    xy = np.zeros((2, 8, 4), np.float32)
    xy[:, :, :] = np.asarray([[4 + 40 * k, 5, 34 + 40 * k, 65] for k in range(8)], np.float32)
    one, zero = np.full((2, 8), 0.9, np.float32), np.zeros((2, 8), np.int32)
    for bad_n, code in ((9, ffi.E_CAPACITY), (-1, ffi.E_INVALID)):
        cnt = np.asarray([1, bad_n], np.int32)
        assert L.rtmodt_ocsort_update_batch(core._h, ffi.ptr(xy), ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt), None) == code
    cnt = np.asarray([2, 0], np.int32)
    assert L.rtmodt_ocsort_update_batch(core._h, None, ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt), None) == ffi.E_INVALID      # null detections
    assert L.rtmodt_ocsort_update_batch(core._h, ffi.ptr(xy), ffi.ptr(one), ffi.ptr(zero), None, None) == ffi.E_INVALID
    assert L.rtmodt_ocsort_update_batch(None, ffi.ptr(xy), ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt), None) == ffi.E_INVALID
    assert L.rtmodt_ocsort_state(core._h, 2, *([None] * 14)) == ffi.E_INVALID and L.rtmodt_ocsort_state(core._h, -1, *([None] * 14)) == ffi.E_INVALID
    assert L.rtmodt_ocsort_reset(core._h, 2) == ffi.E_INVALID and L.rtmodt_ocsort_reset(None, 0) == ffi.E_INVALID
    assert L.rtmodt_ocsort_last_ms(core._h, None) == ffi.E_INVALID                # no update has run yet
    assert L.rtmodt_ocsort_update_from_detector(core._h, None) == ffi.E_INVALID
    assert L.rtmodt_crossing_process_ocsort(None, core._h, 0, None, None) == ffi.E_INVALID
    for s in range(2):
        assert len(core.snapshot(s)["ids"]) == 0 and core.snapshot(s)["frame_count"] == 0      # none of the refused calls touched the state
    with pytest.raises(ValueError):
        core.update(xy[0, :1], one[0, :1], zero[0, :1])                           # update() drives one stream
    # more live tracks than max_tracks in stream 1 only: sticky capacity error there, stream 0 goes on
    with pytest.raises(ffi.RtmodtError) as e:
        core.update_batch(xy, one, zero, np.asarray([2, 5], np.int32))
    assert e.value.code == ffi.E_CAPACITY and "max_tracks" in e.value.msg
    assert len(core.snapshot(0)["ids"]) == 2 and len(core.snapshot(1, allow_capacity=True)["ids"]) == 4
    assert core.last_ms() >= 0
    core.reset(1)
    assert len(core.snapshot(0)["ids"]) == 2 and len(core.snapshot(1)["ids"]) == 0
    core.close()
    h = C.c_void_p()
    cfg = ffi.OcSortCfg(0.6, 0.1, 0.05, 0.2, 30, 3, 3, 0, 32, 16, 1, 0)
    assert L.rtmodt_ocsort_create(C.byref(cfg), C.byref(h)) == ffi.E_INVALID and not h.value     # iou_threshold <= inertia / 2
    # odd capacities: every state array still starts on its own 16-byte boundary
    params, frames = R.sequence_inputs("stream3")
    core, ref = core_cls(pkg)(n_streams=1, max_tracks=7, max_dets=5, **params), R.OcSortRef(**params)
    for f, (b, c, k) in enumerate(frames):
        assert core.update(b, c, k) == len(ref.update(b, c, k)) and R.snapshots_equal(core.snapshot(0), ref.snapshot()) is None, f
    core.close()


@pytest.fixture(scope="module")
def wdir(tmp_path_factory):
    return tmp_path_factory.mktemp("weights_ocsort")


def _weights(pkg, wdir):
    path = os.path.join(str(wdir), "yolov8n_320_noise.rtw")
    if not os.path.exists(path):
        pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    return path


def test_update_from_detector_equals_the_same_detections_fed_by_hand(pkg, wdir):
    B = 2
    det = pkg.Detector(_weights(pkg, wdir), input_size=(320, 320), confidence=0.02, max_det=20, batch=B, warmup=False, autotune=False)
    params = dict(max_age=4, min_hits=2, det_thresh=0.05, low_thresh=0.0, use_byte=True)
    a = core_cls(pkg)(n_streams=B, max_tracks=128, max_dets=20, **params)
    b = core_cls(pkg)(n_streams=B, max_tracks=128, max_dets=20, **params)
    refs = [R.OcSortRef(**params) for _ in range(B)]
    frames = pkg.synth.frames(4 * B, 320, 320, seed=77)
    total = 0
    for t in range(4):
        fr = [frames[t * B + i] for i in range(B)]
        det.enqueue(fr)
        a.update_from_detector(det)
        got = det.fetch()
        xy = np.zeros((B, 20, 4), np.float32); cf = np.zeros((B, 20), np.float32); cl = np.zeros((B, 20), np.int32)
        cnt = np.zeros(B, np.int32)
        for i, d in enumerate(got):
            n = len(d)
            xy[i, :n], cf[i, :n], cl[i, :n], cnt[i] = d.xyxy, d.confidence, d.class_id, n
            refs[i].update(d.xyxy, d.confidence, d.class_id)
            total += n
        b.update_batch(xy, cf, cl, cnt)
        for i in range(B):
            sa, sb = a.snapshot(i), b.snapshot(i)
            assert R.snapshots_equal(sa, sb) is None, (t, i, R.snapshots_equal(sa, sb))
            assert R.snapshots_equal(sb, refs[i].snapshot()) is None, (t, i)
    assert total > 0 and a.last_ms() >= 0
    a.close(); b.close(); det.close()


def _as_dict(e):
    return dict(track_id=e.track_id, kind=e.event_type, index=e.index, direction=e.direction, class_id=e.class_id, bbox_xyxy=e.bbox_xyxy,
                centroid=e.centroid, prev=e.previous, frames=e.frames)


def test_crossing_counter_on_device_state_equals_the_materialised_list(pkg):
    """Boxes march over a line and through a gate, one is not detected for four frames and one is over the line on its second frame:
    rtmodt_crossing_process_ocsort on the device state against CrossingCounter.process on the list OcSortTracker returns, and both
    against the crossing restatement fed from the OC-SORT restatement's returned tracks."""
    CR = crossing_ref
    params = dict(max_age=10, min_hits=3)
    trk = pkg.OcSortTracker(max_tracks=32, max_dets=16, **params)
    oref = R.OcSortRef(**params)
    kw = dict(max_tracks=32, max_gap_frames=8)
    on_device, on_list = pkg.events.CrossingCounter(CR.MARCH_LINES, CR.MARCH_GATES, **kw), pkg.events.CrossingCounter(CR.MARCH_LINES, CR.MARCH_GATES, **kw)
    ref = CR.CrossingRef(CR.MARCH_LINES, CR.MARCH_GATES, **kw)
    n_events = 0
    for f, (xy, cf, cl, _) in enumerate(CR.march_scene(early=True)):
        tracks = trk.update(pkg.Detections(xy, cf, cl))
        idx = oref.update(xy, cf, cl)
        assert R.snapshots_equal(trk._core.snapshot(0), oref.snapshot()) is None, f
        assert [(t.track_id, tuple(t.xyxy)) for t in tracks] == [(i, tuple(b)) for i, b in oref.tracks_out(idx)], f
        got_dev = on_device.process_tracker(trk, f)[0]
        got_list = on_list.process(tracks, f)
        want = ref.process([(oref.tracks[i].id, oref.tracks[i].box, oref.tracks[i].cls) for i in idx], f)
        assert [_as_dict(e) for e in got_dev] == [_as_dict(e) for e in got_list], f
        assert [dict(_as_dict(e), kind=e.event_type.split("_")[0]) for e in got_dev] == [{k: v for k, v in e.items() if k != "track"} for e in want], f
        assert on_device.snapshot() == on_list.snapshot() == ref.snapshot(), f
        cd, cl_ = on_device.counts(), on_list.counts()
        assert all(np.array_equal(cd[k], cl_[k]) for k in ("line_total", "line_class", "gate_total", "gate_class")), f
        n_events += len(got_dev)
    assert n_events > 8 and ref.gate_total == [6]
    assert on_device.process_tracker(SimpleNamespace(_core=trk._core), 99) == [[]]
    trk.close(); on_device.close(); on_list.close()


def test_facade_tracks_trails_and_config(pkg):
    params, frames = R.sequence_inputs("oru")
    trk = pkg.OcSortTracker.from_config({"algorithm": "bytetrack", "ocsort": dict(params, max_tracks=32, max_dets=16, unknown_key=1)})
    ref = R.OcSortRef(**params)
    out = []
    for f, (xy, cf, cl) in enumerate(frames):
        out = trk.update(pkg.Detections(xy, cf, cl))
        want = ref.tracks_out(ref.update(xy, cf, cl))
        assert [t.track_id for t in out] == [i for i, _ in want], f
        assert all(np.array_equal(t.xyxy.view(np.int32), b.view(np.int32)) and t.time_since_update == 0 for t, (_, b) in zip(out, want)), f
    assert [t.track_id for t in out] == [1] and len(out[0].trail) > 1 and trk.algorithm == "ocsort" and trk.needs_frame is False
    assert trk.update(pkg.Detections(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))) == []
    trk.close()


@pytest.mark.parametrize("handoff", [True, False])
def test_pipeline_run_with_ocsort_zone_events_and_crossings(pkg, wdir, tmp_path, handoff):
    """pipeline.run(OcSortTracker, event_engine=ZoneEventEngine, crossing_counter=CrossingCounter), with and without the device hand-off
    of the detections: the tracks reach both consumers as a list, and the events, the crossings and the tracker's final state are the
    ones a hand-driven replay of the same loop produces.  The counter alone reads the tracker's state on the device."""
    det = pkg.Detector(_weights(pkg, wdir), input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    params = dict(max_age=4, min_hits=2, det_thresh=0.0, low_thresh=0.0, max_tracks=128, max_dets=20)
    zones = [{"name": "frame", "polygon": [[0, 0], [320, 0], [320, 320], [0, 320]], "dwell_time_sec": 0.0, "cooldown_sec": 1e9}]
    lines = [{"name": "mid", "a": [160, 0], "b": [160, 320], "direction": "both"}]
    frames = pkg.synth.frames(3, 320, 320, seed=5)

    def parts(tag):
        return (pkg.OcSortTracker(**params), pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / f"events_{tag}.jsonl")),
                pkg.events.CrossingCounter(lines, (), max_tracks=128))

    trk, eng, cnt = parts("run")
    prof = pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=2, log_interval=1000)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), det, trk, prof, max_frames=9, event_engine=eng, crossing_counter=cnt,
                           device_handoff=handoff)
    trk2, eng2, cnt2 = parts("replay")
    events = crossings = 0
    last = []
    for i in range(9):
        last = trk2.update(det.detect(frames[i % 3]))
        events += len(eng2.process(last, i + 1))               # SyntheticSource numbers its frames from 1
        crossings += len(cnt2.process(last, i + 1))
    assert events > 0 and out["events"] == events and out["crossings"] == crossings and out["last_tracks"] == len(last)
    assert R.snapshots_equal(trk._core.snapshot(0), trk2._core.snapshot(0)) is None
    assert cnt.snapshot() == cnt2.snapshot()
    with pytest.raises(TypeError, match="process\\(tracks, frame_id\\)"):
        eng.process_tracker(trk, 99)
    # the counter alone, hand-off on: pipeline.run leaves the list on the device and the counter reads the state there
    trk3, _, cnt3 = parts("alone")
    out3 = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), det, trk3, pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=2, log_interval=1000),
                            max_frames=9, crossing_counter=cnt3, device_handoff=handoff)
    assert out3["crossings"] == crossings and cnt3.snapshot() == cnt2.snapshot()
    for x in (trk, trk2, trk3, eng, eng2, cnt, cnt2, cnt3, det):
        x.close()
