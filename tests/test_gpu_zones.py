"""GPU: the zone event kernel (csrc/zones.hip) against the fixture written by the reference's own
zone_engine.py and against the oracle; everything through the C ABI."""
import gzip
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import tracker_oracle as T
from oracle import zone_oracle as Z
from conftest import GOLDEN
import ledger_boundary as B
import zone_ref as R

pytestmark = pytest.mark.gpu


def load_cases():
    with gzip.open(os.path.join(GOLDEN, "zones_g1.json.gz"), "rt") as f:
        return json.load(f)


def as_dict(e):
    d = {k: getattr(e, k) for k in ("event_type", "zone_name", "track_id", "class_id", "dwell_time_sec", "bbox_xyxy", "centroid", "frame_id")}
    return d


@pytest.mark.parametrize("case", ["epoch_clock", "small_clock"])
def test_zone_engine_matches_reference_fixture(pkg, tmp_path, case):
    g = load_cases()
    eng = pkg.events.ZoneEventEngine(g["zones"], log_path=str(tmp_path / "ev" / "events.jsonl"), max_tracks=64)
    c = g["cases"][case]
    total = 0
    for fr, want in zip(c["frames"], c["expect"]):
        tracks = [SimpleNamespace(track_id=i, xyxy=np.asarray(b, np.float32), class_id=k, class_name="")
                  for i, b, k in zip(fr["ids"], fr["xyxy"], fr["cls"])]
        got = [as_dict(e) for e in eng.process(tracks, fr["frame_id"], now=fr["now"])]
        ref = [{k: v for k, v in e.items() if k != "class_name"} for e in want["events"]]
        assert got == ref, f"frame {fr['frame_id']}"
        snap = eng.snapshot()
        assert snap["occupancy"] == want["occupancy"], f"frame {fr['frame_id']}"
        assert snap["cooldown"] == want["cooldown"], f"frame {fr['frame_id']}"
        total += len(got)
    with open(tmp_path / "ev" / "events.jsonl") as f:          # the alert log (zone_engine.py:153-157)
        lines = [json.loads(x) for x in f]
    assert len(lines) == total > 30 and set(lines[0]) >= {"timestamp_utc", "event_type", "zone_name", "track_id", "dwell_time_sec", "centroid"}
    eng.close()


def test_point_in_polygon_vs_oracle_via_zero_dwell_zones(pkg, tmp_path):
    """Every zone with dwell 0 / cooldown 0 fires exactly when the centroid is inside or on the edge: sweeps a
    grid of integer centroids (vertices and edge points included) over concave and degenerate polygons."""
    polys = [[[10, 10], [60, 10], [60, 60], [35, 30], [10, 60]], [[0, 0], [8, 8], [16, 0], [16, 16], [0, 16]],
             [[20, 5], [40, 5], [40, 5], [55, 25], [30, 50], [5, 25]], [[70, 70], [90, 70]], [[3, 3]]]
    zones = [{"name": f"z{i}", "polygon": p, "dwell_time_sec": 0.0, "cooldown_sec": 0.0} for i, p in enumerate(polys)]
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), max_tracks=4096, max_events=8192)
    pts = [(x, y) for x in range(-2, 95, 1) for y in range(-2, 75, 2)][:4000]
    tracks = [SimpleNamespace(track_id=i + 1, xyxy=np.array([x - 3, y - 2, x + 3, y + 2], np.float32), class_id=0) for i, (x, y) in enumerate(pts)]
    got = {(e.track_id, e.zone_name) for e in eng.process(tracks, 0, now=100.0)}
    want = {(i + 1, f"z{k}") for i, (x, y) in enumerate(pts) for k, p in enumerate(polys) if Z.point_polygon_test(np.array(p, np.int32), x, y) >= 0}
    assert got == want and len(want) > 1000
    eng.close()


def test_zone_engine_on_device_resident_tracker(pkg, tmp_path):
    """process_tracker: zones evaluated on the tracker's device state (tracks matched/spawned this frame) for several
    streams in one launch, against the oracle fed from the tracker oracle's state."""
    zones = [{"name": "left", "polygon": [[0, 0], [320, 0], [320, 640], [0, 640]], "dwell_time_sec": 0.5, "cooldown_sec": 2.0},
             {"name": "mid", "polygon": [[200, 200], [440, 200], [440, 440], [200, 440]], "dwell_time_sec": 0.0, "cooldown_sec": 1.0}]
    S = 3
    core = pkg.tracking.tracker._ByteTrackCore(n_streams=S, max_tracks=256, max_dets=128)
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), n_streams=S, max_tracks=256, max_events=512)
    oras = [(T.TrackerOracle(), Z.ZoneOracle(zones)) for _ in range(S)]
    seqs = [pkg.synth.box_sequence(40 + 10 * s, 640, 50, seed=20 + s) for s in range(S)]
    rng = np.random.default_rng(0)
    now, n_total = 50.0, 0
    for f in range(50):
        now += 0.2
        xyxy = np.zeros((S, 128, 4), np.float32); conf = np.zeros((S, 128), np.float32); cls = np.zeros((S, 128), np.int32)
        cnt = np.zeros(S, np.int32)
        per = []
        for s in range(S):
            xy, cf, cl = seqs[s]
            keep = rng.random(len(cf)) > 0.15                       # detections drop out: tracks go unmatched, return later
            b, c, k = xy[f][keep], cf[keep], cl[keep]
            xyxy[s, :len(c)], conf[s, :len(c)], cls[s, :len(c)], cnt[s] = b, c, k, len(c)
            per.append((b, c, k))
        core.update_batch(xyxy, conf, cls, cnt)
        got = eng.process_tracker(SimpleNamespace(_core=core, report="matched"), f, now=now)
        for s in range(S):
            tor, zor = oras[s]
            tor.update(*per[s])
            st = tor.snapshot()
            passed = [(int(i), st["xyxy"][j], int(st["cls"][j])) for j, i in enumerate(st["ids"]) if st["tsu"][j] == 1]
            want = zor.process(passed, f, now)
            assert [as_dict(e) for e in got[s]] == want, f"frame {f} stream {s}"
            snap = eng.snapshot(s)
            live = set(int(i) for i in st["ids"])
            ref = zor.snapshot()
            assert snap["occupancy"] == ref["occupancy"], f"frame {f} stream {s}"
            assert snap["cooldown"] == [r for r in ref["cooldown"] if r[0] in live], f"frame {f} stream {s}"   # dead ids are dropped
            n_total += len(want)
    assert n_total > 50
    core.close(); eng.close()


def test_zone_engine_limits(pkg, tmp_path):
    zones = [{"name": "all", "polygon": [[0, 0], [1000, 0], [1000, 1000], [0, 1000]], "dwell_time_sec": 0.0, "cooldown_sec": 0.0}]
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), max_tracks=8, max_events=4)
    mk = lambda ids: [SimpleNamespace(track_id=i, xyxy=np.array([10, 10, 20, 20], np.float32), class_id=1) for i in ids]
    assert len(eng.process(mk([5, 3]), 0, now=1.0)) == 2
    assert [e.track_id for e in eng.process(mk([9, 3, 7]), 1, now=2.0)] == [9, 3, 7]            # caller's order, not id order
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        eng.process(mk([1, 1]), 2, now=3.0)                                                    # duplicate id
    assert e.value.code == pkg._ffi.E_INVALID
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        eng.process(mk(range(10, 19)), 3, now=4.0)                                             # 9 tracks > max_tracks
    assert e.value.code == pkg._ffi.E_CAPACITY
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        eng.process(mk(range(20, 26)), 4, now=5.0)                                             # 6 events > max_events (sticky)
    assert e.value.code == pkg._ffi.E_CAPACITY
    eng.close()
    eng = pkg.events.ZoneEventEngine([], log_path=str(tmp_path / "e2.jsonl"), max_tracks=8)    # no zones: nothing to do
    assert eng.process(mk([1, 2]), 0, now=1.0) == [] and eng.get_zone_polygons() == []
    eng.close()


def test_pipeline_loop_with_event_stage(pkg, tmp_path_factory, tmp_path):
    """tools/run_pipeline.py:121-158 incl. the `events` stage: detector -> tracker (report="matched", the opt-in
    corrected filter) -> zone engine; a whole-frame zero-dwell zone must fire once per reported track."""
    wdir = tmp_path_factory.mktemp("w")
    path = str(wdir / "n320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), warmup=False, autotune=False)
    trk = pkg.MultiObjectTracker("bytetrack")
    trk.report = "matched"
    zones = [{"name": "frame", "polygon": [[0, 0], [320, 0], [320, 320], [0, 320]], "dwell_time_sec": 0.0, "cooldown_sec": 1e9}]
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "events.jsonl"))
    prof = pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=2, log_interval=1000)
    frames = pkg.synth.frames(4, 320, 320, seed=3)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), det, trk, prof, max_frames=12, event_engine=eng)
    assert out["events_mean_ms"] > 0 and out["events_p50_ms"] > 0
    reported = set()
    trk2 = pkg.MultiObjectTracker("bytetrack")
    trk2.report = "matched"
    for i in range(12):
        reported |= {t.track_id for t in trk2.update(det.detect(frames[i % 4]))}
    assert out["events"] == len(reported) > 0              # cooldown 1e9: exactly one event per track id ever reported
    det.close(); eng.close()


# ======================================================================================================================
# The ledger at scale, under churn and at its limits: the engine against tests/zone_ref.py (ZoneOracle + the documented
# max_idle_frames / capacity contract) on every call -- events, occupancy and cooldown, compared with ==.  The scenarios
# and their non-vacuity guards are shared with tests/test_zone_ref_cpu.py, where the guards already ran without a GPU.
# ======================================================================================================================
def ns(tracks):
    return [SimpleNamespace(track_id=i, xyxy=b, class_id=k, class_name="") for i, b, k in tracks]


def check_call(eng, model, stream, frame_id, now, tracks, where):
    want = model.process(tracks, frame_id, now)
    got = [as_dict(e) for e in eng.process(ns(tracks), frame_id, stream=stream, now=now)]
    if got != want:                                             # name the first difference: frame, stream and id
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{where}: event {k} of {len(got)} / {len(want)}"
        assert len(got) == len(want), f"{where}: {len(got)} events, expected {len(want)}; first extra {(got + want)[min(len(got), len(want))]}"
    snap, ref = eng.snapshot(stream), model.snapshot()
    for part in ("occupancy", "cooldown"):
        if snap[part] != ref[part]:
            extra = [r for r in snap[part] if r not in ref[part]][:3]
            missing = [r for r in ref[part] if r not in snap[part]][:3]
            assert False, f"{where}: {part} differs: engine only {extra}, model only {missing}"


@pytest.mark.parametrize("max_idle", R.CHURN_IDLE)
def test_ledger_churn_at_scale_three_streams(pkg, tmp_path, max_idle):
    """a. ~1500 ids per stream leaving and returning, 300-700 passed per call, three streams of one engine interleaved
    (stream_base), n_old and n both far above 256: every rank of the merge, every pass of the prefix, expiry on both
    sides of max_idle_frames."""
    S = R.CHURN["n_streams"]
    eng = pkg.events.ZoneEventEngine(R.CHURN_ZONES, log_path=str(tmp_path / "e.jsonl"), n_streams=S, max_tracks=R.CHURN["max_tracks"],
                                     max_events=R.CHURN["max_events"], max_idle_frames=max_idle)
    models = [R.ZoneLedgerRef(R.CHURN_ZONES, R.CHURN["max_tracks"], max_idle) for _ in range(S)]
    for k, (s, frame_id, now, tracks) in enumerate(R.churn_scenario()):
        check_call(eng, models[s], s, frame_id, now, tracks, f"max_idle {max_idle} call {k} stream {s} frame {frame_id}")
    print("churn", max_idle, R.churn_guards(models, max_idle))
    eng.close()


@pytest.mark.parametrize("shared", [False, True], ids=["distinct_names", "shared_names"])
def test_thirty_two_zones_and_a_full_point_table(pkg, tmp_path, shared):
    """b. Z = 32 (key 31, event bit 31), 1954 of 2048 points with a 1500-vertex star and 0- / 1-point / repeated-vertex
    polygons, 600 tracks per frame with idle rows kept for 5 frames; then names z{i % 11}: shared keys in threes."""
    zones, calls = R.full_table_zones(shared), R.full_table_calls()
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), max_tracks=R.FULL["max_tracks"], max_events=R.FULL["max_events"],
                                     max_idle_frames=R.FULL["max_idle"])
    model = R.ZoneLedgerRef(zones, R.FULL["max_tracks"], R.FULL["max_idle"])
    for k, (s, frame_id, now, tracks) in enumerate(calls):
        check_call(eng, model, s, frame_id, now, tracks, f"call {k} frame {frame_id}")
    print("full table", shared, R.full_table_guards(model, zones, calls, shared))
    eng.close()


def test_zone_construction_limits(pkg, tmp_path):
    """b. 33 zones and 2049 points are refused; 32 zones with exactly 2048 points are not."""
    sq = [[0, 0], [10, 0], [10, 10], [0, 10]]
    mk = lambda polys: [{"name": f"z{i}", "polygon": p, "dwell_time_sec": 0.0, "cooldown_sec": 0.0} for i, p in enumerate(polys)]
    for polys in ([sq] * 33, [R.ngon(300, 300, 250, 2045), sq]):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            pkg.events.ZoneEventEngine(mk(polys), log_path=str(tmp_path / "e.jsonl"), max_tracks=8)
        assert e.value.code == pkg._ffi.E_INVALID
    zones = mk([R.ngon(300, 300, 250, 2048 - 31 * 4)] + [sq] * 31)
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), max_tracks=8)
    model = R.ZoneLedgerRef(zones, 8)
    tracks = [(1, np.array([0, 0, 10, 10], np.float32), 0), (2, np.array([290, 290, 310, 310], np.float32), 1), (3, np.array([900, 0, 910, 10], np.float32), 2)]
    check_call(eng, model, 0, 0, 1.7e9, tracks, "full table")
    assert model.n_events == 32
    eng.close()


@pytest.mark.parametrize("step", [0.25, 0.1])
def test_thresholds_met_exactly(pkg, tmp_path, step):
    """c. Clock steps of 0.25 (exact in double): now - first == dwell and now - last == cooldown occur as equalities and
    fire (>=); steps of 0.1: the rounded differences land on either side and the model decides.  One negative dwell."""
    eng = pkg.events.ZoneEventEngine(R.THRESH_ZONES, log_path=str(tmp_path / "e.jsonl"), max_tracks=64, max_events=256)
    model = R.ZoneLedgerRef(R.THRESH_ZONES, 64)
    for s, frame_id, now, tracks in R.threshold_calls(step):
        check_call(eng, model, s, frame_id, now, tracks, f"step {step} frame {frame_id}")
    print("thresholds", step, model.n_events, model.exact_threshold_firings)
    assert model.n_events > 100 and model.events_by_zone["neg"] > 0
    if step == 0.25:
        assert model.exact_threshold_firings >= 5
    eng.close()


def test_centroids_truncate_and_round_like_float32(pkg, tmp_path):
    """d. (x1 + x2) / 2 in float32, truncated toward zero: negative fractions, exact halves, sums above 2^24 that round;
    zone corners and edges on the truncated value and one pixel either side.  |coordinate| <= 2^26 (stated condition:
    the int32 differences of polygon.h, which mirror OpenCV's, cannot overflow there)."""
    zones, tracks = R.centroid_scenario()
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), max_tracks=16, max_events=256)
    model = R.ZoneLedgerRef(zones, 16)
    check_call(eng, model, 0, 0, 1.7e9, tracks, "frame 0")
    check_call(eng, model, 0, 1, 1.7e9 + 1.0, tracks[::-1], "frame 1")
    assert model.n_events == 4 * len(tracks)                    # per track and frame: the corner zone and the edge zone
    got = {e.track_id: e.centroid[0] for e in eng.process(ns(tracks), 2, now=1.7e9 + 2.0)}
    assert got == {i + 1: R.CENTROID_CASES[i][1] for i in range(len(tracks))}
    eng.close()


def test_both_scans_end_at_a_workgroup_pass_then_one_row_too_many(pkg, tmp_path):
    """ledger_boundary.py: 255, 256 and 257 list entries beside 255, 256 and 257 idle rows (max_tracks = 600), ids that return inside
    max_idle_frames and after it, a ledger exactly full and then over by one row: every call equals the model, the last one is
    E_CAPACITY and the handle stays in error."""
    seq = B.calls()
    B.guards(seq)
    zones = [{"name": "left", "polygon": [[0, 0], [300, 0], [300, 480], [0, 480]], "dwell_time_sec": 0.0, "cooldown_sec": 2.0},
             {"name": "band", "polygon": [[0, 100], [640, 100], [640, 300], [0, 300]], "dwell_time_sec": 1.0, "cooldown_sec": 0.0}]
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "e.jsonl"), max_tracks=B.MAX_TRACKS, max_events=2048, max_idle_frames=B.GAP)
    model = R.ZoneLedgerRef(zones, B.MAX_TRACKS, B.GAP)
    for step, ids, idle in seq:
        tracks = [(i, np.array([(i * 7 + step * 40) % 620, (i * 13) % 460, (i * 7 + step * 40) % 620 + 20, (i * 13) % 460 + 20], np.float32), i % 5) for i in ids]
        now = 1.7e9 + step
        if step < B.LAST_STEP:
            check_call(eng, model, 0, step, now, tracks, f"step {step}")
            assert model.history[-1] == (len(ids), idle, len(ids) + idle) and model.overflow is None, step
            continue
        model.process(tracks, step, now)
        assert model.overflow == step and model.rows == 2 * B.MAX_TRACKS + 1
        for attempt in (tracks, []):                            # the overflowing call, then any other
            with pytest.raises(pkg._ffi.RtmodtError) as e:
                eng.process(ns(attempt), step, now=now)
            assert e.value.code == pkg._ffi.E_CAPACITY
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            eng.snapshot()
        assert e.value.code == pkg._ffi.E_CAPACITY
    assert model.n_events > 300 and model.returned_live > 100 and model.returned_expired > 0
    eng.close()


def test_ledger_full(pkg, tmp_path):
    """e. max_tracks = 8: frames pass while passed + retained idle rows <= 16, the frame with exactly 16 included; the
    frame the model predicts raises E_CAPACITY, and from then on the handle stays in error: process and snapshot keep
    raising (include/rtmodt.h, rtmodt_zones_create)."""
    eng = pkg.events.ZoneEventEngine(R.EXPIRY_ZONE, log_path=str(tmp_path / "e.jsonl"), max_tracks=8, max_events=64)
    model = R.ZoneLedgerRef(R.EXPIRY_ZONE, 8)
    mk = lambda ids: [(i, np.array([10, 10, 20, 20], np.float32), 1) for i in ids]
    for frame_id, ids in R.LEDGER_FULL_CALLS[:-1]:
        check_call(eng, model, 0, frame_id, 1.7e9 + frame_id, mk(ids), f"frame {frame_id}")
    assert model.rows == 16 and model.overflow is None
    frame_id, ids = R.LEDGER_FULL_CALLS[-1]
    model.process(mk(ids), frame_id, 1.7e9 + frame_id)
    assert model.overflow == frame_id and model.rows == 17
    for attempt in (mk(ids), mk([1]), []):                      # the overflowing call, then any other
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            eng.process(ns(attempt), frame_id, now=1.7e9 + frame_id)
        assert e.value.code == pkg._ffi.E_CAPACITY
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        eng.snapshot()
    assert e.value.code == pkg._ffi.E_CAPACITY
    eng.close()


@pytest.mark.parametrize("name", ["calls_on_every_frame", "frame_ids_jump", "zero"])
def test_expiry_cases_derived_by_hand_on_engine(pkg, tmp_path, name):
    """The hand-derived cases of tests/test_zone_ref_cpu.py on the engine: max_idle_frames = 3 (0 for "zero"), zero dwell,
    cooldown 1e9 -- an id stays silent up to a gap of 3 frame ids and fires again from 4, whether or not calls were made
    in between."""
    calls, idle = (R.EXPIRY_ZERO, 0) if name == "zero" else (R.EXPIRY_CASES[name], 3)
    eng = pkg.events.ZoneEventEngine(R.EXPIRY_ZONE, log_path=str(tmp_path / "e.jsonl"), max_tracks=8, max_events=64, max_idle_frames=idle)
    model = R.ZoneLedgerRef(R.EXPIRY_ZONE, 8, idle)
    for k, (frame_id, ids, fires) in enumerate(calls):
        tracks = [(i, np.array([10, 10, 20, 20], np.float32), 0) for i in ids]
        got = sorted(e.track_id for e in eng.process(ns(tracks), frame_id, now=1.7e9 + 0.5 * k))
        assert got == sorted(fires), f"frame {frame_id}"
        model.process(tracks, frame_id, 1.7e9 + 0.5 * k)
        assert eng.snapshot() == model.snapshot(), f"frame {frame_id}"
    eng.close()


def test_tracker_source_at_scale(pkg, tmp_path):
    """f. process_tracker on four streams of 400-600 boxes with 15-30 % of the detections away at any time: lost tracks,
    expiry and compaction in the middle of the list, more than 512 rows in a stream -- against the tracker oracle plus
    the model's tracker-source mode.  One more frame with report="reference": nothing is passed, so no events, empty
    occupancy, cooldown untouched."""
    P = R.TRACKER
    S, N = P["n_streams"], P["max_dets"]
    core = pkg.tracking.tracker._ByteTrackCore(n_streams=S, max_dets=N, max_tracks=P["max_tracks"], track_buffer=P["track_buffer"])
    eng = pkg.events.ZoneEventEngine(R.TRACKER_ZONES, log_path=str(tmp_path / "e.jsonl"), n_streams=S, max_tracks=P["max_tracks"], max_events=4096)
    tor = [T.TrackerOracle(track_buffer=P["track_buffer"]) for _ in range(S)]
    models = [R.ZoneLedgerRef(R.TRACKER_ZONES, P["max_tracks"]) for _ in range(S)]
    frames, clock = R.tracker_inputs(pkg.synth.box_sequence)

    def step(f, report):
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32)
        cnt = np.zeros(S, np.int32)
        for s in range(S):
            b, c, k = frames[f][s]
            xyxy[s, :len(c)], conf[s, :len(c)], cls[s, :len(c)], cnt[s] = b, c, k, len(c)
        core.update_batch(xyxy, conf, cls, cnt)
        got = eng.process_tracker(SimpleNamespace(_core=core, report=report), f, now=clock[f])
        for s in range(S):
            tor[s].update(*frames[f][s])
            st = tor[s].snapshot()
            dev = core.snapshot(s)
            assert np.array_equal(dev["ids"], st["ids"]) and np.array_equal(dev["tsu"], st["tsu"]), f"frame {f} stream {s}: the tracker itself differs"
            want = models[s].process_tracker(st["ids"], st["tsu"], st["xyxy"], st["cls"], 1 if report == "matched" else 0, f, clock[f])
            assert [as_dict(e) for e in got[s]] == want, f"frame {f} stream {s}"
            assert eng.snapshot(s) == models[s].snapshot(), f"frame {f} stream {s}"
        return got

    for f in range(P["n_frames"]):
        step(f, "matched")
    print("tracker", R.tracker_guards(models))
    before = [m.snapshot()["cooldown"] for m in models]
    dead_before = [m.tracker_expired for m in models]
    got = step(P["n_frames"], "reference")
    for s in range(S):
        live = set(int(i) for i in tor[s].ids)
        assert got[s] == [] and eng.snapshot(s)["occupancy"] == []
        assert eng.snapshot(s)["cooldown"] == [r for r in before[s] if r[0] in live] and len(before[s]) > 50
    assert sum(m.tracker_expired for m in models) > sum(dead_before)         # ... while rows still leave with their tracks
    core.close(); eng.close()
