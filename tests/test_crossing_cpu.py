"""CPU: the crossing counter's restatement (tests/crossing_ref.py, the authority for csrc/crossing.hip) against cases small
enough to verify on paper, the seeded scenarios' non-vacuity guards, and the Python face's plumbing that needs no GPU."""
import inspect
import re

import numpy as np
import pytest

import crossing_ref as R


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_hand_case(name):
    case = R.HAND_CASES[name]
    m = R.run_case(case)
    if "line_total" in case:
        assert m.line_total == case["line_total"], name
    if "gate_total" in case:
        assert m.gate_total == case["gate_total"], name
    assert not m.ledger_overflow and not m.events_truncated


def test_rules_one_by_one():
    a, b = (10, 0), (10, 20)
    assert [R.side(a, b, p) for p in [(5, 3), (10, -50), (15, 3)]] == [1, 0, -1]
    assert R.path_meets_segment((5, 10), (15, 10), a, b) and not R.path_meets_segment((5, 30), (15, 30), a, b)
    assert R.path_meets_segment((0, 30), (20, 10), a, b)                               # through B itself
    assert R.path_meets_segment((0, -10), (20, 10), a, b)                              # through A itself
    assert R.line_step(0, a, b, None, (5, 3)) == (1, None)                             # fresh row: the side is stored, nothing fires
    assert R.line_step(1, a, b, (5, 3), (10, 3)) == (1, None)                          # on the line: the stored side stays
    assert R.line_step(1, a, b, (10, 3), (15, 3)) == (-1, "neg")
    assert R.line_step(-1, a, b, (15, 3), (5, 3)) == (1, "pos")
    assert R.line_step(1, a, b, (5, 30), (15, 30)) == (-1, None)                       # past the end: the side flips, no count
    assert [R.gate_fires(d, 5, 5) for d in R.GATE_DIRECTIONS] == [True, True, False, True, False]       # the tie fires both axes it points along
    assert [R.gate_fires(d, -5, 4) for d in R.GATE_DIRECTIONS] == [True, False, True, False, False]
    assert [R.gate_fires(d, 0, 0) for d in R.GATE_DIRECTIONS] == [True, False, False, False, False]     # no displacement: only a gate without a direction
    assert [R.gate_fires(d, 3, -4) for d in R.GATE_DIRECTIONS] == [True, False, False, False, True]


def test_centroid_truncates_clamps_and_refuses_non_finite():
    assert R.centroid([-7.5, 0, -2.25, 1]) == (-4, 0)                                  # -4.875 truncates toward zero (the zone engine's rule)
    assert R.centroid([10, -10, 11, -11]) == (10, -10)
    assert R.centroid([3e6, -3e6, 3e6, -3e6]) == (R.LIMIT, -R.LIMIT)                    # the clamp
    assert R.centroid([1048577, 0, 1048579, 0]) == (R.LIMIT, 0) and R.centroid([1048575, 0, 1048577, 0]) == (R.LIMIT, 0)
    assert R.centroid([1048574, 0, 1048576, 0]) == (R.LIMIT - 1, 0) and R.centroid([-1048574, 0, -1048581, 0]) == (-R.LIMIT, 0)
    assert R.centroid([3e38, 0, 3e38, 0]) == (R.LIMIT, 0)                              # the float32 sum overflows to inf: clamped, still passed
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(4):
            b = [1.0, 2.0, 3.0, 4.0]
            b[k] = bad
            assert R.centroid(b) is None


def test_non_finite_box_is_not_passed_and_keeps_the_row():
    m = R.CrossingRef([R.LINE_V], [], max_tracks=8, max_gap_frames=5)
    m.process([(1, R.box(5, 10), 0)], 0)
    before = m.snapshot()
    assert m.process([(1, np.array([np.nan, 0, 1, 1], np.float32), 0), (2, np.array([0, 0, np.inf, 1], np.float32), 0)], 1) == []
    assert m.snapshot() == before                                                      # id 1 untouched, id 2 got no row
    ev = m.process([(1, R.box(15, 10), 0)], 2)
    assert len(ev) == 1 and ev[0]["frames"] == 2 and ev[0]["prev"] == [5, 10] and ev[0]["direction"] == "neg"


def test_clamped_centroids_still_cross():
    line = {"name": "far", "a": [R.LIMIT - 10, -R.LIMIT], "b": [R.LIMIT - 10, R.LIMIT], "direction": "both"}
    m = R.CrossingRef([line], [], max_tracks=8)
    m.process([(1, np.array([0, 0, 20, 20], np.float32), 0)], 0)
    ev = m.process([(1, np.array([4e6, 0, 4e6, 20], np.float32), 0)], 1)                # clamps to x = 2^20: beyond the line
    assert [e["centroid"] for e in ev] == [[R.LIMIT, 10]] and m.line_total == [[0, 1]]


def test_class_outside_range_enters_totals_only():
    m = R.CrossingRef([R.LINE_V], [{"name": "g", "polygon": R.SQUARE, "direction": None}], n_classes=3, max_tracks=8)
    for f, x in enumerate([5, 15, 35]):                                                # over the line, into the square, out of it
        m.process([(1, R.box(x, 20), 3), (2, R.box(x, 15), -1), (3, R.box(x, 12), 2)], f)
    assert m.line_total == [[0, 3]] and m.line_class == [[[0, 0, 0], [0, 0, 1]]]
    assert m.gate_total == [3] and m.gate_class == [[0, 0, 1]]


def test_event_fields_and_order():
    lines = [R.LINE_V, {"name": "v2", "a": [12, 40], "b": [12, 0], "direction": "both"}]
    m = R.CrossingRef(lines, [{"name": "g", "polygon": [[0, 0], [8, 0], [8, 40], [0, 40]], "direction": "left_to_right"}], max_tracks=8)
    m.process([(9, R.box(5, 10), 1), (4, R.box(6, 30), 2)], 7)
    ev = m.process([(9, R.box(15, 10), 1), (4, R.box(16, 30), 2)], 9)
    assert [(e["track_id"], e["track"], e["kind"], e["index"], e["direction"]) for e in ev] == [
        (9, 0, "line", 0, "neg"), (9, 0, "line", 1, "pos"), (9, 0, "gate", 0, "left_to_right"),
        (4, 1, "line", 1, "pos"), (4, 1, "gate", 0, "left_to_right")]                  # list order, lines in order, then gates; y = 30 is past LINE_V's end
    assert ev[0]["frames"] == 2 and ev[0]["prev"] == [5, 10] and ev[0]["centroid"] == [15, 10] and ev[0]["bbox_xyxy"] == [10.0, 6.0, 20.0, 14.0]
    assert ev[2]["prev"] == [5, 10] and ev[2]["frames"] == 2                           # a gate reports where and when the track entered
    assert m.snapshot() == [[4, 9, [16, 30], [-1, 1], []], [9, 9, [15, 10], [-1, 1], []]]


def test_walk_scenario_guards():
    """The seed of the random walk was picked so that the restatement alone sees every kind of thing the GPU comparison is about."""
    models = R.walk_models()
    n_events = 0
    for s, frame_id, tracks in R.walk_scenario():
        ev = models[s].process(tracks, frame_id)
        n_events += len(ev)
        assert not models[s].events_truncated
    fig = R.walk_guards(models)
    assert n_events > 3000 and fig["within"] > 100 and fig["after"] > 100, (n_events, fig)


def test_boundary_scenarios_are_what_they_claim():
    m = R.CrossingRef(R.BOUNDARY_LINES, R.BOUNDARY_GATES, n_classes=80, max_tracks=300, max_events=2048, max_gap_frames=10)
    sizes, rows, events = [], [], []
    for f, tracks in R.boundary_calls():
        events.append(len(m.process(tracks, f)))
        sizes.append(len(tracks)); rows.append(len(m.rows))
    assert sizes == [257, 300, 1, 300] and rows == [257, 300, 300, 300] and events[1] > 100 and events[3] > 100 and not m.ledger_overflow
    m = R.CrossingRef([R.NINE_LINE], [], max_tracks=64, max_events=4)
    ev = [m.process(t, f) for f, t in R.nine_crossings_calls()][-1]
    assert len(ev) == 9 and m.events_truncated and [e["track_id"] for e in ev[:4]] == [9, 8, 7, 6] and m.line_total == [[0, 9]]
    m = R.CrossingRef([R.LINE_V], [], max_tracks=8, max_gap_frames=1000)
    full = []
    for f, ids in R.LEDGER_FULL_CALLS:
        m.process([(i, R.box(5, 5), 0) for i in ids], f)
        full.append(m.ledger_overflow)
    assert full == [False, False, False, False, True, True]


def test_from_zone_configs_takes_exactly_the_crossing_zones(pkg):
    """config/default.yaml:62-77: the reference's two default zones yield one gate, exit_gate, left_to_right."""
    default_zones = [
        {"name": "restricted_area", "polygon": [[100, 200], [400, 200], [400, 500], [100, 500]], "trigger": "intrusion", "dwell_time_sec": 2.0, "cooldown_sec": 10.0},
        {"name": "exit_gate", "polygon": [[500, 100], [700, 100], [700, 300], [500, 300]], "trigger": "crossing", "direction": "left_to_right"},
    ]
    gates = pkg.events.crossing.gates_from_zone_configs(default_zones)                 # what CrossingCounter.from_zone_configs builds its handle from
    assert [(g["name"], g["direction"], g["polygon"]) for g in gates] == [("exit_gate", "left_to_right", default_zones[1]["polygon"])]
    assert gates == R.gates_from_zone_configs(default_zones)
    assert pkg.events.crossing.gates_from_zone_configs([{"name": "z", "polygon": R.SQUARE}]) == []          # the trigger defaults to "intrusion"
    # a left-to-right walk through exit_gate fires once, the opposite walk never
    for walk, want in (([(450, 200), (520, 200), (600, 210), (690, 190), (750, 200)], 1), ([(750, 200), (690, 190), (600, 210), (520, 200), (450, 200)], 0)):
        m = R.CrossingRef([], gates, max_tracks=8)
        for f, tracks in R.walk(walk):
            m.process(tracks, f)
        assert m.gate_total == [want]


def test_python_face_without_a_gpu(pkg):
    sig = inspect.signature(pkg.events.CrossingCounter.__init__)
    assert list(sig.parameters)[1:3] == ["lines", "gates"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_classes"], d["device"], d["n_streams"], d["max_tracks"], d["max_events"], d["max_gap_frames"], d["log_path"]) == (80, 0, 1, 2048, 256, 30, None)
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])
    with pytest.raises(ValueError, match="direction 'sideways'"):
        pkg.events.CrossingCounter(gates=[{"name": "g", "polygon": R.SQUARE, "direction": "sideways"}])
    with pytest.raises(ValueError, match="direction 'up'"):
        pkg.events.CrossingCounter(lines=[dict(R.LINE_V, direction="up")])
    for bad in ([640.7, 0], [float("nan"), 0], [(1 << 20) + 1, 0]):                    # refused, not truncated
        with pytest.raises(ValueError, match="coordinates must be integers"):
            pkg.events.CrossingCounter(lines=[dict(R.LINE_V, a=bad)])
    with pytest.raises(ValueError, match="gate 0: coordinates must be integers"):
        pkg.events.CrossingCounter(gates=[{"name": "g", "polygon": [[0, 0], [10.5, 0], [5, 5]], "direction": None}])
    e = pkg.events.CrossingEvent("t", "gate_crossing", "exit_gate", 0, "left_to_right", 7, 2, "car", [0.0, 1.0, 2.0, 3.0], [1, 2], [0, 2], 5, 40)
    assert '"direction": "left_to_right"' in e.to_json() and '"frames": 5' in e.to_json()
    assert inspect.signature(pkg.pipeline.run).parameters["crossing_counter"].default is None
    ffi = pkg._ffi
    assert (ffi.CrossingEventRec.track.offset, ffi.CrossingEventRec.cls.offset) == (48, 64)
    import ctypes
    assert ctypes.sizeof(ffi.CrossingEventRec) == 72 and ctypes.sizeof(ffi.LineCfg) == 20
    header = open(ffi.HEADER_PATH).read()
    for name, val in list(pkg.events.crossing.GATE_DIRECTIONS.items())[1:]:
        assert re.search(rf"#define \w+_GATE_{name.upper()} {val}\b", header)


def test_create_refuses_out_of_range_coordinates_before_touching_the_device(pkg):
    """rtmodt_crossing_create validates every argument before its first HIP call: the refusals are the same without a GPU."""
    import ctypes as C
    ffi = pkg._ffi
    L = ffi.lib()
    h = C.c_void_p()

    def create(lines=(), gates=(), n_classes=80, max_gap=30):
        lc = (ffi.LineCfg * max(len(lines), 1))(*[ffi.LineCfg(*l) for l in lines])
        keep = [np.ascontiguousarray(g[0], np.int32).reshape(-1, 2) for g in gates]
        gc = (ffi.GateCfg * max(len(gates), 1))(*[ffi.GateCfg(k.ctypes.data_as(C.POINTER(C.c_int32)), len(k), g[1]) for k, g in zip(keep, gates)])
        return L.rtmodt_crossing_create(0, lc, len(lines), gc, len(gates), n_classes, 1, 8, 8, max_gap, C.byref(h))

    lim = 1 << 20
    assert create(lines=[(0, 0, lim + 1, 0, 0)]) == ffi.E_INVALID and b"2^20" in L.rtmodt_last_error()
    assert create(lines=[(0, -lim - 1, 5, 0, 0)]) == ffi.E_INVALID
    assert create(lines=[(0, 0, 5, 0, 3)]) == ffi.E_INVALID
    assert create(gates=[([[0, 0], [lim + 1, 0], [5, 5]], 0)]) == ffi.E_INVALID
    assert create(gates=[([[0, 0], [4, 0], [5, 5]], 5)]) == ffi.E_INVALID
    assert create(lines=[(0, 0, 1, 1, 0)] * 33) == ffi.E_INVALID
    assert create(gates=[([[0, 0]] * 1025, 0)] * 2 + [([[0, 0]], 0)]) == ffi.E_INVALID       # 2051 vertices
    assert create(n_classes=0) == ffi.E_INVALID and create(n_classes=257) == ffi.E_INVALID
    assert create(max_gap=-1) == ffi.E_INVALID
    assert not h.value


class _Det:
    model = type("M", (), {"names": {0: "person"}})()

    def detect(self, frame):
        return type("D", (), {"xyxy": np.zeros((1, 4), np.float32), "confidence": np.ones(1, np.float32), "class_id": np.zeros(1, np.int32),
                              "__len__": lambda self: 1})()


class _Trk:
    def __init__(self):
        self.calls = []

    def update_from_detector(self, det, materialize=True):
        self.calls.append(materialize)
        return [("track", len(self.calls))] if materialize else []

    def update(self, detections):
        self.calls.append("host")
        return [("track", len(self.calls))]


class _Counter:
    def __init__(self):
        self.seen = []

    def process(self, tracks, fid):
        self.seen.append(list(tracks))
        return [("crossing", fid)] if tracks else []

    def process_tracker(self, tracker, fid, class_names=None):
        self.seen.append(("device", class_names))
        return [[("crossing", fid)]]


class _HostEvents:
    def process(self, tracks, fid):
        return [("event", fid)] if tracks else []


class _DeviceEvents(_HostEvents):
    def process_tracker(self, tracker, fid, class_names=None):
        return [("event", fid)], None


@pytest.mark.parametrize("events, handoff, calls, on_device", [
    (None, True, [False] * 3, True),                       # the counter alone leaves the list on the device
    (_DeviceEvents, True, [False] * 3, True),              # beside a device event engine: both read the tracker's state
    (_HostEvents, True, [True] * 3, False),                # a host-only event engine needs the list: the counter takes it too
    (None, False, ["host"] * 3, False),                    # the reference's literal data flow
])
def test_pipeline_calls_the_counter_where_the_event_engine_is_called(pkg, events, handoff, calls, on_device):
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    trk, counter = _Trk(), _Counter()
    prof = pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), trk, prof, max_frames=3, device_stages=False,
                           event_engine=events() if events else None, device_handoff=handoff, crossing_counter=counter)
    assert trk.calls == calls and out["crossings"] == 3 and out["events"] == (3 if events else 0)
    assert counter.seen == ([("device", {0: "person"})] * 3 if on_device else [[("track", k)] for k in (1, 2, 3)])
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof, max_frames=2, device_stages=False)
    assert "crossings" not in out                          # without a counter the summary is what it was
