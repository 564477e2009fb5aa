"""GPU: the frame renderer (csrc/render.hip) bit for bit against the NumPy restatement of its paint rules (tests/render_ref.py),
through FrameRenderer and the C ABI: frame sizes and row strides, host and device frames, batches, every show_* flag, zones,
trails, capacity errors and the pipeline's visualization stage."""
from types import SimpleNamespace

import numpy as np
import pytest

import render_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["person", "car", "", "bicycle", "très_long_nom", "dog"]


def make_tracks(rng, n, h, w, trail=30):
    out = []
    for i in range(n):
        x1 = rng.uniform(-60, w + 20)
        y1 = rng.uniform(-30, h + 20)
        bw, bh = rng.uniform(0, 250), rng.uniform(0, 250)
        tid = int(rng.integers(0, 5000))
        cx, cy = int(x1 + bw / 2), int(y1 + bh / 2)
        k = int(rng.integers(0, trail + 1)) if trail else 0
        pts = [(cx + int(rng.integers(-40, 41)), cy + int(rng.integers(-40, 41))) for _ in range(k)]
        out.append(SimpleNamespace(track_id=tid, xyxy=np.array([x1, y1, x1 + bw, y1 + bh], np.float32),
                                   confidence=np.float32(rng.uniform(0, 1)), class_name=NAMES[i % len(NAMES)], trail=pts))
    return out


ZONES = [("entrance", np.array([[100, 100], [400, 120], [380, 360], [120, 300]], np.int32)),
         ("loading bay", np.array([[300, 200], [600, 180], [610, 500], [320, 520], [450, 350]], np.int32))]     # concave, overlapping


def strided(h, w, stride, rng):
    """An h x w x 3 view over a padded buffer (rows `stride` bytes apart) filled with random bytes; returns (buffer, view)."""
    buf = rng.integers(0, 256, h * stride, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (stride, 3, 1), writeable=True)
    return buf, view


def check(pkg, frame, tracks, zones=None, fps=31.25, lat=12.5, **flags):
    want = R.render(frame, tracks, zones, fps, lat, **flags)
    r = pkg.FrameRenderer(**flags)
    got = r.render(frame, tracks, zones=zones, fps=fps, latency_ms=lat)
    assert got is frame
    bad = np.argwhere(np.any(frame != want, axis=2))
    assert len(bad) == 0, f"{len(bad)} pixels differ, first {bad[:5].tolist()}"
    return r


@pytest.mark.parametrize("h,w,stride", [(640, 640, 1920), (1080, 1920, 5760), (37, 53, 3 * 53 + 7), (64, 100, 304)])
@pytest.mark.parametrize("n", [0, 1, 300])
def test_random_scenes_bit_exact(pkg, h, w, stride, n):
    rng = np.random.default_rng(h * 7 + w + n)
    buf, frame = strided(h, w, stride, rng)
    before = buf.copy()
    tracks = make_tracks(rng, n, h, w)
    check(pkg, frame, tracks, ZONES)
    rows = np.arange(h * stride).reshape(h, stride)[:, 3 * w:].reshape(-1)
    assert np.array_equal(buf[rows], before[rows]), "bytes past the frame rows were written"


def test_edges_labels_above_top_and_tiny_boxes(pkg):
    rng = np.random.default_rng(5)
    _, frame = strided(90, 130, 3 * 130 + 2, rng)
    T = lambda i, b, tr=(): SimpleNamespace(track_id=i, xyxy=np.array(b, np.float32), confidence=np.float32(0.5), class_name="x", trail=list(tr))
    tracks = [T(1, [0, 0, 129, 89]), T(2, [-5.5, 3.9, 40.2, 60.0]), T(3, [100, 80, 200, 200]), T(4, [60, 2, 60, 2]),
              T(5, [50.9, 10.1, 49.1, 10.9]), T(6, [-1e9, -1e9, 1e9, 1e9]), T(7, [20, 40, 80, 45], [(0, 0), (200, 300)]),
              T(-3, [10, 70, 20, 88], [(129, 89), (129, 89)])]
    check(pkg, frame, tracks, None)


@pytest.mark.parametrize("trail_len,trail_length", [(1, 30), (2, 30), (30, 30), (30, 1), (30, 2), (12, 5)])
def test_trails(pkg, trail_len, trail_length):
    rng = np.random.default_rng(trail_len * 31 + trail_length)
    _, frame = strided(200, 260, 780, rng)
    tracks = make_tracks(rng, 20, 200, 260, trail=0)
    for t in tracks:
        t.trail = [(int(rng.integers(-20, 280)), int(rng.integers(-20, 220))) for _ in range(trail_len)]
    check(pkg, frame, tracks, None, trail_length=trail_length)


@pytest.mark.parametrize("case", ["none", "overlap_concave", "degenerate", "names"])
def test_zones(pkg, case):
    rng = np.random.default_rng(11)
    _, frame = strided(540, 700, 2100, rng)
    zones = {"none": [],
             "overlap_concave": ZONES,
             "degenerate": [("line", np.array([[10, 10], [200, 200], [400, 400]], np.int32)), ("dot", np.array([[50, 60]], np.int32)),
                            ("empty", np.zeros((0, 2), np.int32)), ("flat", np.array([[20, 300], [600, 300], [600, 300]], np.int32))],
             "names": [("", ZONES[0][1]), ("zöne ✓", ZONES[1][1]), ("edge", np.array([[0, 0], [40, 0], [40, 30]], np.int32)),
                       ("off", np.array([[-100, -100], [-10, -100], [-10, -20]], np.int32))]}[case]
    tracks = make_tracks(rng, 25, 540, 700)
    check(pkg, frame, tracks, zones)


FLAGS = ["show_boxes", "show_ids", "show_trails", "show_zones", "show_fps"]


@pytest.mark.parametrize("off", FLAGS)
def test_each_flag_off(pkg, off):
    rng = np.random.default_rng(FLAGS.index(off))
    _, frame = strided(360, 480, 1440, rng)
    tracks = make_tracks(rng, 40, 360, 480)
    check(pkg, frame, tracks, ZONES, **{off: False})


def test_flag_changed_after_construction(pkg):
    rng = np.random.default_rng(3)
    _, frame = strided(120, 160, 480, rng)
    tracks = make_tracks(rng, 6, 120, 160)
    r = pkg.FrameRenderer()
    r.show_boxes = False
    want = R.render(frame, tracks, ZONES, 1.0, 2.0, show_boxes=False)
    r.render(frame, tracks, zones=ZONES, fps=1.0, latency_ms=2.0)
    assert np.array_equal(frame, want)


def test_batch_equals_single_calls_and_device_equals_host(pkg):
    rng = np.random.default_rng(8)
    h, w = 300, 420
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(8)]
    lists = [make_tracks(rng, int(rng.integers(0, 60)), h, w) for _ in range(8)]
    r = pkg.FrameRenderer()
    singles = [f.copy() for f in frames]
    for f, t in zip(singles, lists):
        r.render(f, t, zones=ZONES, fps=60.0, latency_ms=4.0)
    batch = [f.copy() for f in frames]
    assert r.render_batch(batch, lists, zones=ZONES, fps=60.0, latency_ms=4.0) is batch
    for i in range(8):
        assert np.array_equal(batch[i], singles[i]), i
        assert np.array_equal(batch[i], R.render(frames[i], lists[i], ZONES, 60.0, 4.0)), i
    # device-resident frames, drawn in place
    dev = pkg._ffi.DeviceBuffer(8 * h * w * 3)
    dev.upload(np.stack(frames))
    assert r.render_batch(dev, lists, zones=ZONES, fps=60.0, latency_ms=4.0, height=h, width=w) is dev
    got = dev.download().reshape(8, h, w, 3)
    for i in range(8):
        assert np.array_equal(got[i], batch[i]), i
    assert r.last_kernel_ms() > 0
    dev.free()


def test_device_frames_with_row_padding(pkg):
    rng = np.random.default_rng(9)
    h, w, stride = 37, 53, 3 * 53 + 7
    host = rng.integers(0, 256, (3, h * stride), dtype=np.uint8)
    lists = [make_tracks(rng, 12, h, w) for _ in range(3)]
    dev = pkg._ffi.DeviceBuffer(host.nbytes + 64)
    dev.upload(host, offset=32)
    guard_lo, guard_hi = dev.download(32, 0), dev.download(32, 32 + host.nbytes)
    pkg.FrameRenderer().render_batch(dev, lists, zones=ZONES, height=h, width=w, stride=stride, offset=32)
    got = dev.download(host.nbytes, 32).reshape(3, h * stride)
    for i in range(3):
        view = np.lib.stride_tricks.as_strided(host[i], (h, w, 3), (stride, 3, 1))
        want = R.render(view, lists[i], ZONES, 0.0, 0.0)
        gv = np.lib.stride_tricks.as_strided(got[i], (h, w, 3), (stride, 3, 1))
        assert np.array_equal(gv, want)
        pad = np.arange(h * stride).reshape(h, stride)[:, 3 * w:].reshape(-1)
        assert np.array_equal(got[i][pad], host[i][pad])
    assert np.array_equal(dev.download(32, 0), guard_lo) and np.array_equal(dev.download(32, 32 + host.nbytes), guard_hi)
    dev.free()


def test_capacity_errors(pkg):
    E = pkg._ffi
    r = pkg.FrameRenderer()
    frame = np.zeros((50, 60, 3), np.uint8)
    tri = np.array([[0, 0], [10, 0], [0, 10]], np.int32)
    with pytest.raises(E.RtmodtError) as e:
        r.render(frame, [], zones=[(f"z{i}", tri) for i in range(33)])
    assert e.value.code == E.E_CAPACITY and "33" in e.value.msg
    with pytest.raises(E.RtmodtError) as e:
        r.render(frame, [], zones=[("big", np.zeros((2049, 2), np.int32))])
    assert e.value.code == E.E_CAPACITY and "2049" in e.value.msg
    t = SimpleNamespace(track_id=1, xyxy=np.zeros(4, np.float32), confidence=1.0, class_name="n" * 260, trail=[])
    with pytest.raises(E.RtmodtError) as e:
        r.render(frame, [t])
    assert e.value.code == E.E_CAPACITY
    assert not frame.any(), "a failed call drew something"
    check(pkg, frame, [SimpleNamespace(track_id=1, xyxy=np.array([5, 20, 30, 40], np.float32), confidence=1.0, class_name="ok", trail=[])],
          [(f"z{i}", tri + i) for i in range(32)])


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
        return [SimpleNamespace(track_id=4, xyxy=np.array([2, 12, 30, 40], np.float32), confidence=0.9, class_name="person",
                                trail=[(5, 5), (16, 26)])] if materialize else []


class _Events:
    def process(self, tracks, fid):
        return []

    def process_tracker(self, tracker, fid, class_names=None):
        return [[]]

    def get_zone_polygons(self):
        return ZONES[:1]


def test_pipeline_visualization_stage(pkg):
    class Src(pkg.pipeline.SyntheticSource):
        def read(self):
            ok, f, i = super().read()
            self.last = f
            return ok, f, i

    frames = np.full((2, 48, 64, 3), 77, np.uint8)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    trk = _Trk()
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), trk, prof(), max_frames=3, device_stages=False,
                           event_engine=_Events())
    assert "visualization_mean_ms" not in out and trk.calls == [False] * 3
    trk = _Trk()
    src = Src(frames)
    out = pkg.pipeline.run(src, _Det(), trk, prof(), max_frames=3, device_stages=False, event_engine=_Events(),
                           renderer=pkg.FrameRenderer(show_fps=False))
    assert "visualization_mean_ms" in out and trk.calls == [True] * 3
    want = R.render(frames[0], trk.update_from_detector(None), ZONES[:1], show_fps=False)
    assert np.array_equal(src.last, want)
