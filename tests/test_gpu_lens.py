"""GPU: the lens corrector (``csrc/lens.hip``) against ``tests/lens_ref.py``: the table the device holds after ``set_model`` and
``set_map`` and every output byte of ``process`` are equal to the restatement (``==`` on integers, nothing is tolerated); every
memory kind, padded rows whose padding stays untouched, odd base addresses, a border colour; streams; every refusal; the hand-over
of rectified device frames to the motion detector; the pipeline's ``undistort`` stage.  Shapes here stay inside the kernel's first
256-pixel tile column (the widest output is 131 pixels): partial tiles in both axes, rows that are no multiple of any vector width,
outputs larger and smaller than the source.  ``tests/test_gpu_lens_tiles.py`` goes past one tile, one wave and to the largest extents
with the cases of ``tests/lens_cases.py``, and compares the kernel with a float64 reference that is independent of the restatement.
Content is random bytes, the worst case for a wrong weight or tap.  PARITY UNPINNED: cv2.undistort / remap are not compared."""
import ctypes as C
import os

import numpy as np
import pytest

import lens_ref as R
from lens_cases import BORDER, image, padded, random_frames, rectify

pytestmark = pytest.mark.gpu

CASES = [((23, 37), (19, 41)), ((77, 131), (48, 64)), ((1, 1), (1, 1))]      # (src, out) as (h, w): 37 x 23 -> 41 x 19, 131 x 77 -> 64 x 48, 1 x 1


def lenses_for(src, out):
    return [R.lens_for(name, src, out) for name in R.LENSES]


def set_lens(lc, stream, lens):
    return lc.set_model(stream, lens.K, lens.k, lens.new_K, lens.r2_limit)


# ---------------------------------------------------------------------------------------------------------------- table and bytes
@pytest.mark.parametrize("src,out", CASES, ids=["37x23-41x19", "131x77-64x48", "1x1"])
def test_table_and_bytes_equal_restatement(pkg, src, out):
    lenses = lenses_for(src, out)
    lc = pkg.ingestion.LensCorrector(5, src, out, border=BORDER)
    tables = []
    for s, lens in enumerate(lenses):
        want = R.build_model(lens, src, out)
        assert set_lens(lc, s, lens) == int(want[2].sum())
        tables.append(want)
    mx, my = R.hostile_map(src, out)
    tables.append(R.build_from_map(mx, my, src))
    assert lc.set_map(4, mx, my) == int(tables[4][2].sum())
    for s, want in enumerate(tables):
        got = lc.map(s)
        assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want)), s
    if src == (23, 37):                                                       # every kind of pixel occurs: borders, corners, fully outside, whole
        o, x0, y0 = tables[0][2], tables[0][0] >> 5, tables[0][1] >> 5
        assert o[0, 0] and o[0, -1] and o[-1, 0] and o[-1, -1] and not o[9, 20]
        part = (o == 0) & ((x0 < 0) | (x0 + 1 >= 37) | (y0 < 0) | (y0 + 1 >= 23))
        assert part[:, :20].any() and part[:, 21:].any() and part[:9].any() and part[10:].any()
    frames = random_frames(5, src, 100 + src[1])
    got = lc.process(frames)
    for s in range(5):
        assert got[s].shape == out + (3,) and np.array_equal(got[s], R.sample(frames[s], tables[s], BORDER)), s
    assert lc.last_ms() >= 0
    lc.close()


def test_identity_lens_copies(pkg):
    size = (48, 64)
    lc = pkg.ingestion.LensCorrector(1, size)
    assert lc.set_model(0, (64.0, 64.0, 31.5, 23.5), [0, 0, 0, 0]) == 0
    qx, qy, outside = lc.map(0)
    assert np.array_equal(qx, np.tile(32 * np.arange(64), (48, 1))) and np.array_equal(qy, np.tile(32 * np.arange(48)[:, None], (1, 64))) and not outside.any()
    frames = random_frames(1, size, 5)
    assert np.array_equal(lc.process(frames)[0], frames[0])
    lc.close()


# ---------------------------------------------------------------------------------------------------------------- memory, pitch, alignment
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dst_kind", ["host", "device"])
@pytest.mark.parametrize("src_kind", ["host", "device"])
def test_memory_kinds_pitches_and_odd_bases(pkg, src_kind, dst_kind, offset):
    for src, out, dextra in (((23, 37), (19, 41), 7), ((23, 37), (19, 41), 9), ((77, 131), (48, 64), 8)):    # dst pitch 130 (never wide), 132 and 200 (wide at offset 0)
        lenses = lenses_for(src, out)
        lc = pkg.ingestion.LensCorrector(2, src, out, border=BORDER)
        set_lens(lc, 0, lenses[0])
        set_lens(lc, 1, lenses[2])
        frames = random_frames(3, src, 7 + dextra)
        streams = [1, 0, 1]
        got = rectify(lc, pkg, frames, streams, out, src_kind=src_kind, dst_kind=dst_kind, spitch=3 * src[1] + 5, dpitch=3 * out[1] + dextra, offset=offset)
        for i, s in enumerate(streams):
            assert np.array_equal(got[i], R.sample(frames[i], R.build_model(lenses[2 * s], src, out), BORDER)), (src, dextra, i)
        lc.close()


# ---------------------------------------------------------------------------------------------------------------- streams
def test_streams_follow_their_lens_and_replacement(pkg):
    src, out = (23, 37), (19, 41)
    lenses = lenses_for(src, out)
    lc = pkg.ingestion.LensCorrector(3, src, out)
    for s in range(3):
        set_lens(lc, s, lenses[s])
    frames = random_frames(3, src, 21)
    got = lc.process(frames, [2, 0, 2])
    for i, s in enumerate([2, 0, 2]):
        assert np.array_equal(got[i], R.sample(frames[i], R.build_model(lenses[s], src, out))), i
    assert not np.array_equal(got[0], R.sample(frames[0], R.build_model(lenses[0], src, out)))
    before = [lc.map(s) for s in (0, 1)]
    set_lens(lc, 2, lenses[3])                                                # replaced between calls: the next call sees it
    got = lc.process(frames, [2, 0, 2])
    for i, s in enumerate([3, 0, 3]):
        assert np.array_equal(got[i], R.sample(frames[i], R.build_model(lenses[s], src, out))), i
    for s in (0, 1):                                                          # streams not named keep theirs
        assert all(np.array_equal(a, b) for a, b in zip(lc.map(s), before[s]))
    mx, my = R.hostile_map(src, out)
    lc.set_map(1, mx, my)                                                     # a model replaced by a map
    assert np.array_equal(lc.process(frames[:1], [1])[0], R.sample(frames[0], R.build_from_map(mx, my, src)))
    lc.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg):
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    L = F.lib()
    size = (23, 37)
    h, w = size
    lenses = lenses_for(size, size)
    for kw, word in ((dict(streams=0, src_size=size), "streams"), (dict(streams=1025, src_size=size), "streams"), (dict(streams=1, src_size=(0, 4)), "outside 1..16384"),
                     (dict(streams=1, src_size=(4, 16385)), "outside 1..16384"), (dict(streams=1, src_size=size, out_size=(16385, 4)), "outside 1..16384"),
                     (dict(streams=1, src_size=size, out_size=(4, 0)), "outside 1..16384")):
        with pytest.raises(E) as e:
            pkg.ingestion.LensCorrector(**kw)
        assert e.value.code == F.E_INVALID and word in e.value.msg, e.value
    lc = pkg.ingestion.LensCorrector(3, size, border=BORDER)
    with pytest.raises(E) as e:
        lc.last_ms()
    assert e.value.code == F.E_INVALID and "no process call" in e.value.msg
    set_lens(lc, 0, lenses[0])
    set_lens(lc, 1, lenses[1])
    frames = random_frames(2, size, 33)
    want = [R.sample(frames[s], R.build_model(lenses[s], size), BORDER) for s in range(2)]

    def refused(code, fragment, call):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == code and fragment in e.value.msg, e.value
        got = lc.process(frames)                                               # the handle still processes a valid call correctly
        assert all(np.array_equal(g, x) for g, x in zip(got, want)), fragment

    refused(F.E_INVALID, "has no lens", lambda: lc.process(frames[:1], [2]))
    refused(F.E_INVALID, "has no lens", lambda: lc.map(2))
    refused(F.E_INVALID, "has no lens", lambda: lc.process(frames + frames[:1]))                          # stream i, and stream 2 has none
    refused(F.E_INVALID, "outside 0..2", lambda: lc.process(frames, [0, 3]))
    refused(F.E_INVALID, "outside 0..2", lambda: lc.process(frames, [-1, 0]))
    refused(F.E_INVALID, "outside 0..2", lambda: set_lens(lc, 3, lenses[0]))
    refused(F.E_INVALID, "outside 0..2", lambda: lc.set_map(-1, np.zeros(size, np.float32), np.zeros(size, np.float32)))
    refused(F.E_INVALID, "outside 0..2", lambda: lc.map(3))
    refused(F.E_INVALID, "created for", lambda: lc.process([f[:, :36] for f in frames]))                   # a geometry other than the handle's
    refused(F.E_INVALID, "created for", lambda: lc.process([f[:22] for f in frames]))
    refused(F.E_INVALID, "created for", lambda: lc.process(frames, out=[np.zeros((h, w + 1, 3), np.uint8) for _ in frames]))
    dev, dev2 = F.DeviceBuffer(4 * h * 3 * w), F.DeviceBuffer(4 * h * 3 * w)
    dev.upload(image(frames, 3 * w, 0)[:2 * h * 3 * w])
    refused(F.E_INVALID, "pitch", lambda: lc.process(dev, [0, 1], dev2, stride=3 * w - 1))
    refused(F.E_INVALID, "pitch", lambda: lc.process(dev, [0, 1], dev2, out_stride=3 * w - 1))
    raw = lambda *a: F.check(L.rtmodt_lens_process(lc._h, *a))
    bufs = [padded(f, 3 * w + 5, 1) for f in frames]
    outs = [padded(np.zeros_like(f), 3 * w + 7, 2) for f in frames]
    sp, dp = (C.c_void_p * 2)(*[v.ctypes.data for _, v in bufs]), (C.c_void_p * 2)(*[v.ctypes.data for _, v in outs])
    hole = (C.c_void_p * 2)(bufs[0][1].ctypes.data, None)
    refused(F.E_INVALID, "null argument", lambda: raw(None, 3 * w + 5, F.MEM_HOST, dp, 3 * w + 7, F.MEM_HOST, None, 2))
    refused(F.E_INVALID, "null argument", lambda: raw(sp, 3 * w + 5, F.MEM_HOST, None, 3 * w + 7, F.MEM_HOST, None, 2))
    refused(F.E_INVALID, "frame 1 is null", lambda: raw(hole, 3 * w + 5, F.MEM_HOST, dp, 3 * w + 7, F.MEM_HOST, None, 2))
    refused(F.E_INVALID, "frame 1 is null", lambda: raw(sp, 3 * w + 5, F.MEM_HOST, hole, 3 * w + 7, F.MEM_HOST, None, 2))
    refused(F.E_INVALID, "mem_kind", lambda: raw(sp, 3 * w + 5, 2, dp, 3 * w + 7, F.MEM_HOST, None, 2))
    refused(F.E_INVALID, "mem_kind", lambda: raw(sp, 3 * w + 5, F.MEM_HOST, dp, 3 * w + 7, 2, None, 2))
    refused(F.E_INVALID, "pitch", lambda: raw(sp, 3 * w - 1, F.MEM_HOST, dp, 3 * w + 7, F.MEM_HOST, None, 2))
    # a gather cannot work in place: the same frames, a destination that begins on a source's last byte, a source that begins in the destination
    refused(F.E_INVALID, "overlaps", lambda: lc.process(dev, [0, 1], dev))
    refused(F.E_INVALID, "overlaps", lambda: lc.process(dev, [0, 1], dev, out_offset=2 * h * 3 * w - 1))
    refused(F.E_INVALID, "overlaps", lambda: lc.process(dev, [0], dev, offset=h * 3 * w - 3))
    refused(F.E_INVALID, "overlaps", lambda: lc.process([v for _, v in bufs], out=[v for _, v in bufs]))
    got = lc.process(dev, [0, 1], dev, out_offset=2 * h * 3 * w)                                           # directly behind the sources: allowed
    assert np.array_equal(got.download(2 * h * 3 * w, 2 * h * 3 * w), np.concatenate([x.ravel() for x in want]))
    for K in ((0.0, 30, 1, 1), (30, float("nan"), 1, 1), (30, float("inf"), 1, 1), (-1.0, 30, 1, 1)):
        refused(F.E_INVALID, "focal", lambda: lc.set_model(1, K, [0, 0, 0, 0]))                            # ... and stream 1 keeps the lens it had
    refused(F.E_INVALID, "focal", lambda: lc.set_model(1, (30, 30, 1, 1), [0, 0, 0, 0], new_K=(30, 0.0, 1, 1)))
    with pytest.raises(ValueError):
        lc.set_map(0, np.zeros((h, w + 1), np.float32), np.zeros((h, w + 1), np.float32))
    assert lc.process([], []) == []                                                                        # n = 0 is a no-op
    raw(None, 0, 7, None, 0, 7, None, 0)
    assert all(np.array_equal(g, x) for g, x in zip(lc.process(frames), want))
    lc.close()


# ---------------------------------------------------------------------------------------------------------------- hand-over
def test_rectified_device_frames_feed_the_motion_detector(pkg):
    F = pkg._ffi
    src, out = (77, 131), (48, 64)
    oh, ow = out
    lc = pkg.ingestion.LensCorrector(2, src, out)
    for s in range(2):
        set_lens(lc, s, lenses_for(src, out)[s])
    on_dev, on_host = pkg.MotionDetector(2, oh, ow, warmup=1, scale=2), pkg.MotionDetector(2, oh, ow, warmup=1, scale=2)
    buf = F.DeviceBuffer(2 * oh * 3 * ow)
    for k in range(3):
        frames = random_frames(2, src, 50 + k)
        assert lc.process(frames, out=buf) is buf
        host = [np.ascontiguousarray(f) for f in buf.download().reshape(2, oh, ow, 3)]
        a, b = on_dev.process(buf), on_host.process(host)
        assert a == b and all(np.array_equal(on_dev.mask(s), on_host.mask(s)) for s in range(2)), k
        assert all(np.array_equal(x, y) for s in range(2) for x, y in zip(on_dev.state(s)[:2], on_host.state(s)[:2]))
    assert any(r.n_raw for r in a)
    lc.close(); on_dev.close(); on_host.close()


# ---------------------------------------------------------------------------------------------------------------- pipeline
class _Counting:
    """The detector with the frames of its detect() calls kept; everything else is the detector's."""

    def __init__(self, det):
        self._det, self.calls = det, []

    def detect(self, frame):
        self.calls.append(frame.copy())
        return self._det.detect(frame)

    def __getattr__(self, name):
        return getattr(self._det, name)


class _Recorder:
    def __init__(self):
        self.frames = []

    def write(self, frame):
        self.frames.append(frame.copy())


def test_pipeline_undistort_stage(pkg, tmp_path):
    path = os.path.join(str(tmp_path), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    detector = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    size = (77, 131)
    lens = R.lens_for("barrel", size, size, zoom=0.8)
    table = R.build_model(lens, size)
    frames = random_frames(6, size, 77)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    tracker = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    base_p = prof()
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), base_p, max_frames=6)
    lc = pkg.ingestion.LensCorrector(1, size)
    set_lens(lc, 0, lens)
    det, rec, p = _Counting(detector), _Recorder(), prof()
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), det, tracker(), p, max_frames=6, lens=lc, recorder=rec,
                           motion=pkg.MotionDetector(1, size[0], size[1]))
    want = [R.sample(f, table) for f in frames]
    assert len(det.calls) == 6 and all(np.array_equal(c, x) for c, x in zip(det.calls, want))            # the detector's input is the rectified frame
    assert len(rec.frames) == 6 and all(np.array_equal(c, x) for c, x in zip(rec.frames, want))
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"undistort_mean_ms", "motion_mean_ms"} and rows(base) <= rows(out)
    order = list(p.STAGE_ORDER)
    assert order.index("undistort") == order.index("decode") + 1 and order.index("motion") == order.index("undistort") + 1
    assert order.index("undistort") < order.index("preprocess")
    # lens=None: the parent's stage table and summary keys
    p = prof()
    none = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=6, lens=None)
    assert set(none) == set(base) and "undistort_mean_ms" not in none
    assert list(p.STAGE_ORDER) == list(base_p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking",
                                                                                                           "events", "visualization", "total"]
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"]
    lc.close()
    detector.close()
