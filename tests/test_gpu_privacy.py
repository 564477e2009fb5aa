"""GPU: the privacy masker (csrc/privacy.hip) byte for byte against the NumPy restatement of its rules (tests/privacy_ref.py),
through PrivacyMask and the C ABI: every edge path of the three modes over small geometries (host frames, and device frames with
their own row pitch, padding bytes included), box lists, the in-place hazard rule of BLUR, capacity and refusals, the
device-state forms of the four trackers and of the detector, and the pipeline's privacy stage.  Every comparison is == on bytes."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import privacy_ref as PR
import render_ref as RR

pytestmark = pytest.mark.gpu

GEOMS = [(1, 1, 3), (5, 3, 9), (16, 64, 192), (37, 70, 211), (33, 131, 396), (128, 192, 576)]
MODES = [dict(mode="fill", color=(7, 200, 31))] + [dict(mode="pixelate", cell=c) for c in (2, 3, 16, 64)] + \
        [dict(mode="blur", radius=r, passes=p) for r, p in ((1, 1), (5, 2), (16, 3))]
CONCAVE = np.array([[3, 2], [40, 4], [22, 15], [44, 33], [5, 30], [14, 16]], np.int32)


def mode_id(m):
    return "-".join(str(v) for k, v in m.items() if k != "color")


@functools.lru_cache(maxsize=None)
def scene(h, w, stride, seed=0):
    """(buffer of h * stride random bytes, boxes, classes): boxes inside, straddling every edge and outside, some inverted."""
    rng = np.random.default_rng(1000 * h + w + seed)
    buf = rng.integers(0, 256, h * stride, dtype=np.uint8)
    k = 7
    x0 = rng.uniform(-0.4 * w - 2, w + 1, k); y0 = rng.uniform(-0.4 * h - 2, h + 1, k)
    bw = rng.uniform(0, 0.7 * w + 2, k); bh = rng.uniform(0, 0.7 * h + 2, k)
    boxes = np.stack([x0, y0, x0 + bw, y0 + bh], 1).astype(np.float32)
    boxes[5] = boxes[5][[2, 1, 0, 3]] - np.float32([0, 0, 1, 0])        # inverted in x
    buf.setflags(write=False)
    boxes.setflags(write=False)
    return buf, boxes, (np.arange(k) % 3).astype(np.int32)


def view(buf, h, w, stride):
    return np.lib.stride_tricks.as_strided(buf, (h, w, 3), (stride, 3, 1), writeable=buf.flags.writeable)


@functools.lru_cache(maxsize=None)
def expected(h, w, stride, key, seed=0):
    """The whole buffer after masking (padding bytes as they were), computed once per case."""
    buf, boxes, cls = scene(h, w, stride, seed)
    out = buf.copy()
    view(out, h, w, stride)[:] = PR.apply(view(buf, h, w, stride), boxes, cls, **dict(key))
    out.setflags(write=False)
    return out


def ref_kw(m):
    return tuple(sorted(m.items()))


def on_device(pkg, mask, buf, h, w, stride, boxes, cls, out_of_place=False):
    """Masks a device copy of ``buf``; returns (the frame's buffer afterwards, the destination's or None)."""
    src = pkg._ffi.DeviceBuffer(len(buf)); src.upload(buf)
    dst = None
    if out_of_place:
        dst = pkg._ffi.DeviceBuffer(len(buf)); dst.upload(np.full(len(buf), 0xA5, np.uint8))
    mask.apply_batch(src, [(boxes, cls)], out=dst, height=h, width=w, stride=stride)
    got = src.download(), (None if dst is None else dst.download())
    src.free()
    if dst is not None:
        dst.free()
    return got


def diff(got, want):
    bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
    return f"{len(bad)} bytes differ, first at {bad[:6].tolist()}" if len(bad) else None


@pytest.mark.parametrize("m", MODES, ids=mode_id)
@pytest.mark.parametrize("h,w,stride", GEOMS)
def test_modes_over_geometries(pkg, h, w, stride, m):
    buf, boxes, cls = scene(h, w, stride)
    want = expected(h, w, stride, ref_kw(m))
    assert diff(want, buf) is not None or (h, w) == (1, 1)                   # the scene masks something
    mask = pkg.visualization.PrivacyMask(**m)
    got, _ = on_device(pkg, mask, buf, h, w, stride, boxes, cls)             # device frames: the kernel sees the odd pitch
    assert diff(got, want) is None, diff(got, want)
    host = buf.copy()
    fr = view(host, h, w, stride)
    assert mask.apply(fr, (boxes, cls)) is fr                                # host frames: staged, masked, copied back
    assert diff(host, want) is None, diff(host, want)
    assert mask.last_kernel_ms() >= 0
    mask.close()


def _straddle(h, w):
    return {"left": [-5.5, 10, 4.2, 20], "right": [w - 3.5, 5, w + 9, 15.9], "top": [20, -7, 31, 2.5], "bottom": [30, h - 2.2, 45, h + 30]}


BOX_LISTS = ["empty", "cover", "outside", "left", "right", "top", "bottom", "inverted", "random300", "class_filter", "head_expand", "polygon"]


@pytest.mark.parametrize("m", [MODES[0], MODES[2], MODES[6]], ids=mode_id)
@pytest.mark.parametrize("name", BOX_LISTS)
def test_box_lists(pkg, name, m):
    h, w, stride = 37, 70, 211
    buf = scene(h, w, stride)[0]
    rng = np.random.default_rng(len(name))
    kw, ref = dict(m), dict(m)
    cls = None
    if name == "empty":
        boxes = np.zeros((0, 4), np.float32)
    elif name == "cover":
        boxes = np.float32([[-3, -3, w + 5, h + 5]])
    elif name == "outside":
        boxes = np.float32([[w, 0, w + 20, h], [-30, -30, -1, -1], [0, h, w, h + 8]])
    elif name in ("left", "right", "top", "bottom"):
        boxes = np.float32([_straddle(h, w)[name]])
    elif name == "inverted":
        boxes = np.float32([[30, 5, 10, 20], [10, 25, 30, 8], [40.9, 3, 40.1, 9]])      # the last truncates to one column, 40..40
    elif name == "random300":
        x0 = rng.uniform(-10, w, 300); y0 = rng.uniform(-10, h, 300)
        boxes = np.stack([x0, y0, x0 + rng.uniform(0, 12, 300), y0 + rng.uniform(0, 9, 300)], 1).astype(np.float32)
    elif name == "class_filter":
        boxes = np.float32([[2, 2, 20, 12], [25, 5, 50, 30], [40, 20, 69, 36], [0, 30, 9, 36]])
        cls = np.int32([0, 3, 5, 7])
        kw["classes"] = ref["classes"] = (3, 7)
    elif name == "head_expand":
        boxes = np.float32([[10, 8, 25, 30], [50, 1, 64, 36], [30, 34, 40, 60]])
        kw.update(region="head", head_fraction=0.3, expand_px=2)
        ref.update(kind=PR.HEAD, head_pm=300, expand_px=2)
    else:
        boxes = np.float32([[50, 3, 66, 14], [46, 25, 80, 33]])
        kw["polygons"] = ref["polygons"] = [CONCAVE, CONCAVE + np.int32([30, 18])]       # the second runs off the frame
    want = buf.copy()
    view(want, h, w, stride)[:] = PR.apply(view(buf, h, w, stride), boxes, cls, **ref)
    if name in ("empty", "outside"):
        assert diff(want, buf) is None
    else:
        assert diff(want, buf) is not None
    if name == "inverted":
        assert PR.regions(boxes, None, h, w).tolist() == [[40, 3, 40, 9]]
    mask = pkg.visualization.PrivacyMask(**kw)
    got, _ = on_device(pkg, mask, buf, h, w, stride, boxes, cls)
    assert diff(got, want) is None, diff(got, want)
    mask.close()


def test_blur_in_place_obeys_the_hazard_rule(pkg):
    """128 x 192, BLUR (16, 3), the mask covering the whole frame: every tile's halo reaches into tiles other workgroups write.
    In place equals the restatement computed from the original, equals the out-of-place result, whose src is unchanged."""
    h, w, stride = 128, 192, 576
    buf = scene(h, w, stride)[0]
    boxes = np.float32([[0, 0, w, h]])
    want = PR.blur_image(view(buf, h, w, stride), 16, 3).reshape(-1)
    mask = pkg.visualization.PrivacyMask(mode="blur", radius=16, passes=3)
    inplace, _ = on_device(pkg, mask, buf, h, w, stride, boxes, None)
    assert diff(inplace, want) is None, diff(inplace, want)
    src, dst = on_device(pkg, mask, buf, h, w, stride, boxes, None, out_of_place=True)
    assert diff(src, buf) is None and diff(dst, want) is None, (diff(src, buf), diff(dst, want))
    # host frames with out=: the clean frames stay clean
    clean = buf.copy(); out = np.full_like(buf, 0x5A)
    res = mask.apply_batch([view(clean, h, w, stride)], [boxes], out=[view(out, h, w, stride)])
    assert len(res) == 1 and diff(clean, buf) is None and diff(out, want) is None
    mask.close()


def test_out_of_place_leaves_padding_and_source(pkg):
    """dst receives the whole masked frame -- unmasked pixels copied from src -- and its bytes past 3w stay as they were."""
    h, w, stride = 37, 70, 211
    buf, boxes, cls = scene(h, w, stride)
    pad = np.ones(h * stride, bool)
    pad.reshape(h, stride)[:, :3 * w] = False
    for m in (MODES[0], MODES[3], MODES[6]):
        want = expected(h, w, stride, ref_kw(m))
        mask = pkg.visualization.PrivacyMask(**m)
        src, dst = on_device(pkg, mask, buf, h, w, stride, boxes, cls, out_of_place=True)
        assert diff(src, buf) is None, m
        assert diff(dst[~pad], want[~pad]) is None and (dst[pad] == 0xA5).all(), m
        mask.close()


def test_capacity_and_refusals(pkg):
    h, w, stride = 37, 70, 211
    buf = scene(h, w, stride)[0]
    rng = np.random.default_rng(65536)
    n = 65537
    x0 = rng.integers(0, w, n); y0 = rng.integers(0, h, n)
    boxes = np.stack([x0, y0, x0 + (rng.random(n) < 0.002) * rng.integers(0, 3, n), y0 + (rng.random(n) < 0.002)], 1).astype(np.float32)
    boxes[:40000, :] = np.float32([68, 35, 69, 36])                            # most chunks of 256 meet only the last tile
    mask = pkg.visualization.PrivacyMask(mode="pixelate", cell=3)
    want = buf.copy()
    view(want, h, w, stride)[:] = PR.apply(view(buf, h, w, stride), boxes[:65536], None, mode="pixelate", cell=3)
    assert diff(want, buf) is not None and len(PR.regions(boxes[:65536], None, h, w)) == 65536
    got, _ = on_device(pkg, mask, buf, h, w, stride, boxes[:65536], None)       # culled through LDS in 256 chunks of 256
    assert diff(got, want) is None, diff(got, want)

    def refused(code, bx, out_shift=None):
        src = pkg._ffi.DeviceBuffer(len(buf) + 64); src.upload(buf)
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            if out_shift is None:
                mask.apply_batch(src, [bx], height=h, width=w, stride=stride)
            else:
                mask.apply_batch(src, [bx], out=src, out_offset=out_shift, height=h, width=w, stride=stride)
        assert e.value.code == code
        assert diff(src.download(len(buf)), buf) is None, "a refused call touched the frame"
        src.free()

    refused(pkg._ffi.E_CAPACITY, boxes)                                         # 65537 regions
    refused(pkg._ffi.E_INVALID, np.float32([[1, 1, 5, 5], [2, np.nan, 9, 9]]))
    refused(pkg._ffi.E_INVALID, np.float32([[1, 1, np.inf, 5]]))
    refused(pkg._ffi.E_INVALID, np.float32([[1, 1, 5, 5]]), out_shift=3)         # dst overlaps src without being it
    small = pkg.visualization.PrivacyMask(mode="fill", max_regions=4)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        small.apply(view(buf.copy(), h, w, stride), np.float32([[1, 1, 2, 2]] * 5))
    assert e.value.code == pkg._ffi.E_CAPACITY
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        pkg.visualization.PrivacyMask(polygons=[CONCAVE] * 33)
    assert e.value.code == pkg._ffi.E_CAPACITY
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        pkg.visualization.PrivacyMask(polygons=[np.zeros((2049, 2), np.int32)])
    assert e.value.code == pkg._ffi.E_CAPACITY
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        pkg.visualization.PrivacyMask().last_kernel_ms()                       # nothing has launched yet
    assert e.value.code == pkg._ffi.E_INVALID
    mask.close(); small.close()


# ---- device-state forms ----------------------------------------------------------------------------------------------
S, N, FH, FW = 2, 16, 37, 70


def scripted(f, s):
    """Frame f of stream s: 8 steady boxes, one present in frames 0 and 1 only (lost at the end), one in frame 2 only (new)."""
    bx = [[2 + 14 * i + f, 2 + 18 * j + s, 11 + 14 * i + f, 14 + 18 * j + s] for j in range(2) for i in range(4)]
    if f < 2:
        bx.append([57, 2 + s, 67, 13 + s])
    if f == 2:
        bx.append([58.5, 21, 75, 33.5 + s])
    xy = np.float32(bx)
    return xy, np.full(len(xy), 0.9, np.float32), (np.arange(len(xy)) % 3).astype(np.int32)


def run_scripted(core, with_frames):
    frames = [np.random.default_rng(s).integers(0, 256, (FH, FW, 3), dtype=np.uint8) for s in range(S)]
    for f in range(3):
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32); cnt = np.zeros(S, np.int32)
        for s in range(S):
            xy, cf, cl = scripted(f, s)
            xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf, cl, len(cf)
        if with_frames:
            core.update_batch(xyxy, conf, cls, cnt, frames=frames)
        else:
            core.update_batch(xyxy, conf, cls, cnt)
    return frames


def _trackers(pkg):
    T = pkg.tracking
    return {
        "bytetrack": (lambda: T.tracker._ByteTrackCore(n_streams=S, max_tracks=32, max_dets=N), False,
                      lambda core, st: np.nonzero(st["tsu"] == 1)[0]),
        "deepsort": (lambda: T.deepsort._DeepSortCore(n_init=2, max_age=5, nn_budget=4, n_streams=S, max_tracks=32, max_dets=N), True,
                     lambda core, st: np.nonzero((st["state"] == 2) & (st["tsu"] == 0))[0]),
        "ocsort": (lambda: T.ocsort._OcSortCore(min_hits=2, n_streams=S, max_tracks=32, max_dets=N), False,
                   lambda core, st: core.returned(st)),
        "botsort": (lambda: T.botsort._BotSortCore(n_streams=S, max_tracks=32, max_dets=N), False,
                    lambda core, st: np.nonzero((st["flag"] == 2) & (st["tsu"] == 0))[0]),
    }


@pytest.mark.parametrize("m", [MODES[3], MODES[6]], ids=mode_id)
@pytest.mark.parametrize("which", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_apply_tracker_equals_apply_on_the_passed_tracks(pkg, which, m):
    make, with_frames, passed = _trackers(pkg)[which]
    core = make()
    frames = run_scripted(core, with_frames)
    mask = pkg.visualization.PrivacyMask(classes=(0, 1), expand_px=1, **m)
    want, n_state, n_pass = [], 0, 0
    for s in range(S):
        st = core.snapshot(s)
        idx = passed(core, st)
        n_state += len(st["ids"]); n_pass += len(idx)
        want.append(mask.apply(frames[s].copy(), (st["xyxy"][idx], st["cls"][idx])))
        assert np.array_equal(want[s], PR.apply(frames[s], st["xyxy"][idx], st["cls"][idx], classes=(0, 1), expand_px=1, **m))
        assert not np.array_equal(want[s], frames[s])
    assert 0 < n_pass < n_state, (n_pass, n_state)                              # a track of the state is not reported
    got = [f.copy() for f in frames]
    tracker = SimpleNamespace(_core=core, report="matched") if which == "bytetrack" else core
    assert mask.apply_tracker(tracker, got) is got
    for s in range(S):
        assert diff(got[s], want[s]) is None, (s, diff(got[s], want[s]))
    # device frames, one buffer holding both streams' frames with a padded pitch
    stride = 3 * FW + 5
    host = np.zeros((S, FH, stride), np.uint8)
    for s in range(S):
        host[s, :, :3 * FW] = frames[s].reshape(FH, 3 * FW)
    dev = pkg._ffi.DeviceBuffer(host.size); dev.upload(host)
    mask.apply_tracker(tracker, dev, height=FH, width=FW, stride=stride)
    back = dev.download().reshape(S, FH, stride)
    for s in range(S):
        assert diff(back[s, :, :3 * FW], want[s]) is None and not back[s, :, 3 * FW:].any()
    dev.free()
    if which == "bytetrack":                                                    # the reference's filter (tsu == 0 after ageing) passes none
        same = [f.copy() for f in frames]
        mask.apply_tracker(SimpleNamespace(_core=core, report="reference"), same)
        assert all(np.array_equal(a, b) for a, b in zip(same, frames))
    with pytest.raises(TypeError, match="apply\\(frame, tracks\\)"):
        mask.apply_tracker(object(), got)
    mask.close(); core.close()


@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_privacy")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, batch=2, warmup=False, autotune=False)
    yield det
    det.close()


def test_apply_detector_equals_apply_on_the_fetched_detections(pkg, detector):
    frames = [f.copy() for f in pkg.synth.frames(2, 320, 320, seed=11)]
    dets = detector.detect_batch(frames)
    assert sum(len(d) for d in dets) > 0
    for m in (MODES[3], MODES[6]):
        mask = pkg.visualization.PrivacyMask(**m)
        want = [mask.apply(f.copy(), d) for f, d in zip(frames, dets)]
        for f, d, w_ in zip(frames, dets, want):
            assert np.array_equal(w_, PR.apply(f, d.xyxy, d.class_id, **m))
        got = [f.copy() for f in frames]
        mask.apply_detector(detector, got)
        for g, w_ in zip(got, want):
            assert diff(g, w_) is None, diff(g, w_)
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            mask.apply_detector(detector, got + [got[0]])                       # more frames than the batch held
        assert e.value.code == pkg._ffi.E_INVALID
        mask.close()


class _Rec:
    def __init__(self):
        self.frames = []

    def write(self, frame):
        self.frames.append(frame.copy())


class _Det:
    model = type("M", (), {"names": {0: "person"}})()

    def detect(self, frame):
        return type("D", (), {"xyxy": np.zeros((1, 4), np.float32), "confidence": np.ones(1, np.float32), "class_id": np.zeros(1, np.int32),
                              "__len__": lambda self: 1})()


class _Trk:
    def update_from_detector(self, det, materialize=True):
        return [SimpleNamespace(track_id=4, xyxy=np.array([2, 12, 30, 40], np.float32), confidence=0.9, class_name="person", class_id=0,
                                trail=[(5, 5), (16, 26)])] if materialize else []


def test_pipeline_privacy_stage(pkg, detector):
    """3 frames: the recorded frame is the render of the masked frame (labels and boxes on top of the mask), and the stage table
    gains exactly the privacy row."""
    frames = np.random.default_rng(9).integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof(), max_frames=3, device_stages=False,
                            renderer=pkg.FrameRenderer(show_fps=False))
    rec = _Rec()
    mask = pkg.visualization.PrivacyMask(mode="pixelate", cell=8)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof(), max_frames=3, device_stages=False,
                           renderer=pkg.FrameRenderer(show_fps=False), recorder=rec, privacy=mask)
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"privacy_mean_ms"} and rows(base) <= rows(out)
    assert pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events", "visualization", "total"]
    tracks = _Trk().update_from_detector(None)
    assert len(rec.frames) == 3
    for i in range(3):
        masked = PR.apply(frames[i % 2], [tracks[0].xyxy], [0], mode="pixelate", cell=8)
        assert not np.array_equal(masked, frames[i % 2])
        assert np.array_equal(rec.frames[i], RR.render(masked, tracks, None, show_fps=False)), i
    # no materialised track list (the crossing counter reads the tracker's device state): the mask does, too
    trk = pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    trk.report = "matched"
    counter = pkg.events.CrossingCounter([{"name": "l", "a": [0, 160], "b": [320, 160]}])
    src = pkg.synth.frames(2, 320, 320, seed=11)
    rec = _Rec()
    pkg.pipeline.run(pkg.pipeline.SyntheticSource(src), detector, trk, prof(), max_frames=3, crossing_counter=counter, recorder=rec, privacy=mask)
    st = trk._core.snapshot(0)
    idx = np.nonzero(st["tsu"] == 1)[0]
    assert len(idx) > 0
    assert np.array_equal(rec.frames[2], PR.apply(src[0], st["xyxy"][idx], st["cls"][idx], mode="pixelate", cell=8))
    mask.close(); counter.close()
