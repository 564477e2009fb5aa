"""GPU: the life of every handle class through the shared skeleton (csrc/handle_host.h, _ffi.Handle), each at its smallest valid size:
created and closed with no call in between; created, one smallest call, its device time positive and finite, closed, closed again;
and the device time of a handle that has launched nothing refused with ``E_INVALID`` in that module's own words.  Each case is a few
launches on a 64 x 64 frame.  A timer with several intervals may report an empty one as 0.0 (OC-SORT has no descriptor launch): every
interval is finite and not negative and their sum is positive."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmc_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
H = W = 64
BOX = np.float32([[8, 8, 40, 48]])
CONF, CLS = np.float32([0.9]), np.int32([0])


def frame(seed=1):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def track(pkg):
    return pkg.Track(track_id=1, xyxy=BOX[0].copy(), confidence=0.9, class_id=0, class_name="person")


def _reid(pkg, tmp_path):
    path = str(tmp_path / "osnet_synth.rtreid")
    pkg.reid_weights.save(path, pkg.reid_weights.synthetic(0))
    return pkg.tracking.reid.ReidEmbedder(path, max_boxes=1, max_frames=1)


def _lens(pkg):
    lc = pkg.ingestion.lens.LensCorrector(1, (H, W))
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    lc.set_map(0, x, y)
    return lc


def _compositor(pkg):
    R = pkg.visualization.compose
    return R.Compositor([(H, W)], [R.Output((H, W))], [R.Cell(0, 0, (0, 0, W, H))])


def _gmc_frames():
    return G.pan_sequence(96, 160, 1, [(3, -2)], margin=32)


# name -> (create(pkg, tmp_path), the smallest call, device time or None, the words of "nothing has launched yet" or None)
CASES = {
    "PrivacyMask": (lambda p, t: p.PrivacyMask(), lambda o, p: o.apply(frame(), BOX), lambda o: o.last_kernel_ms(), "no apply call has launched yet"),
    "FrameRenderer": (lambda p, t: p.FrameRenderer(), lambda o, p: o.render(frame(), [track(p)]), lambda o: o.last_kernel_ms(),
                      "no render_batch has run a kernel yet"),
    "JpegEncoder": (lambda p, t: p.JpegEncoder(max_height=H, max_width=W, max_batch=1), lambda o, p: o.encode(frame()), lambda o: o.last_kernel_ms(),
                    "no encode_batch has run a kernel yet"),
    "JpegDecoder": (lambda p, t: p.JpegDecoder(max_height=H, max_width=W, max_batch=1), lambda o, p: o.decode(_jpeg_file(p)), lambda o: o.last_kernel_ms(),
                    "no decode_batch has run a kernel yet"),
    "Compositor": (lambda p, t: _compositor(p), lambda o, p: o.run([frame()]), lambda o: o.last_ms(), "no run has launched yet"),
    "SnapshotGallery": (lambda p, t: p.visualization.snapshots.SnapshotGallery((8, 8), max_tracks=4), lambda o, p: o.process([track(p)], frame(), 0),
                        lambda o: o.last_kernel_ms(), "no call has been timed yet"),
    "Heatmap": (lambda p, t: p.Heatmap(1, H, W), lambda o, p: o.accumulate([BOX]), lambda o: o.last_kernel_ms(), "no accumulate or overlay call has launched yet"),
    "LensCorrector": (lambda p, t: _lens(p), lambda o, p: o.process([frame()]), lambda o: o.last_ms(), "no process call has launched yet"),
    "Stabilizer": (lambda p, t: p.ingestion.stabilizer.Stabilizer(1, (H, W)), lambda o, p: o.process([frame()], np.float32([[[1, 0, 0], [0, 1, 0]]])),
                   lambda o: o.last_ms(), "no process call has launched yet"),
    "CameraHealth": (lambda p, t: p.ingestion.health.CameraHealth(1, H, W), lambda o, p: o.process([frame()]), lambda o: o.last_kernel_ms(),
                     "no process call has launched yet"),
    "MotionDetector": (lambda p, t: p.MotionDetector(1, H, W), lambda o, p: o.process([frame()]), lambda o: o.last_kernel_ms(), "no process call has launched yet"),
    "LeftObjectDetector": (lambda p, t: p.LeftObjectDetector(1, H, W), lambda o, p: o.process([frame()]), lambda o: o.last_kernel_ms(),
                           "no process call has launched yet"),
    "ReidEmbedder": (_reid, lambda o, p: o.embed([frame()], [BOX]), lambda o: o.last_ms(), "no embed has run yet"),
    "IdSwapGuard": (lambda p, t: p.IdSwapGuard(max_tracks=4), lambda o, p: o.process_arrays([1], BOX, frame(), 0), lambda o: tuple(o.last_ms().values()),
                    "no call has been timed yet"),
    "CrossCameraLinker": (lambda p, t: p.tracking.crosscam.CrossCameraLinker(1, 64, max_tracks=4, max_identities=4, max_queries=4),
                          lambda o, p: o.process([([1], [0], np.full((1, 64), 16, np.int8))]), lambda o: o.last_ms(), "crosscam: no call yet"),
    "CameraMotionEstimator": (lambda p, t: p.CameraMotionEstimator(downscale=1), lambda o, p: [o.estimate([f]) for f in _gmc_frames()], lambda o: o.last_ms(),
                              "no estimate has run yet"),
    "DeepSortCore": (lambda p, t: p.tracking.deepsort._DeepSortCore(max_tracks=4, max_dets=4), lambda o, p: o.update(BOX, CONF, CLS, frame=frame()),
                     lambda o: o.last_ms(), "no update has run yet"),
    "OcSortCore": (lambda p, t: p.tracking.ocsort._OcSortCore(max_tracks=4, max_dets=4), lambda o, p: o.update(BOX, CONF, CLS), lambda o: o.last_ms(),
                   "no update has run yet"),
    "BotSortCore": (lambda p, t: p.tracking.botsort._BotSortCore(max_tracks=4, max_dets=4), lambda o, p: o.update(BOX, CONF, CLS), lambda o: o.last_ms(),
                    "no update has run yet"),
    # no device timer in these four
    "ByteTrackCore": (lambda p, t: p.tracking.tracker._ByteTrackCore(max_tracks=4, max_dets=4), lambda o, p: o.update(BOX, CONF, CLS), None, None),
    "ZoneEventEngine": (lambda p, t: p.ZoneEventEngine([], log_path=str(t / "events.jsonl"), max_tracks=4), lambda o, p: o.process([track(p)], 0, now=0.0), None, None),
    "CrossingCounter": (lambda p, t: p.CrossingCounter(max_tracks=4), lambda o, p: o.process([track(p)], 0), None, None),
    "SpeedEstimator": (lambda p, t: p.SpeedEstimator(mm_per_pixel=1.0, max_tracks=4), lambda o, p: o.process([track(p)], 0), None, None),
}


def _jpeg_file(pkg):
    enc = pkg.JpegEncoder(max_height=H, max_width=W, max_batch=1)
    try:
        return enc.encode(frame())
    finally:
        enc.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_create_and_close(pkg, tmp_path, name):
    obj = CASES[name][0](pkg, tmp_path)
    assert obj._h
    obj.close()
    assert obj._h is None


@pytest.mark.parametrize("name", sorted(CASES))
def test_create_one_call_close_twice(pkg, tmp_path, name):
    create, call, ms, _ = CASES[name]
    obj = create(pkg, tmp_path)
    call(obj, pkg)
    if ms is not None:
        v = ms(obj)
        parts = v if isinstance(v, tuple) else (v,)
        print(f"{name}: device time {parts} ms")
        assert all(math.isfinite(x) and x >= 0 for x in parts) and sum(parts) > 0, parts
    obj.close()
    assert obj._h is None
    obj.close()


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c[3]))
def test_device_time_of_a_fresh_handle(pkg, tmp_path, name):
    create, _, ms, words = CASES[name]
    obj = create(pkg, tmp_path)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        ms(obj)
    assert e.value.code == pkg._ffi.E_INVALID and e.value.msg == words, str(e.value)
    obj.close()
