"""GPU: 4:2:0 (NV12 / I420) input, converted and letterboxed on the GPU (csrc/preprocess.hip: letterbox_yuv420_kernel).
The bar is BIT identity with the BGR path fed the restated BGR frames (tests/yuv420_ref.py): the letterboxed input, the pre-NMS
tensor, the detections (boxes and scores as int32 bit patterns), the tracker state behind the device hand-off -- under every
engine shape, with host (pageable and page-locked) and device frames, padded layouts included."""
import os
import sys

import numpy as np
import pytest

from oracle import yolo_oracle as Y

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv420_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wdir(tmp_path_factory):
    return tmp_path_factory.mktemp("weights_yuv")


def weights_path(pkg, wdir, scale, size):
    path = os.path.join(str(wdir), f"yolov8{scale}_{size}_noise.rtw")
    if not os.path.exists(path):
        pkg.weights.save(path, pkg.weights.synthetic(scale, input_size=size), scale)
    return path


def make(pkg, wdir, size=320, scale="s", **kw):
    kw.setdefault("autotune", False)
    return pkg.Detector(weights_path(pkg, wdir, scale, size), input_size=(size, size), warmup=False, **kw)


def same(a, b):
    return (np.array_equal(a.xyxy.view(np.int32), b.xyxy.view(np.int32)) and np.array_equal(a.confidence.view(np.int32), b.confidence.view(np.int32))
            and np.array_equal(a.class_id, b.class_id))


def yuv_and_bgr(pkg, n, h, w, fmt, seed):
    yuv = pkg.synth.yuv420_frames(n, h, w, fmt, seed=seed)
    bgr = np.stack([R.to_bgr(f, h, w, fmt) for f in yuv])
    return yuv, bgr


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("h,w,size", [(640, 640, 640), (1080, 1920, 640), (480, 640, 640), (720, 1280, 320), (38, 54, 64)])
def test_preprocess_yuv420_bit_exact(pkg, fmt, h, w, size):
    yuv, bgr = yuv_and_bgr(pkg, 1, h, w, fmt, seed=h + w)
    want = Y.preprocess(bgr[0], size, size).astype(np.float16)
    got = pkg._ffi.preprocess_yuv420(yuv[0], fmt, size, size)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # a decoder surface: an odd-looking Y pitch, the chroma after a padded height (1080 -> 1088 rows), a chroma pitch of its own
    rows = h + 8 if h % 16 else h + 16
    cp = 0 if fmt == "nv12" else w // 2 + 3
    buf, kw = R.relayout(yuv[0], h, w, fmt, w + 26, rows, cp)
    fm = pkg._ffi.frame_format(fmt, h, w, **kw)
    got2 = pkg._ffi.preprocess_yuv420(buf, fm, size, size, height=h, width=w)
    assert np.array_equal(got2.view(np.uint16), want.view(np.uint16))


# ------------------------------------------------------------------ through the engine
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("h,w", [(320, 320), (240, 416)])
def test_engine_yuv_equals_bgr_path(pkg, wdir, fmt, h, w):
    """Batch 3 from host pageable, host page-locked and device frames (and a padded device layout): input tensor, pre-NMS tensor and
    detections bit-identical to the BGR path fed the restated frames."""
    B = 3
    yuv, bgr = yuv_and_bgr(pkg, B, h, w, fmt, seed=31)
    ref_det = make(pkg, wdir, batch=B)
    ref = ref_det.detect_batch(list(bgr))
    ref_dbg = [ref_det.debug_fetch(i, want_heads=False) for i in range(B)]
    ref_det.close()
    assert sum(len(d) for d in ref) > 0
    det = make(pkg, wdir, batch=B, pixel_format=fmt)

    def check(got, what):
        for i in range(B):
            assert same(got[i], ref[i]), (what, i)
            inp, _, pred = det.debug_fetch(i, want_heads=False)
            assert np.array_equal(inp.view(np.uint16), ref_dbg[i][0].view(np.uint16)), (what, "input", i)
            assert np.array_equal(pred.view(np.int32), ref_dbg[i][2].view(np.int32)), (what, "pred", i)

    check(det.detect_batch([f.copy() for f in yuv]), "pageable")
    ring = pkg.pipeline.PinnedFrameRing(B, h, w, pixel_format=fmt)
    for i in range(B):
        ring.write(i, yuv[i])
    check(det.detect_batch([ring.frame(i) for i in range(B)]), "page-locked")
    buf = pkg._ffi.DeviceBuffer(yuv.nbytes)
    buf.upload(yuv)
    per = yuv[0].nbytes
    det.enqueue([buf.ptr + i * per for i in range(B)], height=h, width=w)
    check(det.fetch(), "device")
    pads = [R.relayout(f, h, w, fmt, w + 64, h + 16) for f in yuv]
    stride = max(p[0].nbytes for p in pads)
    pbuf = pkg._ffi.DeviceBuffer(stride * B)
    for i, (b, _) in enumerate(pads):
        pbuf.upload(b, i * stride)
    kw = pads[0][1]
    det.enqueue([pbuf.ptr + i * stride for i in range(B)], height=h, width=w, pitch=kw["pitch"], u_offset=kw["u_offset"],
                v_offset=kw.get("v_offset", 0))
    check(det.fetch(), "device, padded layout")
    buf.free(); pbuf.free(); ring.close(); det.close()


@pytest.mark.parametrize("chains", [1, 2, -1, -2], ids=["plain", "two-chains", "two-stages", "three-stages"])
def test_yuv_under_every_engine_shape(pkg, wdir, chains):
    """Batches of 4 pipelined through the plain engine, two sub-batch chains, two and three stages (graphs on), NV12 from the device and
    I420 from the host: the detections of the plain BGR engine, bit for bit."""
    nv, bgr = yuv_and_bgr(pkg, 12, 320, 320, "nv12", seed=77)
    i4, bgr_s = yuv_and_bgr(pkg, 4, 240, 416, "i420", seed=78)
    ref_det = make(pkg, wdir, batch=4, chains=1)
    ref = [ref_det.detect_batch(list(bgr[4 * t:4 * t + 4])) for t in range(3)] + [ref_det.detect_batch(list(bgr_s))]
    ref_det.close()
    det = make(pkg, wdir, batch=4, chains=chains, pixel_format="nv12")
    buf = pkg._ffi.DeviceBuffer(nv.nbytes)
    buf.upload(nv)
    per = nv[0].nbytes
    depth = (det.model.stages + 1) if det.model.stages > 1 else 2
    got = []
    for t in range(3):
        det.enqueue([buf.ptr + (4 * t + i) * per for i in range(4)], height=320, width=320)
        if t >= depth - 1:
            got.append(det.fetch())
    while len(got) < 3:
        got.append(det.fetch())
    det.enqueue(list(i4), pixel_format="i420")
    got.append(det.fetch())
    for t in range(4):
        for i in range(4):
            assert same(got[t][i], ref[t][i]), (chains, t, i)
    assert sum(len(d) for b in got for d in b) > 0
    buf.free()
    det.close()


def test_yuv_rect_mode_1080p(pkg, wdir):
    """rect=True at 1080p: the 384 x 640 rectangle, same input tensor and detections as the BGR path."""
    nv, bgr = yuv_and_bgr(pkg, 1, 1080, 1920, "nv12", seed=9)
    ref_det = make(pkg, wdir, size=640, scale="n", rect=True)
    ref = ref_det.detect(bgr[0])
    ref_inp = ref_det.debug_fetch(0, want_heads=False, want_pred=False)[0]
    ref_det.close()
    det = make(pkg, wdir, size=640, scale="n", rect=True, pixel_format="nv12")
    got = det.detect(nv[0])
    assert det.model.input_hw == (384, 640)
    inp = det.debug_fetch(0, want_heads=False, want_pred=False)[0]
    assert np.array_equal(inp.view(np.uint16), ref_inp.view(np.uint16)) and same(got, ref)
    det.close()


def test_bgr_and_nv12_batches_alternate_on_one_detector(pkg, wdir):
    nv, bgr = yuv_and_bgr(pkg, 6, 320, 320, "nv12", seed=5)
    ref_det = make(pkg, wdir, batch=2)
    ref = [ref_det.detect_batch(list(bgr[2 * t:2 * t + 2])) for t in range(3)]
    ref_det.close()
    det = make(pkg, wdir, batch=2)                             # default bgr24; NV12 per call
    for rnd in range(2):
        for t in range(3):
            if (t + rnd) % 2:
                det.enqueue(list(nv[2 * t:2 * t + 2]), pixel_format="nv12")
            else:
                det.enqueue(list(bgr[2 * t:2 * t + 2]))
            got = det.fetch()
            assert same(got[0], ref[t][0]) and same(got[1], ref[t][1]), (rnd, t)
    det.close()


def test_tracker_handoff_after_nv12_batch(pkg, wdir):
    """rtmodt_tracker_update_from_detector after NV12 batches == after the equivalent BGR batches (device-resident hand-off)."""
    from importlib import import_module
    from oracle import tracker_oracle as T
    core_cls = import_module(pkg.__name__ + ".tracking.tracker")._ByteTrackCore
    B = 4
    nv, bgr = yuv_and_bgr(pkg, 5 * B, 320, 320, "nv12", seed=21)
    dets = {}
    for fmt, frames in (("bgr24", bgr), ("nv12", nv)):
        det = make(pkg, wdir, batch=B, pixel_format=fmt)
        core = core_cls(n_streams=B, max_dets=128, max_tracks=512)
        for t in range(5):
            det.enqueue(list(frames[t * B:(t + 1) * B]))
            core.update_from_detector(det)
            det.fetch()
        dets[fmt] = [T.state_digest(core.snapshot(i)) for i in range(B)]
        n = sum(len(core.snapshot(i)["ids"]) for i in range(B))
        det.close()
    assert n > 0
    for i in range(B):
        assert np.array_equal(dets["bgr24"][i], dets["nv12"][i]), i


def test_pipeline_fed_by_raw_nv12_reader_through_pinned_ring(pkg, wdir, tmp_path):
    """pipeline.run on FrameReader(raw, nv12) writing into a page-locked NV12 ring: every frame the loop read, replayed as BGR through
    the BGR detector and a fresh tracker, gives the same detections and the same tracker state."""
    from oracle import tracker_oracle as T
    h = w = 320
    nv, bgr = yuv_and_bgr(pkg, 6, h, w, "nv12", seed=12)
    path = tmp_path / "clip.nv12"
    path.write_bytes(nv.tobytes())
    ring = pkg.pipeline.PinnedFrameRing(3, h, w, pixel_format="nv12")
    det = make(pkg, wdir, pixel_format="nv12")
    trk = pkg.MultiObjectTracker("bytetrack")

    class Recorder:
        def __init__(self, src):
            self.src, self.seen, self.dets = src, [], []

        def read(self):
            ok, f, fid = self.src.read()
            if ok:
                self.seen.append(f.copy())
            return ok, f, fid

    with pkg.ingestion.FrameReader(str(path), backend="raw", resolution=(w, h), pixel_format="nv12", ring=ring,
                                   reconnect_delay=0.01, max_reconnects=1000) as reader:
        import time
        t0 = time.perf_counter()
        while not reader.read()[0] and time.perf_counter() - t0 < 5.0:
            time.sleep(0.002)
        rec = Recorder(reader)
        prof = pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=2, log_interval=1000)
        out = pkg.pipeline.run(rec, det, trk, prof, max_frames=20)
    assert len(rec.seen) == 20 and all(any(np.array_equal(f, g) for g in nv) for f in rec.seen)
    last_nv = det.detect(rec.seen[-1])
    ref_det = make(pkg, wdir)
    ref_trk = pkg.MultiObjectTracker("bytetrack")
    seen_bgr = np.stack([R.to_bgr(f, h, w, "nv12") for f in rec.seen])
    prof2 = pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=2, log_interval=1000)
    out2 = pkg.pipeline.run(pkg.pipeline.SyntheticSource(seen_bgr), ref_det, ref_trk, prof2, max_frames=20)
    assert out["last_detections"] == out2["last_detections"] and out["last_tracks"] == out2["last_tracks"]
    assert np.array_equal(T.state_digest(trk._core.snapshot()), T.state_digest(ref_trk._core.snapshot()))
    assert same(last_nv, ref_det.detect(seen_bgr[-1]))
    ring.close(); det.close(); ref_det.close()


def test_invalid_layouts_are_refused_and_the_detector_keeps_working(pkg, wdir):
    import ctypes as C
    F = pkg._ffi
    nv, bgr = yuv_and_bgr(pkg, 1, 320, 320, "nv12", seed=3)
    det = make(pkg, wdir, pixel_format="nv12")
    ref = det.detect(nv[0])
    L = F.lib()
    arr = (C.c_void_p * 1)(nv[0].ctypes.data)
    cases = [(F.FrameFormat(F.PIX_NV12, 0, 0, 0, 0, 0), 319, 320, F.E_INVALID),              # odd height
             (F.FrameFormat(F.PIX_NV12, 0, 300, 0, 0, 0), 320, 320, F.E_INVALID),            # pitch < width
             (F.FrameFormat(F.PIX_I420, 0, 0, 0, 320 * 100, 0), 320, 320, F.E_INVALID),      # U inside Y
             (F.FrameFormat(F.PIX_I420, 0, 0, 0, 0, 320 * 320 + 10), 320, 320, F.E_INVALID),  # V inside U
             (F.FrameFormat(9, 0, 0, 0, 0, 0), 320, 320, F.E_INVALID),                        # unknown format
             (F.FrameFormat(F.PIX_NV12, 2, 0, 0, 0, 0), 320, 320, F.E_UNSUPPORTED)]           # BT.709 etc.: not yet
    for fm, h, w, code in cases:
        assert L.rtmodt_detector_enqueue_batch_fmt(det.model.handle, arr, 1, h, w, C.byref(fm), F.MEM_HOST) == code
        assert L.rtmodt_last_error()
    fm = F.FrameFormat(F.PIX_NV12, 0, 0, 0, 1 << 26, 0)           # a span beyond the staging area: E_CAPACITY, sizes in the message
    assert L.rtmodt_detector_enqueue_batch_fmt(det.model.handle, arr, 1, 320, 320, C.byref(fm), F.MEM_HOST) == F.E_CAPACITY
    assert b"spans" in L.rtmodt_last_error()
    with pytest.raises(ValueError):                               # ... which Python refuses before the call: the array is shorter
        det.enqueue([nv[0]], u_offset=1 << 26)
    with pytest.raises(ValueError):
        det.enqueue([nv[0][:-2]])
    assert same(det.detect(nv[0]), ref)
    # fmt == NULL is BGR24 with pitch 3w, exactly enqueue_batch
    arr_b = (C.c_void_p * 1)(bgr[0].ctypes.data)
    F.check(L.rtmodt_detector_enqueue_batch_fmt(det.model.handle, arr_b, 1, 320, 320, None, F.MEM_HOST))
    det._in_flight.append(1); det._keepalive.append(None)
    assert same(det.fetch()[0], ref)
    det.close()
