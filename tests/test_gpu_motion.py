"""GPU: the motion detector (csrc/motion.hip, csrc/motion_model.h) against the NumPy restatement tests/motion_ref.py: after every frame
the status, the counts, the box, the regions, the mask, the block grid and the whole model state are the restatement's; the
interface's behaviour and refusals; the pipeline's motion stage.  Every comparison is == on integers.  PARITY UNPINNED: OpenCV's
MOG2 and Frigate are installed nowhere this runs; no default has been validated on real footage."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import motion_cases as MC
import motion_ref as MR

pytestmark = pytest.mark.gpu

#: (h, w, stride): partial edge cells in both directions, odd pitches; 150 x 530 spans several tiles in x and y at every scale
GEOMETRIES = [(37, 70, 211), (70, 37, 117), (19, 150, 452), (150, 530, 1601)]
SCALES = [1, 2, 4, 8]
KEYS = ("stream", "status", "n_raw", "n_fg", "luma_sum", "bbox", "regions", "n_regions_total", "frames_seen")


def padded(frame, stride, seed):
    """The frame as a view into a buffer of rows `stride` bytes apart whose padding bytes are junk -> (buffer, view)."""
    h, w = frame.shape[:2]
    buf = np.random.default_rng(seed).integers(0, 256, h * stride, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (stride, 3, 1))
    view[:] = frame
    return buf, view


def as_dict(r):
    return dict(stream=r.stream, status=r.status, n_raw=r.n_raw, n_fg=r.n_fg, luma_sum=r.luma_sum, bbox=tuple(r.bbox), regions=list(r.regions),
                n_regions_total=r.n_regions_total, frames_seen=r.frames_seen)


def check(det, ref, got, want, what):
    """One call's results and everything a stream holds afterwards against the restatement."""
    assert len(got) == len(want), what
    for g, w_ in zip(got, want):
        g = as_dict(g)
        for k in KEYS:
            assert g[k] == w_[k], (what, k, g[k] if k != "regions" else g[k][:4], w_[k] if k != "regions" else w_[k][:4])
        s = w_["stream"]
        assert np.array_equal(det.mask(s), ref.masks[s]), (what, "mask", s)
        assert np.array_equal(det.blocks(s), ref.block_grids[s]), (what, "blocks", s)
        bg, dev, seen = det.state(s)
        rbg, rdev, rseen = ref.state(s)
        assert np.array_equal(bg, rbg) and np.array_equal(dev, rdev) and seen == rseen, (what, "state", s)


class DeviceFrames:
    """n frames in one device buffer, the first at `offset`, rows `stride` apart, the padding junk."""

    def __init__(self, pkg, n, h, stride, offset):
        self.n, self.h, self.stride, self.offset = n, h, stride, offset
        self.buf = pkg._ffi.DeviceBuffer(offset + n * h * stride)

    def put(self, frames, seed):
        for i, f in enumerate(frames):
            b, _ = padded(f, self.stride, seed + i)
            self.buf.upload(b, self.offset + i * self.h * self.stride)
        return self.buf


@functools.lru_cache(maxsize=None)
def sequences(h, w, streams):
    return [MC.sequence(h, w, 100 * h + s) for s in range(streams)]


# ---- the 40-frame sequence over geometries and scales -----------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("h,w,stride", GEOMETRIES)
def test_sequence_equals_restatement(pkg, h, w, stride, scale):
    """Host frames at the odd pitch; device frames at the same pitch from a base offset by 1 (the byte path); device frames at
    the pitch rounded up to a multiple of 4 from a base offset by 4 (the wide path).  One restatement for the three."""
    S = 2 if h * w > 20000 else 3
    seqs = sequences(h, w, S)
    ref = MR.Ref(S, h, w, scale=scale)
    wide_stride = (stride + 3) // 4 * 4
    dets = [pkg.MotionDetector(S, h, w, scale=scale) for _ in range(3)]
    dev1, dev4 = DeviceFrames(pkg, S, h, stride, 1), DeviceFrames(pkg, S, h, wide_stride, 4)
    statuses = []
    for f in range(MC.N_FRAMES):
        frames = [seqs[s][f] for s in range(S)]
        want = ref.process(frames)
        statuses.append(want[0]["status"])
        keep = [padded(fr, stride, f * 7 + s) for s, fr in enumerate(frames)]
        check(dets[0], ref, dets[0].process([v for _, v in keep]), want, ("host", f))
        check(dets[1], ref, dets[1].process(dev1.put(frames, f), stride=stride, offset=1), want, ("device + 1", f))
        check(dets[2], ref, dets[2].process(dev4.put(frames, f), stride=wide_stride, offset=4), want, ("device + 4", f))
    assert all(d.last_kernel_ms() >= 0 for d in dets)
    if (h, w) == (150, 530):
        # what the defaults answer on this scene, asserted on the restatement so that equality cannot hide an empty comparison
        W_, S_, M_, X_ = MR.WARMUP, MR.STILL, MR.MOTION, MR.SCENE_CHANGE
        first, n, step = MC.RECT_FIRST, MC.RECT_FRAMES, MC.STEP_AT
        assert statuses == [W_] * 8 + [S_] * (first - 8) + [M_] * n + [S_] * (step - first - n) + [X_] + [W_] * 8 + [S_] * (MC.N_FRAMES - step - 9)
        again = MR.Ref(1, h, w, scale=scale)
        totals = [again.step(0, fr)["n_regions_total"] for fr in seqs[0][:first + n + 1]]
        assert totals[first:first + n] == [1] * n and totals[first + n] == 0 and not any(totals[:first])
    for d in dets:
        d.close()
    dev1.buf.free(); dev4.buf.free()


# ---- sparse speckle: many components, truncation -----------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(37, 70), (150, 530)])
def test_sparse_speckle(pkg, h, w):
    for ci, cfg in enumerate((dict(threshold=6, dev_gain=0, min_neighbors=1, dilate=0, min_area=1), dict(threshold=6, dev_gain=0, min_neighbors=1, dilate=0, min_area=2),
                              dict(threshold=6, dev_gain=0, min_neighbors=2, dilate=1, min_area=3))):
        for max_regions in ((32, 256) if ci == 0 else (32,)):
            rng = np.random.default_rng(h + ci)
            ref = MR.Ref(1, h, w, scale=1, max_regions=max_regions, **cfg)
            det = pkg.MotionDetector(1, h, w, scale=1, max_regions=max_regions, **cfg)
            flat = np.full((h, w), 100 << 8, np.uint16)
            ref.load_state(flat, np.zeros_like(flat), 8)
            det.load_state(flat, np.zeros_like(flat), 8)
            for f in range(3):
                frame = MC.cells_to_frame(MC.speckle(h, w, rng), 1, h, w)
                want = ref.process([frame])
                if ci < 2 and (max_regions == 32 or h == 150):
                    assert want[0]["n_regions_total"] > max_regions and len(want[0]["regions"]) == max_regions, want[0]["n_regions_total"]
                assert want[0]["status"] == MR.MOTION
                check(det, ref, det.process([frame]), want, (cfg, max_regions, f))
            det.close()


# ---- components that cross every tile ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("shape", ["spiral", "comb", "diagonal", "full"])
def test_labelling_shapes(pkg, shape, scale):
    h, w = 150, 530
    cfg = dict(scale=scale, min_neighbors=1, dilate=0, min_area=1, learn_shift_fg=0)
    ref, det = MR.Ref(1, h, w, **cfg), pkg.MotionDetector(1, h, w, **cfg)
    gh, gw = ref.gh, ref.gw
    cells = MC.SHAPES[shape](gh, gw)
    flat = np.full((gh, gw), 100 << 8, np.uint16)
    for frame_cells in (cells, 1 - cells, cells):                               # the shape, its complement, the shape again
        ref.load_state(flat, np.zeros_like(flat), 8)
        det.load_state(flat, np.zeros_like(flat), 8)
        frame = MC.cells_to_frame(100 + 100 * frame_cells.astype(np.uint8), scale, h, w)
        want = ref.process([frame])
        assert np.array_equal(ref.masks[0], frame_cells) and want[0]["n_fg"] == int(frame_cells.sum())
        if frame_cells is cells:
            assert want[0]["n_regions_total"] == 1 and want[0]["regions"] == [(0, 0, w, h, int(cells.sum()))]
        check(det, ref, det.process([frame]), want, (shape, scale))
    det.close()


# ---- absorption --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg", [2, 0])
def test_a_stopped_rectangle_is_absorbed_or_not(pkg, fg):
    h, w, scale = 37, 70, 2
    cfg = dict(scale=scale, learn_shift=2, learn_shift_fg=fg, dev_gain=0)
    ref, det = MR.Ref(1, h, w, **cfg), pkg.MotionDetector(1, h, w, **cfg)
    base = np.full((h, w, 3), 90, np.uint8)
    lit = base.copy()
    lit[10:26, 20:44] = 190
    in_mask = []
    for f in range(8 + 14):
        frame = base if f < 8 else lit
        want = ref.process([frame])
        in_mask.append(want[0]["n_fg"] > 0)
        check(det, ref, det.process([frame]), want, (fg, f))
    # d -= d >> 2 per frame from 25600: 19200, 14400, 10800, 8100, 6075, 4557, 3418, 2564 <= 12 << 8: raw for eight frames
    if fg:
        assert in_mask[8] and not in_mask[-1] and in_mask[8:].index(False) == 8
    else:
        assert all(in_mask[8:])
    det.close()


# ---- interface ---------------------------------------------------------------------------------------------------------
def test_stream_lists_state_round_trip_and_reset(pkg):
    h, w, stride, S, scale = 37, 70, 211, 4, 2
    seqs = [MC.sequence(h, w, 900 + s) for s in range(S)]
    cfg = dict(scale=scale, warmup=3)
    ref, det = MR.Ref(S, h, w, **cfg), pkg.MotionDetector(S, h, w, **cfg)
    clock = [0] * S                                                             # each stream advances through its own sequence

    def go(streams):
        frames = []
        for s in streams:
            frames.append(seqs[s][10 + clock[s]])                               # (from frame 10 on: the rectangle arrives after the short warm-up)
            clock[s] += 1
        before = {s: (det.state(s), det.mask(s), det.blocks(s)) for s in range(S) if s not in streams}
        want = ref.process(frames, streams)
        check(det, ref, det.process([padded(f, stride, 5)[1] for f in frames], streams), want, streams)
        for s, (st, mk, bl) in before.items():                                  # untouched streams keep their state bit for bit
            now = det.state(s)
            assert np.array_equal(now[0], st[0]) and np.array_equal(now[1], st[1]) and now[2] == st[2] and np.array_equal(det.mask(s), mk) \
                and np.array_equal(det.blocks(s), bl), (streams, s)
    for streams in ([0, 1, 2, 3], [3, 1, 0, 2], [2], [1, 3], [3, 0], [0, 1, 2, 3], [2, 1], [1], [1], [1], [3, 2, 1, 0], [0, 2], [1, 2, 3]):
        go(streams)
    assert any(ref.masks[s].any() for s in range(S)) and len(set(ref.seen)) > 1
    # a model survives a restart: a second handle loaded with stream 1's state goes on exactly as the first
    again = pkg.MotionDetector(1, h, w, **cfg)
    bg, dev, seen = det.state(1)
    again.load_state(bg, dev, seen)
    for _ in range(4):
        frame = seqs[1][10 + clock[1]]
        clock[1] += 1
        a, b = det.process([frame], [1])[0], again.process([frame])[0]
        ref.process([frame], [1])
        da, db = as_dict(a), as_dict(b)
        assert {k: da[k] for k in KEYS if k != "stream"} == {k: db[k] for k in KEYS if k != "stream"}
        sa, sb = det.state(1), again.state(0)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2] == sb[2] and np.array_equal(det.mask(1), again.mask(0))
    # reset: one stream, then all
    det.reset(2); ref.reset(2)
    assert det.state(2)[2] == 0 and not det.mask(2).any() and not det.blocks(2).any() and det.state(1)[2] == ref.seen[1] > 0
    go([2, 1])
    assert ref.seen[2] == 1
    det.reset(); ref.reset()
    assert all(det.state(s)[2] == 0 and not det.state(s)[0].any() for s in range(S))
    go([0, 1, 2, 3])
    with pytest.raises(ValueError):
        det.load_state(np.zeros((3, 3), np.uint16), np.zeros((3, 3), np.uint16), 0)
    det.close(); again.close()


def test_refusals(pkg):
    h, w, stride, S = 37, 70, 211, 3
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    L = F.lib()
    fresh = pkg.MotionDetector(S, h, w)
    with pytest.raises(E) as e:
        fresh.last_kernel_ms()                                                  # nothing has launched yet
    assert e.value.code == F.E_INVALID and "no process call" in e.value.msg
    fresh.close()
    det = pkg.MotionDetector(S, h, w, warmup=2)
    ref = MR.Ref(S, h, w, warmup=2)
    seqs = [MC.sequence(h, w, 40 + s, 4) for s in range(S)]
    for f in range(3):
        check(det, ref, det.process([seqs[s][f] for s in range(S)]), ref.process([seqs[s][f] for s in range(S)]), f)
    bufs = [padded(seqs[s][3], stride, s) for s in range(S)]
    frames = [v for _, v in bufs]
    fp = (C.c_void_p * S)(*[b.ctypes.data for b, _ in bufs])
    res = (F.MotionResult * S)()
    reg = np.zeros((S, 32, 5), np.int32)
    two = np.int32([0, 0, 1])

    def unchanged():
        return all(np.array_equal(det.state(s)[0], ref.state(s)[0]) and np.array_equal(det.state(s)[1], ref.state(s)[1]) and det.state(s)[2] == ref.seen[s]
                   and np.array_equal(det.mask(s), ref.masks[s]) for s in range(S))

    def refused(code, fragment, call):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == code and fragment in e.value.msg, e.value
        assert unchanged(), "a refused call changed a model"

    raw = lambda *a: F.check(L.rtmodt_motion_process(det._h, *a))
    refused(F.E_INVALID, "created for", lambda: det.process([f[:, :69] for f in frames]))                   # another frame size
    refused(F.E_INVALID, "created for", lambda: det.process([f[:36] for f in frames]))
    refused(F.E_INVALID, "stride", lambda: raw(fp, None, S, h, w, 3 * w - 1, F.MEM_HOST, res, F.ptr(reg)))
    refused(F.E_INVALID, "mem_kind", lambda: raw(fp, None, S, h, w, stride, 2, res, F.ptr(reg)))
    refused(F.E_INVALID, "outside 0..2", lambda: det.process(frames[:2], [0, 3]))                          # a stream out of range
    refused(F.E_INVALID, "outside 0..2", lambda: det.process(frames[:2], [-1, 0]))
    refused(F.E_INVALID, "named twice", lambda: raw(fp, F.ptr(two), S, h, w, stride, F.MEM_HOST, res, F.ptr(reg)))
    refused(F.E_INVALID, "null argument", lambda: raw(None, None, S, h, w, stride, F.MEM_HOST, res, F.ptr(reg)))
    hole = (C.c_void_p * S)(bufs[0][0].ctypes.data, None, bufs[2][0].ctypes.data)
    refused(F.E_INVALID, "frame 1 is null", lambda: raw(hole, None, S, h, w, stride, F.MEM_HOST, res, F.ptr(reg)))
    four = (C.c_void_p * 4)(*([bufs[0][0].ctypes.data] * 4))
    refused(F.E_INVALID, "4 frames in one call for 3 streams", lambda: raw(four, F.ptr(np.int32([0, 1, 2, 0])), 4, h, w, stride, F.MEM_HOST, res, F.ptr(reg)))
    refused(F.E_INVALID, "no stream list", lambda: raw(fp, None, 2, h, w, stride, F.MEM_HOST, res, F.ptr(reg)))
    refused(F.E_INVALID, "outside 0..2", lambda: det.mask(3))
    refused(F.E_INVALID, "outside 0..2", lambda: det.blocks(-1))
    refused(F.E_INVALID, "outside 0..2", lambda: det.state(3))
    refused(F.E_INVALID, "outside 0..2", lambda: det.reset(3))
    refused(F.E_INVALID, "frames_seen", lambda: det.load_state(*ref.state(0)[:2], -1))
    refused(F.E_INVALID, "frames_seen", lambda: det.load_state(*ref.state(0)[:2], 2 ** 30 + 1))
    assert det.process([], []) == []
    with pytest.raises(ValueError):
        det.process(frames[:2])                                                 # two frames for three streams
    # the next accepted call goes on as if nothing had happened
    check(det, ref, det.process(frames), ref.process([seqs[s][3] for s in range(S)]), "after the refusals")
    assert det.last_kernel_ms() >= 0
    det.close()


# ---- the pipeline's motion stage ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_motion")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    yield det
    det.close()


class _Counting:
    """The detector with its detect() calls counted; everything else is the detector's."""

    def __init__(self, det):
        self._det, self.calls = det, []

    def detect(self, frame):
        self.calls.append(frame.copy())
        return self._det.detect(frame)

    def __getattr__(self, name):
        return getattr(self._det, name)


def pipeline_frames():
    """10 still frames, a bright square moving for 6, 14 still frames."""
    bgd = np.clip(MC.background(320, 320), 0, 255).astype(np.uint8)
    out = []
    for f in range(30):
        fr = bgd.copy()
        if 10 <= f < 16:
            x = 40 + 30 * (f - 10)
            fr[100:160, x:x + 60] = 230
        out.append(fr)
    return out


def test_pipeline_motion_stage(pkg, detector):
    frames = pipeline_frames()
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    ref = MR.Ref(1, 320, 320)
    statuses = [ref.step(0, f)["status"] for f in frames]
    assert statuses == [MR.WARMUP] * 8 + [MR.STILL] * 2 + [MR.MOTION] * 6 + [MR.STILL] * 14
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, pkg.MultiObjectTracker("bytetrack", track_thresh=0.05), prof(),
                            max_frames=30)
    for max_still in (5, 0, 25):
        predicted, run = [], 0                                                  # the frames whose detector pass is not skipped
        for f, st in enumerate(statuses):
            skip = st == MR.STILL and bool(predicted) and (max_still == 0 or run < max_still)
            run = run + 1 if skip else 0
            if not skip:
                predicted.append(f)
        if max_still == 5:
            assert predicted == list(range(8)) + list(range(10, 16)) + [21, 27]          # two forced refreshes in the 14 still frames
        det = _Counting(detector)
        trk = pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
        mo = pkg.MotionDetector(1, 320, 320, max_still=max_still)
        p = prof()
        out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), det, trk, p, max_frames=30, motion=mo,
                               heatmap=pkg.visualization.Heatmap(1, 320, 320, overlay_enabled=False))
        assert len(det.calls) == len(predicted) and all(np.array_equal(c, frames[f]) for c, f in zip(det.calls, predicted)), max_still
        assert (out["motion_frames"], out["still_frames"], out["scene_changes"]) == (6, 16, 0)
        rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
        assert rows(out) - rows(base) == {"motion_mean_ms", "heatmap_mean_ms"} and rows(base) <= rows(out)
        order = list(p.STAGE_ORDER)
        assert order.index("motion") == order.index("decode") + 1
        assert np.array_equal(mo.mask(), ref.masks[0]) and mo.state()[2] == ref.seen[0]
        mo.close()
    # motion=None: the parent's stage table and summary keys
    p = prof()
    none = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, pkg.MultiObjectTracker("bytetrack", track_thresh=0.05), p,
                            max_frames=30, motion=None)
    assert set(none) == set(base) and not {"motion_frames", "still_frames", "scene_changes"} & set(none)
    assert list(p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events",
                                                                                "visualization", "total"]
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"]
    # a scene change is counted: the light goes out
    mo = pkg.MotionDetector(1, 320, 320)
    dark = [frames[0]] * 10 + [frames[0] // 4] * 2
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(dark)), _Counting(detector), pkg.MultiObjectTracker("bytetrack", track_thresh=0.05), prof(),
                           max_frames=12, motion=mo)
    assert (out["motion_frames"], out["still_frames"], out["scene_changes"]) == (0, 2, 1)
    mo.close()
