"""GPU: the stabiliser (``csrc/stab.hip``) against ``tests/stab_ref.py``: after every call of a sequence every output byte, every path
(as bit patterns), every status, HOLD run and coefficient equals the restatement (``==`` on integers, nothing is tolerated); exact
copies; every memory kind, padded rows whose padding stays untouched, odd base addresses, an enlarging crop; every refusal with the
state left as it was; ``state`` / ``load_state`` onto a second handle; the estimator form against the supplied form fed with what
``rtmodt_gmc_result`` returns; the hand-over of stabilised device frames to the motion detector with the shaking-camera case of
``tests/stab_cases.py`` (whose premise ``tests/test_stab_cpu.py`` establishes on the restatements); the pipeline's ``stabilize`` stage.
Shapes: ``stab_cases.SHAPES``.  Content is random bytes, the worst case for a wrong weight or tap.  PARITY UNPINNED: vidstab, OpenCV's
videostab and warpAffine are not compared."""
import itertools
import os

import numpy as np
import pytest

import gmc_ref as G
import motion_ref as M
import stab_cases as SC
import stab_ref as S
from lens_cases import random_frames

pytestmark = pytest.mark.gpu


def stabilizer(pkg, streams, size, **kw):
    return pkg.ingestion.Stabilizer(streams, size, border=SC.BORDER, **kw)


# ---------------------------------------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_sequences_equal_restatement(pkg, name):
    size = SC.SHAPES[name]
    st, ref = stabilizer(pkg, SC.N_STREAMS, size, **SC.CFG), S.Ref(SC.N_STREAMS, size, SC.BORDER, **SC.CFG)
    SC.same_state(st, ref, "fresh")
    seen = set()
    for k, (warps, valid) in enumerate(SC.schedule()):
        frames = random_frames(SC.N_STREAMS, size, 100 * size[1] + k)
        got, want = st.process(frames, warps, valid), ref.process(frames, warps, valid)
        for s in range(SC.N_STREAMS):
            assert got[s].shape == size + (3,) and np.array_equal(got[s], want[s]), (k, s)
        SC.same_state(st, ref, k)
        seen |= set(ref.status)
    assert seen == {S.OK, S.HOLD, S.CLAMPED, S.RESET}
    assert st.last_ms() >= 0
    st.reset(1)                                                               # one stream back to fresh, the others as they were
    ref.reset(1)
    SC.same_state(st, ref, "reset 1")
    st.reset()
    ref.reset()
    SC.same_state(st, ref, "reset all")
    st.close()


def test_streams_are_named_and_no_warp_is_the_identity(pkg):
    size = SC.SHAPES["37x23"]
    st, ref = stabilizer(pkg, 3, size, **SC.CFG), S.Ref(3, size, SC.BORDER, **SC.CFG)
    frames = random_frames(2, size, 9)
    w = np.stack([SC.warp(0.2, 1.0, 2.5, -1.5), SC.warp(-0.3, 1.001, -4.0, 0.25)])
    for streams in ([2, 0], [1, 2], [0, 1]):
        got, want = st.process(frames, w, streams=streams), ref.process(frames, w, streams=streams)
        assert all(np.array_equal(g, x) for g, x in zip(got, want))
        SC.same_state(st, ref, streams)
    got, want = st.process(frames), ref.process(frames)                       # no warps: the identity, the paths decay
    assert all(np.array_equal(g, x) for g, x in zip(got, want))
    SC.same_state(st, ref, "identity")
    st.close()


# ---------------------------------------------------------------------------------------------------------------- exact copies
def test_identity_copies_and_integer_translation_shifts(pkg):
    size = SC.SHAPES["131x77"]
    h, w = size
    st = stabilizer(pkg, 1, size, leak_shift=0, max_shift_px=16)
    frame = random_frames(1, size, 5)[0]
    assert np.array_equal(st.process([frame])[0], frame)
    assert np.array_equal(st.process([frame], np.float32([[1, 0, 0, 0, 1, 0]]))[0], frame)
    out = st.process([frame], np.float32([[1, 0, 5, 0, 1, -3]]))[0]            # the camera moved: the content is found 5 right and 3 up
    want = np.empty_like(frame)
    want[...] = SC.BORDER
    want[3:, :w - 5] = frame[:h - 3, 5:]
    assert np.array_equal(out, want)
    r = st.result()[0]
    assert r.path == (1.0, 0.0, 5.0, -3.0) and r.coef == (65536, 0, 5 * 65536, -3 * 65536) and r.status == S.OK
    assert np.array_equal(st.process([frame], np.float32([[1, 0, -5, 0, 1, 3]]))[0], frame)     # and back: no decay, the copy again
    assert np.array_equal(st.to_source([[10.0, 20.0]]), [[10.0, 20.0]])
    st.close()


# ---------------------------------------------------------------------------------------------------------------- memory, pitch, alignment
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dst_kind", ["host", "device"])
@pytest.mark.parametrize("src_kind", ["host", "device"])
def test_memory_kinds_pitches_odd_bases_and_crop(pkg, src_kind, dst_kind, offset):
    sched = SC.schedule()
    for name, dextra, crop in (("37x23", 7, 1000), ("37x23", 9, 1100), ("131x77", 7, 1250), ("523x9", 3, 1000)):    # dst pitches 118 (never wide), 120, 400, 1572 (wide at offset 0)
        size = SC.SHAPES[name]
        cfg = dict(SC.CFG, crop_zoom_milli=crop)
        st, ref = stabilizer(pkg, 3, size, **cfg), S.Ref(3, size, SC.BORDER, **cfg)
        for k in range(3):
            frames = random_frames(3, size, 7 * k + dextra)
            warps, valid, streams = sched[k + 2][0][:3], sched[k + 2][1][:3], [2, 0, 1]
            got = SC.run(st, pkg, frames, warps=warps, valid=valid, streams=streams, src_kind=src_kind, dst_kind=dst_kind, spitch=3 * size[1] + 5,
                         dpitch=3 * size[1] + dextra, offset=offset)
            want = ref.process(frames, warps, valid, streams)
            for i in range(3):
                assert np.array_equal(got[i], want[i]), (name, dextra, k, i)
            SC.same_state(st, ref, (name, k))
        st.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_state(pkg):
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    size = SC.SHAPES["37x23"]
    h, w = size
    for kw, word in ((dict(streams=0, size=size), "streams"), (dict(streams=1025, size=size), "streams"), (dict(streams=1, size=(0, 4)), "outside 1..16384"),
                     (dict(streams=1, size=(4, 16385)), "outside 1..16384"), (dict(streams=1, size=size, leak_shift=17), "bad parameter"),
                     (dict(streams=1, size=size, crop_zoom_milli=999), "bad parameter")):
        with pytest.raises(E) as e:
            pkg.ingestion.Stabilizer(**kw)
        assert e.value.code == F.E_INVALID and word in e.value.msg, e.value
    st, ref = stabilizer(pkg, 3, size, **SC.CFG), S.Ref(3, size, SC.BORDER, **SC.CFG)
    with pytest.raises(E) as e:
        st.last_ms()
    assert e.value.code == F.E_INVALID and "no process call" in e.value.msg
    sched = SC.schedule()
    frames = random_frames(3, size, 33)
    calls = itertools.count()                                                 # the schedule, round and round

    def advance():                                                            # one valid call more, equal to the restatement
        k = next(calls) % len(sched)
        got, want = st.process(frames, sched[k][0][:3], sched[k][1][:3]), ref.process(frames, sched[k][0][:3], sched[k][1][:3])
        assert all(np.array_equal(g, x) for g, x in zip(got, want)), k
        SC.same_state(st, ref, k)

    def refused(code, fragment, call):
        before = st.result()
        with pytest.raises(E) as e:
            call()
        assert e.value.code == code and fragment in e.value.msg, e.value
        assert st.result() == before, fragment                                # (floats compare by value here; same_state below compares their bits)
        SC.same_state(st, ref, fragment)
        advance()

    advance()
    good = sched[0][0][:3]
    refused(F.E_INVALID, "outside 0..2", lambda: st.process(frames[:2], good[:2], streams=[0, 3]))
    refused(F.E_INVALID, "outside 0..2", lambda: st.process(frames[:2], good[:2], streams=[-1, 0]))
    refused(F.E_INVALID, "named twice", lambda: st.process(frames[:2], good[:2], streams=[1, 1]))
    refused(F.E_CAPACITY, "frames in one call", lambda: st.process(frames + frames[:1], np.concatenate([good, good[:1]]), streams=[0, 1, 2, 0]))
    refused(F.E_INVALID, "created for", lambda: st.process([f[:, :36] for f in frames], good))
    refused(F.E_INVALID, "created for", lambda: st.process(frames, good, out=[np.zeros((h, w + 1, 3), np.uint8) for _ in frames]))
    for bad in (np.nan, np.inf):
        wbad = good.copy()
        wbad[1, 2] = bad
        refused(F.E_INVALID, "warp 1", lambda: st.process(frames, wbad))
    wbad = good.copy()
    wbad[2] = [1e-4, 0, 0, 0, 1e-4, 0]                                        # det = 1e-8
    refused(F.E_INVALID, "warp 2", lambda: st.process(frames, wbad))
    dev, dev2 = F.DeviceBuffer(6 * h * 3 * w), F.DeviceBuffer(6 * h * 3 * w)
    dev.upload(np.concatenate([f.ravel() for f in frames]))
    refused(F.E_INVALID, "pitch", lambda: st.process(dev, good, out=dev2, stride=3 * w - 1))
    refused(F.E_INVALID, "pitch", lambda: st.process(dev, good, out=dev2, out_stride=3 * w - 1))
    # a gather cannot work in place: the same frames, a destination that begins on a source's last byte, a source that begins in the destination
    refused(F.E_INVALID, "overlaps", lambda: st.process(dev, good, out=dev))
    refused(F.E_INVALID, "overlaps", lambda: st.process(dev, good, out=dev, out_offset=3 * h * 3 * w - 1))
    refused(F.E_INVALID, "overlaps", lambda: st.process(frames, good, out=frames))
    k = next(calls) % len(sched)
    got = st.process(dev, sched[k][0][:3], sched[k][1][:3], out=dev, out_offset=3 * h * 3 * w)           # directly behind the sources: allowed
    want = ref.process(frames, sched[k][0][:3], sched[k][1][:3])
    assert np.array_equal(got.download(3 * h * 3 * w, 3 * h * 3 * w), np.concatenate([x.ravel() for x in want]))
    SC.same_state(st, ref, "behind")
    refused(F.E_INVALID, "outside the handle's limits", lambda: st.load_state(0, (1.0, 0.0, 12.5, 0.0)))
    refused(F.E_INVALID, "outside the handle's limits", lambda: st.load_state(0, (1.0, np.nan, 0.0, 0.0)))
    refused(F.E_INVALID, "hold run", lambda: st.load_state(0, S.IDENTITY, -1))
    refused(F.E_INVALID, "outside 0..2", lambda: st.state(3))
    refused(F.E_INVALID, "outside 0..2", lambda: st.reset(3))
    assert st.process([], None) == []                                         # n = 0 is a no-op
    # the estimator's own refusals: fewer estimator streams than frames, a frame below its smallest, a size other than the one it has seen
    E1 = pkg.tracking.gmc.CameraMotionEstimator(n_streams=2, **SC.EST_CFG)
    st.gmc = E1
    refused(F.E_INVALID, "estimator streams", lambda: st.process(frames))
    refused(F.E_INVALID, "smallest accepted", lambda: st.process(frames[:2]))
    big = stabilizer(pkg, 2, SC.EST_SIZE, gmc=E1)
    big.process(SC.est_frames()[:2])                                          # the estimator has now seen 112 x 96 frames
    E2 = pkg.tracking.gmc.CameraMotionEstimator(n_streams=2, downscale=1, coarse_search=0, min_blocks=2, min_inliers=2)
    E2.estimate(SC.est_frames()[:2])
    small = stabilizer(pkg, 2, (32, 48), gmc=E2)
    with pytest.raises(E) as e:
        small.process(random_frames(2, (32, 48), 1))
    assert e.value.code == F.E_INVALID and "frame size changed" in e.value.msg and [r.path for r in small.result()] == [S.IDENTITY] * 2
    if F.device_count() > 1:                                                  # an estimator on another device (needs a second one to make it)
        other = pkg.tracking.gmc.CameraMotionEstimator(n_streams=2, device=1, **SC.EST_CFG)
        st.gmc = other
        refused(F.E_INVALID, "estimator on device", lambda: st.process(frames[:2]))
        other.close()
    st.gmc = None
    advance()
    for x in (big, small, st):
        x.close()
    E1.close(); E2.close()


# ---------------------------------------------------------------------------------------------------------------- state
def test_state_continues_on_a_second_handle(pkg):
    size = SC.SHAPES["131x77"]
    a, ref = stabilizer(pkg, SC.N_STREAMS, size, **SC.CFG), S.Ref(SC.N_STREAMS, size, SC.BORDER, **SC.CFG)
    sched = SC.schedule()
    frames = random_frames(SC.N_STREAMS, size, 61)
    for k in range(5):                                                        # stream 2 is in the middle of its HOLD run
        a.process(frames, *sched[k])
        ref.process(frames, *sched[k])
    assert ref.hold[2] == 2
    b = stabilizer(pkg, SC.N_STREAMS, size, **SC.CFG)
    for s in range(SC.N_STREAMS):
        path, hold = a.state(s)
        assert np.array_equal(path.view(np.uint64), np.float64(ref.path[s]).view(np.uint64)) and hold == ref.hold[s]
        b.load_state(s, path, hold)
    for k in range(5, SC.N_CALLS):
        got, want = b.process(frames, *sched[k]), ref.process(frames, *sched[k])
        assert all(np.array_equal(g, x) for g, x in zip(got, want)), k
        SC.same_state(b, ref, k)
        assert all(np.array_equal(g, x) for g, x in zip(a.process(frames, *sched[k]), want)), k
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- the estimator form
def test_estimator_form_equals_supplied_form(pkg):
    size, CME = SC.EST_SIZE, pkg.tracking.gmc.CameraMotionEstimator
    seqs = [SC.est_frames(17), SC.est_frames(18)]
    est = CME(n_streams=3, **SC.EST_CFG)                                      # one stream more than frames: the estimate runs on streams 0 and 1
    a, b = stabilizer(pkg, 2, size, gmc=est, **SC.EST_STAB), stabilizer(pkg, 2, size, **SC.EST_STAB)
    ref = S.Ref(2, size, SC.BORDER, **SC.EST_STAB)
    m = SC.est_interior()
    dev, out = pkg._ffi.DeviceBuffer(2 * size[0] * 3 * size[1]), pkg._ffi.DeviceBuffer(2 * size[0] * 3 * size[1])
    for k in range(len(seqs[0]) + 1):
        flat = k == len(seqs[0])
        frames = [np.full(size + (3,), 128, np.uint8)] * 2 if flat else [q[k] for q in seqs]       # a flat frame has too few blocks
        if k % 2:                                                             # host frames and device frames alike
            dev.upload(np.concatenate([f.ravel() for f in frames]))
            assert a.process(dev, out=out) is out
            got = list(out.download().reshape((2,) + size + (3,)))
        else:
            got = a.process(frames)
        warp, status = est.result()
        want_status = G.FIRST if k == 0 else G.FEW_BLOCKS if flat else G.OK
        assert list(status[:2]) == [want_status] * 2, (k, status)
        if 0 < k and not flat:
            sx, sy = SC.EST_STEPS[k - 1]
            assert np.array_equal(warp[:2].reshape(2, 6), np.float32([[1, 0, -sx, 0, 1, -sy]] * 2))
        fed = b.process(frames, warp[:2], [s == 0 for s in status[:2]])
        want = ref.process(frames, warp[:2], [s == 0 for s in status[:2]])
        for s in range(2):
            assert np.array_equal(got[s], fed[s]) and np.array_equal(got[s], want[s]), (k, s)
            if not flat:                                                      # no decay and exact translations: the first frame, except the band that left it
                assert np.array_equal(got[s][m:-m, m:-m], seqs[s][0][m:-m, m:-m]), (k, s)
        SC.same_state(a, ref, k)
        SC.same_state(b, ref, k)
        assert [r.status for r in a.result()] == [S.OK if want_status == G.OK else S.HOLD] * 2
        assert est.last_ms() >= 0 and a.last_ms() >= 0
    own = stabilizer(pkg, 1, (480, 640), gmc=True)                            # gmc=True: an estimator with its defaults (downscale 4)
    f = G.pan_sequence(480, 640, 3, [(4, -4)], margin=16)
    own.process([f[0]])
    assert own.result()[0].status == S.HOLD and own.gmc.result()[1][0] == G.FIRST
    own.process([f[1]])
    warp, status = own.gmc.result()
    r, rule = own.result()[0], S.Rule(480, 640)
    path, hold, st1 = S.step(rule, S.IDENTITY, 0, None, False)
    path, hold, st2 = S.step(rule, path, hold, warp[0], status[0] == 0)
    assert status[0] == G.OK and (r.status, r.hold) == (st2, hold) == (S.OK, 0) and r.path == path and r.coef == S.quantise(rule, path), (r, path)
    assert abs(path[2] + 4.0) < 0.25 and abs(path[3] - 4.0) < 0.25            # the content moved by (-4, +4)
    assert np.allclose(own.to_stable(own.to_source([[100.0, 50.0]])), [[100.0, 50.0]], atol=1e-9)
    for x in (a, b, own):
        x.close()
    est.close()


def test_mask_boxes_reach_the_estimator(pkg):
    """Host mask boxes stay optional in the estimator form: with them the stabiliser's estimator answers as one that is called directly."""
    from gmc_cases import Boxes
    size, CME = SC.EST_SIZE, pkg.tracking.gmc.CameraMotionEstimator
    frames = SC.est_frames()
    inner, alone = CME(**SC.EST_CFG), CME(**SC.EST_CFG)
    st = stabilizer(pkg, 1, size, gmc=inner, **SC.EST_STAB)
    boxes = Boxes(np.float32([[40, 40, 50, 50], [0, 0, 3, 3]]), np.float32([0.9, 0.05]))      # four interior blocks; the second is below mask_conf
    for k, f in enumerate(frames[:3]):
        masks = [boxes] if k != 1 else None
        st.process([f], masks=masks)
        warp, status = alone.estimate([f], masks)
        got_warp, got_status = inner.result()
        assert np.array_equal(got_warp.view(np.uint32), warp.view(np.uint32)) and np.array_equal(got_status, status), k
        a, b = inner.debug(0), alone.debug(0)
        assert all(np.array_equal(a["blk"][n], b["blk"][n]) for n in a["blk"]), k
        if k == 2:
            assert int((a["blk"]["reason"] == G.R_MASK).sum()) >= 1 and status[0] == G.OK
    st.close(); inner.close(); alone.close()


# ---------------------------------------------------------------------------------------------------------------- hand-over
def test_stabilised_device_frames_close_the_motion_gate(pkg):
    F = pkg._ffi
    h, w = SC.GATE_SIZE
    frames, warps = SC.gate_frames(), SC.gate_warps()
    st, ref = pkg.ingestion.Stabilizer(1, SC.GATE_SIZE, **SC.GATE_STAB), S.Ref(1, SC.GATE_SIZE, **SC.GATE_STAB)
    on_raw, on_stab = pkg.MotionDetector(1, h, w, **SC.GATE_MOTION), pkg.MotionDetector(1, h, w, **SC.GATE_MOTION)
    ref_raw, ref_stab = M.Ref(1, h, w, **SC.GATE_MOTION), M.Ref(1, h, w, **SC.GATE_MOTION)
    src = F.DeviceBuffer(h * 3 * w)
    raw, stab = [], []
    for f, wp in zip(frames, warps):
        src.upload(f.ravel())
        out = st.process(src, wp.reshape(1, 6))                               # device frames in, a device buffer out
        assert isinstance(out, F.DeviceBuffer)
        want = ref.process([f], wp.reshape(1, 6))[0]
        assert np.array_equal(out.download().reshape(h, w, 3), want)
        a, b = on_raw.process([f])[0], on_stab.process(out)[0]                # ... which the motion detector takes where it lies
        assert a.status == ref_raw.process([f])[0]["status"] and b.status == ref_stab.process([want])[0]["status"]
        raw.append(a.status)
        stab.append(b.status)
    warm = SC.GATE_MOTION["warmup"]
    assert M.MOTION in raw[warm:] and stab[warm:] == [M.STILL] * (len(frames) - warm), (raw, stab)
    for x in (st, on_raw, on_stab):
        x.close()


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


def test_pipeline_stabilize_stage(pkg, tmp_path):
    path = os.path.join(str(tmp_path), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    detector = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    size, frames = SC.EST_SIZE, SC.est_frames()
    n = len(frames)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    tracker = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    base_p = prof()
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), base_p, max_frames=n)
    est = pkg.tracking.gmc.CameraMotionEstimator(**SC.EST_CFG)
    st = pkg.ingestion.Stabilizer(1, size, gmc=est, **SC.EST_STAB)
    lens = pkg.ingestion.LensCorrector(1, size)
    lens.set_model(0, (64.0, 64.0, (size[1] - 1) / 2, (size[0] - 1) / 2), [0, 0, 0, 0])                   # the identity lens: an undistort row, the same pixels
    det, rec, p = _Counting(detector), _Recorder(), prof()
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), det, tracker(), p, max_frames=n, stabilize=st, lens=lens, recorder=rec,
                           motion=pkg.MotionDetector(1, size[0], size[1], max_still=0, warmup=100))
    ref = S.Ref(1, size, **SC.EST_STAB)
    want = [ref.process([f], np.float32([[1, 0, -sx, 0, 1, -sy]]), [k > 0])[0] for k, (f, (sx, sy)) in enumerate(zip(frames, [(0, 0)] + SC.EST_STEPS))]
    assert len(det.calls) == n and all(np.array_equal(c, x) for c, x in zip(det.calls, want))             # the detector's input is the stabilised frame
    assert len(rec.frames) == n and all(np.array_equal(c, x) for c, x in zip(rec.frames, want))
    assert (out["stabilize_holds"], out["stabilize_clamped"], out["stabilize_resets"]) == (1, 0, 0)       # the estimator's first frame
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"undistort_mean_ms", "stabilize_mean_ms", "motion_mean_ms"} and rows(base) <= rows(out)
    order = list(p.STAGE_ORDER)
    assert order.index("stabilize") == order.index("undistort") + 1 and order.index("motion") == order.index("stabilize") + 1
    p = prof()                                                                # without a lens: directly after decode
    pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=n, stabilize=pkg.ingestion.Stabilizer(1, size))
    order = list(p.STAGE_ORDER)
    assert order.index("stabilize") == order.index("decode") + 1 and order.index("stabilize") < order.index("preprocess")
    # stabilize=None: the parent's stage table and summary keys
    p = prof()
    none = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=n, stabilize=None)
    assert set(none) == set(base) and "stabilize_mean_ms" not in none and "stabilize_holds" not in none
    assert list(p.STAGE_ORDER) == list(base_p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking",
                                                                                                           "events", "visualization", "total"]
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"]
    st.close(); est.close(); lens.close()
    detector.close()
