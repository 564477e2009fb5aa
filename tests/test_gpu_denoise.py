"""GPU: the frame denoiser (``csrc/denoise.hip``) against ``tests/denoise_ref.py``: after every call of a 6-frame sequence on 3 streams
every output byte, every byte of padding and surround, the whole ``acc`` state and every result field equal the restatement (``==`` on
integers, nothing is tolerated) -- over the geometries of ``tests/denoise_cases.py`` (frames of one pixel, one row, one column, narrower
than a wave, wider and taller than a tile by one pixel, partial runs), every memory kind, padded rows whose padding stays untouched,
odd base addresses, named streams, ``spatial`` 0 / 128 / 256, ``temporal_shift`` 0 / 1 / 3 / 6 and two threshold pairs; every case's
run sees static pixels, moving pixels and pixels between the thresholds.  Then state / reset / load_state; two handles on one device;
every refusal with the handle usable afterwards; ``want_results=False``; the pipeline's ``denoise`` stage; and the dim moving box of the
noisy night scene through ``FrameDenoiser`` -> ``FrameEnhancer`` -> ``MotionDetector`` with the statuses the restatements gave.
PARITY UNPINNED: no other denoiser is compared."""
import os

import numpy as np
import pytest

import denoise_cases as DC
import denoise_ref as DR
import enhance_cases as EC
import enhance_ref as ER
import motion_ref as MR

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_STREAMS, N_FRAMES = DC.N_STREAMS, DC.N_FRAMES


def make(pkg, streams, h, w, cfg, **kw):
    c = DR.config(**cfg)
    dn = pkg.ingestion.FrameDenoiser(streams, h, w, motion=(c["motion_lo"], c["motion_hi"]), temporal_shift=c["temporal_shift"], spatial=c["spatial"],
                                     spatial_thr=c["spatial_thr"], **kw)
    return dn, DR.Ref(streams, h, w, **cfg)


def image(frames, pitch, offset):
    """The bytes of a buffer that holds `frames` one after another from `offset`, rows `pitch` apart, SENT everywhere else."""
    n, (h, w) = len(frames), frames[0].shape[:2]
    buf = np.full(offset + n * h * pitch + 8, SENT, np.uint8)
    for i, f in enumerate(frames):
        np.lib.stride_tricks.as_strided(buf[offset + i * h * pitch:], (h, w, 3), (pitch, 3, 1))[...] = f
    return buf


def same_state(dn, ref, tag=""):
    for s in range(ref.streams):
        got, want = dn.state(s), ref.state(s)
        assert got[1] == want[1] and got[0].dtype == np.uint16 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (tag, s)


def call(pkg, dn, ref, frames, streams=None, src="host", dst="host", spitch=None, dpitch=None, offset=0, want_results=True, tag=""):
    """One process call in the given memory kinds, pitches and base offset, compared with the restatement: every output byte, every byte
    around the pixels, the sources, the results and the state."""
    F = pkg._ffi
    n, (h, w) = len(frames), frames[0].shape[:2]
    spitch, dpitch = spitch or 3 * w, dpitch or 3 * w
    names = list(range(n)) if streams is None else list(streams)
    want = [ref.step(s, f) for s, f in zip(names, frames)]
    blank = [np.full((h, w, 3), 0x11, np.uint8)] * n
    kw = {}
    if src == "host":
        s_bufs = [EC.padded(f, spitch, SENT, offset) for f in frames]
        s_arg = [v for v, _ in s_bufs]
    else:
        s_arg = F.DeviceBuffer(offset + n * h * spitch + 8)
        s_arg.upload(image(frames, spitch, offset))
        kw.update(stride=spitch, offset=offset)
    if dst == "host":
        d_bufs = [EC.padded(b, dpitch, SENT, offset) for b in blank]
        d_arg = [v for v, _ in d_bufs]
    else:
        d_arg = F.DeviceBuffer(offset + n * h * dpitch + 8)
        d_arg.upload(image(blank, dpitch, offset))
        kw.update(out_stride=dpitch, out_offset=offset)
    res = dn.process(s_arg, d_arg, streams, want_results, **kw)
    outs = [o for o, _ in want]
    if dst == "host":                                                           # the arrays, pixels and padding
        for i, (_, buf) in enumerate(d_bufs):
            assert np.array_equal(buf, EC.padded(outs[i], dpitch, SENT, offset)[1]), (tag, i)
    else:
        assert np.array_equal(d_arg.download(), image(outs, dpitch, offset)), tag
    if src == "host":                                                           # the sources are as they were
        for i, (_, buf) in enumerate(s_bufs):
            assert np.array_equal(buf, EC.padded(frames[i], spitch, SENT, offset)[1]), (tag, i)
    else:
        assert np.array_equal(s_arg.download(), image(frames, spitch, offset)), tag
    if want_results:
        assert [r._asdict() for r in res] == [row for _, row in want], tag
        assert [r.noise_q8 for r in res] == [DR.noise_q8(row) for _, row in want]
    else:
        assert res is None
    same_state(dn, ref, tag)
    return outs


MODES = [("host", "host"), ("device", "device"), ("host", "device"), ("device", "host")]


# ---------------------------------------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("h,w,stride,v,seed", [pytest.param(*c, id=f"{c[0]}x{c[1]}p{c[2]}-v{c[3]}") for c in DC.sequence_cases()])
def test_sequences_equal_restatement(pkg, h, w, stride, v, seed):
    dn, ref = make(pkg, N_STREAMS, h, w, DC.VARIANTS[v])
    for f, frames in enumerate(DC.sequence(h, w, N_FRAMES, N_STREAMS, seed)):
        src, dst = MODES[(f + seed) % len(MODES)]
        call(pkg, dn, ref, frames, src=src, dst=dst, spitch=stride, dpitch=stride, tag=(f, src, dst))
    assert DC.saw_every_branch(ref.history) == (True, True, True)               # no case compares one branch only
    assert dn.kernel_ms() >= 0
    dn.close()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dst", ["host", "device"])
@pytest.mark.parametrize("src", ["host", "device"])
def test_memory_kinds_pitches_odd_bases_and_named_streams(pkg, src, dst, offset):
    """Every source / destination mix at a tight pitch, a padded odd pitch and a padded pitch of dwords (the wide path at offset 0, the
    byte path from an odd base), with streams=[2, 0]."""
    for n_case, (h, w, sp, dp) in enumerate(((37, 70, 210, 215), (36, 72, 220, 216), (19, 150, 452, 456), (17, 257, 771, 772))):
        dn, ref = make(pkg, N_STREAMS, h, w, DC.VARIANTS[(5 * n_case + 3 * offset + 2) % len(DC.VARIANTS)])
        for f, frames in enumerate(DC.sequence(h, w, 4, 2, 5300 + n_case)):
            streams = [[2, 0], [0, 1], [2, 0], [1, 2]][f]
            call(pkg, dn, ref, frames, streams=streams, src=src, dst=dst, spitch=sp, dpitch=dp, offset=offset, tag=(n_case, f))
        assert DC.saw_every_branch(ref.history) == (True, True, True)
        dn.close()


def test_full_hd_frames(pkg):
    """One 1080p stream at the defaults, two calls: every launch at the size the module is for."""
    h, w = 1080, 1920
    dn, ref = make(pkg, 1, h, w, {})
    for f, frames in enumerate(DC.sequence(h, w, 2, 1, 5400)):
        call(pkg, dn, ref, frames, src="device", dst="device", tag=f)
    assert DC.saw_every_branch(ref.history) == (True, True, True)
    dn.close()


# ---------------------------------------------------------------------------------------------------------------- state
def test_state_reset_load_state_continue_the_run(pkg):
    h, w = 37, 70
    cfg = DC.VARIANTS[10]
    a, ref = make(pkg, N_STREAMS, h, w, cfg)
    b, _ = make(pkg, N_STREAMS, h, w, cfg)
    seq = DC.sequence(h, w, 7, N_STREAMS, 5500)
    for frames in seq[:3]:
        call(pkg, a, ref, frames)
    saved = [a.state(s) for s in range(N_STREAMS)]
    assert saved[0][0].shape == (h, w, 3) and saved[0][1] == 3
    a.reset()
    assert all(a.state(s)[1] == 0 and not a.state(s)[0].any() for s in range(N_STREAMS))
    for s in range(N_STREAMS):
        a.load_state(s, saved[s])
        b.load_state(s, saved[s])                                              # and onto a second handle, whose planes were never written
    for frames in seq[3:6]:
        outs = call(pkg, a, ref, frames, dst="device")
        got = [np.empty_like(f) for f in frames]
        b.process(frames, got)
        assert all(np.array_equal(g, o) for g, o in zip(got, outs))
    a.reset(1)                                                                 # one stream back to fresh, the others as they were
    ref.reset(1)
    call(pkg, a, ref, seq[6])
    a.close(); b.close()


def test_two_handles_on_one_device_do_not_disturb_each_other(pkg):
    (h1, w1), (h2, w2) = (37, 70), (19, 150)
    a, ra = make(pkg, 2, h1, w1, DC.VARIANTS[2])
    b, rb = make(pkg, 2, h2, w2, DC.VARIANTS[22])
    for fa, fb in zip(DC.sequence(h1, w1, 4, 2, 5600), DC.sequence(h2, w2, 4, 2, 5601)):
        call(pkg, a, ra, fa, src="device", dst="device")
        call(pkg, b, rb, fb)
        same_state(a, ra, "after the other handle's call")
    a.close(); b.close()


def test_streams_not_named_keep_their_state(pkg):
    h, w = 20, 152
    dn, ref = make(pkg, N_STREAMS, h, w, {})
    seq = DC.sequence(h, w, 4, N_STREAMS, 5650)
    call(pkg, dn, ref, seq[0])
    before = dn.state(1)
    call(pkg, dn, ref, [seq[1][0], seq[1][2]], streams=[0, 2])
    call(pkg, dn, ref, [seq[2][2]], streams=[2])
    after = dn.state(1)
    assert after[1] == before[1] == 1 and np.array_equal(after[0], before[0])
    call(pkg, dn, ref, seq[3])                                                  # stream 1 goes on from its second frame
    dn.close()


def test_want_results_false_returns_nothing_and_the_state_moves(pkg):
    h, w = 70, 37
    dn, ref = make(pkg, 2, h, w, DC.VARIANTS[6])
    for f, frames in enumerate(DC.sequence(h, w, 3, 2, 5700)):
        call(pkg, dn, ref, frames, want_results=f == 2, dst=["host", "device", "host"][f], src=["host", "device", "device"][f])
    assert dn.process([], []) == [] and dn.process([], [], want_results=False) is None   # n = 0 is a no-op
    dn.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_handle_usable(pkg):
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    FD = pkg.ingestion.FrameDenoiser
    h, w = 37, 70
    for kw, word in ((dict(motion=(18, 18)), "motion_hi"), (dict(motion=(54, 18)), "motion_hi"), (dict(motion=(0, 2296)), "motion_hi"), (dict(motion=(-1, 5)), "motion_lo"),
                     (dict(spatial=257), "spatial"), (dict(spatial=-1), "spatial"), (dict(spatial_thr=256), "spatial_thr"), (dict(temporal_shift=7), "temporal_shift"),
                     (dict(temporal_shift=-1), "temporal_shift"), (dict(streams=0), "streams"), (dict(height=16385), "height"), (dict(width=0), "width")):
        with pytest.raises(E) as e:
            FD(**dict(dict(streams=1, height=h, width=w), **kw))
        assert e.value.code == F.E_INVALID and word in e.value.msg, e.value
    dn, ref = make(pkg, N_STREAMS, h, w, {})
    with pytest.raises(E) as e:
        dn.kernel_ms()
    assert e.value.code == F.E_INVALID and "no process call" in e.value.msg
    seq = iter(DC.sequence(h, w, 40, N_STREAMS, 5800))
    frames = next(seq)
    call(pkg, dn, ref, frames)

    def refused(code, fragment, fn):
        before = [dn.state(s) for s in range(N_STREAMS)]
        with pytest.raises(E) as e:
            fn()
        assert e.value.code == code and fragment in e.value.msg, e.value
        assert all(b[1] == dn.state(s)[1] and np.array_equal(b[0], dn.state(s)[0]) for s, b in enumerate(before)), fragment
        call(pkg, dn, ref, next(seq), tag=fragment)                             # usable afterwards, and equal to the restatement

    copies = lambda: [f.copy() for f in frames]                                  # noqa: E731
    blanks = lambda k=N_STREAMS: [np.zeros((h, w, 3), np.uint8) for _ in range(k)]   # noqa: E731
    refused(F.E_INVALID, "outside 0..2", lambda: dn.process(copies()[:2], blanks(2), streams=[0, 3]))
    refused(F.E_INVALID, "outside 0..2", lambda: dn.process(copies()[:2], blanks(2), streams=[-1, 0]))
    refused(F.E_INVALID, "named twice", lambda: dn.process(copies()[:2], blanks(2), streams=[1, 1]))
    refused(F.E_INVALID, "frames in one call", lambda: dn.process(copies() + copies()[:1], blanks(4)))
    refused(F.E_INVALID, "created for", lambda: dn.process([np.ascontiguousarray(f[:, :69]) for f in frames], [np.zeros((h, 69, 3), np.uint8) for _ in frames]))
    refused(F.E_INVALID, "output frames", lambda: dn.process(copies(), [np.zeros((h, w + 1, 3), np.uint8) for _ in frames]))
    nb = N_STREAMS * h * 3 * w
    dev, dev2 = F.DeviceBuffer(2 * nb), F.DeviceBuffer(2 * nb)
    dev.upload(np.concatenate([f.ravel() for f in frames]))
    refused(F.E_INVALID, "pitch", lambda: dn.process(dev, dev2, stride=3 * w - 1))
    refused(F.E_INVALID, "pitch", lambda: dn.process(dev, dev2, out_stride=3 * w - 1))
    # there is no in-place form: the destination on its source, one byte in, one frame on, the last byte, another pitch
    refused(F.E_INVALID, "overlaps", lambda: dn.process(dev, dev))
    refused(F.E_INVALID, "overlaps", lambda: dn.process(dev, dev, out_offset=1))
    refused(F.E_INVALID, "overlaps", lambda: dn.process(dev, dev, out_offset=h * 3 * w))
    refused(F.E_INVALID, "overlaps", lambda: dn.process(dev, dev, out_offset=nb - 1))
    refused(F.E_INVALID, "overlaps", lambda: dn.process(dev, dev, stride=3 * w + 4, out_stride=3 * w))
    same = copies()
    refused(F.E_INVALID, "overlaps", lambda: dn.process(same, same))
    big = np.zeros((h + 1, w, 3), np.uint8)
    refused(F.E_INVALID, "overlaps", lambda: dn.process([big[:h]], [big[1:]], streams=[0]))                 # host frames one row apart
    more = next(seq)
    dev.upload(np.concatenate([f.ravel() for f in more]))
    dn.process(dev, dev, out_offset=nb)                                         # directly behind the sources: allowed
    want = [ref.step(s, f)[0] for s, f in enumerate(more)]
    assert np.array_equal(dev.download(nb, nb), np.concatenate([x.ravel() for x in want]))
    assert np.array_equal(dev.download(nb, 0), np.concatenate([f.ravel() for f in more]))
    good = dn.state(0)
    refused(F.E_INVALID, "shape", lambda: dn.load_state(0, (good[0][:, :69], 1)))
    refused(F.E_INVALID, "shape", lambda: dn.load_state(0, (good[0].ravel(), 1)))
    over = good[0].copy()
    over[3, 4, 2] = 65281
    refused(F.E_INVALID, "above 255 << 8", lambda: dn.load_state(0, (over, 1)))
    refused(F.E_INVALID, "frames_seen", lambda: dn.load_state(0, (good[0], -1)))
    refused(F.E_INVALID, "outside 0..2", lambda: dn.load_state(3, good))
    refused(F.E_INVALID, "outside 0..2", lambda: dn.state(3))
    refused(F.E_INVALID, "outside 0..2", lambda: dn.reset(3))
    dn.close()


# ---------------------------------------------------------------------------------------------------------------- what it is for
def test_the_dim_box_is_still_seen_behind_denoiser_and_enhancer_on_the_device(pkg):
    """FrameDenoiser -> FrameEnhancer -> MotionDetector on device frames of the noisy night scene (+-4, lift 8), with the statuses the
    restatements gave (tests/test_denoise_cpu.py holds the premise: the same statuses as without the filter)."""
    F = pkg._ffi
    h, w = EC.NIGHT_H, EC.NIGHT_W
    frames, _, boxes = DC.noisy_night(4, EC.BOX_LIFT)
    dn, en, md = pkg.ingestion.FrameDenoiser(1, h, w), pkg.ingestion.FrameEnhancer(1, h, w), pkg.MotionDetector(1, h, w)
    ref_dn, ref_en, ref_md = DR.Ref(1, h, w), ER.Ref(1, h, w), MR.Ref(1, h, w)
    src, clean, out = F.DeviceBuffer(h * 3 * w), F.DeviceBuffer(h * 3 * w), F.DeviceBuffer(h * 3 * w)
    got, want = [], []
    for f in frames:
        src.upload(f.ravel())
        dn.process(src, clean, want_results=False)                             # device frames in, device frames out ...
        en.process(clean, out, want_results=False)
        got.append(md.process(out)[0].status)                                  # ... which the next module takes where they lie
        enhanced = ref_en.step(0, ref_dn.step(0, f)[0])[0]
        want.append(ref_md.step(0, enhanced)["status"])
    assert np.array_equal(out.download().reshape(h, w, 3), enhanced)
    assert got == want
    assert [s for s, b in zip(got, boxes) if b is not None] == [MR.MOTION] * DC.NIGHT_MOVING
    for x in (dn, en, md):
        x.close()


# ---------------------------------------------------------------------------------------------------------------- the pipeline's denoise stage
@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_denoise")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    yield det
    det.close()


class SeesFrames:
    """The detector, keeping what it was handed."""

    def __init__(self, det):
        self.det, self.seen = det, []

    def detect(self, frame):
        self.seen.append(np.array(frame))
        return self.det.detect(frame)

    def __getattr__(self, name):
        return getattr(self.det, name)


def test_pipeline_denoise_stage(pkg, detector):
    frames = [f[0] for f in DC.sequence(320, 320, 8, 1, 5900)]
    n = len(frames)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)       # noqa: E731
    tracker = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)                               # noqa: E731
    source = lambda: pkg.pipeline.SyntheticSource(np.stack(frames))                                        # noqa: E731
    FD, FE = pkg.ingestion.FrameDenoiser, pkg.ingestion.FrameEnhancer
    base = pkg.pipeline.run(source(), detector, tracker(), prof(), max_frames=n)
    # alone: where enhance would stand, and the detector sees the restatement's frames
    ref = DR.Ref(1, 320, 320)
    rows = [ref.step(0, f) for f in frames]
    p, det = prof(), SeesFrames(detector)
    alone = pkg.pipeline.run(source(), det, tracker(), p, max_frames=n, denoise=FD(1, 320, 320))
    assert list(p.STAGE_ORDER)[:3] == ["decode", "denoise", "preprocess"]
    assert alone["denoise_mean_noise_q8"] == sum(DR.noise_q8(r) for _, r in rows) / n and alone["denoise_mean_noise_q8"] > 0
    assert det.seen and all(any(np.array_equal(s, o) for o, _ in rows) for s in det.seen) and np.array_equal(det.seen[0], rows[0][0])
    added = set(alone) - set(base)
    assert set(base) <= set(alone) and "denoise_mean_noise_q8" in added and all(k.startswith("denoise_") for k in added)
    # with enhance: directly before it, and the enhancer works on the filtered frames
    ref_en = ER.Ref(1, 320, 320)
    enhanced = [ref_en.step(0, o)[0] for o, _ in rows]
    p, det = prof(), SeesFrames(detector)
    both = pkg.pipeline.run(source(), det, tracker(), p, max_frames=n, denoise=FD(1, 320, 320), enhance=FE(1, 320, 320),
                            health=pkg.ingestion.CameraHealth(1, 320, 320), motion=pkg.MotionDetector(1, 320, 320, max_still=0, warmup=4))
    assert list(p.STAGE_ORDER)[:5] == ["decode", "health", "denoise", "enhance", "motion"]
    assert {"denoise_mean_noise_q8", "enhance_mean_eff"} <= set(both) and both["denoise_mean_noise_q8"] == alone["denoise_mean_noise_q8"]
    assert det.seen and all(any(np.array_equal(s, e) for e in enhanced) for s in det.seen)
    p = prof()
    lens = pkg.ingestion.LensCorrector(1, (320, 320))
    lens.set_model(0, (64.0, 64.0, 159.5, 159.5), [0, 0, 0, 0])
    pkg.pipeline.run(source(), detector, tracker(), p, max_frames=n, denoise=FD(1, 320, 320), lens=lens, stabilize=pkg.ingestion.Stabilizer(1, (320, 320)),
                     enhance=FE(1, 320, 320), motion=pkg.MotionDetector(1, 320, 320))
    assert list(p.STAGE_ORDER)[:6] == ["decode", "undistort", "stabilize", "denoise", "enhance", "motion"]
    p = prof()
    pkg.pipeline.run(source(), detector, tracker(), p, max_frames=n, denoise=FD(1, 320, 320), stabilize=pkg.ingestion.Stabilizer(1, (320, 320)),
                     motion=pkg.MotionDetector(1, 320, 320))
    assert list(p.STAGE_ORDER)[:4] == ["decode", "stabilize", "denoise", "motion"]
    # denoise=None: the parent's stage table and summary keys
    p = prof()
    none = pkg.pipeline.run(source(), detector, tracker(), p, max_frames=n, denoise=None)
    assert set(none) == set(base) and not any(k.startswith("denoise") for k in none)
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"] and none["events"] == base["events"]
    assert list(p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events",
                                                                                "visualization", "total"]
