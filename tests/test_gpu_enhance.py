"""GPU: the frame enhancer (``csrc/enhance.hip``) against ``tests/enhance_ref.py``: after every call of a 6-frame sequence on 3 streams
every output byte, the call's histograms, the whole state and every result field equal the restatement (``==`` on integers, nothing is
tolerated) -- over the geometries and tile grids of ``tests/enhance_cases.py`` (runs that straddle tile boundaries, tiles narrower than
a run, frames narrower than a wave and wider than a workgroup row, row slabs that merge into one histogram, an apply workgroup over
many tile rows), every memory kind, in place, padded rows whose padding stays untouched, odd base addresses, named streams, both colour
rules, three clip limits, ``auto`` on and off; state / reset / load_state; two handles on one device; every refusal with the handle usable
afterwards; ``want_results=False``; the pipeline's ``enhance`` stage; and the dim moving box of ``enhance_cases`` through
``FrameEnhancer`` -> ``MotionDetector`` with the statuses the restatements gave.  PARITY UNPINNED: ``cv2.createCLAHE`` is not compared."""
import os

import numpy as np
import pytest

import enhance_cases as EC
import enhance_ref as ER
import motion_ref as MR

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_STREAMS, N_FRAMES = 3, 6
#: per case index: colour, clip_q8, auto -- every value of each meets every geometry and grid somewhere
VARIANTS = [dict(colour=c, clip_q8=q, auto_lo=a[0], auto_hi=a[1]) for c in (ER.SHIFT, ER.GAIN) for q in EC.CLIP_Q8 for a in ((0, 0), (60, 140))]


def make(pkg, streams, h, w, grid, cfg, **kw):
    en = pkg.ingestion.FrameEnhancer(streams, h, w, tiles=grid, clip_limit=cfg["clip_q8"] / 256, strength=cfg.get("strength", 256),
                                     smooth_shift=cfg.get("smooth_shift", 2), auto=(cfg["auto_lo"], cfg["auto_hi"]), colour=cfg["colour"], **kw)
    ref = ER.Ref(streams, h, w, tiles_y=grid[0], tiles_x=grid[1], **cfg)
    return en, ref


def image(frames, pitch, offset):
    """The bytes of a buffer that holds `frames` one after another from `offset`, rows `pitch` apart, SENT everywhere else."""
    n, (h, w) = len(frames), frames[0].shape[:2]
    buf = np.full(offset + n * h * pitch + 8, SENT, np.uint8)
    for i, f in enumerate(frames):
        np.lib.stride_tricks.as_strided(buf[offset + i * h * pitch:], (h, w, 3), (pitch, 3, 1))[...] = f
    return buf


def same_state(en, ref, streams, tag=""):
    for s in range(ref.streams):
        got, want = en.state(s), ref.state(s)
        assert got[1] == want[1] and got[0].dtype == np.uint16 and np.array_equal(got[0], want[0]), (tag, s)
    for s in streams:
        assert np.array_equal(en.histograms(s), ref.hist[s]), (tag, s)


def call(pkg, en, ref, frames, streams=None, src="host", dst="inplace", spitch=None, dpitch=None, offset=0, want_results=True, tag=""):
    """One process call in the given memory kinds, pitches and base offset, compared with the restatement: every output byte, every byte
    around the pixels, the results, the histograms and the state."""
    F = pkg._ffi
    n, (h, w) = len(frames), frames[0].shape[:2]
    spitch, dpitch = spitch or 3 * w, dpitch or 3 * w
    names = list(range(n)) if streams is None else list(streams)
    want = [ref.step(s, f) for s, f in zip(names, frames)]
    blank = [np.full((h, w, 3), 0x11, np.uint8)] * n
    if src == "host":
        s_bufs = [EC.padded(f, spitch, SENT, offset) for f in frames]
        s_arg, kw = [v for v, _ in s_bufs], {}
    else:
        s_arg = F.DeviceBuffer(offset + n * h * spitch + 8)
        s_arg.upload(image(frames, spitch, offset))
        kw = dict(stride=spitch, offset=offset)
    if dst == "inplace":
        d_arg, dpitch = None, spitch
    elif dst == "host":
        d_bufs = [EC.padded(b, dpitch, SENT, offset) for b in blank]
        d_arg = [v for v, _ in d_bufs]
    else:
        d_arg = F.DeviceBuffer(offset + n * h * dpitch + 8)
        d_arg.upload(image(blank, dpitch, offset))
        kw.update(out_stride=dpitch, out_offset=offset)
    res = en.process(s_arg, d_arg, streams, want_results, **kw)
    outs = [o for o, _ in want]
    where = (dst, src) if dst == "inplace" else (dst,)
    if where[-1] == "host":                                                   # destinations in host memory: the arrays, pixels and padding
        for i, (_, buf) in enumerate(s_bufs if dst == "inplace" else d_bufs):
            assert np.array_equal(buf, EC.padded(outs[i], dpitch, SENT, offset)[1]), (tag, i)
    else:
        assert np.array_equal((s_arg if dst == "inplace" else d_arg).download(), image(outs, dpitch, offset)), tag
    if dst != "inplace":                                                      # the sources are as they were
        if src == "host":
            for i, (_, buf) in enumerate(s_bufs):
                assert np.array_equal(buf, EC.padded(frames[i], spitch, SENT, offset)[1]), (tag, i)
        else:
            assert np.array_equal(s_arg.download(), image(frames, spitch, offset)), tag
    if want_results:
        assert [r._asdict() for r in res] == [row for _, row in want], tag
    else:
        assert res is None
    same_state(en, ref, names, tag)
    return outs


def cases():
    out = []
    for g, (h, w, stride) in enumerate(EC.GEOMETRIES + EC.WIDE_GEOMETRIES):
        for grid in EC.GRIDS:
            if EC.fits(grid, h, w):
                out.append(pytest.param(h, w, stride, grid, len(out), id=f"{h}x{w}p{stride}-{grid[0]}x{grid[1]}"))
    return out


# ---------------------------------------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("h,w,stride,grid,k", cases())
def test_sequences_equal_restatement(pkg, h, w, stride, grid, k):
    cfg = VARIANTS[k % len(VARIANTS)]
    en, ref = make(pkg, N_STREAMS, h, w, grid, cfg)
    seq = EC.sequence(h, w, N_FRAMES, N_STREAMS, 4200 + k)
    modes = [("host", "inplace"), ("device", "device"), ("host", "host"), ("device", "inplace"), ("host", "device"), ("device", "host")]
    for f, frames in enumerate(seq):
        src, dst = modes[(f + k) % len(modes)]
        call(pkg, en, ref, frames, src=src, dst=dst, spitch=stride, dpitch=stride, tag=(f, src, dst))
    assert en.kernel_ms() >= 0
    en.close()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dst", ["host", "device", "inplace"])
@pytest.mark.parametrize("src", ["host", "device"])
def test_memory_kinds_pitches_odd_bases_and_named_streams(pkg, src, dst, offset):
    """Every source / destination mix at a tight pitch, a padded odd pitch and a padded pitch of dwords (the wide path at offset 0, the
    byte path from an odd base), with streams=[2, 0]."""
    for n_case, (h, w, grid, sp, dp) in enumerate(((37, 70, (8, 8), 210, 215), (36, 72, (2, 3), 220, 216), (19, 150, (16, 16), 452, 456), (70, 37, (16, 16), 111, 112))):
        for colour in (ER.SHIFT, ER.GAIN):
            cfg = dict(VARIANTS[(3 * n_case + offset) % len(VARIANTS)], colour=colour)
            en, ref = make(pkg, N_STREAMS, h, w, grid, cfg)
            seq = EC.sequence(h, w, 3, 2, 4300 + n_case)
            for f, frames in enumerate(seq):
                streams = [[2, 0], [0, 1], [2, 0]][f]
                call(pkg, en, ref, frames, streams=streams, src=src, dst=dst, spitch=sp, dpitch=dp, offset=offset, tag=(n_case, f))
            en.close()


def test_full_hd_frame_and_a_night_frame(pkg):
    """One 1080p call at the defaults (every launch at the size the module is for) and a frame with every pixel inside 16 levels."""
    h, w = 1080, 1920
    rng = np.random.default_rng(4400)
    cfg = dict(VARIANTS[2])
    en, ref = make(pkg, 1, h, w, (8, 8), cfg)
    night = np.clip(rng.integers(20, 36, (h, w, 1)) + np.zeros((1, 1, 3), np.int64), 0, 255).astype(np.uint8)
    call(pkg, en, ref, [night], src="device", dst="device")
    call(pkg, en, ref, [EC.content("uniform", h, w, rng)], src="device", dst="inplace")
    en.close()


# ---------------------------------------------------------------------------------------------------------------- state
def test_state_reset_load_state_continue_the_run(pkg):
    h, w, grid = 37, 70, (2, 3)
    cfg = VARIANTS[2]
    a, ref = make(pkg, N_STREAMS, h, w, grid, cfg)
    b, _ = make(pkg, N_STREAMS, h, w, grid, cfg)
    seq = EC.sequence(h, w, 6, N_STREAMS, 4500)
    for frames in seq[:3]:
        call(pkg, a, ref, frames)
    saved = [a.state(s) for s in range(N_STREAMS)]
    assert saved[0][0].shape == (2, 3, 256) and saved[0][1] == 3
    a.reset()
    assert all(a.state(s)[1] == 0 and not a.state(s)[0].any() for s in range(N_STREAMS))
    for s in range(N_STREAMS):
        a.load_state(s, saved[s])
        b.load_state(s, saved[s])                                              # and onto a second handle
    for frames in seq[3:]:
        outs = call(pkg, a, ref, frames, dst="host")
        got = [np.empty_like(f) for f in frames]
        b.process(frames, got)
        assert all(np.array_equal(g, o) for g, o in zip(got, outs))
    a.reset(1)                                                                 # one stream back to fresh, the others as they were
    ref.reset(1)
    call(pkg, a, ref, seq[0])
    a.close(); b.close()


def test_two_handles_on_one_device_do_not_disturb_each_other(pkg):
    (h1, w1, g1), (h2, w2, g2) = (37, 70, (8, 8)), (19, 150, (2, 3))
    a, ra = make(pkg, 2, h1, w1, g1, VARIANTS[1])
    b, rb = make(pkg, 2, h2, w2, g2, VARIANTS[8])
    sa, sb = EC.sequence(h1, w1, 4, 2, 4600), EC.sequence(h2, w2, 4, 2, 4601)
    for fa, fb in zip(sa, sb):
        call(pkg, a, ra, fa, src="device", dst="device")
        call(pkg, b, rb, fb)
        same_state(a, ra, [0, 1], "after the other handle's call")
    a.close(); b.close()


def test_want_results_false_returns_nothing_and_the_state_moves(pkg):
    h, w, grid = 70, 37, (8, 8)
    en, ref = make(pkg, 2, h, w, grid, VARIANTS[5])
    for f, frames in enumerate(EC.sequence(h, w, 3, 2, 4700)):
        call(pkg, en, ref, frames, want_results=f == 2, dst=["inplace", "device", "host"][f], src=["host", "device", "host"][f])
    assert en.process([]) == [] and en.process([], want_results=False) is None   # n = 0 is a no-op
    en.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_handle_usable(pkg):
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    FE = pkg.ingestion.FrameEnhancer
    h, w, grid = 37, 70, (8, 8)
    for kw, word in ((dict(tiles=(0, 8)), "tiles"), (dict(tiles=(8, 17)), "tiles"), (dict(tiles=(16, 16), height=15), "tiles"), (dict(tiles=(4, 9), width=8), "tiles"),
                     (dict(strength=257), "strength"), (dict(strength=-1), "strength"), (dict(smooth_shift=8), "smooth_shift"), (dict(colour="sepia"), "colour"),
                     (dict(colour=2), "colour"), (dict(auto=(10, 9)), "auto"), (dict(auto=(0, 256)), "auto"), (dict(streams=0), "streams"), (dict(height=16385), "height")):
        with pytest.raises(E) as e:
            FE(**dict(dict(streams=1, height=h, width=w), **kw))
        assert e.value.code == F.E_INVALID and word in e.value.msg, e.value
    en, ref = make(pkg, N_STREAMS, h, w, grid, VARIANTS[2])
    with pytest.raises(E) as e:
        en.kernel_ms()
    assert e.value.code == F.E_INVALID and "no process call" in e.value.msg
    with pytest.raises(E) as e:
        en.histograms(0)
    assert e.value.code == F.E_INVALID and "last process call" in e.value.msg
    seq = iter(EC.sequence(h, w, 40, N_STREAMS, 4800))
    frames = next(seq)
    call(pkg, en, ref, frames)

    def refused(code, fragment, fn):
        before = [en.state(s) for s in range(N_STREAMS)]
        with pytest.raises(E) as e:
            fn()
        assert e.value.code == code and fragment in e.value.msg, e.value
        assert all(b[1] == en.state(s)[1] and np.array_equal(b[0], en.state(s)[0]) for s, b in enumerate(before)), fragment
        call(pkg, en, ref, next(seq), tag=fragment)                             # usable afterwards, and equal to the restatement

    copies = lambda: [f.copy() for f in frames]                                  # noqa: E731
    refused(F.E_INVALID, "outside 0..2", lambda: en.process(copies()[:2], streams=[0, 3]))
    refused(F.E_INVALID, "outside 0..2", lambda: en.process(copies()[:2], streams=[-1, 0]))
    refused(F.E_INVALID, "named twice", lambda: en.process(copies()[:2], streams=[1, 1]))
    refused(F.E_INVALID, "frames in one call", lambda: en.process(copies() + copies()[:1]))
    refused(F.E_INVALID, "created for", lambda: en.process([np.ascontiguousarray(f[:, :69]) for f in frames]))
    refused(F.E_INVALID, "output frames", lambda: en.process(copies(), [np.zeros((h, w + 1, 3), np.uint8) for _ in frames]))
    nb = N_STREAMS * h * 3 * w
    dev, dev2 = F.DeviceBuffer(2 * nb), F.DeviceBuffer(2 * nb)
    dev.upload(np.concatenate([f.ravel() for f in frames]))
    refused(F.E_INVALID, "pitch", lambda: en.process(dev, dev2, stride=3 * w - 1))
    refused(F.E_INVALID, "pitch", lambda: en.process(dev, dev2, out_stride=3 * w - 1))
    # in place is allowed; every other meeting of a destination with a source is not: one byte in, one frame on, the last byte
    refused(F.E_INVALID, "overlaps", lambda: en.process(dev, dev, out_offset=1))
    refused(F.E_INVALID, "overlaps", lambda: en.process(dev, dev, out_offset=h * 3 * w))
    refused(F.E_INVALID, "overlaps", lambda: en.process(dev, dev, out_offset=nb - 1))
    refused(F.E_INVALID, "overlaps", lambda: en.process(dev, dev, stride=3 * w + 4, out_stride=3 * w))     # the same base at another pitch
    big = np.zeros((h + 1, w, 3), np.uint8)
    refused(F.E_INVALID, "overlaps", lambda: en.process([big[:h]], [big[1:]], streams=[0]))                 # host frames one row apart
    more = next(seq)
    dev.upload(np.concatenate([f.ravel() for f in more]))
    en.process(dev, dev, out_offset=nb)                                         # directly behind the sources: allowed
    want = [ref.step(s, f)[0] for s, f in enumerate(more)]
    assert np.array_equal(dev.download(nb, nb), np.concatenate([x.ravel() for x in want]))
    assert np.array_equal(dev.download(nb, 0), np.concatenate([f.ravel() for f in more]))
    good = en.state(0)
    refused(F.E_INVALID, "shape", lambda: en.load_state(0, (good[0][:, :7], 1)))
    refused(F.E_INVALID, "shape", lambda: en.load_state(0, (good[0].ravel(), 1)))
    over = good[0].copy()
    over[3, 4, 5] = 65281
    refused(F.E_INVALID, "above 255 << 8", lambda: en.load_state(0, (over, 1)))
    refused(F.E_INVALID, "frames_seen", lambda: en.load_state(0, (good[0], -1)))
    refused(F.E_INVALID, "outside 0..2", lambda: en.load_state(3, good))
    refused(F.E_INVALID, "outside 0..2", lambda: en.state(3))
    refused(F.E_INVALID, "outside 0..2", lambda: en.reset(3))
    refused(F.E_INVALID, "outside 0..2", lambda: en.histograms(3))
    call(pkg, en, ref, next(seq)[:2], streams=[2, 0])
    with pytest.raises(E) as e:
        en.histograms(1)                                                        # the last call did not name stream 1
    assert e.value.code == F.E_INVALID
    en.close()


# ---------------------------------------------------------------------------------------------------------------- what it is for
def test_a_dim_box_is_seen_behind_the_enhancer_on_the_device(pkg):
    """FrameEnhancer -> MotionDetector on device frames, with the statuses the restatements gave (tests/test_enhance_cpu.py holds the
    premise: raw the scene is STILL throughout)."""
    F = pkg._ffi
    h, w = EC.NIGHT_H, EC.NIGHT_W
    frames, moving = EC.night_sequence(True)
    en, md, raw = pkg.ingestion.FrameEnhancer(1, h, w), pkg.MotionDetector(1, h, w), pkg.MotionDetector(1, h, w)
    ref_en, ref_md, ref_raw = ER.Ref(1, h, w), MR.Ref(1, h, w), MR.Ref(1, h, w)
    src, out = F.DeviceBuffer(h * 3 * w), F.DeviceBuffer(h * 3 * w)
    got, got_raw, want, want_raw = [], [], [], []
    for f in frames:
        src.upload(f.ravel())
        en.process(src, out, want_results=False)                               # device frames in, device frames out ...
        got.append(md.process(out)[0].status)                                  # ... which the motion detector takes where they lie
        got_raw.append(raw.process(src)[0].status)
        enhanced = ref_en.step(0, f)[0]
        want.append(ref_md.step(0, enhanced)["status"])
        want_raw.append(ref_raw.step(0, f)["status"])
    assert np.array_equal(out.download().reshape(h, w, 3), enhanced)
    warm = MR.DEFAULTS["warmup"]
    assert got == want and got_raw == want_raw == [MR.WARMUP] * warm + [MR.STILL] * (len(frames) - warm)
    assert [s for s, m in zip(got, moving) if m] == [MR.MOTION] * EC.NIGHT_MOVING and [s for s, m in zip(got[warm:], moving[warm:]) if not m] == [MR.STILL] * (EC.NIGHT_WARM - warm)
    for x in (en, md, raw):
        x.close()


# ---------------------------------------------------------------------------------------------------------------- the pipeline's enhance stage
@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_enhance")), "yolov8n_320.rtw")
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


def test_pipeline_enhance_stage(pkg, detector):
    rng = np.random.default_rng(4900)
    frames = [EC.content("night", 320, 320, rng) for _ in range(8)]
    n = len(frames)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)       # noqa: E731
    tracker = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)                               # noqa: E731
    source = lambda: pkg.pipeline.SyntheticSource(np.stack(frames))                                        # noqa: E731
    base = pkg.pipeline.run(source(), detector, tracker(), prof(), max_frames=n)
    ref = ER.Ref(1, 320, 320, auto_lo=60, auto_hi=140)
    rows = [ref.step(0, f) for f in frames]
    p, det = prof(), SeesFrames(detector)
    out = pkg.pipeline.run(source(), det, tracker(), p, max_frames=n, enhance=pkg.ingestion.FrameEnhancer(1, 320, 320, auto=(60, 140)),
                           health=pkg.ingestion.CameraHealth(1, 320, 320), motion=pkg.MotionDetector(1, 320, 320, max_still=0, warmup=4))
    order = list(p.STAGE_ORDER)
    assert order[:4] == ["decode", "health", "enhance", "motion"]
    assert out["enhance_mean_eff"] == sum(r["eff"] for _, r in rows) / n and 0 < out["enhance_mean_eff"] <= 256
    assert det.seen and all(any(np.array_equal(s, o) for o, _ in rows) for s in det.seen)                     # the detector saw the restatement's frames
    assert np.array_equal(det.seen[0], rows[0][0])
    p = prof()
    lens = pkg.ingestion.LensCorrector(1, (320, 320))
    lens.set_model(0, (64.0, 64.0, 159.5, 159.5), [0, 0, 0, 0])
    pkg.pipeline.run(source(), detector, tracker(), p, max_frames=n, enhance=pkg.ingestion.FrameEnhancer(1, 320, 320), lens=lens,
                     stabilize=pkg.ingestion.Stabilizer(1, (320, 320)), motion=pkg.MotionDetector(1, 320, 320))
    assert list(p.STAGE_ORDER)[:5] == ["decode", "undistort", "stabilize", "enhance", "motion"]
    p = prof()
    alone = pkg.pipeline.run(source(), detector, tracker(), p, max_frames=n, enhance=pkg.ingestion.FrameEnhancer(1, 320, 320))
    assert list(p.STAGE_ORDER)[:3] == ["decode", "enhance", "preprocess"]
    added = set(alone) - set(base)
    assert set(base) <= set(alone) and "enhance_mean_eff" in added and all(k.startswith("enhance_") for k in added) and alone["enhance_mean_eff"] == 256
    # enhance=None: the parent's stage table and summary keys
    p = prof()
    none = pkg.pipeline.run(source(), detector, tracker(), p, max_frames=n, enhance=None)
    assert set(none) == set(base) and not any(k.startswith("enhance") for k in none)
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"] and none["events"] == base["events"]
    assert list(p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events",
                                                                                "visualization", "total"]
