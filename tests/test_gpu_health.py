"""GPU: the camera-health monitor (csrc/health.hip, csrc/health_rule.h) against the NumPy restatement tests/health_ref.py: after every
call every result field, every event and everything a stream holds (R, the previous luma grid, ref_sharp, the counters, the masks)
are the restatement's; the interface's behaviour and refusals; the pipeline's health stage.  Every comparison is == on integers.
PARITY UNPINNED: the reference has no counterpart and no default has been validated on real footage."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import health_cases as HC
import health_ref as HR
from test_gpu_motion import DeviceFrames, padded

pytestmark = pytest.mark.gpu

#: (h, w, stride): partial edge cells in both directions, odd pitches; 150 x 530 spans several tiles in x and y at every scale;
#: 5 x 9 has no interior cell at scale 4 / 8 (and at scale 2 fewer reference edges than min_ref_edges): NO_STRUCTURE
GEOMETRIES = [(37, 70, 211), (70, 37, 117), (19, 150, 452), (150, 530, 1601), (5, 9, 29)]
SCALES = [1, 2, 4, 8]
FIELDS = ("stream", "raw", "active", "frames_seen", "ref_sharp", "learned") + HR.COUNTS
STATE = ("ref_sharp", "frames_seen", "active", "pending", "run", "off")
D, B, CV, MV, DF, FZ = range(6)
UP, DOWN, REBASED = HR.RAISED, HR.CLEARED, HR.REBASED
#: what stream 0 of the 150 x 530 sequence answers per scale under HC.TIMERS, as (frame, condition, kind): covered from frame 6,
#: blurred from 18, shifted from 27, dark from 36, bright from 41, repeated from 49.  At scale 1 the texture itself is structure that a
#: shifted copy keeps by chance, at scale 8 the few coarse cells do: no MOVED there.
COMMON_HEAD = [(8, CV, UP), (15, CV, DOWN), (20, DF, UP), (24, DF, DOWN)]
COMMON_TAIL = [(38, D, UP), (38, CV, UP), (42, D, DOWN), (43, B, UP), (47, B, DOWN), (47, CV, DOWN), (51, FZ, UP)]
MOVED = [(29, MV, UP), (33, MV, DOWN)]
EVENTS = {1: COMMON_HEAD + COMMON_TAIL, 2: COMMON_HEAD + MOVED + COMMON_TAIL, 4: COMMON_HEAD + MOVED + COMMON_TAIL, 8: COMMON_HEAD + COMMON_TAIL}
#: the same with relearn_frames = 4: the cover, latched on frame 8, rebases the stream on frame 12 and the covered picture becomes the
#: reference, which has no structure to lose (at scale 2 its noise has: MOVED); so does the dark picture on frame 42
RELEARN_TAIL = [(38, D, UP), (38, CV, UP), (42, D, DOWN), (42, CV, DOWN), (42, -1, REBASED), (51, FZ, UP)]
RELEARN = {s: [(8, CV, UP), (12, CV, DOWN), (12, -1, REBASED)] + (MOVED if s == 2 else []) + RELEARN_TAIL for s in SCALES}


def as_dict(r):
    d = {k: getattr(r, k) for k in FIELDS}
    d["events"] = [(e.condition, e.kind, e.frame_id) for e in r.events]
    return d


def same_state(got, want):
    return np.array_equal(got.r, want["r"]) and np.array_equal(got.prev, want["prev"]) and all(getattr(got, k) == want[k] for k in STATE)


def check(mon, ref, got, want, what):
    """One call's results and everything a stream holds afterwards against the restatement."""
    assert len(got) == len(want), what
    for g, w_ in zip(got, want):
        gd = as_dict(g)
        for k in FIELDS + ("events",):
            assert gd[k] == w_[k], (what, k, gd[k], w_[k])
        assert g.names == HR.names_of(w_["active"]) and g.mean_luma == w_["luma_sum"] / (ref.gh * ref.gw), what
        s = w_["stream"]
        st, rs = mon.state(s), ref.state(s)
        assert np.array_equal(st.r, rs["r"]), (what, "R", s)
        assert np.array_equal(st.prev, rs["prev"]), (what, "previous Y", s)
        assert {k: getattr(st, k) for k in STATE} == {k: rs[k] for k in STATE}, (what, "state", s)


@functools.lru_cache(maxsize=None)
def sequences(h, w, streams):
    return [HC.sequence(h, w, 100 * h + s)[0] for s in range(streams)]


# ---- the sequence over geometries and scales ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("h,w,stride", GEOMETRIES)
def test_sequence_equals_restatement(pkg, h, w, stride, scale):
    """Host frames at the odd pitch; device frames at the same pitch from a base offset by 1 (the byte path); device frames at
    the pitch rounded up to a multiple of 4 from a base offset by 4 (the wide path): one restatement for the three.  A fourth
    monitor, on host frames, runs with relearn_frames = 4 against a restatement of its own."""
    S = 2 if h * w > 20000 else 3
    seqs = sequences(h, w, S)
    cfg = dict(HC.TIMERS, scale=scale)
    ref, ref4 = HR.Ref(S, h, w, **cfg), HR.Ref(S, h, w, relearn_frames=4, **cfg)
    wide_stride = (stride + 3) // 4 * 4
    mons = [pkg.ingestion.CameraHealth(S, h, w, **cfg) for _ in range(3)] + [pkg.ingestion.CameraHealth(S, h, w, relearn_frames=4, **cfg)]
    dev1, dev4 = DeviceFrames(pkg, S, h, stride, 1), DeviceFrames(pkg, S, h, wide_stride, 4)
    events, events4, flags = [], [], 0
    for f in range(HC.N_FRAMES):
        frames = [seqs[s][f] for s in range(S)]
        want, want4 = ref.process(frames), ref4.process(frames)
        events += [(f, c_, k) for c_, k, fid in want[0]["events"] if fid == f]
        events4 += [(f, c_, k) for c_, k, fid in want4[0]["events"] if fid == f]
        flags |= want[0]["raw"]
        keep = [padded(fr, stride, f * 7 + s) for s, fr in enumerate(frames)]
        check(mons[0], ref, mons[0].process([v for _, v in keep]), want, ("host", f))
        check(mons[1], ref, mons[1].process(dev1.put(frames, f), stride=stride, offset=1), want, ("device + 1", f))
        check(mons[2], ref, mons[2].process(dev4.put(frames, f), stride=wide_stride, offset=4), want, ("device + 4", f))
        check(mons[3], ref4, mons[3].process([v for _, v in keep]), want4, ("relearn", f))
    assert all(m.last_kernel_ms() >= 0 for m in mons)
    if (h, w) == (150, 530):
        # asserted on the restatement, so that equality cannot hide an empty comparison
        assert events == EVENTS[scale] and events4 == RELEARN[scale]
    if (h, w) == (5, 9) and scale >= 2:
        assert flags & HR.NO_STRUCTURE and not any(c_ in (CV, MV, DF) for _, c_, _ in events)
    else:
        assert not flags & HR.NO_STRUCTURE
    for m in mons:
        m.close()
    dev1.buf.free(); dev4.buf.free()


# ---- interface ---------------------------------------------------------------------------------------------------------
def test_stream_lists_state_round_trip_rebase_and_reset(pkg):
    h, w, stride, S = 37, 70, 211, 4
    seqs = [HC.sequence(h, w, 900 + s)[0] for s in range(S)]
    cfg = dict(HC.TIMERS, scale=2)
    ref, mon = HR.Ref(S, h, w, **cfg), pkg.ingestion.CameraHealth(S, h, w, **cfg)
    clock = [0] * S                                                             # each stream advances through its own sequence

    def go(streams, ids=None):
        frames = []
        for s in streams:
            frames.append(seqs[s][clock[s] % HC.N_FRAMES])
            clock[s] += 1
        before = {s: mon.state(s) for s in range(S) if s not in streams}
        want = ref.process(frames, streams, ids)
        got = mon.process([padded(f, stride, 5)[1] for f in frames], streams, ids)
        check(mon, ref, got, want, streams)
        for s, st in before.items():                                            # untouched streams keep their state bit for bit
            now = mon.state(s)
            assert np.array_equal(now.r, st.r) and np.array_equal(now.prev, st.prev) and all(getattr(now, k) == getattr(st, k) for k in STATE), (streams, s)
        return want
    for streams in ([0, 1, 2, 3], [3, 1, 0, 2], [2], [1, 3], [3, 0], [0, 1, 2, 3], [2, 1], [1], [1], [1], [3, 2, 1, 0], [0, 2], [1, 2, 3]):
        go(streams)
    for _ in range(3):                                                          # stream 1 alone, further into its covered stretch (frames 10..12 of its own clock)
        go([1])
    assert ref.st[1]["active"] == 1 << CV and len({st["frames_seen"] for st in ref.st}) > 1
    assert go([3, 1], [1000, 2000])[1]["events"] == [] and ref.frame_no[1] == 2001                   # the caller's frame ids
    # a monitor survives a restart: a second handle loaded with stream 1's state goes on exactly as the first
    again = pkg.ingestion.CameraHealth(1, h, w, **cfg)
    again.load_state(mon.state(1))
    seen_events = []
    for _ in range(8):
        frame = seqs[1][clock[1] % HC.N_FRAMES]
        clock[1] += 1
        a, b = mon.process([frame], [1], [clock[1]])[0], again.process([frame], None, [clock[1]])[0]
        ref.process([frame], [1], [clock[1]])
        da, db = as_dict(a), as_dict(b)
        assert {k: da[k] for k in da if k != "stream"} == {k: db[k] for k in db if k != "stream"}
        sa, sb = mon.state(1), again.state(0)
        assert np.array_equal(sa.r, sb.r) and np.array_equal(sa.prev, sb.prev) and all(getattr(sa, k) == getattr(sb, k) for k in STATE)
        seen_events += da["events"]
    assert (CV, DOWN) in [(c_, k) for c_, k, _ in seen_events] and same_state(mon.state(1), ref.state(1))
    # rebase: stream 2 into its cover, then the operator's word; the next call reports CLEARED and REBASED first and starts a new reference
    while ref.st[2]["active"] != 1 << CV:
        go([2])
    mon.rebase(2); ref.rebase(2)
    assert same_state(mon.state(2), ref.state(2)) and mon.state(2).pending == HR.PENDING_REBASE | 1 << CV and mon.state(2).frames_seen == 0
    want = go([2, 0])
    assert [e[:2] for e in want[0]["events"]] == [(CV, DOWN), (-1, REBASED)] and want[0]["learned"] == HR.LEARN_SET and ref.st[2]["pending"] == 0
    mon.rebase(3); ref.rebase(3)                                                # nothing active: REBASED alone
    assert [e[:2] for e in go([3])[0]["events"]] == [(-1, REBASED)]
    # reset: one stream, then all
    mon.reset(2); ref.reset(2); ref.frame_no[2] = 0
    st = mon.state(2)
    assert (st.frames_seen, st.active, st.pending, st.ref_sharp) == (0, 0, 0, 0) and not st.r.any() and not st.prev.any() and mon.state(1).frames_seen == ref.st[1]["frames_seen"] > 0
    assert go([2, 1])[0]["n_changed"] == ref.gh * ref.gw and ref.st[2]["frames_seen"] == 1
    mon.reset(); ref.reset(); ref.frame_no = [0] * S
    assert all(mon.state(s).frames_seen == 0 and not mon.state(s).r.any() for s in range(S))
    go([0, 1, 2, 3])
    with pytest.raises(ValueError):
        bad = mon.state(0)
        bad.r = np.zeros((3, 3), np.uint16)
        mon.load_state(bad)
    mon.close(); again.close()


def test_refusals(pkg):
    h, w, stride, S = 37, 70, 211, 3
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    L = F.lib()
    fresh = pkg.ingestion.CameraHealth(S, h, w)
    with pytest.raises(E) as e:
        fresh.last_kernel_ms()                                                  # nothing has launched yet
    assert e.value.code == F.E_INVALID and "no process call" in e.value.msg
    fresh.close()
    cfg = dict(HC.TIMERS, warmup=2)
    mon, ref = pkg.ingestion.CameraHealth(S, h, w, **cfg), HR.Ref(S, h, w, **cfg)
    seqs = [HC.sequence(h, w, 40 + s)[0] for s in range(S)]
    for f in range(3):
        check(mon, ref, mon.process([seqs[s][f] for s in range(S)]), ref.process([seqs[s][f] for s in range(S)]), f)
    bufs = [padded(seqs[s][3], stride, s) for s in range(S)]
    frames = [v for _, v in bufs]
    fp = (C.c_void_p * S)(*[b.ctypes.data for b, _ in bufs])
    res = (F.HealthResult * S)()
    ev = (F.HealthEvent * (S * 8))()
    two = np.int32([0, 0, 1])

    def unchanged():
        return all(same_state(mon.state(s), ref.state(s)) for s in range(S))

    def refused(code, fragment, call):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == code and fragment in e.value.msg, e.value
        assert unchanged(), "a refused call changed a stream"

    raw = lambda *a: F.check(L.rtmodt_health_process(mon._h, *a))               # noqa: E731
    refused(F.E_INVALID, "created for", lambda: mon.process([f[:, :69] for f in frames]))                   # another frame size
    refused(F.E_INVALID, "created for", lambda: mon.process([f[:36] for f in frames]))
    refused(F.E_INVALID, "stride", lambda: raw(fp, None, None, S, h, w, 3 * w - 1, F.MEM_HOST, res, ev))
    refused(F.E_INVALID, "mem_kind", lambda: raw(fp, None, None, S, h, w, stride, 2, res, ev))
    refused(F.E_INVALID, "outside 0..2", lambda: mon.process(frames[:2], [0, 3]))                          # a stream out of range
    refused(F.E_INVALID, "outside 0..2", lambda: mon.process(frames[:2], [-1, 0]))
    refused(F.E_INVALID, "named twice", lambda: raw(fp, F.ptr(two), None, S, h, w, stride, F.MEM_HOST, res, ev))
    refused(F.E_INVALID, "null argument", lambda: raw(None, None, None, S, h, w, stride, F.MEM_HOST, res, ev))
    hole = (C.c_void_p * S)(bufs[0][0].ctypes.data, None, bufs[2][0].ctypes.data)
    refused(F.E_INVALID, "frame 1 is null", lambda: raw(hole, None, None, S, h, w, stride, F.MEM_HOST, res, ev))
    four = (C.c_void_p * 4)(*([bufs[0][0].ctypes.data] * 4))
    refused(F.E_INVALID, "4 frames in one call for 3 streams", lambda: raw(four, F.ptr(np.int32([0, 1, 2, 0])), None, 4, h, w, stride, F.MEM_HOST, res, ev))
    refused(F.E_INVALID, "no stream list", lambda: raw(fp, None, None, 2, h, w, stride, F.MEM_HOST, res, ev))
    refused(F.E_INVALID, "outside 0..2", lambda: mon.state(3))
    refused(F.E_INVALID, "outside 0..2", lambda: mon.reset(3))
    refused(F.E_INVALID, "outside 0..2", lambda: mon.rebase(-1))
    good = mon.state(0)
    for field, value in (("frames_seen", -1), ("frames_seen", 2 ** 30 + 1), ("active", 64), ("pending", 4), ("pending", 256), ("run", (0, 0, 0, 0, 0, -1))):
        bad = mon.state(0)                                                      # (pending 256 with frames_seen 3: owed events behind no rebase)
        setattr(bad, field, value)
        refused(F.E_INVALID, "health state", lambda: mon.load_state(bad))
    bad = mon.state(0)
    bad.r = bad.r.copy()
    bad.r[1, 1] = 65281
    refused(F.E_INVALID, "above 255 << 8", lambda: mon.load_state(bad))
    assert same_state(mon.state(0), ref.state(0)) and good.frames_seen == 3
    assert mon.process([], []) == []
    with pytest.raises(ValueError):
        mon.process(frames[:2])                                                 # two frames for three streams
    with pytest.raises(ValueError):
        mon.process(frames, frame_ids=[1, 2])
    # the next accepted call goes on as if nothing had happened
    check(mon, ref, mon.process(frames), ref.process([seqs[s][3] for s in range(S)]), "after the refusals")
    assert mon.last_kernel_ms() >= 0
    mon.close()


# ---- the pipeline's health stage ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_health")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    yield det
    det.close()


def test_pipeline_health_stage(pkg, detector):
    """10 healthy frames, 8 covered ones, 6 healthy ones: one alarm, COVERED in the flags, nothing else changed."""
    frames, _ = HC.sequence(320, 320, 11, (("healthy", 10), ("covered", 8), ("healthy", 6)))
    n = len(frames)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)       # noqa: E731
    tracker = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)                               # noqa: E731
    ref = HR.Ref(1, 320, 320, **HC.TIMERS)
    rows = [ref.step(0, f, i + 1) for i, f in enumerate(frames)]                # SyntheticSource numbers its frames from 1
    events = [e for r in rows for e in r["events"]]
    assert events == [(CV, UP, 13), (CV, DOWN, 20)]
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), prof(), max_frames=n)
    mon = pkg.ingestion.CameraHealth(1, 320, 320, **HC.TIMERS)
    p = prof()
    lens = pkg.ingestion.LensCorrector(1, (320, 320))
    lens.set_model(0, (64.0, 64.0, 159.5, 159.5), [0, 0, 0, 0])                  # the identity lens: an undistort row, the same pixels
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=n, health=mon,
                           motion=pkg.MotionDetector(1, 320, 320, max_still=1), lens=lens)
    assert (out["health_alarms"], out["health_flags"]) == (1, 1 << CV)
    order = list(p.STAGE_ORDER)
    assert order.index("health") == order.index("decode") + 1 and order.index("undistort") == order.index("health") + 1 and "motion" in order
    assert same_state(mon.state(0), ref.state(0))                              # the stage saw the delivered frames, with the source's frame ids
    p = prof()
    alone = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=n, health=pkg.ingestion.CameraHealth(1, 320, 320, **HC.TIMERS))
    added = set(alone) - set(base)
    assert set(base) <= set(alone) and added >= {"health_alarms", "health_flags", "health_mean_ms"} and all(k.startswith("health_") for k in added)
    assert (alone["health_alarms"], alone["health_flags"]) == (1, 1 << CV)
    assert alone["last_detections"] == base["last_detections"] and alone["last_tracks"] == base["last_tracks"] and alone["events"] == base["events"]
    # health=None: the parent's stage table and summary keys
    p = prof()
    none = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=n, health=None)
    assert set(none) == set(base) and not any(k.startswith("health") for k in none)
    assert list(p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events",
                                                                                "visualization", "total"]
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"]
    mon.close(); lens.close()
