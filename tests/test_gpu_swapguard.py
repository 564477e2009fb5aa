"""GPU: the ID-swap guard (csrc/swapguard.hip) against its plain-Python restatement (tests/swapguard_ref.py): the corrected ids, the
events, the ledger snapshot and the revert count compared after EVERY frame, with exact equality; everything through the C ABI.
The design document's B.4 / G.1 "appearance verification"; PARITY UNPINNED (there is no reference implementation)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import swapguard_ref as R

pytestmark = pytest.mark.gpu

# name -> (scene factory, restatement / guard parameters)
SCENES = {
    "s1": (R.scene_pair, {}),
    "s2_chain": (R.scene_s2, {}),
    "s3_twins": (R.scene_s3, {}),
    "s4_nan_corner": (R.scene_s4_nan_corner, {}),
    "s4_outside": (R.scene_s4_outside, {}),
    "s4_gap_kept": (lambda: R.scene_s4_gap(3), dict(max_gap_frames=4, history=8, min_history=1)),
    "s4_gap_expired": (lambda: R.scene_s4_gap(4), dict(max_gap_frames=4)),
    "s4_short_history": (R.scene_s4_short_history, dict(window=1)),
    "s4_window_inside": (lambda: R.scene_s4_window(24), {}),
    "s4_window_outside": (lambda: R.scene_s4_window(25), {}),
    "s5_32_pairs": (R.scene_s5, dict(max_tracks=64)),
    "s5_short_ring": (R.scene_s5, dict(max_tracks=64, history=2, min_history=2, min_similarity_pm=900, min_gain_pm=50, contact_iou=0.05)),
    "s6_capacity": (R.scene_s6, dict(max_tracks=4, max_gap_frames=1000)),
}
for _seed in R.FUZZ_SEEDS:
    SCENES[f"s7_fuzz{_seed}"] = (functools.partial(R.scene_s7, _seed), dict(max_tracks=16))


def guard_kwargs(kw):
    """Restatement parameters -> IdSwapGuard's."""
    kw = dict(kw)
    if "min_similarity_pm" in kw:
        kw["min_similarity"] = kw.pop("min_similarity_pm") / 1000.0
    kw.setdefault("max_tracks", 32)
    return kw


def ref_kwargs(kw):
    kw = dict(kw)
    kw.setdefault("max_tracks", 32)
    return kw


def as_dict(e):
    return dict(frame_id=e.frame_id, track_a=e.track_a, track_b=e.track_b, id_a=e.id_a, id_b=e.id_b, sims=list(e.similarities))


@functools.lru_cache(maxsize=None)
def trace(name):
    """The scene and what the restatement makes of it, once for every test that plays it: per frame (ids out, events, snapshot, reverts, in error)."""
    factory, kw = SCENES[name]
    scene = factory()
    ref = R.SwapGuardRef(**ref_kwargs(kw))
    steps = []

    def process(ids, boxes, img, fid):
        out, ev = ref.process_frame(ids, boxes, img, fid)
        steps.append((out, ev, ref.snapshot(), ref.n_reverted, ref.ledger_overflow))
        return out, ev

    for _ in R.play(scene, process):
        pass
    return scene, steps, ref


def play_on_gpu(pkg, name, device_frames):
    scene, steps, ref = trace(name)
    ffi = pkg._ffi
    guard = pkg.tracking.IdSwapGuard(**guard_kwargs(SCENES[name][1]))
    h, w = scene["h"], scene["w"]
    buf = ffi.DeviceBuffer(h * w * 3) if device_frames else None
    k = [0]

    def process(ids, boxes, img, fid):
        want_ids, want_ev, want_state, want_n, overflow = steps[k[0]]
        k[0] += 1
        where = f"{name} frame {fid}"
        if buf is not None:
            buf.upload(img)
            call = lambda: guard.process_arrays(ids, boxes, buf.ptr, fid, height=h, width=w, stride=3 * w, mem_kind=ffi.MEM_DEVICE)
        else:
            call = lambda: guard.process_arrays(ids, boxes, img, fid)
        if overflow:                                       # the documented contract: E_CAPACITY on that frame and from then on, never a fault
            with pytest.raises(ffi.RtmodtError) as e:
                call()
            assert e.value.code == ffi.E_CAPACITY and "ledger full" in str(e.value), where
            with pytest.raises(ffi.RtmodtError) as e:
                guard.state()
            assert e.value.code == ffi.E_CAPACITY, where
            assert [as_dict(x) for x in guard.last_events[0]] == want_ev and guard.reverted() == want_n, where
            return want_ids, want_ev
        got_ids, got_ev = call()
        assert got_ids.tolist() == want_ids, where
        assert [as_dict(x) for x in got_ev] == want_ev, where
        assert guard.state() == want_state, where
        assert guard.reverted() == want_n, where
        return got_ids, got_ev

    for _ in R.play(scene, process):
        pass
    assert k[0] == len(steps)
    if buf is not None:
        buf.free()
    guard.close()
    return steps, ref


@pytest.mark.parametrize("device_frames", [False, True], ids=["host_frames", "device_frames"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_through_process(pkg, name, device_frames):
    """S1 .. S7 through rtmodt_swapguard_process, the caller adopting ids_out; host and device frames."""
    steps, ref = play_on_gpu(pkg, name, device_frames)
    n_events = sum(len(s[1]) for s in steps)
    if name == "s1":
        assert [(e["frame_id"], e["sims"]) for s in steps for e in s[1]] == [(22, [0, 1000, 0, 1000])]
    if name == "s5_32_pairs":
        assert n_events == 16 and len(steps[19][1]) == 16
    if name == "s6_capacity":
        assert steps[2][4] and not steps[1][4]
    if name.startswith("s7"):
        assert n_events >= 5 and ref.refused >= 5          # the condition tests/test_swapguard_cpu.py asserts on the restatement alone
    if name in ("s2_chain", "s3_twins", "s4_outside", "s4_short_history", "s4_window_outside"):
        assert n_events == 0 and ref.refused > 0


def tracker_inputs():
    """Stream 0: S1's detections.  Stream 1: S5's 64 boxes as detections; the even pairs are listed in the opposite order after the
    frame where the two boxes coincide, which is what makes ByteTrack exchange their ids."""
    s1, h1, w1 = R.s1_frames()
    s5 = R.scene_s5(frames=34)
    out = []
    for f in range(34):
        tr = s5["frames"][f]["tracks"]
        order = []
        for p in range(32):
            pair = [2 * p, 2 * p + 1]
            order += pair[::-1] if (p % 2 == 0 and f > 14) else pair
        xy5 = np.asarray([tr[i][1] for i in order], np.float32)
        out.append(((s1[f][0], s1[f][1]), (s5["frames"][f]["img"], xy5)))
    return out, (h1, w1), (s5["h"], s5["w"])


@pytest.mark.parametrize("assign", ["greedy", "lapjv"])
def test_bytetrack_device_state(pkg, assign, tmp_path):
    """rtmodt_swapguard_process_tracker on a real ByteTrack handle, 2 streams in one call carrying different scenes (S1 and S5, on frames
    of one size: S1's is pasted into a 360 x 640 canvas).  The restatement is fed from the handle's own state as it stands before the
    call; afterwards the state shows the exchanged ids and nothing else changed, and a second handle that runs without the guard
    differs from the first in the ids alone.  A crossing counter reading the guarded handle counts S1's two objects once each under
    their own ids, and a zone engine reading it agrees with one that is handed the same tracks as a list (the exchange leaves the
    tracker's list out of id order: both kernels then place their ledger rows by counting).  (Under lapjv the frame where the boxes coincide is a tie between two optimal assignments, so whether the handle
    swaps at all is read off the unguarded handle; under greedy it is certain: tests/test_swapguard_cpu.py.)"""
    ffi = pkg._ffi
    S, N, M, MG = 2, 64, 512, 128
    mode = {"greedy": ffi.ASSIGN_GREEDY, "lapjv": ffi.ASSIGN_LAPJV}[assign]
    Core = pkg.tracking.tracker._ByteTrackCore
    core, plain = (Core(0.5, 30, 0.8, n_streams=S, max_tracks=M, max_dets=N, assign_mode=mode) for _ in range(2))
    guard = pkg.tracking.IdSwapGuard(n_streams=S, max_tracks=MG)
    lines = [{"name": "left", "a": [70, 0], "b": [70, 119], "direction": "both"}, {"name": "right", "a": [140, 0], "b": [140, 119], "direction": "both"}]
    counters = [pkg.events.CrossingCounter(lines, n_streams=S, max_tracks=M) for _ in range(2)]
    zone = [{"name": "left_third", "polygon": [[40, 0], [100, 0], [100, 119], [40, 119]], "dwell_time_sec": 0.1, "cooldown_sec": 0.15}]
    zones_dev, zones_host = (pkg.events.ZoneEventEngine(zone, log_path=str(tmp_path / f"z{k}.jsonl"), n_streams=S, max_tracks=M) for k in range(2))
    zone_events = 0
    refs = [R.SwapGuardRef(max_tracks=MG) for _ in range(S)]
    frames, (h1, w1), (H, W) = tracker_inputs()
    crossed = [[], []]
    total = [0, 0]
    for f, per_stream in enumerate(frames):
        canvas = np.zeros((H, W, 3), np.uint8)
        canvas[:h1, :w1] = per_stream[0][0]
        imgs = [canvas, per_stream[1][0]]
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32); cnt = np.zeros(S, np.int32)
        for s in range(S):
            xy = per_stream[s][1]
            xyxy[s, :len(xy)], conf[s, :len(xy)], cnt[s] = xy, 0.9, len(xy)
        core.update_batch(xyxy, conf, cls, cnt)
        plain.update_batch(xyxy, conf, cls, cnt)
        before = [core.snapshot(s) for s in range(S)]
        got = guard.process_tracker(SimpleNamespace(_core=core, report="matched"), imgs, f)
        for s in range(S):
            pre, post, other = before[s], core.snapshot(s), plain.snapshot(s)
            passed = np.nonzero(pre["tsu"] == 1)[0]
            out, ev = refs[s].process_frame(pre["ids"][passed], pre["xyxy"][passed], imgs[s], f)
            want_ids = pre["ids"].copy()
            want_ids[passed] = out
            want = [dict(e, track_a=int(passed[e["track_a"]]), track_b=int(passed[e["track_b"]])) for e in ev]
            where = f"frame {f} stream {s}"
            assert [as_dict(e) for e in got[s]] == want and all(e.stream == s for e in got[s]), where
            assert guard.state(s) == refs[s].snapshot() and guard.reverted(s) == refs[s].n_reverted, where
            assert post["ids"].tolist() == want_ids.tolist() and post["next_id"] == pre["next_id"] == other["next_id"], where
            for key in ("xyxy", "conf", "cls", "age", "tsu"):
                assert np.array_equal(post[key], pre[key]) and np.array_equal(post[key], other[key]), (where, key)
            assert sorted(post["ids"].tolist()) == sorted(other["ids"].tolist()), where
            total[s] += len(ev)
        now = 100.0 + 0.04 * f
        zd = zones_dev.process_tracker(SimpleNamespace(_core=core, report="matched"), f, now=now)
        for s in range(S):
            st = core.snapshot(s)
            listed = [SimpleNamespace(track_id=int(st["ids"][i]), xyxy=st["xyxy"][i], class_id=int(st["cls"][i])) for i in np.nonzero(st["tsu"] == 1)[0]]
            zh = zones_host.process(listed, f, stream=s, now=now)
            assert [(e.track_id, e.zone_name, e.dwell_time_sec) for e in zd[s]] == [(e.track_id, e.zone_name, e.dwell_time_sec) for e in zh], (f, s)
            assert zones_dev.snapshot(s) == zones_host.snapshot(s), (f, s)
            zone_events += len(zh) if s == 0 else 0
        for k, c in enumerate((core, plain)):
            crossed[k] += [(e.track_id, e.name) for e in counters[k].process_tracker(SimpleNamespace(_core=c, report="matched"), f)[0]]
    last = plain.snapshot(0)
    a_box = frames[-1][0][1][1]                             # S1 lists B, A after frame 12
    swapped = int(last["ids"][[i for i in range(len(last["ids"])) if np.array_equal(last["xyxy"][i], a_box)][0]]) == 2
    if assign == "greedy":
        assert swapped and total[1] >= 8                    # S5's even pairs
    assert total[0] == int(swapped)
    assert sorted(crossed[0]) == [(1, "right"), (2, "left")]              # guarded: A (id 1) passes x = 140, B (id 2) passes x = 70
    assert sorted(crossed[1]) == ([(1, "left"), (2, "right")] if swapped else [(1, "right"), (2, "left")])      # unguarded: each under the other's id
    assert np.array_equal(core.snapshot(0)["ids"], plain.snapshot(0)["ids"]) != swapped
    assert zone_events >= 4                                  # B dwells in the zone before and after the revert, A early on
    for x in (core, plain, guard, zones_dev, zones_host, *counters):
        x.close()


class _ScriptedDetector:
    """S1's detections, one frame a call (pipeline.run with device_handoff=False hands them to tracker.update)."""

    def __init__(self, pkg, dets):
        self.pkg, self.dets, self.k = pkg, dets, 0

    def detect(self, frame):
        _, xy, cf, cl = self.dets[self.k]
        self.k += 1
        return self.pkg.Detections(xy, cf, cl)


def test_guard_object_and_pipeline(pkg):
    """IdSwapGuard.process on Track-like objects, and pipeline.run(swap_guard=...) around a MultiObjectTracker: one swap reverted on S1."""
    frames, h, w = R.s1_frames()
    guard = pkg.tracking.IdSwapGuard(max_tracks=8)
    ids = {"a": 1, "b": 2}
    events = []
    for fr in R.scene_pair()["frames"]:
        if fr["frame_id"] == 13:
            ids = {"a": 2, "b": 1}
        tracks = [SimpleNamespace(track_id=ids[k], xyxy=b) for k, b in fr["tracks"]]
        out, ev = guard.process(tracks, fr["img"], fr["frame_id"])
        ids = {k: int(i) for (k, _), i in zip(fr["tracks"], out)}
        events += ev
    assert len(events) == 1 and isinstance(events[0], pkg.SwapEvent) and events[0].similarities == (0, 1000, 0, 1000) and ids == {"a": 1, "b": 2}
    ms = guard.last_ms()
    assert ms["describe"] > 0 and ms["step"] > 0
    with pytest.raises(TypeError, match="process\\(tracks, frame, frame_id\\)"):
        guard.process_tracker(object(), [frames[0][0]], 0)
    guard.close()

    guard = pkg.tracking.IdSwapGuard(max_tracks=8)                              # MultiObjectTracker's capacity (2048) is larger than the guard's: only the passed tracks count
    trk = pkg.MultiObjectTracker("bytetrack")
    trk.report = "matched"
    seen = []

    class _Events:
        def process(self, tracks, fid):
            seen.append(sorted((t.track_id, int(t.xyxy[0])) for t in tracks))
            return []

    prof = pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack([f[0] for f in frames])), _ScriptedDetector(pkg, frames), trk, prof, max_frames=40,
                           device_stages=False, device_handoff=False, event_engine=_Events(), swap_guard=guard)
    assert out["id_swaps_reverted"] == 1 and guard.reverted() == 1
    assert seen[21] == [(1, 66), (2, 102)] and seen[22] == [(1, 104), (2, 64)] and seen[39] == [(1, 138), (2, 30)]   # id 1 is A (x = 60 + 2f) again from frame 22
    guard.close()


def test_invalid_arguments_and_capacity_are_error_codes(pkg):
    ffi = pkg._ffi
    G = pkg.tracking.IdSwapGuard
    for bad in (dict(history=9), dict(history=0), dict(min_history=6), dict(min_history=0), dict(window=-1), dict(min_similarity=1.5), dict(min_gain_pm=-1),
                dict(contact_iou=float("nan")), dict(max_gap_frames=-1), dict(max_tracks=1025), dict(max_tracks=0), dict(n_streams=65), dict(max_events=0)):
        with pytest.raises(ffi.RtmodtError) as e:
            G(**bad)
        assert e.value.code == ffi.E_INVALID, bad
    img = np.zeros((32, 48, 3), np.uint8)
    box = np.asarray([[0, 0, 8, 8], [10, 0, 18, 8], [20, 0, 28, 8]], np.float32)
    g = G(max_tracks=2, n_streams=2, max_events=1)
    for call, code in ((lambda: g.process_arrays([1, 1], box[:2], img, 0), ffi.E_INVALID),                  # duplicate id
                       (lambda: g.process_arrays([1, 2, 3], box, img, 0), ffi.E_CAPACITY),                  # more than max_tracks
                       (lambda: g.process_arrays([1], box[:1], img, 0, stream=2), ffi.E_INVALID),
                       (lambda: g.process_arrays([1], box[:1], 1, 0, height=32, width=48, stride=100, mem_kind=ffi.MEM_DEVICE), ffi.E_INVALID),   # pitch < 3 w
                       (lambda: g.process_arrays([1], box[:1], img, 0, mem_kind=7), ffi.E_INVALID)):
        with pytest.raises(ffi.RtmodtError) as e:
            call()
        assert e.value.code == code
    assert g.state(0) == [] and g.state(1) == []                                                           # nothing was launched
    ids, ev = g.process_arrays([5, 6], box[:2], img, 0, stream=1)
    assert ids.tolist() == [5, 6] and ev == [] and [r[:5] for r in g.state(1)] == [[5, 0, 1, 0, -1], [6, 0, 1, 0, -1]]
    # a tracker with three passed tracks against max_tracks = 2: E_CAPACITY, and the stream stays in error
    core = pkg.tracking.tracker._ByteTrackCore(n_streams=1, max_tracks=16, max_dets=8)
    core.update(box, np.full(3, 0.9, np.float32), np.zeros(3, np.int32))
    trk = SimpleNamespace(_core=core, report="matched")
    with pytest.raises(ffi.RtmodtError) as e:
        g.process_tracker(trk, [img], 1)
    assert e.value.code == ffi.E_CAPACITY and "max_tracks" in str(e.value)
    with pytest.raises(ffi.RtmodtError) as e:
        g.state(0)
    assert e.value.code == ffi.E_CAPACITY and len(g.state(1)) == 2                                         # the other stream is not affected
    with pytest.raises(ValueError):
        g.process_tracker(trk, [img, img], 2)
    core.close(); g.close()


def test_event_overflow_truncates_events_not_reverts(pkg):
    """max_events = 4 and S5's sixteen reverts in one frame: E_CAPACITY, the first four events, all sixteen exchanges applied."""
    scene, steps, _ = trace("s5_32_pairs")
    ffi = pkg._ffi
    guard = pkg.tracking.IdSwapGuard(max_tracks=64, max_events=4)
    k = [0]

    def process(ids, boxes, img, fid):
        want_ids, want_ev, want_state, want_n, _ = steps[k[0]]
        k[0] += 1
        if len(want_ev) <= 4:
            got_ids, got_ev = guard.process_arrays(ids, boxes, img, fid)
            assert got_ids.tolist() == want_ids and [as_dict(e) for e in got_ev] == want_ev
        else:
            with pytest.raises(ffi.RtmodtError) as e:
                guard.process_arrays(ids, boxes, img, fid)
            assert e.value.code == ffi.E_CAPACITY and "16 reverts" in str(e.value)
            assert [as_dict(e) for e in guard.last_events[0]] == want_ev[:4]
        assert guard.state() == want_state and guard.reverted() == want_n, fid
        return want_ids, want_ev

    for _ in R.play(scene, process):
        pass
    assert guard.reverted() == 16
    guard.close()
