"""GPU: the BoT-SORT tracker (csrc/botsort.hip) against its restatement (tests/botsort_ref.py).  After every frame
rtmodt_botsort_state equals the restatement's snapshot exactly -- integers as integers, float32 state as bit patterns, the int16 /
int8 features as integers -- and the returned count matches.  tests/test_botsort_cpu.py shows every assignment optimum of these
sequences unique with a margin, and that the three component scenes change their identities when the warp / the appearance / the
score fusion is switched off.  PARITY UNPINNED: BoT-SORT and boxmot are not installed; the restatement is the published algorithm as
this project reads it."""
import os
import sys
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import botsort_ref as R  # noqa: E402
import crossing_ref  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def core_cls(pkg):
    return import_module(pkg.__name__ + ".tracking.botsort")._BotSortCore


def _run_streams(pkg, names, max_tracks=32, max_dets=16, feed="desc"):
    """Advance len(names) streams in one call per frame; compare the state with the restatement after every frame.  feed: "desc"
    (caller descriptors, or none on a motion-only sequence), "host" / "device" (frames, described on the GPU)."""
    ffi = pkg._ffi
    inputs = [R.sequence_inputs(n) for n in names]
    params, dim = inputs[0][0], inputs[0][1]
    assert all(p == params and d == dim for p, d, _ in inputs)
    S = len(names)
    core = core_cls(pkg)(n_streams=S, max_tracks=max_tracks, max_dets=max_dets, embedder="colorhist" if dim else "none", dim=dim, **params)
    assert core.dim == dim
    refs = [R.BotSortRef(dim=dim, **params) for _ in names]
    dev = []
    for f in range(max(len(fr) for _, _, fr in inputs)):
        xy = np.zeros((S, max_dets, 4), F32); cf = np.zeros((S, max_dets), F32); cl = np.zeros((S, max_dets), np.int32)
        emb = np.zeros((S, max_dets, dim), np.int8) if dim else None
        warp = np.tile(R.affine(), (S, 1))
        cnt, want, images, any_warp = np.zeros(S, np.int32), [], [], False
        for s, (_, _, fr) in enumerate(inputs):
            b, c, k, d, w, img = fr[f] if f < len(fr) else (np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32), None, None, fr[-1][5])
            n = len(b)
            xy[s, :n], cf[s, :n], cl[s, :n], cnt[s] = b, c, k, n
            if dim and n:
                emb[s, :n] = d
            if w is not None:
                warp[s], any_warp = w, True
            images.append(img)
            want.append(len(refs[s].update(b, c, k, d if n else None, w)))
        kw = dict(warp=warp if any_warp else None)
        if feed == "desc":
            ret = core.update_batch(xy, cf, cl, cnt, embeddings=emb, **kw)
        elif feed == "host":
            ret = core.update_batch(xy, cf, cl, cnt, frames=images, **kw)
        else:
            h, w_ = images[0].shape[:2]
            dev = dev or [ffi.DeviceBuffer(img.nbytes) for img in images]
            for d_, img in zip(dev, images):
                d_.upload(np.ascontiguousarray(img))
            ret = core.update_batch(xy, cf, cl, cnt, frames=[d_.ptr for d_ in dev], mem_kind=ffi.MEM_DEVICE, height=h, width=w_, stride=3 * w_, **kw)
        for s in range(S):
            got = core.snapshot(s)
            diff = R.snapshots_equal(got, refs[s].snapshot())
            assert diff is None, (names[s], f, diff)
            assert ret[s] == want[s] == len(core.returned(got)), (names[s], f)
    for d_ in dev:
        d_.free()
    core.close()
    return refs


@pytest.mark.parametrize("name", ["gmc", "reid64", "reid512", "fuse", "fuse_off"])
def test_component_scene_state_equals_restatement_bit_for_bit(pkg, name):
    """The scenes whose final identities change when the component is switched off in the restatement (tests/test_botsort_cpu.py);
    caller descriptors at dim 64 and 512, the extremes of the dot product's k-loop."""
    ref = _run_streams(pkg, [name])[0]
    assert [t.id for t in ref.tracks] == {"fuse": [1]}.get(name, [1, 2])
    if name.startswith("reid"):
        assert all(any(v < 0 for v in t.f16) and max(abs(v) for v in t.f8) <= 127 for t in ref.tracks)


@pytest.mark.parametrize("name", ["occlusion", "lifecycle", "thresholds", "warped", "empty"])
def test_sequence_state_equals_restatement_bit_for_bit(pkg, name):
    """Gaps below, at and past track_buffer (re-activation, expiry); births and deletions of one-off detections; low-confidence
    detections (some exactly at a threshold) in the second association; warps with rotation and scale; frames with no detection,
    and with no track."""
    ref = _run_streams(pkg, [name])[0]
    frames = R.sequence_inputs(name)[2]
    if name == "occlusion":
        assert ref.next_id - 1 == 5 + 2
    if name == "thresholds":
        assert sum(int((f[1] == F32(0.6)).sum() + (f[1] == F32(0.1)).sum()) for f in frames) > 3
    if name == "empty":
        assert len(frames[0][0]) == 0 and sum(len(f[0]) == 0 for f in frames) >= 7 and ref.next_id > 4


@pytest.mark.parametrize("feed", ["device", "host", "desc"])
def test_builtin_descriptor_from_rendered_frames(pkg, feed):
    """dim 192: the descriptors are computed on the GPU from 64 x 48 frames (device or host memory) and equal the restatement's;
    the same rows handed in by the caller give the same state."""
    ref = _run_streams(pkg, ["rendered"], feed=feed)[0]
    assert len(ref.tracks) == 4 and all(len(t.f8) == 192 for t in ref.tracks)


def test_eight_streams_with_ragged_counts_and_a_warp_each_in_one_call(pkg):
    """Different warps per stream (one the identity row, two none at all), a stream with tracks and no detections, one with
    detections and no tracks; caller descriptors at dim 64."""
    _run_streams(pkg, [f"stream{k}" for k in range(8)])


def test_250_tracks_against_950_detections(pkg):
    """A track count that is no multiple of 64 near the 256 x 1024 capacity, few contested pairs (tests/test_botsort_cpu.py)."""
    ref = _run_streams(pkg, ["big"], max_tracks=256, max_dets=1024)[0]
    assert len(ref.tracks) == 250


def test_first_association_at_the_contested_pair_limit_and_past_it(pkg):
    """32 tracks against 64 detections that all overlap them: exactly 2048 admissible pairs, none isolated -- the most lap.h's edge
    array holds -- and the state equals the restatement.  One more track with a single pair into a contested column, 2049, is refused
    with E_CAPACITY: nothing faults, the state stays readable, and the handle answers again after a reset."""
    ffi = pkg._ffi
    ref = _run_streams(pkg, ["limit"], max_tracks=128, max_dets=64)[0]
    assert len(ref.tracks) == 64 and sum(t.flag == R.TRACKED for t in ref.tracks) == 32
    params = R.SEQUENCES["limit"][0]
    core = core_cls(pkg)(n_streams=1, max_tracks=128, max_dets=64, **params)
    frames = R.OC.pair_limit_frames(True)
    assert core.update(*frames[0]) == 33 and len(core.snapshot(0)["ids"]) == 33
    with pytest.raises(ffi.RtmodtError) as e:
        core.update(*frames[1])
    assert e.value.code == ffi.E_CAPACITY and "contested" in e.value.msg
    with pytest.raises(ffi.RtmodtError) as e:                                     # sticky
        core.snapshot(0)
    assert e.value.code == ffi.E_CAPACITY
    st = core.snapshot(0, allow_capacity=True)                                    # ... and readable: a well-formed list
    assert st["error"] == ffi.E_CAPACITY and st["frame_count"] == 2 and 33 <= len(st["ids"]) <= 97 and (np.diff(st["ids"]) > 0).all()
    assert np.isfinite(st["mean"]).all() and st["next_id"] > st["ids"].max()
    core.reset()
    assert len(core.snapshot(0)["ids"]) == 0 and core.snapshot(0)["frame_count"] == 0
    xy, cf, cl = frames[0]
    assert core.update(xy[:3], cf[:3], cl[:3]) == 3 and len(core.snapshot(0)["ids"]) == 3
    core.close()


def test_limits_and_bad_arguments_return_codes(pkg):
    ffi = pkg._ffi
    L = ffi.lib()
    core = core_cls(pkg)(n_streams=2, max_tracks=4, max_dets=8, track_buffer=3)
    xy = np.zeros((2, 8, 4), F32)
    xy[:, :, :] = np.asarray([[4 + 40 * k, 5, 34 + 40 * k, 65] for k in range(8)], F32)
    one, zero = np.full((2, 8), 0.9, F32), np.zeros((2, 8), np.int32)
    tail = (None, 0, 0, 0, 0, None, None, None)
    for bad_n, code in ((9, ffi.E_CAPACITY), (-1, ffi.E_INVALID)):
        cnt = np.asarray([1, bad_n], np.int32)
        assert L.rtmodt_botsort_update_batch(core._h, ffi.ptr(xy), ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt), *tail) == code
    cnt = np.asarray([2, 0], np.int32)
    assert L.rtmodt_botsort_update_batch(core._h, None, ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt), *tail) == ffi.E_INVALID      # null detections
    assert L.rtmodt_botsort_update_batch(core._h, ffi.ptr(xy), ffi.ptr(one), ffi.ptr(zero), None, *tail) == ffi.E_INVALID
    # a motion-only handle takes neither frames nor descriptors; a singular or non-finite warp is refused before anything is launched
    emb, img = np.zeros((2, 8, 64), np.int8), np.zeros((48, 64, 3), np.uint8)
    for kw in (dict(embeddings=emb), dict(frames=[img, img])):
        with pytest.raises(ffi.RtmodtError) as e:
            core.update_batch(xy, one, zero, cnt, **kw)
        assert e.value.code == ffi.E_INVALID and "motion only" in e.value.msg
    for bad in (np.zeros(6, F32), np.asarray([1, 0, np.nan, 0, 1, 0], F32)):
        with pytest.raises(ffi.RtmodtError) as e:
            core.update_batch(xy, one, zero, cnt, warp=np.stack([R.affine(), bad]))
        assert e.value.code == ffi.E_INVALID
    assert L.rtmodt_botsort_state(core._h, 2, *([None] * 16)) == ffi.E_INVALID and L.rtmodt_botsort_state(core._h, -1, *([None] * 16)) == ffi.E_INVALID
    assert L.rtmodt_botsort_reset(core._h, 2) == ffi.E_INVALID
    assert L.rtmodt_botsort_last_ms(core._h, None, None, None) == ffi.E_INVALID    # no update has run yet
    assert L.rtmodt_botsort_update_from_detector(core._h, None, None, 0, 0, 0, 0, 0, None) == ffi.E_INVALID
    assert L.rtmodt_crossing_process_botsort(None, core._h, 0, None, None) == ffi.E_INVALID
    for s in range(2):
        assert len(core.snapshot(s)["ids"]) == 0 and core.snapshot(s)["frame_count"] == 0      # none of the refused calls touched the state
    # more live tracks than max_tracks in stream 1 only: sticky capacity error there, stream 0 goes on
    with pytest.raises(ffi.RtmodtError) as e:
        core.update_batch(xy, one, zero, np.asarray([2, 5], np.int32))
    assert e.value.code == ffi.E_CAPACITY and "max_tracks" in e.value.msg
    assert len(core.snapshot(0)["ids"]) == 2 and len(core.snapshot(1, allow_capacity=True)["ids"]) == 4
    assert min(core.last_ms()) >= 0 and core.last_ms()[:2] == (0.0, 0.0)
    core.reset(1)
    assert len(core.snapshot(0)["ids"]) == 2 and len(core.snapshot(1)["ids"]) == 0
    core.close()
    # a handle with descriptors: frames and descriptors together, or neither with detections, are refused; frames need dim 192
    core = core_cls(pkg)(n_streams=2, max_tracks=4, max_dets=8, embedder="colorhist", dim=64)
    for kw, word in ((dict(embeddings=emb, frames=[img, img]), "not both"), (dict(), "need frames"), (dict(frames=[img, img]), "built-in descriptor has")):
        with pytest.raises(ffi.RtmodtError) as e:
            core.update_batch(xy, one, zero, cnt, **kw)
        assert e.value.code == ffi.E_INVALID and word in e.value.msg, word
    assert core.update_batch(xy, one, zero, np.zeros(2, np.int32))[0] == 0           # no detections: neither is needed
    core.close()
    # odd capacities: every state array still starts on its own 16-byte boundary
    params, dim, frames = R.sequence_inputs("stream3")
    core, ref = core_cls(pkg)(n_streams=1, max_tracks=13, max_dets=9, embedder="colorhist", dim=dim, **params), R.BotSortRef(dim=dim, **params)
    for f, (b, c, k, d, w, _) in enumerate(frames):
        assert core.update(b, c, k, embeddings=d if len(b) else None, warp=w) == len(ref.update(b, c, k, d, w))
        assert R.snapshots_equal(core.snapshot(0), ref.snapshot()) is None, f
    core.close()


@pytest.fixture(scope="module")
def wdir(tmp_path_factory):
    return tmp_path_factory.mktemp("weights_botsort")


def _weights(pkg, wdir):
    path = os.path.join(str(wdir), "yolov8n_320_noise.rtw")
    if not os.path.exists(path):
        pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    return path


@pytest.mark.parametrize("embedder", ["none", "colorhist"])
def test_update_from_detector_with_a_warp_equals_the_same_detections_fed_by_hand(pkg, wdir, embedder):
    B = 2
    det = pkg.Detector(_weights(pkg, wdir), input_size=(320, 320), confidence=0.02, max_det=20, batch=B, warmup=False, autotune=False)
    params = dict(track_buffer=4, track_high_thresh=0.05, track_low_thresh=0.0, new_track_thresh=0.05)
    dim = 192 if embedder == "colorhist" else 0
    a = core_cls(pkg)(n_streams=B, max_tracks=128, max_dets=20, embedder=embedder, **params)
    b = core_cls(pkg)(n_streams=B, max_tracks=128, max_dets=20, embedder=embedder, **params)
    refs = [R.BotSortRef(dim=dim, **params) for _ in range(B)]
    frames = pkg.synth.frames(4 * B, 320, 320, seed=77)
    warps = [np.stack([R.affine(1.0, 1.0, 1.5, -0.5), R.affine()]), np.stack([R.affine(-2.0, 1.01, 0.0, 2.0), R.affine(0.5, 0.99, -1.0, 0.25)])]
    total = 0
    for t in range(4):
        fr = [frames[t * B + i] for i in range(B)]
        warp = None if t == 0 else warps[t % 2]
        det.enqueue(fr)
        a.update_from_detector(det, fr if dim else None, warp)
        got = det.fetch()
        xy = np.zeros((B, 20, 4), F32); cf = np.zeros((B, 20), F32); cl = np.zeros((B, 20), np.int32)
        cnt = np.zeros(B, np.int32)
        for i, d in enumerate(got):
            n = len(d)
            xy[i, :n], cf[i, :n], cl[i, :n], cnt[i] = d.xyxy, d.confidence, d.class_id, n
            refs[i].update(d.xyxy, d.confidence, d.class_id, R.DS.describe(fr[i], d.xyxy)[0] if dim else None, None if warp is None else warp[i])
            total += n
        b.update_batch(xy, cf, cl, cnt, frames=fr if dim else None, warp=warp)
        for i in range(B):
            sa, sb = a.snapshot(i), b.snapshot(i)
            assert R.snapshots_equal(sa, sb) is None, (t, i, R.snapshots_equal(sa, sb))
            assert R.snapshots_equal(sb, refs[i].snapshot()) is None, (t, i, R.snapshots_equal(sb, refs[i].snapshot()))
    assert total > 0 and min(a.last_ms()) >= 0
    with pytest.raises(pkg._ffi.RtmodtError):                                     # refused before anything is queued on the detector's stream
        a.update_from_detector(det, fr if dim else None, np.zeros((B, 6), F32))
    a.close(); b.close(); det.close()


def _as_dict(e):
    return dict(track_id=e.track_id, kind=e.event_type, index=e.index, direction=e.direction, class_id=e.class_id, bbox_xyxy=e.bbox_xyxy,
                centroid=e.centroid, prev=e.previous, frames=e.frames)


def test_crossing_counter_on_device_state_equals_the_crossing_restatement(pkg):
    """Boxes march over a line and through a gate, one is not detected for four frames and one is over the line on its second frame:
    rtmodt_crossing_process_botsort on the device
    state against the crossing restatement fed the BoT-SORT restatement's returned tracks that were matched this frame (tsu == 0),
    with the matched detection as the box."""
    CR = crossing_ref
    params = dict(track_buffer=10)
    trk = pkg.BotSortTracker(max_tracks=32, max_dets=16, **params)
    bref = R.BotSortRef(**params)
    kw = dict(max_tracks=32, max_gap_frames=8)
    on_device = pkg.events.CrossingCounter(CR.MARCH_LINES, CR.MARCH_GATES, **kw)
    ref = CR.CrossingRef(CR.MARCH_LINES, CR.MARCH_GATES, **kw)
    n_events = 0
    for f, (xy, cf, cl, _) in enumerate(CR.march_scene(early=True)):
        tracks = trk.update(pkg.Detections(xy, cf, cl))
        idx = bref.update(xy, cf, cl)
        assert R.snapshots_equal(trk._core.snapshot(0), bref.snapshot()) is None, f
        want_tracks = bref.tracks_out(idx)
        assert [(t.track_id, t.time_since_update) for t in tracks] == [(bref.tracks[i].id, bref.tracks[i].tsu) for i in idx], f
        assert all(np.array_equal(t.xyxy.view(np.int32), b.view(np.int32)) for t, (_, b) in zip(tracks, want_tracks)), f
        got = on_device.process_tracker(trk, f)[0]
        want = ref.process([(bref.tracks[i].id, bref.tracks[i].box, bref.tracks[i].cls) for i in idx if bref.tracks[i].tsu == 0], f)
        assert [dict(_as_dict(e), kind=e.event_type.split("_")[0]) for e in got] == [{k: v for k, v in e.items() if k != "track"} for e in want], f
        assert on_device.snapshot() == ref.snapshot(), f
        n_events += len(got)
    assert n_events > 8 and ref.gate_total == [6] and all(t.time_since_update == 0 for t in tracks)
    assert on_device.process_tracker(SimpleNamespace(_core=trk._core), 99) == [[]]
    trk.close(); on_device.close()


def test_embedder_network_features_are_the_quantised_ema_of_its_descriptors(pkg, tmp_path):
    """embedder = an .rtreid file (synthetic weights): two frames; the state, feat16 / feat8 included, equals the restatement fed the
    rows rtmodt_reid_embed gives for the same boxes."""
    wpath = str(tmp_path / "osnet_synth.rtreid")
    pkg.reid_weights.save(wpath, pkg.reid_weights.synthetic(0))
    N = 4
    core = core_cls(pkg)(n_streams=1, max_tracks=8, max_dets=N, embedder=wpath)
    assert core.dim == 512
    e = pkg.tracking.ReidEmbedder(wpath, max_boxes=N, max_frames=1)
    ref = R.BotSortRef(dim=512)
    boxes = np.asarray([[6, 4, 26, 44], [36, 6, 58, 46]], F32)
    col = R.DS.PALETTE[:2]
    for f in range(2):
        b = boxes + F32(f)
        img = R.DS.render_scene(b, col, 48, 64, seed=f)
        xy = np.zeros((1, N, 4), F32)
        xy[0, :2] = b
        _, desc = e.embed([img], xy, [2])
        cf, cl = np.full(2, 0.9, F32), np.zeros(2, np.int32)
        assert core.update(b, cf, cl, frame=img) == len(ref.update(b, cf, cl, desc[0, :2]))
        got = core.snapshot(0)
        assert R.snapshots_equal(got, ref.snapshot()) is None, (f, R.snapshots_equal(got, ref.snapshot()))
    assert [t.flag for t in ref.tracks] == [2, 2] and np.abs(got["feat8"]).max() > 0
    with pytest.raises(pkg._ffi.RtmodtError) as err:
        core.update(b, cf, cl, embeddings=np.zeros((2, 512), np.int8))
    assert err.value.code == pkg._ffi.E_INVALID and "embedder network" in err.value.msg
    core.close(); e.close()


def test_facade_tracks_trails_warp_and_config(pkg):
    params, dim, frames = R.sequence_inputs("gmc")
    trk = pkg.BotSortTracker.from_config({"algorithm": "bytetrack", "botsort": dict(params, max_tracks=32, max_dets=16, unknown_key=1)})
    ref = R.BotSortRef(**params)
    out = []
    for f, (xy, cf, cl, _, warp, _) in enumerate(frames):
        out = trk.update(pkg.Detections(xy, cf, cl), warp=warp.reshape(2, 3))
        want = ref.tracks_out(ref.update(xy, cf, cl, None, warp))
        assert [t.track_id for t in out] == [i for i, _ in want], f
        assert all(np.array_equal(t.xyxy.view(np.int32), b.view(np.int32)) for t, (_, b) in zip(out, want)), f
    assert [t.track_id for t in out] == [1, 2] and len(out[0].trail) > 1 and trk.algorithm == "botsort" and trk.needs_frame is False
    empty = pkg.Detections(np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32))
    assert trk.update(empty) == []                         # unmatched: lost, not returned
    with pytest.raises(pkg._ffi.RtmodtError):
        trk.update(empty, warp=np.zeros((2, 3), F32))
    with pytest.raises(ValueError, match="motion only"):
        trk.update(empty, embeddings=np.zeros((0, 64), np.int8))
    trk.close()
    hist = pkg.BotSortTracker(embedder="colorhist", max_tracks=8, max_dets=8)
    rows = pkg.BotSortTracker(embedding_dim=64, max_tracks=8, max_dets=8)
    assert hist.needs_frame is True and rows.needs_frame is False and rows._core.dim == 64
    xy, cf, cl = frames[0][:3]
    with pytest.raises(ValueError, match="exactly one"):
        hist.update(pkg.Detections(xy, cf, cl))
    assert len(rows.update(pkg.Detections(xy, cf, cl), embeddings=np.eye(2, 64, dtype=np.float32))) == 2
    hist.close(); rows.close()
