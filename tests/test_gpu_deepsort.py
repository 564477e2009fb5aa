"""GPU: the DeepSORT tracker (csrc/deepsort.hip, csrc/appearance.hip) against its restatement (tests/deepsort_ref.py).  Everything is
compared exactly: integers as integers, float32 state as bit patterns, descriptors and galleries byte for byte.  The first test
settles the operand lane map of v_mfma_i32_16x16x64_i8 with operands in which every (row, k) and (k, column) entry is
distinguishable.  PARITY UNPINNED: deep_sort_realtime is not installed; the restatement is the published algorithm."""
import ctypes as C
import os
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deepsort_ref as R  # noqa: E402
import eval_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def core_cls(pkg):
    return import_module(pkg.__name__ + ".tracking.deepsort")._DeepSortCore


# ------------------------------------------------------------------------------------------------------------ lane map
@pytest.mark.parametrize("T,N,dim", [(1, 1, 64), (17, 33, 192), (100, 300, 512), (256, 1024, 64), (17, 1024, 192), (256, 33, 512), (100, 1, 192),
                                     (1, 300, 512)])
def test_dotmax_equals_integer_restatement(pkg, T, N, dim):
    """Operands built so that a wrong (row, k) or (k, column) placement changes the result: every entry of the gallery and of the
    descriptors is a different function of (track, sample, k) / (k, detection), with both signs and the extremes -128 / 127 present,
    the shapes are not multiples of 16 or 64, and the gallery counts are ragged (0 .. budget)."""
    rng = np.random.default_rng(T * 7919 + N * 31 + dim)
    budget = 37 if T > 1 else 128
    t, s, k = np.meshgrid(np.arange(T), np.arange(budget), np.arange(dim), indexing="ij")
    gal = ((t * 131 + s * 31 + k * 7 + (k * k) % 13 + rng.integers(0, 3, t.shape)) % 256 - 128).astype(np.int8)
    n, k2 = np.meshgrid(np.arange(N), np.arange(dim), indexing="ij")
    det = ((n * 17 + k2 * 29 + (n * k2) % 11 + rng.integers(0, 3, n.shape)) % 256 - 128).astype(np.int8)
    counts = rng.integers(0, budget + 1, T).astype(np.int32)
    counts[0] = budget if T == 1 else 0
    if T > 2:
        counts[1], counts[2] = budget, 1
    # one-hot probes: sample 0 of the last track is e_k0, so its dot product with detection j is det[j, k0] alone
    k0 = dim - 3
    if counts[-1] == 0:
        counts[-1] = 1
    gal[-1, :counts[-1]] = 0
    gal[-1, 0, k0] = 1
    got = pkg._ffi.appearance_dotmax(gal, counts, det)
    want = R.dotmax(gal, counts, det)
    assert got.shape == (T, N) and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(got[-1], np.maximum(det[:, k0].astype(np.int32), 0) if counts[-1] > 1 else det[:, k0].astype(np.int32))
    if T > 1:
        assert (got[0] == R.INT32_MIN).all()


# ---------------------------------------------------------------------------------------------------------- descriptor
def _boxes(h, w, rng):
    fixed = [[-50, -50, -10, -10], [w + 5, 3, w + 40, 20], [10, 10, 10, 30], [5, 8, 30, 8], [30, 20, 10, 5], [7, 9, 8, 10], [0, 0, w, h],
             [-1e9, -1e9, 1e9, 1e9], [3.99, 4.01, 20.5, 31.999], [w - 1.5, h - 1.2, w + 0.7, h + 3], [float("nan"), 1, 9, 9],
             [0.5, 0.5, w * 0.5, h * 0.9]]
    rnd = []
    for _ in range(20):
        x0, y0 = rng.uniform(-10, w - 2), rng.uniform(-10, h - 2)
        rnd.append([x0, y0, x0 + rng.uniform(1, w / 2), y0 + rng.uniform(1, h / 2)])
    return np.asarray(fixed + rnd, np.float32)


@pytest.mark.parametrize("h,w,pad", [(48, 64, 0), (479, 641, 5), (1080, 1920, 64)])
@pytest.mark.parametrize("kind", ["host", "device"])
def test_descriptor_counts_and_bytes_equal_restatement(pkg, h, w, pad, kind):
    rng = np.random.default_rng(h + w)
    n_frames = 2
    pitch = 3 * w + pad
    bufs = [rng.integers(0, 256, (h, pitch), dtype=np.uint8) for _ in range(n_frames)]
    for b in bufs:
        b[h // 3:h // 2, :3 * (w // 2)] = 200                       # a flat patch: many equal pixels in one bin
    views = [np.lib.stride_tricks.as_strided(b, (h, w, 3), (pitch, 3, 1)) for b in bufs]
    boxes = [_boxes(h, w, rng), _boxes(h, w, rng)[:7]]
    want = [R.describe(v, b) for v, b in zip(views, boxes)]
    before = [b.copy() for b in bufs]
    if kind == "host":
        desc, counts = pkg._ffi.appearance_describe(views, boxes, want_counts=True)
        after = bufs
    else:
        dev = [pkg._ffi.DeviceBuffer(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            d.upload(b)
        desc, counts = pkg._ffi.appearance_describe([d.ptr for d in dev], boxes, height=h, width=w, stride=pitch, mem_kind=pkg._ffi.MEM_DEVICE,
                                                    want_counts=True)
        after = [d.download().reshape(h, pitch) for d in dev]
        for d in dev:
            d.free()
    for i in range(n_frames):
        assert np.array_equal(counts[i], want[i][1]), (i, np.argwhere(counts[i] != want[i][1])[:5])
        assert np.array_equal(desc[i], want[i][0]), i
        assert np.array_equal(after[i], before[i]), "the frame was written to"
    assert counts[0][6].sum() == 3 * h * w and not counts[0][0].any() and not counts[0][10].any()


# ----------------------------------------------------------------------------------------------------------- # sequences
def _run_streams(pkg, names, mode, max_tracks=32, max_dets=16):
    """Advance len(names) streams in one call per frame and compare rtmodt_deepsort_state with the restatement after every frame."""
    inputs = [R.sequence_inputs(n) for n in names]
    params = inputs[0][0]
    assert all(p == params for p, _ in inputs)
    S = len(names)
    core = core_cls(pkg)(n_streams=S, max_tracks=max_tracks, max_dets=max_dets, **params)
    refs = [R.DeepSortRef(**params) for _ in names]
    h, w = inputs[0][1][0][0].shape[:2]
    blank = np.zeros((h, w, 3), np.uint8)
    dev = [pkg._ffi.DeviceBuffer(blank.nbytes) for _ in range(S)] if mode == "device" else None
    T = max(len(fr) for _, fr in inputs)
    returned = [[] for _ in names]
    for f in range(T):
        xy = np.zeros((S, max_dets, 4), np.float32); cf = np.zeros((S, max_dets), np.float32); cl = np.zeros((S, max_dets), np.int32)
        emb = np.zeros((S, max_dets, R.DIM), np.int8)
        cnt, frames = np.zeros(S, np.int32), []
        for s, (_, fr) in enumerate(inputs):
            if f < len(fr):
                img, b, c, k, _ = fr[f]
            else:
                img, b, c, k = blank, np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)
            n = len(b)
            xy[s, :n], cf[s, :n], cl[s, :n], cnt[s] = b, c, k, n
            d = R.describe(img, b)[0]
            emb[s, :n] = d
            frames.append(img)
            idx = refs[s].update(b, c, k, d)
            returned[s].append(refs[s].tracks_out(idx))
        if mode == "desc":
            ret = core.update_batch(xy, cf, cl, cnt, embeddings=emb)
        elif mode == "device":
            for d, img in zip(dev, frames):
                d.upload(img)
            ret = core.update_batch(xy, cf, cl, cnt, frames=[d.ptr for d in dev], mem_kind=pkg._ffi.MEM_DEVICE, height=h, width=w, stride=3 * w)
        else:
            ret = core.update_batch(xy, cf, cl, cnt, frames=frames)
        for s in range(S):
            diff = R.snapshots_equal(core.snapshot(s), refs[s].snapshot())
            assert diff is None, (names[s], f, diff)
            assert ret[s] == len(returned[s][-1])
    core.close()
    for d in dev or []:
        d.free()
    return refs, returned, inputs


@pytest.mark.parametrize("name,mode", [("crossing", "frames"), ("occlusion", "frames"), ("lifecycle", "device"), ("budget", "frames"),
                                       ("min_confidence", "frames"), ("crossing", "desc"), ("occlusion", "desc")])
def test_sequence_state_equals_restatement_bit_for_bit(pkg, name, mode):
    """crossing pairs; occlusion gaps up to and past max_age; tentative deletion and n_init confirmation; more than nn_budget updates
    of one track; min_confidence filtering -- with descriptors computed on the GPU from host or device frames, and with caller
    descriptors."""
    refs, returned, inputs = _run_streams(pkg, [name], mode)
    ref = refs[0]
    if name == "occlusion":       # max_age = 5: a track missed for 3 or 4 frames comes back at time_since_update 4 or 5 and is matched by the
        assert ref.next_id - 1 == 5 + 3   # cascade; missed for 5, 9 or 30 frames it comes back past the last level: deleted, a new id is born
    if name == "budget":
        assert max(ref.hits) > ref.nn_budget and all(len(g) == ref.nn_budget for g in ref.gallery)
    if name == "lifecycle":
        assert ref.next_id - 1 > len(ref.ids) + 5             # tentative tracks were born and deleted
    if name == "min_confidence":
        assert sum(int((cf < np.float32(0.3)).sum()) for _, _, cf, _, _ in inputs[0][1]) > 20


def test_eight_streams_with_ragged_counts_in_one_call(pkg):
    _run_streams(pkg, [f"stream{k}" for k in range(8)], "frames")


def test_caller_descriptors_of_another_dimension(pkg):
    """dim = 64 embeddings (deepsort_ref.EMBEDDED) quantised by rtmodt_appearance_quantize."""
    params, dim, frames = R.embedded_inputs("embed64")
    core = core_cls(pkg)(n_streams=1, max_tracks=16, max_dets=8, dim=dim, **params)
    ref = R.DeepSortRef(dim=dim, **params)
    for f, (x, xy, cf, cl, _) in enumerate(frames):
        q = pkg._ffi.appearance_quantize(x)
        assert np.array_equal(q, R.quantize_rows(x))
        ref.update(xy, cf, cl, q)
        core.update(xy, cf, cl, embeddings=q)
        assert R.snapshots_equal(core.snapshot(0), ref.snapshot()) is None, f
    assert ref.next_id - 1 == 6                               # the 7-frame gap is past the last cascade level (max_age = 5), the 3-frame gap is not
    with pytest.raises(pkg._ffi.RtmodtError) as e:            # this handle has no built-in descriptor for frames
        core.update(frames[0][1], frames[0][2], frames[0][3], frame=np.zeros((240, 320, 3), np.uint8))
    assert e.value.code == pkg._ffi.E_INVALID
    core.close()


@pytest.fixture(scope="module")
def wdir(tmp_path_factory):
    return tmp_path_factory.mktemp("weights_deepsort")


def test_update_from_detector_equals_the_same_detections_fed_by_hand(pkg, wdir):
    path = os.path.join(str(wdir), "yolov8n_320_noise.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    B = 2
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, batch=B, warmup=False, autotune=False)
    params = dict(max_age=4, n_init=2, nn_budget=8, min_confidence=0.0)
    a = core_cls(pkg)(n_streams=B, max_tracks=128, max_dets=20, **params)
    b = core_cls(pkg)(n_streams=B, max_tracks=128, max_dets=20, **params)
    refs = [R.DeepSortRef(**params) for _ in range(B)]
    frames = pkg.synth.frames(4 * B, 320, 320, seed=77)
    total = 0
    for t in range(4):
        fr = [frames[t * B + i] for i in range(B)]
        det.enqueue(fr)
        a.update_from_detector(det, fr)
        got = det.fetch()
        xy = np.zeros((B, 20, 4), np.float32); cf = np.zeros((B, 20), np.float32); cl = np.zeros((B, 20), np.int32)
        cnt = np.zeros(B, np.int32)
        for i, d in enumerate(got):
            n = len(d)
            xy[i, :n], cf[i, :n], cl[i, :n], cnt[i] = d.xyxy, d.confidence, d.class_id, n
            refs[i].update(d.xyxy, d.confidence, d.class_id, R.describe(fr[i], d.xyxy)[0])
            total += n
        b.update_batch(xy, cf, cl, cnt, frames=fr)
        for i in range(B):
            sa, sb = a.snapshot(i), b.snapshot(i)
            assert R.snapshots_equal(sa, sb) is None, (t, i, R.snapshots_equal(sa, sb))
            assert R.snapshots_equal(sb, refs[i].snapshot()) is None, (t, i)
    assert total > 0
    assert all(v >= 0 for v in a.last_ms())
    a.close(); b.close(); det.close()


# ------------------------------------------------------------------------------------------------------------- limits
def test_limits_and_bad_arguments_return_codes(pkg):
    ffi = pkg._ffi
    L = ffi.lib()
    core = core_cls(pkg)(n_streams=1, max_tracks=4, max_dets=8, max_age=3, n_init=2, nn_budget=4)
    frame = R.render_scene([], [], 64, 96)
    xy = np.asarray([[4 + 11 * k, 5, 12 + 11 * k, 40] for k in range(8)], np.float32)
    one = np.ones(8, np.float32)
    zero = np.zeros(8, np.int32)
    for bad_n in (9, -1):                                   # more than max_dets / negative
        cnt = np.asarray([bad_n], np.int32)
        rc = L.rtmodt_deepsort_update_batch(core._h, ffi.ptr(np.zeros((1, 8, 4), np.float32)), ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt), None, 0, 0, 0, 0,
                                            None, None)
        assert rc == (ffi.E_CAPACITY if bad_n > 0 else ffi.E_INVALID)
    cnt = np.asarray([2], np.int32)
    args = (core._h, ffi.ptr(xy.reshape(1, 8, 4)), ffi.ptr(one), ffi.ptr(zero), ffi.ptr(cnt))
    assert L.rtmodt_deepsort_update_batch(*args, None, 0, 0, 0, 0, None, None) == ffi.E_INVALID                # neither frames nor descriptors
    fp, keep = ffi.frame_pointers([frame], ffi.MEM_HOST)[:2]
    emb = np.zeros((1, 8, 192), np.int8)
    assert L.rtmodt_deepsort_update_batch(*args, fp, 64, 96, 288, 0, ffi.ptr(emb), None) == ffi.E_INVALID     # both
    assert L.rtmodt_deepsort_update_batch(*args, fp, 64, 96, 100, 0, None, None) == ffi.E_INVALID              # pitch < 3w
    assert L.rtmodt_deepsort_update_batch(*args, fp, 64, 96, 288, 7, None, None) == ffi.E_INVALID              # mem_kind
    assert L.rtmodt_deepsort_state(core._h, 3, *([None] * 14)) == ffi.E_INVALID
    assert len(core.snapshot(0)["ids"]) == 0                 # none of the refused calls touched the state
    # more live tracks than max_tracks: sticky capacity error, no fault
    with pytest.raises(ffi.RtmodtError) as e:
        core.update(xy, one, zero, frame=frame)
    assert e.value.code == ffi.E_CAPACITY and "max_tracks" in e.value.msg
    core.close()
    # odd capacities: every state array still starts on its own 16-byte boundary
    _run_streams(pkg, ["tiny"] * 3, "frames", max_tracks=5, max_dets=3)
    # the contested-pair limit of lap.h: 50 tentative tracks against 50 detections that all overlap one another = 2500 admissible
    # pairs in the IoU stage, none isolated (> 2048): sticky capacity error, nothing faults, the handle can be reset
    core = core_cls(pkg)(n_streams=1, max_tracks=64, max_dets=64, max_age=3, n_init=3, nn_budget=4)
    crowd = np.asarray([[10 + 0.1 * k, 10 + 0.1 * k, 50 + 0.1 * k, 50 + 0.1 * k] for k in range(50)], np.float32)
    conf50, cls50 = np.full(50, 0.9, np.float32), np.zeros(50, np.int32)
    assert core.update(crowd, conf50, cls50, frame=frame) == 0 and len(core.snapshot(0)["ids"]) == 50
    with pytest.raises(ffi.RtmodtError) as e:
        core.update(crowd, conf50, cls50, frame=frame)
    assert e.value.code == ffi.E_CAPACITY and "contested" in e.value.msg
    with pytest.raises(ffi.RtmodtError) as e:                                     # sticky
        core.snapshot(0)
    assert e.value.code == ffi.E_CAPACITY
    core.reset()
    assert len(core.snapshot(0)["ids"]) == 0
    assert core.update(crowd[:3], conf50[:3], cls50[:3], frame=frame) == 0 and len(core.snapshot(0)["ids"]) == 3
    core.close()
    # the standalone entry points
    g = np.zeros((2, 4, 64), np.int8)
    d = np.zeros((3, 64), np.int8)
    out = np.zeros((2, 3), np.int32)
    assert L.rtmodt_appearance_dotmax(0, ffi.ptr(g), ffi.ptr(np.asarray([1, 5], np.int32)), 2, 4, ffi.ptr(d), 3, 64, ffi.ptr(out)) == ffi.E_INVALID
    assert L.rtmodt_appearance_dotmax(0, ffi.ptr(g), ffi.ptr(np.asarray([1, 1], np.int32)), 2, 4, ffi.ptr(d), 3, 100, ffi.ptr(out)) == ffi.E_INVALID
    assert L.rtmodt_appearance_dotmax(0, ffi.ptr(g), ffi.ptr(np.asarray([1, 1], np.int32)), 257, 4, ffi.ptr(d), 3, 64, ffi.ptr(out)) == ffi.E_CAPACITY
    assert L.rtmodt_appearance_dotmax(0, ffi.ptr(g), ffi.ptr(np.asarray([1, 1], np.int32)), 2, 129, ffi.ptr(d), 3, 64, ffi.ptr(out)) == ffi.E_CAPACITY
    assert L.rtmodt_appearance_dotmax(0, ffi.ptr(g), ffi.ptr(np.asarray([1, 1], np.int32)), 2, 4, ffi.ptr(d), 1025, 64, ffi.ptr(out)) == ffi.E_CAPACITY
    nb = np.asarray([1], np.int32)
    desc = np.zeros((1, 1, 192), np.int8)
    assert L.rtmodt_appearance_describe(0, fp, 1, 64, 96, 288, 0, ffi.ptr(xy), ffi.ptr(np.asarray([2], np.int32)), 1, ffi.ptr(desc), None) == ffi.E_CAPACITY
    assert L.rtmodt_appearance_describe(0, fp, 1, 64, 96, 10, 0, ffi.ptr(xy), ffi.ptr(nb), 1, ffi.ptr(desc), None) == ffi.E_INVALID
    assert L.rtmodt_appearance_describe(0, fp, 1, 64, 96, 288, 0, ffi.ptr(xy), ffi.ptr(nb), 1025, ffi.ptr(desc), None) == ffi.E_CAPACITY
    assert L.rtmodt_appearance_describe(0, fp, 65, 64, 96, 288, 0, ffi.ptr(xy), ffi.ptr(nb), 1, ffi.ptr(desc), None) == ffi.E_CAPACITY
    del keep


def test_iou_stage_at_the_contested_pair_limit(pkg):
    """32 tentative tracks against 64 detections that all overlap them: exactly 2048 admissible pairs, none isolated -- the most
    lap.h's edge array holds -- and the state equals the restatement bit for bit (tests/test_deepsort_cpu.py shows that frame's
    optimum unique and equal to scipy's).  One more track with a single pair into a contested column, 2049, is refused."""
    ffi = pkg._ffi
    params, frames = R.pair_limit_frames(False)
    core = core_cls(pkg)(n_streams=1, max_tracks=128, max_dets=64, **params)
    ref = R.DeepSortRef(**params)
    for f, (xy, cf, cl, desc) in enumerate(frames):
        ref.update(xy, cf, cl, desc)
        core.update(xy, cf, cl, embeddings=desc)
        assert R.snapshots_equal(core.snapshot(0), ref.snapshot()) is None, (f, R.snapshots_equal(core.snapshot(0), ref.snapshot()))
    assert len(ref.ids) == 64 and sum(h == 2 for h in ref.hits) == 32      # all 32 tracks matched, 32 detections left over
    core.reset()
    params, frames = R.pair_limit_frames(True)
    core.update(*frames[0][:3], embeddings=frames[0][3])
    assert len(core.snapshot(0)["ids"]) == 33
    with pytest.raises(ffi.RtmodtError) as e:
        core.update(*frames[1][:3], embeddings=frames[1][3])
    assert e.value.code == ffi.E_CAPACITY and "contested" in e.value.msg
    core.reset()                                               # the handle answers again
    xy, cf, cl, desc = frames[0]
    assert core.update(xy[:3], cf[:3], cl[:3], embeddings=desc[:3]) == 0 and len(core.snapshot(0)["ids"]) == 3
    core.close()


# -------------------------------------------------------------------------------------------------------------- facade
def test_facade_is_switch_free_on_the_rendered_crossing_scene(pkg):
    """DeepSortTracker.update on the rendered frames of the CPU behaviour test, descriptors computed on the GPU: the tracks it
    returns equal the restatement's and carry no identity switch."""
    params, frames = R.sequence_inputs("crossing")
    trk = pkg.DeepSortTracker(max_tracks=32, max_dets=16, **params)
    ref = R.DeepSortRef(**params)
    hyp, gt = [], []
    for f, (img, xy, cf, cl, ids) in enumerate(frames):
        out = trk.update(pkg.Detections(xy, cf, cl), frame=img)
        want = ref.tracks_out(ref.update(xy, cf, cl, R.describe(img, xy)[0]))
        assert [t.track_id for t in out] == [i for i, _ in want], f
        assert all(np.array_equal(t.xyxy.view(np.int32), b.view(np.int32)) for t, (_, b) in zip(out, want)), f
        hyp += [[f + 1, t.track_id, t.xyxy[0], t.xyxy[1], t.xyxy[2] - t.xyxy[0], t.xyxy[3] - t.xyxy[1]] for t in out]
        gt += [[f + 1, int(o), b[0], b[1], b[2] - b[0], b[3] - b[1]] for o, b in zip(ids, xy)]
    res = eval_ref.mot_ref(np.asarray(gt, np.float64), np.asarray(hyp, np.float64))
    assert res["num_switches"] == 0 and res["num_matches"] > 0.8 * res["num_objects"], res["num_switches"]
    assert len(out[0].trail) > 1 and trk.update(pkg.Detections(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))) == []
    with pytest.raises(ValueError, match="exactly one"):
        trk.update(pkg.Detections(frames[0][1], frames[0][2], frames[0][3]))
    trk.close()


@pytest.mark.parametrize("handoff", [True, False])
def test_pipeline_run_with_deepsort_and_zone_events(pkg, wdir, tmp_path, handoff):
    """pipeline.run(DeepSortTracker, event_engine=ZoneEventEngine), with and without the device hand-off of the detections: the
    frame reaches the tracker, the tracks reach the zone engine as a list (process(), never the ByteTrack-only process_tracker), and
    a whole-frame zero-dwell zone fires once per returned track id -- the ids a hand-driven replay of the same loop returns."""
    path = os.path.join(str(wdir), "yolov8n_320_noise_pipe.rtw")
    if not os.path.exists(path):
        pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    params = dict(max_age=4, n_init=2, nn_budget=8, min_confidence=0.0, max_tracks=128, max_dets=20)
    zones = [{"name": "frame", "polygon": [[0, 0], [320, 0], [320, 320], [0, 320]], "dwell_time_sec": 0.0, "cooldown_sec": 1e9}]
    eng = pkg.events.ZoneEventEngine(zones, log_path=str(tmp_path / "events.jsonl"))
    frames = pkg.synth.frames(3, 320, 320, seed=5)
    trk = pkg.DeepSortTracker(**params)
    prof = pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=2, log_interval=1000)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), det, trk, prof, max_frames=9, event_engine=eng, device_handoff=handoff)
    trk2 = pkg.DeepSortTracker(**params)
    reported, last = set(), []
    for i in range(9):
        last = trk2.update(det.detect(frames[i % 3]), frame=frames[i % 3])
        reported |= {t.track_id for t in last}
    assert len(reported) > 0 and out["events"] == len(reported) and out["last_tracks"] == len(last)
    assert R.snapshots_equal(trk._core.snapshot(0), trk2._core.snapshot(0)) is None
    with pytest.raises(TypeError, match="process\\(tracks, frame_id\\)"):
        eng.process_tracker(trk, 99)
    trk.close(); trk2.close(); eng.close(); det.close()
