"""GPU: the re-identification embedder (csrc/reid.hip) against its restatement (tests/reid_ref.py).  The crop and the int8
quantiser are compared exactly; every network tap is compared with float64 computed from the device's own previous tap, within
tolerances that come from the fp16 contract's emulator (reid_ref.TOL_TAP), never from the device's own error; six deliberate
defects of the reference must each throw the device out of its tolerance by 5x.  PARITY UNPINNED: torchreid / cv2 /
deep_sort_realtime are installed nowhere this runs."""
import ctypes as C
import os
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deepsort_ref as DR  # noqa: E402
import reid_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = ((80, 96, 7, 1), (47, 33, 0, 2))            # (h, w, row padding, seed): a 96 x 80 frame with a padded pitch, a 33 x 47 one


@pytest.fixture(scope="module")
def wts(pkg):
    return pkg.reid_weights.synthetic(0)


@pytest.fixture(scope="module")
def wpath(pkg, wts, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("reid") / "osnet_synth.rtreid")
    pkg.reid_weights.save(path, wts)
    return path


@pytest.fixture(scope="module")
def eng(pkg, wpath):
    e = pkg.tracking.ReidEmbedder(wpath, max_boxes=24, max_frames=3)
    yield e
    e.close()


def _embed_scene(pkg, eng, h, w, pad, seed, counts, kind):
    buf, view = R.scene_frame(h, w, pad, seed)
    boxes = R.scene_boxes(h, w, seed)
    xy = np.zeros((len(counts), len(boxes), 4), np.float32)
    xy[:] = boxes
    if kind == "host":
        feat, desc = eng.embed([view] * len(counts), xy, counts)
    else:
        dev = pkg._ffi.DeviceBuffer(buf.nbytes)
        dev.upload(buf)
        feat, desc = eng.embed([dev.ptr] * len(counts), xy, counts, mem_kind=pkg._ffi.MEM_DEVICE, height=h, width=w, stride=buf.strides[0])
        assert np.array_equal(dev.download().reshape(buf.shape), buf), "the frame was written to"
        dev.free()
    return view, boxes, feat, desc


# ------------------------------------------------------------------------------------------------------------ 1: crop
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("scene", SCENES)
def test_crop_tap_is_bit_exact(pkg, eng, scene, kind):
    counts = [17, 1, 0]
    view, boxes, feat, desc = _embed_scene(pkg, eng, *scene, counts, kind)
    crops = eng.tap("crop")
    seen = 0
    for f, n in enumerate(counts):
        for b in range(len(boxes)):
            want = R.crop(view, boxes[b]) if b < n else None
            if want is None:
                assert not desc[f, b].any() and not feat[f, b].any(), (f, b)
            else:
                assert np.array_equal(crops[f, b], want), (f, b, np.argwhere(crops[f, b] != want)[:3])
                assert desc[f, b].any()
                seen += 1
    assert seen == 17 - len(R.EMPTY_ROWS) + 1


# ------------------------------------------------------------------------------------------- 2-4: the network's taps
@pytest.fixture(scope="module")
def run(pkg, eng, wts):
    """One embed of the 17 boxes of both scenes (two calls: frames of a call share their size); the device's taps of the valid
    boxes, the float64 reference of each tap computed from the device's previous tap, and the free-running float64 network."""
    taps = {k: [] for k in R.TAPS}
    feats, descs = [], []
    for scene in SCENES:
        view, boxes, feat, desc = _embed_scene(pkg, eng, *scene, [17], "host")
        ok = [b for b in range(17) if R.crop(view, boxes[b]) is not None]
        for k in R.TAPS:
            taps[k].append(eng.tap(k)[0, ok])
        feats.append(feat[0, ok]); descs.append(desc[0, ok])
    taps = {k: np.concatenate(v) for k, v in taps.items()}
    out = {"dev": taps, "feat": np.concatenate(feats), "desc": np.concatenate(descs), "free": R.forward(taps["crop"], wts)}
    assert np.array_equal(out["feat"], taps["feat"])
    out["forced"] = {k: R.step(k, taps[R.TAPS[i]], wts) for i, k in enumerate(R.TAPS[1:])}
    return out


def _emulator_forced(pkg, wts, k, prev):
    """The contract's emulator (package, torch float32, fp16 roundings) on the device's previous tap."""
    import torch
    RW = pkg.reid_weights
    x = RW.normalize(prev) if k == "conv1" else prev.astype(np.float32)
    y = RW.torch_step(k, torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))), wts, torch.float32, emulate=True).numpy().astype(np.float64)
    return y.transpose(0, 2, 3, 1) if y.ndim == 4 else y


@pytest.mark.parametrize("k", R.TAPS[1:])
def test_every_tap_teacher_forced_against_float64(pkg, wts, run, k):
    dev, ref = run["dev"][k].astype(np.float64), run["forced"][k]
    prev = run["dev"][R.TAPS[R.TAPS.index(k) - 1]]
    scale = np.abs(ref).max()
    err = np.abs(dev - ref).max() / scale
    emu = np.abs(_emulator_forced(pkg, wts, k, prev) - ref).max() / scale
    print(f"reid tap {k}: device {err:.3e}, emulator {emu:.3e}, tolerance {R.TOL_TAP[k]:.3e} (x max|ref64| = {scale:.3f})")
    assert scale > 0.5 and np.isfinite(dev).all()
    assert err <= R.TOL_TAP[k], (k, err, R.TOL_TAP[k])


def test_free_running_feature_and_descriptor(run):
    feat, ref = run["feat"].astype(np.float64), run["free"]["feat"]
    scale = np.abs(ref).max()
    err = np.abs(feat - ref).max() / scale
    cos = (feat * ref).sum(1) / np.sqrt((feat * feat).sum(1) * (ref * ref).sum(1))
    print(f"reid free-running feat: {err:.3e} of max|ref64| = {scale:.3f}, tolerance {R.TOL_FEAT:.3e}; cosine min {cos.min():.8f}")
    assert np.array_equal(run["desc"], R.quantize_rows(run["feat"]))               # exact, from the device's own feature
    assert err <= R.TOL_FEAT
    lsb = R.lsb_bound(ref, R.TOL_FEAT * scale)
    d = np.abs(run["desc"].astype(int) - R.quantize_rows(ref.astype(np.float32)).astype(int)).max()
    print(f"reid desc: {d} LSB from the quantised float64 feature, bound {lsb}")
    assert d <= lsb and cos.min() > 0.9999


@pytest.mark.parametrize("m", R.MUTATIONS)
def test_tolerances_see_real_defects(pkg, wts, run, m):
    """The float64 reference is computed wrongly in one way; the device must then MISS the tolerance at the first affected tap by at
    least 5x (and meet it against the right reference: test_every_tap_teacher_forced_against_float64)."""
    k = R.FIRST_TAP[m]
    w = wts
    if m == "eps1e-3":
        RW = pkg.reid_weights
        w = RW.round_stored(RW.from_state_dict(RW.synthetic_state_dict(0), eps=1e-3))
    ref = R.step(k, run["dev"][R.TAPS[R.TAPS.index(k) - 1]], w, mutate=m)
    err = np.abs(run["dev"][k].astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"reid mutation {m} at {k}: device is {err:.3e} from the mutant = {err / R.TOL_TAP[k]:.0f} x tolerance")
    assert err >= 5 * R.TOL_TAP[k], (m, err)


# ----------------------------------------------------------------------------------------------- 5: batch independence
def test_descriptor_does_not_depend_on_the_batch(pkg, wpath):
    h, w, pad, seed = SCENES[0]
    _, view = R.scene_frame(h, w, pad, seed)
    others = R.scene_boxes(h, w, seed)
    box = others[0]
    rng = np.random.default_rng(9)
    e = pkg.tracking.ReidEmbedder(wpath, max_boxes=30, max_frames=3)
    f1, d1 = e.embed([view], [box[None]])
    assert d1[0, 0].any()
    f17, d17 = e.embed([view], [np.concatenate([others[1:9], box[None], others[9:]])])            # among 17, slot 8
    many = [np.concatenate([others, others[rng.integers(0, 17, 13)]]) for _ in range(3)]            # 30 boxes per frame
    many[0] = many[0][:30]; many[1] = many[1][:20]; many[2] = many[2][:15]                            # 65 boxes across 3 frames
    many[2][11] = box
    f65, d65 = e.embed([view, view, view], many)
    for f, d, where in ((f17, d17, (0, 8)), (f65, d65, (2, 11))):
        assert np.array_equal(d[where], d1[0, 0]) and np.array_equal(f[where].view(np.int32), f1[0, 0].view(np.int32)), where
    assert sum(len(m) for m in many) == 65
    assert not d65[1, 20:].any() and not d65[2, 15:].any() and not f65[1, 20:].any()                 # rows past n_boxes
    for r in R.EMPTY_ROWS:
        assert not d65[0, r].any() and not f65[0, r].any()                                           # rows of empty boxes
    with pytest.raises(pkg._ffi.RtmodtError) as err:
        e.embed([view] * 4, [box[None]] * 4)
    assert err.value.code == pkg._ffi.E_CAPACITY
    with pytest.raises(pkg._ffi.RtmodtError) as err:
        e.embed([view], [np.repeat(box[None], 31, 0)])
    assert err.value.code == pkg._ffi.E_CAPACITY
    assert all(v >= 0 for v in e.last_ms())
    e.close()


# --------------------------------------------------------------------------------------------------- 6: in the tracker
def _video(seed):
    scene, h, w = DR.random_scene(seed, frames=20, n_obj=6, h=240, w=320, speed=6.0)
    return [(DR.render_scene(xy, col, h, w, seed=500 + seed + f), xy, cf, cl) for f, (xy, cf, cl, ids, col) in enumerate(scene)]


def test_tracker_state_equals_restatement_fed_the_embedders_rows(pkg, wpath, tmp_path_factory):
    core_cls = import_module(pkg.__name__ + ".tracking.deepsort")._DeepSortCore
    S, N = 2, 8
    params = dict(max_age=6, n_init=2, nn_budget=8)
    vids = [_video(3), _video(4)]
    core = core_cls(n_streams=S, max_tracks=32, max_dets=N, embedder=wpath, **params)
    assert core.dim == 512
    refs = [DR.DeepSortRef(dim=512, **params) for _ in range(S)]
    e = pkg.tracking.ReidEmbedder(wpath, max_boxes=N, max_frames=S)
    hist = core_cls(n_streams=S, max_tracks=32, max_dets=N, **params)                    # a colorhist handle in the same process
    hist_refs = [DR.DeepSortRef(**params) for _ in range(S)]
    for f in range(20):
        xy = np.zeros((S, N, 4), np.float32); cf = np.zeros((S, N), np.float32); cl = np.zeros((S, N), np.int32)
        cnt = np.zeros(S, np.int32)
        frames = []
        for s in range(S):
            img, b, c, k = vids[s][f]
            xy[s, :len(b)], cf[s, :len(b)], cl[s, :len(b)], cnt[s] = b, c, k, len(b)
            frames.append(img)
        _, desc = e.embed(frames, xy, cnt)
        core.update_batch(xy, cf, cl, cnt, frames=frames)
        hist.update_batch(xy, cf, cl, cnt, frames=frames)
        for s in range(S):
            n = cnt[s]
            refs[s].update(xy[s, :n], cf[s, :n], cl[s, :n], desc[s, :n])
            hist_refs[s].update(xy[s, :n], cf[s, :n], cl[s, :n], DR.describe(frames[s], xy[s, :n])[0])
            diff = DR.snapshots_equal(core.snapshot(s), refs[s].snapshot())
            assert diff is None, (f, s, diff)
            assert DR.snapshots_equal(hist.snapshot(s), hist_refs[s].snapshot()) is None, (f, s)
    assert all(len(r.ids) >= 5 and max(r.hits) > 10 for r in refs)
    emb = np.zeros((S, N, 512), np.int8)
    with pytest.raises(pkg._ffi.RtmodtError) as err:                                       # never both, and never caller rows on this handle
        core.update_batch(xy, cf, cl, cnt, embeddings=emb)
    assert err.value.code == pkg._ffi.E_INVALID and "embedder network" in err.value.msg
    core.close(); hist.close(); e.close()


def test_update_from_detector_agrees_with_update_batch(pkg, wpath, tmp_path_factory):
    core_cls = import_module(pkg.__name__ + ".tracking.deepsort")._DeepSortCore
    path = str(tmp_path_factory.mktemp("reid_det") / "yolov8n_320_noise.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    B = 2
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=12, batch=B, warmup=False, autotune=False)
    params = dict(max_age=4, n_init=2, nn_budget=8, min_confidence=0.0)
    a = core_cls(n_streams=B, max_tracks=64, max_dets=12, embedder=wpath, **params)
    b = core_cls(n_streams=B, max_tracks=64, max_dets=12, embedder=wpath, **params)
    frames = pkg.synth.frames(3 * B, 320, 320, seed=77)
    total = 0
    for t in range(3):
        fr = [frames[t * B + i] for i in range(B)]
        det.enqueue(fr)
        a.update_from_detector(det, fr)
        got = det.fetch()
        xy = np.zeros((B, 12, 4), np.float32); cf = np.zeros((B, 12), np.float32); cl = np.zeros((B, 12), np.int32)
        cnt = np.zeros(B, np.int32)
        for i, d in enumerate(got):
            n = len(d)
            xy[i, :n], cf[i, :n], cl[i, :n], cnt[i] = d.xyxy, d.confidence, d.class_id, n
            total += n
        b.update_batch(xy, cf, cl, cnt, frames=fr)
        for i in range(B):
            diff = DR.snapshots_equal(a.snapshot(i), b.snapshot(i))
            assert diff is None, (t, i, diff)
    assert total > 0 and a.snapshot(0)["gallery"].any()
    a.close(); b.close(); det.close()


# ------------------------------------------------------------------------------------- 7: what this embedder exists for
def test_deepsort_tracker_constructs_and_tracks_with_the_network(pkg, wpath):
    h = C.c_void_p()
    cfg = pkg._ffi.DeepSortCfg(0.2, 0.3, 0.7, 70, 3, 100, wpath.encode(), 0, 32, 16, 1, 0)
    assert pkg._ffi.lib().rtmodt_deepsort_create(C.byref(cfg), C.byref(h)) == pkg._ffi.OK and h.value
    pkg._ffi.lib().rtmodt_deepsort_destroy(h)
    trk = pkg.DeepSortTracker(embedder=wpath, max_age=6, n_init=2, nn_budget=8, max_tracks=32, max_dets=8)
    assert trk.embedder == wpath and trk.needs_frame and trk._core.dim == 512
    cfgd = pkg.DeepSortTracker.from_config({"algorithm": "deepsort", "deepsort": {"max_age": 6, "embedder": wpath}}, max_tracks=32, max_dets=8)
    assert cfgd.embedder == wpath
    cfgd.close()
    sized = pkg.DeepSortTracker(embedder=wpath)                                         # a network's default: 128 slots of 2.9 MB, not 1024
    assert sized._core.max_dets == 128 and pkg.DeepSortTracker.__init__.__kwdefaults__["max_dets"] is None
    sized.close()
    ids = set()
    for img, xy, cf, cl in _video(3):
        out = trk.update(pkg.Detections(xy, cf, cl), frame=img)
        ids |= {t.track_id for t in out}
    assert len(out) >= 4 and len(ids) >= 4 and len(out[0].trail) > 1
    with pytest.raises(ValueError, match="embedder network"):
        trk.update(pkg.Detections(xy, cf, cl), embeddings=np.zeros((len(xy), 512), np.int8))
    trk.close()
