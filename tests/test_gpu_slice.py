"""GPU: sliced inference (csrc/slice.hip) against the plain restatement tests/slice_ref.py, bit for bit -- the tile bytes of
slice_gather, the merge kernel alone on seeded candidates, and the whole path (gather -> detector -> merge -> tracker) against
a plain detector fed the restated tiles.  Floats are compared as int32 bit patterns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slice_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def same(a, b):
    return (np.array_equal(bits(a.xyxy), bits(b.xyxy)) and np.array_equal(bits(a.confidence), bits(b.confidence))
            and np.array_equal(a.class_id, b.class_id))


class RawSlicer:
    """The C handle alone (no detector)."""

    def __init__(self, pkg, max_det=16, **kw):
        self.F, self.S = pkg._ffi, pkg.detection.sliced
        self.cfg = self.S.slice_cfg(**kw)
        self.h = C.c_void_p()
        self.F.check(self.F.lib().rtmodt_slicer_create(C.byref(self.cfg), max_det, C.byref(self.h)))
        t, i, w, h = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.F.check(self.F.lib().rtmodt_slicer_info(self.h, C.byref(t), C.byref(i), C.byref(w), C.byref(h)))
        self.T, self.I, self.te = t.value, i.value, (w.value, h.value)

    def gather(self, ptrs, n, pitch, kind):
        out = np.full((n * self.I, self.te[1], self.te[0], 3), 0xA5, np.uint8)
        self.F.check(self.F.lib().rtmodt_slicer_gather(self.h, ptrs, n, pitch, kind, self.F.ptr(out)))
        return out

    def close(self):
        self.F.lib().rtmodt_slicer_destroy(self.h)


# ------------------------------------------------------------------ gather
GATHER = [  # frame (w, h), tile (w, h), overlap, frames, extra pitch bytes
    ((96, 80), (64, 64), 16, 2, 0),
    ((97, 83), (64, 48), 15, 2, 7),            # odd width, pitch 3w + 7, window starts of every alignment
    ((50, 40), (64, 64), 16, 1, 0),            # frame smaller than the tile: one tile, the frame itself
    ((320, 240), (128, 128), 32, 3, 0),
]


@pytest.mark.parametrize("overview", [True, False], ids=["overview", "tiles-only"])
@pytest.mark.parametrize("frame,tile,ov,n,pad", GATHER, ids=[f"{g[0][0]}x{g[0][1]}" for g in GATHER])
def test_gather_equals_the_restatement(pkg, frame, tile, ov, n, pad, overview):
    w, h = frame
    frames = pkg.synth.structured_frames(n, h, w, seed=w + h)
    want = R.gather(frames, tile[0], tile[1], ov, ov, overview)
    s = RawSlicer(pkg, frame_size=frame, tile=tile, overlap=(ov, ov), overview=overview, max_frames=n)
    assert (s.T, s.I, s.te) == (len(R.grid(w, h, *tile, ov, ov)[0]), want.shape[0] // n, (want.shape[2], want.shape[1]))
    pitch = 3 * w + pad
    raw = np.full((n, h, pitch), 0x5A, np.uint8)
    raw[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
    host = [np.lib.stride_tricks.as_strided(raw[i], (h, w, 3), (pitch, 3, 1)) for i in range(n)]
    fp, keep, fh, fw, p = pkg._ffi.frame_pointers(host, pkg._ffi.MEM_HOST)
    assert (fh, fw, p) == (h, w, pitch)
    got = s.gather(fp, n, pitch, pkg._ffi.MEM_HOST)
    assert np.array_equal(got, want), "host frames"
    # device frames, the first one byte off a 16-byte boundary so that no row of it starts aligned
    buf = pkg._ffi.DeviceBuffer(raw.nbytes + 16)
    buf.upload(raw, 1)
    ptrs = (C.c_void_p * n)(*[buf.ptr + 1 + i * h * pitch for i in range(n)])
    got = s.gather(ptrs, n, pitch, pkg._ffi.MEM_DEVICE)
    assert np.array_equal(got, want), "device frames"
    buf.free()
    s.close()


# ------------------------------------------------------------------ merge kernel alone
def clustered_frame(rng, geom, overview, max_det, counts, n_clusters=5, n_cls=2):
    """Per-image detections of one frame, in image coordinates: boxes scattered around a few cluster centres of the frame (so that
    chains of overlaps exist), each written into an image that sees it; a block of identical scores; identical boxes."""
    W, H = geom[0], geom[1]
    tiles, (te_w, te_h) = R.grid(*geom)
    I = len(tiles) + int(overview)
    gain, pad_x, pad_y = R.overview_geometry(W, H, te_w, te_h)
    xy, cf, cl = np.zeros((I, max_det, 4), F32), np.zeros((I, max_det), F32), np.zeros((I, max_det), np.int32)
    centres = [(rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H, rng.uniform(8, 0.3 * min(te_w, te_h))) for _ in range(n_clusters)]
    for j in range(I):
        for s in range(counts[j]):
            cx, cy, r = centres[rng.integers(n_clusters)]
            if j < len(tiles):                                       # pull the centre into the tile, as a detector only sees what is inside
                cx = min(max(cx, tiles[j][0] + 2), tiles[j][0] + te_w - 2)
                cy = min(max(cy, tiles[j][1] + 2), tiles[j][1] + te_h - 2)
            jit = rng.normal(0, 0.15 * r, 4)
            b = np.array([cx - r + jit[0], cy - r + jit[1], cx + r + jit[2], cy + r + jit[3]])
            if j < len(tiles):
                b -= [tiles[j][0], tiles[j][1]] * 2
                b = np.clip(b, 0, [te_w, te_h] * 2)
            else:
                b = b * float(gain) + [float(pad_x), float(pad_y)] * 2
            xy[j, s] = b.astype(F32)
            cf[j, s] = F32(rng.uniform(0.05, 0.95))
            cl[j, s] = rng.integers(n_cls)
            if s % 3 == 1:
                cf[j, s] = F32(0.5)                                   # the block of identical scores
            if s % 4 == 3:
                xy[j, s] = xy[j, s - 1]                               # identical boxes (the class may differ)
    return xy, cf, cl


def ref_frames(geom, overview, xy, cf, cl, counts, **kw):
    tiles, _ = R.grid(*geom)
    I = len(tiles) + int(overview)
    out = []
    for f in range(len(counts) // I):
        images = [(xy[i, :counts[i]], cf[i, :counts[i]], cl[i, :counts[i]]) for i in range(f * I, (f + 1) * I)]
        out.append(R.merge(R.to_frame(images, *geom, overview=overview), **kw))
    return out


def check_frames(got, want):
    merged = plain = 0
    for f, (g, w) in enumerate(zip(got, want)):
        assert len(g[1]) == len(w[1]), (f, len(g[1]), len(w[1]))
        assert np.array_equal(bits(g[0]), bits(w[0])), (f, "boxes")
        assert np.array_equal(bits(g[1]), bits(w[1])), (f, "conf")
        assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]), (f, "cls / n_merged")
        merged += int((w[3] > 0).sum())
        plain += int((w[3] == 0).sum())
    assert merged > 0 and plain > 0, (merged, plain)              # neither path is vacuous


COMBOS = [(m, k, a) for m in (R.NMM, R.NMS) for k in (R.IOS, R.IOU) for a in (False, True)]


@pytest.mark.parametrize("mode,metric,agnostic", COMBOS, ids=[f"{m}-{k}-{'agnostic' if a else 'per-class'}" for m, k, a in COMBOS])
def test_merge_kernel_equals_the_restatement(pkg, mode, metric, agnostic):
    """Six frames of unlike counts in ONE launch (0, 1 and 7 candidates, a full frame, two ragged ones), 10 images x 16 slots each."""
    S = pkg.detection.sliced
    geom, overview, max_det = (160, 120, 64, 64, 16, 16), True, 16
    rng = np.random.default_rng(17)
    I = len(R.grid(*geom)[0]) + 1
    assert I == 10
    per_frame = [[0] * I, [0] * 4 + [1] + [0] * 5, [2, 0, 1, 0, 3, 0, 0, 0, 0, 1], [max_det] * I,
                 list(rng.integers(0, max_det + 1, I)), list(rng.integers(0, 6, I))]
    parts = [clustered_frame(rng, geom, overview, max_det, c) for c in per_frame]
    xy, cf, cl = (np.concatenate([p[k] for p in parts]) for k in range(3))
    counts = np.array([c for f in per_frame for c in f], np.int32)
    for max_out in (300, 5):
        cfg = S.slice_cfg(geom[:2], geom[2:4], geom[4:6], overview, mode, metric, 0.5, agnostic, max_out)
        got = S.slice_merge(cfg, xy, cf, cl, counts)
        want = ref_frames(geom, overview, xy, cf, cl, counts, mode=mode, metric=metric, thresh=0.5, agnostic=agnostic, max_out=max_out)
        assert [len(w[1]) for w in want[:3]] == [0, 1, min(max_out, len(want[2][1]))] and len(want[2][1]) >= 2
        check_frames(got, want)


@pytest.mark.parametrize("mode,metric,agnostic", COMBOS, ids=[f"{m}-{k}-{'agnostic' if a else 'per-class'}" for m, k, a in COMBOS])
def test_merge_kernel_at_the_candidate_cap(pkg, mode, metric, agnostic):
    """8192 candidates = 64 images x 128 slots, every slot taken: the full LDS sort, the first 16 keepers."""
    S = pkg.detection.sliced
    geom, overview, max_det, max_out = (512, 512, 64, 64, 0, 0), False, 128, 16
    rng = np.random.default_rng(23)
    assert len(R.grid(*geom)[0]) == 64
    xy, cf, cl = clustered_frame(rng, geom, overview, max_det, [max_det] * 64, n_clusters=40)
    for s in range(max_det):                                      # image 0: 3 x 3 boxes on a 4-pixel pitch, no two of them overlap
        xy[0, s] = [4 * (s % 16), 4 * (s // 16), 4 * (s % 16) + 3, 4 * (s // 16) + 3]
    cf[cf > F32(0.9)] = F32(0.9)                                   # the top of the order is one long tie, image 0 first
    counts = np.full(64, max_det, np.int32)
    cfg = S.slice_cfg(geom[:2], geom[2:4], geom[4:6], overview, mode, metric, 0.5, agnostic, max_out)
    got = S.slice_merge(cfg, xy, cf, cl, counts)
    want = ref_frames(geom, overview, xy, cf, cl, counts, mode=mode, metric=metric, thresh=0.5, agnostic=agnostic, max_out=max_out)
    assert len(want[0][1]) == max_out
    check_frames(got, want)
    with pytest.raises(pkg._ffi.RtmodtError) as e:                 # one slot more per image is refused, nothing is launched
        S.slice_merge(cfg, np.zeros((64, 129, 4), F32), np.zeros((64, 129), F32), np.zeros((64, 129), np.int32), np.zeros(64, np.int32))
    assert e.value.code == pkg._ffi.E_CAPACITY


# ------------------------------------------------------------------ end to end
FRAME, TILE, OVERLAP, STREAMS = (560, 480), (320, 320), (64, 64), 2
#: chosen on the GPU so that the synthetic network yields per-tile detections that merge (asserted below)
CONF, MATCH = 0.05, 0.1
GEOM = (*FRAME, *TILE, *OVERLAP)


@pytest.fixture(scope="module")
def wpath(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_slice")), "yolov8s_320_noise.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("s", input_size=320), "s")
    return path


def sliced(pkg, wpath, **kw):
    kw.setdefault("streams", STREAMS)
    return pkg.SlicedDetector(wpath, frame_size=FRAME, tile=TILE, overlap=OVERLAP, overview=True, match_threshold=MATCH, confidence=CONF,
                              autotune=False, warmup=False, **kw)


@pytest.fixture(scope="module")
def frames(pkg):
    return pkg.synth.structured_frames(8, FRAME[1], FRAME[0], seed=41)


@pytest.fixture(scope="module")
def host_run(pkg, wpath, frames):
    """Four host-fed batches of two frames: (merged detections, per-tile detections, n_merged) per frame, computed once."""
    sd = sliced(pkg, wpath)
    out = []
    for t in range(4):
        dets = sd.detect_batch(list(frames[2 * t:2 * t + 2]))
        out += [(dets[i], sd.last_tiles[i], sd.n_merged[i]) for i in range(2)]
    assert sd.grid() == R.grid(*GEOM) and sd.images_per_frame == 5
    sd.close()
    return out


def test_per_tile_detections_equal_a_plain_detector_on_the_restated_tiles(pkg, wpath, frames, host_run):
    det = pkg.Detector(wpath, input_size=TILE, confidence=CONF, batch=10, autotune=False, warmup=False)
    total = 0
    for t in range(4):
        images = R.gather(frames[2 * t:2 * t + 2], *TILE, *OVERLAP, True)
        assert images.shape == (10, 320, 320, 3)
        ref = det.detect_batch(list(images))
        for i in range(10):
            assert same(host_run[2 * t + i // 5][1][i % 5], ref[i]), (t, i)
            total += len(ref[i])
    det.close()
    assert total > 0


def test_merged_output_equals_the_restated_merge(host_run):
    total = merged = 0
    for f, (dets, tiles, nm) in enumerate(host_run):
        images = [(d.xyxy, d.confidence, d.class_id) for d in tiles]
        xy, cf, cl, n = R.merge(R.to_frame(images, *GEOM), mode=R.NMM, metric=R.IOS, thresh=MATCH, agnostic=False, max_out=300)
        assert len(dets) == len(cf), (f, len(dets), len(cf))
        assert np.array_equal(bits(dets.xyxy), bits(xy)) and np.array_equal(bits(dets.confidence), bits(cf)), f
        assert np.array_equal(dets.class_id, cl) and np.array_equal(nm, n), f
        total += sum(len(d) for d in tiles)
        merged += int(n.sum())
    print(f"per-tile detections {total}, absorbed {merged}, merged detections {sum(len(h[0]) for h in host_run)}")
    assert total > 0 and merged > 0


def test_device_frames_and_two_batches_in_flight(pkg, wpath, frames, host_run):
    sd = sliced(pkg, wpath)
    buf = pkg._ffi.DeviceBuffer(frames.nbytes)
    buf.upload(frames)
    per = frames[0].nbytes
    got = []
    sd.enqueue([buf.ptr + i * per for i in (0, 1)])
    for t in range(1, 4):
        sd.enqueue([buf.ptr + (2 * t + i) * per for i in (0, 1)])            # t in flight behind t - 1
        got.append((sd.fetch(), sd.last_tiles, sd.n_merged))
    got.append((sd.fetch(), sd.last_tiles, sd.n_merged))
    for t in range(4):
        for i in range(2):
            want = host_run[2 * t + i]
            assert same(got[t][0][i], want[0]) and np.array_equal(got[t][2][i], want[2]), (t, i)
            assert all(same(a, b) for a, b in zip(got[t][1][i], want[1])), (t, i)
    buf.free()
    sd.close()


def test_tracker_from_sliced_equals_tracker_fed_the_fetched_arrays(pkg, wpath, frames):
    from importlib import import_module
    from oracle import tracker_oracle as T
    core_cls = import_module(pkg.__name__ + ".tracking.tracker")._ByteTrackCore
    sd = sliced(pkg, wpath)
    a = core_cls(track_thresh=CONF, n_streams=2, max_dets=sd.max_out, max_tracks=512)
    b = core_cls(track_thresh=CONF, n_streams=2, max_dets=sd.max_out, max_tracks=512)
    for t in range(4):
        sd.enqueue(list(frames[2 * t:2 * t + 2]))
        a.update_from_sliced(sd)
        dets = sd.fetch()
        xy, cf, cl = np.zeros((2, sd.max_out, 4), F32), np.zeros((2, sd.max_out), F32), np.zeros((2, sd.max_out), np.int32)
        for i, d in enumerate(dets):
            xy[i, :len(d)], cf[i, :len(d)], cl[i, :len(d)] = d.xyxy, d.confidence, d.class_id
        b.update_batch(xy, cf, cl, [len(d) for d in dets])
    n = 0
    for i in range(2):
        assert np.array_equal(T.state_digest(a.snapshot(i)), T.state_digest(b.snapshot(i))), i
        n += len(a.snapshot(i)["ids"])
    assert n > 0
    # the facade, one stream: the device hand-over against update() fed the fetched detections
    trk, ref = (pkg.MultiObjectTracker("bytetrack", track_thresh=CONF, max_dets=sd.max_out) for _ in range(2))
    one = sliced(pkg, wpath, streams=1)
    for t in range(2):
        one.enqueue([frames[t]])
        assert trk.update_from_sliced(one) == []
        ref.update(one.fetch()[0])
    assert np.array_equal(T.state_digest(trk._core.snapshot()), T.state_digest(ref._core.snapshot())) and len(trk._core.snapshot()["ids"]) > 0
    one.close(); a.close(); b.close(); sd.close()


# ------------------------------------------------------------------ refusals
def test_refusals_return_their_codes_and_the_next_call_works(pkg, wpath, frames):
    F = pkg._ffi
    L = F.lib()
    with pytest.raises(F.RtmodtError) as e:                          # overlap >= tile: refused at create
        pkg.SlicedDetector(wpath, frame_size=FRAME, tile=TILE, overlap=(320, 64), autotune=False, warmup=False)
    assert e.value.code == F.E_INVALID
    sd = sliced(pkg, wpath)
    ref = sd.detect_batch(list(frames[:2]))
    fp, keep, h, w, pitch = F.frame_pointers(list(frames[:2]), F.MEM_HOST)
    # a detector whose batch holds one frame's images only
    small = pkg.Detector(wpath, input_size=TILE, confidence=CONF, batch=5, autotune=False, warmup=False)
    assert L.rtmodt_slicer_enqueue(sd._h, small.model.handle, fp, 2, pitch, F.MEM_HOST) == F.E_CAPACITY and b"detector batch 5" in L.rtmodt_last_error()
    F.check(L.rtmodt_slicer_enqueue(sd._h, small.model.handle, fp, 1, pitch, F.MEM_HOST))      # one frame fits it
    n, tn = np.zeros(2, np.int32), np.zeros(5, np.int32)
    xy, cf = np.zeros((2, sd.max_out, 4), F32), np.zeros((2, sd.max_out), F32)
    txy, tcf, tcl = np.zeros((5, 100, 4), F32), np.zeros((5, 100), F32), np.zeros((5, 100), np.int32)
    F.check(L.rtmodt_slicer_fetch(sd._h, small.model.handle, F.ptr(xy), F.ptr(cf), None, None, F.ptr(n), F.ptr(txy), F.ptr(tcf), F.ptr(tcl), F.ptr(tn)))
    # (a detector of another batch size runs other conv tiles: its detections need not equal `ref`'s bit for bit; the merge of its own do)
    want = R.merge(R.to_frame([(txy[i, :tn[i]], tcf[i, :tn[i]], tcl[i, :tn[i]]) for i in range(5)], *GEOM), thresh=MATCH)
    assert n[0] == len(want[1]) > 0 and np.array_equal(bits(xy[0, :n[0]]), bits(want[0])) and np.array_equal(bits(cf[0, :n[0]]), bits(want[1]))
    small.close()
    # a detector that accepts no source frame as large as the tile
    tiny = pkg.Detector(wpath, input_size=TILE, confidence=CONF, batch=10, max_source_size=(256, 256), autotune=False, warmup=False)
    assert L.rtmodt_slicer_enqueue(sd._h, tiny.model.handle, fp, 2, pitch, F.MEM_HOST) == F.E_CAPACITY and b"max_src 256x256" in L.rtmodt_last_error()
    tiny.close()
    # a third batch in flight
    sd.enqueue(list(frames[:2]))
    sd.enqueue(list(frames[2:4]))
    with pytest.raises(F.RtmodtError) as e:
        sd.enqueue(list(frames[4:6]))
    assert e.value.code == F.E_INVALID and len(sd._in_flight) == 2
    first = sd.fetch()
    sd.enqueue(list(frames[4:6]))                                    # ... fits again after a fetch
    sd.fetch(); sd.fetch()
    assert all(same(a, b) for a, b in zip(first, ref))
    with pytest.raises(RuntimeError):
        sd.fetch()
    assert L.rtmodt_slicer_fetch(sd._h, sd.detector.model.handle, None, None, None, None, F.ptr(n), None, None, None, None) == F.E_INVALID
    assert L.rtmodt_slicer_enqueue(sd._h, sd.detector.model.handle, fp, 2, pitch - 1, F.MEM_HOST) == F.E_INVALID       # pitch < 3w
    assert L.rtmodt_slicer_enqueue(sd._h, sd.detector.model.handle, fp, 3, pitch, F.MEM_HOST) == F.E_INVALID           # n > max_frames
    assert all(same(a, b) for a, b in zip(sd.detect_batch(list(frames[:2])), ref))
    sd.close()
