"""GPU: the occupancy heatmap (csrc/heatmap.hip) against the NumPy restatement of its rules (tests/heatmap_ref.py), through
Heatmap and the C ABI: the three footprints over small grids with clipped edge cells and more than one tile, the cull loop past
its LDS batch, saturation and decay, the overlay on host frames and on device frames with their own row pitch (padding bytes
included), zone sums, the device-state forms of the four trackers and of the detector, housekeeping, every refusal, and the
pipeline's heatmap stage.  Every comparison is == on integers."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import heatmap_ref as HR
import render_ref as RR

pytestmark = pytest.mark.gpu

GEOMS = [(37, 70, 211), (70, 37, 117), (19, 150, 452)]          # h, w, row stride of the frames; 150 cells span three 64-cell tiles
KINDS = [HR.BOX, HR.DISC, HR.FOOT]
U32_MAX = HR.U32_MAX
CONCAVE = np.array([[3, 2], [40, 4], [22, 15], [44, 33], [5, 30], [14, 16]], np.int32)


@functools.lru_cache(maxsize=None)
def scene(h, w, s, f):
    """Stream s, frame f: boxes inside, straddling every edge, outside, inverted, smaller than a cell; classes 0..2."""
    rng = np.random.default_rng(100000 * h + 100 * w + 10 * s + f)
    k = 9
    x0 = rng.uniform(-0.3 * w - 2, w + 1, k); y0 = rng.uniform(-0.3 * h - 2, h + 1, k)
    bw = rng.uniform(0, 0.6 * w + 2, k); bh = rng.uniform(0, 0.6 * h + 2, k)
    boxes = np.stack([x0, y0, x0 + bw, y0 + bh], 1).astype(np.float32)
    boxes[5] = boxes[5][[2, 1, 0, 3]] - np.float32([0, 0, 1, 0])        # inverted in x
    boxes[6] = np.float32([w / 2 + f, h / 2 + s, w / 2 + f + 1.5, h / 2 + s + 0.5])     # smaller than a cell
    boxes[7] = np.float32([w - 2.5, h - 3.5, w + 8, h + 9])                                # over the bottom-right corner
    boxes.setflags(write=False)
    return boxes, (np.arange(k) % 3).astype(np.int32)


def diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    return f"{len(bad)} values differ, first at {bad[:6].tolist()}: {got.reshape(-1)[bad[:6]].tolist()} != {want.reshape(-1)[bad[:6]].tolist()}" \
        if len(bad) else None


def view(buf, h, w, stride):
    return np.lib.stride_tricks.as_strided(buf, (h, w, 3), (stride, 3, 1), writeable=buf.flags.writeable)


# ---- accumulate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cell", [1, 2, 4, 16])
@pytest.mark.parametrize("h,w", [g[:2] for g in GEOMS])
def test_footprints_over_cells_and_geometries(pkg, h, w, cell, kind):
    S = 3 if (h, w) == (37, 70) else 2
    kw = dict(foot_radius=3, weight=5, classes=(0, 2))
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell, footprint=kind, **kw)
    refs = [HR.Ref(h, w, cell, kind=kind, **kw) for _ in range(S)]
    assert hm.grid_shape == HR.grid_shape(h, w, cell)
    for f in range(4):
        hm.accumulate([scene(h, w, s, f) for s in range(S)])
        for s in range(S):
            want = refs[s].accumulate(*scene(h, w, s, f))
            assert diff(hm.grid(s), want) is None, (f, s, diff(hm.grid(s), want))
    assert all(r.grid.any() for r in refs) and hm.last_kernel_ms() >= 0
    assert not np.array_equal(refs[0].grid, refs[1].grid)
    hm.close()


@pytest.mark.parametrize("weight", [1, 1024])
def test_300_boxes_cross_the_cull_batch(pkg, weight):
    """300 boxes on a 37 x 70 frame (one tile at cell 2): the cull loop runs two batches of 256; the first 120 share their cells."""
    h, w = 37, 70
    rng = np.random.default_rng(300)
    x0 = rng.uniform(-8, w, 300); y0 = rng.uniform(-8, h, 300)
    boxes = np.stack([x0, y0, x0 + rng.uniform(0, 14, 300), y0 + rng.uniform(0, 11, 300)], 1).astype(np.float32)
    boxes[:120] = np.float32([20.5, 9, 31, 22.5])
    boxes[290:] = np.float32([60, 30, 75, 40])
    for kind, cell in ((HR.DISC, 2), (HR.BOX, 1), (HR.FOOT, 4)):
        hm = pkg.visualization.Heatmap(2, h, w, cell=cell, footprint=kind, foot_radius=5, weight=weight)
        ref = HR.Ref(h, w, cell, kind=kind, foot_radius=5, weight=weight)
        hm.accumulate([boxes, np.zeros((0, 4), np.float32)])
        want = ref.accumulate(boxes)
        assert want.max() >= 120 * weight
        assert diff(hm.grid(0), want) is None, (kind, diff(hm.grid(0), want))
        assert not hm.grid(1).any()
        hm.accumulate([boxes[::-1].copy(), boxes[:3]])                           # the order of the boxes does not matter
        assert diff(hm.grid(0), ref.accumulate(boxes)) is None
        hm.close()


def test_saturation_and_decay(pkg):
    h, w, cell = 37, 70, 4
    gh, gw = HR.grid_shape(h, w, cell)
    rng = np.random.default_rng(32)
    box = np.float32([[10, 6, 50, 30], [12, 8, 30, 20]])
    # saturation: cells within 0..2048 of the top, stamped with weight 1024 once or twice
    near = (U32_MAX - rng.integers(0, 2049, (gh, gw))).astype(np.uint32)
    hm = pkg.visualization.Heatmap(2, h, w, cell=cell, footprint="box", weight=1024)
    hm.load(near, 1)
    hm.accumulate([box[:0], box])
    want = HR.stamp(near, HR.counts(box, None, h, w, cell, kind=HR.BOX), 1024)
    assert (want == U32_MAX).sum() > 10 and (want != U32_MAX).any() and (want[2:5, 3:7] > near[2:5, 3:7]).any()
    assert diff(hm.grid(1), want) is None, diff(hm.grid(1), want)
    assert not hm.grid(0).any()
    hm.close()
    # decay in every second call, fused into the stamp pass; call 2 carries no box at all and still decays
    for shift in (1, 16):
        start = rng.integers(0, 1 << 32, (gh, gw), dtype=np.uint64).astype(np.uint32)
        start[0, :4] = [0, 1, 65535, 65536]
        hm = pkg.visualization.Heatmap(2, h, w, cell=cell, footprint="disc", weight=3, decay_shift=shift, decay_every=2)
        refs = [HR.Ref(h, w, cell, kind=HR.DISC, weight=3, decay_shift=shift, decay_every=2) for _ in range(2)]
        hm.load(start, 0)
        refs[0].grid = start.copy()
        for call in range(1, 6):
            lists = [box[:0], box[:0]] if call == 2 else [box, box[1:]]
            hm.accumulate(lists)
            for s in range(2):
                want = refs[s].accumulate(lists[s])
                assert diff(hm.grid(s), want) is None, (shift, call, s, diff(hm.grid(s), want))
            if call == 2:
                assert diff(refs[0].grid, HR.decay(HR.stamp(start, HR.counts(box, None, h, w, cell, kind=HR.DISC), 3), shift)) is None
        hm.close()


# ---- overlay ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def heat(h, w, cell, s):
    """A grid with zeros, small counts and a few large cells."""
    rng = np.random.default_rng(7 * h + w + cell + s)
    gh, gw = HR.grid_shape(h, w, cell)
    g = rng.integers(0, 40, (gh, gw)).astype(np.uint32)
    g[rng.random((gh, gw)) < 0.3] = 0
    if s == 1:                                              # heat * 255 + m / 2 past 2^32 below a maximum of 2^32 - 1
        g[1, 1] = 1 << 31; g[1, 2] = 3000000000; g[2, 1] = 20000000
    g[0, 0] = 1000 + s; g[gh - 1, gw - 1] = 3; g[gh // 2, gw // 2] = U32_MAX if s == 1 else 77
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def frame_buf(h, stride, s):
    buf = np.random.default_rng(h + stride + s).integers(0, 256, h * stride, dtype=np.uint8)
    buf.setflags(write=False)
    return buf


@pytest.mark.parametrize("alpha", [0, 128, 256])
@pytest.mark.parametrize("min_level", [1, 200])
@pytest.mark.parametrize("h,w,stride", GEOMS)
def test_overlay_alpha_and_min_level(pkg, h, w, stride, min_level, alpha):
    cell, S = (1 if w == 150 else 4), 2
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell, alpha=alpha, min_level=min_level)
    for s in range(S):
        hm.load(heat(h, w, cell, s), s)
    want = []
    for s in range(S):
        buf = frame_buf(h, stride, s)
        out = buf.copy()
        view(out, h, w, stride)[:] = HR.overlay(view(buf, h, w, stride), heat(h, w, cell, s), cell, alpha, min_level)
        want.append(out)
    assert alpha == 0 or all(diff(want[s], frame_buf(h, stride, s)) is not None for s in range(S))
    # host frames with padded rows: staged, blended, copied back; the padding is not written
    host = [frame_buf(h, stride, s).copy() for s in range(S)]
    frames = [view(b, h, w, stride) for b in host]
    assert hm.overlay(frames) is frames
    for s in range(S):
        assert diff(host[s], want[s]) is None, (s, diff(host[s], want[s]))
    # device frames, one buffer holding both with the padded pitch: the kernel sees the odd stride
    dev = pkg._ffi.DeviceBuffer(S * h * stride)
    dev.upload(np.concatenate([frame_buf(h, stride, s) for s in range(S)]))
    hm.overlay(dev, stride=stride)
    back = dev.download().reshape(S, h * stride)
    for s in range(S):
        assert diff(back[s], want[s]) is None, (s, diff(back[s], want[s]))
    pad = np.ones((h, stride), bool); pad[:, :3 * w] = False
    assert pad.any() and np.array_equal(back[0].reshape(h, stride)[pad], frame_buf(h, stride, 0).reshape(h, stride)[pad])
    assert hm.last_kernel_ms() >= 0
    dev.free(); hm.close()


def test_overlay_scale_max_table_and_stream_subset(pkg):
    h, w, stride, cell, S = 37, 70, 211, 2, 3
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell)
    for s in (0, 1):
        hm.load(heat(h, w, cell, s), s)                                          # stream 2 stays all zero
    fr = lambda s: view(frame_buf(h, stride, s), h, w, stride)
    # scale_max below the true maximum: levels clamp at 255; and far above it: most cells fall below min_level
    for scale in (20, 5000):
        got = [fr(s).copy() for s in range(S)]
        hm.overlay(got, scale_max=scale, alpha=200, min_level=2)
        for s in range(S):
            want = HR.overlay(fr(s), hm.grid(s), cell, 200, 2, scale_max=scale)
            assert diff(got[s], want) is None, (scale, s, diff(got[s], want))
        assert HR.levels(heat(h, w, cell, 0), 20).max() == 255 and np.array_equal(got[2], fr(2)) and not np.array_equal(got[0], fr(0))
    # scale_max 0 on an all-zero grid: the frame is untouched (stream 2); the others scale to their own maxima
    got = [fr(s).copy() for s in range(S)]
    hm.overlay(got)
    assert np.array_equal(got[2], fr(2))
    for s in (0, 1):
        assert diff(got[s], HR.overlay(fr(s), heat(h, w, cell, s), cell)) is None
    # a custom table, then the default again
    table = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    hm.set_colormap(table)
    got = [fr(s).copy() for s in range(S)]
    hm.overlay(got, alpha=256)
    assert diff(got[0], HR.overlay(fr(0), heat(h, w, cell, 0), cell, 256, lut=table)) is None
    hm.set_colormap(None)
    one = [fr(0).copy()]
    hm.overlay(one, streams=[0], alpha=256)
    assert diff(one[0], HR.overlay(fr(0), heat(h, w, cell, 0), cell, 256)) is None and not np.array_equal(one[0], got[0])
    # a subset of the streams, out of order and repeated: frame i shows grid streams[i]
    sub = [fr(0).copy(), fr(1).copy(), fr(2).copy()]
    hm.overlay(sub, streams=[1, 1, 0], alpha=77)
    for i, s in enumerate((1, 1, 0)):
        assert diff(sub[i], HR.overlay(fr(i), heat(h, w, cell, s), cell, 77)) is None, i
    dev = pkg._ffi.DeviceBuffer(h * stride)
    dev.upload(frame_buf(h, stride, 2))
    hm.overlay(dev, streams=[1], stride=stride)
    want = frame_buf(h, stride, 2).copy()
    view(want, h, w, stride)[:] = HR.overlay(fr(2), heat(h, w, cell, 1), cell)
    assert diff(dev.download(), want) is None
    dev.free(); hm.close()


# ---- zone sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 4, 16])
def test_zone_sums(pkg, cell):
    h, w, S = 37, 70, 2
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell)
    for s in range(S):
        hm.load(heat(h, w, cell, s), s)
    c = cell // 2
    polys = [CONCAVE,                                                             # concave
             np.int32([[10, 5], [60, 5], [60, 30], [10, 30]]), np.int32([[30, 0], [69, 0], [69, 36], [30, 36]]),   # overlapping
             np.int32([[2 * cell + c, cell + c], [50, cell + c], [50, 33]]),       # a vertex on the centre pixel of cell (2, 1)
             CONCAVE + np.int32([40, 20]),                                        # runs off the frame
             np.int32([[-50, -50], [500, -50], [500, 500], [-50, 500]]),          # the whole grid
             np.int32([[200, 200], [210, 200], [210, 210]]), np.zeros((0, 2), np.int32)]   # outside; empty
    assert HR.zone_mask(polys[3], h, w, cell)[1, 2]
    for s in range(S):
        want = HR.zone_sums(heat(h, w, cell, s), polys, h, w, cell)
        got = hm.zone_sums(polys, stream=s)
        assert got.dtype == np.uint64 and got.tolist() == want, (s, got.tolist(), want)
        assert want[5] == int(heat(h, w, cell, s).astype(np.uint64).sum()) and want[6] == want[7] == 0 and 0 < want[0] < want[5]
    assert want[5] > U32_MAX                                                      # (stream 1 holds a saturated cell: a 64-bit sum)
    assert hm.zone_sums([]).tolist() == []
    # object-frames: weight 1, FOOT radius 0, three frames of two boxes standing in the zone and one outside it; every footprint is
    # one cell, and at cell 1 the zone's sum is exactly the object-frames spent in it (coarser cells belong to a zone by their centre)
    foot = pkg.visualization.Heatmap(1, h, w, cell=cell, footprint="foot", foot_radius=0)
    fref = HR.Ref(h, w, cell, kind=HR.FOOT)
    for f in range(3):
        bx = np.float32([[12 + f, 6, 18 + f, 20], [40, 10, 48, 25 + f], [62, 2, 68, 34]])
        foot.accumulate([bx])
        fref.accumulate(bx)
    assert foot.zone_sums([polys[1]]).tolist() == HR.zone_sums(fref.grid, [polys[1]], h, w, cell) and int(foot.grid().sum()) == 9
    assert cell != 1 or foot.zone_sums([polys[1]]).tolist() == [6]
    foot.close(); hm.close()


# ---- device-state forms ----------------------------------------------------------------------------------------------
S, N, FH, FW = 2, 16, 37, 70


def scripted(f, s):
    """Frame f of stream s: 8 steady boxes, one present in frames 0 and 1 only (lost at the end), one in frame 2 only (new)."""
    bx = [[2 + 14 * i + f, 2 + 18 * j + s, 11 + 14 * i + f, 14 + 18 * j + s] for j in range(2) for i in range(4)]
    if f < 2:
        bx.append([57, 2 + s, 67, 13 + s])
    if f == 2:
        bx.append([58.5, 21, 75, 33.5 + s])
    xy = np.float32(bx)
    return xy, np.full(len(xy), 0.9, np.float32), (np.arange(len(xy)) % 3).astype(np.int32)


def run_scripted(core, with_frames):
    frames = [np.random.default_rng(s).integers(0, 256, (FH, FW, 3), dtype=np.uint8) for s in range(S)]
    for f in range(3):
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32); cnt = np.zeros(S, np.int32)
        for s in range(S):
            xy, cf, cl = scripted(f, s)
            xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf, cl, len(cf)
        if with_frames:
            core.update_batch(xyxy, conf, cls, cnt, frames=frames)
        else:
            core.update_batch(xyxy, conf, cls, cnt)
    return frames


def _trackers(pkg):
    T = pkg.tracking
    return {
        "bytetrack": (lambda n=S: T.tracker._ByteTrackCore(n_streams=n, max_tracks=32, max_dets=N), False,
                      lambda core, st: np.nonzero(st["tsu"] == 1)[0]),
        "deepsort": (lambda: T.deepsort._DeepSortCore(n_init=2, max_age=5, nn_budget=4, n_streams=S, max_tracks=32, max_dets=N), True,
                     lambda core, st: np.nonzero((st["state"] == 2) & (st["tsu"] == 0))[0]),
        "ocsort": (lambda: T.ocsort._OcSortCore(min_hits=2, n_streams=S, max_tracks=32, max_dets=N), False,
                   lambda core, st: core.returned(st)),
        "botsort": (lambda: T.botsort._BotSortCore(n_streams=S, max_tracks=32, max_dets=N), False,
                    lambda core, st: np.nonzero((st["flag"] == 2) & (st["tsu"] == 0))[0]),
    }


@pytest.mark.parametrize("which", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_accumulate_tracker_equals_accumulate_on_the_passed_tracks(pkg, which):
    make, with_frames, passed = _trackers(pkg)[which]
    core = make()
    run_scripted(core, with_frames)
    kw = dict(cell=2, footprint="disc", weight=7, classes=(0, 1))
    dev, host = pkg.visualization.Heatmap(S, FH, FW, **kw), pkg.visualization.Heatmap(S, FH, FW, **kw)
    lists, n_state, n_pass = [], 0, 0
    for s in range(S):
        st = core.snapshot(s)
        idx = passed(core, st)
        n_state += len(st["ids"]); n_pass += len(idx)
        lists.append((st["xyxy"][idx], st["cls"][idx]))
    assert 0 < n_pass < n_state, (n_pass, n_state)                              # a track of the state is not reported
    tracker = SimpleNamespace(_core=core, report="matched") if which == "bytetrack" else core
    for call in range(2):
        host.accumulate(lists)
        dev.accumulate_tracker(tracker)
        for s in range(S):
            want = HR.stamp(np.zeros(host.grid_shape, np.uint32), (call + 1) * HR.counts(*lists[s], FH, FW, 2, kind=HR.DISC, classes=(0, 1)), 7)
            assert want.any() and diff(host.grid(s), want) is None, (s, diff(host.grid(s), want))
            assert diff(dev.grid(s), want) is None, (s, diff(dev.grid(s), want))
    if which == "bytetrack":                                                    # the reference's filter (tsu == 0 after ageing) passes none
        before = [dev.grid(s) for s in range(S)]
        dev.accumulate_tracker(SimpleNamespace(_core=core, report="reference"))
        assert all(np.array_equal(dev.grid(s), before[s]) for s in range(S))
        # a tracker of another stream count is refused, the grid as it was
        other = make(3)
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            dev.accumulate_tracker(SimpleNamespace(_core=other, report="matched"))
        assert e.value.code == pkg._ffi.E_INVALID and all(np.array_equal(dev.grid(s), before[s]) for s in range(S))
        other.close()
    with pytest.raises(TypeError, match="accumulate\\(\\[tracks\\]\\)"):
        dev.accumulate_tracker(object())
    dev.close(); host.close(); core.close()


@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("weights_heatmap")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, batch=2, warmup=False, autotune=False)
    yield det
    det.close()


def test_accumulate_detector_equals_accumulate_on_the_fetched_detections(pkg, detector):
    frames = [f.copy() for f in pkg.synth.frames(2, 320, 320, seed=11)]
    dets = detector.detect_batch(frames)
    assert sum(len(d) for d in dets) > 0
    for kind, cell in ((HR.FOOT, 4), (HR.DISC, 16)):
        hm = pkg.visualization.Heatmap(2, 320, 320, cell=cell, footprint=kind, foot_radius=6)
        hm.accumulate_detector(detector)
        for s, d in enumerate(dets):
            want = HR.stamp(np.zeros(hm.grid_shape, np.uint32), HR.counts(d.xyxy, d.class_id, 320, 320, cell, kind=kind, foot_radius=6))
            assert diff(hm.grid(s), want) is None, (kind, s, diff(hm.grid(s), want))
        hm.close()
    three = pkg.visualization.Heatmap(3, 320, 320)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        three.accumulate_detector(detector)                                     # the batch held two frames
    assert e.value.code == pkg._ffi.E_INVALID and not any(three.grid(s).any() for s in range(3))
    three.close()


# ---- housekeeping and refusals ---------------------------------------------------------------------------------------
def test_read_load_reset_round_trip(pkg):
    h, w, cell, S = 19, 150, 4, 3
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell)
    assert all(hm.grid(s).shape == HR.grid_shape(h, w, cell) and not hm.grid(s).any() for s in range(S))     # zero at creation
    saved = [heat(h, w, cell, s) for s in range(S)]
    for s in range(S):
        hm.load(saved[s], s)
    assert all(np.array_equal(hm.grid(s), saved[s]) for s in range(S))
    # a map survives a restart: a fresh handle loaded with the saved grid goes on exactly as the old one
    again = pkg.visualization.Heatmap(S, h, w, cell=cell)
    again.load(hm.grid(1), 1)
    for m in (hm, again):
        m.accumulate([scene(h, w, s, 0) for s in range(S)])
    assert np.array_equal(again.grid(1), hm.grid(1)) and not np.array_equal(hm.grid(1), saved[1])
    hm.reset(1)
    assert not hm.grid(1).any() and hm.grid(0).any() and hm.grid(2).any()
    hm.reset()
    assert not any(hm.grid(s).any() for s in range(S))
    with pytest.raises(ValueError):
        hm.load(np.zeros((3, 3), np.uint32))
    hm.close(); again.close()


def test_refusals_leave_grid_and_frames_unchanged(pkg):
    h, w, stride, cell, S = 37, 70, 211, 4, 2
    F, E = pkg._ffi, pkg._ffi.RtmodtError
    L = F.lib()
    fresh = pkg.visualization.Heatmap(S, h, w, cell=cell)
    with pytest.raises(E) as e:
        fresh.last_kernel_ms()                                                  # nothing has launched yet
    assert e.value.code == F.E_INVALID
    fresh.close()
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell, footprint="box", decay_shift=1, decay_every=2)
    ref = [HR.Ref(h, w, cell, kind=HR.BOX, decay_shift=1, decay_every=2) for _ in range(S)]
    for s in range(S):
        hm.load(heat(h, w, cell, s), s)
        ref[s].grid = heat(h, w, cell, s).copy()
    good = np.float32([[1, 1, 30, 20]])
    bufs = [frame_buf(h, stride, s).copy() for s in range(S)]
    frames = [view(b, h, w, stride) for b in bufs]

    def unchanged():
        return all(np.array_equal(hm.grid(s), ref[s].grid) for s in range(S)) and all(np.array_equal(bufs[s], frame_buf(h, stride, s)) for s in range(S))

    def refused(code, call):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == code, e.value
        assert unchanged(), "a refused call changed the grid or a frame"

    # accumulate: a non-finite coordinate in the LAST stream (the first stream's boxes are fine), too many boxes
    refused(F.E_INVALID, lambda: hm.accumulate([good, np.float32([[1, 1, 5, 5], [2, np.nan, 9, 9]])]))
    refused(F.E_INVALID, lambda: hm.accumulate([good, np.float32([[1, 1, np.inf, 5]])]))
    refused(F.E_INVALID, lambda: hm.accumulate([np.float32([[-np.inf, 1, 3, 5]]), good]))
    many = np.tile(np.float32([[1, 1, 30, 20], [50, 20, 90, 50]]), (32769, 1))
    refused(F.E_CAPACITY, lambda: hm.accumulate([good, many[:65537]]))
    with pytest.raises(ValueError):
        hm.accumulate([good])                                                   # one list for two streams
    # overlay: another geometry, a short stride, alpha / min_level outside their ranges, a stream that does not exist, a frame
    # count that is not the stream count without a stream list
    refused(F.E_INVALID, lambda: hm.overlay([f[:, :69] for f in frames]))
    refused(F.E_INVALID, lambda: hm.overlay([f[:36] for f in frames]))
    fp = (C.c_void_p * S)(*[b.ctypes.data for b in bufs])
    refused(F.E_INVALID, lambda: F.check(L.rtmodt_heatmap_overlay(hm._h, fp, None, S, h, w, 3 * w - 1, F.MEM_HOST, 128, 1, 0)))
    refused(F.E_INVALID, lambda: F.check(L.rtmodt_heatmap_overlay(hm._h, fp, None, S, h, w, stride, 2, 128, 1, 0)))
    for kw in (dict(alpha=-1), dict(alpha=257), dict(min_level=0), dict(min_level=256)):
        refused(F.E_INVALID, lambda: hm.overlay(frames, **kw))
    refused(F.E_INVALID, lambda: hm.overlay(frames, streams=[0, 2]))
    refused(F.E_INVALID, lambda: hm.overlay(frames, streams=[-1, 0]))
    refused(F.E_INVALID, lambda: F.check(L.rtmodt_heatmap_overlay(hm._h, fp, None, 1, h, w, stride, F.MEM_HOST, 128, 1, 0)))
    # zone sums, read, load, reset
    refused(F.E_CAPACITY, lambda: hm.zone_sums([CONCAVE] * 33))
    refused(F.E_CAPACITY, lambda: hm.zone_sums([np.zeros((2049, 2), np.int32)]))
    refused(F.E_INVALID, lambda: hm.zone_sums([CONCAVE], stream=2))
    refused(F.E_INVALID, lambda: hm.grid(2))
    refused(F.E_INVALID, lambda: hm.load(heat(h, w, cell, 0), -1))
    refused(F.E_INVALID, lambda: hm.reset(2))
    refused(F.E_INVALID, lambda: hm.reset(-2))
    # refused calls are not counted: the next accepted call is call 1 (no decay), the one after it call 2 (decay)
    for call in range(2):
        hm.accumulate([good, many[:65536]])                                     # 65536 boxes are accepted: 256 cull batches
        two = HR.counts(many[:2], None, h, w, cell, kind=HR.BOX)
        for s in range(S):
            ref[s].calls += 1
            if ref[s].calls % 2 == 0:
                ref[s].grid = HR.decay(ref[s].grid, 1)
            ref[s].grid = HR.stamp(ref[s].grid, HR.counts(good, None, h, w, cell, kind=HR.BOX) if s == 0 else 32768 * two)
        assert unchanged(), call
    hm.close()


# ---- the pipeline's heatmap stage ------------------------------------------------------------------------------------
class _Rec:
    def __init__(self):
        self.frames = []

    def write(self, frame):
        self.frames.append(frame.copy())


class _Det:
    model = type("M", (), {"names": {0: "person"}})()

    def detect(self, frame):
        return type("D", (), {"xyxy": np.zeros((1, 4), np.float32), "confidence": np.ones(1, np.float32), "class_id": np.zeros(1, np.int32),
                              "__len__": lambda self: 1})()


class _Trk:
    def update_from_detector(self, det, materialize=True):
        return [SimpleNamespace(track_id=4, xyxy=np.array([2, 12, 30, 40], np.float32), confidence=0.9, class_name="person", class_id=0,
                                trail=[(5, 5), (16, 26)])] if materialize else []


def test_pipeline_heatmap_stage(pkg, detector):
    """3 frames: every frame is accumulated, the recorded frame is the render of the frame with the heat blended in (labels and
    boxes on top of the heat), and the stage table gains exactly the heatmap row, after privacy and before visualization."""
    frames = np.random.default_rng(9).integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof(), max_frames=3, device_stages=False,
                            renderer=pkg.FrameRenderer(show_fps=False))
    rec = _Rec()
    hm = pkg.visualization.Heatmap(1, 48, 64, cell=4, footprint="box", alpha=160)
    mask = pkg.visualization.PrivacyMask(mode="pixelate", cell=8)
    p = prof()
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), p, max_frames=3, device_stages=False,
                           renderer=pkg.FrameRenderer(show_fps=False), recorder=rec, heatmap=hm, privacy=mask)
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"heatmap_mean_ms", "privacy_mean_ms"} and rows(base) <= rows(out)
    order = list(p.STAGE_ORDER)
    assert order.index("privacy") + 1 == order.index("heatmap") == order.index("visualization") - 1
    assert pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events", "visualization", "total"]
    tracks = _Trk().update_from_detector(None)
    ref = HR.Ref(48, 64, 4, kind=HR.BOX)
    assert len(rec.frames) == 3
    import privacy_ref as PR
    for i in range(3):
        g = ref.accumulate([tracks[0].xyxy], [0]).copy()
        masked = PR.apply(frames[i % 2], [tracks[0].xyxy], [0], mode="pixelate", cell=8)
        heated = HR.overlay(masked, g, 4, alpha=160)
        assert not np.array_equal(heated, masked)
        assert np.array_equal(rec.frames[i], RR.render(heated, tracks, None, show_fps=False)), i
    assert diff(hm.grid(), ref.grid) is None and ref.grid.max() == 3
    mask.close(); hm.close()
    # no materialised track list (the crossing counter reads the tracker's device state): the heatmap does, too; overlay_enabled
    # off: the frames are accumulated and left as they are
    trk = pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    trk.report = "matched"
    counter = pkg.events.CrossingCounter([{"name": "l", "a": [0, 160], "b": [320, 160]}])
    src = pkg.synth.frames(2, 320, 320, seed=11)
    hm = pkg.visualization.Heatmap(1, 320, 320, cell=8, footprint="foot", foot_radius=9, overlay_enabled=False)
    ref = HR.Ref(320, 320, 8, kind=HR.FOOT, foot_radius=9)
    n_pass = 0
    for f in range(3):
        rec = _Rec()
        out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(src), detector, trk, prof(), max_frames=1, crossing_counter=counter, recorder=rec, heatmap=hm)
        assert "heatmap_mean_ms" in out and np.array_equal(rec.frames[0], src[0])
        st = trk._core.snapshot(0)
        idx = np.nonzero(st["tsu"] == 1)[0]
        n_pass += len(idx)
        ref.accumulate(st["xyxy"][idx], st["cls"][idx])
        assert diff(hm.grid(), ref.grid) is None, (f, diff(hm.grid(), ref.grid))
    assert n_pass > 0 and ref.grid.any()
    hm.close(); counter.close()
