"""GPU: motion detection (csrc/motion.hip), left / removed objects (csrc/leftobj.hip) and camera health (csrc/health.hip) at the sizes
their shared headers are written for -- csrc/cell_grid.h (the pixel reader), csrc/grid_host.h (the launch geometry), csrc/ccl_dev.h
(the union-find labelling and the ranking of its roots by chunks of 4096 cells) -- against the restatements, with == on integers
after every call (the check functions of test_gpu_motion.py, test_gpu_leftobj.py and test_gpu_health.py).  The scenarios are those of
tests/grid_limit_cases.py; tests/test_grid_limit_cases_cpu.py proves on the restatements alone that each of them reaches the code it
is meant for: more than 256 chunks (a second pass of ccl_scan_chunks), the cut of ccl_emit_chunk on a chunk boundary, inside the
partly filled last chunk and beyond the total, with roots that fail min_area / max_area next to it; components of half a million
cells in the left-object accumulators; masks at the 8-connected percolation threshold; stream lists over many chunks; 1080p at scale
4 and 1; sides of 32768 px."""
import numpy as np
import pytest

import grid_limit_cases as G
import health_ref as HR
import leftobj_ref as LR
import motion_ref as MR
import test_gpu_health as TH
import test_gpu_leftobj as TL
import test_gpu_motion as TM
from test_gpu_motion import DeviceFrames

pytestmark = pytest.mark.gpu


# ---- masks into the detectors --------------------------------------------------------------------------------------------------
def motion_step(det, ref, masks, streams, what):
    """One call: the named streams get the flat model and a frame whose mask is theirs of ``masks``."""
    for s in streams:
        G.motion_load(ref, ref.gh, ref.gw, s)
        G.motion_load(det, ref.gh, ref.gw, s)
    frames = [G.motion_frame(m, ref.c["scale"], ref.h, ref.w) for m in masks]
    want = ref.process(frames, streams)
    for m, w_ in zip(masks, want):
        assert np.array_equal(ref.masks[w_["stream"]], m), what
    TM.check(det, ref, det.process(frames, streams), want, what)
    return want


def leftobj_step(pkg, det, ref, masks, streams, what):
    """The same for the left-object detector: a model whose mask cells are one frame short of static (the ledgers go on)."""
    dtype = pkg.detection.left_objects.CELL_DTYPE
    for s, m in zip(streams, masks):
        model = G.lo_model(m, ref.c["static_frames"])
        G.lo_load_ref(ref, model, s)
        det.load_state(G.lo_cells(model, dtype), model["luma"], ref.c["warmup"], s)
    frames = [G.lo_frame(m, ref.h, ref.w) for m in masks]
    want = ref.process(frames, streams=streams)
    for m, w_ in zip(masks, want):
        assert np.array_equal(ref.masks[w_["stream"]], m), what
    TL.check(det, ref, det.process(frames, streams=streams, want_objects=True), want, what)
    return want


# ---------------------------------------------------------------------------------------------------------------- 0. the handles
@pytest.mark.parametrize("h,w,scale", [(G.BIG_H, G.BIG_W, 1), (G.PROD_H, G.PROD_W, 4), (G.PROD_H, G.PROD_W, 1), (4, G.MAX_SIDE, 8), (G.MAX_SIDE, 4, 1)])
def test_the_grids_are_geometry_s(pkg, h, w, scale):
    """The grid the library makes of a frame size is the one the scenarios' chunk and tile counts are worked out from."""
    geo = G.geometry(h, w, scale)
    for make in (pkg.MotionDetector, pkg.LeftObjectDetector, pkg.ingestion.CameraHealth):
        det = make(1, h, w, scale=scale)
        assert tuple(det.grid_shape) == (geo["gh"], geo["gw"]), make
        det.close()
    ref = MR.Ref(1, h, w, scale=scale)
    assert (ref.gh, ref.gw) == (geo["gh"], geo["gw"]) and geo["n_chunks"] == -(-ref.gh * ref.gw // G.CHUNK)


def test_a_state_loaded_directly_after_create_stays(pkg):
    """create zeroes three streams of 2^20 cells; a load_state that follows at once must find that done: what is read back is what
    was loaded, in the last stream and the first, and the other stream is zero."""
    S, h, w = 3, G.BIG_H, G.BIG_W
    rng = np.random.default_rng(11)
    bg, dev = rng.integers(0, 65536, (h, w)).astype(np.uint16), rng.integers(0, 65536, (h, w)).astype(np.uint16)
    mo = pkg.MotionDetector(S, h, w, scale=1)
    mo.load_state(bg, dev, 5, 2)
    mo.load_state(dev, bg, 6, 0)
    for s, want in ((2, (bg, dev, 5)), (0, (dev, bg, 6)), (1, (0 * bg, 0 * bg, 0))):
        got = mo.state(s)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], ("motion", s)
    mo.close()
    cells, luma = rng.integers(0, 2 ** 63, (h, w)).astype(np.uint64), rng.integers(0, 256, (h, w)).astype(np.uint8)
    lo = pkg.LeftObjectDetector(S, h, w, scale=1)
    lo.load_state(cells, luma, 5, 2)
    lo.load_state(cells[::-1], luma[::-1], 6, 0)
    for s, want in ((2, (cells, luma, 5)), (0, (cells[::-1], luma[::-1], 6)), (1, (0 * cells, 0 * luma, 0))):
        got = lo.state(s)
        assert np.array_equal(got[0].view(np.uint64), want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], ("left objects", s)
    lo.close()
    hm = pkg.ingestion.CameraHealth(S, h, w, scale=1)
    st = hm.state(2)
    st.r, st.prev, st.frames_seen = (bg >> 8 << 8).astype(np.uint16), luma, 5      # (R is at most 255 << 8)
    hm.load_state(st, 2)
    got, other = hm.state(2), hm.state(0)
    assert np.array_equal(got.r, st.r) and np.array_equal(got.prev, luma) and got.frames_seen == 5
    assert not other.r.any() and not other.prev.any() and other.frames_seen == 0
    hm.close()


# ---------------------------------------------------------------------------------------------------------------- 1. chunk_edges
@pytest.mark.parametrize("cut", ["a", "b", "c", "d"])
def test_chunk_edges_motion(pkg, cut):
    """257 chunks; max_regions falls (a) exactly before chunk 255, which emits nothing, (b) exactly before chunk 256, (c) inside the
    quarter-full chunk 256, (d) beyond the total.  Two calls: the chunk table of the first must not show in the second."""
    n = G.edge_cuts(**G.EDGE_MOTION)[cut]
    cfg = dict(scale=1, max_regions=n, **G.EDGE_MOTION, **G.MOTION_MASK_CFG)
    ref, det = MR.Ref(1, G.BIG_H, G.BIG_W, **cfg), pkg.MotionDetector(1, G.BIG_H, G.BIG_W, **cfg)
    total = len(G.edge_roots(**G.EDGE_MOTION))
    for call in range(2):
        want = motion_step(det, ref, [G.edge_mask()], [0], ("chunk_edges", cut, call))
        assert want[0]["n_regions_total"] == total and len(want[0]["regions"]) == min(n, total)
    det.close()


@pytest.mark.parametrize("cut", ["a", "b", "c", "d"])
def test_chunk_edges_leftobj(pkg, cut):
    """The same cuts in the left-object detector, with roots above max_area among the decoys; the second call matches the rows of
    the first."""
    n = G.edge_cuts(**G.EDGE_LEFTOBJ)[cut]
    cfg = dict(G.LO_MASK_CFG, max_regions=n, max_objects=32, **G.EDGE_LEFTOBJ)
    ref, det = LR.Ref(1, G.BIG_H, G.BIG_W, **cfg), pkg.LeftObjectDetector(1, G.BIG_H, G.BIG_W, **cfg)
    total = len(G.edge_roots(**G.EDGE_LEFTOBJ))
    for call in range(2):
        want = leftobj_step(pkg, det, ref, [G.edge_mask()], [0], ("chunk_edges", cut, call))
        assert want[0]["n_regions_total"] == total and len(want[0]["regions"]) == min(n, total) == want[0]["n_objects"]
    assert len(want[0]["events"]) == min(n, total)                              # alarm_frames 2: every row alarms on the second call
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 2. speckle_wide
@pytest.mark.parametrize("max_regions", G.SPECKLE_MAX_REGIONS)
def test_speckle_wide(pkg, max_regions):
    """About 19 000 regions, some in every chunk: every chunk's rank comes out of the two-pass scan, the first chunks emit."""
    cfg = dict(G.SPECKLE_CFG, max_regions=max_regions)
    ref, det = MR.Ref(1, G.BIG_H, G.BIG_W, **cfg), pkg.MotionDetector(1, G.BIG_H, G.BIG_W, **cfg)
    for f in range(G.SPECKLE_FRAMES):
        G.motion_load(ref, ref.gh, ref.gw)
        G.motion_load(det, ref.gh, ref.gw)
        frame = G.MC.cells_to_frame(G.speckle_cells(f), 1, G.BIG_H, G.BIG_W)
        want = ref.process([frame])
        assert want[0]["n_regions_total"] > 10000 and len(want[0]["regions"]) == max_regions
        TM.check(det, ref, det.process([frame]), want, ("speckle_wide", max_regions, f))
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 3. shapes_big
@pytest.mark.parametrize("shape", G.SHAPES)
def test_shapes_big_motion(pkg, shape):
    """One component over all 257 chunks (the spiral: a path of half a million cells), its complement, the shape again."""
    cfg = dict(scale=1, min_area=1, **G.MOTION_MASK_CFG)
    ref, det = MR.Ref(1, G.BIG_H, G.BIG_W, **cfg), pkg.MotionDetector(1, G.BIG_H, G.BIG_W, **cfg)
    for k, mask in enumerate(G.shape_frames(shape)):
        want = motion_step(det, ref, [mask], [0], ("shapes_big", shape, k))
        if k != 1:
            assert want[0]["n_regions_total"] == 1 and want[0]["regions"] == [(0, 0, G.BIG_W, G.BIG_H, int(mask.sum()))]
        print(f"motion {shape} frame {k}: last_kernel_ms {det.last_kernel_ms():.3f}")
    det.close()


@pytest.mark.parametrize("shape", G.SHAPES)
def test_shapes_big_leftobj(pkg, shape):
    """The same through the per-root accumulators: area, box, minimum and maximum age and both edge sums of one component of up to
    2^20 cells."""
    cfg = dict(G.LO_MASK_CFG, max_regions=4, max_objects=4)
    ref, det = LR.Ref(1, G.BIG_H, G.BIG_W, **cfg), pkg.LeftObjectDetector(1, G.BIG_H, G.BIG_W, **cfg)
    for k, mask in enumerate(G.shape_frames(shape)):
        want = leftobj_step(pkg, det, ref, [mask], [0], ("shapes_big", shape, k))
        if k != 1:
            g = want[0]["regions"][0]
            assert want[0]["n_regions_total"] == 1 and (g["area"], g["age_min"], g["age_max"]) == (int(mask.sum()), 4, 8)
            assert want[0]["status"] == (LR.SCENE_CHANGE if shape == "full" else LR.STATIC)
        print(f"leftobj {shape} frame {k}: last_kernel_ms {det.last_kernel_ms():.3f}")
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 4. dense
@pytest.mark.parametrize("fill", G.FILLS)
def test_dense_motion(pkg, fill):
    """Random masks below, at and above the 8-connected percolation threshold: most cells have N and W set, so the links that
    ccl_link_cell leaves to a neighbour carry the labelling."""
    ref, det = MR.Ref(1, G.MID_H, G.MID_W, **G.DENSE_MOTION), pkg.MotionDetector(1, G.MID_H, G.MID_W, **G.DENSE_MOTION)
    for seed in G.SEEDS:
        want = motion_step(det, ref, [G.dense_mask(fill, seed)], [0], ("dense", fill, seed))
        assert want[0]["n_regions_total"] > 0
    det.close()


@pytest.mark.parametrize("fill", G.FILLS)
def test_dense_leftobj(pkg, fill):
    ref, det = LR.Ref(1, G.MID_H, G.MID_W, **G.DENSE_LEFTOBJ), pkg.LeftObjectDetector(1, G.MID_H, G.MID_W, **G.DENSE_LEFTOBJ)
    for seed in G.SEEDS:
        want = leftobj_step(pkg, det, ref, [G.dense_mask(fill, seed)], [0], ("dense", fill, seed))
        assert want[0]["n_regions_total"] > 0
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 5. streams_big
def test_streams_big_motion(pkg):
    """Three streams of 257 chunks each, named in another order than their slots, singly and in pairs: the chunk table goes by the
    slot, the cell state by the stream; a stream that is not named keeps state, mask and block grid bit for bit."""
    S = 3
    ref, det = MR.Ref(S, G.BIG_H, G.BIG_W, **G.STREAMS_MOTION), pkg.MotionDetector(S, G.BIG_H, G.BIG_W, **G.STREAMS_MOTION)
    for call, streams in enumerate(G.STREAM_LISTS):
        before = {s: (det.state(s), det.mask(s), det.blocks(s)) for s in range(S) if s not in streams}
        want = motion_step(det, ref, [G.stream_mask_big(call, s) for s in streams], streams, ("streams_big", call))
        assert len({w_["n_regions_total"] for w_ in want}) == len(streams)
        for s, (st, mk, bl) in before.items():
            now = det.state(s)
            assert np.array_equal(now[0], st[0]) and np.array_equal(now[1], st[1]) and now[2] == st[2] and np.array_equal(det.mask(s), mk) \
                and np.array_equal(det.blocks(s), bl), (call, s)
            assert np.array_equal(mk, ref.masks[s]), (call, s)
    det.close()


def test_streams_big_leftobj(pkg):
    """The same over 20 chunks with the ledgers: rows are born, matched, alarm and clear per stream."""
    S = 3
    ref, det = LR.Ref(S, G.MID_H, G.MID_W, **G.STREAMS_LEFTOBJ), pkg.LeftObjectDetector(S, G.MID_H, G.MID_W, **G.STREAMS_LEFTOBJ)
    n_events = 0
    for call, streams in enumerate(G.STREAM_LISTS):
        before = {s: (det.state(s), det.mask(s), det.ledger(s)) for s in range(S) if s not in streams}
        want = leftobj_step(pkg, det, ref, [G.stream_mask_mid(call, s) for s in streams], streams, ("streams_big", call))
        n_events += sum(len(w_["events"]) for w_ in want)
        for s, ((cells, luma, seen), mk, led) in before.items():
            now = det.state(s)
            assert np.array_equal(now[0], cells) and np.array_equal(now[1], luma) and now[2] == seen and np.array_equal(det.mask(s), mk) \
                and det.ledger(s) == led, (call, s)
            TL.check_stream(det, ref, s, ("unnamed", call, s))
    assert n_events > 0
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 6. production
def production(pkg, frames, ref, make, check, process):
    """Host frames at pitch 5760 (the dword path) and device frames at an odd pitch from an odd offset (the byte path) against one
    restatement."""
    h, w = G.PROD_H, G.PROD_W
    stride, offset = G.PROD_ODD
    host, dev = make(), make()
    buf = DeviceFrames(pkg, 1, h, stride, offset)
    wants = []
    for f, frame in enumerate(frames):
        assert frame.strides == (G.PROD_PITCH, 3, 1)
        want = ref.process([frame])
        check(host, ref, process(host, [frame]), want, ("host", f))
        check(dev, ref, process(dev, buf.put([frame], f), stride=stride, offset=offset), want, ("device", f))
        wants.append(want[0])
    host.close(); dev.close()
    buf.buf.free()
    return wants


def test_production_motion(pkg):
    """1080 x 1920 at the default configuration (scale 4: 32 chunks, 8 x 68 reader tiles): warm-up, still, the rectangle, still."""
    wants = production(pkg, G.motion_frames(G.PROD_H, G.PROD_W, 1, G.MOTION_PICK), MR.Ref(1, G.PROD_H, G.PROD_W),
                       lambda: pkg.MotionDetector(1, G.PROD_H, G.PROD_W), TM.check, lambda d, fr, **kw: d.process(fr, **kw))
    assert [w_["status"] for w_ in wants] == [MR.WARMUP] * 8 + [MR.STILL] + [MR.MOTION] * 2 + [MR.STILL] * 2


def test_production_motion_scale_1(pkg):
    """1080 x 1920 at scale 1: 507 chunks, a region on either side of chunk 256."""
    wants = production(pkg, G.motion_frames(G.PROD_H, G.PROD_W, 2, G.MOTION_SCALE1_PICK, low=True), MR.Ref(1, G.PROD_H, G.PROD_W, **G.MOTION_SCALE1),
                       lambda: pkg.MotionDetector(1, G.PROD_H, G.PROD_W, **G.MOTION_SCALE1), TM.check, lambda d, fr, **kw: d.process(fr, **kw))
    assert [w_["n_regions_total"] for w_ in wants] == [0, 0, 0, 2, 0]


def test_production_leftobj(pkg):
    """The scripted block under the sequence's own small timers (the defaults need 100 frames to call a cell static): the alarm and
    the return to clear; then the first frames under the default configuration."""
    wants = production(pkg, G.leftobj_frames(G.PROD_H, G.PROD_W, 3, G.LEFTOBJ_PICK), LR.Ref(1, G.PROD_H, G.PROD_W, **G.LEFTOBJ_PROD),
                       lambda: pkg.LeftObjectDetector(1, G.PROD_H, G.PROD_W, **G.LEFTOBJ_PROD), TL.check,
                       lambda d, fr, **kw: d.process(fr, want_objects=True, **kw))
    assert [e["kind"] for w_ in wants for e in w_["events"]] == [LR.ABANDONED] and wants[-1]["status"] == LR.CLEAR
    wants = production(pkg, G.leftobj_frames(G.PROD_H, G.PROD_W, 3, G.LEFTOBJ_PICK[:G.DEFAULT_FRAMES]), LR.Ref(1, G.PROD_H, G.PROD_W),
                       lambda: pkg.LeftObjectDetector(1, G.PROD_H, G.PROD_W), TL.check, lambda d, fr, **kw: d.process(fr, want_objects=True, **kw))
    assert [w_["status"] for w_ in wants] == [LR.WARMUP] * 8 + [LR.CLEAR] * 2 and wants[-1]["n_fg"] > 1000


def test_production_health(pkg):
    """A covered camera under the health sequence's own small timers (the default warm-up alone is 25 frames): raised and cleared;
    then the first frames under the default configuration, which learns from all of them."""
    wants = production(pkg, G.health_frames(G.PROD_H, G.PROD_W, 5), HR.Ref(1, G.PROD_H, G.PROD_W, **G.HC.TIMERS),
                       lambda: pkg.ingestion.CameraHealth(1, G.PROD_H, G.PROD_W, **G.HC.TIMERS), TH.check, lambda m, fr, **kw: m.process(fr, **kw))
    assert [e[:2] for w_ in wants for e in w_["events"]] == [(HR.COVERED, HR.RAISED), (HR.COVERED, HR.CLEARED)]
    wants = production(pkg, G.health_frames(G.PROD_H, G.PROD_W, 5)[:G.DEFAULT_FRAMES], HR.Ref(1, G.PROD_H, G.PROD_W),
                       lambda: pkg.ingestion.CameraHealth(1, G.PROD_H, G.PROD_W), TH.check, lambda m, fr, **kw: m.process(fr, **kw))
    assert [w_["learned"] for w_ in wants] == [HR.LEARN_SET] + [HR.LEARN_AVERAGE] * (G.DEFAULT_FRAMES - 1)


# ---------------------------------------------------------------------------------------------------------------- 7. max_side
def side(pkg, h, w, frames, ref, make, check, process):
    """Host frames (rows 3 w bytes apart) and device frames at an odd pitch from an odd offset."""
    stride = 3 * w + 1
    host, dev = make(), make()
    buf = DeviceFrames(pkg, 1, h, stride, 3)
    wants = []
    for f, frame in enumerate(frames):
        want = ref.process([frame])
        check(host, ref, process(host, [frame]), want, ("host", f))
        check(dev, ref, process(dev, buf.put([frame], f), stride=stride, offset=3), want, ("device", f))
        wants.append(want[0])
    host.close(); dev.close()
    buf.buf.free()
    return wants


@pytest.mark.parametrize("scale", G.SIDE_SCALES)
@pytest.mark.parametrize("h,w", G.SIDE_SHAPES)
def test_max_side(pkg, h, w, scale):
    """The largest side the modules accept, along x (128 reader tiles and 512 filter tiles across at scale 1) and along y, with a
    rectangle across an edge of the reader's and of the filter's tiles at either scale and one up to the last pixel."""
    wants = side(pkg, h, w, G.side_motion_frames(h, w), MR.Ref(1, h, w, scale=scale, **G.SIDE_MOTION),
                 lambda: pkg.MotionDetector(1, h, w, scale=scale, **G.SIDE_MOTION), TM.check, lambda d, fr, **kw: d.process(fr, **kw))
    assert [w_["n_regions_total"] for w_ in wants] == [0, 0, 0, 1, 1, 0]
    wants = side(pkg, h, w, G.side_leftobj_frames(h, w), LR.Ref(1, h, w, scale=scale, **G.SIDE_LEFTOBJ),
                 lambda: pkg.LeftObjectDetector(1, h, w, scale=scale, **G.SIDE_LEFTOBJ), TL.check, lambda d, fr, **kw: d.process(fr, want_objects=True, **kw))
    assert sum(len(w_["events"]) for w_ in wants) == 2
    wants = side(pkg, h, w, G.side_health_frames(h, w), HR.Ref(1, h, w, scale=scale, **G.SIDE_HEALTH),
                 lambda: pkg.ingestion.CameraHealth(1, h, w, scale=scale, **G.SIDE_HEALTH), TH.check, lambda m, fr, **kw: m.process(fr, **kw))
    assert any(w_["events"] for w_ in wants)


def test_a_side_of_32769_is_refused(pkg):
    """Before any launch: no handle is made."""
    E = pkg._ffi.RtmodtError
    for make in (pkg.MotionDetector, pkg.LeftObjectDetector, pkg.ingestion.CameraHealth):
        for h, w in ((4, G.MAX_SIDE + 1), (G.MAX_SIDE + 1, 4)):
            with pytest.raises(E) as e:
                make(1, h, w)
            assert e.value.code == pkg._ffi.E_INVALID and "bad frame geometry" in e.value.msg, (make, h, w)
