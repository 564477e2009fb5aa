"""GPU: the camera-motion estimator (csrc/gmc.hip) against its restatement (tests/gmc_ref.py): after every frame of a sequence every
intermediate rtmodt_gmc_debug returns, the warp's bits and the status are the restatement's.  PARITY UNPINNED: OpenCV and BoT-SORT's
GMC are installed nowhere this runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import botsort_ref as B  # noqa: E402
import gmc_ref as G  # noqa: E402
from gmc_run import _bits, _est, _run, _same  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS = [(3, -2), (-5, 4), (0, 7), (6, 6), (-4, -1)]         # five moves: a 6-frame sequence


def test_160x96_at_full_resolution(pkg):
    seen = _run(pkg, [G.pan_sequence(96, 160, 1, STEPS, margin=32)], downscale=1)
    assert seen[0] == [G.FIRST] and all(s == [G.OK] for s in seen[1:])


def test_322x182_padded_rows_dropped_cells_and_a_partial_block_row(pkg):
    frames = []
    for f in G.pan_sequence(182, 322, 2, [(2 * x, 2 * y) for x, y in STEPS], margin=64):
        buf = np.zeros((182, 327, 3), np.uint8)
        buf[:, :322] = f
        frames.append(buf[:, :322])
    assert frames[0].strides[0] == 981 > 3 * 322
    seen = _run(pkg, [frames], downscale=2)
    assert all(s == [G.OK] for s in seen[1:])


def test_1080p_has_more_blocks_than_a_workgroup_has_threads(pkg):
    seen = _run(pkg, [G.pan_sequence(1080, 1920, 3, [(4 * x, 4 * y) for x, y in STEPS], margin=64)], downscale=2)
    assert all(s == [G.OK] for s in seen[1:])


def test_eight_streams_with_their_own_motion_in_one_call(pkg):
    h, w = 192, 320
    cvs = [G.canvas(h + 120, w + 120, 20 + s) for s in range(8)]
    warps = [None, G.similarity(0.4, 1.0, 3.3, -2.6, (160, 96)), G.similarity(-0.3, 1.01, -5.5, 1.25, (160, 96)), None, None, None, None,
             G.similarity(0.0, 0.99, 0.5, 0.5, (160, 96))]
    streams = []
    for s in range(8):
        if s == 3:
            streams.append([np.full((h, w, 3), 90, np.uint8)] * 6)                       # flat
        elif warps[s] is not None:                                                      # sub-pixel motion: alternate the two views
            streams.append([G.crop(cvs[s], 60, 60, h, w) if f % 2 == 0 else G.sample(cvs[s], warps[s], h, w, (60, 60)) for f in range(6)])
        else:
            streams.append(G.pan_sequence(h, w, 20 + s, [((s + 1) * x, (s - 4) * y) for x, y in STEPS], margin=60))
    D = pkg.Detections
    masks = [None] * 8
    masks[5] = D(np.asarray([[0, 0, w, h]], F32), np.ones(1, F32), np.zeros(1, np.int32))                       # fully masked
    masks[0] = D(np.asarray([[40, 40, 120, 100], [200, 20, 260, 180]], F32), np.asarray([0.9, 0.05], F32), np.zeros(2, np.int32))
    seen = np.asarray(_run(pkg, streams, masks=masks, reset_at=(6, 3), downscale=2))
    assert (seen[0] == G.FIRST).all() and (seen[1:, 3] == G.FEW_BLOCKS).all() and (seen[1:, 5] == G.FEW_BLOCKS).all()
    assert seen[3, 6] == G.FIRST and seen[4, 6] == G.OK and (seen[1:, [0, 1, 2, 4, 7]] == G.OK).all()


def test_64_streams(pkg):
    streams = [G.pan_sequence(96, 160, 40 + s, [((s % 5 - 2) * x, (s % 3 - 1) * y) for x, y in STEPS], margin=64) for s in range(64)]
    seen = np.asarray(_run(pkg, streams, downscale=1))
    assert (seen[0] == G.FIRST).all() and (seen[1:] == G.OK).mean() > 0.5


def test_striped_frames_tie_in_both_stages(pkg):
    """A pattern of period 4 in x and y at level 0: level 1 is flat (every coarse SAD is 0), and a block matches at every shift that
    is a multiple of 4 inside the search square; the tie rule has to pick the same one."""
    y, x = np.mgrid[0:96 + 8, 0:160 + 8]
    base = np.repeat((40 + 150 * ((x % 4 < 2) ^ (y % 4 < 2)))[..., None], 3, 2).astype(np.uint8)
    frames = [np.ascontiguousarray(base[oy:oy + 96, ox:ox + 160]) for ox, oy in ((0, 0), (1, 0), (1, 2), (3, 3), (0, 0), (2, 1))]
    _run(pkg, [frames], downscale=1, min_sep=8.0)
    ref = G.GmcRef(downscale=1)
    ref.estimate(frames[0])
    dbg = ref.estimate(frames[1])[2]
    assert (dbg["table"] == 0).all() and dbg["coarse"] == (0, 0)
    assert set(dbg["blk"]["dx"][dbg["blk"]["reason"] == 0].tolist()) == {-1} and (dbg["blk"]["sad"] == 0).all()      # -1 and +3 tie on the SAD


def test_no_coarse_stage_widest_search_and_256_hypotheses(pkg):
    seen = _run(pkg, [G.pan_sequence(96, 160, 5, STEPS, margin=32)], downscale=1, coarse_search=0, search=8, n_hyp=256)
    assert all(s == [G.OK] for s in seen[1:])


def test_widest_coarse_search_follows_100_px_a_frame(pkg):
    """coarse_search = 16 at 640x360, d = 2: a table of 33 x 33 shifts (more than a workgroup's threads), moves beyond the 64 px
    that the default of 8 reaches."""
    frames = G.pan_sequence(360, 640, 8, [(100, -90), (-96, 84), (-70, -100), (66, 40), (0, 66)], margin=120)
    seen = _run(pkg, [frames], downscale=2, coarse_search=16)
    assert all(s == [G.OK] for s in seen[1:])


def test_limits_are_refused_before_any_launch_and_the_handle_stays_usable(pkg):
    ffi = pkg._ffi
    L = ffi.lib()
    gmc = import_gmc(pkg)
    cfg = gmc.default_cfg()
    cfg.n_streams = 65
    h = C.c_void_p()
    assert L.rtmodt_gmc_create(C.byref(cfg), C.byref(h)) == ffi.E_CAPACITY and not h.value
    for bad in (dict(downscale=3), dict(search=0), dict(coarse_search=17), dict(n_hyp=257), dict(min_blocks=1)):
        with pytest.raises(ffi.RtmodtError) as e:
            _est(pkg, **bad)
        assert e.value.code == ffi.E_INVALID
    est = _est(pkg, downscale=1)
    frames = G.pan_sequence(96, 160, 1, STEPS[:2], margin=32)
    ref = G.GmcRef(downscale=1)

    def code(frame):
        with pytest.raises(ffi.RtmodtError) as e:
            est.estimate([frame])
        return e.value.code
    assert code(np.zeros((1024, 1040, 3), np.uint8)) == ffi.E_CAPACITY                 # 65 x 64 = 4160 blocks
    assert code(np.zeros((96, 3856, 3), np.uint8)) == ffi.E_CAPACITY                   # wider than 3840
    assert code(np.zeros((79, 160, 3), np.uint8)) == ffi.E_INVALID                     # level 1 is 40 x 19 < 20
    est.estimate([frames[0]]); ref.estimate(frames[0])
    assert code(np.zeros((112, 160, 3), np.uint8)) == ffi.E_INVALID                    # a changed size without a reset
    with pytest.raises((ffi.RtmodtError, ValueError)):
        est.estimate([frames[1]], [pkg.Detections(np.zeros((1025, 4), F32), np.zeros(1025, F32), np.zeros(1025, np.int32))])
    warp, status = est.estimate([frames[1]])                                            # none of the refused calls moved the state
    _same(est, 0, warp[0], status[0], ref.estimate(frames[1]), "after refusals")
    assert status[0] == G.OK
    est.reset()
    assert est.estimate([np.ascontiguousarray(frames[2][:80])])[1][0] == G.FIRST        # after a reset the size may change
    est.close()


def import_gmc(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + ".tracking.gmc")


@pytest.fixture(scope="module")
def wdir(tmp_path_factory):
    return tmp_path_factory.mktemp("weights_gmc")


def _detector(pkg, wdir, batch):
    path = os.path.join(str(wdir), "yolov8n_320_noise.rtw")
    if not os.path.exists(path):
        pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    return pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, batch=batch, warmup=False, autotune=False)


def test_estimate_from_detector_equals_the_same_boxes_from_the_host(pkg, wdir):
    Bn = 2
    det = _detector(pkg, wdir, Bn)
    a, b = _est(pkg, n_streams=Bn, downscale=2, mask_conf=0.0, max_boxes=20), _est(pkg, n_streams=Bn, downscale=2, mask_conf=0.0, max_boxes=20)
    streams = [G.pan_sequence(320, 320, 60 + s, [(2 * x, 2 * y) for x, y in STEPS[:3]], margin=48) for s in range(Bn)]
    masked = 0
    for f in range(4):
        fr = [streams[s][f] for s in range(Bn)]
        det.enqueue(fr)
        a.estimate_from_detector(det, fr)
        wa, sa = a.result()
        got = det.fetch()
        wb, sb = b.estimate(fr, got)
        assert _bits(wa) == _bits(wb) and sa.tolist() == sb.tolist(), f
        for s in range(Bn):
            da, db = a.debug(s), b.debug(s)
            if f:
                assert all(np.array_equal(da["blk"][k], db["blk"][k]) for k in da["blk"]) and np.array_equal(da["order"], db["order"])
                masked += int((da["blk"]["reason"] == G.R_MASK).sum())
    assert masked > 0 and sum(len(d) for d in got) > 0
    a.close(); b.close(); det.close()


def _scene(h=360, w=480):
    scene = B.gmc_scene()
    return scene, G.gmc_scene_frames(scene, h, w)


def test_botsort_fed_on_the_device_equals_botsort_fed_the_host_copy_of_the_warps(pkg, wdir):
    """rtmodt_botsort_update_from_detector_gmc against rtmodt_botsort_update_from_detector fed the host copy of the same warps: the
    state is identical bit for bit after every frame.  The detector runs synthetic weights, so its boxes are noise: what the identities
    do on the scene's own detections is the next test."""
    core = __import__("importlib").import_module(pkg.__name__ + ".tracking.botsort")._BotSortCore
    det = _detector(pkg, wdir, 1)
    params = dict(track_buffer=4, track_high_thresh=0.05, track_low_thresh=0.0, new_track_thresh=0.05, max_tracks=128, max_dets=20)
    a, b = core(**params), core(**params)
    ga, gb = _est(pkg, downscale=2, mask_conf=0.5), _est(pkg, downscale=2, mask_conf=0.5)      # (the noise boxes are weak: few blocks go)
    _, frames = _scene()
    moved = 0
    for f, img in enumerate(frames):
        det.enqueue([img])
        a.update_from_detector_gmc(det, ga, [img])
        gb.estimate_from_detector(det, [img])
        warp, status = gb.result()
        b.update_from_detector(det, None, warp)
        assert _bits(ga.result()[0]) == _bits(warp)
        assert B.snapshots_equal(a.snapshot(0), b.snapshot(0)) is None, f
        moved += int(status[0] == G.OK and _bits(warp) != _bits(G.IDENTITY))
        det.fetch()
    assert moved >= 8
    for o in (a, b, ga, gb, det):
        o.close()


def test_tracker_with_an_estimator_holds_the_identities_of_the_rendered_scene(pkg):
    """The rendered gmc_scene through BotSortTracker(gmc=...).update: equal to update(warp=estimated) track for track, two identities
    at the end; without a warp the same detections fragment."""
    scene, frames = _scene()
    T, D = pkg.BotSortTracker, pkg.Detections
    with_gmc, by_hand, without = T(max_tracks=32, max_dets=16, gmc=_est(pkg, downscale=2)), T(max_tracks=32, max_dets=16), T(max_tracks=32, max_dets=16)
    est, ref = _est(pkg, downscale=2), G.GmcRef(downscale=2)
    for img, (xy, cf, cl, _, truth) in zip(frames, scene):
        d = D(xy, cf, cl)
        warp, status = est.estimate([img], [d])
        rw, rs, _ = ref.estimate(img, xy, cf)
        assert _bits(warp[0]) == _bits(rw) and status[0] == rs
        out_a, out_b = with_gmc.update(d, frame=img), by_hand.update(d, warp=warp[0])
        without.update(d)
        assert [(t.track_id, _bits(t.xyxy), t.time_since_update) for t in out_a] == [(t.track_id, _bits(t.xyxy), t.time_since_update) for t in out_b]
    assert [t.track_id for t in out_a] == [1, 2]
    assert without._core.snapshot(0)["next_id"] > 10
    with pytest.raises(ValueError, match="pass no warp"):
        with_gmc.update(d, frame=img, warp=np.eye(2, 3, dtype=F32))
    assert with_gmc.needs_frame and not by_hand.needs_frame
