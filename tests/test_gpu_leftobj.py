"""GPU: the left / removed object detector (csrc/leftobj.hip, csrc/leftobj_rule.h) against the restatement tests/leftobj_ref.py: after
every frame the results, the regions, the events, the retired list, the whole cell state, the mask, the luma grid and the ledger are
the restatement's; the interface's behaviour and refusals; the pipeline's left_objects stage.  Every comparison is == on integers.
PARITY UNPINNED: the reference has no counterpart and no default has been validated on real footage."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import leftobj_cases as LC
import leftobj_ref as LR
from test_gpu_motion import DeviceFrames, padded

pytestmark = pytest.mark.gpu

#: (h, w, stride): partial edge cells in both directions, odd pitches; 150 x 530 spans several 64 x 16 tiles in x and y at every
#: scale and more than one 4096-cell chunk at scale 1 and 2
GEOMETRIES = [(37, 70, 211), (70, 37, 117), (150, 530, 1601)]
SCALES = [1, 2, 4, 8]
KEYS = ("stream", "status", "frames_seen", "n_fg", "n_static", "n_regions_total", "n_objects", "dropped", "next_oid", "regions", "events", "retired", "objects")


def as_dict(r):
    return dict(stream=r.stream, status=r.status, frames_seen=r.frames_seen, n_fg=r.n_fg, n_static=r.n_static, n_regions_total=r.n_regions_total,
                n_objects=r.n_objects, dropped=r.dropped, next_oid=r.next_oid, regions=r.regions,
                events=[dict(oid=e.oid, kind=e.kind, box=e.box, area=e.area, first_frame=e.first_frame, frame_id=e.frame_id, owner=e.owner) for e in r.events],
                retired=r.retired, objects=r.objects)


def check(det, ref, got, want, what):
    """One call's results and everything a stream holds afterwards against the restatement."""
    assert len(got) == len(want), what
    for g, w_ in zip(got, want):
        g = as_dict(g)
        for k in KEYS:
            assert g[k] == w_[k], (what, k, g[k] if not isinstance(g[k], list) else g[k][:3], w_[k] if not isinstance(w_[k], list) else w_[k][:3])
        check_stream(det, ref, w_["stream"], what)


def check_stream(det, ref, s, what):
    assert np.array_equal(det.mask(s), ref.masks[s]), (what, "mask", s)
    cells, luma, seen = det.state(s)
    bg, cand, age, miss, flags, rluma, rseen = ref.state(s)
    for name, r_ in (("bg", bg), ("cand", cand), ("age", age), ("miss", miss), ("flags", flags)):
        assert np.array_equal(cells[name].astype(np.int64), r_), (what, name, s)
    assert np.array_equal(luma.astype(np.int64), rluma) and seen == rseen, (what, "luma / frames_seen", s)
    assert det.ledger(s) == (ref.ledgers[s], ref.next_oid[s]), (what, "ledger", s)


@functools.lru_cache(maxsize=None)
def sequences(h, w, streams):
    return [LC.sequence(h, w, 100 * h + s) for s in range(streams)]


# ---- the scripted sequence over geometries and scales -------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("h,w,stride", GEOMETRIES)
def test_sequence_equals_restatement(pkg, h, w, stride, scale):
    """Host frames at the odd pitch; device frames at the same pitch from a base offset by 1 (the byte path); device frames at
    the pitch rounded up to a multiple of 4 from a base offset by 4 (the wide path).  One restatement for the three."""
    S = 2
    seqs = sequences(h, w, S)
    kw = dict(scale=scale, **LC.SEQ_CFG)
    ref = LR.Ref(S, h, w, **kw)
    wide_stride = (stride + 3) // 4 * 4
    dets = [pkg.LeftObjectDetector(S, h, w, **kw) for _ in range(3)]
    dev1, dev4 = DeviceFrames(pkg, S, h, stride, 1), DeviceFrames(pkg, S, h, wide_stride, 4)
    statuses, events, retired = [], [], []
    for f in range(LC.N_FRAMES):
        frames = [seqs[s][f] for s in range(S)]
        want = ref.process(frames)
        statuses.append(want[0]["status"])
        events += [(f, e["oid"], e["kind"]) for e in want[0]["events"]]
        retired += [(f,) + r for r in want[0]["retired"]]
        keep = [padded(fr, stride, f * 7 + s) for s, fr in enumerate(frames)]
        check(dets[0], ref, dets[0].process([v for _, v in keep], want_objects=True), want, ("host", f))
        check(dets[1], ref, dets[1].process(dev1.put(frames, f), stride=stride, offset=1, want_objects=True), want, ("device + 1", f))
        check(dets[2], ref, dets[2].process(dev4.put(frames, f), stride=wide_stride, offset=4, want_objects=True), want, ("device + 4", f))
    assert all(d.last_kernel_ms() >= 0 for d in dets)
    if (h, w) == (150, 530):
        # what the scripted scene answers, asserted on the restatement so that equality cannot hide an empty comparison: the block is
        # static static_frames after PLACE (the walker's two frames are ridden out), alarms alarm_frames calls after its birth, is
        # absorbed absorb_frames after it; the hole it leaves alarms REMOVED; the global step resets
        W_, C_, S_, X_ = LR.WARMUP, LR.CLEAR, LR.STATIC, LR.SCENE_CHANGE
        born = LC.PLACE + 4
        gone = LC.TAKE + 4
        assert statuses == ([W_] * 4 + [C_] * (born - 4) + [S_] * 31 + [C_] * (gone - born - 31) + [S_] * (LC.STEP_AT - gone)
                            + [X_] + [W_] * (LC.N_FRAMES - LC.STEP_AT - 1))
        assert events == [(born + 7, 1, LR.ABANDONED), (gone + 7, 2, LR.REMOVED)]
        assert retired == [(born + 30, 1, LR.ABSORBED, 1), (LC.STEP_AT, 2, LR.RESET, 1)]
    for d in dets:
        d.close()
    dev1.buf.free(); dev4.buf.free()


# ---- the ledger and the regions at scale ---------------------------------------------------------------------------------
BLOB = dict(scale=1, warmup=1, static_frames=2, alarm_frames=3, min_neighbors=4, min_area=4, miss_frames=1)


def run_cells(pkg, gh, gw, scenes, tracks=None, streams=1, **kw):
    """Grey frames whose cells are ``scenes[f]`` through a detector and the restatement, compared after every frame."""
    cfg = dict(BLOB, **kw)
    ref_kw = dict(cfg)
    det = pkg.LeftObjectDetector(streams, gh, gw, **cfg)
    ref = LR.Ref(streams, gh, gw, owner_classes=ref_kw.pop("owner_classes", (0,)), report_tracked=ref_kw.pop("report_tracked", ()), **ref_kw)
    out = []
    for f, cells in enumerate(scenes):
        frame = LC.cells_to_frame(cells, 1, gh, gw)
        tr = None if tracks is None else tracks[f]
        want = ref.process([frame] * streams, tracks=None if tr is None else [tr] * streams)
        check(det, ref, det.process([frame] * streams, tracks=None if tr is None else [tr] * streams, want_objects=True), want, f)
        out.append(want[0])
    det.close()
    return out


def test_seventy_blobs_fill_a_ledger_past_one_wave(pkg):
    gh, gw = 40, 60
    flat = np.full((gh, gw), 100, np.uint8)
    blobs, boxes = LC.blob_cells(gh, gw, 70)
    scenes = [flat] + [blobs] * 6
    out = run_cells(pkg, gh, gw, scenes, max_objects=256, max_regions=256)
    assert out[-1]["n_objects"] == 70 and [o["cells"] for o in out[-1]["objects"]] == boxes and out[-1]["dropped"] == 0
    assert sum(len(o["events"]) for o in out) == 70 and {e["kind"] for o in out for e in o["events"]} == {LR.ABANDONED}
    # four rows only: 66 births are dropped on every call, the four first regions keep their rows
    out = run_cells(pkg, gh, gw, scenes, max_objects=4, max_regions=256)
    assert out[-1]["n_objects"] == 4 and out[-1]["dropped"] == 66 and [o["oid"] for o in out[-1]["objects"]] == [1, 2, 3, 4]
    # 32 stored regions of 70
    out = run_cells(pkg, gh, gw, scenes, max_objects=256, max_regions=32)
    assert out[-1]["n_regions_total"] == 70 and len(out[-1]["regions"]) == 32 and out[-1]["n_objects"] == 32
    # then the blobs go: every row clears after miss_frames + 1 unmatched calls
    out = run_cells(pkg, gh, gw, scenes + [flat] * 6, max_objects=256, max_regions=256, occlusion=0)
    assert sorted(r[1] for o in out for r in o["retired"]) == [LR.CLEARED] * 70 and out[-1]["n_objects"] == 0


def test_rows_that_alarm_and_absorb_make_room_for_births_that_alarm(pkg):
    """alarm_frames 1 and a full ledger: four attended rows lose their owner on the call that absorbs them, so they alarm and leave,
    and the four regions that were dropped until then are born and alarm at once: 2 x max_objects events in one call."""
    gh, gw = 40, 60
    flat = np.full((gh, gw), 100, np.uint8)
    old = flat.copy()
    for y0 in (5, 20):
        for x0 in (5, 15):
            old[y0:y0 + 4, x0:x0 + 4] = 200
    both = old.copy()
    both[:, 30:] = old[:, :30]                                       # the same four, 30 cells to the right
    owner = (np.int64([77]), np.float32([[0, 0, 28, 40]]), np.int32([0]))
    out = run_cells(pkg, gh, gw, [flat, old] + [both] * 6, [None] + [owner] * 5 + [None] * 2, max_objects=4, alarm_frames=1, absorb_frames=4, attend_margin=0)
    assert [len(o["events"]) for o in out] == [0] * 6 + [8, 0] and [o["dropped"] for o in out] == [0, 0, 0, 4, 4, 4, 0, 0]
    assert [(e["oid"], e["owner"]) for e in out[6]["events"]] == [(k, 77) for k in (1, 2, 3, 4)] + [(k, -1) for k in (5, 6, 7, 8)]
    assert out[6]["retired"] == [(k, LR.ABSORBED, 1) for k in (1, 2, 3, 4)] and [o["oid"] for o in out[6]["objects"]] == [5, 6, 7, 8]


def test_two_blobs_grow_into_one_region(pkg):
    gh, gw = 20, 30
    flat = np.full((gh, gw), 100, np.uint8)
    two = flat.copy()
    two[5:9, 4:8] = two[5:9, 12:16] = 200
    one = two.copy()
    one[5:9, 8:12] = 200
    out = run_cells(pkg, gh, gw, [flat] + [two] * 4 + [one] * 5)
    assert out[4]["n_objects"] == 2 and out[-1]["n_regions_total"] == 1
    # the merged region takes the lower oid (the tie on shared cells); the other row clears
    assert [o["oid"] for o in out[-1]["objects"]] == [1] and (2, LR.CLEARED, 1) in [r for o in out for r in o["retired"]]


# ---- tracks ------------------------------------------------------------------------------------------------------------------
def test_three_hundred_tracks_owner_leaves_then_the_alarm(pkg):
    """A list past one pass of 256 threads; the owner (the largest attending id wins) stands by, leaves, and alarm_frames later the
    alarm names it.  A covering track of no report class holds the timer; one of a report class makes it TRACKED_STATIC."""
    gh, gw = 30, 40
    flat = np.full((gh, gw), 100, np.uint8)
    bag = flat.copy()
    bag[10:14, 10:15] = 200                                          # the region's pixel box: (10, 10, 15, 14)
    rng = np.random.default_rng(5)
    far = np.float32([[30 + (i % 7), 20 + (i % 5), 33 + (i % 7), 24 + (i % 5)] for i in range(298)])      # class 0, beyond the margin
    ids = np.arange(1000, 1300, dtype=np.int64)
    near = np.float32([[16.5, 9.0, 19.0, 15.0], [2.0, 2.0, 8.0, 8.0]])    # 2 px right of the bag: attends at margin 2; the other does not
    cls = np.zeros(300, np.int32)
    perm = rng.permutation(300)
    with_owner = (ids[perm], np.concatenate([far, near])[perm], cls[perm])
    without = (ids[:298], far, cls[:298])
    scenes = [flat] + [bag] * 12
    tracks = [None] + [with_owner] * 5 + [without] * 7
    out = run_cells(pkg, gh, gw, scenes, tracks, attend_margin=2, max_tracks=300)
    assert out[3]["regions"][0]["attended"] == 1 and out[5]["objects"][0]["owner"] == 1298 and out[5]["objects"][0]["idle"] == 0
    ev = [(f, e["kind"], e["owner"]) for f, o in enumerate(out) for e in o["events"]]
    assert ev == [(8, LR.ABANDONED, 1298)]                            # the owner is last seen on call 5: idle 1, 2, 3 on calls 6, 7, 8
    out = run_cells(pkg, gh, gw, scenes, [None] + [with_owner] * 12, attend_margin=1, max_tracks=300)     # one pixel short: never attended
    assert [(f, e["owner"]) for f, o in enumerate(out) for e in o["events"]] == [(4, -1)]
    # a standing person (class 0 is an owner class too) over the bag, then a parked "car" of class 2
    person = (np.int64([7]), np.float32([[9, 8, 16, 20]]), np.int32([0]))
    out = run_cells(pkg, gh, gw, scenes, [None] + [person] * 12)
    assert not any(o["events"] for o in out) and out[-1]["regions"][0]["covered"] == 1 and out[-1]["objects"][0]["idle"] == 0
    car = (np.int64([8]), np.float32([[9, 8, 16, 20]]), np.int32([2]))
    out = run_cells(pkg, gh, gw, scenes, [None] + [car] * 12)
    assert not any(o["events"] for o in out) and out[-1]["objects"][0]["idle"] == 0       # covered, no report class: the timer holds
    out = run_cells(pkg, gh, gw, scenes, [None] + [car] * 12, report_tracked=(2,))
    assert [(e["kind"], e["owner"]) for o in out for e in o["events"]] == [(LR.TRACKED_STATIC, -1)] and out[-1]["regions"][0]["covered"] == 3


@pytest.mark.parametrize("which", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_tracker_handles_equal_the_list_of_the_selected_tracks(pkg, which):
    import test_gpu_speed as TS
    make, with_frames, passed = TS._trackers(pkg)[which]
    core = make()
    S, N, H, W = TS.S, TS.N, TS.FH, TS.FW
    kw = dict(scale=4, warmup=1, static_frames=2, alarm_frames=4, min_neighbors=4, min_area=4, miss_frames=1, attend_margin=8, covered_pm=300,
              owner_classes=(0, 1), report_tracked=(2,), max_tracks=64)
    dev, host = (pkg.LeftObjectDetector(S, H, W, **kw) for _ in range(2))
    ref = LR.Ref(S, H, W, **kw)
    rng = np.random.default_rng(9)
    cells = np.full((H // 4, W // 4), 100, np.uint8)
    lit = cells.copy()
    for k in range(12):                                               # a left object of 6 x 5 cells in each of the scene's lanes
        x0 = int(rng.integers(5, 80))
        lit[3 + 7 * k:8 + 7 * k, x0:x0 + 6] = 190
    frames_rgb = [np.random.default_rng(s).integers(0, 256, (H, W, 3), dtype=np.uint8) for s in range(S)]
    tracker = SimpleNamespace(_core=core, report="matched") if which == "bytetrack" else core
    n_pass = n_state = n_ev = n_att = 0
    for f in range(24):
        xyxy = np.zeros((S, N, 4), np.float32); conf = np.zeros((S, N), np.float32); cls = np.zeros((S, N), np.int32); cnt = np.zeros(S, np.int32)
        for s in range(S):
            xy, cf, cl = TS.scene(f, s)
            xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf, cl, len(cf)
        if with_frames:
            core.update_batch(xyxy, conf, cls, cnt, frames=frames_rgb)
        else:
            core.update_batch(xyxy, conf, cls, cnt)
        frame = LC.cells_to_frame(cells if f == 0 else lit, 4, H, W)
        lists = []
        for s in range(S):
            st = core.snapshot(s)
            idx = passed(core, st)
            n_state += len(st["ids"]); n_pass += len(idx)
            lists.append((np.int64([st["ids"][i] for i in idx]), np.float32([st["xyxy"][i] for i in idx]).reshape(-1, 4), np.int32([st["cls"][i] for i in idx])))
        want = ref.process([frame] * S, tracks=lists)
        check(dev, ref, dev.process([frame] * S, tracker=tracker, want_objects=True), want, (which, f, "device state"))
        check(host, ref, host.process([frame] * S, tracks=lists, want_objects=True), want, (which, f, "list"))
        n_ev += sum(len(w_["events"]) for w_ in want)
        n_att += sum(g["attended"] + (g["covered"] & 1) for w_ in want for g in w_["regions"])
    assert 0 < n_pass < n_state and n_ev > 0 and n_att > 0, (n_pass, n_state, n_ev, n_att)
    with pytest.raises(TypeError):
        dev.process([frame] * S, tracker=object())
    dev.close(); host.close(); core.close()


# ---- the ignore grid, the restart, reset, unnamed streams ---------------------------------------------------------------
def test_ignore_grid_and_polygons(pkg):
    h, w, scale = 64, 96, 4
    kw = dict(scale=scale, warmup=1, static_frames=2, alarm_frames=3)
    det, ref = pkg.LeftObjectDetector(1, h, w, **kw), LR.Ref(1, h, w, **kw)
    cells = np.full((16, 24), 100, np.uint8)
    lit = cells.copy()
    lit[2:6, 2:7] = 200                                               # a "TV screen" inside the polygon
    lit[9:13, 14:19] = 200                                            # a bag outside
    grid = det.ignore_polygons(0, [[(4, 4), (34, 4), (34, 30), (4, 30)]])
    want_grid = np.zeros((16, 24), np.uint8)
    want_grid[1:7, 1:8] = 1                                           # centres 4k + 2 inside 4 < x < 34, 4 < y < 30
    assert np.array_equal(grid, want_grid) and np.array_equal(det.ignore(0), want_grid)
    ref.set_ignore(want_grid)
    got = []
    for f, c_ in enumerate([cells] + [lit] * 5):
        frame = LC.cells_to_frame(c_, scale, h, w)
        want = ref.process([frame])
        check(det, ref, det.process([frame], want_objects=True), want, f)
        got.append(want[0])
    assert [g["cells"] for g in got[-1]["regions"]] == [(14, 9, 18, 12)] and len([e for o in got for e in o["events"]]) == 1
    inv = det.ignore_polygons(0, [[(4, 4), (34, 4), (34, 30), (4, 30)]], invert=True)
    assert np.array_equal(inv, 1 - want_grid)
    det.reset(0)                                                      # the ignore grid stays
    ref.reset(0); ref.set_ignore(1 - want_grid)
    check_stream(det, ref, 0, "after reset")
    for f, c_ in enumerate([cells] + [lit] * 5):
        frame = LC.cells_to_frame(c_, scale, h, w)
        want = ref.process([frame])
        check(det, ref, det.process([frame], want_objects=True), want, ("inverted", f))
    assert [g["cells"] for g in want[0]["regions"]] == [(2, 2, 6, 5)] and want[0]["objects"][0]["oid"] == 1
    det.close()


def test_restart_round_trip_and_unnamed_streams(pkg):
    h, w = 37, 70
    kw = dict(scale=2, **LC.SEQ_CFG)
    seqs = sequences(h, w, 2)
    ref = LR.Ref(2, h, w, **kw)
    det = pkg.LeftObjectDetector(2, h, w, **kw)
    for f in range(25):                                               # mid-sequence: the object lives and has alarmed
        want = ref.process([seqs[0][f], seqs[1][f]])
        check(det, ref, det.process([seqs[0][f], seqs[1][f]], want_objects=True), want, f)
    assert ref.ledgers[0] and ref.ledgers[0][0]["alarmed"] == 1
    fresh = pkg.LeftObjectDetector(2, h, w, **kw)
    for s in range(2):
        cells, luma, seen = det.state(s)
        fresh.load_state(cells, luma, seen, s)
        fresh.load_mask(det.mask(s), s)
        fresh.load_ledger(*det.ledger(s), stream=s)
        check_stream(fresh, ref, s, ("loaded", s))
    det.close()
    for f in range(25, 50):                                           # only stream 1 is named on odd frames; stream 0 keeps its state
        if f % 2:
            want = ref.process([seqs[1][f]], streams=[1], frame_id=f)
            check(fresh, ref, fresh.process([seqs[1][f]], streams=[1], frame_id=f, want_objects=True), want, f)
            check_stream(fresh, ref, 0, ("unnamed", f))
        else:
            want = ref.process([seqs[1][f], seqs[0][f]], streams=[1, 0], frame_id=f)
            check(fresh, ref, fresh.process([seqs[1][f], seqs[0][f]], streams=[1, 0], frame_id=f, want_objects=True), want, f)
    assert ref.next_oid[0] >= 2 and ref.next_oid[1] >= 2                # each stream has seen its block absorbed and its hole born
    assert fresh.process([seqs[0][50], seqs[1][50]], outputs=False) == []             # no output asked for: nothing comes back
    ref.process([seqs[0][50], seqs[1][50]])
    check_stream(fresh, ref, 0, "no outputs"); check_stream(fresh, ref, 1, "no outputs")
    fresh.reset()
    ref.reset(0); ref.reset(1)
    check_stream(fresh, ref, 0, "reset"); check_stream(fresh, ref, 1, "reset")
    fresh.close()


def test_refusals_launch_nothing(pkg):
    """Every bad argument is rejected by the host before any launch; the state afterwards is untouched."""
    h, w = 37, 70
    det = pkg.LeftObjectDetector(2, h, w, scale=2, max_tracks=4)
    ok = np.zeros((h, w, 3), np.uint8)
    E = pkg._ffi.RtmodtError
    for bad in (lambda: det.process([np.zeros((h + 1, w, 3), np.uint8)] * 2), lambda: det.process([ok], streams=[2]), lambda: det.process([ok, ok], streams=[1, 1]),
                lambda: det.process([ok], streams=[-1]), lambda: det.process([ok] * 3, streams=[0, 1, 0]),
                lambda: det.process([ok], streams=[0], tracks=(np.arange(5), np.zeros((5, 4), np.float32), np.zeros(5, np.int32)))):
        with pytest.raises((E, ValueError)) as e:
            bad()
        assert not isinstance(e.value, E) or e.value.code == pkg._ffi.E_INVALID
    L = pkg._ffi.lib()
    fid = np.zeros(2, np.int64)
    null = (C.c_void_p * 2)(ok.ctypes.data, None)
    assert L.rtmodt_leftobj_process(det._h, null, None, pkg._ffi.ptr(fid), 2, h, w, 3 * w, 0, None, None) == pkg._ffi.E_INVALID
    trk = pkg.tracking.tracker._ByteTrackCore(0.5, 5, 0.3, n_streams=3, max_tracks=8, max_dets=8)        # three streams against two
    with pytest.raises(E) as e:
        det.process([ok, ok], tracker=trk)
    assert e.value.code == pkg._ffi.E_INVALID and "streams" in e.value.msg
    trk.close()
    _, _, seen = det.state(0)
    assert seen == 0 and det.ledger(0) == ([], 1)
    with pytest.raises(E):
        det.last_kernel_ms()
    det.close()


# ---- the pipeline stage ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(pkg, tmp_path_factory):
    import os
    path = os.path.join(str(tmp_path_factory.mktemp("weights_leftobj")), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    yield det
    det.close()


def test_pipeline_left_objects_stage(pkg, detector):
    """A block put down on frame 6 of 30 still frames alarms once; the stage row stands directly before snapshots, else before
    privacy, else before visualization; the detector's state after the run is the restatement's.  (track_thresh 0.99: the synthetic network's detections
    found no track, so the restatement runs without tracks.)"""
    bgd = np.clip(LC.background(320, 320), 0, 255).astype(np.uint8)
    frames = []
    for f in range(30):
        fr = bgd.copy()
        if f >= 6:
            fr[100:180, 120:220] = 230
        frames.append(fr)
    kw = dict(scale=4, warmup=4, static_frames=5, alarm_frames=8, miss_frames=3)
    ref = LR.Ref(1, 320, 320, **kw)
    want = [ref.step(0, fr, f + 1) for f, fr in enumerate(frames)]              # the source counts frames from 1
    assert sum(len(w_["events"]) for w_ in want) == 1 and want[17]["events"][0]["kind"] == LR.ABANDONED
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)     # noqa: E731
    src = lambda: pkg.pipeline.SyntheticSource(np.stack(frames))                                          # noqa: E731
    trk = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.99)                                  # noqa: E731
    base = pkg.pipeline.run(src(), detector, trk(), prof(), max_frames=30)
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}                                             # noqa: E731
    for extra, before in ((dict(), "visualization"), (dict(snapshots=pkg.visualization.SnapshotGallery(max_tracks=2048)), "snapshots"),
                          (dict(snapshots=pkg.visualization.SnapshotGallery(max_tracks=2048), privacy=pkg.visualization.PrivacyMask(mode="fill")), "snapshots"),
                          (dict(privacy=pkg.visualization.PrivacyMask(mode="fill")), "privacy"),
                          (dict(renderer=pkg.FrameRenderer(show_fps=False)), "visualization")):
        lo = pkg.LeftObjectDetector(1, 320, 320, **kw)
        p = prof()
        out = pkg.pipeline.run(src(), detector, trk(), p, max_frames=30, left_objects=lo, **extra)
        assert (out["left_object_alarms"], out["left_objects_retired"]) == (1, 0), extra
        assert "left_objects_mean_ms" in rows(out) - rows(base) and rows(base) <= rows(out)
        order = list(p.STAGE_ORDER)
        assert order.index("left_objects") + 1 == order.index(before), order
        check_stream(lo, ref, 0, ("pipeline", tuple(extra)))
        lo.close()
    p = prof()
    none = pkg.pipeline.run(src(), detector, trk(), p, max_frames=30, left_objects=None)
    assert set(none) == set(base) and not {"left_object_alarms", "left_objects_retired"} & set(none)
    assert list(p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER
    assert none["last_detections"] == base["last_detections"] and none["last_tracks"] == base["last_tracks"] and none["events"] == base["events"]
