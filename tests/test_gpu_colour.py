"""GPU: the colour attributes (csrc/colour.hip) against the NumPy restatement of their rules (tests/colour_ref.py), through the C ABI
and the Python class: `updated`, `retired`, the whole ledger, flags and errors compared after EVERY call, with exact equality --
odd and aligned frame geometries on the host and on the device, boxes cut by the borders, 1 x 1 and outside, sampled rectangles past
max_side, more samples than one pass of the workgroup, the occluder cap, three streams in one call, churn, more members than a
workgroup has threads, ledger overflow, state round trips, the four trackers as the source and the pipeline's colours stage."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_cases as CC  # noqa: E402
import colour_ref as R  # noqa: E402
from test_gpu_privacy import FH, FW, S, _trackers, run_scripted, scripted  # noqa: E402,F401
from test_gpu_snapshot import Frame  # noqa: E402

pytestmark = pytest.mark.gpu

THRESHOLDS = ("black_max", "chroma_min", "sat_split", "sat_hi_pm", "sat_lo_pm", "y_black", "y_white", "hue", "pink_mx", "red_brown_mx", "orange_brown_mx",
              "yellow_brown_mx")


def tuples(rows):
    """Rows of ROW_DTYPE as the restatement's tuples."""
    return [(int(r["track_id"]), int(r["first_frame"]), int(r["last_frame"]), r["hist"].ravel().tolist(), int(r["cls"]), int(r["frames_used"]), int(r["flags"]),
             int(r["track"]), int(r["frame_samples"]), [tuple(int(v) for v in l) for l in r["label"]]) for r in rows]


class Dev:
    """One ColourAttributes object, called through the C ABI with raw frame pointers, and the restatement beside it."""

    def __init__(self, pkg, cfg: R.Cfg, n_streams, max_tracks):
        self.F, self.L = pkg._ffi, pkg._ffi.lib()
        self.ca = pkg.ColourAttributes(n_streams=n_streams, max_tracks=max_tracks, inset_x_pm=cfg.inset_x_pm, top_pm=cfg.top_pm, split_pm=cfg.split_pm,
                                       bottom_pm=cfg.bottom_pm, max_side=cfg.max_side, skip_occluded=cfg.skip_occluded, min_samples=cfg.min_samples,
                                       retire_after=cfg.retire_after, classes=cfg.classes, thresholds={k: getattr(cfg, k) for k in THRESHOLDS})
        self.cfg, self.S, self.M = cfg, n_streams, max_tracks
        self.ref = [R.Stream(cfg, max_tracks) for _ in range(n_streams)]

    def close(self):
        self.ca.close()

    def got(self, d):
        ca = self.ca
        return tuples(ca._upd[d, :int(ca._cnt[0, d])]), tuples(ca._ret[d, :int(ca._cnt[1, d])])

    def same(self, s):
        """The whole ledger of stream s, labels included, equals the restatement's; a stream in error still hands its rows out."""
        rows, n = np.zeros(2 * self.M, self.ca._upd.dtype), C.c_int32(-1)
        rc = self.L.rtmodt_colour_state(self.ca._h, s, self.F.ptr(rows), C.byref(n))
        assert rc == (self.F.E_CAPACITY if self.ref[s].err else 0), self.L.rtmodt_last_error()
        assert tuples(rows[:n.value]) == self.ref[s].state(), s

    def process(self, s, ids, xy, cls, fr, fid, want_out=True):
        """One stream through rtmodt_colour_process and through the restatement; asserts the results, then the whole state."""
        ids, xy, cls = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(xy, np.float32).reshape(-1, 4), np.ascontiguousarray(cls, np.int32)
        rc = self.L.rtmodt_colour_process(self.ca._h, s, self.F.ptr(ids), self.F.ptr(xy), self.F.ptr(cls), len(ids), C.c_void_p(fr.ptr), fr.h, fr.w, fr.stride, fr.mem,
                                          fid, C.byref(self.ca._out) if want_out else None)
        code, u, r = self.ref[s].process(ids.tolist(), xy, cls.tolist(), fr.view, fid)
        if want_out:
            assert rc == code, (rc, code, self.L.rtmodt_last_error())
            assert self.got(0) == (u, r)
        else:
            assert rc == 0
        self.same(s)
        assert fr.unchanged()
        return code, u, r


BOXES = np.float32([
    [-10, 5, 9.5, 30],                   # cut by the left border
    [50, -8, 80, 30],                    # cut by the top and the right
    [20, 20, 45, 60],                    # cut by the bottom; the nearest: it hides a part of [12, 2, 33, 34]
    [30, 20, 30, 20],                    # 1 x 1: a row, no sample
    [12, 2, 33, 34],
    [-40, -40, -30, -30],                # fully outside: a row, no sample
    [np.nan, 5, 20, 20],                 # NaN: no row
    [5, 5, np.inf, 20],                  # inf: no row
    [20, 30, 10, 35],                    # inverted: no row
    [40, 10, 47, 35],                    # class 3: filtered, no row
    [52, 3, 66, 33],
])
BOX_CLS = np.int32([0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 0])


@pytest.mark.parametrize("geom", [(37, 70, 211, 1), (36, 72, 216, 0)], ids=["37x70-odd", "36x72-aligned"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_small_frame_every_box_case(pkg, device, geom):
    h, w, stride, lead = geom
    cfg = R.Cfg(min_samples=4, retire_after=5, classes=(0, 1, 2))
    d = Dev(pkg, cfg, 1, 16)
    fr = Frame(pkg, h, w, stride, 1, device, lead=lead)
    n = len(BOXES)
    ids = np.arange(100, 100 + n)[::-1].copy()                          # the list is not in id order
    code, u, r = d.process(0, ids, BOXES, BOX_CLS, fr, 10)
    assert code == 0 and len(u) == 7 and all(x[6] & R.F_NEW for x in u) and sum(x[8] == 0 for x in u) == 2 and sum(bool(x[6] & R.F_THIN) for x in u) == 2
    assert [x[7] for x in u] == [0, 1, 2, 3, 4, 5, 10]                  # in the caller's order
    d.process(0, ids, BOXES + np.float32([1, 0, 1, 0]), BOX_CLS, fr, 11)
    d.process(0, ids[:3], BOXES[:3], BOX_CLS[:3], fr, 13, want_out=False)       # no outputs: nothing waits, the ledger moves all the same
    fr2 = Frame(pkg, h, w, stride + 3, 2, device, lead=lead)
    full = np.float32([[0, 0, w - 1, h - 1]])                           # the whole frame, last pixel included: nearer than everything
    code, u, r = d.process(0, np.append(ids, 500), np.concatenate([BOXES, full]), np.append(BOX_CLS, 0), fr2, 20)      # 20 - 13 > 5: every row retires
    assert len(r) == 7 and all(x[6] & R.F_NEW for x in u) and u[-1][8] > 256
    with pytest.raises(KeyError):
        d.ca.attributes(5)
    d.close(); fr.free(); fr2.free()


@pytest.mark.parametrize("max_side", [48, 8])
def test_sampled_rectangle_past_max_side_and_one_pass(pkg, max_side):
    """200 x 260: the box's sampled rectangle is 151 x 143 -- past max_side both ways; at 48 the grid holds 38 x 48 = 1824 samples, more
    than seven passes of the 256 threads, at 8 it holds 8 x 8."""
    cfg = R.Cfg(max_side=max_side)
    d = Dev(pkg, cfg, 1, 4)
    fr = Frame(pkg, 200, 260, 3 * 260 + 1, 3, True)
    P = R.plan(cfg, (4, 3, 255, 193), 200, 260)
    assert P["rect"][2] - P["rect"][0] + 1 > 48 and P["rect"][3] - P["rect"][1] + 1 > 48 and P["sx"] > 1 and P["sy"] > 1
    assert P["nx"] * P["ny"] > 256 if max_side == 48 else P["nx"] * P["ny"] == 64
    code, u, r = d.process(0, [7, 3], [(4, 3, 255, 193), (100, 80, 140, 199)], [0, 0], fr, 0)      # box 3 reaches lower: it hides a part of box 7
    assert 0 < u[0][8] < P["nx"] * P["ny"] and u[1][8] == (25 * 45 if max_side == 48 else 7 * 8)
    d.process(0, [7], [(0, 0, 259, 199)], [0], fr, 1)
    d.close(); fr.free()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_pixel_of_the_frame_up_to_the_last(pkg, device):
    """No inset, rows 0..1000, max_side 256: a box that covers the frame samples each of its 37 x 70 pixels once, the last one included."""
    cfg = R.Cfg(inset_x_pm=0, top_pm=0, bottom_pm=1000, max_side=256, min_samples=1)
    d = Dev(pkg, cfg, 1, 2)
    fr = Frame(pkg, 37, 70, 211, 11, device)
    code, u, r = d.process(0, [1], [(-9, -9, 99, 99)], [0], fr, 0)
    assert u[0][8] == 37 * 70 and u[0][9][R.UPPER][4] == 37 * 70 and u[0][9][R.LOWER][4] == 0      # the split row 45 lies below the frame
    assert u[0][3] == np.bincount(R.name_vec(cfg, fr.view).ravel(), minlength=12).tolist() + [0] * 12
    d.close(); fr.free()


def test_nine_overlapping_boxes_reach_the_occluder_cap(pkg):
    cfg = R.Cfg(min_samples=1)
    d = Dev(pkg, cfg, 1, 16)
    fr = Frame(pkg, 37, 70, 211, 4, False)
    # box 0's sampled rectangle is rows 4..19; the nine others are nearer and hide it from row 10 + q on.  In list order (ascending id,
    # the reverse of the caller's) box 1 comes last: it is the one the cap leaves out, so row 11 stays visible
    boxes = [(2, 1, 40, 22)] + [(2 + q, 10 + q, 40 + q, 30 + q) for q in range(1, 10)]
    ids = [50 - q for q in range(10)]
    code, u, r = d.process(0, ids, boxes, [0] * 10, fr, 0)
    assert [bool(x[6] & R.F_MANY_OCCLUDERS) for x in u] == [True] + [False] * 9 and code == 0 and u[0][8] == 25 * 8
    code, u, r = d.process(0, ids[:9], boxes[:9], [0] * 9, fr, 1)       # 8 occluders: the cap exactly, no flag
    assert not any(x[6] & R.F_MANY_OCCLUDERS for x in u) and u[0][8] == 25 * 7
    d2 = Dev(pkg, R.Cfg(min_samples=1, skip_occluded=0), 1, 16)
    code, u2, _ = d2.process(0, ids, boxes, [0] * 10, fr, 0)
    assert sum(x[8] for x in u2) > sum(x[8] for x in u)
    d.close(); d2.close()


def batch(d, lists, frames, fids, named=None):
    """All streams in one call (`named`: only these, one by one) through the Python class; compares every stream with the restatement."""
    if named is None:
        d.ca.process_batch([(i, b, c) for i, b, c in lists], frames, fids)
        streams = list(range(d.S))
    else:
        streams = named
    for s in streams:
        ids, xy, cl = lists[s]
        if named is not None:
            d.ca.process((ids, xy, cl), frames[s], fids[s], stream=s)
        code, u, r = d.ref[s].process(ids.tolist(), xy, cl.tolist(), frames[s], fids[s])
        assert code == 0
        if named is None:
            assert tuples(d.ca.updated[d.ca.updated_stream == s]) == u and tuples(d.ca.retired[d.ca.retired_stream == s]) == r, s
        else:
            assert (tuples(d.ca.updated), tuples(d.ca.retired)) == (u, r), s
    for s in range(d.S):
        d.same(s)


def test_three_streams_six_frames_with_churn(pkg):
    """Tracks appear, vanish, return inside retire_after and retire after it; all streams in one call, then streams named one by one with
    stream 1 left out (its rows stay as they were)."""
    cfg = R.Cfg(retire_after=2, min_samples=8)
    d = Dev(pkg, cfg, 3, 8)
    n_ret = 0
    for f in range(6):
        frames = [CC.noise_frame(37, 70, 10 * f + s) for s in range(3)]
        lists = [CC.churn(f, s) for s in range(3)]
        if f < 4:
            batch(d, lists, frames, [f, 100 + f, 7 * f + 1])
        else:
            before = d.ca.state(1)
            batch(d, lists, frames, [f, 100 + f, 7 * f + 1], named=[2, 0])
            assert tuples(d.ca.state(1)) == tuples(before)
        n_ret += len(d.ca.retired)
    assert n_ret >= 2 and any(len(d.ref[s].rows) >= 4 for s in range(3))
    # the Python reading forms, on what the restatement holds
    ref = d.ref[0]
    t = next(iter(ref.rows))
    want = [R.label(ref.rows[t].hist, p) for p in range(3)]
    got = d.ca.attributes(t, 0)
    assert [(R.NAMES.index(g.name) if g.name else -1, g.share_pm, R.NAMES.index(g.second) if g.second else -1, g.second_pm, g.samples) for g in got] == want
    up, lo = ref.label(t)
    assert d.ca.label(t, 0) == f"{up or '-'} / {lo or '-'}"
    for part in range(3):
        for name in range(12):
            want = [(s, t) for s in range(3) for t in sorted(d.ref[s].rows) if (lambda l: l[0] == name and l[1] >= 300)(R.label(d.ref[s].rows[t].hist, part))]
            assert d.ca.find(("upper", "lower", "whole")[part], R.NAMES[name], 300) == want
    d.close()


def test_three_hundred_tracks_in_one_stream(pkg):
    """More members than the workgroup has threads, ids not ascending, half of them absent in the second call, all of them retired by the
    third."""
    cfg = R.Cfg(min_samples=0, retire_after=1)
    d = Dev(pkg, cfg, 1, 300)
    fr = Frame(pkg, 37, 70, 211, 6, True)
    rng = np.random.default_rng(6)
    ids = rng.permutation(1000)[:300] + 5
    x0, y0 = rng.integers(-1, 69, 300), rng.integers(-1, 36, 300)
    boxes = np.stack([x0, y0, x0 + 1, y0 + 1], 1).astype(np.float32)    # 2 x 2 boxes
    code, u, r = d.process(0, ids, boxes, np.zeros(300, np.int32), fr, 0)
    assert len(u) == 300 and len(d.ref[0].rows) == 300
    d.process(0, ids[::2], boxes[::2], np.zeros(150, np.int32), fr, 1)
    code, u, r = d.process(0, ids[:3], boxes[:3], np.zeros(3, np.int32), fr, 3)
    assert len(r) >= 297 and len(u) == 3
    d.close(); fr.free()


def test_ledger_overflow_is_sticky_until_reset(pkg):
    cfg = R.Cfg(min_samples=1, retire_after=100)
    d = Dev(pkg, cfg, 2, 4)
    fr = Frame(pkg, 37, 70, 211, 7, False)
    box = lambda q: (3 + 5 * q, 2, 20 + 5 * q, 30)
    d.process(0, [1, 2, 3, 4], [box(q) for q in range(4)], [0] * 4, fr, 0)
    d.process(0, [5, 6, 7, 8], [box(q) for q in range(4)], [0] * 4, fr, 1)               # 8 rows: full
    code, u, r = d.process(0, [9, 2], [box(0), box(1)], [0, 0], fr, 2)                    # 7 idle + 2 members > 8
    assert code == R_E_CAPACITY(pkg) and [x[0] for x in d.ref[0].state()] == [2, 9]
    code, _, _ = d.process(0, [9], [box(0)], [0], fr, 3)
    assert code == R_E_CAPACITY(pkg)                                                      # sticky
    d.process(1, [1], [box(0)], [0], fr, 0)                                               # the other stream works
    d.ca.reset(0)
    d.ref[0] = R.Stream(cfg, 4)
    code, u, r = d.process(0, [9], [box(0)], [0], fr, 0)                                  # the frame ids start over, too
    assert code == 0 and u[0][6] & R.F_NEW
    # refusals leave the state alone
    L, F = d.L, d.F
    one = (F.ptr(np.int64([1])), F.ptr(np.float32([0, 0, 5, 5])), F.ptr(np.int32([0])))
    assert L.rtmodt_colour_process(d.ca._h, 0, *one, 1, C.c_void_p(fr.ptr), fr.h, fr.w, fr.stride, fr.mem, 0, None) == F.E_INVALID       # frame id not later
    assert L.rtmodt_colour_process(d.ca._h, 0, *one, 1, C.c_void_p(fr.ptr), fr.h, fr.w, 3 * fr.w - 1, fr.mem, 5, None) == F.E_INVALID
    assert L.rtmodt_colour_process(d.ca._h, 2, *one, 1, C.c_void_p(fr.ptr), fr.h, fr.w, fr.stride, fr.mem, 5, None) == F.E_INVALID
    assert L.rtmodt_colour_process(d.ca._h, 0, *one, 5, C.c_void_p(fr.ptr), fr.h, fr.w, fr.stride, fr.mem, 5, None) == F.E_CAPACITY
    two = (F.ptr(np.int64([1, 1])), F.ptr(np.float32([0, 0, 5, 5] * 2)), F.ptr(np.int32([0, 0])))
    assert L.rtmodt_colour_process(d.ca._h, 0, *two, 2, C.c_void_p(fr.ptr), fr.h, fr.w, fr.stride, fr.mem, 5, None) == F.E_INVALID and b"twice" in L.rtmodt_last_error()
    d.same(0); d.same(1)
    d.close()


def R_E_CAPACITY(pkg):
    return pkg._ffi.E_CAPACITY


def test_state_round_trip_and_reset(pkg):
    cfg = R.Cfg(retire_after=2, min_samples=8)
    a, b = Dev(pkg, cfg, 1, 8), Dev(pkg, cfg, 2, 8)
    frames = [CC.noise_frame(37, 70, 40 + f) for f in range(6)]
    for f in range(3):
        ids, xy, cl = CC.churn(f, 0)
        a.ca.process((ids, xy, cl), frames[f], f)
    st = a.ca.state()
    assert len(st) >= 4
    b.ca.load_state(st, stream=1)
    assert tuples(b.ca.state(1)) == tuples(st) and len(b.ca.state(0)) == 0
    with pytest.raises(pkg._ffi.RtmodtError):                           # the loaded rows carry the stream's last frame id
        b.ca.process(CC.churn(3, 0), frames[3], 2, stream=1)
    for f in range(3, 6):
        ids, xy, cl = CC.churn(f, 0)
        ua, ra = a.ca.process((ids, xy, cl), frames[f], f)
        ub, rb = b.ca.process((ids, xy, cl), frames[f], f, stream=1)
        assert tuples(ua) == tuples(ub) and tuples(ra) == tuples(rb) and tuples(a.ca.state()) == tuples(b.ca.state(1)), f
    bad = st.copy()
    bad["track_id"][1] = bad["track_id"][0]
    with pytest.raises(pkg._ffi.RtmodtError):
        b.ca.load_state(bad, stream=0)
    assert len(b.ca.state(0)) == 0
    b.ca.reset()
    assert len(b.ca.state(1)) == 0
    b.ca.load_state(st[:0], stream=1)
    assert b.ca.last_kernel_ms() >= 0
    a.close(); b.close()


@pytest.mark.parametrize("which", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_tracker_forms_equal_the_list_form_on_the_passed_tracks(pkg, which):
    make, with_frames, passed = _trackers(pkg)[which]
    core = make()
    frames = run_scripted(core, with_frames)
    cfg = R.Cfg(min_samples=4, retire_after=0, classes=(0, 1))
    d = Dev(pkg, cfg, S, 32)
    lists = Dev(pkg, cfg, S, 32)
    n_pass = 0
    for call in range(2):
        if call == 1:                                                   # one more update: the frame-2-only track is lost, boxes move on
            xyxy = np.zeros((S, 16, 4), np.float32); conf = np.zeros((S, 16), np.float32); cls = np.zeros((S, 16), np.int32); cnt = np.zeros(S, np.int32)
            for s in range(S):
                xy, cf, cl = scripted(3, s)
                xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf * np.float32(0.9 + 0.02 * s), cl, len(cf)
            core.update_batch(xyxy, conf, cls, cnt, **({"frames": frames} if with_frames else {}))
        fid = [call, 10 + call]
        d.ca.process_tracker(core, frames, fid)
        for s in range(S):
            st = core.snapshot(s)
            sel = np.zeros(len(st["ids"]), bool)
            sel[passed(core, st)] = True
            n_pass += int(sel.sum())
            code, u, r = d.ref[s].process(st["ids"].tolist(), st["xyxy"], st["cls"].tolist(), frames[s], fid[s], sel, list_order="given")
            assert code == 0 and tuples(d.ca.updated[d.ca.updated_stream == s]) == u and tuples(d.ca.retired[d.ca.retired_stream == s]) == r, (call, s)
            d.same(s)
            # the host-list form fed with the same selected tracks: `track` counts the selected entries only
            keep = np.nonzero(sel)[0]
            ul, rl = lists.ca.process((st["ids"][keep], st["xyxy"][keep], st["cls"][keep]), frames[s], fid[s], stream=s)
            strip = lambda rows: [x[:7] + x[8:] for x in rows]
            assert strip(tuples(ul)) == strip(u) and tuples(rl) == r and tuples(lists.ca.state(s)) == tuples(d.ca.state(s))
    assert n_pass > 0 and any(len(d.ref[s].rows) for s in range(S))
    small = pkg.ColourAttributes(n_streams=1, max_tracks=4)
    with pytest.raises(ValueError, match="ColourAttributes"):
        small.process_tracker(core, frames, 0)
    small.close(); d.close(); lists.close(); core.close()


# ---- the pipeline's colours stage ---------------------------------------------------------------------------------------------------
class _Det:
    model = type("M", (), {"names": {0: "person"}})()

    def detect(self, frame):
        return type("D", (), {"xyxy": np.zeros((1, 4), np.float32), "confidence": np.ones(1, np.float32), "class_id": np.zeros(1, np.int32),
                              "__len__": lambda self: 1})()


def _script(f):
    tr = [SimpleNamespace(track_id=4, xyxy=np.float32([2 + f, 4, 30 + 2 * f, 44]), confidence=0.5, class_name="person", class_id=0, trail=[])]
    if f < 2:
        tr.append(SimpleNamespace(track_id=9, xyxy=np.float32([30, 5, 60, 45]), confidence=0.7, class_name="person", class_id=0, trail=[]))
    return tr


class _Trk:
    def __init__(self):
        self.f = -1

    def update(self, detections):
        self.f += 1
        return _script(self.f)


def test_pipeline_colours_stage(pkg):
    rng = np.random.default_rng(9)
    frames = np.stack([CC.textured(48, 64, rng) for _ in range(2)])
    for fr in frames:
        CC.paint_person(fr, (2, 4, 40, 44), "red", "blue", rng)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    run = lambda **kw: pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof(), max_frames=6, device_stages=False, device_handoff=False, **kw)
    base = run()
    again = run(colours=None)
    assert set(again) == set(base) and "colours_retired" not in base
    ca = pkg.ColourAttributes(max_tracks=8, retire_after=1, min_samples=4)
    mask = pkg.visualization.PrivacyMask(mode="fill")
    gal = pkg.visualization.SnapshotGallery((16, 16), max_tracks=8, min_side=4)
    p = prof()
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), p, max_frames=6, device_stages=False, device_handoff=False, colours=ca, privacy=mask,
                           snapshots=gal)
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"colours_mean_ms", "snapshots_mean_ms", "privacy_mean_ms"}
    order = list(p.STAGE_ORDER)
    assert order.index("colours") + 1 == order.index("snapshots") and order.index("snapshots") + 1 == order.index("privacy")
    assert pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events", "visualization", "total"]
    p2 = prof()
    ca2 = pkg.ColourAttributes(max_tracks=8)
    pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), p2, max_frames=2, device_stages=False, device_handoff=False, colours=ca2)
    assert list(p2.STAGE_ORDER).index("colours") + 1 == list(p2.STAGE_ORDER).index("visualization")
    ref = R.Stream(R.Cfg(retire_after=1, min_samples=4), 8)
    n_rt = 0
    src = pkg.pipeline.SyntheticSource(frames)
    for f in range(6):
        ok, frame, fid = src.read()
        tr = _script(f)
        code, u, r = ref.process([t.track_id for t in tr], [t.xyxy for t in tr], [0] * len(tr), frame, fid)
        n_rt += len(r)
    assert out["colours_retired"] == n_rt == 1
    assert tuples(ca.state()) == ref.state() and ca.label(4) == "red / blue"       # the clean pixels: the stage runs before privacy
    mask.close(); gal.close(); ca.close(); ca2.close()
