"""CPU: the left / removed object detector's rules without a GPU.  ``tests/leftobj_ref.py`` (the restatement the kernels of
``csrc/leftobj.hip`` are pinned to) against hand-worked literal cases, its vectorised forms against its loop forms and a flood fill;
the rules of ``csrc/leftobj_rule.h`` against the restatement, through the host-only entry point ``rtmodt_leftobj_cell`` and through
``tests/native/leftobj_rule_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer); the ABI's refusals, which need no device.  PARITY UNPINNED: the reference has no
counterpart."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leftobj_cases as LC  # noqa: E402
import leftobj_ref as LR  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "leftobj_rule_check.cpp")
SMALL = dict(warmup=2, static_frames=3, occlusion=2, threshold=16, stable=10, cand_shift=3, learn_shift=6, warm_shift=2)


def one(yc, cell, seen, **kw):
    c = LR.config(**dict(SMALL, **kw))
    got = LR.cell_loop(yc, cell, seen, c)
    a = [np.int64([[v]]) for v in cell[:4]]
    fg, bg, cand, age, miss = LR.update([[yc]], *a, seen, c)
    assert (int(bg[0, 0]), int(cand[0, 0]), int(age[0, 0]), int(miss[0, 0]), cell[4]) == got[0] and bool(fg[0, 0]) == got[1]
    return got


# ---- hand-worked literal cases: the cell ----------------------------------------------------------------------------------
def test_cell_first_frame_and_warmup():
    assert one(37, (999, 777, 5, 1, 1), 0) == ((37 * 256, 37 * 256, 0, 0, 1), False, False)       # initialises; the flags stay
    assert one(99, (25600, 25600, 0, 0, 0), 1) == ((25600 - 64, 25600, 0, 0, 0), False, False)     # d = -256: -256 >> 2 = -64
    assert one(100, (25601, 0, 0, 0, 0), 1) == ((25600, 0, 0, 0, 0), False, False)                 # -1 >> 2 = -1: floor, not towards zero
    assert one(250, (25600, 25600, 0, 0, 0), 1) == ((25600 + (38400 >> 2), 25600, 0, 0, 0), False, False)     # far off, still warming up: no fg


def test_cell_background_and_the_miss_paths():
    assert one(116, (25600, 25600, 0, 0, 0), 2) == ((25600 + (4096 >> 6), 25600, 0, 0, 0), False, False)       # |d| = 16 << 8 exactly: not fg
    assert one(117, (25600, 25600, 0, 0, 0), 2) == ((25600, 117 * 256, 1, 0, 0), True, False)                  # fg, cand far: a new candidate
    # a background frame on a cell that holds a candidate: miss 0 -> 1 -> 2, and the third takes it above occlusion = 2
    assert one(100, (25600, 51200, 7, 0, 0), 2) == ((25600, 51200, 7, 1, 0), False, True)
    assert one(100, (25600, 51200, 7, 1, 0), 2) == ((25600, 51200, 7, 2, 0), False, True)
    assert one(100, (25600, 51200, 7, 2, 0), 2) == ((25600, 51200, 0, 0, 0), False, False)
    assert one(100, (25600, 51200, 0, 5, 0), 2) == ((25600, 51200, 0, 5, 0), False, False)                     # no candidate: miss is not counted
    # stable foreground: cand moves by e >> 3, age counts, miss clears
    assert one(205, (25600, 51200, 2, 2, 0), 2) == ((25600, 51200 + (1280 >> 3), 3, 0, 0), True, True)         # age reaches static_frames = 3
    assert one(210, (25600, 51200, 2, 0, 0), 2) == ((25600, 51200 + (2560 >> 3), 3, 0, 0), True, True)         # |e| = 10 << 8 exactly: stable
    assert one(195, (25600, 51200, 2, 0, 0), 2) == ((25600, 51200 + (-1280 >> 3), 3, 0, 0), True, True)
    # someone walks in front (fg, not stable): miss 0 -> 1 -> 2 with cand and age kept, then the candidate is replaced
    assert one(30, (25600, 51200, 9, 0, 0), 2) == ((25600, 51200, 9, 1, 0), True, True)
    assert one(30, (25600, 51200, 9, 1, 0), 2) == ((25600, 51200, 9, 2, 0), True, True)
    assert one(30, (25600, 51200, 9, 2, 0), 2) == ((25600, 30 * 256, 1, 0, 0), True, False)
    assert one(211, (25600, 51200, 0, 0, 0), 2) == ((25600, 211 * 256, 1, 0, 0), True, False)                  # 11 levels off, no age to keep
    assert one(30, (25600, 51200, 9, 0, 0), 2, occlusion=0) == ((25600, 30 * 256, 1, 0, 0), True, False)       # occlusion 0: no walker is ridden out


def test_cell_saturation_and_ignore():
    assert one(200, (25600, 51200, 65534, 0, 0), 2) == ((25600, 51200, 65535, 0, 0), True, True)
    assert one(200, (25600, 51200, 65535, 0, 0), 2) == ((25600, 51200, 65535, 0, 0), True, True)
    assert one(200, (25600, 51200, 65535, 0, 1), 2) == ((25600, 51200, 65535, 0, 1), True, False)              # ignored: the model runs, never static
    assert one(200, (25600, 51200, 2, 0, 0), 2, static_frames=4)[2] is False


# ---- hand-worked literal cases: kind ----------------------------------------------------------------------------------------
def five(block_in_picture, block_in_model):
    """A 5 x 5 grid, a static 3 x 3 block in the middle: -> (cur, bgc) of its region."""
    dark, bright = 50, 200
    luma = np.full((5, 5), dark, np.int64)
    bg = np.full((5, 5), dark << 8, np.int64)
    cand = np.full((5, 5), dark << 8, np.int64)
    if block_in_picture:
        luma[1:4, 1:4] = bright
        cand[1:4, 1:4] = bright << 8
    if block_in_model:
        bg[1:4, 1:4] = bright << 8
    mask = np.zeros((5, 5), np.uint8)
    mask[1:4, 1:4] = 1
    lab, comps = LR.labels_of(mask)
    assert comps == [(6, 9, 1, 1, 3, 3)]
    got = LR.edge_sums(lab, 6, cand, bg, luma)
    assert got == LR.edge_sums_loop(lab, 6, cand, bg, luma)
    return got


def test_kind_abandoned_removed_unknown():
    # 12 edges leave the block (3 per side; the corners' diagonals do not count), each |200 - 50| = 150
    assert five(True, False) == (1800, 0) and LR.kind_of(1800, 0) == LR.ABANDONED         # the edge is in the picture
    assert five(False, True) == (0, 1800) and LR.kind_of(0, 1800) == LR.REMOVED           # the block sits in bg and is gone from the picture
    assert five(False, False) == (0, 0) and LR.kind_of(0, 0) == LR.UNKNOWN                # flat
    assert five(True, True) == (1800, 1800) and LR.kind_of(7, 7) == LR.UNKNOWN
    # a block at the grid's corner has fewer neighbours inside the grid: 2 + 2 edges
    mask = np.zeros((4, 4), np.uint8)
    mask[:2, :2] = 1
    lab, _ = LR.labels_of(mask)
    z = np.zeros((4, 4), np.int64)
    assert LR.edge_sums(lab, 0, z + (9 << 8), z, z + 1) == LR.edge_sums_loop(lab, 0, z + (9 << 8), z, z + 1) == (4 * 8, 0)


# ---- hand-worked literal cases: tracks, match, timers, ledger ----------------------------------------------------------------
def test_track_box_covered_and_attended_at_their_thresholds():
    assert LR.track_box([1.5, 2.0, 3.25, 4.0]) == (1, 2, 4, 4) and LR.track_box([-0.5, -1.0, 0.5, 0.0]) == (-1, -1, 1, 0)
    assert LR.track_box([3.0, 1.0, 3.0, 2.0]) is None and LR.track_box([np.nan, 0, 1, 1]) is None and LR.track_box([0, 0, np.inf, 1]) is None
    assert LR.track_box([-3e9, 0, 3e9, 1]) == (-2 ** 20, 0, 2 ** 20, 1)
    region = (10, 10, 30, 20)                                         # 200 pixels; covered_pm = 500 asks for 100
    assert LR.covered((10, 10, 20, 20), region, 500) and not LR.covered((10, 10, 19, 20), region, 500)         # 100 | 90
    assert LR.covered((0, 0, 99, 99), region, 1000) and not LR.covered((11, 10, 99, 99), region, 1000)
    assert LR.attended((32, 12, 40, 18), region, 3) and not LR.attended((33, 12, 40, 18), region, 3)           # grown to x0 = 29 | 30
    assert LR.attended((0, 22, 40, 30), region, 3) and not LR.attended((0, 23, 40, 30), region, 3)


def region(cells, kind=LR.ABANDONED, root=0, **kw):
    cx0, cy0, cx1, cy1 = cells
    return dict(dict(box=(cx0 * 4, cy0 * 4, cx1 * 4 + 4, cy1 * 4 + 4), cells=cells, area=(cx1 - cx0 + 1) * (cy1 - cy0 + 1), kind=kind, covered=0,
                     attended=0, _owner=None, oid=0, root=root), **kw)


def entry(oid, cells, **kw):
    return dict(dict(oid=oid, kind=LR.UNKNOWN, area=1, idle=0, unmatched=0, alarmed=0, first_frame=0, owner=-1, cells=cells, box=(0, 0, 1, 1)), **kw)


def test_match_takes_the_most_shared_cells_and_the_lowest_oid_on_a_tie():
    c = LR.config(alarm_frames=99)
    assert LR.shared_cells((0, 0, 3, 3), (3, 3, 5, 5)) == 1 and LR.shared_cells((0, 0, 3, 3), (4, 0, 5, 5)) == 0
    ledger = [entry(3, (0, 0, 3, 3)), entry(5, (4, 0, 7, 3)), entry(9, (20, 20, 21, 21))]
    regs = [region((2, 0, 5, 3)), region((2, 0, 5, 3), root=1), region((30, 30, 31, 31), root=2)]       # 8 cells shared with either: oid 3 wins
    new, nxt, ev, ret, dropped, _ = LR.ledger_step(ledger, 10, regs, 7, c)
    assert [g["oid"] for g in regs] == [3, 5, 10] and nxt == 11 and not ret and dropped == 0
    assert [(e["oid"], e["unmatched"], e["cells"]) for e in new] == [(3, 0, (2, 0, 5, 3)), (5, 0, (2, 0, 5, 3)), (9, 1, (20, 20, 21, 21)), (10, 0, (30, 30, 31, 31))]
    regs = [region((3, 0, 5, 3))]                                     # 4 cells of oid 3, 8 of oid 5
    LR.ledger_step(ledger, 10, regs, 7, c)
    assert regs[0]["oid"] == 5


def test_timers_owner_return_capacity_cleared_absorbed():
    c = LR.config(alarm_frames=3, miss_frames=2, absorb_frames=10, max_objects=2)
    led, nxt, log = [], 1, []
    script = [0, 0, 1, 0, 0, 0, 0]                                    # attended on call 2: idle 1, 2, 0, 1, 2, 3 -> the alarm on call 5
    for f, att in enumerate(script):
        g = region((1, 1, 2, 2), attended=att, _owner=44 if att else None)
        led, nxt, ev, ret, dropped, _ = LR.ledger_step(led, nxt, [g], f, c)
        log.append((led[0]["idle"], led[0]["alarmed"], [e["owner"] for e in ev]))
    assert log == [(1, 0, []), (2, 0, []), (0, 0, []), (1, 0, []), (2, 0, []), (3, 1, [44]), (4, 1, [])]
    # covered by no report class: the timer holds; by a report class: it runs and the kind says so
    e = entry(1, (1, 1, 2, 2), idle=2)
    assert not LR.timer(e, region((1, 1, 2, 2), covered=1), c) and e["idle"] == 2
    assert LR.timer(e, region((1, 1, 2, 2), covered=3), c) and (e["idle"], e["kind"], e["alarmed"]) == (3, LR.TRACKED_STATIC, 1)
    assert not LR.timer(e, region((1, 1, 2, 2), kind=LR.REMOVED), c) and e["kind"] == LR.TRACKED_STATIC        # frozen after the alarm
    # capacity: two rows, three regions -> the third birth is dropped and takes no oid
    regs = [region((0, 0, 1, 1)), region((5, 5, 6, 6), root=1), region((9, 9, 10, 10), root=2)]
    led, nxt, ev, ret, dropped, _ = LR.ledger_step([], 1, regs, 0, c)
    assert [e["oid"] for e in led] == [1, 2] and nxt == 3 and dropped == 1 and regs[2]["oid"] == 0
    # CLEARED after exactly miss_frames + 1 = 3 unmatched calls
    hist = []
    for f in range(1, 4):
        led, nxt, ev, ret, dropped, _ = LR.ledger_step(led, nxt, [], f, c)
        hist.append((len(led), ret))
    assert hist == [(2, []), (2, []), (0, [(1, LR.CLEARED, 0), (2, LR.CLEARED, 0)])]
    # ABSORBED when frame_id - first_frame reaches absorb_frames, on a matched call; the root is handed on
    led = [entry(7, (1, 1, 2, 2), first_frame=5, alarmed=1)]
    led, nxt, ev, ret, dropped, ab = LR.ledger_step(led, 8, [region((1, 1, 2, 2), root=33)], 14, c)
    assert len(led) == 1 and not ret and not ab
    led, nxt, ev, ret, dropped, ab = LR.ledger_step(led, 8, [region((1, 1, 2, 2), root=33)], 15, c)
    assert led == [] and ret == [(7, LR.ABSORBED, 1)] and ab == [33]


def test_absorbed_then_removed_and_reset_on_a_scene_change():
    """A 3 x 3 block on a 9 x 12 grid: static, alarmed ABANDONED, absorbed; taken away it alarms REMOVED; a flood of light resets."""
    kw = dict(scale=1, warmup=1, static_frames=2, alarm_frames=3, absorb_frames=6, occlusion=0, miss_frames=1, min_neighbors=4, min_area=4)
    ref = LR.Ref(1, 9, 12, **kw)
    flat = np.full((9, 12), 60, np.uint8)
    lit = flat.copy()
    lit[3:6, 4:7] = 200
    out = [ref.step(0, LC.cells_to_frame(c_, 1, 9, 12)) for c_ in [flat] + [lit] * 9 + [flat] * 5 + [flat + 100]]
    ev = [(f, e["oid"], e["kind"], e["box"], e["first_frame"]) for f, o in enumerate(out) for e in o["events"]]
    ret = [(f,) + r for f, o in enumerate(out) for r in o["retired"]]
    # fg on 1, static and born on 2 (idle 1), alarm on 4, absorbed on 8 = 2 + 6; the hole: fg on 10, born on 11, alarm on 13
    assert ev == [(4, 1, LR.ABANDONED, (4, 3, 7, 6), 2), (13, 2, LR.REMOVED, (4, 3, 7, 6), 11)]
    assert ret == [(8, 1, LR.ABSORBED, 1), (15, 2, LR.RESET, 1)]
    assert [o["status"] for o in out] == [LR.WARMUP, LR.CLEAR] + [LR.STATIC] * 7 + [LR.CLEAR] * 2 + [LR.STATIC] * 4 + [LR.SCENE_CHANGE]
    assert out[9]["n_fg"] == 0 and (ref.bg[0][3:6, 4:7] >> 8 == 200).all()            # absorbed: the block is background now
    assert out[15]["n_fg"] == 108 and ref.seen[0] == 0 and ref.ledgers[0] == [] and ref.next_oid[0] == 3


# ---- labelling against a flood fill, the vectorised cell against the loop --------------------------------------------------
def test_labelling_and_update_equal_their_loop_forms_on_random_scenes():
    rng = np.random.default_rng(3031)
    for i in range(20):
        gh, gw = [(9, 12), (17, 31), (5, 5), (24, 40)][i % 4]
        mask = (rng.random((gh, gw)) < [0.2, 0.45, 0.7][i % 3]).astype(np.uint8)
        lab, comps = LR.labels_of(mask)
        assert comps == MR.components_flood(mask)
        for first, area, cx0, cy0, cx1, cy1 in comps:
            ys, xs = np.nonzero(lab == first)
            assert (len(ys), xs.min(), ys.min(), xs.max(), ys.max(), ys[0] * gw + xs[0]) == (area, cx0, cy0, cx1, cy1, first)
        assert ((lab >= 0) == (mask != 0)).all()
        z = rng.integers(0, 65281, (3, gh, gw))
        for first, *_ in comps[:3]:
            assert LR.edge_sums(lab, first, z[0], z[1], z[2] >> 8) == LR.edge_sums_loop(lab, first, z[0], z[1], z[2] >> 8)
        st = (rng.random((gh, gw)) < 0.5)
        for mn in (1, 4, 9):
            assert LR.mask_of(st, mn).tolist() == MR.mask_loop(st, mn, 0).tolist()
    for case in cell_cases()[:1500]:
        rule, yc, seen, cell = case
        one(yc, cell, seen, **dict(zip(LR.RULE_FIELDS, rule)))


# ---- the per-cell rule of the library ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_cases():
    """((the eight rule fields), yc, frames_seen, (bg, cand, age, miss, flags))"""
    rng = np.random.default_rng(3032)
    out = []
    for i in range(4000):
        warm = int(rng.choice([1, 2, 8, 255]))
        occ = int(rng.choice([0, 1, 2, 50, 254]))
        stat = int(rng.choice([1, 3, 100, 65535]))
        rule = (warm, int(rng.integers(1, 9)), int(rng.integers(1, 13)), int(rng.choice([1, 16, 255, int(rng.integers(1, 256))])),
                int(rng.choice([1, 10, 255, int(rng.integers(1, 256))])), int(rng.integers(1, 9)), occ, stat)
        seen = int(rng.choice([0, 1, warm - 1, warm, warm + 1, 2 ** 30]))
        yc = int(rng.choice([0, 255, int(rng.integers(0, 256))]))
        near = lambda: int(np.clip(yc * 256 + rng.integers(-5000, 5001), 0, 65280))          # noqa: E731
        bg = int(rng.choice([0, 65280, yc * 256, near(), int(rng.integers(0, 65281))]))
        cand = int(rng.choice([0, 65280, yc * 256, near(), int(rng.integers(0, 65281))]))
        age = int(rng.choice([0, 0, 1, stat - 1, stat, 65534, 65535]))
        miss = int(rng.choice([0, 0, max(occ - 1, 0), occ, min(occ + 1, 255), 255]))
        out.append((rule, yc, seen, (bg, cand, age, miss, int(rng.choice([0, 0, 1, 254])))))
    return out


def ref_cell(case):
    rule, yc, seen, cell = case
    c, fg, st = LR.cell_loop(yc, cell, seen, LR.config(**dict(zip(LR.RULE_FIELDS, rule))))
    return (int(fg), int(st)) + c


def test_leftobj_cell_entry_point_equals_restatement(pkg):
    LO = pkg.detection.left_objects
    n_fg = n_static = 0
    for case in cell_cases():
        rule, yc, seen, cell = case
        c, fg, st = LO.leftobj_cell(yc, seen, cell, **dict(zip(LR.RULE_FIELDS, rule)))
        assert (int(fg), int(st)) + c == ref_cell(case), case
        n_fg += fg; n_static += st
    assert 400 < n_fg < 3600 and 200 < n_static < 3800, (n_fg, n_static)        # both outcomes are well covered
    for bad in (dict(warmup=0), dict(warmup=256), dict(warm_shift=0), dict(warm_shift=9), dict(learn_shift=0), dict(learn_shift=13), dict(threshold=0),
                dict(threshold=256), dict(stable=0), dict(stable=256), dict(cand_shift=0), dict(cand_shift=9), dict(occlusion=-1), dict(occlusion=255),
                dict(static_frames=0), dict(static_frames=65536)):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            LO.leftobj_cell(10, 1, (0, 0, 0, 0, 0), **bad)
        assert e.value.code == pkg._ffi.E_INVALID, bad
    with pytest.raises(pkg._ffi.RtmodtError):
        LO.leftobj_cell(256, 1, (0, 0, 0, 0, 0))
    assert LO.unpack_cell(LO.pack_cell(65280, 1, 65535, 255, 129)) == (65280, 1, 65535, 255, 129)


def test_leftobj_cfg_defaults_refusals_and_exports(pkg):
    import ctypes as C
    LO = pkg.detection.left_objects
    L = pkg._ffi.lib()
    cfg = LO.make_cfg()
    got = {f: getattr(cfg, f) for f in LO.CFG_FIELDS}
    assert got == LR.DEFAULTS and (cfg.streams, cfg.height, cfg.width, cfg.device) == (1, 0, 0, 0)
    assert (cfg.n_owner_classes, cfg.owner_classes[0], cfg.n_report_classes) == (1, 0, 0)
    ok = dict(streams=2, height=37, width=70)
    # a parameter outside its range is refused before the device is touched (this machine has none); the defaults lack a frame size
    for kw in (dict(), dict(ok, streams=0), dict(ok, streams=1025), dict(ok, height=0), dict(ok, width=32769), dict(ok, scale=0), dict(ok, scale=3),
               dict(ok, scale=16), dict(ok, warmup=0), dict(ok, warm_shift=9), dict(ok, learn_shift=13), dict(ok, threshold=0), dict(ok, stable=256),
               dict(ok, cand_shift=0), dict(ok, occlusion=255), dict(ok, static_frames=0), dict(ok, min_neighbors=0), dict(ok, min_neighbors=10),
               dict(ok, min_area=0), dict(ok, min_area=5, max_area=4), dict(ok, max_regions=0), dict(ok, max_regions=257), dict(ok, scene_pm=0),
               dict(ok, scene_pm=1001), dict(ok, max_objects=0), dict(ok, max_objects=257), dict(ok, miss_frames=-1), dict(ok, miss_frames=65536),
               dict(ok, alarm_frames=0), dict(ok, absorb_frames=-1), dict(ok, covered_pm=0), dict(ok, covered_pm=1001), dict(ok, attend_margin=-1),
               dict(ok, attend_margin=32769), dict(ok, max_tracks=0), dict(ok, max_tracks=4097)):
        h = C.c_void_p()
        bad = LO.make_cfg(**kw)
        assert L.rtmodt_leftobj_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw
    bad = LO.make_cfg(**ok)
    bad.n_owner_classes = 9
    h = C.c_void_p()
    assert L.rtmodt_leftobj_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value
    big = LO.make_cfg(streams=1, height=8192, width=8192, scale=1)              # 2^26 cells
    assert L.rtmodt_leftobj_create(C.byref(big), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value and b"cells" in L.rtmodt_last_error()
    many = LO.make_cfg(streams=1024, height=4096, width=4096, scale=4)          # 2^20 cells x 1024 streams
    assert L.rtmodt_leftobj_create(C.byref(many), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value
    assert L.rtmodt_leftobj_process(None, None, None, None, 0, 1, 1, 3, 0, None, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_leftobj_reset(None, 0) == pkg._ffi.E_INVALID and L.rtmodt_leftobj_read_mask(None, 0, None) == pkg._ffi.E_INVALID
    with pytest.raises(TypeError):
        LO.make_cfg(dilate=1)
    with pytest.raises(ValueError):
        LO.make_cfg(owner_classes=range(9))
    assert pkg.LeftObjectDetector is LO.LeftObjectDetector and "LeftObjectDetector" in pkg.detection.__all__ and "LeftObjectDetector" in pkg.__all__
    declared = [s for s in pkg._ffi.header_symbols() if s.startswith("rtmodt_leftobj_")]
    assert len(declared) == 15 and all(hasattr(L, s) and s in L._signatures for s in declared)


def test_polygons_rasterise_at_cell_centres(pkg):
    LO = pkg.detection.left_objects
    tri = LO.rasterise_polygons((4, 4), 4, [[(0, 0), (16, 0), (0, 16)]])      # centres (4k + 2, 4j + 2) with x + y < 16
    assert tri.tolist() == [[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    assert LO.rasterise_polygons((4, 4), 4, [[(0, 0), (16, 0), (0, 16)]], invert=True).tolist() == (1 - tri).tolist()
    two = LO.rasterise_polygons((2, 6), 2, [[(0, 0), (4, 0), (4, 4), (0, 4)], [(8, 0), (12, 0), (12, 2), (8, 2)]])
    assert two.tolist() == [[1, 1, 0, 0, 1, 1], [1, 1, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        LO.rasterise_polygons((2, 2), 4, [[(0, 0), (1, 1)]])


# ---- the header through a stand-alone program, plain and sanitized -------------------------------------------------------
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("leftobj_rule_check_san" if sanitize else "leftobj_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built leftobj_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_leftobj_rule_header_equals_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    rng = np.random.default_rng(3033)
    lines, want = [], []
    for case in cell_cases():
        rule, yc, seen, cell = case
        lines.append("c " + " ".join(str(v) for v in rule + (yc, seen) + cell))
        want.append(" ".join(str(v) for v in ref_cell(case)))
    boxes = [(1.5, 2.0, 3.25, 4.0), (-0.5, -1.0, 0.5, 0.0), (3.0, 1.0, 3.0, 2.0), (-3e9, 0.0, 3e9, 1.0), (10.0, 10.0, 20.0, 20.0), (10.0, 10.0, 19.0, 20.0),
             (32.0, 12.0, 40.0, 18.0), (33.0, 12.0, 40.0, 18.0), (9.99, 9.01, 30.01, 20.5), (1048576.5, 0.0, 1048580.0, 4.0)]
    boxes += [tuple(float(np.float32(v)) for v in rng.uniform(-20, 60, 4)) for _ in range(300)]
    for b in boxes:
        pm, margin = int(rng.choice([1, 500, 1000])), int(rng.choice([0, 3, 32]))
        lines.append("t " + " ".join(repr(v) for v in b) + f" 10 10 30 20 {pm} {margin}")
        tb = LR.track_box(b)
        want.append("skip" if tb is None else " ".join(str(v) for v in tb + (int(LR.covered(tb, (10, 10, 30, 20), pm)), int(LR.attended(tb, (10, 10, 30, 20), margin)))))
    for _ in range(200):
        a, b = (tuple(int(v) for v in (x0, y0, x0 + dx, y0 + dy)) for x0, y0, dx, dy in rng.integers(0, 12, (2, 4)))
        lines.append("m " + " ".join(str(v) for v in a + b))
        want.append(str(LR.shared_cells(a, b)))
    for cur, bgc in ((0, 0), (1, 0), (0, 1), (2 ** 40, 2 ** 40), (2 ** 40 + 1, 2 ** 40), (5, 2 ** 34)):
        lines.append(f"k {cur} {bgc}")
        want.append(str(LR.kind_of(cur, bgc)))
    for seen, warm, n_fg, pm, cells, total in ((0, 8, 0, 600, 100, 0), (7, 8, 100, 600, 100, 3), (8, 8, 60, 600, 100, 0), (8, 8, 59, 600, 100, 0),
                                               (8, 8, 59, 600, 100, 2), (2 ** 30, 1, 0, 1, 2 ** 24, 0), (2 ** 30, 255, 2 ** 24, 1000, 2 ** 24, 9)):
        lines.append(f"s {seen} {warm} {n_fg} {pm} {cells} {total}")
        st = LR.status_of(seen, n_fg, cells, total, LR.config(warmup=warm, scene_pm=pm))
        want.append(f"{st} {LR.next_seen(seen, st)}")
    for _ in range(300):
        idle, kind, alarmed = int(rng.choice([0, 1, 2, 7, 2 ** 30])), int(rng.integers(0, 4)), int(rng.integers(0, 2))
        owner, rk, att, oid = int(rng.choice([-1, 5])), int(rng.integers(0, 3)), int(rng.integers(0, 2)), int(rng.integers(1, 99))
        cov = int(rng.choice([0, 1, 3]))
        alarm, fid, first, absorb = int(rng.choice([1, 3, 8])), int(rng.integers(0, 50)), int(rng.integers(0, 50)), int(rng.choice([0, 1, 10]))
        lines.append(f"e {idle} {kind} {alarmed} {owner} {rk} {att} {oid} {cov & 1} {cov >> 1} {alarm} {fid} {first} {absorb}")
        e = dict(idle=idle, kind=kind, alarmed=alarmed, owner=owner)
        fired = LR.timer(e, dict(attended=att, _owner=oid, covered=cov, kind=rk), LR.config(alarm_frames=alarm))
        want.append(f"{int(fired)} {e['idle']} {e['kind']} {e['alarmed']} {e['owner']} {int(absorb > 0 and fid - first >= absorb)}")
    extra = ["c 0 2 6 16 10 3 2 3 10 1 0 0 0 0 0", "c 2 2 6 16 10 3 255 3 10 1 0 0 0 0 0", "c 2 2 6 16 10 3 2 3 256 1 0 0 0 0 0",
             "c 2 2 6 16 10 3 2 3 10 1 65536 0 0 0 0", "c 2 2 6 16 10 3 2 3 10 1 0 0 0 256 0"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(want) + len(extra) + 1 and got[-1] == f"done {len(want) + len(extra)}"
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, (lines[i], g[:200], w_[:200])
    assert got[len(want):-1] == ["bad"] * len(extra)
