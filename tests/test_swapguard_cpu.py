"""CPU: the restatement of the ID-swap guard (tests/swapguard_ref.py) against cases worked by hand, the scenes of the GPU suite with
their expected outcomes, the C ABI's declarations, and pipeline.run's hand-over.  The design document's B.4 / G.1 "appearance
verification"; PARITY UNPINNED (there is no reference implementation)."""
import ctypes
import math
import re

import numpy as np
import pytest

import swapguard_ref as R
from deepsort_ref import describe

ENTRY_POINTS = ["rtmodt_swapguard_create", "rtmodt_swapguard_destroy", "rtmodt_swapguard_process", "rtmodt_swapguard_process_tracker",
                "rtmodt_swapguard_state", "rtmodt_swapguard_counts", "rtmodt_swapguard_last_ms"]


def test_similarity_on_toy_vectors():
    """(1000 * dot) // max(1, isqrt(n2(q) * n2(ref))), worked by hand on 4-bin vectors."""
    assert R.similarity([1, 0, 0, 0], [3, 0, 0, 0]) == 1000                   # 3000 // isqrt(1 * 9)
    assert R.similarity([3, 4, 0, 0], [4, 3, 0, 0]) == 960                    # 24000 // isqrt(25 * 25)
    assert R.similarity([3, 4, 0, 0], [0, 0, 5, 0]) == 0
    assert R.similarity([1, 2, 2, 0], [6, 3, 6, 0]) == 888                    # dot 24, isqrt(9 * 81) = 27, 24000 // 27
    assert R.similarity([2, 1, 0, 0], [1, 2, 0, 0]) == 800                    # 4000 // isqrt(25)
    assert R.similarity([1, 1, 0, 0], [1, 0, 0, 0]) == 1000                   # isqrt(2) = 1: the floor of the root, not the root
    assert R.similarity([0, 0, 0, 0], [1, 2, 3, 4]) == 0                      # a zero norm divides by 1
    assert R.similarity([127] * 4, [8 * 127] * 4) == 1000                     # the largest bins a ring of 8 can hold


def test_the_products_fit_their_integers():
    """history <= 8: a ring's norm fits 31 bits and the product of the two norms 63 (what csrc/swapguard.hip asserts statically)."""
    n2q, n2r = 192 * 127 * 127, 192 * (8 * 127) ** 2
    assert n2r < 2 ** 31 and 192 * 127 * 8 * 127 < 2 ** 31 and n2q * n2r < 2 ** 63


def test_partner_rules():
    """The largest IoU wins, ties go to the lowest index, a NaN is never the largest, contact is strict."""
    nan = float("nan")
    boxes = [[0, 0, 10, 10], [5, 0, 15, 10], [-5, 0, 5, 10], [100, 0, 110, 10], [nan, 0, 10, 10], [10, 0, 20, 10]]
    pc = R.partners(boxes, 0.0)
    assert pc[0] == (1, True)                                                 # boxes 1 and 2 overlap box 0 equally: the lower index
    assert pc[1] == (0, True) and pc[2] == (0, True)                          # box 5 overlaps box 1 by as much as box 0 does: the lower index
    assert pc[3] == (0, False)                                                # touches nothing: IoU 0 with everyone, partner 0, no contact
    assert pc[4] == (-1, False)                                               # every IoU is NaN
    assert pc[5] == (1, True)
    assert R.partners(boxes[:1], 0.0) == [(-1, False)]
    third = float(np.float32(50) / (np.float32(150) + np.float32(1e-6)))
    assert R.partners(boxes[:2], third)[0] == (1, False) and R.partners(boxes[:2], np.nextafter(np.float32(third), np.float32(0)))[0] == (1, True)


@pytest.mark.parametrize("assign", ["greedy", "lapjv"])
def test_s1_tracker_swaps_and_the_guard_reverts_once(assign):
    """S1 through TrackerOracle(0.5, 30, 0.8): without the guard the two ids are exchanged from frame 13 to the end; with it there is
    exactly one event, at frame 22 (the first contact-free frame), and the ids are right from there on."""
    A, B = R.COL_A, R.COL_B
    seen, events = R.run_tracker_s1(assign, None)
    assert events == [] and all(seen[f] == {A: 1, B: 2} for f in range(12))
    assert all(seen[f] == {A: 2, B: 1} for f in range(13, 40))
    guard = R.SwapGuardRef()
    seen, events = R.run_tracker_s1(assign, guard)
    assert events == [dict(frame_id=22, track_a=0, track_b=1, id_a=1, id_b=2, sims=[0, 1000, 0, 1000])]
    assert all(seen[f] == {A: 2, B: 1} for f in range(13, 22)) and all(seen[f] == {A: 1, B: 2} for f in range(22, 40))
    assert guard.n_reverted == 1 and not guard.ledger_overflow
    rows = guard.snapshot()
    assert [r[:5] for r in rows][:2] == [[1, 39, 5, 21, -1], [2, 39, 5, 21, -1]]      # (greedy spawns a short-lived id 3 at frame 12, where the boxes coincide)


def test_s2_chain_is_not_mutual():
    ref, events, idmap = R.play_ref(R.scene_s2())
    assert events == [] and idmap == {"a": 2, "b": 1, "c": 3} and ref.refused > 0
    assert [r[:5] for r in ref.snapshot()] == [[1, 15, 5, 9, 3], [2, 15, 5, 9, 1], [3, 15, 5, 9, 1]]


def test_s3_twins_are_blocked_by_the_gain():
    ref, events, idmap = R.play_ref(R.scene_s3())
    assert events == [] and idmap == {"a": 2, "b": 1} and ref.refused == 18              # frames 22 .. 39
    ref0, events0, _ = R.play_ref(R.scene_s3(), min_gain_pm=0)                            # without the gain the twins would flip
    assert len(events0) >= 1 and events0[0]["sims"] == [1000, 1000, 1000, 1000]


def test_s4_blind_tracks():
    """A NaN corner at frame 22: the revert waits one frame; meanwhile B, alone, has pushed its descriptor into row 1 (three of A, one
    of B), so the similarities are 3 / sqrt(10) and 1 / sqrt(10) of 1000.  A box outside the frame for four frames: the window passes."""
    scene = R.scene_s4_nan_corner()
    ref, events, idmap = R.play_ref(scene)
    q = describe(scene["frames"][0]["img"], [scene["frames"][0]["tracks"][0][1]])[0][0].astype(np.int64)
    N = int((q * q).sum())
    den = math.isqrt(N * 10 * N)
    assert events == [dict(frame_id=23, track_a=0, track_b=1, id_a=2, id_b=1, sims=[0, 3000 * N // den, 1000 * N // den, 1000])]
    assert events[0]["sims"][1] == 948 and events[0]["sims"][2] == 316 and idmap == {"a": 1, "b": 2}
    ref, events, idmap = R.play_ref(R.scene_s4_outside())
    assert events == [] and idmap == {"a": 2, "b": 1}


def test_s4_gap_expiry():
    """max_gap_frames = 4: back after 3 absent frames (frame_id - last = 4) the row is kept and its ring fills up; after 4 absent frames
    (5 > 4) it starts again."""
    ref, _, _ = R.play_ref(R.scene_s4_gap(3), max_gap_frames=4)
    assert [r[:5] for r in ref.snapshot()] == [[7, 8, 5, 0, -1]]
    ref, _, _ = R.play_ref(R.scene_s4_gap(4), max_gap_frames=4)
    assert [r[:5] for r in ref.snapshot()] == [[7, 9, 2, 0, -1]]


def test_s4_short_history_and_window():
    ref, events, idmap = R.play_ref(R.scene_s4_short_history(), window=1)
    assert events == [] and idmap == {"a": 2, "b": 1}                                   # count 2 < min_history at frame 22, too late at 23
    ref, events, idmap = R.play_ref(R.scene_s4_window(24))
    assert [(e["frame_id"], e["sims"]) for e in events] == [(24, [0, 1000, 0, 1000])] and idmap == {"a": 1, "b": 2}
    ref, events, idmap = R.play_ref(R.scene_s4_window(25))
    assert events == [] and idmap == {"a": 2, "b": 1} and ref.refused == 15              # 25 - 21 = window + 1


def test_s5_sixteen_pairs_in_one_frame():
    ref, events, idmap = R.play_ref(R.scene_s5(), max_tracks=64)
    assert len(events) == 16 and {e["frame_id"] for e in events} == {19} and all(idmap[k] == k + 1 for k in idmap)
    assert [e["track_a"] for e in events] == sorted(e["track_a"] for e in events)


def test_s6_capacity_sticks():
    ref, events, _ = R.play_ref(R.scene_s6(), max_tracks=4, max_gap_frames=1000)
    assert ref.ledger_overflow and sorted(ref.rows) == list(range(108, 116))        # frame 2 dropped the idle rows, frame 3 fits again
    with pytest.raises(ValueError):
        R.SwapGuardRef().process([1, 1], np.zeros((2, 4)), np.zeros((2, 192), np.int8), 0)


@pytest.mark.parametrize("seed", R.FUZZ_SEEDS)
def test_s7_fuzz_seeds_revert_and_refuse(seed):
    """The condition the GPU fuzz rests on: the restatement alone reverts at least 5 swaps and refuses at least 5 candidates."""
    ref, events, _ = R.play_ref(R.scene_s7(seed), max_tracks=16)
    assert len(events) >= 5 and ref.refused >= 5 and ref.n_reverted == len(events)


def test_header_and_ffi_declare_every_entry_point(pkg):
    ffi = pkg._ffi
    declared = ffi.header_symbols()
    src = open(ffi.__file__).read()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert re.search(rf'"{name}":', src), name
    assert ctypes.sizeof(ffi.SwapGuardCfg) == 48 and ctypes.sizeof(ffi.SwapEventRec) == 48
    header = open(ffi.HEADER_PATH).read()
    block = header[header.index("ID-swap guard"):]
    assert block.count("PARITY UNPINNED") >= 6 and "B.4" in block and "G.1 row 1" in block


class _Det:
    model = type("M", (), {"names": {0: "person"}})()

    def detect(self, frame):
        return type("D", (), {"xyxy": np.zeros((1, 4), np.float32), "confidence": np.ones(1, np.float32), "class_id": np.zeros(1, np.int32),
                              "__len__": lambda self: 1})()


class _Trk:
    def __init__(self, log):
        self.log = log

    def update_from_detector(self, det, materialize=True):
        self.log.append("track")
        return [type("T", (), {"track_id": 1})(), type("T", (), {"track_id": 2})()] if materialize else []


class _Events:
    def __init__(self, log):
        self.log, self.ids = log, []

    def process(self, tracks, fid):
        self.log.append("events")
        self.ids.append([t.track_id for t in tracks])
        return []


class _Guard:
    def __init__(self, log, pkg):
        self.log, self.pkg = log, pkg

    def process_tracker(self, tracker, frames, fid):
        self.log.append("guard")
        assert len(frames) == 1 and frames[0].shape == (8, 8, 3)
        ev = self.pkg.tracking.swapguard.SwapEvent(fid, 0, 1, 1, 2, (0, 1000, 0, 1000))
        return [[ev] if fid == 2 else []]


def _run(pkg, **kw):
    log = []
    ev = _Events(log)
    prof = pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    guard = _Guard(log, pkg) if kw.pop("guard", False) else None
    if guard is not None:
        kw["swap_guard"] = guard
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.zeros((2, 8, 8, 3), np.uint8)), _Det(), _Trk(log), prof, max_frames=3, device_stages=False,
                           event_engine=ev, **kw)
    return out, log, ev


def test_pipeline_without_a_guard_is_unchanged(pkg):
    base, log0, _ = _run(pkg)
    none, log1, _ = _run(pkg, swap_guard=None)
    timing = re.compile(r"_ms$|^fps_")
    assert {k: v for k, v in base.items() if not timing.search(k)} == {k: v for k, v in none.items() if not timing.search(k)}
    assert sorted(base) == sorted(none) and "id_swaps_reverted" not in none and log0 == log1 == ["track", "events"] * 3


def test_pipeline_calls_the_guard_between_tracking_and_events(pkg):
    out, log, ev = _run(pkg, guard=True)
    assert log == ["track", "guard", "events"] * 3 and out["id_swaps_reverted"] == 1
    assert ev.ids == [[1, 2], [2, 1], [1, 2]]                                           # the materialised list adopts the exchange (frame ids 1, 2, 3)
