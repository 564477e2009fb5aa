"""CPU: the camera-health monitor's rules without a GPU.  ``tests/health_ref.py`` (the restatement the kernels of ``csrc/health.hip``
are pinned to) against hand-worked literal cases and its vectorised forms against its loop forms; the rules of ``csrc/health_rule.h``
against the restatement, through the host-only entry point ``rtmodt_health_decide`` and through ``tests/native/health_rule_check.cpp``, a
stand-alone program built plain and with the address / undefined-behaviour sanitizers (nothing is loaded into Python under a
sanitizer); the ABI's refusals, which need no device; and the premises of the module on the restatements alone: what a blurred, a
covered, a re-aimed and a frozen picture answer under the default thresholds, and what the motion detector makes of a covered lens.
PARITY UNPINNED: the reference has no counterpart, and no default has been validated on real footage."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import health_cases as HC  # noqa: E402
import health_ref as HR  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "health_rule_check.cpp")
RULE_FIELDS = tuple(k for k in HR.DEFAULTS if k != "scale")
D, B, C_, M, F_, Z = (1 << i for i in range(6))                                  # dark, bright, covered, moved, defocused, frozen


def grey(rows):
    """A frame whose pixel (x, y) has luma rows[y][x] exactly (B = G = R = v gives Y = v)."""
    a = np.asarray(rows, np.uint8)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2))


def counts(**kw):
    return dict(dict(luma_sum=0, sharp=0, n_dark=0, n_bright=0, n_changed=1000, n_edge=0, n_ref_edge=0, n_kept=0), **kw)


def state(**kw):
    return dict(HR.fresh_state(), **kw)


# ---- hand-worked literal cases: G and F ------------------------------------------------------------------------------------
def test_coarse_structure_on_a_3x3_grid():
    y = [[10, 20, 30], [40, 50, 90], [70, 80, 200]]
    want = [[0, 0, 0], [0, abs(90 - 40) + abs(80 - 20), 0], [0, 0, 0]]               # 110: only the centre cell is interior
    assert HR.coarse(y).tolist() == want == HR.coarse_loop(y).tolist()
    assert HR.coarse([[0, 0, 0], [0, 9, 255], [0, 255, 0]])[1, 1] == 255              # 255 + 255 saturates
    assert HR.coarse([[0, 7, 0], [3, 9, 3], [0, 7, 0]])[1, 1] == 0                    # the cell itself does not count
    assert not HR.coarse(np.full((2, 9), 50)).any() and not HR.coarse(np.full((9, 2), 50)).any() and not HR.coarse([[5]]).any()
    y4 = np.int64([[0, 0, 0, 0], [10, 20, 40, 80], [0, 0, 0, 0]])
    assert HR.coarse(y4).tolist() == [[0] * 4, [0, 30, 60, 0], [0] * 4]
    rng = np.random.default_rng(3701)
    for gh, gw in ((3, 3), (5, 9), (1, 7), (12, 4), (17, 31)):
        y = rng.integers(0, 256, (gh, gw))
        assert HR.coarse(y).tolist() == HR.coarse_loop(y).tolist()


def test_fine_detail_on_a_two_row_frame():
    frame = grey([[10, 20, 15, 15, 40], [0, 255, 0, 255, 0]])                        # row 0: |d| = 10, 5, 0, 25; row 1: 255 four times
    assert HR.fine_detail(frame, 1).tolist() == [[10, 5, 0, 25, 0], [255, 255, 255, 255, 0]]        # the last column has no x + 1 < w
    assert HR.fine_detail(frame, 2).tolist() == [[10 + 5 + 510, 0 + 25 + 510, 0]]    # the pair (1, 2) belongs to pixel 1's cell
    assert HR.fine_detail(frame, 4).tolist() == [[40 + 1020, 0]]                     # (3, 4) crosses the cell border and counts for cell 0
    assert HR.fine_detail(frame, 8).tolist() == [[1060]]
    for scale in (1, 2, 4, 8):
        assert HR.fine_detail(frame, scale).tolist() == HR.fine_detail_loop(frame, scale).tolist()
    assert HR.fine_detail(grey([[7], [9]]), 1).tolist() == [[0], [0]]                # one column: no neighbour at all
    rng = np.random.default_rng(3702)
    for h, w, scale in ((5, 9, 4), (7, 13, 2), (3, 17, 8), (6, 6, 1)):
        fr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert HR.fine_detail(fr, scale).tolist() == HR.fine_detail_loop(fr, scale).tolist()
        assert MR.cell_luma(fr, scale).tolist() == MR.cell_luma_loop(fr, scale).tolist()


def test_counts_on_a_small_grid():
    c = HR.config(edge_threshold=24, dark_level=16, bright_level=240)
    yc = np.int64([[16, 17, 240, 239], [100, 100, 130, 100], [100, 100, 100, 100]])
    g = HR.coarse(yc)
    assert g.tolist() == [[0] * 4, [0, 30 + 83, 0 + 140, 0], [0] * 4]
    r = np.int64([[0, 0, 0, 0], [9999, 24 << 8, (24 << 8) - 1, 0], [0, 0, 0, 0]])
    prev = yc.copy()
    prev[2, 3] = 99
    k = HR.counts_of(yc, np.int64([[1, 2], [3, 4]]), g, prev, r, 5, c)
    # R holds a reference edge at (1, 0) and (1, 1); only (1, 1) is an edge now ((1, 0) is no interior cell: G 0); (1, 2) is one below
    assert k == dict(luma_sum=int(yc.sum()), sharp=10, n_dark=1, n_bright=1, n_changed=1, n_edge=2, n_ref_edge=2, n_kept=1)
    assert HR.counts_of(yc, np.int64([[0]]), g, prev, r, 0, c)["n_changed"] == 12                   # the first frame: every cell
    g[1, 1] = 11                                                                                    # 2 G = 22 < 24: not even a weak edge
    assert HR.counts_of(yc, np.int64([[0]]), g, prev, r, 5, c)["n_kept"] == 0
    g[1, 1] = 12
    assert HR.counts_of(yc, np.int64([[0]]), g, prev, r, 5, c)["n_kept"] == 1 and HR.counts_of(yc, np.int64([[0]]), g, prev, r, 5, c)["n_edge"] == 1


# ---- hand-worked literal cases: each condition at its threshold and one below ---------------------------------------------------
def test_raw_conditions_at_their_thresholds():
    c = HR.config()
    raw = lambda seen=25, ref=1000 << 8, cfg=c, **kw: HR.raw_of(counts(**kw), 1000, seen, ref, cfg)          # noqa: E731
    ok = dict(n_ref_edge=100, n_kept=100, n_edge=100, sharp=1000)
    assert raw(**ok) == 0
    assert raw(**dict(ok, n_dark=950)) == D and raw(**dict(ok, n_dark=949)) == 0
    assert raw(**dict(ok, n_bright=950)) == B and raw(**dict(ok, n_bright=949)) == 0
    assert raw(**dict(ok, n_kept=50)) == 0 and raw(**dict(ok, n_kept=49)) == M                       # 49 000 < 500 x 100: lost, with edges of its own
    assert raw(**dict(ok, n_kept=49, n_edge=30)) == M and raw(**dict(ok, n_kept=49, n_edge=29)) == C_   # 29 000 < 300 x 100
    assert raw(**dict(ok, sharp=500)) == 0 and raw(**dict(ok, sharp=499)) == F_                      # 499 000 < 500 x 1000
    assert raw(ref=(1000 << 8) + 255, **dict(ok, sharp=500)) == 0                                    # the fraction of ref_sharp is dropped
    assert raw(**dict(ok, n_kept=49, sharp=0)) == M                                                  # lost: never defocused
    assert raw(**dict(ok, n_ref_edge=16, n_kept=16, n_edge=16)) == 0
    assert raw(**dict(ok, n_ref_edge=15, n_kept=0, n_edge=0, sharp=0)) == HR.NO_STRUCTURE              # too little to judge by
    assert raw(**dict(ok, n_ref_edge=15, n_kept=0, n_dark=1000)) == D | HR.NO_STRUCTURE
    assert raw(seen=24, **dict(ok, n_dark=1000, n_kept=0, sharp=0)) == 0                             # warm-up: only FROZEN is evaluated
    assert raw(**dict(ok, n_changed=0)) == Z and raw(**dict(ok, n_changed=1)) == 0
    assert raw(seen=1, **dict(ok, n_changed=0)) == Z and raw(seen=0, **dict(ok, n_changed=0)) == 0
    assert raw(cfg=HR.config(freeze_cells=7), **dict(ok, n_changed=7)) == Z and raw(cfg=HR.config(freeze_cells=7), **dict(ok, n_changed=8)) == 0
    # a parameter of 0 switches its condition off
    assert raw(cfg=HR.config(dark_pm=0), **dict(ok, n_dark=1000)) == 0 and raw(cfg=HR.config(bright_pm=0), **dict(ok, n_bright=1000)) == 0
    assert raw(cfg=HR.config(retain_pm=0), **dict(ok, n_kept=0, n_edge=0)) == 0
    assert raw(cfg=HR.config(cover_pm=0), **dict(ok, n_kept=0, n_edge=0)) == M
    assert raw(cfg=HR.config(defocus_pm=0), **dict(ok, sharp=0)) == 0 and raw(cfg=HR.config(freeze_frames=0), **dict(ok, n_changed=0)) == 0
    assert raw(cfg=HR.config(min_ref_edges=0), **dict(ok, n_ref_edge=0, n_kept=0, n_edge=0)) == 0     # 0 < 0 never holds


# ---- hand-worked literal cases: debounce, learning, relearn --------------------------------------------------------------------
def run_script(script, c, st=None):
    """One frame per letter -- c overed, m oved, f (de)focused, d ark, z frozen, . healthy -> (events per frame, learn per frame, state)."""
    ok = dict(n_ref_edge=100, n_kept=100, n_edge=100, sharp=1000)
    rows = {".": ok, "c": dict(ok, n_kept=0, n_edge=0), "m": dict(ok, n_kept=0), "f": dict(ok, sharp=10), "d": dict(ok, n_dark=1000), "z": dict(ok, n_changed=0)}
    st = state(frames_seen=100, ref_sharp=1000 << 8) if st is None else st
    ev, learn = [], []
    for ch in script:
        _, l_, e = HR.decide(counts(**rows[ch]), 1000, st, c)
        ev.append(e)
        learn.append(l_)
    return ev, learn, st


def test_debounce_runs():
    c = HR.config(hold_frames=3, clear_frames=2, freeze_frames=3, ref_shift=1)
    R_, X_ = HR.RAISED, HR.CLEARED
    ev, learn, st = run_script("cc.ccc.c..", c)
    #                  a run of two is forgotten; the third of three raises; one healthy frame does not clear, two do
    assert ev == [[], [], [], [], [], [(HR.COVERED, R_)], [], [], [], [(HR.COVERED, X_)]]
    assert learn == [0, 0, 1, 0, 0, 0, 0, 0, 0, 1]                                   # neither a raw nor an active frame is learned
    assert st["active"] == 0 and st["run"] == [0] * 6 and st["off"] == [0] * 6
    ev, _, st = run_script("zzzz.zz", c)
    assert ev == [[], [], [(HR.FROZEN, R_)], [], [(HR.FROZEN, X_)], [], []]          # FROZEN clears on the first changed frame
    assert st["run"][HR.FROZEN] == 2
    ev, learn, _ = run_script("zzz", c)
    assert learn == [1, 1, 1]                                                        # a frozen picture is still the scene: it is learned
    ev, _, st = run_script("mmmccc", c)                                              # moved, then covered: both latched for a while
    assert ev == [[], [], [(HR.MOVED, R_)], [], [(HR.MOVED, X_)], [(HR.COVERED, R_)]]
    ev, _, st = run_script("cccccc", c)
    assert st["active"] == C_ and st["run"][HR.COVERED] == 3 and st["off"][HR.COVERED] == 0      # its age: three frames since it was raised
    # ref_sharp: set on the first frame, an arithmetic shift after
    st = state()
    HR.decide(counts(sharp=1000), 1000, st, c)
    assert (st["ref_sharp"], st["frames_seen"]) == (1000 << 8, 1)
    assert HR.decide(counts(sharp=999), 1000, st, c)[1] == HR.LEARN_AVERAGE and st["ref_sharp"] == (1000 << 8) - 128
    HR.decide(counts(sharp=0), 1000, state(frames_seen=1, ref_sharp=1), c)
    st = state(frames_seen=1, ref_sharp=1)
    HR.decide(counts(sharp=0), 1000, st, c)
    assert st["ref_sharp"] == 0                                                      # -1 >> 1 = -1: floor, not towards zero
    assert HR.learn_r(np.int64([25600, 25601, 0]), np.int64([99, 100, 255]), HR.LEARN_AVERAGE, HR.config(ref_shift=2)).tolist() == [25600 - 64, 25600, 16320]
    assert HR.learn_r(np.int64([7]), np.int64([3]), HR.LEARN_SET, c).tolist() == [768] and HR.learn_r(np.int64([7]), np.int64([3]), HR.LEARN_NONE, c).tolist() == [7]


def test_relearn_order_of_events_and_the_most_a_call_can_emit():
    c = HR.config(hold_frames=3, clear_frames=9, freeze_frames=3, relearn_frames=4)
    R_, X_, RB = HR.RAISED, HR.CLEARED, HR.REBASED
    ev, learn, st = run_script("ccccccc.", c)                                        # raised on frame 2, age 4 on frame 6
    assert ev == [[], [], [(HR.COVERED, R_)], [], [], [], [(HR.COVERED, X_), (-1, RB)], []]
    assert learn == [0] * 7 + [HR.LEARN_SET] and st["frames_seen"] == 1 and st["active"] == 0        # the next frame starts the new reference
    # two latched structure conditions: CLEARED in condition order, then REBASED
    st = state(frames_seen=100, ref_sharp=1000 << 8, active=C_ | F_, run=[0, 0, 1, 0, 3, 0], off=[0, 0, 4, 0, 0, 0])
    ev, _, st = run_script("f", c, st)
    assert ev == [[(HR.COVERED, X_), (HR.DEFOCUSED, X_), (-1, RB)]] and st["frames_seen"] == 0 and st["run"] == [0] * 6 and st["off"] == [0] * 6
    # an operator's rebase: the state changes at once, the events come first in the next call
    st = state(frames_seen=100, ref_sharp=1000 << 8, active=D | M | Z, run=[5, 0, 0, 7, 0, 9])
    HR.rebase_now(st)
    assert (st["frames_seen"], st["active"], st["pending"], st["run"]) == (0, D | Z, HR.PENDING_REBASE | M, [5, 0, 0, 0, 0, 9])
    ev, learn, st = run_script(".", HR.config(hold_frames=3, clear_frames=1, freeze_frames=3), st)
    assert ev == [[(HR.MOVED, X_), (-1, RB), (HR.DARK, X_), (HR.FROZEN, X_)]] and learn == [HR.LEARN_SET] and st["pending"] == 0
    st = state(frames_seen=3)
    HR.rebase_now(st)
    assert st["pending"] == HR.PENDING_REBASE and run_script(".", c, st)[0] == [[(-1, RB)]]
    # eight events: dark, bright and frozen clear, moved is raised, and the relearn clears the three structure conditions
    c8 = HR.config(hold_frames=3, clear_frames=2, freeze_frames=3, relearn_frames=4)
    st = state(frames_seen=100, ref_sharp=1000 << 8, active=D | B | C_ | F_ | Z, run=[9, 9, 3, 2, 1, 9], off=[1, 1, 0, 0, 0, 0])
    ev, _, st = run_script("m", c8, st)
    assert ev == [[(HR.DARK, X_), (HR.BRIGHT, X_), (HR.MOVED, R_), (HR.FROZEN, X_), (HR.COVERED, X_), (HR.MOVED, X_), (HR.DEFOCUSED, X_), (-1, RB)]]
    assert len(ev[0]) == HR.MAX_EVENTS and st["active"] == 0


# ---- the header: random counts and states --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decide_cases():
    """((the sixteen rule fields), cells, counts, state)"""
    rng = np.random.default_rng(3703)
    out = []
    pick = lambda *v: int(rng.choice(v))                                             # noqa: E731
    for i in range(3000):
        hold, clear, freeze, relearn = pick(1, 2, 3, 25, 65535), pick(1, 2, 25, 65535), pick(0, 1, 3, 50, 65535), pick(0, 0, 1, 4, 2 ** 30)
        warm = pick(1, 4, 25, 255)
        rule = dict(edge_threshold=pick(1, 24, 255), ref_shift=pick(1, 6, 12), warmup=warm, dark_level=pick(0, 16, 255), dark_pm=pick(0, 1, 950, 1000),
                    bright_level=pick(0, 240, 255), bright_pm=pick(0, 950, 1000), retain_pm=pick(0, 500, 1000), cover_pm=pick(0, 300, 1000),
                    defocus_pm=pick(0, 500, 1000), min_ref_edges=pick(0, 16, 2 ** 24), hold_frames=hold, clear_frames=clear, freeze_frames=freeze,
                    freeze_cells=pick(0, 0, 5, 2 ** 24), relearn_frames=relearn)
        cells = pick(1, 6, 1000, 129600, 2 ** 24)
        n = lambda: int(min(cells, pick(0, 1, cells // 2, cells * 19 // 20, cells * 19 // 20 + 1, cells, int(rng.integers(0, cells + 1)))))      # noqa: E731
        ref_edges = n()
        near = lambda pm: int(np.clip(ref_edges * pm // 1000 + pick(-1, 0, 1), 0, cells))          # noqa: E731
        sharp = pick(0, 1, 1000, 123456789, 2 ** 38, int(rng.integers(0, 2 ** 30)))
        k = dict(luma_sum=int(rng.integers(0, 255 * cells + 1)), sharp=sharp, n_dark=n(), n_bright=n(), n_changed=min(cells, pick(0, 0, 1, 5, 6, cells)),
                 n_edge=pick(n(), near(rule["cover_pm"])), n_ref_edge=ref_edges, n_kept=pick(n(), near(rule["retain_pm"])))
        timer = lambda: pick(0, 0, 1, hold - 1, hold, clear - 1, max(freeze - 1, 0), max(relearn - 1, 0), relearn, 2 ** 30)       # noqa: E731
        pending = pick(0, 0, 0, HR.PENDING_REBASE, HR.PENDING_REBASE | C_, HR.PENDING_REBASE | HR.STRUCTURE)
        st = dict(ref_sharp=pick(0, 1, sharp << 8, (2 * sharp << 8) + 255, (2 * sharp << 8) + 256, 2 ** 46), frames_seen=pick(0, 1, warm - 1, warm, warm + 1, 2 ** 30),
                  active=int(rng.integers(0, 64)), pending=pending, run=[timer() for _ in range(6)], off=[timer() for _ in range(6)])
        if pending:                                                                  # what a rebase leaves behind until the next frame
            st["frames_seen"], st["active"] = 0, st["active"] & ~HR.STRUCTURE
        out.append((rule, cells, k, st))
    return out


def state_text(st):
    return " ".join(str(v) for v in [st["ref_sharp"], st["frames_seen"], st["active"], st["pending"]] + list(st["run"]) + list(st["off"]))


def ref_decide(case):
    rule, cells, k, st = case
    st = copy.deepcopy(st)
    raw, learn, ev = HR.decide(k, cells, st, HR.config(**rule))
    return raw, learn, ev, st


def test_the_cases_reach_every_condition_event_and_step():
    seen_raw = seen_kinds = 0
    learns, most = set(), 0
    for case in decide_cases():
        raw, learn, ev, _ = ref_decide(case)
        seen_raw |= raw
        learns.add(learn)
        most = max(most, len(ev))
        for cond, kind in ev:
            seen_kinds |= 1 << kind
    assert seen_raw == 63 | HR.NO_STRUCTURE and learns == {0, 1, 2} and seen_kinds == 0b1110 and most >= 6


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("health_rule_check_san" if sanitize else "health_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built health_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_health_rule_header_equals_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    rng = np.random.default_rng(3704)
    lines, want = [], []
    for case in decide_cases():
        rule, cells, k, st = case
        lines.append("d " + " ".join(str(rule[f]) for f in RULE_FIELDS) + f" {cells} " + " ".join(str(k[f]) for f in HR.COUNTS) + " " + state_text(st))
        raw, learn, ev, new = ref_decide(case)
        want.append(f"{raw} {learn} {state_text(new)} {len(ev)}" + "".join(f" {c_} {kind}" for c_, kind in ev))
        if len(want) % 10 == 0:
            lines.append("b " + state_text(st))
            new = copy.deepcopy(st)
            HR.rebase_now(new)
            want.append(state_text(new))
    for _ in range(300):
        l_, r_, u_, d_ = (int(v) for v in rng.choice([0, 1, 127, 128, 255, int(rng.integers(0, 256))], 4))
        lines.append(f"g {l_} {r_} {u_} {d_}")
        want.append(str(min(255, abs(r_ - l_) + abs(d_ - u_))))
    for _ in range(600):
        big_r, g = int(rng.choice([0, 1, 65280, (24 << 8) - 1, 24 << 8, int(rng.integers(0, 65281))])), int(rng.choice([0, 11, 12, 23, 24, 255, int(rng.integers(0, 256))]))
        learn, shift, thr = int(rng.integers(0, 3)), int(rng.integers(1, 13)), int(rng.choice([1, 24, 255]))
        lines.append(f"r {big_r} {g} {learn} {shift} {thr}")
        got_r = int(HR.learn_r(np.int64([big_r]), np.int64([g]), learn, dict(ref_shift=shift))[0])
        assert 0 <= got_r <= 65280
        want.append(f"{got_r} {int(g >= thr)} {int(2 * g >= thr)} {int(big_r >= thr << 8)}")
    zeros = " ".join(["0"] * 12)
    good_rule = " ".join(str(HR.DEFAULTS[f]) for f in RULE_FIELDS)
    extra = [f"d {good_rule.replace('24', '0', 1)} 10 0 0 0 0 0 0 0 0 0 0 0 0 {zeros}",          # edge_threshold 0
             f"d {good_rule} 0 0 0 0 0 0 0 0 0 0 0 0 0 {zeros}",                                    # no cells
             f"d {good_rule} 10 0 0 0 0 0 0 0 0 0 -1 0 0 {zeros}",                                  # frames_seen -1
             f"d {good_rule} 10 0 0 0 0 0 0 0 0 0 0 64 0 {zeros}",                                  # an unknown active bit
             f"d {good_rule} 10 0 0 0 0 0 0 0 0 0 0 0 4 {zeros}",                                   # owed events without a rebase
             f"d {good_rule} 10 0 0 0 0 0 0 0 0 0 5 0 256 {zeros}",                                 # an owed rebase and frames_seen 5
             f"d {good_rule} 10 0 0 0 0 0 0 0 0 0 0 4 256 {zeros}",                                 # an owed rebase and COVERED active
             f"b 0 0 0 0 {' '.join(['0'] * 11)} -1", "r 65281 0 0 1 1"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(want) + len(extra) + 1 and got[-1] == f"done {len(want) + len(extra)}"
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert g_ == w_, (lines[i], g_[:300], w_[:300])
    assert got[len(want):-1] == ["bad"] * len(extra)


# ---- the library: the host-only entry point, defaults, refusals, exports ----------------------------------------------------------
def test_health_decide_entry_point_equals_restatement(pkg):
    H = pkg.ingestion.health
    for case in decide_cases()[:1500]:
        rule, cells, k, st = case
        raw, learn, ev, new = H.health_decide(k, cells, st, frame_id=77, **rule)
        w_raw, w_learn, w_ev, w_new = ref_decide(case)
        assert (raw, learn, ev, new) == (w_raw, w_learn, [(c_, kind, 77) for c_, kind in w_ev], w_new), case
    k, st = counts(), HR.fresh_state()
    E = pkg._ffi.RtmodtError
    for bad in (dict(edge_threshold=0), dict(edge_threshold=256), dict(ref_shift=0), dict(ref_shift=13), dict(warmup=0), dict(warmup=256), dict(dark_level=-1),
                dict(bright_level=256), dict(dark_pm=-1), dict(bright_pm=1001), dict(retain_pm=1001), dict(cover_pm=-1), dict(defocus_pm=1001),
                dict(min_ref_edges=-1), dict(hold_frames=0), dict(hold_frames=65536), dict(clear_frames=0), dict(freeze_frames=-1), dict(freeze_frames=65536),
                dict(freeze_cells=-1), dict(relearn_frames=-1), dict(relearn_frames=2 ** 30 + 1)):
        with pytest.raises(E) as e:
            H.health_decide(k, 1000, st, **bad)
        assert e.value.code == pkg._ffi.E_INVALID, bad
    for bad_k, bad_st, cells in ((dict(k, n_dark=1001), st, 1000), (dict(k, sharp=2 ** 40), st, 1000), (dict(k, n_changed=0), dict(st, frames_seen=-1), 1000),
                                 (dict(k, n_changed=0), dict(st, active=64), 1000), (dict(k, n_changed=0), dict(st, pending=4), 1000), (dict(k, n_changed=0), dict(st, pending=256, frames_seen=5), 1000),
                                 (dict(k, n_changed=0), dict(st, pending=256, active=4), 1000),
                                 (dict(k, n_changed=0), dict(st, run=[0, 0, 0, 0, 0, -1]), 1000), (dict(k, n_changed=0), st, 0)):
        with pytest.raises(E) as e:
            H.health_decide(bad_k, cells, bad_st)
        assert e.value.code == pkg._ffi.E_INVALID, (bad_k, bad_st)


def test_health_cfg_defaults_refusals_and_exports(pkg):
    import ctypes as C
    H = pkg.ingestion.health
    L = pkg._ffi.lib()
    cfg = H.make_cfg()
    assert {f: getattr(cfg, f) for f in H.CFG_FIELDS} == HR.DEFAULTS and (cfg.streams, cfg.height, cfg.width, cfg.device) == (1, 0, 0, 0)
    assert HR.DEFAULTS == dict(scale=4, edge_threshold=24, ref_shift=6, warmup=25, dark_level=16, dark_pm=950, bright_level=240, bright_pm=950, retain_pm=500,
                               cover_pm=300, defocus_pm=500, min_ref_edges=16, hold_frames=25, clear_frames=25, freeze_frames=50, freeze_cells=0, relearn_frames=0)
    ok = dict(streams=2, height=37, width=70)
    # a parameter outside its range is refused before the device is touched (no device is needed for it); the defaults lack a frame size
    for kw in (dict(), dict(ok, streams=0), dict(ok, streams=1025), dict(ok, height=0), dict(ok, width=32769), dict(ok, scale=0), dict(ok, scale=3),
               dict(ok, scale=16), dict(ok, edge_threshold=0), dict(ok, edge_threshold=256), dict(ok, ref_shift=0), dict(ok, ref_shift=13), dict(ok, warmup=0),
               dict(ok, warmup=256), dict(ok, dark_level=256), dict(ok, bright_level=-1), dict(ok, dark_pm=1001), dict(ok, bright_pm=-1), dict(ok, retain_pm=1001),
               dict(ok, cover_pm=1001), dict(ok, defocus_pm=-1), dict(ok, min_ref_edges=-1), dict(ok, hold_frames=0), dict(ok, clear_frames=65536),
               dict(ok, freeze_frames=-1), dict(ok, freeze_cells=-1), dict(ok, relearn_frames=-1)):
        h = C.c_void_p()
        bad = H.make_cfg(**kw)
        assert L.rtmodt_health_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw
    h = C.c_void_p()
    big = H.make_cfg(streams=1, height=8192, width=8192, scale=1)                # 2^26 cells
    assert L.rtmodt_health_create(C.byref(big), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value and b"cells" in L.rtmodt_last_error()
    many = H.make_cfg(streams=1024, height=4096, width=4096, scale=4)            # 2^20 cells x 1024 streams
    assert L.rtmodt_health_create(C.byref(many), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value
    assert L.rtmodt_health_create(None, C.byref(h)) == pkg._ffi.E_INVALID
    assert L.rtmodt_health_process(None, None, None, None, 0, 1, 1, 3, 0, None, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_health_reset(None, 0) == pkg._ffi.E_INVALID and L.rtmodt_health_rebase(None, 0) == pkg._ffi.E_INVALID
    assert L.rtmodt_health_read_state(None, 0, None, None, None) == pkg._ffi.E_INVALID and L.rtmodt_health_last_ms(None, None) == pkg._ffi.E_INVALID
    L.rtmodt_health_destroy(None)
    with pytest.raises(TypeError):
        H.make_cfg(dilate=1)
    assert pkg.ingestion.CameraHealth is H.CameraHealth
    assert (H.CONDITION_NAMES, H.NO_STRUCTURE, H.MAX_EVENTS) == (HR.NAMES, HR.NO_STRUCTURE, HR.MAX_EVENTS)
    assert H.condition_names(C_ | Z) == ("covered", "frozen") == HR.names_of(C_ | Z)
    declared = [s for s in pkg._ffi.header_symbols() if s.startswith("rtmodt_health_")]
    assert len(declared) == 10 and all(hasattr(L, s) and s in L._signatures for s in declared)
    import inspect
    assert inspect.signature(pkg.pipeline.run).parameters["health"].default is None


# ---- the premises, on the restatements alone -------------------------------------------------------------------------------------
H_, W_ = 120, 160


@functools.lru_cache(maxsize=None)
def premise(kind, n=60):
    """40 healthy frames, then `n` frames of `kind`, through the default configuration -> the rows of the `n` frames."""
    rng = np.random.default_rng(3705)
    base = HC.scene(H_, W_, 1)
    ref = HR.Ref(1, H_, W_)
    for _ in range(40):
        row = ref.step(0, HC.noisy(base, rng))
        assert row["raw"] == 0 and not row["events"]
    v = HC.view(kind, base, H_, W_)
    rows, frame = [], None
    for _ in range(n):
        frame = frame if kind == "repeated" and frame is not None else HC.noisy(v, rng)
        rows.append(ref.step(0, frame))
    return rows


def raised(rows):
    return [(cond, kind, fid - 40) for r in rows for cond, kind, fid in r["events"]]


def test_premise_a_blurred_copy_is_defocused_and_not_lost():
    rows = premise("blurred")
    assert all(r["raw"] == F_ for r in rows)
    assert all(1000 * r["n_kept"] >= 500 * r["n_ref_edge"] and r["n_ref_edge"] >= 100 for r in rows)         # the structure is in place
    assert all(1000 * r["sharp"] < 500 * (r["ref_sharp"] >> 8) for r in rows)                                # less than half of the fine detail
    assert raised(rows) == [(HR.DEFOCUSED, HR.RAISED, 24)] and all(r["learned"] == 0 for r in rows)


def test_premise_a_uniform_grey_with_noise_is_covered():
    rows = premise("covered")
    assert all(r["raw"] == C_ and r["n_edge"] == 0 and r["n_kept"] == 0 for r in rows)
    assert raised(rows) == [(HR.COVERED, HR.RAISED, 24)] and rows[-1]["active"] == C_ and all(r["learned"] == 0 for r in rows)


def test_premise_the_scene_shifted_by_a_third_is_moved():
    rows = premise("shifted")
    assert all(r["raw"] == M and 1000 * r["n_edge"] >= 900 * r["n_ref_edge"] for r in rows)                  # as much structure, elsewhere
    assert raised(rows) == [(HR.MOVED, HR.RAISED, 24)]


def test_premise_a_repeated_frame_is_frozen():
    rows = premise("repeated", 70)
    assert [r["n_changed"] for r in rows][1:] == [0] * 69 and rows[0]["n_changed"] > 0
    assert all(r["raw"] == Z for r in rows[1:]) and raised(rows) == [(HR.FROZEN, HR.RAISED, 50)]              # the 50th repetition


def test_premise_darkness_and_dazzle():
    assert raised(premise("dark")) == [(HR.DARK, HR.RAISED, 24), (HR.COVERED, HR.RAISED, 24)]                # a black picture has no structure either
    assert raised(premise("bright")) == [(HR.BRIGHT, HR.RAISED, 24), (HR.COVERED, HR.RAISED, 24)]


def test_premise_the_unchanged_scene_raises_nothing_over_200_frames():
    rows = premise("healthy", 200)
    assert all(r["raw"] == 0 and r["active"] == 0 and not r["events"] and r["learned"] == 1 for r in rows)
    assert min(r["n_changed"] for r in rows) > 50


def test_premise_the_motion_detector_learns_a_covered_lens_as_background():
    """The gap the module closes: one SCENE_CHANGE, a warm-up on the covered picture, then STILL for good."""
    rng = np.random.default_rng(3706)
    base = HC.scene(H_, W_, 1)
    mo = MR.Ref(1, H_, W_)
    before = [mo.step(0, HC.noisy(base, rng))["status"] for _ in range(40)]
    after = [mo.step(0, HC.noisy(HC.covered(H_, W_), rng))["status"] for _ in range(60)]
    assert before == [MR.WARMUP] * 8 + [MR.STILL] * 32
    assert after == [MR.SCENE_CHANGE] + [MR.WARMUP] * 8 + [MR.STILL] * 51
