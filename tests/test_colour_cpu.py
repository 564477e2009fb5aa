"""CPU: the colour attributes' rules without a GPU.  ``tests/colour_ref.py`` (the restatement the kernels of ``csrc/colour.hip`` are
pinned to) against literals -- the sRGB names, every hue bound from both sides, hand-worked plans, occluder order and cap, ageing,
label ties, the retention sequence -- and with one deliberate defect at a time, which the literals catch; an exhaustive sweep of a
5-stepped RGB cube (plain ints against the vectorised statement); the rules of ``csrc/colour_rule.h`` against the restatement,
through ``tests/native/colour_rule_check.cpp`` -- a stand-alone program built plain and with the address / undefined-behaviour
sanitizers (nothing is loaded into Python under a sanitizer) -- and through the host-only entry points ``rtmodt_colour_name`` /
``rtmodt_colour_plan``; the ABI's refusals, which need no device; and the premise of the module on the restatement alone.
PARITY UNPINNED: agreement of the names with human colour naming or any product's; every default, validated on no real footage."""
import ctypes as C
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_cases as CC  # noqa: E402
import colour_ref as R  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402
from test_motion_cpu import lcg_bytes  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "colour_rule_check.cpp")
K = R.Cfg()
H, W = 240, 320


def name_of(r, g, b, defect=None):
    return R.NAMES[R.name_int(K, b, g, r, defect)]


# ---- the name of a pixel ------------------------------------------------------------------------------------------------------
def test_name_literals():
    for want, pixels in CC.NAME_LITERALS.items():
        for r, g, b in pixels:
            assert name_of(r, g, b) == want, (want, (r, g, b))
    assert len(R.NAMES) == 12 and R.NAMES == ("black", "grey", "white", "red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown")


def test_hue_floor_literal():
    """(b, g, r) = (168, 71, 200): c = 129, (g - b) * 256 / c = -24832 / 129 = -192.49..., floor -193 -> 1343, PURPLE; truncation gives
    -192 -> 1344, PINK."""
    assert R.hue_int(168, 71, 200) == 1343 and R.hue_int(168, 71, 200, "trunc_hue") == 1344
    assert name_of(200, 71, 168) == "purple" and name_of(200, 71, 168, "trunc_hue") == "pink"


def second_hue(b, g, r):
    """The hue from exact fractions: a second statement of the floor."""
    mx, c = max(b, g, r), max(b, g, r) - min(b, g, r)
    if r == mx:
        return math.floor(Fraction((g - b) * 256, c)) % 1536
    if g == mx:
        return (512 + math.floor(Fraction((b - r) * 256, c))) % 1536
    return (1024 + math.floor(Fraction((r - g) * 256, c))) % 1536


def bright_pixels():
    """Saturated pixels with max 255 and min 0: the pink and brown cases do not apply, every hue 0..1535 but the few c = 255 skips."""
    out = {}
    for v in range(256):
        for b, g, r in ((0, v, 255), (0, 255, v), (v, 255, 0), (255, v, 0), (255, 0, v), (v, 0, 255)):
            out.setdefault(second_hue(b, g, r), (b, g, r))
    return out


def test_every_hue_bound_from_both_sides():
    px = bright_pixels()
    for bound, below, above in CC.HUE_SIDES:
        lo = max(h for h in px if h < bound)
        hi = min(h for h in px if h >= bound)
        assert bound - lo <= 2 and hi - bound <= 1, (bound, lo, hi)
        for h, want in ((lo, below), (hi, above)):
            b, g, r = px[h]
            assert R.hue_int(b, g, r) == h and name_of(r, g, b) == want, (bound, h, (b, g, r))
    # c = 128 doubles (g - b): hue 62 is red, hue 64 orange, hand-worked; and the two ends of the circle
    assert name_of(255, 158, 127) == "red" and name_of(255, 159, 127) == "orange"
    assert R.hue_int(0, 0, 255) == 0 and R.hue_int(1, 0, 255) == 1534 and name_of(255, 0, 1) == "red"
    # the pink and brown cases of the red, orange and yellow ranges: thresholds from both sides
    assert name_of(192, 120, 120) == "pink" and name_of(191, 120, 120) == "red"            # 2 c < mx, mx >= 192 | mx 191
    assert name_of(192, 96, 96) == "red"                                                    # 2 c == mx: not pink
    assert name_of(95, 10, 10) == "brown" and name_of(96, 10, 10) == "red"
    assert name_of(175, 80, 10) == "brown" and name_of(176, 80, 10) == "orange"            # hue 108 / 107
    assert name_of(127, 120, 10) == "brown" and name_of(128, 121, 10) == "yellow"
    # the achromatic rules: black_max, chroma_min, both saturations, both luma thresholds
    assert name_of(47, 0, 0) == "black" and name_of(48, 0, 0) == "brown" and name_of(100, 0, 0) == "red"      # black_max, then red_brown_mx
    assert name_of(119, 100, 100) == "grey" and name_of(220, 181, 181) == "white" and name_of(220, 180, 180) == "pink"   # 39000 <= 39600 | 40000
    assert name_of(95, 57, 57) == "grey" and name_of(95, 56, 56) == "brown"                # sat_lo: 38000 <= 38000 | 39000 > 38000
    assert name_of(63, 63, 63) == "black" and name_of(64, 64, 64) == "grey" and name_of(175, 175, 175) == "grey" and name_of(176, 176, 176) == "white"


def test_noise_leaves_the_twelve_names_alone():
    rng = np.random.default_rng(12)
    for want, pixels in CC.NAME_LITERALS.items():
        r, g, b = pixels[0]
        px = np.clip(np.array([b, g, r])[None, :] + rng.integers(-6, 7, (4000, 3)), 0, 255)
        assert (R.name_vec(K, px) == R.NAMES.index(want)).all(), want


def test_cube_sweep_one_name_per_pixel_and_both_statements_agree():
    v = np.arange(0, 256, 5)
    cube = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    vec = R.name_vec(K, cube)
    assert vec.min() >= 0 and vec.max() <= 11 and len(set(vec.tolist())) == 12
    loop = [R.name_int(K, *p) for p in cube.tolist()]
    assert loop == vec.tolist()
    other = R.Cfg(black_max=30, chroma_min=0, sat_hi_pm=0, sat_lo_pm=0, hue=(10, 100, 300, 700, 900, 1100, 1300, 1536), pink_mx=0, red_brown_mx=256)
    sub = cube[::7]
    assert [R.name_int(other, *p) for p in sub.tolist()] == R.name_vec(other, sub).tolist()


def test_channel_tie_order_cannot_show_with_a_true_floor():
    """At r == g the r form gives 256 c / c = 256 and the g form 512 - 256; likewise 768 at g == b and 1280 at b == r: the forms meet
    exactly where two channels tie, so asking g before r changes no pixel.  (It would with a truncating division, which the
    literal of test_hue_floor_literal rules out.)"""
    v = np.arange(0, 256, 5)
    for a in v.tolist():
        for o in v.tolist():
            for b, g, r in ((o, a, a), (a, a, o), (a, o, a)):
                if max(b, g, r) != min(b, g, r):
                    assert R.hue_int(b, g, r, "tie_g_first") == R.hue_int(b, g, r) == second_hue(b, g, r)


# ---- plans ----------------------------------------------------------------------------------------------------------------------
def flat(P):
    return None if P is None else (P["raw"], P["box"], P["rect"], P["ys"], P["sx"], P["sy"], P["nx"], P["ny"])


def test_hand_worked_plans():
    for xyxy, want in CC.PLANS:
        assert flat(R.plan(K, xyxy, H, W)) == want, xyxy
    assert R.plan(R.Cfg(classes=(1, 2)), (100, 50, 139, 149), H, W, cls=0) is None
    assert R.plan(R.Cfg(classes=(1, 2)), (100, 50, 139, 149), H, W, cls=2) is not None
    # max_side 8: a stride in both axes; the last sample stays inside the rectangle
    P = R.plan(R.Cfg(max_side=8), (100, 50, 139, 149), H, W)
    assert (P["sx"], P["sy"], P["nx"], P["ny"]) == (3, 10, 8, 8) and 108 + 7 * 3 <= 131 and 65 + 7 * 10 <= 139
    # the floor-stride defect is caught by the max_side + 1 literal
    assert flat(R.plan(K, (10, 10, 90, 74), H, W, defect="stride_floor")) != CC.PLANS[8][1]


def test_split_row_belongs_to_lower():
    rng = np.random.default_rng(3)
    frame = CC.textured(40, 40, rng)
    CC.paint(frame, (10, 20, 19, 20), "red", rng)
    CC.paint(frame, (10, 21, 19, 21), "blue", rng)
    plans = [R.plan(K, (10, 20, 19, 22), 40, 40)]
    hist, fl = R.frame_hist(K, frame, plans, [1], 0)
    assert hist[R.RED] == 6 and hist[12 + R.BLUE] == 6 and sum(hist) == 12 and fl == 0
    bad, _ = R.frame_hist(K, frame, plans, [1], 0, defect="split_upper")
    assert bad != hist and bad[R.BLUE] == 6


# ---- occluders ------------------------------------------------------------------------------------------------------------------
def test_occluder_order_and_cap():
    boxes = [(10, 10, 60, 100), (20, 5, 70, 110), (15, 30, 65, 100)]          # ids 1, 2, 3: bottoms 100, 110, 100
    plans = [R.plan(K, b, H, W) for b in boxes]
    ids = [1, 2, 3]
    assert R.occluders(plans, ids, 0) == ([(20, 5, 70, 110), (15, 30, 65, 100)], False)       # 2: lower bottom; 3: same bottom, larger id
    assert R.occluders(plans, ids, 1) == ([], False)
    assert R.occluders(plans, ids, 2) == ([(20, 5, 70, 110)], False)
    assert R.occluders(plans, ids, 0, defect="occl_y0") != R.occluders(plans, ids, 0)           # on y0, box 2 (top 5) would stand BEHIND box 1
    far = plans + [R.plan(K, (200, 10, 250, 120), H, W)]                                        # nearer, but it does not meet the rectangle
    assert R.occluders(far, [1, 2, 3, 4], 0)[0] == R.occluders(plans, ids, 0)[0]
    # ten nearer boxes over one: the first 8 in list order are used, the flag says there were more
    many = [R.plan(K, (10, 10, 60, 100), H, W)] + [R.plan(K, (10 + q, 10, 60 + q, 101 + q), H, W) for q in range(10)]
    occ, more = R.occluders(many, list(range(11)), 0)
    assert more and occ == [(10 + q, 10, 60 + q, 101 + q) for q in range(8)]
    assert R.occluders(many[:9], list(range(9)), 0) == ([(10 + q, 10, 60 + q, 101 + q) for q in range(8)], False)
    # a hidden sample is not counted: the nearer box covers the left half of the sampled rectangle
    rng = np.random.default_rng(5)
    frame = CC.textured(H, W, rng)
    CC.paint(frame, (100, 50, 139, 149), "red", rng)
    two = [R.plan(K, (100, 50, 139, 149), H, W), R.plan(K, (60, 40, 119, 160), H, W)]
    hist, _ = R.frame_hist(K, frame, two, [1, 2], 0)
    assert sum(hist) == 12 * 38 and hist[R.RED] + hist[12 + R.RED] == 12 * 38              # columns 120..131 of 108..131 remain
    assert sum(R.frame_hist(R.Cfg(skip_occluded=0), frame, two, [1, 2], 0)[0]) == 24 * 38


# ---- rows -----------------------------------------------------------------------------------------------------------------------
def test_ageing_label_ties_and_thin_frames():
    row = [0] * 24
    row[R.RED] = (1 << 24) - 10
    assert R.accumulate(row, [0] * 3 + [10] + [0] * 20, 10) and row[R.RED] == 1 << 24            # == 2^24: not halved
    assert R.accumulate(row, [0] * 3 + [5] + [0] * 8 + [0] * 8 + [6] + [0] * 3, 11)
    assert row[R.RED] == ((1 << 24) + 5) // 2 and row[12 + R.BLUE] == 6                             # the upper part halved, the lower not
    assert not R.accumulate(row, [1] * 15 + [0] * 9, 16) and row[12 + R.BLUE] == 6                  # 15 samples < 16: not added
    assert R.label([0] * 24, R.WHOLE) == (-1, 0, -1, 0, 0)
    tie = [0] * 24
    tie[R.GREEN] = tie[R.RED] = 5
    tie[R.BLUE] = 3
    assert R.label(tie, R.UPPER) == (R.RED, 384, R.GREEN, 384, 13)                                 # ties: the lower index; 5000 // 13 = 384
    tie[12 + R.GREEN] = 1
    assert R.label(tie, R.WHOLE) == (R.GREEN, 428, R.RED, 357, 14) and R.label(tie, R.LOWER) == (R.GREEN, 1000, -1, 0, 1)


def test_retention_sequence():
    k = R.Cfg(retire_after=2, min_samples=1)
    st = R.Stream(k, 4)
    rng = np.random.default_rng(8)
    frame = CC.textured(60, 80, rng)
    CC.paint_person(frame, (10, 5, 29, 54), "red", "blue", rng)
    one = ([5], [(10, 5, 29, 54)], [0])
    code, u, r = st.process(*one, frame, 10)
    assert code == 0 and len(u) == 1 and u[0][6] == R.F_NEW and u[0][7] == 0 and r == [] and st.label(5) == ("red", "blue")
    assert st.process([], [], [], frame, 11)[1:] == ([], []) and st.process([], [], [], frame, 12)[1:] == ([], [])
    code, u, r = st.process(*one, frame, 12 + 1)                                                    # 13 - 10 = 3 > 2: retired, and a new row
    assert [x[0] for x in r] == [5] and r[0][2] == 10 and u[0][6] == R.F_NEW and u[0][1] == 13
    code, u, r = st.process([], [], [], frame, 14)
    assert r == [] and [x[0] for x in st.state()] == [5]
    code, u, r = st.process(*one, frame, 15)                                                        # 15 - 13 = 2: kept
    assert r == [] and u[0][6] == 0 and u[0][1] == 13 and u[0][5] == 2
    # overflow: 8 rows held, 5 idle + 4 members > 8: the idle rows go, the error stays
    st = R.Stream(k, 4)
    ids = list(range(8))
    assert st.process(ids[:4], [(10, 5, 29, 54)] * 4, [0] * 4, frame, 0)[0] == 0 and st.process(ids[4:], [(10, 5, 29, 54)] * 4, [0] * 4, frame, 1)[0] == 0
    code, u, r = st.process([3, 20, 21, 22], [(10, 5, 29, 54)] * 4, [0] * 4, frame, 2)
    assert code == -4 and r == [] and [x[0] for x in st.state()] == [3, 20, 21, 22]
    assert u[0][5:7] == (1, R.F_THIN) and u[3][5:7] == (1, R.F_NEW)           # the same box four times: only the largest id is not hidden
    assert st.process([], [], [], frame, 3)[0] == -4


# ---- the premise, on the restatement alone ------------------------------------------------------------------------------------------
def test_premise_person_and_occluded_box():
    rng = np.random.default_rng(2024)
    st = R.Stream(K, 8)
    person = (60, 40, 99, 199)
    for f in range(5):
        frame = CC.textured(H, W, rng)
        box = (person[0] + 3 * f, person[1], person[2] + 3 * f, person[3])
        CC.paint_person(frame, box, "red", "blue", rng)
        code, u, r = st.process([1], [box], [0], frame, f)
        assert code == 0 and st.label(1) == ("red", "blue"), f
        assert R.NAMES[u[0][9][R.UPPER][0]] == "red" and R.NAMES[u[0][9][R.LOWER][0]] == "blue"
    # a red box, 60 % of it behind a nearer yellow one
    frame = CC.textured(H, W, rng)
    red, yellow = (200, 50, 249, 149), (200, 60, 229, 170)                     # the yellow box covers columns 200..229 of 200..249
    CC.paint(frame, red, "red", rng)
    CC.paint(frame, yellow, "yellow", rng)
    for skip, want in ((1, "red"), (0, "yellow")):
        s2 = R.Stream(R.Cfg(skip_occluded=skip), 8)
        s2.process([1, 2], [red, yellow], [0, 0], frame, 0)
        assert R.NAMES[R.label(s2.rows[1].hist, R.WHOLE)[0]] == want, skip
        assert s2.label(2) == ("yellow", "yellow")


# ---- the rule header through a stand-alone program -------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("colour_rule_check_san" if sanitize else "colour_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built colour_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def walk_cases():
    """(h, w, pitch, base, seed, max_side, skip, inset, top, bottom, boxes).  With inset 0 and bottom 1000 a box that covers the frame is
    sampled up to the frame's last pixel, whose last byte is the buffer's last byte."""
    crowd = [(q, (2 + q, 1, 30 + q, 20 + q)) for q in range(11)]
    return [(37, 70, 211, 1, 1, 48, 1, 200, 150, 900, [(4, (0, 0, 69, 36)), (2, (10, 5, 40, 36)), (9, (30, 10, 80, 50))]),
            (37, 70, 210, 0, 2, 256, 1, 0, 0, 1000, [(1, (40, 10, 69, 40)), (3, (-5, -5, 20, 20)), (5, (5, 5, 5, 5)), (6, (90, 90, 99, 99)), (0, (0, 0, 69, 36))]),
            (37, 70, 211, 3, 8, 256, 0, 0, 0, 1000, [(1, (-9, -9, 99, 99))]),
            (36, 72, 216, 0, 3, 8, 1, 200, 150, 900, [(1, (0, 0, 71, 39)), (2, (20, 0, 60, 44))]),
            (36, 72, 216, 4, 4, 48, 0, 200, 150, 900, [(1, (0, 0, 71, 39)), (2, (20, 0, 60, 44))]),
            (30, 50, 150, 0, 5, 48, 1, 200, 150, 900, crowd),
            (1, 1, 3, 0, 6, 48, 1, 0, 0, 1000, [(1, (0, 0, 0, 0))]),
            (200, 260, 780, 0, 7, 48, 1, 200, 150, 900, [(1, (5, 5, 255, 199))])]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_colour_rule_header_equals_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    rng = np.random.default_rng(77)
    lines, want = [], []
    px = [p for ps in CC.NAME_LITERALS.values() for p in ps] + [tuple(v) for v in rng.integers(0, 256, (3000, 3)).tolist()] + [(200, 71, 168)]
    px += [tuple(reversed(p)) for p in bright_pixels().values()][::3]
    for r, g, b in px:
        lines.append(f"n {b} {g} {r}")
        want.append(str(R.name_int(K, b, g, r)))
    boxes = [c[0] for c in CC.PLANS] + [tuple(v) for v in (rng.integers(-60, 400, (300, 4)) + rng.random((300, 4))).tolist()]
    for q, xyxy in enumerate(boxes):
        k = K if q < len(CC.PLANS) else R.Cfg(inset_x_pm=int(rng.integers(0, 500)), top_pm=int(rng.integers(0, 300)), split_pm=int(rng.integers(300, 600)),
                                              bottom_pm=int(rng.integers(600, 1001)), max_side=int(rng.integers(1, 257)))
        lines.append("p " + " ".join(repr(float(np.float32(v))) for v in xyxy) + f" {H} {W} {k.inset_x_pm} {k.top_pm} {k.split_pm} {k.bottom_pm} {k.max_side}")
        P = R.plan(k, xyxy, H, W)
        want.append("0" if P is None else "1 " + " ".join(str(v) for v in (*P["raw"], *P["box"], *P["rect"], P["ys"], P["sx"], P["sy"], P["nx"], P["ny"])))
    for q in range(300):
        row = rng.integers(0, int(rng.choice([2, 50, 1 << 24])), 24)
        if q % 3 == 0:
            row[rng.integers(0, 24, 12)] = 0
        if q % 5 == 0:
            row[rng.integers(0, 24)] = row.max()                 # ties
        lines.append("l " + " ".join(str(int(v)) for v in row))
        want.append(" ".join(" ".join(str(v) for v in R.label(row.tolist(), p)) for p in range(3)))
    for q in range(300):
        row = rng.integers(0, int(rng.choice([5, (1 << 24) // 6, (1 << 24) // 3])), 24)
        fr = rng.integers(0, int(rng.choice([2, 100])), 24)
        ms = int(rng.choice([0, 16, int(fr.sum()), int(fr.sum()) + 1]))
        lines.append(f"a {ms} " + " ".join(str(int(v)) for v in row) + " " + " ".join(str(int(v)) for v in fr))
        r2 = row.tolist()
        added = R.accumulate(r2, fr.tolist(), ms)
        want.append(f"{int(added)} " + " ".join(str(v) for v in r2))
    for h, w, pitch, base, seed, max_side, skip, inset, top, bottom, tracks in walk_cases():
        lines.append(f"w {h} {w} {pitch} {base} {seed} {max_side} {skip} {inset} {top} {bottom} {len(tracks)} " + " ".join(f"{t} " + " ".join(str(v) for v in b) for t, b in tracks))
        buf = lcg_bytes(base + (h - 1) * pitch + 3 * w, seed)
        fr = np.stack([buf[base + y * pitch:base + y * pitch + 3 * w] for y in range(h)]).reshape(h, w, 3)
        k = R.Cfg(max_side=max_side, skip_occluded=skip, inset_x_pm=inset, top_pm=top, bottom_pm=bottom)
        if bottom == 1000 and skip == 0:
            assert R.plan(k, tracks[0][1], h, w)["rect"] == (0, 0, w - 1, h - 1)              # the last pixel is sampled
        plans, ids = [R.plan(k, b, h, w) for _, b in tracks], [t for t, _ in tracks]
        cells = []
        for i in range(len(tracks)):
            if plans[i] is None:
                cells.append("| x")
            else:
                hist, fl = R.frame_hist(k, fr, plans, ids, i)
                cells.append(f"| {fl} " + " ".join(str(v) for v in hist))
        want.append(" ".join(cells))
    assert any("| 2 " in w_ for w_ in want[-len(walk_cases()):])                   # the crowd reaches the cap of 8
    extra = ["n 256 0 0", "n 0 -1 0", "p 0 0 9 9 240 320 500 150 500 900 48", "p 0 0 9 9 240 320 200 500 500 900 48", "p 0 0 9 9 240 320 200 150 500 1001 48",
             "p 0 0 9 9 240 320 200 150 500 900 0", "p 0 0 9 9 240 320 200 150 500 900 257", "p 0 0 9 9 0 320 200 150 500 900 48", "a -1 " + " ".join(["0"] * 48),
             "w 4 8 23 0 1 48 1 200 150 900 0", "w 4 8 24 0 1 48 2 200 150 900 0", "w 0 8 24 0 1 48 1 200 150 900 0", "w 4 8 24 0 1 48 1 500 150 900 0"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(want) + len(extra) + 1 and got[-1] == f"done {len(want) + len(extra)}"
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert g_ == w_, (lines[i][:200], g_[:300], w_[:300])
    assert got[len(want):-1] == ["bad"] * len(extra)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]


# ---- the library: the host-only entry points, defaults, refusals, exports -------------------------------------------------------------------
def default_cfg(pkg):
    cfg = pkg._ffi.ColourCfg()
    pkg._ffi.lib().rtmodt_colour_default_cfg(C.byref(cfg))
    return cfg


def test_defaults_are_the_restatements(pkg):
    cfg = default_cfg(pkg)
    for f in ("black_max", "chroma_min", "sat_split", "sat_hi_pm", "sat_lo_pm", "y_black", "y_white", "pink_mx", "red_brown_mx", "orange_brown_mx",
              "yellow_brown_mx", "inset_x_pm", "top_pm", "split_pm", "bottom_pm", "max_side", "skip_occluded", "min_samples", "retire_after"):
        assert getattr(cfg, f) == getattr(K, f), f
    assert tuple(cfg.hue) == K.hue and cfg.device == 0 and cfg.n_classes == 0 and not cfg.classes
    assert (cfg.inset_x_pm, cfg.top_pm, cfg.split_pm, cfg.bottom_pm, cfg.max_side, cfg.min_samples, cfg.retire_after) == (200, 150, 500, 900, 48, 16, 30)
    assert pkg.events.colours.NAMES == R.NAMES and pkg.events.ColourAttributes is pkg.ColourAttributes


def test_name_and_plan_entry_points_equal_restatement(pkg):
    L = pkg._ffi.lib()
    cfg = default_cfg(pkg)
    rng = np.random.default_rng(31)
    px = [tuple(reversed(p)) for ps in CC.NAME_LITERALS.values() for p in ps] + [tuple(v) for v in rng.integers(0, 256, (2000, 3)).tolist()] + [(168, 71, 200)]
    assert [L.rtmodt_colour_name(b, g, r, C.byref(cfg)) for b, g, r in px] == [R.name_int(K, b, g, r) for b, g, r in px]
    out = pkg._ffi.ColourPlan()
    for xyxy, want in CC.PLANS:
        box = np.float32(xyxy)
        assert L.rtmodt_colour_plan(C.byref(cfg), pkg._ffi.ptr(box), H, W, C.byref(out)) == 0
        got = None if not out.sampled else (tuple(out.raw), tuple(out.box), tuple(out.rect), out.split_row, out.sx, out.sy, out.nx, out.ny)
        assert got == want, xyxy
    cfg.max_side, cfg.inset_x_pm = 8, 0
    for xyxy in (rng.integers(-60, 400, (200, 4)) + rng.random((200, 4))).tolist():
        box = np.float32(xyxy)
        assert L.rtmodt_colour_plan(C.byref(cfg), pkg._ffi.ptr(box), H, W, C.byref(out)) == 0
        P = R.plan(R.Cfg(max_side=8, inset_x_pm=0), box, H, W)
        assert (None if not out.sampled else (tuple(out.raw), tuple(out.box), tuple(out.rect), out.split_row, out.sx, out.sy, out.nx, out.ny)) == flat(P)


REFUSED = [("black_max", 257), ("chroma_min", -1), ("sat_split", 257), ("sat_hi_pm", 1001), ("sat_lo_pm", -1), ("y_black", 200), ("y_white", 257),
           ("pink_mx", -1), ("red_brown_mx", 257), ("orange_brown_mx", 257), ("yellow_brown_mx", -1), ("inset_x_pm", 500), ("inset_x_pm", -1), ("top_pm", -1),
           ("top_pm", 500), ("split_pm", 900), ("bottom_pm", 1001), ("max_side", 0), ("max_side", 257), ("skip_occluded", 2), ("min_samples", -1),
           ("min_samples", 65537), ("retire_after", -1)]


def test_every_refusal_without_a_device(pkg):
    L, E = pkg._ffi.lib(), pkg._ffi.E_INVALID
    h = C.c_void_p()
    out = pkg._ffi.ColourPlan()
    box = np.float32([0, 0, 9, 9])
    for field, v in REFUSED:
        cfg = default_cfg(pkg)
        setattr(cfg, field, v)
        assert L.rtmodt_colour_create(C.byref(cfg), 1, 4, C.byref(h)) == E and not h.value, field
        assert field.split("_")[0] in L.rtmodt_last_error().decode(), (field, L.rtmodt_last_error())
        assert L.rtmodt_colour_plan(C.byref(cfg), pkg._ffi.ptr(box), H, W, C.byref(out)) == E, field
        if field not in ("retire_after",):
            assert L.rtmodt_colour_name(1, 2, 3, C.byref(cfg)) == E, field
    for k, v in ((0, 65), (3, 298), (7, 1537)):                                # the hue bounds ascend within 0..1536
        cfg = default_cfg(pkg)
        cfg.hue[k] = v if k != 0 else 193
        assert L.rtmodt_colour_create(C.byref(cfg), 1, 4, C.byref(h)) == E and "hue" in L.rtmodt_last_error().decode()
    cfg = default_cfg(pkg)
    few = (C.c_int32 * 1)(0)
    cfg.classes, cfg.n_classes = few, 257
    assert L.rtmodt_colour_create(C.byref(cfg), 1, 4, C.byref(h)) == E
    cfg = default_cfg(pkg)
    for s, m in ((0, 4), (4097, 4), (1, 0), (1, 4097)):
        assert L.rtmodt_colour_create(C.byref(cfg), s, m, C.byref(h)) == E and not h.value
    assert L.rtmodt_colour_create(None, 1, 4, C.byref(h)) == E and L.rtmodt_colour_create(C.byref(cfg), 1, 4, None) == E
    for b, g, r in ((256, 0, 0), (0, -1, 0), (0, 0, 300)):
        assert L.rtmodt_colour_name(b, g, r, C.byref(cfg)) == E
    assert L.rtmodt_colour_name(0, 0, 0, None) == E
    assert L.rtmodt_colour_plan(C.byref(cfg), pkg._ffi.ptr(box), 0, W, C.byref(out)) == E and L.rtmodt_colour_plan(C.byref(cfg), pkg._ffi.ptr(box), H, 16385, C.byref(out)) == E
    assert L.rtmodt_colour_plan(None, pkg._ffi.ptr(box), H, W, C.byref(out)) == E and L.rtmodt_colour_plan(C.byref(cfg), None, H, W, C.byref(out)) == E
    for fn in ("state", "reset", "last_ms"):                                   # a null handle is refused, not followed
        args = {"state": (None, 0, None, None), "reset": (None, 0), "last_ms": (None, None)}[fn]
        assert getattr(L, f"rtmodt_colour_{fn}")(*args) == E
    assert L.rtmodt_colour_load(None, 0, None, 0) == E
    L.rtmodt_colour_destroy(None)
    with pytest.raises(ValueError, match="unknown threshold"):
        pkg.ColourAttributes(thresholds={"nope": 1})


def test_exports(pkg):
    L = pkg._ffi.lib()
    declared = [s for s in pkg._ffi.header_symbols() if s.startswith("rtmodt_colour_")]
    assert len(declared) == 15 and all(hasattr(L, s) and s in L._signatures for s in declared)
    assert C.sizeof(pkg._ffi.ColourRow) == 208 == pkg.events.colours.ROW_DTYPE.itemsize and C.sizeof(pkg._ffi.ColourLabel) == 20
    for f, (_, off) in pkg.events.colours.ROW_DTYPE.fields.items():
        assert getattr(pkg._ffi.ColourRow, f).offset == off, f


def test_create_on_a_device_that_cannot_exist(pkg):
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        pkg.ColourAttributes(max_tracks=1, device=1 << 20)
    assert e.value.code == pkg._ffi.E_HIP and "hipSetDevice" in e.value.msg
