"""CPU: the speed estimator's rules without a GPU.  ``tests/speed_ref.py`` (the restatement the kernels of ``csrc/speed.hip`` are
pinned to) against hand-worked literal cases; the per-point rules of ``csrc/ground_plane.h`` against the restatement through
``tests/native/ground_plane_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer); the plane fit -- restatement, header and the host-only entry point
``rtmodt_speed_fit_plane`` -- against planes known by construction."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speed_ref as R  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "ground_plane_check.cpp")
SEC = 1_000_000


def run_case(case, **extra):
    ref = R.SpeedRef(case["plane"], max_tracks=64, **{**case["kwargs"], **extra})
    out = [ref.process(rows, t) for t, rows in case["calls"]]
    return ref, out


# ---------------------------------------------------------------------------------------------------------------- hand cases
def test_affine_walk_literals():
    case = R.HAND_CASES["affine_walk"]
    ref, out = run_case(case)
    assert [o[0][0]["world"] for o in out] == case["world"]
    assert [o[0][0]["speed_mm_s"] for o in out] == case["speeds"]
    assert [o[0][0]["odometer_mm"] for o in out] == case["odometer"]
    assert [(k, e["kind"], e["speed_mm_s"]) for k, o in enumerate(out) for e in o[1]] == case["events"]
    assert ref.hist == case["hist"]
    assert out[-1][0][0]["peak_mm_s"] == 500 and out[0][0][0]["flags"] == R.F_NEW and out[1][0][0]["flags"] == 0
    assert out[3][0][0]["heading"] == [150, 0] and out[0][0][0]["heading"] == [0, 0]
    assert out[2][1][0]["world_mm"] == [400, 1000] and out[2][1][0]["t_us"] == 200_000 and out[2][1][0]["class_id"] == 2


def test_head_on_literals():
    case = R.HAND_CASES["head_on"]
    ref, out = run_case(case)
    assert [(k, e["kind"], e["speed_mm_s"], e["track_id"]) for k, o in enumerate(out) for e in o[1]] == [(3, "wrong_way", 1000, 2)]
    assert {k: o[2] for k, o in enumerate(out) if o[2]} == case["pairs"]
    assert [r["speed_mm_s"] for r in out[4][0]] == [2000, 1000] and [r["odometer_mm"] for r in out[4][0]] == [4000, 2000]
    assert [r["world"] for r in out[2][0]] == [[1300, 1600], [1300, 2960]]


def test_perspective_points():
    for (u, v), want in R.PERSP_POINTS:
        assert R.project(R.PERSP_H, np.float32(u), np.float32(v)) == want, (u, v)
    assert R.anchor(R.FOOT, [1.0, 2.0, 4.0, 9.0]) == (2.5, 9.0) and R.anchor(R.CENTRE, [1.0, 2.0, 4.0, 9.0]) == (2.5, 5.5)
    assert R.anchor(R.FOOT, [float("nan"), 0, 1, 1]) is None and R.anchor(R.FOOT, [0, 0, float("inf"), 1]) is None
    assert R.anchor(R.FOOT, [3e38, 0, 3e38, 1]) is None                        # the float32 sum overflows
    case = R.HAND_CASES["perspective"]
    _, out = run_case(case)
    assert [r["world"] for r in out[0][0]] == case["first_call_world"] == [[750, 500000], [625, 750000], [313, 750000], [-312, 750000], [536870500, 500000]]
    assert [r["track_id"] for r in out[0][0]] == case["first_call_ids"] == [4, 5, 6, 7, 9] and [r["track"] for r in out[0][0]] == [3, 4, 5, 6, 8]
    ref = R.SpeedRef(R.PERSP_H, max_tracks=8)
    rows, _, _, _ = ref.process([(1, R.box(0.0, -600.0), 0), (2, R.box(0.75, 500.0), 0), (3, [float("nan"), 0, 1, 1], 0)], 0)
    assert [r["track_id"] for r in rows] == [2] and rows[0]["track"] == 1 and [r[0] for r in ref.snapshot()] == [2]     # not sampled, not clamped


def test_isqrt_and_speed_literals():
    for k in (0, 1, 2, 3, 255, 65535, 46341, 2 ** 30, 1518500249):
        for n in (k * k - 1, k * k, k * k + 1):
            if n >= 0:
                r = math.isqrt(n)
                assert r * r <= n < (r + 1) * (r + 1)
    assert math.isqrt(2 ** 61 - 1) == 1518500249 and math.isqrt(0) == 0 and math.isqrt(1) == 1 and math.isqrt(3) == 1 and math.isqrt(4) == 2
    assert R.speed_of(50, 100_000) == 500 and R.speed_of(100, 300_000) == 333 and R.speed_of(2 ** 31, 1) == R.INT32_MAX


# ---------------------------------------------------------------------------------------------------------------- ledger rules
def walk(ref, xs, dt=100_000, tid=1, t0=0):
    return [ref.process([(tid, R.box(x, 52.0), 0)], t0 + k * dt)[0:2] for k, x in enumerate(xs)]


def test_window_wraps_around():
    """window = 4 over 11 samples: the ring holds the last four, the chord starts at the oldest of them."""
    ref = R.SpeedRef(R.AFFINE_H, window=4, min_samples=2, max_tracks=8)
    xs = [0.5 * k * k for k in range(11)]                                      # accelerating: every chord differs
    out = walk(ref, xs)
    X = [int(20 * x + 100) for x in xs]
    for k in range(1, 11):
        o = max(0, k - 3)
        assert out[k][0][0]["speed_mm_s"] == (X[k] - X[o]) * SEC // ((k - o) * 100_000), k
        assert out[k][0][0]["n_samples"] == min(k + 1, 4)
    assert ref.snapshot()[0][2] == [[X[k], 1000, k * 100_000] for k in (7, 8, 9, 10)]


def test_each_alarm_rearms():
    # SPEEDING: limit 400, hold 2: fires on the 2nd fast sample, not again while fast, again after one slow sample and two fast ones
    ref = R.SpeedRef(R.AFFINE_H, window=2, hold=2, limit_mm_s=400, min_step_mm=0, max_tracks=8)
    xs = [0, 5, 10, 15, 15, 20, 25, 30]                                        # 100 mm per 100 ms = 1000 mm/s, one stop in the middle
    ev = [[e["kind"] for e in o[1]] for o in walk(ref, xs)]
    assert ev == [[], [], ["speeding"], [], [], [], ["speeding"], []]
    # STOPPED: below 100 mm/s for 200 ms; fires once, re-arms on motion, fires again
    ref = R.SpeedRef(R.AFFINE_H, window=2, stop_mm_s=100, stop_us=200_000, min_step_mm=0, max_tracks=8)
    xs = [0, 0, 0, 0, 0, 5, 5, 5, 5]
    ev = [[e["kind"] for e in o[1]] for o in walk(ref, xs)]
    assert ev == [[], [], [], ["stopped"], [], [], [], [], ["stopped"]]
    # WRONG_WAY: allowed +x, hold 2, at least 500 mm/s: fires on the 2nd backward sample, re-arms on a forward one
    ref = R.SpeedRef(R.AFFINE_H, window=2, hold=2, allowed_dir=(1, 0), wrong_way_min_mm_s=500, min_step_mm=0, max_tracks=8)
    xs = [50, 45, 40, 35, 40, 35, 30, 29.5, 29]                                # the last two: backwards but only 100 mm/s
    ev = [[e["kind"] for e in o[1]] for o in walk(ref, xs)]
    assert ev == [[], [], ["wrong_way"], [], [], [], ["wrong_way"], [], []]
    # everything off: no alarm at all
    ref = R.SpeedRef(R.AFFINE_H, window=2, max_tracks=8)
    assert all(o[1] == [] for o in walk(ref, [0, 50, 0, 50]))


def test_dead_band():
    """Jitter of 20 mm under min_step_mm = 30 never reaches the odometer; a slow creep does once it has moved 30 mm from the anchor."""
    ref = R.SpeedRef(R.AFFINE_H, min_step_mm=30, max_tracks=8)
    out = walk(ref, [10, 11, 10, 11, 10, 10.5, 11, 11.5, 12])                  # world x: 300 320 300 320 300 310 320 330 340
    assert [o[0][0]["odometer_mm"] for o in out] == [0, 0, 0, 0, 0, 0, 0, 30, 30]
    assert ref.snapshot()[0][4] == [330, 1000]
    ref = R.SpeedRef(R.AFFINE_H, min_step_mm=0, max_tracks=8)
    assert [o[0][0]["odometer_mm"] for o in walk(ref, [10, 11, 10, 11])] == [0, 20, 40, 60]


def test_drop_after_max_gap_and_time_must_increase():
    ref = R.SpeedRef(R.AFFINE_H, max_gap_us=300_000, min_step_mm=0, max_tracks=8)
    ref.process([(1, R.box(10, 52), 0), (2, R.box(20, 52), 0)], 0)
    ref.process([(1, R.box(11, 52), 0)], 100_000)
    rows, _, _, _ = ref.process([(1, R.box(12, 52), 0), (2, R.box(21, 52), 0)], 300_000)      # 2 returns after exactly max_gap: same row
    assert [r["n_samples"] for r in rows] == [3, 2] and rows[1]["odometer_mm"] == 20
    ref.process([(1, R.box(13, 52), 0)], 400_000)
    rows, _, _, _ = ref.process([(1, R.box(14, 52), 0), (2, R.box(22, 52), 0)], 601_000)      # 301 ms: dropped, starts fresh
    assert [r["n_samples"] for r in rows] == [5, 1] and rows[1]["odometer_mm"] == 0 and rows[1]["flags"] == R.F_NEW and rows[1]["speed_mm_s"] == -1
    ref.process([], 1_000_000)
    assert ref.snapshot() == []                                                # both rows expired with nobody in the list
    for t in (1_000_000, 999_999):
        with pytest.raises(AssertionError, match="t_us must increase"):
            ref.process([], t)


def test_histogram_last_bin_and_percentile(pkg):
    ref = R.SpeedRef(R.AFFINE_H, window=2, bins=3, bin_mm_s=500, min_step_mm=0, max_tracks=8)
    walk(ref, [0, 1, 2, 4.5, 7, 57, 157])                                      # 200 200 500 500 10000 20000 mm/s
    assert ref.hist == [2, 2, 2]                                               # 10000 and 20000 both land in the open-ended last bin
    assert R.percentile_of([2, 2, 2], 500, 50) == 1000 and R.percentile_of([2, 2, 2], 500, 33) == 500 and R.percentile_of([2, 2, 2], 500, 85) == math.inf
    assert R.percentile_of([0, 0, 0], 500, 85) is None and R.percentile_of([], 500, 85) is None
    h = [0, 3, 10, 40, 30, 12, 4, 1, 0]                                        # 100 samples: the 85th is the 85th smallest -> bin 5 (cumulative 95)
    assert R.percentile_of(h, 1000, 85) == 6000 and R.percentile_of(h, 1000, 83) == 5000 and R.percentile_of(h, 1000, 0) == 2000
    assert R.percentile_of(h, 1000, 100) == 8000
    P = pkg.events.speed.percentile_of
    for p in (0, 1, 33, 50, 83, 85, 99.5, 100):
        assert P(h, 1000, p) == R.percentile_of(h, 1000, p) and P([2, 2, 2], 500, p) == R.percentile_of([2, 2, 2], 500, p)


def test_class_filter_and_capacity():
    ref = R.SpeedRef(R.AFFINE_H, classes=(0, 2), max_tracks=2, max_gap_us=10 * SEC)
    rows, _, _, _ = ref.process([(1, R.box(1, 52), 0), (2, R.box(2, 52), 1), (3, R.box(3, 52), 2)], 0)
    assert [(r["track_id"], r["track"]) for r in rows] == [(1, 0), (3, 2)]
    ref.process([(4, R.box(1, 52), 0), (5, R.box(2, 52), 0)], 1)                # 4 rows: full
    assert not ref.ledger_overflow and len(ref.rows) == 4
    ref.process([(6, R.box(1, 52), 0)], 2)                                      # a fifth: the idle rows go
    assert ref.ledger_overflow and sorted(ref.rows) == [6]


def test_constant_velocity_against_the_truth():
    """A track moving at a constant world velocity on the perspective road plane: the estimate is within the derived bound of the truth.
    Two endpoint roundings move the chord by at most sqrt(2) mm (half a millimetre per axis and end), the floor root by less than
    1 mm, the floor division by less than 1 mm/s: |estimate - truth| <= (sqrt(2) + 1) * 1e6 / dt_us + 1."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for window, dt in ((2, 33_333), (8, 40_000), (32, 100_000)):
        for _ in range(20):
            p0 = np.array([rng.uniform(2000, 18000), rng.uniform(1000, 6000)])          # stays in front of the camera for the whole walk
            vel = np.array([rng.uniform(-3000, 3000), rng.uniform(200, 1500)])      # mm/s
            ref = R.SpeedRef(R.ROAD_H, window=window, min_step_mm=0, max_tracks=8)
            seen = []                                                          # (exact world point of the anchor the estimator saw, t)
            for k in range(window + 5):
                t = k * dt
                uv = R._inverse_project(R.ROAD_H, (p0 + vel * (t / 1e6))[None])[0]
                bx = np.float32([uv[0] - 10, uv[1] - 30, uv[0] + 10, uv[1]])
                au, av = R.anchor(R.FOOT, bx)                                  # a float32 pixel: the truth is the world point of THAT anchor
                seen.append((R.project64(R.ROAD_H, [[np.float64(au), np.float64(av)]])[0], t))
                rows, _, _, _ = ref.process([(1, bx, 0)], t)
                assert len(rows) == 1
                if rows[0]["speed_mm_s"] < 0:
                    continue
                (wa, ta), (wb, tb) = seen[-window:][0], seen[-1]
                truth = float(np.hypot(*(wb - wa))) * 1e6 / (tb - ta)
                bound = (math.sqrt(2) + 1) * 1e6 / (tb - ta) + 1
                err = abs(rows[0]["speed_mm_s"] - truth)
                worst = max(worst, err / bound)
                assert err <= bound, (window, dt, k, rows[0]["speed_mm_s"], truth, bound)
    print(f"constant velocity: worst |estimate - truth| / bound = {worst:.3f}")
    assert worst > 0.0


# ---------------------------------------------------------------------------------------------------------------- fit_plane
def residual_vs_truth(H, img, world):
    return float(np.sqrt(((R.project64(H, img) - world) ** 2).sum(axis=1)).max())


def lib_fit(pkg, img, world):
    H, res = np.zeros(9), C.c_double(0.0)
    a, b = np.ascontiguousarray(img, np.float64), np.ascontiguousarray(world, np.float64)
    rc = pkg._ffi.lib().rtmodt_speed_fit_plane(pkg._ffi.ptr(a), pkg._ffi.ptr(b), len(a), pkg._ffi.ptr(H), C.byref(res))
    return rc, H.reshape(3, 3), res.value


def test_fit_plane_recovers_constructed_planes(pkg):
    """Planes known by construction: the residual against the constructed truth, for the restatement and for the library's host-only
    entry point, stays within 8 x the measured figure; the same fit without the normalisation, on points crowded around (1900, 1000),
    misses that bound."""
    worst = 0.0
    for name, img, world in R.fit_cases():
        H, res = R.fit_plane(img, world)
        rc, HL, resL = lib_fit(pkg, img, world)
        assert rc == 0, name
        for who, h in (("restatement", H), ("library", HL)):
            e = residual_vs_truth(h, img, world)
            print(f"fit_plane {name} {who}: residual against the truth {e:.3e} mm")
            worst = max(worst, e)
            assert e <= R.FIT_RESIDUAL_BOUND_MM, (name, who, e)
        assert res <= R.FIT_RESIDUAL_BOUND_MM and resL <= R.FIT_RESIDUAL_BOUND_MM
        assert np.allclose(HL / HL[2, 2], R.ROAD_H, rtol=1e-9, atol=1e-9) and np.allclose(H / H[2, 2], R.ROAD_H, rtol=1e-9, atol=1e-9)
    print(f"fit_plane: largest residual {worst:.3e} mm (recorded {R.FIT_RESIDUAL_MEASURED_MM:.1e}, bound {R.FIT_RESIDUAL_BOUND_MM:.1e})")
    img, world = R.defect_case()
    good, bad = R.fit_plane(img, world), R.fit_plane(img, world, normalise=False)
    assert residual_vs_truth(good[0], img, world) <= R.FIT_RESIDUAL_BOUND_MM
    assert bad is not None and residual_vs_truth(bad[0], img, world) > R.FIT_RESIDUAL_BOUND_MM     # the defect misses the bound
    print(f"fit_plane defect: normalised {residual_vs_truth(good[0], img, world):.3e} mm, normalisation dropped {residual_vs_truth(bad[0], img, world):.3e} mm")


def test_fit_plane_refuses_degenerate_input(pkg):
    E = pkg._ffi.E_INVALID
    sq = [[0, 0], [100, 0], [100, 100], [0, 100]]
    assert lib_fit(pkg, sq[:3], sq[:3])[0] == E and R.fit_plane(sq[:3], sq[:3]) is None                       # n < 4
    col = [[0, 0], [50, 50], [100, 100], [100, 0]]                                                          # three collinear image points
    assert lib_fit(pkg, col, sq)[0] == E and R.fit_plane(col, sq) is None
    assert lib_fit(pkg, sq, col)[0] == E and R.fit_plane(sq, col) is None                                     # three collinear world points
    same = [[5, 5]] * 4
    assert lib_fit(pkg, same, sq)[0] == E and R.fit_plane(same, sq) is None
    nan = [[0, 0], [100, 0], [100, float("nan")], [0, 100]]
    assert lib_fit(pkg, nan, sq)[0] == E and R.fit_plane(nan, sq) is None
    rc, H, res = lib_fit(pkg, sq, [[0, 0], [2000, 0], [2000, 2000], [0, 2000]])                               # a plain scale: 20 mm per pixel
    assert rc == 0 and np.allclose(H, np.diag([20, 20, 1]), atol=1e-9) and res < 1e-9


# ---------------------------------------------------------------------------------------------------------------- the header
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("ground_plane_check_san" if sanitize else "ground_plane_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built ground_plane_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def b32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]


def b64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def from_b64(s):
    return struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]


def header_cases():
    rng = np.random.default_rng(30)
    lines, want = [], []
    nan, inf = float("nan"), float("inf")
    boxes = [[1, 2, 4, 9], [0.5, 0.25, 0.75, 7.125], [nan, 0, 1, 1], [0, 0, inf, 1], [3e38, 0, 3e38, 1], [0, 3e38, 1, 3e38], [-7.5, -1, -2.25, 1]]
    boxes += rng.uniform(-500, 2500, (40, 4)).tolist()
    for kind in (R.FOOT, R.CENTRE):
        for b in boxes:
            lines.append(f"a {kind} " + " ".join(b32(v) for v in b))
            uv = R.anchor(kind, b)
            want.append("none" if uv is None else f"{b32(uv[0])} {b32(uv[1])}")
    planes = [(R.PERSP_H, [p for p, _ in R.PERSP_POINTS]), (R.AFFINE_H, [(10.0, 52.0), (12.5, 0.5), (-3.5, 1e7), (2.7e7, 1.0), (-2.7e7, 1.0)]),
              (R.ROAD_H.reshape(9).tolist(), np.c_[rng.uniform(-200, 2200, 300), rng.uniform(-700, 1300, 300)].tolist()),
              ([1, 0, 0, 0, 1, 0, 0, 0, nan], [(1.0, 1.0)]), ([1, 0, 0, 0, 1, 0, 0, 0, inf], [(1.0, 1.0)]), ([inf, 0, 0, 0, 1, 0, 0, 0, 1], [(1.0, 1.0), (0.0, 1.0)])]
    for H, pts in planes:
        for u, v in pts:
            lines.append("p " + " ".join(b64(h) for h in H) + f" {b32(u)} {b32(v)}")
            got = R.project(H, np.float32(u), np.float32(v))
            want.append("off" if got is None else f"{got[0]} {got[1]}")
    ns = {0, 1, 2, 3, 2 ** 61 - 1, 2 ** 61 - 2, 2 ** 60, 2 * (2 ** 30) ** 2}
    for k in (2, 3, 255, 256, 65535, 65536, 46340, 46341, 2 ** 30, 2 ** 30 + 1, 1518500249, 3037000499):
        ns |= {k * k - 1, k * k, k * k + 1}
    ns |= {int(v) for v in rng.integers(0, 2 ** 61, 200)}
    for n in sorted(ns):
        lines.append(f"q {n}")
        want.append(str(math.isqrt(n)))
    for d, dt in [(50, 100_000), (100, 300_000), (0, 1), (2 ** 31, 1), (1518500249, 1), (1518500249, 10 ** 12), (2147, 1_000_000), (2148, 1000)] + \
            [(int(a), int(b)) for a, b in zip(rng.integers(0, 2 ** 31, 50), rng.integers(1, 10 ** 9, 50))]:
        lines.append(f"s {d} {dt}")
        want.append(str(R.speed_of(d, dt)))
    return lines, want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_ground_plane_header_equals_restatement(tmp_path, sanitize):
    lines, want = header_cases()
    fits = [(1, img, world, False) for _, img, world in R.fit_cases()] + [(1,) + R.defect_case() + (False,), (0,) + R.defect_case() + (False,)]
    sq = np.array([[0, 0], [100, 0], [100, 100], [0, 100]], float)
    fits += [(1, sq[:3], sq[:3], True), (1, np.array([[0, 0], [50, 50], [100, 100], [100, 0]], float), sq, True)]     # n < 4; three collinear
    for normalise, img, world, _ in fits:
        lines.append(f"f {normalise} {len(img)} " + " ".join(f"{b64(a[0])} {b64(a[1])} {b64(b[0])} {b64(b[1])}" for a, b in zip(img, world)))
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) + 1 and got[-1] == f"done {len(lines)}"
    for k, w in enumerate(want):
        assert got[k] == w, (lines[k], got[k], w)
    worst = 0.0
    for (normalise, img, world, refused), line in zip(fits, got[len(want):-1]):
        if refused:
            assert line == "bad"
            continue
        vals = [from_b64(s) for s in line.split()]
        e = residual_vs_truth(np.array(vals[:9]).reshape(3, 3), img, world)
        print(f"ground_plane_check fit n={len(img)} normalise={normalise}: residual against the truth {e:.3e} mm")
        if normalise:
            worst = max(worst, e)
            assert e <= R.FIT_RESIDUAL_BOUND_MM and vals[9] <= R.FIT_RESIDUAL_BOUND_MM
        else:
            assert e > R.FIT_RESIDUAL_BOUND_MM                                 # the normalisation dropped: misses the bound
    print(f"ground_plane_check: largest residual {worst:.3e} mm")
