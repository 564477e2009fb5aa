"""CPU: the stabiliser's rules without a GPU.  ``tests/stab_ref.py`` (the restatement the kernels of ``csrc/stab.hip`` are pinned to)
against hand-worked literals, against a float64 bilinear warp it does not itself define, and against the closed form of the decay;
``csrc/stab_rule.h`` against the restatement through ``tests/native/stab_rule_check.cpp``, a stand-alone program built plain and
with the address / undefined-behaviour sanitizers (nothing is loaded into Python under a sanitizer); the host-only entry points
``rtmodt_stab_step`` / ``rtmodt_stab_points`` against the restatement, exactly; the point round trip; and the condition on the
inputs of the GPU motion-gate test: the raw shaking frames are MOTION, the restatement's stabilised frames are STILL."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmc_ref as G  # noqa: E402
import motion_ref as M  # noqa: E402
import stab_cases as SC  # noqa: E402
import stab_ref as S  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "stab_rule_check.cpp")


def b64(v):
    return struct.pack(">d", float(v)).hex()


def b32(v):
    return struct.pack(">f", np.float32(v)).hex()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- 1. literals
def test_identity_literals():
    r = S.Rule(5, 7)
    path, hold, status = S.step(r, S.IDENTITY, 0, S.IDENTITY_WARP, True)
    assert path == (1.0, 0.0, 0.0, 0.0) and hold == 0 and status == S.OK
    assert S.step(r, S.IDENTITY, 0, None, True) == (S.IDENTITY, 0, S.OK)
    assert S.quantise(r, path) == (65536, 0, 0, 0)
    qx, qy = S.positions((65536, 0, 0, 0), 5, 7)
    assert np.array_equal(qx, np.tile(32 * np.arange(7), (5, 1))) and np.array_equal(qy, np.tile(32 * np.arange(5)[:, None], (1, 7)))
    src = np.random.default_rng(1).integers(0, 256, (5, 7, 3), np.uint8)
    assert np.array_equal(S.sample(src, (65536, 0, 0, 0), (9, 9, 9)), src)


def test_integer_translation_literals():
    r = S.Rule(5, 7, leak_shift=0)
    path, hold, status = S.step(r, S.IDENTITY, 0, np.float32([1, 0, 3, 0, 1, -2]), True)
    # cx = 3, cy = 2: wtx = ((1 x 3 - 0 x 2) + 3) - 3 = 3, wty = ((0 x 3 + 1 x 2) - 2) - 2 = -2; U = ((3 + 3) - 3) + 0 = 3, V = ((-2 + 2) - 0) - 2 = -2
    assert path == (1.0, 0.0, 3.0, -2.0) and status == S.OK
    assert S.quantise(r, path) == (65536, 0, 3 * 65536, -2 * 65536)
    src = np.random.default_rng(2).integers(0, 256, (5, 7, 3), np.uint8)
    out = S.sample(src, S.quantise(r, path), (1, 2, 3))
    want = np.empty_like(src)
    want[...] = (1, 2, 3)
    want[2:, :4] = src[:3, 3:]                                                # out(x, y) = src(x + 3, y - 2)
    assert np.array_equal(out, want)


def test_small_rotation_literals():
    """a = 1, b = 2^-6 about the pixel origin of a 9 x 5 frame (cx = 4, cy = 2), no decay: wtx = ((4 - 2^-5) + 0) - 4 = -2^-5, wty = ((2^-4 +
    2) + 0) - 2 = 2^-4; J = (1, 2^-6, -2^-5, 2^-4); U = ((-2^-5 + 4) - 4) + 2^-6 x 2 = 0, V = ((2^-4 + 2) - 2^-6 x 4) - 2 = 0: the
    rotation about the pixel origin that W is.  A = 65536, B = 1024.  Pixel (8, 4): X = 65536 x 8 - 1024 x 4 = 520192, qx = 521216 >>
    11 = 254 (254.5 floored); Y = 1024 x 8 + 65536 x 4 = 270336, qy = 271360 >> 11 = 132 (132.5 floored)."""
    r = S.Rule(5, 9, leak_shift=0)
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([1, -2.0 ** -6, 0, 2.0 ** -6, 1, 0]), True)
    assert path == (1.0, 2.0 ** -6, -2.0 ** -5, 2.0 ** -4) and status == S.OK
    assert S.affine(r, path) == (1.0, 2.0 ** -6, 0.0, 0.0)
    coef = S.quantise(r, path)
    assert coef == (65536, 1024, 0, 0)
    qx, qy = S.positions(coef, 5, 9)
    assert (qx[4, 8], qy[4, 8]) == (254, 132) and (qx[0, 0], qy[0, 0]) == (0, 0)
    assert (qx[0, 8], qy[0, 8]) == (256, (1024 * 8 + 1024) >> 11) == (256, 4) and (qx[4, 0], qy[4, 0]) == ((-4096 + 1024) >> 11, 128) == (-2, 128)
    # pixel (8, 4) blends taps x0 = 7 (weight 2) and 8 (30), y0 = 4 (28) and 5 (off the source, 4): (2 x 28 x 10 + 30 x 28 x 200 + 32 x 4 x 50 + 512) >> 10
    src = np.zeros((5, 9, 1), np.uint8)
    src[4, 7], src[4, 8] = 10, 200
    assert S.sample(src, coef, (50,))[4, 8, 0] == (2 * 28 * 10 + 30 * 28 * 200 + 32 * 4 * 50 + 512) >> 10 == 171


def test_decay_step_literals():
    r = S.Rule(5, 7, leak_shift=1)                                            # k = 0.5
    path, hold, status = S.step(r, (1.03125, 0.015625, 8.0, -4.0), 0, None, True)
    assert path == (1.015625, 0.0078125, 4.0, -2.0) and (hold, status) == (0, S.OK)


def test_each_clamp_literals():
    r = S.Rule(5, 7, leak_shift=0, max_shift_px=4)
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([1, 0, 10, 0, 1, -10]), True)
    assert path == (1.0, 0.0, 4.0, -4.0) and status == S.CLAMPED
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([1, 0, 4, 0, 1, -4]), True)
    assert path == (1.0, 0.0, 4.0, -4.0) and status == S.OK                  # on the limit is inside it
    r = S.Rule(1, 1, leak_shift=0)                                            # cx = cy = 0: the translation stays 0
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([1, -0.0625, 0, 0.0625, 1, 0]), True)
    assert path == (1.0, 35.0 / 1000.0, 0.0, 0.0) and status == S.CLAMPED
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([1, 0.0625, 0, -0.0625, 1, 0]), True)
    assert path == (1.0, -(35.0 / 1000.0), 0.0, 0.0) and status == S.CLAMPED
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([1.25, 0, 0, 0, 1.25, 0]), True)
    assert path == (1.0 + 50.0 / 1000.0, 0.0, 0.0, 0.0) and status == S.CLAMPED
    path, _, status = S.step(r, S.IDENTITY, 0, np.float32([0.75, 0, 0, 0, 0.75, 0]), True)
    assert path == (1.0 - 50.0 / 1000.0, 0.0, 0.0, 0.0) and status == S.CLAMPED


def test_hold_run_up_to_reset_literals():
    r = S.Rule(5, 7, leak_shift=1, reset_after=3)
    path, hold = (1.0, 0.0, 8.0, -4.0), 0
    seen = []
    for valid, W in ((False, None), (True, np.float32([1, 0, np.nan, 0, 1, 0])), (True, np.float32([0, 0, 0, 0, 0, 0])), (False, None), (True, None)):
        path, hold, status = S.step(r, path, hold, W, valid)
        seen.append((path, hold, status))
    # an invalid flag, a NaN and a singular warp all count as the identity: the path only decays
    assert seen[0] == ((1.0, 0.0, 4.0, -2.0), 1, S.HOLD) and seen[1] == ((1.0, 0.0, 2.0, -1.0), 2, S.HOLD)
    assert seen[2] == (S.IDENTITY, 0, S.RESET)
    assert seen[3] == (S.IDENTITY, 1, S.HOLD) and seen[4] == (S.IDENTITY, 0, S.OK)
    r0 = S.Rule(5, 7, leak_shift=0, reset_after=0)                            # 0: never
    path, hold = (1.0, 0.0, 8.0, -4.0), 0
    for k in range(40):
        path, hold, status = S.step(r0, path, hold, None, False)
        assert (path, hold, status) == ((1.0, 0.0, 8.0, -4.0), k + 1, S.HOLD)


# ---------------------------------------------------------------------------------------------------------------- 2. an independent warp
RAMP = (7, 8, 0)                                                              # I = 7 x + 8 y: integers, so a bilinear blend of it is the ramp itself
RAMP_SIZE = (17, 17)                                                          # 7 x 16 + 8 x 16 = 240 <= 255


def ramp_errors(sample_fn):
    """Worst |bytes - ramp at the float64 position| over the pixels whose taps all lie on the source, for several paths -> (worst, count)."""
    h, w = RAMP_SIZE
    a, b, c = RAMP
    ys, xs = np.mgrid[0:h, 0:w]
    src = np.repeat((a * xs + b * ys + c).astype(np.uint8)[..., None], 3, 2)
    r = S.Rule(h, w, leak_shift=0, crop_zoom_milli=1250)
    cx, cy, z = (w - 1) / 2, (h - 1) / 2, 1.25
    worst, count = 0.0, 0
    for path in ((1.0, 0.0, 0.3, -0.7), (1.01, 0.02, 1.37, 0.61), (0.97, -0.03, -0.55, 1.9), (1.04, 0.035, 0.015625, -0.984375)):
        out = sample_fn(src, S.quantise(r, path), r).astype(np.float64)[..., 0]
        za, zb, tx, ty = path
        px = cx + (za * (xs - cx) - zb * (ys - cy)) / z + tx                  # the textbook form, written here and nowhere else
        py = cy + (zb * (xs - cx) + za * (ys - cy)) / z + ty
        inner = (px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2)
        assert inner.sum() > 100
        worst = max(worst, float(np.abs(out - (a * px + b * py + c))[inner].max()))
        count += int(inner.sum())
    return worst, count


def ramp_bound():
    """The source is an integer ramp, so a bilinear blend with exact weights IS the ramp at the sampled position.  What is left:
    rule 7 rounds the position to the nearest 1 / 32 pixel, at most 1 / 64 pixel per axis; rule 6 rounds A, B, U, V to Q16, at most
    2^-17 each, which moves the position by at most ((w - 1) + (h - 1) + 1) 2^-17 pixel per axis at the largest coordinate; the ramp
    turns a move of (ex, ey) into |a| ex + |b| ey levels; the 5-bit weights multiply exactly and (sum + 512) >> 10 rounds the blend by
    at most 0.5.  The float64 arithmetic on either side contributes below 1e-9."""
    h, w = RAMP_SIZE
    a, b, _ = RAMP
    return 0.5 + (abs(a) + abs(b)) * (1.0 / 64 + (w + h - 1) / 2.0 ** 17) + 1e-9


def test_sampler_follows_a_float64_warp_and_two_defects_do_not():
    bound = ramp_bound()
    worst, count = ramp_errors(lambda src, coef, r: S.sample(src, coef))
    print(f"restatement: {count} pixels, worst {worst:.4f} levels, bound {bound:.4f}")
    assert worst <= bound

    def no_rounding(src, coef, r):                                            # defect 1: the + 1024 is missing, positions are floored
        A, B, U, V = coef
        y, x = np.mgrid[0:r.h, 0:r.w].astype(np.int64)
        return S.LR.sample(src, ((A * x - B * y + U) >> 11, (B * x + A * y + V) >> 11, np.zeros((r.h, r.w), np.int64)))

    def b_flipped(src, coef, r):                                              # defect 2: B with the wrong sign
        A, B, U, V = coef
        return S.sample(src, (A, -B, U, V))

    for name, fn in (("missing + 1024", no_rounding), ("B with the wrong sign", b_flipped)):
        w2, _ = ramp_errors(fn)
        print(f"{name}: worst {w2:.4f} levels")
        assert w2 > bound, name


# ---------------------------------------------------------------------------------------------------------------- 3. decay, points
@pytest.mark.parametrize("leak_shift", [1, 3, 6, 16])
def test_decay_follows_the_closed_form(leak_shift):
    """After an excursion and with zero input, tx is multiplied by k once per call (wtx = (cx + 0) - cx = 0 exactly, and a x tx' - b x
    ty' + 0 = tx' exactly for a = 1, b = 0): n roundings of 2^-53 relative each, and k^n itself carries up to n more."""
    r = S.Rule(77, 131, leak_shift=leak_shift, max_shift_px=32)
    path, hold, status = S.step(r, S.IDENTITY, 0, np.float32([1, 0, 21.3, 0, 1, -17.9]), True)
    assert status == S.OK
    tx0, ty0 = path[2], path[3]
    k = 1.0 - 2.0 ** -leak_shift
    for n in range(1, 41):
        path, hold, status = S.step(r, path, hold, None, True)
        assert status == S.OK and path[0] == 1.0 and path[1] == 0.0
        tol = 2 * n * 2.0 ** -53
        assert abs(path[2] - k ** n * tx0) <= tol * abs(tx0) and abs(path[3] - k ** n * ty0) <= tol * abs(ty0), n


def test_points_round_trip():
    """to_stable(to_source(p)) = p within rounding: the forward map is about 8 operations on numbers up to Mag = (sa + |sb|) (|x| + |y|) +
    |U| + |V|, each within 2^-53 relative; the inverse multiplies that error by at most (sa + |sb|) / d with d = sa^2 + sb^2 and adds as many
    operations of its own.  The limits give sa + |sb| <= (1 + Z + R) / z and d >= ((1 - Z) / z)^2, so the error is at most 32 x 2^-53 x Mag x
    z (1 + Z + R) / (1 - Z)^2."""
    rng = np.random.default_rng(3)
    for crop in (1000, 1300):
        r = S.Rule(1080, 1920, max_rot_milli=500, max_zoom_milli=500, crop_zoom_milli=crop)
        Z, R, z = 0.5, 0.5, crop / 1000.0
        for _ in range(200):
            path = (1.0 + rng.uniform(-Z, Z), rng.uniform(-R, R), rng.uniform(-32, 32), rng.uniform(-32, 32))
            assert S.path_ok(r, path)
            x, y = rng.uniform(-100, 2100), rng.uniform(-100, 1200)
            sa, sb, U, V = S.affine(r, path)
            mag = (abs(sa) + abs(sb)) * (abs(x) + abs(y)) + abs(U) + abs(V)
            bound = 32 * 2.0 ** -53 * mag * z * (1 + Z + R) / (1 - Z) ** 2
            X, Y = S.point(r, path, True, x, y)
            bx, by = S.point(r, path, False, X, Y)
            assert abs(bx - x) <= bound and abs(by - y) <= bound, (path, x, y, bx - x, by - y, bound)
    r = S.Rule(5, 7, leak_shift=0)
    assert S.point(r, (1.0, 0.0, 3.0, -2.0), True, 1.0, 2.0) == (4.0, 0.0) and S.point(r, (1.0, 0.0, 3.0, -2.0), False, 4.0, 0.0) == (1.0, 2.0)


# ---------------------------------------------------------------------------------------------------------------- 4. the header
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("stab_rule_check_san" if sanitize else "stab_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built stab_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def rule_words(r):
    return f"{r.h} {r.w} {r.leak_shift} {r.max_shift_px} {r.max_rot_milli} {r.max_zoom_milli} {r.crop_zoom_milli} {r.reset_after}"


def path_words(path):
    return " ".join(b64(v) for v in path)


def rules():
    out = [S.Rule(h, w, **SC.CFG) for h, w in SC.SHAPES.values()]
    out += [S.Rule(77, 131, crop_zoom_milli=1100, **SC.CFG), S.Rule(1080, 1920), S.Rule(23, 37, leak_shift=0, reset_after=0), S.Rule(16384, 16384, 16, 16384, 500, 500, 8000, 2)]
    return out


@pytest.fixture(scope="module")
def header_cases():
    """(stdin lines, expected stdout lines) over the step sequences of every stream of stab_cases.schedule under several rules, points
    in both directions, and sampled bytes of the small shapes."""
    lines, want = [], []
    sched = SC.schedule()
    for r in rules():
        for s in range(SC.N_STREAMS):
            path, hold, words, res = S.IDENTITY, 0, [], []
            for k, (warps, valid) in enumerate(sched):
                has = not (s == 0 and k == 5)                                 # one call without a warp: the identity
                words.append(f"{int(valid[s])} {int(has)} " + " ".join(b32(v) for v in warps[s]))
                path, hold, status = S.step(r, path, hold, warps[s] if has else None, valid[s])
                res.append(f"{status} {hold} {path_words(path)} " + " ".join(str(v) for v in S.quantise(r, path)))
            lines.append(f"t {rule_words(r)} {path_words(S.IDENTITY)} 0 {len(sched)} " + " ".join(words))
            want.append("  ".join(res))
    rng = np.random.default_rng(8)
    paths = [(1.0, 0.0, 0.0, 0.0), (1.01, 0.0125, 3.7, -2.2), (0.985, -0.02, -11.5, 7.25), (1.03, 0.02, 12.0, -12.0)]
    for r in rules()[:5]:
        for path in paths:
            for to_source in (1, 0):
                x, y = rng.uniform(-50, 2000), rng.uniform(-50, 1200)
                lines.append(f"p {rule_words(r)} {path_words(path)} {to_source} {b64(x)} {b64(y)}")
                want.append(" ".join(b64(v) for v in S.point(r, path, bool(to_source), x, y)))
    for name in ("37x23", "1x1", "523x9"):
        h, w = SC.SHAPES[name]
        src = rng.integers(0, 256, (h, w, 1), np.uint8)
        for crop in (1000, 1100):
            r = S.Rule(h, w, crop_zoom_milli=crop, **SC.CFG)
            for path in paths:
                lines.append(f"s {rule_words(r)} {path_words(path)} 93 " + " ".join(str(v) for v in src.ravel()))
                want.append(" ".join(str(v) for v in S.sample(src, S.quantise(r, path), (93,)).ravel()))
    return lines, want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_stab_rule_header_equals_restatement(tmp_path, header_cases, sanitize):
    lines, want = header_cases
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) + 1 and got[-1] == f"done {len(lines)}"
    for k, w in enumerate(want):
        assert got[k] == w, (lines[k][:200], got[k][:400], w[:400])
    statuses = {int(part.split()[0]) for w in want[:len(rules()) * SC.N_STREAMS] for part in w.split("  ")}
    assert statuses == {S.OK, S.HOLD, S.CLAMPED, S.RESET}                     # the sequences reach every status


def test_schedule_reaches_what_it_is_for():
    r = S.Rule(77, 131, **SC.CFG)
    seen = {s: [] for s in range(SC.N_STREAMS)}
    clamped = {s: set() for s in range(SC.N_STREAMS)}
    path, hold = [S.IDENTITY] * SC.N_STREAMS, [0] * SC.N_STREAMS
    M_, R_, Z_ = float(r.max_shift_px), r.max_rot_milli / 1000.0, r.max_zoom_milli / 1000.0
    for warps, valid in SC.schedule():
        for s in range(SC.N_STREAMS):
            path[s], hold[s], status = S.step(r, path[s], hold[s], warps[s], valid[s])
            seen[s].append(status)
            za, zb, tx, ty = path[s]
            clamped[s] |= {n for n, hit in (("shift", abs(tx) == M_ or abs(ty) == M_), ("rot", abs(zb) == R_), ("zoom", abs(za - 1.0) == Z_ or za == 1.0 + Z_)) if hit}
    assert set(seen[0]) == {S.OK}
    assert S.CLAMPED in seen[1] and {"shift", "rot"} <= clamped[1]
    assert seen[2][3:7] == [S.HOLD, S.HOLD, S.HOLD, S.RESET] and seen[2][-1] == S.OK
    assert S.CLAMPED in seen[3] and "zoom" in clamped[3]


# ---------------------------------------------------------------------------------------------------------------- 5. the host entry points
def test_host_entry_points_equal_restatement(pkg):
    st = pkg.ingestion.stabilizer
    for r in rules()[:6]:
        cfg = st.make_cfg((r.h, r.w), leak_shift=r.leak_shift, max_shift_px=r.max_shift_px, max_rot_milli=r.max_rot_milli, max_zoom_milli=r.max_zoom_milli,
                          crop_zoom_milli=r.crop_zoom_milli, reset_after=r.reset_after)
        for s in range(SC.N_STREAMS):
            path, hold = S.IDENTITY, 0
            j, jh = np.float64(S.IDENTITY), 0
            for warps, valid in SC.schedule():
                path, hold, status = S.step(r, path, hold, warps[s], valid[s])
                j, jh, jstatus, coef = st.rule_step(cfg, j, jh, warps[s], valid[s])
                assert np.array_equal(bits(j), bits(path)) and (jh, jstatus) == (hold, status) and tuple(int(v) for v in coef) == S.quantise(r, path)
            pts = np.random.default_rng(s).uniform(-50, 1500, (16, 2))
            for to_source in (True, False):
                got = st.map_points(cfg, path, pts, to_source)
                want = np.float64([S.point(r, path, to_source, x, y) for x, y in pts])
                assert np.array_equal(bits(got), bits(want))
    E = pkg._ffi.RtmodtError
    for kw in (dict(leak_shift=17), dict(max_shift_px=-1), dict(max_rot_milli=501), dict(max_zoom_milli=501), dict(crop_zoom_milli=999), dict(reset_after=-1)):
        with pytest.raises(E) as e:
            st.rule_step(st.make_cfg((5, 7), **kw), S.IDENTITY, 0)
        assert e.value.code == pkg._ffi.E_INVALID and "bad parameter" in e.value.msg
    with pytest.raises(E) as e:
        st.map_points(st.make_cfg((0, 7)), S.IDENTITY, np.zeros((1, 2)), True)
    assert e.value.code == pkg._ffi.E_INVALID and "outside 1..16384" in e.value.msg


# ---------------------------------------------------------------------------------------------------------------- 6. the motion gate's inputs
def gate_statuses(frames):
    h, w = SC.GATE_SIZE
    ref = M.Ref(1, h, w, **SC.GATE_MOTION)
    return [ref.process([f])[0]["status"] for f in frames]


def test_shaking_camera_is_motion_raw_and_still_stabilised():
    """A condition on the chosen inputs of tests/test_gpu_stab.py's motion-gate case, established on the restatements alone."""
    frames, warps = SC.gate_frames(), SC.gate_warps()
    warm = SC.GATE_MOTION["warmup"]
    raw = gate_statuses(frames)
    assert raw[:warm] == [M.WARMUP] * warm and M.MOTION in raw[warm:], raw
    ref = S.Ref(1, SC.GATE_SIZE, **SC.GATE_STAB)
    stable = []
    for f, w in zip(frames, warps):
        stable.append(ref.process([f], [w])[0])
        assert ref.status[0] == S.OK
    got = gate_statuses(stable)
    assert got[:warm] == [M.WARMUP] * warm and got[warm:] == [M.STILL] * (len(frames) - warm), got
    assert all(np.array_equal(s, stable[0]) for s in stable)                  # integer shakes and no decay: the same picture every time


def test_estimator_case_is_status_ok_on_the_restatement():
    """The estimator form's frames at their small size: the restatement of gmc reports status 0 and the exact integer translation on
    every frame after the first, which is what the GPU test's exact-interior check rests on."""
    est = G.GmcRef(**SC.EST_CFG)
    frames = SC.est_frames()
    warp, status, _ = est.estimate(frames[0])
    assert status == G.FIRST
    for k, (sx, sy) in enumerate(SC.EST_STEPS):
        warp, status, _ = est.estimate(frames[k + 1])
        assert status == G.OK and np.array_equal(warp, np.float32([1, 0, -sx, 0, 1, -sy])), (k, status, warp)
