"""CPU: the lens corrector's rules without a GPU.  ``tests/lens_ref.py`` (the restatement the table and the kernel of
``csrc/lens.hip`` are pinned to) against hand-worked literals and against geometry it does not itself define; ``csrc/lens_model.h``
against the restatement through ``tests/native/lens_model_check.cpp``, a stand-alone program built plain and with the address /
undefined-behaviour sanitizers (nothing is loaded into Python under a sanitizer); the host-only entry points
``rtmodt_lens_build_map`` / ``quantise_map`` / ``distort_points`` / ``undistort_points`` against the restatement, exactly; the
point round trip; the two NumPy helpers."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_cases as LC  # noqa: E402
import lens_ref as R  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "lens_model_check.cpp")


def b64(v):
    return struct.pack(">d", float(v)).hex()


def b32(v):
    return struct.pack(">f", np.float32(v)).hex()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- 1. literals
def test_identity_lens_literals():
    h, w = 5, 7
    lens = R.Lens(64.0, 32.0, 3.0, 2.0)                                        # powers of two: (u - cx) / fx * fx + cx is exact anyway
    qx, qy, outside = R.build_model(lens, (h, w))
    assert np.array_equal(qx, np.tile(32 * np.arange(w), (h, 1))) and np.array_equal(qy, np.tile(32 * np.arange(h)[:, None], (1, w)))
    assert not outside.any()
    src = np.random.default_rng(1).integers(0, 256, (h, w, 3), np.uint8)
    assert np.array_equal(R.sample(src, (qx, qy, outside), border=(9, 9, 9)), src)


def test_half_pixel_shift_literals():
    h, w = 2, 4
    src = np.zeros((h, w, 3), np.uint8)
    src[0, :, 0] = [10, 20, 0, 255]
    src[1, :, 0] = [7, 8, 100, 3]
    src[..., 1] = 200
    src[..., 2] = src[..., 0]
    v, u = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    table = R.build_from_map(u + 0.5, v, (h, w))
    assert np.array_equal(table[0], np.tile(32 * np.arange(w) + 16, (h, 1))) and not table[2].any()
    out = R.sample(src, table, border=(50, 60, 70))
    # ax = 16, ay = 0: weights 512, 512, 0, 0.  (10, 20): (512 * 30 + 512) >> 10 = 15872 >> 10 = 15 = (10 + 20 + 1) >> 1.
    # (0, 255): (130560 + 512) >> 10 = 131072 >> 10 = 128.  (7, 8): (7680 + 512) >> 10 = 8192 >> 10 = 8.
    assert out[0, 0, 0] == 15 and out[0, 2, 0] == 128 and out[1, 0, 0] == 8
    assert out[0, 1, 0] == (20 + 0 + 1) >> 1 == 10 and out[1, 1, 0] == (8 + 100 + 1) >> 1 == 54
    assert (out[..., 1][:, :3] == 200).all()
    # the last column blends with the border: (255 + 50 + 1) >> 1, (3 + 50 + 1) >> 1; green (200 + 60 + 1) >> 1; red (255 + 70 + 1) >> 1
    assert out[0, 3].tolist() == [153, 130, 163] and out[1, 3].tolist() == [27, 130, 37]


def test_map_off_the_picture_is_all_border():
    oh, ow = 3, 5
    mx, my = np.full((oh, ow), -5.0, np.float32), np.full((oh, ow), 1.0, np.float32)
    table = R.build_from_map(mx, my, (4, 6))
    assert table[2].sum() == oh * ow and not table[0].any() and not table[1].any()
    out = R.sample(np.full((4, 6, 3), 77, np.uint8), table, border=(1, 2, 3))
    assert (out == np.array([1, 2, 3], np.uint8)).all()
    # a position exactly on the last pixel centre is inside; one step of 1 / 32 before the first pixel still blends; a whole pixel before does not
    t = R.build_from_map(np.float32([[5.0, -1 / 32, -1.0, 5.0 + 1 / 32, 6.0]]), np.float32([[0, 0, 0, 0, 0]]), (4, 6))
    assert t[2].tolist() == [[0, 0, 1, 0, 1]] and t[0].tolist() == [[160, -1, 0, 161, 0]]


# ---------------------------------------------------------------------------------------------------------------- 2. geometry
def model_plain(lens, u, v):
    """The lens model written a second time: plain Python floats, powers instead of Horner, OpenCV's textbook form."""
    m = lens.resolved()
    k1, k2, p1, p2, k3, k4, k5, k6 = m.k
    x, y = (u - m.ncx) / m.nfx, (v - m.ncy) / m.nfy
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return m.fx * xd + m.cx, m.fy * yd + m.cy


@pytest.mark.parametrize("name", R.LENSES)
def test_ramp_follows_the_model(name):
    """A source that is the integer-rounded ramp I = a sx + b sy + c comes out as the ramp at the model's position, within
    1 + (|a| + |b|) / 64 levels: the source rounding (+-0.5) survives a convex blend, bilinear sampling of a ramp is exact, the
    position is quantised to +-1/64 px per axis (|a| / 64 + |b| / 64 levels), and the final rounding adds +-0.5."""
    a, b, c = 2.0, -1.5, 75.0
    src_size, out_size = (48, 64), (40, 72)
    ys, xs = np.meshgrid(np.arange(48.0), np.arange(64.0), indexing="ij")
    ramp = np.rint(a * xs + b * ys + c)
    assert ramp.min() >= 0 and ramp.max() <= 255
    src = np.repeat(ramp.astype(np.uint8)[..., None], 3, 2)
    lens = R.lens_for(name, src_size, out_size, zoom=0.8)
    qx, qy, outside = R.build_model(lens, src_size, out_size)
    out = R.sample(src, (qx, qy, outside), border=(0, 0, 0))
    x0, y0 = qx >> 5, qy >> 5
    whole = (outside == 0) & (x0 >= 0) & (x0 + 1 < 64) & (y0 >= 0) & (y0 + 1 < 48)              # all four taps on the source: no border in the blend
    assert whole.sum() > 1000 and outside.sum() > 0
    bound = 1 + (abs(a) + abs(b)) / 64
    worst = 0.0
    for v, u in zip(*np.nonzero(whole)):
        sx, sy = model_plain(lens, float(u), float(v))
        worst = max(worst, abs(float(out[v, u, 0]) - (a * sx + b * sy + c)))
    print(f"{name}: {int(whole.sum())} pixels, worst {worst:.4f} levels, bound {bound:.4f}")
    assert worst <= bound


# ---------------------------------------------------------------------------------------------------------------- 3. the header
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("lens_model_check_san" if sanitize else "lens_model_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built lens_model_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def table_line(table):
    qx, qy, o = table
    return f"{int(o.sum())}  " + " ".join(f"{a} {b} {c}" for a, b, c in zip(qx.ravel().tolist(), qy.ravel().tolist(), o.ravel().tolist()))


def lens_bits(lens):
    return " ".join(b64(v) for v in lens.as_list())


def sample_case():
    rng = np.random.default_rng(3)
    sh, sw, border = 5, 6, 201
    src = rng.integers(0, 256, (sh, sw, 1), np.uint8)
    qx = rng.integers(-80, 32 * sw + 48, 200).astype(np.int32)
    qy = rng.integers(-80, 32 * sh + 48, 200).astype(np.int32)
    want = R.sample(src, (qx[None], qy[None], np.zeros((1, 200), np.uint8)), border=(border,))[0, :, 0]
    line = f"s {sh} {sw} {border} 200 " + " ".join(str(int(t)) for t in src.ravel()) + " " + " ".join(f"{a} {b}" for a, b in zip(qx, qy))
    return line, " ".join(str(int(v)) for v in want)


@pytest.fixture(scope="module")
def header_cases():
    lines, want = [], []
    for _, lens, (sh, sw), (oh, ow) in R.table_cases():
        lines.append(f"m {sh} {sw} {oh} {ow} {lens_bits(lens)}")
        want.append(table_line(R.build_model(lens, (sh, sw), (oh, ow))))
    for limit in (0.0, 0.55):                                                                   # r2_limit cuts the fold-back off
        lines.append(f"m 23 37 19 41 {lens_bits(R.fold_lens(limit))}")
        want.append(table_line(R.build_model(R.fold_lens(limit), (23, 37), (19, 41))))
    mx, my = R.hostile_map()
    lines.append("c 23 37 19 41 " + " ".join(f"{b32(x)} {b32(y)}" for x, y in zip(mx.ravel(), my.ravel())))
    want.append(table_line(R.build_from_map(mx, my, (23, 37))))
    for lens, x, y in R.point_cases():
        d = R.distort_points(lens, [[x, y]])[0]
        lines.append(f"d {lens_bits(lens)} {b64(x)} {b64(y)}")
        want.append(f"{b64(d[0])} {b64(d[1])}")
        p, r = R.undistort_points(lens, [[x, y]])
        lines.append(f"u {lens_bits(lens)} {b64(x)} {b64(y)}")
        want.append(f"{b64(p[0, 0])} {b64(p[0, 1])} {b64(r[0])}")
    bad = R.Lens(1000.0, 1000.0, 959.5, 539.5, (-2.0,))                                           # does not converge: inf / nan inside
    for x, y in ((0.0, 0.0), (1919.0, 1079.0), (959.5, 539.5)):
        p, r = R.undistort_points(bad, [[x, y]])
        lines.append(f"u {lens_bits(bad)} {b64(x)} {b64(y)}")
        want.append(f"{b64(p[0, 0])} {b64(p[0, 1])} {b64(r[0])}")
    line, w = sample_case()
    lines.append(line)
    want.append(w)
    for c in LC.CASES:                                                                          # past one tile, and the largest extents
        (sh, sw), (oh, ow) = c.src, c.out
        if c.lens is not None:
            lines.append(f"m {sh} {sw} {oh} {ow} {lens_bits(c.lens)}")
        else:
            lines.append(f"c {sh} {sw} {oh} {ow} " + " ".join(f"{b32(x)} {b32(y)}" for x, y in zip(c.map[0].ravel(), c.map[1].ravel())))
        want.append(table_line(LC.table(c.name)))
    return lines, want


def header_subset(lines, want, sanitize):
    """The sanitised program gets every case but max_height (16384 rows of 3 pixels add nothing a sanitizer can see that max_width's 3
    rows of 16384 do not); the plain one gets all."""
    if not sanitize:
        return lines, want
    skip = len(lines) - len(LC.CASES) + [c.name for c in LC.CASES].index("max_height")
    assert lines[skip].startswith("m 16384 3 16384 3 ")
    return lines[:skip] + lines[skip + 1:], want[:skip] + want[skip + 1:]


def nan_insensitive(line):
    """Bit patterns of NaNs differ between NumPy and the FPU (sign, payload): every NaN reads 'nan'."""
    out = []
    for tok in line.split():
        if len(tok) == 16 and (int(tok, 16) & 0x7ff0000000000000) == 0x7ff0000000000000 and int(tok, 16) & 0xfffffffffffff:
            tok = "nan"
        out.append(tok)
    return " ".join(out)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_lens_model_header_equals_restatement(tmp_path, header_cases, sanitize):
    lines, want = header_subset(*header_cases, sanitize)
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) + 1 and got[-1] == f"done {len(lines)}"
    for k, w in enumerate(want):
        assert nan_insensitive(got[k]) == nan_insensitive(w), (lines[k][:200], got[k][:400], w[:400])
    hostile = want[len(R.table_cases()) + 2].split()
    assert 0 < int(hostile[0]) < 19 * 41                                     # the hostile map has both kinds of pixel


# ---------------------------------------------------------------------------------------------------------------- 4. the library, host only
def test_library_tables_equal_restatement(pkg):
    L = pkg.ingestion.lens
    for name, lens, src, out in R.table_cases():
        got = L.build_map(lens.K, lens.k, src, out, lens.new_K, lens.r2_limit)
        want = R.build_model(lens, src, out)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
    n_out = []
    for limit in (0.0, 0.55):                                                                   # r2_limit cuts the fold-back off
        fold = R.fold_lens(limit)
        got, want = L.build_map(fold.K, fold.k, (23, 37), (19, 41), fold.new_K, limit), R.build_model(fold, (23, 37), (19, 41))
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        n_out.append(int(want[2].sum()))
    assert 0 < n_out[0] < n_out[1] < 19 * 41
    mx, my = R.hostile_map()
    assert all(np.array_equal(g, w) for g, w in zip(L.quantise_map(mx, my, (23, 37)), R.build_from_map(mx, my, (23, 37))))
    # dist of 4 and 5 coefficients; new_K None copies K
    l4 = R.Lens(30.0, 31.0, 18.0, 11.0, (-0.2, 0.03, 0.002, -0.001))
    assert all(np.array_equal(g, w) for g, w in zip(L.build_map(l4.K, l4.k[:4], (23, 37)), R.build_model(l4, (23, 37))))
    assert all(np.array_equal(g, w) for g, w in zip(L.build_map(np.array([[30.0, 0, 18.0], [0, 31.0, 11.0], [0, 0, 1]]), l4.k[:5], (23, 37)), R.build_model(l4, (23, 37))))


def test_library_points_equal_restatement(pkg):
    L = pkg.ingestion.lens
    for name in R.LENSES:
        cases = [c for c in R.point_cases() if c[0].k == tuple(float(v) for v in R.COEFFS[name])]
        lens, xy = cases[0][0], np.array([[c[1], c[2]] for c in cases])
        assert np.array_equal(bits(L.distort_points(xy, lens.K, lens.k, lens.new_K)), bits(R.distort_points(lens, xy))), name
        got, res = L.undistort_points(xy, lens.K, lens.k, lens.new_K)
        want, wres = R.undistort_points(lens, xy)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(res), bits(wres)), name
        assert np.array_equal(bits(pkg.ingestion.LensCorrector.undistort_points(xy, lens.K, lens.k, lens.new_K)[0]), bits(want))


def test_library_refuses_bad_focal_lengths_and_sizes(pkg):
    L, E = pkg.ingestion.lens, pkg._ffi.E_INVALID
    for K in ((0.0, 30, 1, 1), (30, -1.0, 1, 1), (float("nan"), 30, 1, 1), (30, float("inf"), 1, 1)):
        with pytest.raises(pkg._ffi.RtmodtError, match="focal") as e:
            L.build_map(K, [0, 0, 0, 0], (4, 4))
        assert e.value.code == E
        with pytest.raises(pkg._ffi.RtmodtError, match="focal"):
            L.undistort_points([[1.0, 2.0]], K, [0, 0, 0, 0])
    with pytest.raises(pkg._ffi.RtmodtError, match="focal"):
        L.build_map((30, 30, 1, 1), [0, 0, 0, 0], (4, 4), new_K=(-30, 30, 1, 1))
    for src, out in (((0, 4), (4, 4)), ((4, 16385), (4, 4)), ((4, 4), (16385, 4)), ((4, 4), (4, 0))):
        with pytest.raises(pkg._ffi.RtmodtError, match="outside 1..16384") as e:
            L.build_map((30, 30, 1, 1), [0, 0, 0, 0], src, out)
        assert e.value.code == E
    with pytest.raises(ValueError, match="4, 5 or 8"):
        L.build_map((30, 30, 1, 1), [0, 0, 0], (4, 4))


# ---------------------------------------------------------------------------------------------------------------- 5. point round trip
def test_point_round_trip_residual():
    grid = R.grid_1080()
    for name in R.LENSES:
        lens = R.lens_1080(name)
        rect, res = R.undistort_points(lens, grid)
        worst = float(res.max())
        print(f"{name}: worst residual {worst:.3e} px over {len(grid)} points (bound {R.RESIDUAL_BOUND_PX:.3e})")
        assert worst <= R.RESIDUAL_BOUND_PX, name
        assert np.abs(R.distort_points(lens, rect) - grid).max() <= R.RESIDUAL_BOUND_PX, name   # the residual is what it says it is


def test_library_round_trip_residual(pkg):
    grid = R.grid_1080()
    for name in R.LENSES:
        lens = R.lens_1080(name)
        _, res = pkg.ingestion.lens.undistort_points(grid, lens.K, lens.k)
        assert float(res.max()) <= R.RESIDUAL_BOUND_PX, name


def test_non_invertible_lens_says_so(pkg):
    """k1 = -2 folds the picture back long before the corners: no rectified point maps there, and the residual reports it."""
    bad = R.Lens(R.F_1080, R.F_1080, 959.5, 539.5, (-2.0,))
    corners = np.array([[0.0, 0.0], [1919.0, 0.0], [0.0, 1079.0], [1919.0, 1079.0]])
    assert (R.undistort_points(bad, corners)[1] > 1.0).all()
    assert (pkg.ingestion.lens.undistort_points(corners, bad.K, bad.k)[1] > 1.0).all()
    assert R.undistort_points(bad, [[959.5, 539.5]])[1][0] == 0.0                          # the axis itself is fine


# ---------------------------------------------------------------------------------------------------------------- 6. helpers
def test_fisheye_map_helper(pkg):
    fisheye_map = pkg.ingestion.fisheye_map
    K, D = (300.0, 310.0, 320.0, 240.0), (0.05, -0.01, 0.002, -0.0003)
    mx, my = fisheye_map(K, D, K, (481, 641))
    assert mx.dtype == np.float32 and mx.shape == (481, 641)
    assert mx[240, 320] == 320.0 and my[240, 320] == 240.0                                    # the centre pixel maps to (cx, cy)
    # mirrored K (cx -> w - 1 - cx): the map is the mirror image
    Km = (300.0, 310.0, 640 - 320.0, 240.0)
    mxm, mym = fisheye_map(Km, D, Km, (481, 641))
    assert np.allclose(mxm, 640 - mx[:, ::-1], atol=1e-3) and np.allclose(mym, my[:, ::-1], atol=1e-3)
    # barrel-like: the corner reads closer to the centre than the pinhole would
    assert mx[0, 0] > 0 and my[0, 0] > 0
    mx2, _ = fisheye_map(K, D, None, (481, 641))
    assert np.array_equal(mx2, mx)
    with pytest.raises(ValueError):
        fisheye_map(K, (0.1, 0.2), K, (4, 4))


def test_monotonic_r2_helper(pkg):
    monotonic_r2 = pkg.ingestion.monotonic_r2
    step = 1e-3
    assert abs(monotonic_r2([-0.3, 0, 0, 0], step=step) - 1 / (3 * 0.3)) <= step                # d/dr r (1 + k1 r^2) = 0 at r^2 = -1 / (3 k1)
    assert monotonic_r2([0.25, 0.05, 0, 0]) == 0.0                                               # pincushion grows throughout
    assert abs(monotonic_r2([-2.0, 0, 0, 0], step=1e-4) - 1 / 6) <= 1e-4
