"""CPU: the compositor's rules without a GPU.  ``tests/compose_ref.py`` (the restatement the kernel of ``csrc/compose.hip`` is pinned
to) against hand-worked literals and against resamplers it does not itself define -- the snapshot gallery's area average, the
oracle's cv::resize tables, Pillow's ``Image.reduce`` on power-of-two factors; the 4:2:0 round trip over the whole colour cube; two
deliberately wrong restatements that must differ on the GPU test's own inputs; ``csrc/compose_rule.h`` against the restatement
through ``tests/native/compose_rule_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour
sanitizers (nothing is loaded into Python under a sanitizer); the host-only checks of the C ABI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_cases as CC  # noqa: E402
import compose_ref as R  # noqa: E402
import snapshot_ref as SR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "compose_rule_check.cpp")


# ---------------------------------------------------------------------------------------------------------------- 1. literals
def test_shrink_4x2_to_2x1_literals():
    src = np.zeros((2, 4, 3), np.uint8)
    src[0, :, 0], src[1, :, 0] = [10, 20, 30, 40], [50, 60, 70, 81]
    src[..., 1], src[..., 2] = 255, src[..., 0] // 2
    # x: S 4 -> D 2, each destination covers two source pixels with weight 2; y: S 2 -> D 1, weight 1 each; T = 8.
    # (2 * (10 + 20 + 50 + 60) + 4) // 8 = 284 // 8 = 35; (2 * (30 + 40 + 70 + 81) + 4) // 8 = 446 // 8 = 55.
    out = R.resample(src, 1, 2)
    assert out[0, :, 0].tolist() == [35, 55] and out[0, :, 1].tolist() == [255, 255]
    # red: 5 10 15 20 / 25 30 35 40 -> (2 * 70 + 4) // 8 = 18, (2 * 110 + 4) // 8 = 28
    assert out[0, :, 2].tolist() == [18, 28]
    idx, w, tot = R.taps(4, 2)
    assert idx.tolist() == [[0, 1], [2, 3]] and w.tolist() == [[2, 2], [2, 2]] and tot == 4
    p = R.Plan((0, 0, 4, 2), (0, 0, 2, 1), R.SHRINK, R.SHRINK)
    assert [R.pixel(src, p, x, 0, 0) for x in range(2)] == [35, 55]


def test_enlarge_2_to_5_literals():
    # scale 0.4: positions -0.3, 0.1, 0.5, 0.9, 1.3 -> (0, 2048, 0), (0, 1843, 205), (0, 1024, 1024), (0, 205, 1843), (1, 2048, 0)
    ofs, c0, c1 = R.enlarge_table(5, 2)
    assert ofs.tolist() == [0, 0, 0, 0, 1] and c0.tolist() == [2048, 1843, 1024, 205, 2048] and c1.tolist() == [0, 205, 1024, 1843, 0]
    src = np.zeros((1, 2, 3), np.uint8)
    src[0, :, :] = [[100, 0, 255], [200, 0, 0]]
    out = R.resample(src, 1, 5)
    # (1843 * 100 + 205 * 200 + 1024) // 2048 = 226324 // 2048 = 110; (1024 * 300 + 1024) // 2048 = 150; (205 * 100 + 1843 * 200 + 1024) // 2048 = 190
    assert out[0, :, 0].tolist() == [100, 110, 150, 190, 200] and not out[..., 1].any()
    # 255 -> 0: (1843 * 255 + 1024) // 2048 = 229; (1024 * 255 + 1024) // 2048 = 128; (205 * 255 + 1024) // 2048 = 26
    assert out[0, :, 2].tolist() == [255, 229, 128, 26, 0]


def test_fit_with_bars_literals():
    # a 4 x 2 (w x h) source into the 6 x 6 rectangle at (1, 1): 4 * 6 >= 2 * 6, so the width fills and the height is (2 * 6 + 2) // 4 = 3,
    # centred at (6 - 3) // 2 = 1: the inner picture is (1, 2, 6, 3)
    cell = R.Cell(0, 0, (1, 1, 6, 6), fit=R.FIT, pad=(1, 2, 3))
    p = R.plan((2, 4), cell, False)
    assert p == R.Plan((0, 0, 4, 2), (1, 2, 6, 3), R.ENLARGE, R.ENLARGE)
    src = np.full((2, 4, 3), 77, np.uint8)
    out = R.compose([(2, 4)], [R.Output(8, 8, background=(9, 9, 9))], [cell], [src])[0]
    assert (out[2:5, 1:7] == 77).all() and (out[1, 1:7] == [1, 2, 3]).all() and (out[5:7, 1:7] == [1, 2, 3]).all()
    assert (out[0] == 9).all() and (out[7] == 9).all() and (out[:, 0] == 9).all() and (out[:, 7] == 9).all()
    # 4:2:0: an odd inner picture becomes even -- size up, origin down
    q = R.plan((30, 50), R.Cell(0, 0, (2, 4, 40, 30), fit=R.FIT), True)
    assert R.plan((30, 50), R.Cell(0, 0, (2, 4, 40, 30), fit=R.FIT), False).inner == (2, 7, 40, 24) and q.inner == (2, 6, 40, 24)
    q = R.plan((37, 53), R.Cell(0, 0, (2, 4, 40, 30), fit=R.FIT), True)
    assert R.plan((37, 53), R.Cell(0, 0, (2, 4, 40, 30), fit=R.FIT), False).inner == (2, 5, 40, 28) and q.inner == (2, 4, 40, 28)
    q = R.plan((10, 90), R.Cell(0, 0, (0, 0, 10, 10), fit=R.FIT), True)            # 10 x 1 -> 10 x 2 at y = 4
    assert R.plan((10, 90), R.Cell(0, 0, (0, 0, 10, 10), fit=R.FIT), False).inner == (0, 4, 10, 1) and q.inner == (0, 4, 10, 2)
    # FILL cuts the crop centrally: a 50 x 30 source into a square keeps 30 x 30 from x = 10
    assert R.plan((30, 50), R.Cell(0, 0, (0, 0, 8, 8), fit=R.FILL), False).crop == (10, 0, 30, 30)


# ---------------------------------------------------------------------------------------------------------------- 2. other resamplers
@pytest.mark.parametrize("src,dst", [((37, 53), (9, 16)), ((40, 64), (20, 32)), ((17, 300), (1, 7)), ((64, 3), (63, 1)), ((5, 5), (5, 4))])
def test_pure_shrinks_equal_the_snapshot_resampler(src, dst):
    img = CC.frame(src[0], src[1], 5)
    assert np.array_equal(R.resample(img, dst[0], dst[1]), SR.resample(img, dst[0], dst[1]))


@pytest.mark.parametrize("D,S", [(5, 2), (12, 5), (11, 4), (640, 360), (23, 10), (7, 1), (16384, 3), (100, 99)])
def test_enlarging_taps_equal_the_oracle(D, S):
    from oracle import yolo_oracle
    idx, a0, a1 = yolo_oracle._resize_coeffs(D, S)
    ofs, c0, c1 = R.enlarge_table(D, S)
    assert np.array_equal(ofs, idx) and np.array_equal(c0, a0) and np.array_equal(c1, a1)
    ti, tw, tot = R.taps(S, D)
    assert tot == 2048 and np.array_equal(ti[:, 0], idx) and np.array_equal(ti[:, 1], np.minimum(idx + 1, S - 1))
    assert (tw.sum(1) == 2048).all()


@pytest.mark.parametrize("fx,fy", [(2, 2), (4, 1), (2, 1), (1, 2), (16, 16)])
def test_power_of_two_factors_equal_pillow_reduce(fx, fy):
    """Pillow's ``Image.reduce`` is the box filter with one rounding; for factors whose product is a power of two its shift is exact
    and every byte is equal.  For other factors Pillow multiplies by a truncated reciprocal and is off by one ((3, 3), (2, 3)): a
    known difference, not asserted here."""
    from PIL import Image
    h, w = 6 * fy, 5 * fx
    img = CC.frame(h, w, 40 + fx + 3 * fy)
    want = np.asarray(Image.fromarray(img).reduce((fx, fy)))
    assert want.shape == (6, 5, 3)
    assert np.array_equal(R.resample(img, 6, 5), want)


# ---------------------------------------------------------------------------------------------------------------- 3. 4:2:0
def test_yuv_literals():
    assert (R.yuv_y(0, 0, 0), R.yuv_u(0, 0, 0), R.yuv_v(0, 0, 0)) == (16, 128, 128)
    assert (R.yuv_y(255, 255, 255), R.yuv_u(255, 255, 255), R.yuv_v(255, 255, 255)) == (235, 128, 128)
    assert (R.yuv_u(255, 0, 0), R.yuv_v(0, 0, 255)) == (240, 240)                  # pure blue / pure red
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 0], img[0, 1], img[1, 0], img[1, 1] = (10, 20, 30), (11, 20, 30), (12, 23, 30), (13, 20, 33)
    Y, U, V = R.to_yuv420(img)
    # block means: b (46 + 2) >> 2 = 12, g (83 + 2) >> 2 = 21, r (123 + 2) >> 2 = 31
    assert U[0, 0] == R.yuv_u(12, 21, 31) and V[0, 0] == R.yuv_v(12, 21, 31) and Y[1, 1] == R.yuv_y(13, 20, 33)


def test_yuv_round_trip_over_the_whole_cube():
    """Forward by the restatement, back by the restatement of csrc/preprocess.hip's conversion, on pictures that are constant on every
    2 x 2 block (so the block mean is the colour itself): within 2 / 1 / 2 levels of B / G / R, each bound attained; Y in 16..235,
    U and V in 16..240.  All 2^24 colours, one blue value at a time."""
    g, r = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst = np.zeros(3, np.int64)
    lo, hi = np.full(3, 255, np.int64), np.zeros(3, np.int64)
    for b in range(256):
        m = (np.full_like(g, b) * 4 + 2) >> 2, (g * 4 + 2) >> 2, (r * 4 + 2) >> 2
        Y, U, V = R.yuv_y(b, g, r), R.yuv_u(*m), R.yuv_v(*m)
        for k, a in enumerate((Y, U, V)):
            lo[k], hi[k] = min(lo[k], a.min()), max(hi[k], a.max())
        b2, g2, r2 = R.yuv_to_bgr(Y, U, V)
        worst = np.maximum(worst, [np.abs(b2 - b).max(), np.abs(g2 - g).max(), np.abs(r2 - r).max()])
    print("round trip worst |B G R|:", worst.tolist(), "Y U V min:", lo.tolist(), "max:", hi.tolist())
    assert worst.tolist() == [2, 1, 2]
    assert lo[0] >= 16 and hi[0] <= 235 and lo[1:].min() >= 16 and hi[1:].max() <= 240
    assert (lo[0], hi[0]) == (16, 235) and (lo[1], hi[1], lo[2], hi[2]) == (16, 240, 16, 240)


# ---------------------------------------------------------------------------------------------------------------- 4. discrimination
@pytest.mark.parametrize("name", CC.RESAMPLING)
def test_rounding_between_the_passes_differs_on_the_gpu_inputs(name):
    sources, outputs, cells, _ = CC.CASES[name]
    wrong = R.compose(sources, outputs, cells, list(CC.frames(name)), round_between=True)
    assert any(not np.array_equal(a, b) for a, b in zip(wrong, CC.expected(name))), "the inputs are too bland: change the inputs"


@pytest.mark.parametrize("name", CC.YUV)
def test_top_left_chroma_differs_on_the_gpu_inputs(name):
    _, outputs, _, _ = CC.CASES[name]
    differs = 0
    for o, img in zip(outputs, CC.expected(name)):
        if o.fmt == R.BGR24:
            continue
        _, U, V = R.to_yuv420(img)
        _, U2, V2 = R.to_yuv420(img, chroma_top_left=True)
        differs += int(not (np.array_equal(U, U2) and np.array_equal(V, V2)))
    assert differs == sum(o.fmt != R.BGR24 for o in outputs), "the inputs are too bland: change the inputs"


# ---------------------------------------------------------------------------------------------------------------- 5. the header, natively
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("compose_rule_check_san" if sanitize else "compose_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built compose_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def native_source(h, w, seed):
    i = np.arange(h * w * 3, dtype=np.int64)
    return ((i * 7919 + seed * 104729 + (i >> 3) * 31) % 251).astype(np.uint8).reshape(h, w, 3)


def plan_line(p):
    return " ".join(str(v) for v in (*p.crop, *p.inner, p.kind_x, p.kind_y))


@pytest.fixture(scope="module")
def header_cases():
    lines, want = [], []
    rng = np.random.default_rng(7)
    geoms = [((2, 4), (0, 0, 0, 0), (1, 1, 6, 6)), ((16384, 16384), (0, 0, 0, 0), (0, 0, 1, 1)), ((1, 1), (0, 0, 0, 0), (0, 0, 16384, 16384)),
             ((1080, 1920), (0, 0, 0, 0), (0, 0, 640, 360)), ((1080, 1920), (100, 50, 333, 777), (2, 2, 960, 540))]
    for _ in range(40):
        sh, sw = (int(v) for v in rng.integers(1, 400, 2))
        cw, ch = int(rng.integers(1, sw + 1)), int(rng.integers(1, sh + 1))
        crop = (int(rng.integers(0, sw - cw + 1)), int(rng.integers(0, sh - ch + 1)), cw, ch)
        geoms.append(((sh, sw), crop, (2 * int(rng.integers(0, 9)), 2 * int(rng.integers(0, 9)), 2 * int(rng.integers(1, 200)), 2 * int(rng.integers(1, 200)))))
    for (sh, sw), crop, rect in geoms:
        for fit in (R.STRETCH, R.FIT, R.FILL):
            for yuv in (0, 1):
                if yuv and any(v & 1 for v in rect):                 # a 4:2:0 output takes even rectangles only
                    continue
                lines.append(f"p {sh} {sw} {' '.join(map(str, crop))} {' '.join(map(str, rect))} {fit} {yuv}")
                want.append(plan_line(R.plan((sh, sw), R.Cell(0, 0, rect, crop, fit), bool(yuv))))
    pix = [((37, 53), (0, 0, 0, 0), (0, 0, 16, 9), R.STRETCH, 0), ((4, 5), (0, 0, 0, 0), (0, 0, 12, 11), R.STRETCH, 0), ((10, 40), (0, 0, 0, 0), (0, 0, 13, 23), R.STRETCH, 0),
           ((9, 33), (0, 0, 0, 0), (4, 2, 33, 9), R.STRETCH, 0), ((30, 50), (3, 2, 40, 27), (2, 4, 40, 30), R.FIT, 1), ((30, 50), (3, 2, 40, 27), (2, 4, 26, 16), R.FILL, 1),
           ((3, 16384), (0, 0, 0, 0), (0, 0, 1, 1), R.STRETCH, 0), ((300, 1100), (0, 0, 0, 0), (0, 0, 20, 5), R.STRETCH, 0), ((1, 1), (0, 0, 0, 0), (0, 0, 7, 5), R.STRETCH, 0)]
    for seed, ((sh, sw), crop, rect, fit, yuv) in enumerate(pix):
        p = R.plan((sh, sw), R.Cell(0, 0, rect, crop, fit), bool(yuv))
        cx, cy, cw, ch = p.crop
        img = R.resample(native_source(sh, sw, seed)[cy:cy + ch, cx:cx + cw], p.inner[3], p.inner[2])
        lines.append(f"x {sh} {sw} {' '.join(map(str, crop))} {' '.join(map(str, rect))} {fit} {yuv} {seed}")
        want.append(plan_line(p) + " " + " ".join(map(str, img.ravel().tolist())))
    for D, S in ((5, 2), (12, 5), (640, 360), (16384, 3), (7, 1)):
        ofs, c0, c1 = R.enlarge_table(D, S)
        lines.append(f"t {D} {S}")
        want.append(" ".join(f"{a} {b} {c}" for a, b, c in zip(ofs.tolist(), c0.tolist(), c1.tolist())))
    for b, g, r in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (17, 130, 201)] + rng.integers(0, 256, (30, 3)).tolist():
        lines.append(f"y {b} {g} {r}")
        want.append(f"{R.yuv_y(b, g, r)} {R.yuv_u(b, g, r)} {R.yuv_v(b, g, r)}")
    return lines, want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_compose_rule_header_equals_restatement(tmp_path, header_cases, sanitize):
    lines, want = header_cases
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) + 1 and got[-1] == f"done {len(lines)}"
    for k, w in enumerate(want):
        assert got[k].split() == w.split(), (lines[k][:200], got[k][:400], w[:400])


# ---------------------------------------------------------------------------------------------------------------- 6. the library, host only
def test_library_plans_equal_restatement(pkg):
    VC = pkg.visualization.compose
    for name, (sources, outputs, cells, _) in CC.CASES.items():
        plans = VC.plan_layout(sources, [VC.Output((o.h, o.w), o.fmt, o.background) for o in outputs],
                               [VC.Cell(c.output, c.source, c.rect, c.crop, c.fit, c.pad, c.offline) for c in cells])
        for c, got in zip(cells, plans):
            want = R.plan(sources[c.source], c, outputs[c.output].fmt != R.BGR24)
            assert (got.crop, got.inner, VC.KINDS.index(got.kind_x), VC.KINDS.index(got.kind_y)) == (want.crop, want.inner, want.kind_x, want.kind_y), name


def test_grid_and_point_mapping(pkg):
    VC = pkg.visualization.compose
    cells = VC.Compositor.grid_cells(8, (1080, 1920), cols=4)
    assert [c.rect for c in cells][:5] == [(0, 0, 480, 540), (480, 0, 480, 540), (960, 0, 480, 540), (1440, 0, 480, 540), (0, 540, 480, 540)]
    assert [c.source for c in cells] == list(range(8))
    plans = VC.plan_layout([(1080, 1920)] * 8, [VC.Output((1080, 1920))], cells)
    assert plans[5].inner == (480, 540 + 135, 480, 270) and plans[5].kind_x == "shrink"
    want = R.map_points(R.Plan(plans[5].crop, plans[5].inner, 0, 0), [[-0.5, -0.5], [1919.5, 1079.5], [959.5, 539.5]])
    assert np.allclose(want, [[479.5, 674.5], [959.5, 944.5], [719.5, 809.5]])


def _layout_rc(pkg, handle, sources, outputs, cells):
    VC = pkg.visualization.compose
    cs, co, cc = VC._c_layout(sources, outputs, cells)
    L = pkg._ffi.lib()
    rc = L.rtmodt_compose_set_layout(handle, cs, len(sources), co, len(outputs), cc, len(cells))
    rc2 = L.rtmodt_compose_plan(cs, len(sources), co, len(outputs), cc, len(cells), (pkg._ffi.ComposePlan * max(len(cells), 1))())
    return rc, rc2, L.rtmodt_last_error().decode()


def test_abi_refuses_before_the_first_hip_call(pkg):
    """Every refusal below is decided on the host, before the library touches a device: the same on a machine without a GPU."""
    F, VC, L = pkg._ffi, pkg.visualization.compose, pkg._ffi.lib()
    cfg = F.ComposeCfg()
    L.rtmodt_compose_default_cfg(C.byref(cfg))
    assert (cfg.max_sources, cfg.max_outputs, cfg.max_cells, cfg.max_dim) == (64, 16, 64, 16384)
    h = C.c_void_p()
    for field, bad in (("max_sources", 0), ("max_sources", 65), ("max_outputs", 17), ("max_cells", 65), ("max_dim", 16385), ("max_dim", 0), ("device", -1)):
        c = F.ComposeCfg.from_buffer_copy(cfg)
        setattr(c, field, bad)
        assert L.rtmodt_compose_create(C.byref(c), C.byref(h)) == F.E_INVALID and not h.value, field
        assert field.split("_")[-1] in L.rtmodt_last_error().decode()
    assert L.rtmodt_compose_create(None, C.byref(h)) == F.E_INVALID
    assert L.rtmodt_compose_create(C.byref(cfg), C.byref(h)) == F.OK and h.value
    try:
        O, K = VC.Output, VC.Cell
        ok_src, ok_out = [(10, 20)], [O((8, 8))]
        refusals = [
            ("65 sources", [(4, 4)] * 65, ok_out, [], F.E_CAPACITY, "sources"),
            ("17 outputs", ok_src, [O((4, 4))] * 17, [], F.E_CAPACITY, "outputs"),
            ("65 cells", ok_src, ok_out, [K(0, 0, (0, 0, 1, 1))] * 65, F.E_CAPACITY, "cells"),
            ("no source", [], ok_out, [], F.E_INVALID, "at least one"),
            ("empty source", [(0, 5)], ok_out, [], F.E_INVALID, "outside 1..16384"),
            ("huge source", [(5, 16385)], ok_out, [], F.E_INVALID, "outside 1..16384"),
            ("huge output", ok_src, [O((16385, 4))], [], F.E_INVALID, "outside 1..16384"),
            ("odd nv12", ok_src, [O((8, 7), "nv12")], [], F.E_INVALID, "even"),
            ("odd i420", ok_src, [O((7, 8), "i420")], [], F.E_INVALID, "even"),
            ("format", ok_src, [O((8, 8), 0)], [], None, ""),
            ("output index", ok_src, ok_out, [K(1, 0, (0, 0, 4, 4))], F.E_INVALID, "output 1"),
            ("source index", ok_src, ok_out, [K(0, -1, (0, 0, 4, 4))], F.E_INVALID, "source -1"),
            ("rect leaves", ok_src, ok_out, [K(0, 0, (5, 0, 4, 4))], F.E_INVALID, "leaves"),
            ("rect negative", ok_src, ok_out, [K(0, 0, (-1, 0, 4, 4))], F.E_INVALID, "leaves"),
            ("rect empty", ok_src, ok_out, [K(0, 0, (0, 0, 0, 4))], F.E_INVALID, "leaves"),
            ("odd rect on nv12", ok_src, [O((8, 8), "nv12")], [K(0, 0, (1, 0, 4, 4))], F.E_INVALID, "even"),
            ("crop leaves", ok_src, ok_out, [K(0, 0, (0, 0, 4, 4), crop=(10, 0, 11, 5))], F.E_INVALID, "crop"),
            ("crop negative", ok_src, ok_out, [K(0, 0, (0, 0, 4, 4), crop=(0, -1, 5, 5))], F.E_INVALID, "crop"),
            ("crop empty", ok_src, ok_out, [K(0, 0, (0, 0, 4, 4), crop=(1, 1, 0, 5))], F.E_INVALID, "crop"),
        ]
        for name, s, o, c, code, word in refusals:
            if code is None:
                continue
            rc, rc2, msg = _layout_rc(pkg, h, s, o, c)
            assert rc == code and rc2 == code and word in msg, (name, rc, rc2, msg)
        # unknown format / fit mode: through the structs, Python's own checks aside
        cs, co, cc = VC._c_layout(ok_src, ok_out, [K(0, 0, (0, 0, 4, 4))])
        co[0].pixel_format = 7
        assert L.rtmodt_compose_set_layout(h, cs, 1, co, 1, cc, 1) == F.E_INVALID and "pixel format 7" in L.rtmodt_last_error().decode()
        co[0].pixel_format, cc[0].fit = 0, 3
        assert L.rtmodt_compose_set_layout(h, cs, 1, co, 1, cc, 1) == F.E_INVALID and "fit mode 3" in L.rtmodt_last_error().decode()
        assert L.rtmodt_compose_set_layout(h, None, 1, co, 1, cc, 1) == F.E_INVALID
        # nothing was set: a run, a crop, an output and a time are refused, still without a device
        sp, dp = (C.c_void_p * 1)(), (C.c_void_p * 1)()
        assert L.rtmodt_compose_run(h, sp, None, F.MEM_HOST, dp, None, F.MEM_HOST) == F.E_INVALID and "no layout" in L.rtmodt_last_error().decode()
        assert L.rtmodt_compose_set_crop(h, 0, 0, 0, 1, 1) == F.E_INVALID and "no layout" in L.rtmodt_last_error().decode()
        p, pitch, ms = C.c_void_p(), C.c_size_t(0), C.c_float(0)
        assert L.rtmodt_compose_output(h, 0, C.byref(p), C.byref(pitch)) == F.E_INVALID
        assert L.rtmodt_compose_last_ms(h, C.byref(ms)) == F.E_INVALID and "no run" in L.rtmodt_last_error().decode()
        assert L.rtmodt_compose_run(None, sp, None, F.MEM_HOST, dp, None, F.MEM_HOST) == F.E_INVALID
    finally:
        L.rtmodt_compose_destroy(h)
    # a handle with smaller limits refuses what the largest limits take
    c = F.ComposeCfg.from_buffer_copy(cfg)
    c.max_dim, c.max_cells = 100, 2
    assert L.rtmodt_compose_create(C.byref(c), C.byref(h)) == F.OK
    try:
        rc, rc2, msg = _layout_rc(pkg, h, [(101, 5)], [VC.Output((8, 8))], [])
        assert rc == F.E_INVALID and rc2 == F.OK and "outside 1..100" in msg
        rc, rc2, _ = _layout_rc(pkg, h, [(5, 5)], [VC.Output((8, 8))], [VC.Cell(0, 0, (0, 0, 1, 1))] * 3)
        assert rc == F.E_CAPACITY and rc2 == F.OK
    finally:
        L.rtmodt_compose_destroy(h)
    with pytest.raises(ValueError, match="fit mode"):
        VC.plan_layout([(4, 4)], [VC.Output((4, 4))], [VC.Cell(0, 0, (0, 0, 4, 4), fit="cover")])
