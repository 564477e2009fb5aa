"""CPU: the occupancy heatmap's rules without a GPU.  ``tests/heatmap_ref.py`` (the NumPy restatement the kernels of
``csrc/heatmap.hip`` are pinned to) against hand-worked literal cases and against its own exhaustive per-cell loop; the footprint
rule of ``csrc/heatmap_stamp.h`` against the restatement, through the host-only entry point ``rtmodt_heatmap_footprint`` and through
``tests/native/heatmap_stamp_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as HR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

F32 = np.float32
SRC = os.path.join(ROOT, "tests", "native", "heatmap_stamp_check.cpp")
KINDS = [HR.BOX, HR.DISC, HR.FOOT]


def cells(box, h, w, cell, kind, r=0, cls=0, classes=None):
    """The footprint as a set of (cx, cy), after checking the vectorised restatement against the per-cell loop."""
    m = HR.footprint(box, cls, h, w, cell, kind, r, classes)
    got = {(x, y) for x, y in HR.cells_of(m)}
    assert got == HR.footprint_loop(box, cls, h, w, cell, kind, r, classes), (box, kind)
    return got


def rect(x0, y0, x1, y1):
    return {(x, y) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)}


# ---- hand-worked literal cases ---------------------------------------------------------------------------------------
def test_footprint_3x3_box_at_cell_1():
    """X = 2..4, Y = 2..4.  DISC: centre (6, 6) doubled, d = 3; a corner cell is at (+-2, +-2): 8 <= 9, so all nine.
    FOOT r = 1: centre (6, 8), d = 3, the square x 2..4, y 3..5, corners 8 <= 9: nine cells one row lower.  FOOT r = 0: (3, 4) alone."""
    b = [2.0, 2.9, 4.5, 4.0]
    assert cells(b, 10, 10, 1, HR.BOX) == rect(2, 2, 4, 4)
    assert cells(b, 10, 10, 1, HR.DISC) == rect(2, 2, 4, 4)
    assert cells(b, 10, 10, 1, HR.FOOT, 1) == rect(2, 3, 4, 5)
    assert cells(b, 10, 10, 1, HR.FOOT, 0) == {(3, 4)}
    # 5 x 5, X = 1..5: centre (6, 6), d = 5; corners at (+-4, +-4): 32 > 25 fall out, (+-4, +-2): 20 stay
    assert cells([1, 1, 5, 5], 10, 10, 1, HR.DISC) == rect(1, 1, 5, 5) - {(1, 1), (5, 1), (1, 5), (5, 5)}
    # an even width: X = 2..5, Y = 2..4: centre (7, 6), d = 3; cell 2 is at dx = -3: 9 + dy^2 <= 9 only in the middle row
    assert cells([2, 2, 5, 4], 10, 10, 1, HR.DISC) == {(3, 2), (4, 2), (2, 3), (3, 3), (4, 3), (5, 3), (3, 4), (4, 4)}
    # FOOT r = 2 on the same box: centre (7, 8), d = 5, cxp = 3, the square x 1..5, y 2..6; dx = -5, -3, -1, 1, 3, dy = -4..4:
    # column 1 (dx^2 = 25) keeps dy = 0 alone, the other four columns (dx^2 <= 9, dy^2 <= 16) all five rows: 1 + 20 = 21 cells
    want = rect(2, 2, 5, 6) | {(1, 4)}
    assert cells([2, 2, 5, 4], 10, 10, 1, HR.FOOT, 2) == want and len(want) == 21


def test_footprint_smaller_than_a_cell_at_cell_16():
    """X = 20..22, Y = 20..21 in cell (1, 1), whose centre is (47, 47) doubled.  DISC: centre (42, 41), d = 2: 25 + 36 > 4, the
    distance test fails and only the centre pixel (21, 20) stamps the cell.  FOOT r = 0: centre (42, 42), d = 1: likewise, (21, 21)."""
    b = [20.2, 20.7, 22.9, 21.5]
    assert cells(b, 64, 64, 16, HR.BOX) == {(1, 1)}
    assert cells(b, 64, 64, 16, HR.DISC) == {(1, 1)}
    assert cells(b, 64, 64, 16, HR.FOOT, 0) == {(1, 1)}
    st = HR._stamp(b, 0, 64, 64, HR.DISC, 0, None)
    assert st == ((20, 20, 22, 21), (42, 41, 2), (21, 20)) and (47 - 42) ** 2 + (47 - 41) ** 2 > 2 * 2
    # ... while a box whose centre sits on the cell's centre passes the distance test as well: X = 23..24: (47 - 47)^2 <= 4
    assert cells([23, 23, 24, 24], 64, 64, 16, HR.DISC) == {(1, 1)}
    # straddling four cells, too small to reach any of their centres: only the centre pixel's cell
    assert cells([14, 14, 17, 17], 64, 64, 16, HR.DISC) == {(0, 0)} and cells([14, 14, 17, 17], 64, 64, 16, HR.BOX) == rect(0, 0, 1, 1)
    # the clipped edge cell of a 37-row frame: rows 32..36 are cell row 2
    assert cells([3, 33, 5, 36.5], 37, 70, 16, HR.FOOT, 0) == {(0, 2)}


def test_footprint_half_outside_wholly_outside_and_inverted():
    """X = -4..2, Y = 2..6 in 10 x 10 at cell 1: BOX keeps columns 0..2.  DISC: centre (-2, 8), d = 5: column 0 (dx = 2) keeps
    dy^2 <= 21, all five rows; column 1 (dx = 4) dy^2 <= 9: rows 3..5; column 2 (dx = 6): none; the centre pixel (-1, 4) is outside."""
    b = [-4.5, 2, 2, 6]
    assert cells(b, 10, 10, 1, HR.BOX) == rect(0, 2, 2, 6)
    assert cells(b, 10, 10, 1, HR.DISC) == rect(0, 2, 0, 6) | {(1, 3), (1, 4), (1, 5)}
    # FOOT: the contact pixel (-1, 6) is outside; r = 2 reaches columns 0..1: centre (-2, 12), d = 5: dx = 2: dy^2 <= 21, dx = 4: dy^2 <= 9
    assert cells(b, 10, 10, 1, HR.FOOT, 0) == set()
    assert cells(b, 10, 10, 1, HR.FOOT, 2) == rect(0, 4, 0, 8) | {(1, 5), (1, 6), (1, 7)}
    # the bottom edge below the frame: FOOT's contact pixel is gone, DISC still marks what lies inside
    assert cells([2, 6, 4, 14], 10, 10, 1, HR.FOOT, 0) == set() and (3, 9) in cells([2, 6, 4, 14], 10, 10, 1, HR.DISC)
    for kind in KINDS:
        assert cells([12, 3, 15, 5], 10, 10, 1, kind, 1) == set()                   # wholly outside
        assert cells([-9, -9, -1.5, -1.5], 10, 10, 2, kind, 1) == set()
        assert cells([5.2, 1, 4.9, 3], 10, 10, 1, kind, 1) == set()                  # 5, 4 after truncation: inverted
        assert cells([1, 3.1, 4, 2.9], 10, 10, 1, kind, 1) == set()
        assert cells([5.9, 1, 5.1, 3], 10, 10, 1, kind, 0) != set()                  # 5, 5 after truncation: one column
        assert cells([1, 1, 3, 3], 10, 10, 1, kind, 0, cls=7, classes=(3, 5)) == set()
        assert cells([1, 1, 3, 3], 10, 10, 1, kind, 0, cls=5, classes=(3, 5)) != set()
        assert cells([1, 1, 3, 3], 10, 10, 1, kind, 0, classes=()) == set()
    assert cells([-0.5, -0.5, 0.5, 0.5], 10, 10, 1, HR.DISC) == {(0, 0)}            # int(-0.5) = 0
    assert cells([-3e9, -3e9, 3e9, 3e9], 4, 6, 2, HR.BOX) == rect(0, 0, 2, 1)      # clamped to +-2^20


def test_decay_saturation_level_and_jet_literals():
    assert HR.decay([1000, 1, 0, 8, 7], 3).tolist() == [875, 1, 0, 7, 7]          # 1000 - 125; 1 - 0; 8 - 1; 7 - 0
    assert HR.decay([1000, 65535, 65536, HR.U32_MAX], 16).tolist() == [1000, 65535, 65535, HR.U32_MAX - 65535]
    assert HR.decay([1, 3, HR.U32_MAX], 1).tolist() == [1, 2, 2 ** 31]
    top = HR.U32_MAX
    assert HR.stamp([top - 5, top - 5, top, top - 1024, 0], [5, 6, 1, 1, 0], 1).tolist() == [top, top, top, top - 1023, 0]
    assert HR.stamp([top - 1024, top - 1023, 7], [1, 1, 3], 1024).tolist() == [top, top, 3079]
    assert HR.stamp([top], [65536], 1024).tolist() == [top]                        # 64-bit sum: no wrap
    assert HR.levels([0, 1, 2, 3, 4], 3).tolist() == [0, 85, 170, 255, 255]         # (255 + 1) // 3, (510 + 1) // 3, 766 // 3, clamp
    assert HR.levels([1, 2, 3], 4).tolist() == [64, 128, 191]                       # (255 + 2) // 4 = 64, 512 // 4, 767 // 4
    assert HR.levels([top, top // 2], top).tolist() == [255, 127]                   # no overflow at the top
    jet = HR.jet_table()
    assert jet[0].tolist() == [127, 0, 0] and jet[64].tolist() == [255, 128, 0] and jet[128].tolist() == [125, 255, 129] \
        and jet[255].tolist() == [0, 0, 127]
    # a Ref handle: decay in every second call, before the stamp
    ref = HR.Ref(4, 4, 1, kind=HR.BOX, weight=1000, decay_shift=3, decay_every=2)
    assert ref.accumulate([[0, 0, 0, 0]])[0, 0] == 1000 and ref.accumulate([])[0, 0] == 875 and ref.accumulate([[0, 0, 0, 0]])[0, 0] == 1875
    # overlay: v < min_level keeps the pixel; alpha 256 is the table, alpha 0 the pixel
    fr = np.full((2, 2, 3), 200, np.uint8)
    g = np.array([[0, 1], [2, 3]], np.uint32)
    out = HR.overlay(fr, g, 1, alpha=256, min_level=1)
    assert out[0, 0].tolist() == [200] * 3 and out[0, 1].tolist() == jet[85].tolist() and out[1, 1].tolist() == jet[255].tolist()
    assert np.array_equal(HR.overlay(fr, g, 1, alpha=0), fr) and np.array_equal(HR.overlay(fr, g * 0, 1), fr)
    assert HR.overlay(fr, g, 1, alpha=128, min_level=200)[1].tolist() == [[200] * 3, [(200 * 128 + int(c) * 128 + 128) >> 8 for c in jet[255]]]
    assert HR.overlay(fr, g, 1, alpha=256, scale_max=2)[1, 0].tolist() == jet[255].tolist()


def test_zone_mask_uses_the_cells_centre_pixel():
    """cell 4 in a 10 x 10 frame: centres at 2, 6 and min(10, 9) = 9.  A polygon with a vertex on (6, 6) owns cell (1, 1)."""
    tri = [[6, 6], [9, 6], [9, 9]]
    m = HR.zone_mask(tri, 10, 10, 4)
    assert m.tolist() == [[False, False, False], [False, True, True], [False, False, True]]
    assert HR.zone_sums(np.arange(9, dtype=np.uint32).reshape(3, 3), [tri, []], 10, 10, 4) == [4 + 5 + 8, 0]


# ---- the footprint rule of the library -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def footprint_cases():
    """(kind index, foot_radius, cell, h, w, classes or None, cls, box) -- off-frame, inverted, at +-2^20, fractional, tiny and huge."""
    rng = np.random.default_rng(2027)
    out = []
    special = np.array([0.0, -0.0, 0.5, -0.5, -0.999, 0.999, 1.0, -1.0, 2.0 ** 20, -(2.0 ** 20), 2.0 ** 20 + 1, 3e9, -3e9, 1048575.94, 1e-30,
                        36.999996, 69.5, 15.999, 16.0, 31.5], F32)
    for i in range(1500):
        h, w = [(37, 70), (70, 37), (19, 150), (1, 1), (5, 3)][i % 5]
        kind = i % 3
        radius = int(rng.choice([0, 0, 1, 2, 5, 17, 256]))
        cell = int(rng.choice([1, 2, 4, 8, 16]))
        classes = [None, None, (), (0,), (3, 5, 80), tuple(range(256))][int(rng.integers(0, 6))]
        cls = int(rng.integers(0, 8))
        t = i % 7
        if t == 0:
            box = rng.uniform(-20, max(h, w) + 20, 4)
        elif t == 1:
            box = rng.choice(special, 4)
        elif t == 2:
            box = rng.uniform(-1.5e6, 1.5e6, 4)
        elif t == 3:                                                 # smaller than a cell
            x, y = rng.uniform(-2, w + 2), rng.uniform(-2, h + 2)
            box = [x, y, x + rng.uniform(0, 3), y + rng.uniform(0, 3)]
        else:
            a = np.sort(rng.uniform(-0.3 * w - 3, 1.3 * w + 3, 2)); b = np.sort(rng.uniform(-0.3 * h - 3, 1.3 * h + 3, 2))
            box = [a[0], b[0], a[1], b[1]] if i % 11 else [a[1], b[0], a[0], b[1]]
        out.append((kind, radius, cell, h, w, classes, cls, tuple(float(F32(v)) for v in box)))
    return out


@functools.lru_cache(maxsize=None)
def ref_cells(c):
    kind, radius, cell, h, w, classes, cls, box = c
    return HR.cells_of(HR.footprint(box, cls, h, w, cell, KINDS[kind], radius, classes))


def test_restatement_equals_its_per_cell_loop():
    kept = 0
    for c in footprint_cases()[::3]:
        kind, radius, cell, h, w, classes, cls, box = c
        loop = HR.footprint_loop(box, cls, h, w, cell, KINDS[kind], radius, classes)
        assert {tuple(v) for v in ref_cells(c)} == loop, c
        kept += bool(loop)
    assert 100 < kept < 450, kept


def test_heatmap_footprint_entry_point_equals_restatement(pkg):
    H = pkg.visualization.heatmap
    kept = 0
    for c in footprint_cases():
        kind, radius, cell, h, w, classes, cls, box = c
        got = H.footprint_cells(box, cls, h, w, cell=cell, footprint=KINDS[kind], foot_radius=radius, classes=classes)
        assert got.tolist() == ref_cells(c), c
        kept += len(got) > 0
    assert 300 < kept < 1350, kept
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            H.footprint_cells([1, 1, bad, 2], 0, 10, 10)
        assert e.value.code == pkg._ffi.E_INVALID
    # the two-call protocol reports the need without writing
    import ctypes as C
    cfg, _ = H.make_cfg(height=10, width=10, cell=1, footprint="box")
    need = C.c_int32(0)
    small = np.full((2, 2), -7, np.int32)
    xy = np.float32([2, 2, 4, 4])
    assert pkg._ffi.lib().rtmodt_heatmap_footprint(C.byref(cfg), pkg._ffi.ptr(xy), 0, pkg._ffi.ptr(small), 2, C.byref(need)) == 0
    assert need.value == 9 and (small == -7).all()


def test_heatmap_cfg_defaults_and_ranges(pkg):
    import ctypes as C
    H = pkg.visualization.heatmap
    L = pkg._ffi.lib()
    cfg = pkg._ffi.HeatmapCfg()
    L.rtmodt_heatmap_default_cfg(C.byref(cfg))
    assert (cfg.n_streams, cfg.height, cfg.width, cfg.cell, cfg.footprint, cfg.foot_radius, cfg.weight, cfg.decay_shift, cfg.decay_every,
            cfg.n_classes, cfg.device) == (1, 0, 0, 4, 1, 0, 1, 0, 1, 0, 0) and not cfg.classes
    mine, _ = H.make_cfg()
    assert all(getattr(mine, f) == getattr(cfg, f) for f, _ in cfg._fields_ if f != "classes") and not mine.classes
    # a parameter outside its range is refused before the device is touched (this machine has none); the defaults lack a frame size
    ok = dict(n_streams=2, height=37, width=70)
    for kw in (dict(), dict(ok, n_streams=0), dict(ok, n_streams=1025), dict(ok, height=0), dict(ok, width=32769), dict(ok, cell=0), dict(ok, cell=3),
               dict(ok, cell=32), dict(ok, foot_radius=-1), dict(ok, foot_radius=257), dict(ok, weight=0), dict(ok, weight=1025),
               dict(ok, decay_shift=-1), dict(ok, decay_shift=17), dict(ok, decay_every=0), dict(ok, decay_every=65537),
               dict(ok, classes=range(257)), dict(n_streams=2, height=32768, width=32768, cell=1)):
        bad, keep = H.make_cfg(**kw)
        h = C.c_void_p()
        assert L.rtmodt_heatmap_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw
    bad, _ = H.make_cfg(**ok)
    bad.footprint = 3
    h = C.c_void_p()
    assert L.rtmodt_heatmap_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value
    with pytest.raises(ValueError):
        H.make_cfg(footprint="circle")


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("heatmap_stamp_check_san" if sanitize else "heatmap_stamp_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built heatmap_stamp_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_heatmap_stamp_header_equals_restatement(tmp_path, sanitize):
    cases = footprint_cases()
    exe = build(tmp_path, sanitize)
    lines = []
    for kind, radius, cell, h, w, classes, cls, box in cases:
        cl = "-1" if classes is None else " ".join([str(len(classes))] + [str(c) for c in classes])
        lines.append(f"{kind} {radius} {cell} {h} {w} {cl} {cls} " + " ".join(f"{int(F32(v).view(np.uint32)):08x}" for v in box))
    # refusals: a configuration outside its ranges, a non-finite coordinate
    one = "3f800000 3f800000 40000000 40000000"
    extra = [f"3 0 4 10 10 -1 0 {one}", f"1 257 4 10 10 -1 0 {one}", f"1 -1 4 10 10 -1 0 {one}", f"1 0 3 10 10 -1 0 {one}", f"1 0 32 10 10 -1 0 {one}",
             f"1 0 4 0 10 -1 0 {one}", "1 0 4 10 10 -1 0 7fc00000 3f800000 40000000 40000000", "2 0 4 10 10 -1 0 3f800000 ff800000 40000000 40000000"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(cases) + len(extra) + 1 and got[-1] == f"done {len(cases) + len(extra)}"
    for c, g in zip(cases, got):
        want = ref_cells(c)
        assert g == " ".join([str(len(want))] + [f"{x} {y}" for x, y in want]), (c, g[:200])
    assert got[len(cases):-1] == ["bad"] * len(extra)
