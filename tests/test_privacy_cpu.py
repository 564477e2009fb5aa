"""CPU: the privacy masker's rules without a GPU.  ``tests/privacy_ref.py`` (the NumPy restatement the kernels of
``csrc/privacy.hip`` are pinned to) against hand-worked literal cases and against a naive per-pixel blur; the region arithmetic
of ``csrc/privacy_regions.h`` against the restatement, through the host-only entry point ``rtmodt_privacy_regions`` and through
``tests/native/privacy_regions_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour
sanitizers (nothing is loaded into Python under a sanitizer)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import privacy_ref as PR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

F32 = np.float32
SRC = os.path.join(ROOT, "tests", "native", "privacy_regions_check.cpp")


# ---- hand-worked literal cases ---------------------------------------------------------------------------------------
def test_pixelate_worked_cases():
    """(10 + 11 + 12 + 14 + 2) // 4 = 49 // 4 = 12; a clipped cell of 1, 2: (3 + 1) // 2 = 2."""
    img = np.zeros((2, 2, 3), np.uint8)
    img[..., 0] = [[10, 11], [12, 14]]
    img[..., 1] = [[0, 0], [0, 1]]                         # (1 + 2) // 4 = 0
    img[..., 2] = [[255, 255], [255, 254]]                 # (1019 + 2) // 4 = 255
    out = PR.pixelate_image(img, 2)
    assert out[..., 0].tolist() == [[12, 12], [12, 12]] and out[..., 1].tolist() == [[0, 0], [0, 0]] and out[..., 2].tolist() == [[255, 255], [255, 255]]
    # a 2 x 3 frame with cell 2: the right-hand cell is clipped to one column holding 1, 2
    img = np.zeros((2, 3, 3), np.uint8)
    img[:, 2, :] = [[1, 1, 1], [2, 2, 2]]
    out = PR.pixelate_image(img, 2)
    assert out[:, 2, 0].tolist() == [2, 2] and out[:, :2].max() == 0
    # pixels outside the mask count in the mean, and only masked pixels change
    fr = np.zeros((2, 2, 3), np.uint8)
    fr[..., 0] = [[10, 11], [12, 14]]
    got = PR.apply(fr, [[0, 0, 0, 0]], mode="pixelate", cell=2)
    assert got[..., 0].tolist() == [[12, 11], [12, 14]]


def test_blur_worked_5x5():
    """r = 1, one pass, v[y][x] = 10 * y + x (+ 100 in channel 1):
    corner (0, 0): 0 + 1 + 10 + 11 = 22, n = 4 -> (22 + 2) // 4 = 6;  edge (0, 2): 1 + 2 + 3 + 11 + 12 + 13 = 42, n = 6 -> 45 // 6 = 7;
    edge (2, 0): 10 + 11 + 20 + 21 + 30 + 31 = 123, n = 6 -> 126 // 6 = 21;  centre (2, 2): 9 * 22 = 198, n = 9 -> 202 // 9 = 22;
    corner (4, 4): 33 + 34 + 43 + 44 = 154 -> 156 // 4 = 39."""
    v = (10 * np.arange(5)[:, None] + np.arange(5)[None, :]).astype(np.uint8)
    img = np.stack([v, v + 100, 255 - v], axis=-1)
    for one in (PR.blur_pass, PR.blur_pass_naive):
        out = one(img, 1)
        assert (out[0, 0, 0], out[0, 2, 0], out[2, 0, 0], out[2, 2, 0], out[4, 4, 0]) == (6, 7, 21, 22, 39)
        assert (out[0, 0, 1], out[2, 2, 1]) == (106, 122)
        assert out[2, 2, 2] == 233                          # 9 * 233 = 2097 -> 2101 // 9 = 233
    # a radius larger than the frame: every window is the whole frame
    big = PR.blur_pass(img, 16)
    assert (big[..., 0] == (int(v.sum()) + 12) // 25).all()


@pytest.mark.parametrize("H, pm, rows", [(1, 1, 1), (1, 300, 1), (1, 1000, 1), (3, 1, 1), (3, 300, 1), (3, 1000, 3),
                                         (10, 1, 1), (10, 300, 3), (10, 1000, 10)])
def test_head_rows_worked(H, pm, rows):
    """max(1, (H * pm + 999) // 1000): H = 3 at 300: (900 + 999) // 1000 = 1; H = 10 at 300: 3999 // 1000 = 3; at 1: (10 + 999) // 1000 = 1."""
    assert PR.head_rows(H, pm) == rows
    r = PR.region([2.0, 5.0, 4.0, 5.0 + H - 1], 0, 64, 64, kind=PR.HEAD, head_pm=pm)
    assert r == (2, 5, 4, 5 + rows - 1)


def test_region_worked_cases():
    assert PR.region([1.9, -0.9, 3.2, 2.99], 0, 10, 10) == (1, 0, 3, 2)             # truncation toward zero, also below zero
    assert PR.region([-3.5, -2.5, -0.5, 4.0], 0, 10, 10) == (0, 0, 0, 4)            # int(-0.5) = 0 reaches column 0
    assert PR.region([-3.5, -2.5, -1.5, 4.0], 0, 10, 10) is None                    # clipped away
    assert PR.region([5.0, 5.0, 4.0, 6.0], 0, 10, 10) is None                       # inverted
    assert PR.region([5.0, 5.0, 4.0, 6.0], 0, 10, 10, expand_px=3) is None          # ... and expansion does not revive it
    assert PR.region([12.0, 3.0, 14.0, 4.0], 0, 10, 10, expand_px=3) == (9, 0, 9, 7)
    assert PR.region([-3e9, -3e9, 3e9, 3e9], 0, 10, 12) == (0, 0, 11, 9)           # clamped to +-2^20
    assert PR.region([1, 1, 2, 2], 7, 10, 10, classes=[3, 5]) is None and PR.region([1, 1, 2, 2], 5, 10, 10, classes=[3, 5]) == (1, 1, 2, 2)
    assert PR.region([1, 1, 2, 2], 0, 10, 10, classes=[]) is None


# ---- the restatement's blur against a naive loop ---------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 16])
@pytest.mark.parametrize("passes", [1, 2, 3])
def test_blur_restatement_equals_naive_loop(radius, passes):
    rng = np.random.default_rng(100 * radius + passes)
    for h, w in ((1, 1), (5, 3), (17, 23), (23, 17), (2, 19)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if (h, w) == (17, 23):
            img[:, :, 0] = 255                              # the largest sums
        assert np.array_equal(PR.blur_image(img, radius, passes), PR.blur_image(img, radius, passes, PR.blur_pass_naive)), (h, w)


# ---- the region arithmetic of the library ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def region_cases():
    """(kind, head_pm, expand_px, h, w, classes or None, cls, box) -- off-frame, inverted, at +-2^20, fractional and negative."""
    rng = np.random.default_rng(20260)
    out = []
    special = np.array([0.0, -0.0, 0.5, -0.5, -0.999, 0.999, 1.0, -1.0, 2.0 ** 20, -(2.0 ** 20), 2.0 ** 20 + 1, -(2.0 ** 20) - 1, 3e9, -3e9,
                        1048575.94, -1048575.94, 1e-30, 36.999996, 69.5], F32)
    for i in range(4000):
        h, w = [(37, 70), (1, 1), (1080, 1920), (5, 3)][i % 4]
        kind = i % 2
        head_pm = int(rng.choice([1, 300, 999, 1000, int(rng.integers(1, 1001))]))
        expand = int(rng.choice([0, 0, 1, 7, 256]))
        classes = [None, (), (0,), (3, 5, 80), tuple(range(256))][int(rng.integers(0, 5))]
        cls = int(rng.integers(0, 8))
        t = i % 5
        if t == 0:
            box = rng.uniform(-20, max(h, w) + 20, 4)
        elif t == 1:
            a = rng.uniform(-10, w + 10, 2); b = rng.uniform(-10, h + 10, 2)
            box = [a.min(), b.min(), a.max(), b.max()]
        elif t == 2:
            box = rng.choice(special, 4)
        elif t == 3:
            box = rng.uniform(-1.5e6, 1.5e6, 4)
        else:
            a = np.sort(rng.uniform(-3, w + 3, 2)); b = np.sort(rng.uniform(-3, h + 3, 2))
            box = [a[0], b[0], a[1], b[1]] if i % 10 else [a[1], b[0], a[0], b[1]]
        out.append((kind, head_pm, expand, h, w, classes, cls, tuple(float(F32(v)) for v in box)))
    return out


def ref_region(c):
    kind, head_pm, expand, h, w, classes, cls, box = c
    return PR.region(box, cls, h, w, kind=(PR.HEAD if kind else PR.BOX), head_pm=head_pm, expand_px=expand, classes=classes)


def test_privacy_regions_entry_point_equals_restatement(pkg):
    P = pkg.visualization.privacy
    cases = region_cases()
    groups = {}
    for c in cases:
        groups.setdefault(c[:6], []).append(c)
    checked = kept = 0
    for key, cs in groups.items():
        kind, head_pm, expand, h, w, classes = key
        boxes = np.array([c[7] for c in cs], F32)
        cls = np.array([c[6] for c in cs], np.int32)
        got = P.regions(boxes, cls, h, w, region="head" if kind else "box", head_fraction=head_pm / 1000.0, expand_px=expand, classes=classes)
        want = [r for r in map(ref_region, cs) if r is not None]
        assert got.tolist() == [list(r) for r in want], key
        checked += len(cs); kept += len(want)
    assert checked == 4000 and 400 < kept < 3600, (checked, kept)
    # without a class list the classes may be left out; the two-call protocol reports the need without writing
    assert P.regions([[1, 1, 2, 2]], None, 10, 10).tolist() == [[1, 1, 2, 2]]
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            P.regions([[1, 1, bad, 2]], None, 10, 10)
        assert e.value.code == pkg._ffi.E_INVALID


def test_privacy_cfg_defaults_and_ranges(pkg):
    import ctypes as C
    P = pkg.visualization.privacy
    L = pkg._ffi.lib()
    cfg = pkg._ffi.PrivacyCfg()
    L.rtmodt_privacy_default_cfg(C.byref(cfg))
    assert (cfg.mode, cfg.cell, cfg.radius, cfg.passes, cfg.region, cfg.head_pm, cfg.expand_px, cfg.n_classes, cfg.max_regions, cfg.device) == \
        (1, 16, 8, 2, 0, 300, 0, 0, 65536, 0) and not cfg.classes and list(cfg.fill_bgr)[:3] == [0, 0, 0]
    mine, _ = P.make_cfg()
    assert all(getattr(mine, f) == getattr(cfg, f) for f, _ in cfg._fields_ if f not in ("fill_bgr", "classes")) and not mine.classes
    # a parameter outside its range is refused before the device is touched (this machine has none)
    for kw in (dict(cell=1), dict(cell=65), dict(radius=0), dict(radius=17), dict(passes=0), dict(passes=4), dict(head_fraction=0.0),
               dict(head_fraction=1.001), dict(expand_px=-1), dict(expand_px=257), dict(classes=range(257)), dict(max_regions=0),
               dict(max_regions=65537)):
        bad, keep = P.make_cfg(**kw)
        h = C.c_void_p()
        assert L.rtmodt_privacy_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("privacy_regions_check_san" if sanitize else "privacy_regions_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built privacy_regions_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_privacy_regions_header_equals_restatement(tmp_path, sanitize):
    cases = region_cases()
    exe = build(tmp_path, sanitize)
    lines = []
    for kind, head_pm, expand, h, w, classes, cls, box in cases:
        cl = "-1" if classes is None else " ".join([str(len(classes))] + [str(c) for c in classes])
        lines.append(f"{kind} {head_pm} {expand} {h} {w} {cl} {cls} " + " ".join(f"{int(F32(v).view(np.uint32)):08x}" for v in box))
    # refusals: a configuration outside its ranges, a non-finite coordinate
    extra = ["2 300 0 10 10 -1 0 3f800000 3f800000 40000000 40000000", "0 0 0 10 10 -1 0 3f800000 3f800000 40000000 40000000",
             "0 300 257 10 10 -1 0 3f800000 3f800000 40000000 40000000", "0 300 0 10 10 -1 0 7fc00000 3f800000 40000000 40000000",
             "0 300 0 10 10 -1 0 3f800000 ff800000 40000000 40000000"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(cases) + len(extra) + 1 and got[-1] == f"done {len(cases) + len(extra)}"
    for c, g in zip(cases, got):
        r = ref_region(c)
        assert g == ("none" if r is None else "%d %d %d %d" % r), (c, g)
    assert got[len(cases):-1] == ["bad"] * len(extra)
