"""CPU: ``csrc/letterbox.h`` -- the one statement of the letterbox geometry, of scale_boxes' gain and pads and of cv::resize's
INTER_LINEAR tables that the detector (engine.hip) and the overview of sliced inference (slice.hip) both use -- against
``oracle/yolo_oracle.py`` over a sweep of geometries, square and ``rect``.  ``tests/native/letterbox_check.cpp`` is a stand-alone
program around the header, built plain and with the address / undefined-behaviour sanitizers; every line it prints is compared.

The oracle cannot state the table of an axis whose resized side rounds to 0 (``_resize_coeffs`` divides by it), so that axis'
three table lines are not compared in such a case (the header prints them empty); everything else of the case still is.  Of the
11 152 cases 114 have a resized width of 0 and 130 a resized height of 0 (the test prints and cross-checks the counts)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import yolo_oracle as Y  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

F32 = np.float32
SRC = os.path.join(ROOT, "tests", "native", "letterbox_check.cpp")
HS = list(range(1, 260, 7)) + [360, 480, 720, 1080]
WS = list(range(1, 340, 11)) + [640, 1280, 1920]
SIZES = (32, 64, 320, 640)


def cases():
    """(h, w, in_h, in_w, rect): square S x S, and the padded rectangle LetterBox(auto=True) makes of S x S -- the shape a
    detector is built with for ``rect``."""
    out = []
    for S in SIZES:
        for h in HS:
            for w in WS:
                out.append((h, w, S, S, 0))
                uw, uh, top, bottom, left, right = Y.letterbox_params(h, w, S, S, auto=True)
                out.append((h, w, uh + top + bottom, uw + left + right, 1))
    return out


@functools.lru_cache(maxsize=None)
def table_lines(dst, src, names):
    return tuple(f"{n} " + " ".join(str(int(v)) for v in t) for n, t in zip(names, Y._resize_coeffs(dst, src)))


def expected(h, w, in_h, in_w, rect):
    """The eight lines after ``case``; None where the oracle has no statement."""
    S = max(in_h, in_w)
    uw, uh, top, _, left, _ = Y.letterbox_params(h, w, S, S, auto=True) if rect else Y.letterbox_params(h, w, in_h, in_w)
    # scale_boxes' first three lines (oracle/yolo_oracle.py), which it does not return
    gain = min(in_h / h, in_w / w)
    pad_x = Y._round_half_even((in_w - w * gain) / 2 - 0.1)
    pad_y = Y._round_half_even((in_h - h * gain) / 2 - 0.1)
    if gain > 0:      # ... tied to scale_boxes itself through the canvas centre, which lands inside the frame (no clipping)
        c = np.array([[in_w / 2, in_h / 2, in_w / 2, in_h / 2]], F32)
        want = (c - np.array([pad_x, pad_y, pad_x, pad_y], F32)) / F32(gain)
        if 0 < want[0, 0] < w and 0 < want[0, 1] < h:
            assert np.array_equal(Y.scale_boxes(c, in_h, in_w, h, w), want), (h, w, in_h, in_w)
    lines = [f"geom {h} {w} {uw} {uh} {top} {left} {int(uw != w or uh != h)}",
             f"back {int(F32(gain).view(np.uint32)):08x} {pad_x} {pad_y}"]
    lines += table_lines(uw, w, ("xofs", "xa0", "xa1")) if uw >= 1 else (None,) * 3
    lines += table_lines(uh, h, ("yofs", "yb0", "yb1")) if uh >= 1 else (None,) * 3
    return lines, uw, uh


@functools.lru_cache(maxsize=None)
def reference():
    """Computed once for both builds."""
    cs = cases()
    return cs, [expected(*c) for c in cs]


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("letterbox_check_san" if sanitize else "letterbox_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built letterbox_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def test_the_sweep_is_the_one_specified():
    cs = cases()
    assert len(cs) == 11152 and len(set(cs)) == len(cs)
    assert sum(c[4] for c in cs) == 5576


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_letterbox_header_equals_the_oracle(tmp_path, sanitize):
    cs, ref = reference()
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in cs), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == 9 * len(cs) + 1 and got[-1] == f"done {len(cs)}"
    no_x = no_y = compared = 0
    for i, (c, (lines, uw, uh)) in enumerate(zip(cs, ref)):
        assert got[9 * i] == "case %d %d %d %d %d" % c
        no_x += uw < 1
        no_y += uh < 1
        for k, want in enumerate(lines):
            if want is not None:
                assert got[9 * i + 1 + k] == want, (c, k, got[9 * i + 1 + k][:200], want[:200])
                compared += 1
    print(f"{len(cs)} cases, {compared} lines compared; resized width 0 in {no_x} cases, resized height 0 in {no_y}")
    assert compared == 8 * len(cs) - 3 * (no_x + no_y)
