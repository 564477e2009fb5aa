"""CPU: the frame enhancer's rules without a GPU.  ``tests/enhance_ref.py`` (the restatement the kernels of ``csrc/enhance.hip`` are
pinned to) against hand-worked literal cases, against a second statement (the curve with ``Fraction`` and OpenCV's serial residual
loop, the axis with ``Fraction``, the interpolation in float64) and with one deliberate defect at a time, which the literals catch;
properties over random frames; the rules of ``csrc/enhance_rule.h`` against the restatement, through
``tests/native/enhance_rule_check.cpp`` -- a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer) -- and through the host-only entry points ``rtmodt_enhance_curve`` /
``rtmodt_enhance_axis``; the ABI's refusals, which need no device; and the premise of the module on the restatements alone: a dim box
moving through a dark scene is STILL to the motion detector raw and MOTION enhanced, and the enhanced boxless scene stays STILL.
PARITY UNPINNED: the reference has no counterpart, ``cv2.createCLAHE`` is installed nowhere this runs, and no default has been
validated on real footage."""
import functools
import gc
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enhance_cases as EC  # noqa: E402
import enhance_ref as ER  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402
from test_motion_cpu import lcg_bytes  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "enhance_rule_check.cpp")
DEFECTS = ("origins", "no_residual", "cdf32", "no_first")


def grey(rows):
    """A frame whose pixel (x, y) has luma rows[y][x] exactly (B = G = R = v gives Y = v)."""
    a = np.asarray(rows, np.uint8)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2))


def one_bin(b, n):
    h = np.zeros(256, np.int64)
    h[b] = n
    return h


# ---- hand-worked literal cases; each takes the defect to switch in (None: the restatement as it is) -----------------------------
FOUR = [[10, 10, 20, 20], [10, 10, 20, 20], [30, 30, 40, 40], [30, 30, 40, 40]]


def literal_4x4_one_tile(defect=None):
    """n = 16, four levels of four pixels.  Without a clip cdf = 4, 8, 12, 16 and curve = (cdf * 255 + 8) // 16 = 64, 128, 191, 255.
    clip_q8 512: clip = max(1, 8192 >> 16) = 1, excess 12, no batch, res 12, step 21: bins 0, 21, .., 231 gain one.  cdf(10) = 1 + 1,
    cdf(20) = 1 + 2, cdf(30) = 2 + 3, cdf(40) = 2 + 4 -> (510 + 8) // 16 = 32, 48, 80, 96."""
    r = ER.Ref(1, 4, 4, defect, tiles_y=1, tiles_x=1, clip_q8=0)
    out, row = r.step(0, grey(FOUR))
    assert out[..., 0].tolist() == out[..., 1].tolist() == out[..., 2].tolist() == [[64, 64, 128, 128], [64, 64, 128, 128], [191, 191, 255, 255], [191, 191, 255, 255]]
    assert row == dict(stream=0, frames_seen=1, luma_sum=4 * (10 + 20 + 30 + 40), eff=256, clipped=0)
    r = ER.Ref(1, 4, 4, defect, tiles_y=1, tiles_x=1, clip_q8=512)
    out, row = r.step(0, grey(FOUR))
    assert out[..., 1].tolist() == [[32, 32, 48, 48], [32, 32, 48, 48], [80, 80, 96, 96], [80, 80, 96, 96]] and row["clipped"] == 12
    r = ER.Ref(1, 4, 4, defect, tiles_y=1, tiles_x=1, clip_q8=0, strength=128)          # 10 + ((54 * 128 + 128) >> 8) = 37, ...
    assert r.step(0, grey(FOUR))[0][..., 2].tolist() == [[37, 37, 74, 74], [37, 37, 74, 74], [111, 111, 148, 148], [111, 111, 148, 148]]


def literal_even_histogram(defect=None):
    """Four pixels in every bin, n = 1024: cdf = 4 (v + 1), curve = ((v + 1) * 255 + 128) // 256 -- v + 1 up to 127, v from 128 on, 255 at
    255.  clip_q8 512 gives clip 8: nothing is above it."""
    want = [v + 1 if v < 128 else v for v in range(255)] + [255]
    for clip_q8 in (0, 512):
        cur, ex, cdf = ER.curve(np.full(256, 4), 1024, clip_q8, defect)
        assert cur.tolist() == want and ex == 0 and cdf[255] == 1024


def literal_one_bin_and_residuals(defect=None):
    # 1000 pixels in bin 7, clip 7 (512 * 1000 >> 16), excess 993 = 3 * 256 + 225, step 1: bins 0..224 hold 4, the rest 3, bin 7 holds 11
    cur, ex, cdf = ER.curve(one_bin(7, 1000), 1000, 512, defect)
    assert (ex, int(cdf[6]), int(cdf[7]), int(cdf[224]), int(cdf[255])) == (993, 28, 39, 28 + 11 + 217 * 4, 1000)
    assert (int(cur[6]), int(cur[7]), int(cur[255])) == (7, 10, 255)                    # (7140 + 500) // 1000, (9945 + 500) // 1000
    # clip forced to 1 (clip_q8 1), one bin at 100.  n 258: excess 257, batch 1, res 1, step 256: bin 0 gains one
    cur, ex, cdf = ER.curve(one_bin(100, 258), 258, 1, defect)
    assert ex == 257 and cdf.tolist() == [v + 2 + (v >= 100) for v in range(256)]
    assert int(cur[0]) == (2 * 255 + 129) // 258 == 2 and int(cur[255]) == 255
    # n 385: excess 384, batch 1, res 128, step 2: the even bins gain one
    cur, ex, cdf = ER.curve(one_bin(100, 385), 385, 1, defect)
    assert ex == 384 and cdf.tolist() == [v + 1 + v // 2 + 1 + (v >= 100) for v in range(256)] and int(cur[255]) == 255
    # n 256: excess 255 (below 256: no batch), res 255, step 1: bins 0..254 gain one, bin 255 nothing
    cur, ex, cdf = ER.curve(one_bin(100, 256), 256, 1, defect)
    assert ex == 255 and cdf.tolist() == [v + 1 + (v >= 100) for v in range(255)] + [256] and int(cur[254]) == int(cur[255]) == 255
    cur, ex, cdf = ER.curve(one_bin(255, 256), 256, 1, defect)
    assert cdf.tolist() == [v + 1 for v in range(256)]


def literal_whole_frame_in_one_tile(defect=None):
    """A 16384 x 16384 frame in one tile: cdf * 255 passes 2^32."""
    cur, ex, cdf = ER.curve(one_bin(0, 1 << 28), 1 << 28, 0, defect)
    assert cur.tolist() == [255] * 256 and ex == 0
    h = np.zeros(256, np.int64)
    h[10] = h[200] = 1 << 27
    assert ER.curve(h, 1 << 28, 0, defect)[0].tolist() == [0] * 10 + [128] * 190 + [255] * 56      # (2^27 * 255 + 2^27) >> 28 = 128


def literal_axis_tables(defect=None):
    """w 7, 3 tiles: bounds 0 2 4 7, twice the centres 1 5 10.  x 1: (2 - 1) * 256 / 4 = 64; x 3: (6 - 5) * 256 / 5 = 51.2; x 5 is at the last centre."""
    k, f = ER.axis(7, 3, defect)
    assert ER.bounds(7, 3) == [0, 2, 4, 7]
    assert (k.tolist(), f.tolist()) == ([0, 0, 0, 1, 1, 2, 2], [0, 64, 192, 51, 154, 0, 0])
    # w 37, 16 tiles: tiles of 2 and 3 pixels, narrower than a run of 4; twice the centres 1 5 9 14 19 23 28 33 37 42 47 51 56 61 65 70
    assert ER.bounds(37, 16) == [0, 2, 4, 6, 9, 11, 13, 16, 18, 20, 23, 25, 27, 30, 32, 34, 37]
    k, f = ER.axis(37, 16, defect)
    assert k.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6, 6, 7, 7, 8, 8, 9, 9, 9, 10, 10, 11, 11, 12, 12, 12, 13, 13, 14, 14, 15, 15]
    assert f.tolist() == [0, 64, 192, 64, 192, 51, 154, 0, 102, 205, 64, 192, 51, 154, 0, 102, 205, 64, 192, 51, 154, 0, 102, 205, 64, 192, 51, 154, 0, 102, 205,
                          64, 192, 51, 154, 0, 0]
    assert [v.tolist() for v in ER.axis(5, 1, defect)] == [[0] * 5, [0] * 5]


def literal_ema_steps(defect=None):
    e = lambda s, cur, seen, shift: int(ER.ema(np.int64([s]), np.int64([cur]), seen, shift, defect)[0])      # noqa: E731
    assert e(0, 100, 0, 2) == 25600 and e(777, 100, 0, 7) == 25600                      # the first frame sets
    assert e(25600, 120, 1, 2) == 25600 + 1280 and e(25600, 80, 1, 2) == 25600 - 1280   # the second moves a quarter of the way
    assert e(25600, 120, 5, 0) == 30720 and e(25600, 80, 5, 0) == 20480                 # shift 0 follows at once
    assert e(25599, 100, 9, 2) == 25599 and e(25603, 100, 9, 2) == 25603                # stalled within 2^shift, from below and from above
    assert e(25596, 100, 9, 2) == 25597 and e(25604, 100, 9, 2) == 25603                # (an arithmetic shift of -3 would have moved)
    assert ER.lut8(np.int64([25599, 25603, 25600 + 127, 25600 + 128, 65280, 0])).tolist() == [100, 100, 100, 101, 255, 0]


def literal_strength_and_colour(defect=None):
    c = ER.config(strength=256, auto_lo=40, auto_hi=120)
    px = 1000
    eff = lambda m: ER.eff_of(c, m * px + px - 1, px)                                      # noqa: E731  (the mean is floored)
    assert [eff(m) for m in (0, 40, 41, 80, 100, 119, 120, 255)] == [256, 256, 256 * 79 // 80, 128, 64, 3, 0, 0]
    assert ER.eff_of(ER.config(strength=200), 255 * px, px) == 200 and ER.eff_of(ER.config(strength=77, auto_lo=9, auto_hi=9), 0, px) == 77
    y2 = lambda y, y1, e: int(ER.y2_of(np.int64([y]), np.int64([y1]), e)[0])              # noqa: E731
    assert (y2(10, 64, 256), y2(10, 64, 128), y2(10, 64, 0), y2(200, 100, 256), y2(200, 199, 128), y2(200, 199, 127)) == (64, 37, 10, 100, 200, 200)
    assert y2(200, 197, 128) == 199 and y2(200, 197, 43) == 199 and y2(200, 197, 42) == 200    # -3 * 43 + 128 = -1, and floor(-1 / 256) = -1
    col = lambda bgr, y, y2_, rule: ER.colour_of(np.uint8([[bgr]]), np.int64([[y]]), np.int64([[y2_]]), rule)[0, 0].tolist()      # noqa: E731
    assert int(MR.pixel_luma(np.uint8([[[4, 0, 0]]]))[0, 0]) == 0
    assert col([4, 0, 0], 0, 10, ER.GAIN) == [14, 10, 10] and col([4, 0, 0], 0, 255, ER.GAIN) == [255, 255, 255]      # Y 0: c + Y2
    assert col([200, 100, 3], 100, 200, ER.GAIN) == [255, 200, 6]                         # 40050 // 100 saturates; 20050 // 100; 650 // 100
    assert col([200, 100, 3], 100, 50, ER.GAIN) == [100, 50, 2]                           # Y2 < Y: 10050 // 100, 5050 // 100, 200 // 100
    assert col([250, 100, 5], 100, 120, ER.SHIFT) == [255, 120, 25] and col([250, 100, 5], 100, 80, ER.SHIFT) == [230, 80, 0]
    for rule in (ER.SHIFT, ER.GAIN):                                                      # eff 0: Y2 == Y, the input bytes
        assert col([250, 100, 5], 103, 103, rule) == [250, 100, 5] and col([4, 0, 0], 0, 0, rule) == [4, 0, 0]


def literal_interpolation_between_centres(defect=None):
    """A 1 x 7 frame of level 0 over 3 tiles whose curves map 0 to 0, 100 and 200: the pixels at the centres (0.5 -> pixel 0 is left of
    it, 2.5, 5) take their tile's value, those between are weighted by f."""
    lut = np.zeros((1, 3, 256), np.int64)
    lut[0, :, 0] = [0, 100, 200]
    got = ER.interpolate(np.zeros((1, 7), np.int64), lut, 1, 3, defect)[0].tolist()
    assert got == [0, (64 * 100 * 256 + 32768) >> 16, (192 * 100 * 256 + 32768) >> 16, ((205 * 100 + 51 * 200) * 256 + 32768) >> 16,
                   ((102 * 100 + 154 * 200) * 256 + 32768) >> 16, 200, 200] == [0, 25, 75, 120, 160, 200, 200]


LITERALS = (literal_4x4_one_tile, literal_even_histogram, literal_one_bin_and_residuals, literal_whole_frame_in_one_tile, literal_axis_tables,
            literal_ema_steps, literal_strength_and_colour, literal_interpolation_between_centres)


@pytest.mark.parametrize("literal", LITERALS, ids=lambda f: f.__name__)
def test_restatement_equals_hand_worked_literals(literal):
    literal()


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_deliberate_defect_fails_a_literal(defect):
    """origins: interpolating from tile origins instead of centres; no_residual: the residual dropped; cdf32: a 32-bit cdf * 255;
    no_first: the EMA without the first-frame rule."""
    failed = []
    for literal in LITERALS:
        try:
            literal(defect)
        except AssertionError:
            failed.append(literal.__name__)
    assert failed, defect
    expected = dict(origins="literal_axis_tables", no_residual="literal_one_bin_and_residuals", cdf32="literal_whole_frame_in_one_tile", no_first="literal_ema_steps")
    assert expected[defect] in failed


# ---- a second statement ---------------------------------------------------------------------------------------------------------------
def curve_second(hist, n, clip_q8):
    """OpenCV's order of steps with its serial residual loop, and the level as a rounded Fraction."""
    hist = [int(v) for v in hist]
    if clip_q8 > 0:
        clip = max(1, clip_q8 * n // 65536)
        clipped = 0
        for i in range(256):
            if hist[i] > clip:
                clipped += hist[i] - clip
                hist[i] = clip
        batch, residual = clipped // 256, clipped % 256
        hist = [v + batch for v in hist]
        if residual:
            step, i = max(256 // residual, 1), 0
            while i < 256 and residual > 0:
                hist[i] += 1
                i += step
                residual -= 1
            assert residual == 0
    out, cdf = [], 0
    for v in hist:
        cdf += v
        out.append(math.floor(Fraction(cdf * 255, n) + Fraction(1, 2)))
    return out, cdf


def axis_second(px, t):
    b = [k * px // t for k in range(t + 1)]
    c = [Fraction(b[k] + b[k + 1] - 1, 2) for k in range(t)]                              # the centre of tile k, in pixel coordinates
    out = []
    for x in range(px):
        if t == 1 or x <= c[0]:
            out.append((0, 0))
        elif x >= c[-1]:
            out.append((t - 1, 0))
        else:
            k = max(i for i in range(t) if c[i] <= x)
            out.append((k, math.floor((x - c[k]) / (c[k + 1] - c[k]) * 256 + Fraction(1, 2))))
    return out


def random_hist(rng, n):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        p = rng.dirichlet(np.full(256, 0.05))
    elif kind == 1:
        p = np.zeros(256)
        lo = int(rng.integers(0, 240))
        p[lo:lo + 16] = 1 / 16
    else:
        p = rng.dirichlet(np.ones(256))
    return rng.multinomial(n, p).astype(np.int64)


@functools.lru_cache(maxsize=None)
def curve_cases():
    rng = np.random.default_rng(4110)
    out = []
    for i in range(400):
        n = int(rng.choice([1, 2, 6, 255, 256, 257, 1200, 32400, 1 << 20, 1 << 28, int(rng.integers(1, 1 << 20))]))
        clip_q8 = int(rng.choice([0, 1, 256, 512, 1024, 65536, int(rng.integers(1, 4096))]))
        out.append((random_hist(rng, n), n, clip_q8))
    return out


def test_second_statements_agree_everywhere():
    for hist, n, clip_q8 in curve_cases():
        cur, ex, cdf = ER.curve(hist, n, clip_q8)
        want, total = curve_second(hist, n, clip_q8)
        assert cur.tolist() == want and total == n == int(cdf[255]), (n, clip_q8)
        assert int(cur[255]) == 255 and (np.diff(cur) >= 0).all()
    for px in list(range(1, 40)) + [70, 150, 530, 1920, 16384]:
        for t in range(1, min(px, 16) + 1):
            k, f = ER.axis(px, t)
            assert list(zip(k.tolist(), f.tolist())) == axis_second(px, t), (px, t)
            assert (f >= 0).all() and (f <= 256).all() and (np.diff(k) >= 0).all()
    rng = np.random.default_rng(4111)
    for h, w, ty, tx in ((37, 70, 8, 8), (5, 9, 2, 3), (19, 150, 16, 16), (70, 37, 16, 16)):
        lut = np.sort(rng.integers(0, 256, (ty, tx, 256)), axis=2)
        y = rng.integers(0, 256, (h, w))
        (ky, fy), (kx, fx) = ER.axis(h, ty), ER.axis(w, tx)
        wy, wx = (fy / 256.0)[:, None], (fx / 256.0)[None, :]                           # exact in float64
        ky, kx = ky[:, None], kx[None, :]
        ky1, kx1 = np.minimum(ky + 1, ty - 1), np.minimum(kx + 1, tx - 1)
        val = (1 - wy) * ((1 - wx) * lut[ky, kx, y] + wx * lut[ky, kx1, y]) + wy * ((1 - wx) * lut[ky1, kx, y] + wx * lut[ky1, kx1, y])
        assert (val * 65536 == np.round(val * 65536)).all()                             # multiples of 1 / 65536: no tie at + 32768 / 65536 ... but exactly .5
        assert ER.interpolate(y, lut, ty, tx).tolist() == np.floor(val + 0.5).astype(np.int64).tolist()


# ---- properties over random frames ----------------------------------------------------------------------------------------------------------
def geometry_grid_cases():
    return [(h, w, g) for h, w, _ in EC.GEOMETRIES + EC.WIDE_GEOMETRIES[:2] for g in EC.GRIDS if EC.fits(g, h, w)]


@pytest.mark.parametrize("h,w,grid", geometry_grid_cases())
def test_properties_of_random_frames(h, w, grid):
    rng = np.random.default_rng(4120 + h + 7 * grid[0])
    kinds = EC.CONTENTS
    for n_case, kind in enumerate(kinds):
        frame = EC.content(kind, h, w, rng)
        clip_q8 = EC.CLIP_Q8[n_case % 3]
        hist = ER.histograms(frame, *grid)
        by, bx = ER.bounds(h, grid[0]), ER.bounds(w, grid[1])
        for j in range(grid[0]):
            for i in range(grid[1]):
                n = (by[j + 1] - by[j]) * (bx[i + 1] - bx[i])
                cur, ex, cdf = ER.curve(hist[j, i], n, clip_q8)
                assert hist[j, i].sum() == n and cdf[255] == n and cur[255] == 255 and (np.diff(cur) >= 0).all() and 0 <= ex < n
        assert hist.sum() == h * w
        for colour in (ER.SHIFT, ER.GAIN):
            # eff 0 is the identity, by strength and by auto on a frame brighter than auto_hi
            out, row = ER.Ref(1, h, w, tiles_y=grid[0], tiles_x=grid[1], clip_q8=clip_q8, strength=0, colour=colour).step(0, frame)
            assert row["eff"] == 0 and np.array_equal(out, frame)
        bright = np.maximum(frame, 200)
        out, row = ER.Ref(1, h, w, tiles_y=grid[0], tiles_x=grid[1], auto_lo=40, auto_hi=120).step(0, bright)
        assert row["eff"] == 0 and np.array_equal(out, bright)
        # SHIFT leaves c - Y unchanged wherever nothing clamps: every channel moves by the same amount
        out, _ = ER.Ref(1, h, w, tiles_y=grid[0], tiles_x=grid[1], clip_q8=clip_q8).step(0, frame)
        d = out.astype(np.int64) - frame
        free = ((out > 0) & (out < 255)).all(2)
        assert (d[free] == d[free][:, :1]).all()
        if kind == "constant":
            # a constant frame of level v: a tile's curve at v depends on its area alone -- it is 255 without a clip -- and every pixel
            # moves by a weighted mean of its tiles' values: the frame stays constant where the tiles agree, and always without a clip
            v = int(MR.pixel_luma(frame)[0, 0])
            areas = {(by[j + 1] - by[j]) * (bx[i + 1] - bx[i]) for j in range(grid[0]) for i in range(grid[1])}
            moves = [int(ER.curve(one_bin(v, n), n, clip_q8)[0][v]) - v for n in areas]
            assert (d[free] >= min(moves)).all() and (d[free] <= max(moves)).all()
            if clip_q8 == 0:
                assert moves == [255 - v] * len(moves)
            if len(set(moves)) == 1:
                assert (out == out[0, 0]).all() and (d[free] == moves[0]).all()
    out, _ = ER.Ref(1, h, w, tiles_y=grid[0], tiles_x=grid[1], clip_q8=0).step(0, EC.content("constant", h, w, rng))
    assert (out == 255).all()                                                            # every tile's curve is 255 at the one level there is
    # one tile, no clip, first frame: a global histogram equalisation, computed here from the whole frame's cumulative counts
    frame = EC.content("night", h, w, rng)
    y = MR.pixel_luma(frame)
    cdf = np.cumsum(np.bincount(y.ravel(), minlength=256))
    y1 = (cdf[y] * 255 + h * w // 2) // (h * w)
    out, _ = ER.Ref(1, h, w, tiles_y=1, tiles_x=1, clip_q8=0).step(0, frame)
    assert np.array_equal(out, np.clip(frame.astype(np.int64) + (y1 - y)[..., None], 0, 255))


# ---- the rule header through a stand-alone program ----------------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("enhance_rule_check_san" if sanitize else "enhance_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built enhance_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def walk_cases():
    """(h, w, pitch, base, wide, ty, tx, seed): a pitch of 3w puts the frame's last byte at the buffer's last byte; partial runs, tiles
    narrower than a run, more than 64 runs to a row (a lane walks several), the dword path only with an aligned pitch and base."""
    return [(5, 9, 27, 0, 0, 2, 3, 1), (5, 9, 29, 1, 0, 5, 9, 2), (4, 8, 24, 0, 1, 1, 1, 3), (4, 8, 24, 4, 1, 4, 8, 4), (3, 37, 111, 3, 0, 3, 16, 5),
            (3, 36, 108, 0, 1, 2, 16, 6), (2, 300, 900, 0, 1, 2, 7, 7), (2, 301, 903, 0, 0, 1, 16, 8), (7, 70, 212, 8, 1, 7, 8, 9), (1, 1, 3, 0, 0, 1, 1, 10),
            (1, 4, 12, 0, 1, 1, 4, 11), (6, 5, 16, 0, 1, 2, 2, 12)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_enhance_rule_header_equals_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    rng = np.random.default_rng(4130)
    lines, want = [], []
    for hist, n, clip_q8 in curve_cases()[:200]:
        lines.append(f"c {clip_q8} {n} " + " ".join(str(int(v)) for v in hist))
        cur, ex, _ = ER.curve(hist, n, clip_q8)
        want.append(" ".join(str(int(v)) for v in [ex] + cur.tolist()))
    for clip_q8, b, n in ((0, 0, 1 << 28), (512, 255, 1 << 28), (65536, 9, 1 << 28), (1, 100, 258), (1, 100, 385), (1, 100, 256), (512, 7, 1000)):
        lines.append(f"1 {clip_q8} {b} {n}")                                              # 2^28 pixels in one tile
        cur, ex, _ = ER.curve(one_bin(b, n), n, clip_q8)
        want.append(" ".join(str(int(v)) for v in [ex] + cur.tolist()))
    for px, t in [(7, 3), (37, 16), (1, 1), (16, 16), (17, 16), (70, 8), (530, 16), (16384, 16), (16383, 7), (5, 5), (9, 2)]:
        lines.append(f"a {px} {t}")
        k, f = ER.axis(px, t)
        b = ER.bounds(px, t)
        own = np.searchsorted(b, np.arange(px), side="right") - 1
        want.append(" ".join(str(v) for v in b) + "".join(f" {a} {c} {o}" for a, c, o in zip(k.tolist(), f.tolist(), own.tolist())))
    for _ in range(400):
        s, cur = int(rng.choice([0, 1, 65280, 25600, int(rng.integers(0, 65281))])), int(rng.choice([0, 100, 255, int(rng.integers(0, 256))]))
        seen, shift = int(rng.choice([0, 1, 2 ** 30])), int(rng.integers(0, 8))
        lines.append(f"e {s} {cur} {seen} {shift}")
        v = int(ER.ema(np.int64([s]), np.int64([cur]), seen, shift)[0])
        assert 0 <= v <= 65280
        want.append(f"{v} {int(ER.lut8(np.int64([v]))[0])} {min(seen + 1, 2 ** 30)}")
    for _ in range(400):
        a, b, c, d = (int(v) for v in rng.choice([0, 1, 128, 255, int(rng.integers(0, 256))], 4))
        fx, fy = (int(v) for v in rng.choice([0, 1, 128, 255, 256, int(rng.integers(0, 257))], 2))
        lines.append(f"i {a} {b} {c} {d} {fx} {fy}")
        want.append(str(((256 - fy) * ((256 - fx) * a + fx * b) + fy * ((256 - fx) * c + fx * d) + 32768) >> 16))
    for _ in range(400):
        strength, lo = int(rng.choice([0, 1, 128, 255, 256])), int(rng.integers(0, 200))
        hi = int(rng.choice([lo, lo + 1, 255, int(rng.integers(lo, 256))]))
        px = int(rng.choice([1, 45, 1 << 28]))
        luma = int(rng.integers(0, 255 * px + 1))
        y, y1 = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        lines.append(f"y {strength} {lo} {hi} {luma} {px} {y} {y1}")
        eff = ER.eff_of(ER.config(strength=strength, auto_lo=lo, auto_hi=hi), luma, px)
        want.append(f"{eff} {int(ER.y2_of(np.int64([y]), np.int64([y1]), eff)[0])}")
    for _ in range(600):
        colour, c = int(rng.integers(0, 2)), int(rng.choice([0, 1, 254, 255, int(rng.integers(0, 256))]))
        y, y2 = int(rng.choice([0, 1, 255, int(rng.integers(0, 256))])), int(rng.choice([0, 1, 255, int(rng.integers(0, 256))]))
        lines.append(f"p {colour} {c} {y} {y2}")
        want.append(str(int(ER.colour_of(np.uint8([[[c, c, c]]]), np.int64([[y]]), np.int64([[y2]]), colour)[0, 0, 0])))
    for h, w, pitch, base, wide, ty, tx, seed in walk_cases():
        lines.append(f"h {h} {w} {pitch} {base} {wide} {ty} {tx} {seed}")
        buf = lcg_bytes(base + (h - 1) * pitch + 3 * w, seed)
        fr = np.stack([buf[base + y * pitch:base + y * pitch + 3 * w] for y in range(h)]).reshape(h, w, 3)
        want.append(" ".join(str(int(v)) for v in ER.histograms(fr, ty, tx).ravel()))
    zeros = " ".join(["0"] * 256)
    extra = [f"c 512 5 {zeros}", "1 512 0 0", f"1 512 0 {(1 << 28) + 1}", "1 -1 0 5", "a 5 6", "a 20 17", "a 0 1", "a 16385 1", "e 65281 0 1 0", "e 0 256 1 0",
             "e 0 0 1 8", "i 256 0 0 0 0 0", "i 0 0 0 0 257 0", "y 257 0 0 0 1 0 0", "y 256 9 8 0 1 0 0", "y 256 0 256 0 1 0 0", "p 2 0 0 0", "p 0 256 0 0",
             "h 4 8 24 2 1 1 1 1", "h 4 8 23 0 0 1 1 1", "h 4 8 24 0 0 5 1 1"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(want) + len(extra) + 1 and got[-1] == f"done {len(want) + len(extra)}"
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert g_ == w_, (lines[i][:200], g_[:300], w_[:300])
    assert got[len(want):-1] == ["bad"] * len(extra)


# ---- the library: the host-only entry points, defaults, refusals, exports ----------------------------------------------------------------------
def test_curve_and_axis_entry_points_equal_restatement(pkg):
    EN = pkg.ingestion.enhance
    for hist, n, clip_q8 in curve_cases()[:150] + [(one_bin(3, 1 << 28), 1 << 28, 512)]:
        cur, ex = EN.curve(hist, n, clip_q8)
        w_cur, w_ex, _ = ER.curve(hist, n, clip_q8)
        assert cur.tolist() == w_cur.tolist() and ex == w_ex
    for px, t in [(7, 3), (37, 16), (1, 1), (530, 16), (16384, 16), (150, 8)]:
        k, f, b = EN.axis_table(px, t)
        wk, wf = ER.axis(px, t)
        assert (k.tolist(), f.tolist(), b.tolist()) == (wk.tolist(), wf.tolist(), ER.bounds(px, t))
    E = pkg._ffi.RtmodtError
    for bad in ((np.zeros(256), 0, 512), (one_bin(0, 5), 6, 512), (one_bin(0, 5), 5, -1), (one_bin(0, 5), 5, 65537), (one_bin(0, (1 << 28) + 1), (1 << 28) + 1, 0)):
        with pytest.raises(E) as e:
            EN.curve(*bad)
        assert e.value.code == pkg._ffi.E_INVALID
    for px, t in ((5, 6), (20, 17), (0, 1), (16385, 4), (8, 0)):
        with pytest.raises(E) as e:
            EN.axis_table(px, t)
        assert e.value.code == pkg._ffi.E_INVALID and "tiles" in e.value.msg or "pixels" in e.value.msg
    with pytest.raises(ValueError):
        EN.curve(np.zeros(255), 1, 0)


def test_enhance_cfg_defaults_refusals_and_exports(pkg):
    import ctypes as C
    import inspect
    EN = pkg.ingestion.enhance
    L = pkg._ffi.lib()
    cfg = EN.make_cfg(tiles=None)
    assert {k: getattr(cfg, k) for k in ER.DEFAULTS} == ER.DEFAULTS and (cfg.streams, cfg.height, cfg.width, cfg.device) == (1, 0, 0, 0)
    assert ER.DEFAULTS == dict(tiles_y=8, tiles_x=8, clip_q8=512, strength=256, smooth_shift=2, auto_lo=0, auto_hi=0, colour=0)
    assert EN.clip_q8(2.0) == 512 and EN.clip_q8(0) == 0 and (EN.SHIFT, EN.GAIN) == (ER.SHIFT, ER.GAIN)
    sig = inspect.signature(EN.FrameEnhancer.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[4:]] == [("tiles", (8, 8)), ("clip_limit", 2.0), ("strength", 256), ("smooth_shift", 2), ("auto", (0, 0)),
                                                           ("colour", "shift"), ("device", 0)]
    ok = dict(streams=2, height=37, width=70)
    # a parameter outside its range is refused before the device is touched, and the message names it; the defaults lack a frame size
    for kw, word in ((dict(), "height"), (dict(ok, streams=0), "streams"), (dict(ok, streams=1025), "streams"), (dict(ok, height=16385), "height"),
                     (dict(ok, width=0), "width"), (dict(ok, tiles=(0, 8)), "tiles"), (dict(ok, tiles=(8, 17)), "tiles"), (dict(ok, tiles=(16, 16), height=15), "tiles"),
                     (dict(ok, tiles=(8, 8), width=7), "tiles"), (dict(ok, strength=-1), "strength"), (dict(ok, strength=257), "strength"),
                     (dict(ok, smooth_shift=-1), "smooth_shift"), (dict(ok, smooth_shift=8), "smooth_shift"), (dict(ok, colour=2), "colour"),
                     (dict(ok, colour=-1), "colour"), (dict(ok, auto=(10, 9)), "auto"), (dict(ok, auto=(0, 256)), "auto"), (dict(ok, auto=(-1, 5)), "auto"),
                     (dict(ok, clip_limit=-1.0), "clip_limit"), (dict(ok, clip_limit=256.5), "clip_limit")):
        h = C.c_void_p()
        bad = EN.make_cfg(**kw)
        assert L.rtmodt_enhance_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw
        assert word.encode() in L.rtmodt_last_error(), (kw, L.rtmodt_last_error())
    h = C.c_void_p()
    many = EN.make_cfg(streams=1024, height=64, width=64, tiles=(16, 16))               # 2^18 tiles over all streams
    assert L.rtmodt_enhance_create(C.byref(many), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value
    assert L.rtmodt_enhance_create(None, C.byref(h)) == pkg._ffi.E_INVALID
    assert L.rtmodt_enhance_process(None, None, 0, 0, None, 0, 0, None, 0, 1, 1, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_enhance_reset(None, 0) == pkg._ffi.E_INVALID and L.rtmodt_enhance_histograms(None, 0, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_enhance_read_state(None, 0, None, None) == pkg._ffi.E_INVALID and L.rtmodt_enhance_last_ms(None, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_enhance_load_state(None, 0, None, 0, 0) == pkg._ffi.E_INVALID
    L.rtmodt_enhance_destroy(None)
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        EN.make_cfg(**dict(ok, colour="sepia"))
    assert e.value.code == pkg._ffi.E_INVALID and "colour" in e.value.msg
    assert pkg.ingestion.FrameEnhancer is EN.FrameEnhancer is pkg.FrameEnhancer
    declared = [s for s in pkg._ffi.header_symbols() if s.startswith("rtmodt_enhance_")]
    assert len(declared) == 11 and all(hasattr(L, s) and s in L._signatures for s in declared)
    assert inspect.signature(pkg.pipeline.run).parameters["enhance"].default is None


def test_create_on_a_device_that_cannot_exist(pkg):
    """As tests/test_handle_lifecycle_cpu.py does for the other handles: the create fails at hipSetDevice inside the shared open, the
    half-built handle is released, and what is left of the Python object closes twice and is collected without a sound."""
    E = pkg._ffi.RtmodtError
    shell = None
    with pytest.raises(E) as info:
        try:
            pkg.ingestion.enhance.FrameEnhancer(1, 8, 8, device=1 << 20)
        except E as e:
            tb = e.__traceback__
            while tb is not None:
                me = tb.tb_frame.f_locals.get("self")
                if isinstance(me, pkg._ffi.Handle):
                    shell = me
                tb = tb.tb_next
            raise
    assert info.value.code == pkg._ffi.E_HIP == -3, str(info.value)
    assert "hipSetDevice" in info.value.msg, info.value.msg
    assert shell is not None and not getattr(shell, "_h", None)
    shell.close()
    assert shell._h is None
    shell.close()
    del shell, info
    gc.collect()


# ---- why it is worth having, on the restatements alone ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def premise(with_box, enhanced, n_moving, **cfg):
    """The night scene through motion_ref at its defaults, raw or behind the enhancer at its defaults (but for `cfg`) -> (statuses, moving)"""
    frames, moving = EC.night_sequence(with_box, n_moving=n_moving)
    mo = MR.Ref(1, EC.NIGHT_H, EC.NIGHT_W)
    en = ER.Ref(1, EC.NIGHT_H, EC.NIGHT_W, **cfg)
    return [mo.step(0, en.step(0, f)[0] if enhanced else f)["status"] for f in frames], moving


def test_premise_a_dim_box_moves_unseen_raw_and_seen_enhanced():
    assert EC.BOX_LIFT < MR.DEFAULTS["threshold"]                                       # raw, no cell can differ by more than the box adds
    warm = MR.DEFAULTS["warmup"]
    raw, moving = premise(True, False, EC.NIGHT_MOVING)
    assert raw == [MR.WARMUP] * warm + [MR.STILL] * (len(raw) - warm) and sum(moving) == EC.NIGHT_MOVING
    enh, moving = premise(True, True, EC.NIGHT_MOVING)
    assert enh[:warm] == [MR.WARMUP] * warm
    assert [s for s, m in zip(enh[warm:], moving[warm:]) if not m] == [MR.STILL] * (EC.NIGHT_WARM - warm)
    assert [s for s, m in zip(enh, moving) if m] == [MR.MOTION] * EC.NIGHT_MOVING


def test_premise_the_enhanced_boxless_scene_stays_still_over_100_frames():
    """No flicker-made motion at the default smooth_shift.  (At these amplitudes smooth_shift = 0, a fresh curve per frame, stays STILL
    too: the state is not what keeps THIS scene still; the README says so.)"""
    warm = MR.DEFAULTS["warmup"]
    enh, _ = premise(False, True, 100)
    assert enh == [MR.WARMUP] * warm + [MR.STILL] * (EC.NIGHT_WARM + 100 - warm)
