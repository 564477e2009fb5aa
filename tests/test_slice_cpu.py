"""CPU: the rules of sliced inference (csrc/slice.hip) without a GPU -- the grid's worked values and its
coverage over a sweep, the library's host-only grid entry against the restatement (tests/slice_ref.py), the merge on hand-worked
cases whose expected outputs are written out here (not computed by the restatement), the overview's round trip, the refusals
that happen before any device call, and csrc/slice_grid.h under the address / undefined-behaviour sanitizers as a stand-alone
program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slice_ref as R  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

F32 = np.float32
SRC = os.path.join(ROOT, "tests", "native", "slice_grid_check.cpp")


# ------------------------------------------------------------------ grid
def test_worked_grid_values():
    assert R.axis(1920, 640, 128) == ([0, 512, 1024, 1280], 640)
    assert R.axis(1080, 640, 128) == ([0, 440], 640)
    assert R.axis(640, 640, 128) == ([0], 640)
    assert R.axis(50, 64, 16) == ([0], 50)
    tiles, te = R.grid(1920, 1080, 640, 640, 128, 128)
    assert te == (640, 640) and len(tiles) == 8                    # 9 images with the overview
    assert tiles == [(0, 0), (512, 0), (1024, 0), (1280, 0), (0, 440), (512, 440), (1024, 440), (1280, 440)]


SWEEP = [(L, t, o) for L in list(range(1, 70)) + [97, 128, 300, 641, 1080, 1920] for t in (1, 2, 7, 16, 33, 64, 640) for o in (0, 1, 5, 15, 32, 128) if o < t]


def test_every_grid_covers_the_axis_inside_the_frame():
    for L, t, o in SWEEP:
        pos, te = R.axis(L, t, o)
        assert te == min(t, L) and pos[0] == 0 and pos == sorted(set(pos)), (L, t, o)
        assert all(0 <= p and p + te <= L for p in pos), (L, t, o)
        cov = np.zeros(L, bool)
        for p in pos:
            cov[p:p + te] = True
        assert cov.all() and pos[-1] + te == L, (L, t, o)
        assert all(b - a <= te for a, b in zip(pos, pos[1:])), (L, t, o)          # no gap between neighbours


def lib_grid(F, W, H, tw, th, ow, oh):
    xs, ys = np.full(64, -1, np.int32), np.full(64, -1, np.int32)
    n, a, b = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = F.lib().rtmodt_slice_grid(W, H, tw, th, ow, oh, F.ptr(xs), F.ptr(ys), C.byref(n), C.byref(a), C.byref(b))
    return rc, [(int(xs[i]), int(ys[i])) for i in range(max(n.value, 0))], (a.value, b.value)


def test_library_grid_equals_the_restatement(pkg):
    """The host-only entry point: the library loads and answers without a GPU, as the ABI tests rely on."""
    F = pkg._ffi
    done = 0
    for i, (L, t, o) in enumerate(SWEEP):
        L2, t2, o2 = SWEEP[(i * 7 + 3) % len(SWEEP)]
        if len(R.axis(L, t, o)[0]) * len(R.axis(L2, t2, o2)[0]) > 64:
            assert lib_grid(F, L, L2, t, t2, o, o2)[0] == F.E_CAPACITY
            continue
        rc, tiles, te = lib_grid(F, L, L2, t, t2, o, o2)
        assert rc == 0 and (tiles, te) == R.grid(L, L2, t, t2, o, o2), (L, L2, t, t2, o, o2)
        done += 1
    assert done > 300
    assert pkg.detection.sliced.slice_grid((1920, 1080)) == R.grid(1920, 1080, 640, 640, 128, 128)
    for bad in ((100, 100, 64, 64, 64, 0), (100, 100, 64, 64, 0, 70), (0, 100, 64, 64, 0, 0), (100, 100, 0, 64, 0, 0), (100, 100, 64, 64, -1, 0)):
        assert lib_grid(F, *bad)[0] == F.E_INVALID and F.lib().rtmodt_last_error()
    assert lib_grid(F, 513, 512, 64, 64, 0, 0)[0] == F.E_CAPACITY
    assert F.lib().rtmodt_slice_grid(1920, 1080, 640, 640, 128, 128, None, None, None, None, None) == 0      # every output is optional


def test_create_refusals_come_before_any_device_call(pkg):
    F = pkg._ffi
    S = pkg.detection.sliced
    h = C.c_void_p()

    def create(max_det=100, **kw):
        cfg = S.slice_cfg(kw.pop("frame_size", (1920, 1080)), **kw)
        return F.lib().rtmodt_slicer_create(C.byref(cfg), max_det, C.byref(h))

    assert create(overlap=(640, 128)) == F.E_INVALID and b"overlap" in F.lib().rtmodt_last_error()
    assert create(overlap=(128, 700)) == F.E_INVALID
    assert create(max_out=0) == F.E_INVALID and create(max_det=0) == F.E_INVALID
    assert create(max_det=1000) == F.E_CAPACITY and b"9 images x max_det 1000" in F.lib().rtmodt_last_error()     # 9000 > 8192 candidates
    assert create(max_frames=8) == F.E_CAPACITY                                                                   # 72 images > a detector batch
    assert create(frame_size=(6400, 6400), overlap=(0, 0)) == F.E_CAPACITY                                        # 100 tiles
    assert not h.value
    cfg = S.slice_cfg((1920, 1080))
    cfg.merge = 2
    assert F.lib().rtmodt_slicer_create(C.byref(cfg), 100, C.byref(h)) == F.E_INVALID
    with pytest.raises(ValueError):
        S.slice_cfg((1920, 1080), merge="wbf")
    assert C.sizeof(F.SliceCfg) == 56


# ------------------------------------------------------------------ merge: hand-worked literals
# frame 128 x 128, tile 64, overlap 0: tiles at (0, 0), (64, 0), (0, 64), (64, 64); the overview is the frame at gain 0.5, pad 0
GEOM = (128, 128, 64, 64, 0, 0)
NONE = (np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32))


def img(*dets):
    """(box, conf, cls) triples -> one image's detections."""
    return (np.array([d[0] for d in dets], F32).reshape(-1, 4), np.array([d[1] for d in dets], F32), np.array([d[2] for d in dets], np.int32))


def run(images, **kw):
    xy, cf, cl, nm = R.merge(R.to_frame(images, *GEOM, overview=len(images) == 5), **kw)
    return xy.tolist(), [round(float(c), 6) for c in cf], cl.tolist(), nm.tolist()


FRAGMENTS = [img(((30, 20, 64, 40), 0.8, 1)),            # tile 0: the left part of an object cut at x = 64
             img(((0, 22, 26, 42), 0.7, 1)),             # tile 1: its right part -> frame (64, 22, 90, 42)
             NONE, NONE,
             img(((16, 10, 44, 20), 0.9, 1))]            # overview: the whole object -> frame (32, 20, 88, 40), area 1120


def test_two_fragments_and_an_overview_box_merge_into_their_union():
    # IoS of the overview box with the left part: 32 * 20 / 680, with the right part: 24 * 18 / 520 -- both above 0.5
    assert run(FRAGMENTS, mode=R.NMM, metric=R.IOS) == ([[30.0, 20.0, 90.0, 42.0]], [0.9], [1], [2])
    # the fragments alone only touch (iw = 0): nothing merges
    assert run(FRAGMENTS[:4], mode=R.NMM, metric=R.IOS) == ([[30.0, 20.0, 64.0, 40.0], [64.0, 22.0, 90.0, 42.0]], [0.8, 0.7], [1, 1], [0, 0])


def test_the_same_under_nms_keeps_the_overview_box_itself():
    assert run(FRAGMENTS, mode=R.NMS, metric=R.IOS) == ([[32.0, 20.0, 88.0, 40.0]], [0.9], [1], [2])
    # IoU of the overview box with the parts is 640 / 1160 and 432 / 1208: only the left part goes
    assert run(FRAGMENTS, mode=R.NMS, metric=R.IOU) == ([[32.0, 20.0, 88.0, 40.0], [64.0, 22.0, 90.0, 42.0]], [0.9, 0.7], [1, 1], [1, 0])


def test_a_score_tie_is_decided_by_image_then_slot():
    images = [img(((10, 10, 30, 30), 0.6, 3)), NONE, NONE, NONE, img(((5, 5, 15, 15), 0.6, 7))]      # the same frame box twice
    assert run(images, agnostic=True) == ([[10.0, 10.0, 30.0, 30.0]], [0.6], [3], [1])                 # image 0 before image 4
    images = [NONE, NONE, img(((0, 0, 20, 20), 0.5, 4), ((1, 1, 21, 21), 0.5, 5)), NONE, NONE]         # tile 2 at (0, 64)
    assert run(images, agnostic=True, mode=R.NMS) == ([[0.0, 64.0, 20.0, 84.0]], [0.5], [4], [1])       # slot 0 before slot 1


def test_equal_boxes_of_different_classes():
    images = [img(((10, 10, 30, 30), 0.9, 0), ((10, 10, 30, 30), 0.8, 1)), NONE, NONE, NONE]
    assert run(images) == ([[10.0, 10.0, 30.0, 30.0]] * 2, [0.9, 0.8], [0, 1], [0, 0])
    assert run(images, agnostic=True) == ([[10.0, 10.0, 30.0, 30.0]], [0.9], [0], [1])


def test_a_zero_area_box_matches_nothing():
    line, big = (10, 10, 10, 30), (5, 5, 40, 40)                  # the zero-area box lies inside the other one
    for metric in (R.IOS, R.IOU):
        # as the keeper (IoS: min area 0, the denominator is not positive) and as the candidate (inter = 0, 0 > 0 is false)
        assert run([img((line, 0.9, 0), (big, 0.8, 0)), NONE, NONE, NONE], metric=metric, thresh=0.0) == (
            [[10.0, 10.0, 10.0, 30.0], [5.0, 5.0, 40.0, 40.0]], [0.9, 0.8], [0, 0], [0, 0])
        assert run([img((line, 0.8, 0), (big, 0.9, 0)), NONE, NONE, NONE], metric=metric, thresh=0.0) == (
            [[5.0, 5.0, 40.0, 40.0], [10.0, 10.0, 10.0, 30.0]], [0.9, 0.8], [0, 0], [0, 0])


def test_max_out_truncates_in_order():
    images = [img(((0, 0, 10, 10), 0.3, 0), ((20, 0, 30, 10), 0.9, 0)), img(((0, 0, 10, 10), 0.5, 0)), NONE, NONE]
    assert run(images, max_out=2) == ([[20.0, 0.0, 30.0, 10.0], [64.0, 0.0, 74.0, 10.0]], [0.9, 0.5], [0, 0], [0, 0])
    assert len(run(images, max_out=3)[0]) == 3 and len(run(images, max_out=1)[0]) == 1


def test_a_metric_equal_to_the_threshold_does_not_match():
    ios = [img(((0, 0, 20, 20), 0.9, 0), ((10, 0, 30, 20), 0.8, 0)), NONE, NONE, NONE]           # 200 / min(400, 400) = 0.5
    assert run(ios, metric=R.IOS, thresh=0.5)[3] == [0, 0]
    assert run(ios, metric=R.IOS, thresh=0.49) == ([[0.0, 0.0, 30.0, 20.0]], [0.9], [0], [1])
    iou = [img(((0, 0, 30, 10), 0.9, 0), ((10, 0, 40, 10), 0.8, 0)), NONE, NONE, NONE]           # 200 / (300 + 300 - 200) = 0.5
    assert run(iou, metric=R.IOU, thresh=0.5)[3] == [0, 0]
    assert run(iou, metric=R.IOU, thresh=0.49)[3] == [1]


def test_overview_round_trip_is_within_a_pixel():
    """A frame box drawn where LetterBox puts it (x * uw / W + left) and mapped back by to_frame (scale_boxes) lands within 1 px
    on the geometries this feature is specified and measured on.  In general scale_boxes is not LetterBox's exact inverse, and the
    bound follows from the two roundings it does not share with it: its pad round((te - L * gain) / 2 - 0.1) may differ from
    LetterBox's round((te - round(L * gain)) / 2 - 0.1) by one letterbox pixel, and uw = round(W * gain) is off W * gain by at
    most half of one -- 1.5 letterbox pixels, 1.5 / gain frame pixels, asserted on every geometry (97 x 83 and 50 x 40 reach
    1.4 px: there the pads differ)."""
    rng = np.random.default_rng(4)
    for W, H, t in ((1920, 1080, 640), (1280, 720, 640), (560, 480, 320), (97, 83, 64), (50, 40, 64)):
        bound = 1.0 if W >= 560 else None
        tiles, (te_w, te_h) = R.grid(W, H, t, t, t // 5, t // 5)
        uw, uh, top, _, left, _ = R.Y.letterbox_params(H, W, te_h, te_w)
        images = [NONE for _ in tiles]
        boxes = []
        for _ in range(50):
            x1, y1 = rng.uniform(0, W - 2), rng.uniform(0, H - 2)
            boxes.append((x1, y1, rng.uniform(x1 + 1, W), rng.uniform(y1 + 1, H)))
        boxes.append((0.0, 0.0, float(W), float(H)))
        inside = [((b[0] * uw / W + left, b[1] * uh / H + top, b[2] * uw / W + left, b[3] * uh / H + top), 0.5, 0) for b in boxes]
        back = R.to_frame(images + [img(*inside)], W, H, t, t, t // 5, t // 5)
        assert len(back) == len(boxes)
        gain = min(te_h / H, te_w / W)
        for (b, _, _, j, _), want in zip(back, boxes):
            err = np.abs(b.astype(np.float64) - np.array(want)).max()
            assert j == len(tiles) and err <= 1.5 / gain + 1e-3, (W, H, b, want)
            assert bound is None or err <= bound, (W, H, b, want)


# ------------------------------------------------------------------ slice_grid.h on the host, plain and sanitized
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("slice_grid_check_san" if sanitize else "slice_grid_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built slice_grid_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_slice_grid_header_on_the_host(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert [l.split()[1] for l in lines if l.startswith("ok ")] == ["worked", "axes", "grid", "tables", "letterbox"]
    assert lines[-1] == "all ok" and not any(l.startswith("FAIL") for l in lines)
