"""CPU: the motion detector's rules without a GPU.  ``tests/motion_ref.py`` (the NumPy restatement the kernels of ``csrc/motion.hip``
are pinned to) against hand-worked literal cases and against its own loop forms and flood fill; the per-cell rule of
``csrc/motion_model.h`` against the restatement, through the host-only entry point ``rtmodt_motion_cell`` and through
``tests/native/motion_model_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer); the same program walks ``csrc/cell_grid.h``, the one reader of frame memory, over
frames that end where their buffer ends.  PARITY UNPINNED: OpenCV's MOG2 and Frigate are installed nowhere this runs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_cases as MC  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "motion_model_check.cpp")


def grey(values):
    v = np.asarray(values, np.uint8)
    return np.repeat(v[:, :, None], 3, 2)


def labelled(mask):
    """components() after checking it against the flood fill."""
    c = MR.components(mask)
    assert c == MR.components_flood(mask)
    return c


# ---- hand-worked literal cases ---------------------------------------------------------------------------------------
def test_luma_and_partial_edge_cells():
    """3 x 5 pixels at scale 2: a 2 x 3 grid whose last column is one pixel wide and whose last row is one pixel high."""
    assert MR.pixel_luma(np.uint8([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]])).tolist() == [[29, 150, 76, 255, 0]]
    fr = grey([[1, 2, 1, 1, 10],
               [2, 2, 2, 2, 11],
               [10, 13, 7, 7, 9]])
    # (7 + 2) // 4 = 2; 1 + 1 + 2 + 2: (6 + 2) // 4 = 2 (half rounds up); two pixels 10, 11: (21 + 1) // 2 = 11;
    # one row 10, 13: (23 + 1) // 2 = 12; the corner cell is the one pixel 9: (9 + 0) // 1
    want = [[2, 2, 11], [12, 7, 9]]
    assert MR.cell_luma(fr, 2).tolist() == want and MR.cell_luma_loop(fr, 2).tolist() == want
    fr = grey([[1, 1, 1], [1, 1, 2], [1, 1, 1]])
    assert MR.cell_luma(fr, 4).tolist() == [[1]]                 # (10 + 4) // 9 = 1
    fr[0, 0] = fr[1, 1] = fr[2, 2] = 2
    assert MR.cell_luma(fr, 8).tolist() == [[1]]                 # (13 + 4) // 9 = 1
    fr[2, 0] = 2
    assert MR.cell_luma(fr, 8).tolist() == [[2]]                 # (14 + 4) // 9 = 2


def one(yc, bg, dev, seen, **kw):
    c = MR.config(**kw)
    raw, b, d = MR.update([[yc]], [[bg]], [[dev]], seen, c)
    got = (bool(raw[0, 0]), int(b[0, 0]), int(d[0, 0]))
    assert got == MR.cell_loop(yc, bg, dev, seen, c)
    return got


def test_update_shifts_a_negative_difference_arithmetically():
    assert one(99, 25600, 0, 3) == (False, 25600 - 16, 16)       # d = -256: -256 >> 4 = -16; dev += (256 - 0) >> 4
    assert one(100, 25601, 0, 3) == (False, 25600, 0)            # d = -1: -1 >> 4 = -1 (floor, not towards zero); (1 - 0) >> 4 = 0
    assert one(100, 25601, 5, 3) == (False, 25600, 4)            # (1 - 5) >> 4 = -1
    assert one(100, 25599, 5, 3) == (False, 25599, 4)            # d = +1: 1 >> 4 = 0
    assert one(37, 999, 777, 0) == (False, 37 * 256, 0)          # the first frame initialises
    assert one(0, 255 * 256, 65535, 1, learn_shift=1) == (False, 32640, 65535 + ((65280 - 65535) >> 1))
    # raw cells: bg moves by d >> learn_shift_fg, dev stays; learn_shift_fg = 0: nothing moves
    assert one(200, 25600, 40, 8) == (True, 25600 + (25600 >> 8), 40)
    assert one(50, 25600, 40, 8) == (True, 25600 + (-12800 >> 8), 40)
    assert one(200, 25600, 40, 8, learn_shift_fg=0) == (True, 25600, 40)
    assert one(200, 25600, 40, 7) == (False, 25600 + (25600 >> 4), 40 + ((25600 - 40) >> 4))        # still warming up: never raw


def test_threshold_is_strict():
    assert one(112, 25600, 0, 8)[0] is False                     # ad = 12 << 8 exactly: > , not >=
    assert one(113, 25600, 0, 8)[0] is True
    assert one(88, 25600, 0, 8)[0] is False and one(87, 25600, 0, 8)[0] is True
    assert one(113, 25600, 128, 8)[0] is False                   # 3072 + 2 * 128 = 3328 = 13 << 8
    assert one(114, 25600, 128, 8)[0] is True
    assert one(113, 25600, 128, 8, dev_gain=0)[0] is True


def test_n3_at_a_grid_corner_and_dilation():
    raw = np.zeros((5, 8), np.uint8)
    raw[:2, :2] = 1                                              # each of the four corner cells sees exactly the four
    for m, l in ((MR.mask_of, "vector"), (MR.mask_loop, "loop")):
        assert m(raw, 4, 0).tolist() == raw.tolist(), l
        assert m(raw, 5, 0).sum() == 0, l
        assert m(raw, 4, 1)[:3, :3].all() and m(raw, 4, 1).sum() == 9, l       # dilation is clipped at the grid's edge
    raw = np.zeros((5, 8), np.uint8)
    raw[2, 2] = raw[2, 5] = 1                                    # two cells with a gap of two
    assert [c[1:] for c in labelled(MR.mask_of(raw, 1, 0))] == [(1, 2, 2, 2, 2), (1, 5, 2, 5, 2)]
    assert [c[1:] for c in labelled(MR.mask_of(raw, 1, 1))] == [(18, 1, 1, 6, 3)]       # 3 x 3 around each: they touch
    assert MR.mask_of(raw, 2, 1).sum() == 0                      # an isolated raw cell has n3 = 1


def test_diagonal_contact_min_area_order_and_truncation():
    m = np.zeros((6, 9), np.uint8)
    m[1, 1] = m[2, 2] = 1                                        # corners touch: one region of two cells
    m[0, 5:8] = 1                                                # three cells, first in raster order
    m[4, 0] = m[5, 1] = m[4, 2] = m[5, 3] = 1                    # a zigzag of four
    comps = labelled(m)
    assert comps == [(5, 3, 5, 0, 7, 0), (10, 2, 1, 1, 2, 2), (36, 4, 0, 4, 3, 5)]
    assert MR.regions_of(m, 1, 32, 4, 22, 35) == ([(20, 0, 32, 4, 3), (4, 4, 12, 12, 2), (0, 16, 16, 22, 4)], 3)    # y1 clipped to h = 22
    assert MR.regions_of(m, 3, 32, 4, 24, 36) == ([(20, 0, 32, 4, 3), (0, 16, 16, 24, 4)], 2)      # min_area - 1 = 2 cells: dropped
    assert MR.regions_of(m, 4, 32, 4, 24, 36) == ([(0, 16, 16, 24, 4)], 1)
    assert MR.regions_of(m, 1, 2, 1, 6, 9) == ([(5, 0, 8, 1, 3), (1, 1, 3, 3, 2)], 3)              # truncated in raster order; the total stays
    assert MR.regions_of(m, 5, 2, 1, 6, 9) == ([], 0)
    assert MR.mask_box(m, 4, 22, 35) == (0, 0, 32, 22) and MR.mask_box(m * 0, 4, 22, 35) == (0, 0, 0, 0)
    assert MR.block_grid(m, 4).tolist() == [[2, 3, 0], [4, 0, 0]]


def test_scene_change_at_equality_and_reinitialisation():
    c = MR.config(scene_pm=600, warmup=2)
    assert MR.status_of(2, 6, 10, 0, c) == MR.SCENE_CHANGE      # 6000 >= 6000
    assert MR.status_of(2, 5, 10, 1, c) == MR.MOTION and MR.status_of(2, 5, 10, 0, c) == MR.STILL
    assert MR.status_of(1, 10, 10, 1, c) == MR.WARMUP            # warm-up wins
    assert MR.next_seen(5, MR.SCENE_CHANGE) == 0 and MR.next_seen(5, MR.STILL) == 6 and MR.next_seen(2 ** 30, MR.MOTION) == 2 ** 30
    ref = MR.Ref(1, 4, 20, scale=2, warmup=2, min_neighbors=1, dilate=0, min_area=1, scene_pm=600)     # a 2 x 10 grid
    flat = np.full((2, 10), 100, np.uint8)
    assert [ref.step(0, MC.cells_to_frame(flat, 2, 4, 20))["status"] for _ in range(3)] == [MR.WARMUP, MR.WARMUP, MR.STILL]
    lit = flat.copy()
    lit[0, :6] = lit[1, :5] = 180                                # 11 of 20 cells: 11000 < 12000
    r = ref.step(0, MC.cells_to_frame(lit, 2, 4, 20))
    assert (r["status"], r["n_raw"], r["n_regions_total"], r["frames_seen"]) == (MR.MOTION, 11, 1, 4)
    lit[1, 5] = 180                                              # 12 of 20: equality
    r = ref.step(0, MC.cells_to_frame(lit, 2, 4, 20))
    assert (r["status"], r["n_raw"], r["frames_seen"]) == (MR.SCENE_CHANGE, 12, 0)
    r = ref.step(0, MC.cells_to_frame(lit, 2, 4, 20))            # the next frame re-initialises: the lit scene is the background now
    assert (r["status"], r["n_raw"], r["frames_seen"]) == (MR.WARMUP, 0, 1)
    assert ref.bg[0].tolist() == (lit.astype(np.int64) << 8).tolist() and not ref.dev[0].any()
    assert [ref.step(0, MC.cells_to_frame(lit, 2, 4, 20))["status"] for _ in range(2)] == [MR.WARMUP, MR.STILL]


def test_shapes_are_what_they_claim():
    for gh, gw in ((150, 530), (38, 133), (7, 5)):
        for name in ("spiral", "comb", "diagonal", "full"):
            m = MC.SHAPES[name](gh, gw)
            comps = MR.components(m)
            assert len(comps) == 1 and comps[0][1] == int(m.sum()) and comps[0][2:] == (0, 0, gw - 1, gh - 1), (name, gh, gw)
        assert MC.spiral(gh, gw).sum() > gh * gw // 3 and MC.diagonal(gh, gw).sum() == max(gh, gw)
    assert labelled(MC.spiral(38, 133)) and labelled(MC.comb(9, 12)) and labelled(MC.diagonal(38, 133))


# ---- the vectorised form against the loop form -------------------------------------------------------------------------
def test_restatement_equals_its_loop_forms_on_random_scenes():
    rng = np.random.default_rng(2031)
    for i in range(24):
        h, w = [(37, 70), (19, 50), (9, 33), (16, 16)][i % 4]
        scale = [1, 2, 4, 8][(i // 4) % 4]
        fr = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        yc = MR.cell_luma(fr, scale)
        if i % 3 == 0 or scale > 1:
            assert yc.tolist() == MR.cell_luma_loop(fr, scale).tolist()
        c = MR.config(learn_shift=int(rng.integers(1, 9)), learn_shift_fg=int(rng.choice([0, 8, 12])), threshold=int(rng.integers(1, 40)),
                      dev_gain=int(rng.integers(0, 9)), warmup=int(rng.integers(1, 6)))
        bg = rng.integers(0, 65281, yc.shape)
        dev = rng.integers(0, 3000, yc.shape)
        for seen in (0, c["warmup"] - 1, c["warmup"], 2 ** 30):
            raw, b, d = MR.update(yc, bg, dev, seen, c)
            loop = [MR.cell_loop(yc[y, x], bg[y, x], dev[y, x], seen, c) for y in range(yc.shape[0]) for x in range(yc.shape[1])]
            assert list(zip(raw.ravel().tolist(), b.ravel().tolist(), d.ravel().tolist())) == loop
            assert b.min() >= 0 and b.max() <= 65280 and d.min() >= 0 and d.max() <= 65535
        raw = rng.random(yc.shape) < [0.1, 0.3, 0.6][i % 3]
        for mn, dl in ((1, 0), (3, 1), (2, 2), (9, 3), (5, 1)):
            m = MR.mask_of(raw, mn, dl)
            assert m.tolist() == MR.mask_loop(raw, mn, dl).tolist()
            labelled(m)


# ---- the per-cell rule of the library ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_cases():
    """(learn_shift, learn_shift_fg, threshold, dev_gain, warmup, yc, frames_seen, bg, dev)"""
    rng = np.random.default_rng(2032)
    out = []
    for i in range(4000):
        ls = int(rng.integers(1, 9))
        fg = int(rng.choice([0, ls, 12, int(rng.integers(ls, 13))]))
        warm = int(rng.choice([1, 2, 8, 255]))
        seen = int(rng.choice([0, 1, warm - 1, warm, warm + 1, 2 ** 30]))
        yc = int(rng.choice([0, 255, int(rng.integers(0, 256))]))
        bg = int(rng.choice([0, 65280, yc * 256, max(0, yc * 256 - 1), min(65280, yc * 256 + 1), int(rng.integers(0, 65281))]))
        dev = int(rng.choice([0, 0, 65535, int(rng.integers(0, 300)), int(rng.integers(0, 4000)), int(rng.integers(0, 65536))]))
        thr = int(rng.choice([1, 6, 12, 40, 255, int(rng.integers(1, 256))]))
        out.append((ls, fg, thr, int(rng.integers(0, 9)), warm, yc, seen, bg, dev))
    return out


def ref_cell(case):
    ls, fg, thr, gain, warm, yc, seen, bg, dev = case
    raw, b, d = MR.cell_loop(yc, bg, dev, seen, MR.config(learn_shift=ls, learn_shift_fg=fg, threshold=thr, dev_gain=gain, warmup=warm))
    return int(raw), b, d


def test_motion_cell_entry_point_equals_restatement(pkg):
    M = pkg.detection.motion
    n_raw = 0
    for case in cell_cases():
        ls, fg, thr, gain, warm, yc, seen, bg, dev = case
        b, d, raw = M.motion_cell(yc, seen, bg, dev, learn_shift=ls, learn_shift_fg=fg, threshold=thr, dev_gain=gain, warmup=warm)
        assert (int(raw), b, d) == ref_cell(case), case
        n_raw += raw
    assert 400 < n_raw < 3600, n_raw                             # both outcomes are well covered
    for bad in (dict(learn_shift=0), dict(learn_shift=9), dict(learn_shift=4, learn_shift_fg=3), dict(learn_shift_fg=13), dict(threshold=0),
                dict(threshold=256), dict(dev_gain=-1), dict(dev_gain=9), dict(warmup=0), dict(warmup=256)):
        with pytest.raises(pkg._ffi.RtmodtError) as e:
            M.motion_cell(10, 1, 0, 0, **bad)
        assert e.value.code == pkg._ffi.E_INVALID, bad
    with pytest.raises(pkg._ffi.RtmodtError):
        M.motion_cell(256, 1, 0, 0)


def test_motion_cfg_defaults_and_ranges(pkg):
    import ctypes as C
    M = pkg.detection.motion
    L = pkg._ffi.lib()
    cfg = M.make_cfg()
    got = {f: getattr(cfg, f) for f, _ in cfg._fields_}
    assert got == dict(MR.DEFAULTS, streams=1, height=0, width=0, device=0)
    ok = dict(streams=2, height=37, width=70)
    # a parameter outside its range is refused before the device is touched (this machine has none); the defaults lack a frame size
    for kw in (dict(), dict(ok, streams=0), dict(ok, streams=1025), dict(ok, height=0), dict(ok, width=32769), dict(ok, scale=0), dict(ok, scale=3),
               dict(ok, scale=16), dict(ok, learn_shift=0), dict(ok, learn_shift=9), dict(ok, learn_shift_fg=3), dict(ok, learn_shift_fg=13),
               dict(ok, threshold=0), dict(ok, threshold=256), dict(ok, dev_gain=-1), dict(ok, dev_gain=9), dict(ok, min_neighbors=0),
               dict(ok, min_neighbors=10), dict(ok, dilate=-1), dict(ok, dilate=4), dict(ok, warmup=0), dict(ok, warmup=256), dict(ok, scene_pm=0),
               dict(ok, scene_pm=1001), dict(ok, min_area=0), dict(ok, max_regions=0), dict(ok, max_regions=257), dict(ok, block=2), dict(ok, block=12),
               dict(ok, block=64)):
        h = C.c_void_p()
        bad = M.make_cfg(**kw)
        assert L.rtmodt_motion_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw
    h = C.c_void_p()
    big = M.make_cfg(streams=1, height=8192, width=8192, scale=1)            # 2^26 cells
    assert L.rtmodt_motion_create(C.byref(big), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value
    assert b"cells" in L.rtmodt_last_error()
    with pytest.raises(TypeError):
        M.make_cfg(cell=4)
    assert pkg.MotionDetector is M.MotionDetector and "MotionDetector" in pkg.detection.__all__


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("motion_model_check_san" if sanitize else "motion_model_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built motion_model_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def lcg_bytes(n, seed):
    x = int(seed)
    out = np.empty(n, np.uint8)
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        out[i] = x >> 24
    return out


def lcg_frame(h, w, seed):
    return lcg_bytes(h * w * 3, seed).reshape(h, w, 3)


def reader_cases():
    """(scale, h, w, pitch, base_offset, wide, seed): the smallest shapes that reach every branch of cell_grid.h's reader.  With PX the
    pixels of a thread's run (4, at scale 8: 8), w = PX - 1 is one partial run, 2 PX two full runs, 2 PX + 1 two full runs and a run of
    one pixel; h = scale is full cell rows only, scale + 1 adds a cell row one pixel high.  A pitch of 3w puts the frame's last byte
    at the buffer's last byte.  The dword path is taken only as the host takes it: an aligned pitch and base."""
    out = []
    for scale in (1, 2, 4, 8):
        px = 8 if scale == 8 else 4
        for w in (px - 1, 2 * px, 2 * px + 1):
            for h in (scale, scale + 1):
                aligned = (3 * w + 3) // 4 * 4
                for pitch in dict.fromkeys((3 * w, 3 * w + 1, aligned)):
                    out += [(scale, h, w, pitch, base, 0) for base in (0, 1)]
                out += [(scale, h, w, aligned, base, 1) for base in (0, 4)]
    return [c + (100 + i,) for i, c in enumerate(out)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_motion_model_header_equals_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    cases = cell_cases()
    lines = ["c " + " ".join(str(v) for v in c) for c in cases]
    want = [" ".join(str(v) for v in ref_cell(c)) for c in cases]
    frames = [(1, 5, 7, 1), (2, 5, 7, 2), (4, 9, 13, 3), (8, 9, 13, 4), (8, 17, 16, 5), (2, 1, 1, 6), (4, 37, 70, 7)]
    for scale, h, w, seed in frames:
        lines.append(f"f {scale} {h} {w} {seed}")
        yc = MR.cell_luma(lcg_frame(h, w, seed), scale)
        want.append(" ".join(str(v) for v in [yc.shape[1], yc.shape[0]] + yc.ravel().tolist()))
    for scale, h, w, pitch, base, wide, seed in reader_cases():
        lines.append(f"r {scale} {h} {w} {pitch} {base} {wide} {seed}")
        buf = lcg_bytes(base + (h - 1) * pitch + 3 * w, seed)
        fr = np.stack([buf[base + y * pitch:base + y * pitch + 3 * w] for y in range(h)]).reshape(h, w, 3)
        yc = MR.cell_luma(fr, scale)
        want.append(" ".join(str(v) for v in [yc.shape[1], yc.shape[0]] + yc.ravel().tolist()))
    for box in ((0, 0, 0, 0, 4, 35, 22), (1, 2, 8, 5, 4, 35, 22), (3, 1, 7, 2, 8, 64, 24), (0, 0, 69, 36, 1, 70, 37), (2, 2, 2, 2, 2, 5, 5)):
        lines.append("b " + " ".join(str(v) for v in box))
        want.append(" ".join(str(v) for v in MR.px_box(*box[:5], box[6], box[5])))
    for seen, warm, n_raw, pm, cells, total in ((0, 8, 0, 600, 100, 0), (7, 8, 100, 600, 100, 3), (8, 8, 60, 600, 100, 0), (8, 8, 59, 600, 100, 0),
                                                (8, 8, 59, 600, 100, 2), (2 ** 30, 1, 0, 1, 2 ** 24, 0), (2 ** 30, 255, 2 ** 24, 1000, 2 ** 24, 9),
                                                (9, 8, 1, 1, 1000, 0), (9, 8, 1, 1, 1001, 0)):
        lines.append(f"s {seen} {warm} {n_raw} {pm} {cells} {total}")
        st = MR.status_of(seen, n_raw, cells, total, MR.config(warmup=warm, scene_pm=pm))
        want.append(f"{st} {MR.next_seen(seen, st)}")
    extra = ["c 0 8 12 2 8 10 1 0 0", "c 4 3 12 2 8 10 1 0 0", "c 4 8 12 2 8 256 1 0 0", "c 4 8 12 2 8 10 1 65536 0", "f 3 5 5 1", "b 0 0 1 1 5 10 10",
             "r 3 5 5 15 0 0 1", "r 4 5 5 14 0 0 1", "r 4 5 5 18 0 1 1", "r 4 5 5 16 1 1 1"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(want) + len(extra) + 1 and got[-1] == f"done {len(want) + len(extra)}"
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, (lines[i], g[:200], w_[:200])
    assert got[len(want):-1] == ["bad"] * len(extra)
