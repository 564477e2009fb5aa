"""CPU: the snapshot gallery's rules without a GPU.  ``tests/snapshot_ref.py`` (the restatement the kernels of ``csrc/snapshot.hip``
are pinned to) against hand-worked literals; ``csrc/snapshot_rule.h`` against the restatement through
``tests/native/snapshot_rule_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer); the host-only entry point ``rtmodt_snapshot_plan`` against the restatement."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snapshot_ref as R  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "snapshot_rule_check.cpp")


def b32(v):
    return struct.pack(">f", np.float32(v)).hex()


# ---------------------------------------------------------------------------------------------------------------- 1. literals
def test_weights_five_to_two():
    w = R.axis_weights(5, 2)
    assert w.tolist() == [[2, 2, 1, 0, 0], [0, 0, 1, 2, 2]]
    assert R.axis_weights(7, 7).tolist() == (7 * np.eye(7, dtype=np.int64)).tolist()          # D == S: a byte copy
    for S, D in ((9, 4), (1500, 16), (13, 1)):
        assert (R.axis_weights(S, D).sum(1) == S).all() and (R.axis_weights(S, D).sum(0) == D).all()


def test_four_by_four_to_two_by_two_rounds_half_up():
    img = np.zeros((4, 4, 3), np.uint8)
    img[0:2, 0:2, 0] = [[1, 2], [3, 4]]          # 2.5  -> (40 + 8) // 16 = 3
    img[0:2, 2:4, 0] = [[0, 0], [0, 1]]          # 0.25 -> (4 + 8) // 16 = 0
    img[2:4, 0:2, 0] = [[1, 1], [1, 0]]          # 0.75 -> (12 + 8) // 16 = 1
    img[2:4, 2:4, 0] = [[255, 255], [255, 254]]  # 254.75 -> 255
    img[..., 1] = 200
    out = R.resample(img, 2, 2)
    assert out[..., 0].tolist() == [[3, 0], [1, 255]] and (out[..., 1] == 200).all() and (out[..., 2] == 0).all()


def test_copy_with_padding():
    cfg = R.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=1)
    frame = np.arange(20 * 20 * 3, dtype=np.uint32).astype(np.uint8).reshape(20, 20, 3)
    p = R.plan(cfg, [5.9, 5.2, 9.99, 8.0], 20, 20)
    assert (p.raw, p.crop, p.sw, p.sh, p.dw, p.dh, p.ox, p.oy, p.cut, p.area) == ((5, 5, 9, 8), (5, 5, 9, 8), 5, 4, 5, 4, 1, 2, 0, 20)
    t = R.thumbnail(cfg, frame, p)
    assert np.array_equal(t[2:6, 1:6], frame[5:9, 5:10])
    mask = np.ones((8, 8), bool)
    mask[2:6, 1:6] = False
    assert (t[mask] == 114).all()


def test_box_half_outside_the_frame():
    cfg = R.Cfg(thumb_h=16, thumb_w=16, margin_pm=100, min_side=8)
    p = R.plan(cfg, [-10.0, 5.0, 9.0, 14.0], 30, 40)
    assert p.raw == (-10, 5, 9, 14) and p.box == (0, 5, 9, 14) and p.crop == (0, 4, 11, 15)
    assert (p.sw, p.sh, p.dw, p.dh, p.ox, p.oy, p.cut, p.area) == (12, 12, 12, 12, 2, 2, 1, 100)
    assert R.plan(cfg, [-30.0, 5.0, -20.0, 14.0], 30, 40) is None                                # fully outside
    assert R.plan(cfg, [float("nan"), 5.0, 9.0, 14.0], 30, 40) is None and R.plan(cfg, [0.0, 5.0, float("inf"), 14.0], 30, 40) is None
    assert R.plan(cfg, [3.0, 3.0, 8.0, 20.0], 30, 40) is None                                     # 6 + 0 wide < min_side 8
    wide = R.plan(cfg, [0.0, 0.0, 39.0, 9.0], 30, 40)                                             # 40 x 11 (margin 1 row below) -> 16 x 4
    assert (wide.sw, wide.sh, wide.dw, wide.dh, wide.ox, wide.oy) == (40, 11, 16, 4, 0, 6)
    two = R.plan(R.Cfg(thumb_h=16, thumb_w=16, margin_pm=0), [4.0, 4.0, 35.0, 19.0], 30, 40)      # exactly 2 : 1
    assert (two.sw, two.sh, two.dw, two.dh, two.ox, two.oy) == (32, 16, 16, 8, 0, 4)


def test_score_penalties_and_replacement():
    assert R.conf_milli(0.8) == 800 and R.conf_milli(np.float32(0.29)) == 290 and R.conf_milli(float("nan")) == 0
    assert R.conf_milli(1.5) == 1000 and R.conf_milli(-0.5) == 0 and R.conf_milli(None) == 1000 and R.conf_milli(0.0009) == 0
    assert R.score(800, 100, False, False) == 80000 and R.score(800, 100, True, False) == 40000 and R.score(800, 100, True, True) == 20000
    assert R.score(801, 1, True, False) == 400                                                    # a shift, not a division with rounding
    a, b = (0, 0, 9, 9), (5, 0, 14, 9)                                                            # inter 50, union 150: IoU 1 / 3
    assert R.occludes(a, b, 333) and not R.occludes(a, b, 334) and not R.occludes(a, b, 0)
    assert not R.occludes(a, (10, 0, 19, 9), 1) and not R.occludes(a, (5, 5, 4, 9), 1)            # disjoint; empty
    assert not R.replaces(1000, 1000, 0)                                                          # an equal score never rewrites
    assert R.replaces(1001, 1000, 0)
    assert not R.replaces(1100, 1000, 100) and R.replaces(1101, 1000, 100)                        # min_gain_pm at its boundary
    assert R.replaces(1, 0, 10000) and not R.replaces(0, 0, 0)


def test_ledger_keeps_the_best_shot_and_reuses_a_slot_one_call_late():
    cfg = R.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=2, retire_after=1, occl_iou_pm=0, min_gain_pm=0)
    st = R.Stream(cfg, 2)
    frame = np.random.default_rng(0).integers(0, 256, (40, 40, 3), np.uint8)
    big, small = [10.0, 10.0, 19.0, 19.0], [10.0, 10.0, 14.0, 14.0]
    code, upd, ret, _ = st.process([7], [small], [0.5], [0], frame, 0)
    assert code == 0 and upd == [(7, 500 * 25, 0, R.F_NEW, 0)] and ret == []
    code, upd, ret, nrw = st.process([7, 9], [big, small], [0.5, 0.5], [0, 1], frame, 1)
    assert upd == [(7, 500 * 100, 0, R.F_REWRITTEN, 0), (9, 500 * 25, 1, R.F_NEW, 1)] and nrw == 1
    assert np.array_equal(st.atlas[0], R.resample(frame[10:20, 10:20], 8, 8))
    code, upd, ret, nrw = st.process([7, 9], [big, small], [0.5, 0.5], [0, 1], frame, 2)           # equal scores: nothing is rewritten
    assert upd == [] and nrw == 0 and [r.flags for r in st.ledger()] == [0, 0]
    code, upd, ret, _ = st.process([9], [small], [0.4], [1], frame, 3)                              # 7 idle for 1 frame: kept
    assert ret == [] and upd == []
    keep = st.atlas[0].copy()
    code, upd, ret, _ = st.process([9, 11], [small, small], [0.4, 0.4], [1, 2], frame, 4)           # 7 retires; 11 must NOT take slot 0 yet
    assert [r.track_id for r in ret] == [7] and ret[0].slot == 0 and ret[0].best_frame == 1 and ret[0].n_rewrites == 1
    assert upd == [(11, 400 * 25, 2, R.F_NEW, 1)] and np.array_equal(st.atlas[0], keep)
    assert st.bitmap().tolist() == [0b110]
    code, upd, ret, _ = st.process([9, 11, 12], [small, small, small], [0.4, 0.4, 0.4], [1, 2, 3], frame, 5)   # one call later slot 0 is free again
    assert upd == [(12, 400 * 25, 0, R.F_NEW, 2)] and st.bitmap().tolist() == [0b111]
    assert st.process([9], [small], None, [1], frame, 5)[0] == R.E_INVALID                           # frame ids must increase


# ---------------------------------------------------------------------------------------------------------------- 2. the header
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("snapshot_rule_check_san" if sanitize else "snapshot_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built snapshot_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def seeded_frame(h, w, seed):
    k = np.arange(h * w * 3, dtype=np.uint64)
    return (((k * 2654435761 + seed * 40503) & 0xffffffff) >> 24).astype(np.uint8).reshape(h, w, 3)


def plan_line(p):
    return "0" if p is None else "1 " + " ".join(str(v) for v in (*p.raw, *p.box, *p.crop, p.sw, p.sh, p.dw, p.dh, p.ox, p.oy, p.cut, p.area))


@pytest.fixture(scope="module")
def header_cases():
    rng = np.random.default_rng(11)
    lines, want = [], []
    frames = [(61, 97), (1, 1), (3, 2000), (1080, 1920), (40, 1536), (16384, 16384)]
    thumbs = [(16, 16), (24, 40), (8, 512), (512, 8), (96, 96)]
    special = [[0, 0, 1e9, 1e9], [-1e9, -1e9, 1e9, 1e9], [5, 5, 5, 5], [5.5, 5.5, 5.6, 5.6], [10, 10, 9, 20], [float("nan"), 0, 5, 5],
               [0, 0, float("inf"), 5], [-50, -50, -40, -40], [-0.5, -0.5, 0.5, 0.5], [0, 3, 1e7, 3.5]]
    for h, w in frames:
        for th, tw in thumbs:
            boxes = list(special)
            for _ in range(6):
                x0, y0 = rng.uniform(-0.2 * w, w), rng.uniform(-0.2 * h, h)
                boxes.append([x0, y0, x0 + rng.uniform(0, 1.3 * w), y0 + rng.uniform(0, 1.3 * h)])
            boxes.append([0, 0, w - 1, h - 1])
            boxes.append([1, 1, w - 2, h - 2])
            for b in boxes:
                margin, min_side, cap = int(rng.integers(0, 1001)), int(rng.choice([1, 2, 8])), int(rng.choice([1, 1 << 10, 1 << 28]))
                cfg = R.Cfg(thumb_h=th, thumb_w=tw, margin_pm=margin, min_side=min_side, area_cap=cap)
                lines.append(f"p {th} {tw} {margin} {min_side} {cap} {h} {w} " + " ".join(b32(v) for v in b))
                want.append(plan_line(R.plan(cfg, b, h, w)))
    for S, D in ((5, 2), (1, 1), (7, 7), (1500, 16), (16384, 1), (16384, 512), (97, 40), (513, 512)):
        wts = R.axis_weights(S, D)
        parts = []
        for j in range(D):
            nz = np.nonzero(wts[j])[0]
            parts.append(f"{nz[0]} " + " ".join(str(int(v)) for v in wts[j, nz[0]:nz[-1] + 1]))
        lines.append(f"w {S} {D}")
        want.append(" | ".join(parts))
    # whole thumbnails, degenerate crops included: 1 x 1, a frame-wide strip, thumbnails larger than the crop, non-integer ratios
    renders = [((61, 97), (16, 16), 0, 1, [30, 20, 30, 20]), ((61, 97), (16, 16), 0, 1, [0, 30, 96, 30]), ((61, 97), (40, 24), 100, 1, [10, 10, 20, 20]),
               ((61, 97), (16, 16), 0, 1, [0, 0, 96, 60]), ((61, 97), (24, 40), 250, 2, [-20, 7, 55, 58]), ((40, 1536), (16, 16), 0, 1, [18, 0, 1517, 39]),
               ((40, 1536), (24, 40), 0, 1, [18, 3, 1517, 33]), ((33, 35), (8, 8), 0, 1, [1, 1, 33, 31]), ((200, 5), (16, 16), 0, 1, [2, 0, 2, 199])]
    for k, ((h, w), (th, tw), margin, min_side, b) in enumerate(renders):
        cfg = R.Cfg(thumb_h=th, thumb_w=tw, margin_pm=margin, min_side=min_side)
        lines.append(f"r {th} {tw} {margin} {min_side} {h} {w} {k + 3} " + " ".join(b32(v) for v in b))
        p = R.plan(cfg, b, h, w)
        want.append("0" if p is None else "1 " + R.thumbnail(cfg, seeded_frame(h, w, k + 3), p).tobytes().hex())
    for v in (0.0, 0.8, 0.29, 0.999, 0.9999, 1.0, 1.5, -0.5, 0.0009, 0.001, float("nan"), float("inf"), -float("inf"), 1e30, 0.57, 0.07):
        lines.append(f"c {b32(v)}")
        want.append(str(R.conf_milli(v)))
    for cm, area, cut, occl, best, gain in ((800, 100, 0, 0, 80000, 0), (800, 100, 1, 1, 19999, 0), (1000, 1 << 28, 0, 0, (1000 << 28) - 1, 0),
                                            (1000, 1 << 28, 0, 0, 1000 << 28, 10000), (11, 100, 0, 0, 1000, 100), (1101, 1, 0, 0, 1000, 100), (801, 1, 1, 0, 0, 0)):
        s = R.score(cm, area, bool(cut), bool(occl))
        lines.append(f"s {cm} {area} {cut} {occl} {best} {gain}")
        want.append(f"{s} {int(R.replaces(s, best, gain))}")
    for pm, a, b in ((333, (0, 0, 9, 9), (5, 0, 14, 9)), (334, (0, 0, 9, 9), (5, 0, 14, 9)), (0, (0, 0, 9, 9), (0, 0, 9, 9)), (1000, (0, 0, 9, 9), (0, 0, 9, 9)),
                     (1, (0, 0, 9, 9), (10, 0, 19, 9)), (1, (0, 0, 16383, 16383), (16383, 16383, 16383, 16383)), (1, (0, 0, 9, 9), (5, 5, 4, 9))):
        lines.append(f"o {pm} " + " ".join(str(v) for v in (*a, *b)))
        want.append(str(int(R.occludes(a, b, pm))))
    return lines, want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_snapshot_rule_header_equals_restatement(tmp_path, header_cases, sanitize):
    lines, want = header_cases
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines) + 1 and got[-1] == f"done {len(lines)}"
    for k, w in enumerate(want):
        assert got[k] == w, (lines[k][:200], got[k][:400], w[:400])
    assert sum(1 for w in want if w == "0") > 20 and sum(1 for w in want if w.startswith("1 ")) > 200      # both kinds of box


# ---------------------------------------------------------------------------------------------------------------- 3. the library, host only
def test_library_plan_equals_restatement(pkg):
    L, F = pkg._ffi.lib(), pkg._ffi
    rng = np.random.default_rng(5)
    n_sampled = 0
    for (h, w), (th, tw) in (((61, 97), (16, 16)), ((61, 97), (24, 40)), ((1080, 1920), (96, 96)), ((40, 1536), (16, 16)), ((16384, 16384), (512, 8))):
        boxes = [[0, 0, w - 1, h - 1], [5, 5, 5, 5], [float("nan"), 0, 5, 5], [-50, -50, -40, -40], [-1e9, -1e9, 1e9, 1e9]]
        for _ in range(20):
            x0, y0 = rng.uniform(-0.2 * w, w), rng.uniform(-0.2 * h, h)
            boxes.append([x0, y0, x0 + rng.uniform(0, 1.3 * w), y0 + rng.uniform(0, 1.3 * h)])
        for b in boxes:
            margin, min_side = int(rng.integers(0, 1001)), int(rng.choice([1, 2, 8]))
            cfg = F.SnapshotCfg()
            L.rtmodt_snapshot_default_cfg(C.byref(cfg))
            cfg.thumb_h, cfg.thumb_w, cfg.margin_pm, cfg.min_side = th, tw, margin, min_side
            out = F.SnapshotPlan()
            xy = np.asarray(b, np.float32)
            F.check(L.rtmodt_snapshot_plan(C.byref(cfg), F.ptr(xy), h, w, C.byref(out)))
            p = R.plan(R.Cfg(thumb_h=th, thumb_w=tw, margin_pm=margin, min_side=min_side), b, h, w)
            assert bool(out.sampled) == (p is not None), b
            if p is not None:
                n_sampled += 1
                got = (tuple(out.raw), tuple(out.box), tuple(out.crop), out.sw, out.sh, out.dw, out.dh, out.ox, out.oy, out.cut, out.area)
                assert got == (p.raw, p.box, p.crop, p.sw, p.sh, p.dw, p.dh, p.ox, p.oy, p.cut, p.area), b
    assert n_sampled > 60


def test_library_defaults_and_refusals(pkg):
    L, F = pkg._ffi.lib(), pkg._ffi
    cfg = F.SnapshotCfg()
    L.rtmodt_snapshot_default_cfg(C.byref(cfg))
    d = R.Cfg()
    assert (cfg.thumb_h, cfg.thumb_w, cfg.margin_pm, cfg.min_side, cfg.area_cap, cfg.occl_iou_pm, cfg.min_gain_pm, cfg.retire_after, tuple(cfg.pad_bgr)[:3],
            cfg.max_updated, cfg.max_retired) == (d.thumb_h, d.thumb_w, d.margin_pm, d.min_side, d.area_cap, d.occl_iou_pm, d.min_gain_pm, d.retire_after,
                                                  d.pad_bgr, d.max_updated, d.max_retired)
    out, xy = F.SnapshotPlan(), np.float32([0, 0, 5, 5])
    for field, bad in (("thumb_h", 7), ("thumb_w", 513), ("margin_pm", 1001), ("min_side", 0), ("area_cap", 0), ("area_cap", (1 << 28) + 1),
                       ("occl_iou_pm", 1001), ("min_gain_pm", 10001), ("retire_after", -1)):
        c2 = F.SnapshotCfg()
        L.rtmodt_snapshot_default_cfg(C.byref(c2))
        setattr(c2, field, bad)
        assert L.rtmodt_snapshot_plan(C.byref(c2), F.ptr(xy), 10, 10, C.byref(out)) == F.E_INVALID, field
        h = C.c_void_p()
        assert L.rtmodt_snapshot_create(C.byref(c2), 1, 4, C.byref(h)) == F.E_INVALID and not h.value, field      # refused before any HIP call
    assert L.rtmodt_snapshot_plan(C.byref(cfg), F.ptr(xy), 0, 10, C.byref(out)) == F.E_INVALID
    h = C.c_void_p()
    assert L.rtmodt_snapshot_create(C.byref(cfg), 1, 4097, C.byref(h)) == F.E_INVALID and not h.value
