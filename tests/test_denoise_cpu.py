"""CPU: the frame denoiser's rules.  ``tests/denoise_ref.py`` against hand-worked literals (each deliberate defect fails at least one),
its vectorised form against its per-pixel loop, the properties the rule header states (``acc`` needs no clamp, the identity settings, the
fixed point), ``csrc/denoise_rule.h`` through a stand-alone program built plain and under the address / UB sanitizers, the library's
host-only entry point and refusals, and the premise on restatements alone: on the enhancer's night scene under sensor noise the filter
gains the derived PSNR, shrinks the JPEG, leaves no trail behind a moving box and changes no motion status.  PARITY UNPINNED: no other
denoiser is compared."""
import functools
import gc
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_cases as DC  # noqa: E402
import denoise_ref as DR  # noqa: E402
import enhance_cases as EC  # noqa: E402
import enhance_ref as ER  # noqa: E402
import jpeg_ref  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "denoise_rule_check.cpp")


def grey(rows):
    return np.array(rows, np.uint8)[..., None].repeat(3, 2)


def run(frames, defect=None, **cfg):
    """The frames of one stream through the restatement -> [(grey output rows, acc of channel 0, a, row)]"""
    ref = DR.Ref(1, len(frames[0]), len(frames[0][0]), defect=defect, **cfg)
    out = []
    for f in frames:
        o, row = ref.step(0, grey(f))
        assert (o[..., 0] == o[..., 1]).all() and (o[..., 0] == o[..., 2]).all()
        out.append((o[..., 0].tolist(), ref.acc[0][..., 0].tolist(), ref.a[0].tolist(), row))
    return out


# ---- hand-worked literals -------------------------------------------------------------------------------------------------------------
def literal_one_pixel_of_the_issue(defect=None):
    """100; 116: D = 9 * 16 = 144 >= 54, a = 256, w = 256; 118: D = 18 <= 18, a = 0, w = 32, acc = 29696 + ((512 * 32 + 128) >> 8)."""
    s = run([[[100]], [[116]], [[118]]], defect)
    assert [(o, acc, a) for o, acc, a, _ in s] == [([[100]], [[25600]], [[256]]), ([[116]], [[29696]], [[256]]), ([[116]], [[29760]], [[0]])]
    assert s[2][3] == dict(stream=0, frames_seen=3, n_static=1, n_moving=0, absdiff_static=2)
    # 119 in place of 118: D = 27, a = 9 * 256 // 36 = 64, w = 32 + 56 = 88, acc = 29696 + ((768 * 88 + 128) >> 8) = 29960
    s = run([[[100]], [[116]], [[119]]], defect)
    assert s[2][:3] == ([[117]], [[29960]], [[64]]) and (s[2][3]["n_static"], s[2][3]["n_moving"]) == (0, 0)


def literal_first_frame_passes(defect=None):
    """A black first frame: D = 0, and still a = 256 -- the pixel counts as moving, not static."""
    s = run([[[0]]], defect)
    assert s[0] == ([[0]], [[0]], [[256]], dict(stream=0, frames_seen=1, n_static=0, n_moving=1, absdiff_static=0))


def literal_rounding(defect=None):
    """100 then 105: D = 45, a = 27 * 256 // 36 = 192, w = 32 + ((224 * 192 + 128) >> 8) = 200,
    acc = 25600 + ((1280 * 200 + 128) >> 8) = 26600 = 103 * 256 + 232, out = (26600 + 128) >> 8 = 104."""
    s = run([[[100]], [[105]]], defect)
    assert s[1][:3] == ([[104]], [[26600]], [[192]])


def literal_clamp_at_the_border(defect=None):
    """1 x 2, 100 100 then 104 100: dY = 4 0.  Left pixel: the clamp makes three rows of (4, 4, 0), D = 24, a = 6 * 256 // 36 = 42; zeros
    outside would give D = 4.  Its sigma filter takes both pixels, s = (204 + 1) // 2 = 102, xs = 104 + ((-2 * 42 * 256 + 32768) >> 16) = 104;
    w = 32 + ((224 * 42 + 128) >> 8) = 69, acc = 25600 + ((1024 * 69 + 128) >> 8) = 25876, out = 101.  Right pixel: D = 12, a = 0."""
    s = run([[[100, 100]], [[104, 100]]], defect)
    assert s[1][:3] == ([[101, 100]], [[25876, 25600]], [[42, 0]])
    assert s[1][3] == dict(stream=0, frames_seen=2, n_static=1, n_moving=0, absdiff_static=0)


def literal_noise_cancels_in_the_sum(defect=None):
    """1 x 2, 100 100 then 104 96: dY = 4 -4.  Left: 3 * (4 + 4 - 4) = 12, right: |3 * (4 - 4 - 4)| = 12: both static; the sum of absolute
    values would be 36.  a = 0: w = 32, acc = 25600 +- ((1024 * 32 + 128) >> 8): 25728 and, by the floor of the negative value, 25472."""
    s = run([[[100, 100]], [[104, 96]]], defect)
    assert s[1][:3] == ([[101, 100]], [[25728, 25472]], [[0, 0]])
    assert s[1][3] == dict(stream=0, frames_seen=2, n_static=2, n_moving=0, absdiff_static=8)


def literal_sigma_membership_and_rounding(defect=None):
    """First frames (a = 256, spatial = 256: xs = s).  10 12 30 at spatial_thr 6: the 30 is no member left of it and has no member but
    itself: (22 + 1) // 2 = 11, 11, 30.  10 12 13: the middle mean (35 + 1) // 3 = 12 rounds up.  10 13: (23 + 1) // 2 = 12 twice --
    with the clamped neighbours counted the left pixel would be (3 * 33 + 4) // 9 = 11."""
    assert run([[[10, 12, 30]]], defect)[0][0] == [[11, 11, 30]]
    assert run([[[10, 12, 13]]], defect)[0][:2] == ([[11, 12, 13]], [[11 << 8, 12 << 8, 13 << 8]])
    assert run([[[10, 13]]], defect)[0][0] == [[12, 12]]
    assert run([[[10], [13]]], defect)[0][0] == [[12], [12]]
    # spatial = 128 takes half of it: 10 + ((2 * 256 * 128 + 32768) >> 16) = 11, 13 + ((-1 * 256 * 128 + 32768) >> 16) = 13
    assert run([[[10, 13]]], defect, spatial=128)[0][0] == [[11, 13]]


LITERALS = (literal_one_pixel_of_the_issue, literal_first_frame_passes, literal_rounding, literal_clamp_at_the_border, literal_noise_cancels_in_the_sum,
            literal_sigma_membership_and_rounding)


@pytest.mark.parametrize("literal", LITERALS, ids=lambda f: f.__name__)
def test_restatement_equals_hand_worked_literals(literal):
    literal()


@pytest.mark.parametrize("defect", DR.DEFECTS)
def test_each_deliberate_defect_fails_a_literal(defect):
    failed = []
    for literal in LITERALS:
        try:
            literal(defect)
        except AssertionError:
            failed.append(literal.__name__)
    assert failed, f"no literal catches the defect {defect!r}"


# ---- the two statements, and the properties the header states ----------------------------------------------------------------------------
def random_frames(h, w, n, rng):
    """Noise around a level, a jump, random bytes, black and white: every branch and both ends of the range."""
    level = rng.integers(0, 256, (h, w, 1))
    out = []
    for f in range(n):
        kind = f % 5
        if kind in (0, 1):
            out.append(np.clip(level + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8))
        elif kind == 2:
            out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        elif kind == 3:
            out.append(np.full((h, w, 3), 255 * int(rng.integers(0, 2)), np.uint8))
        else:
            out.append(np.clip(level + 9 + rng.integers(-1, 2, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (5, 7), (6, 4)])
def test_vectorised_form_equals_the_loop(h, w):
    rng = np.random.default_rng(5110 + h * 16 + w)
    for k, cfg in enumerate(DC.VARIANTS[::5] + [{}]):
        a, b = DR.Ref(1, h, w, **cfg), DR.Ref(1, h, w, **cfg)
        for f in random_frames(h, w, 6, rng):
            oa, ra = a.step(0, f)
            ob, rb = b.step(0, f, loop=True)
            assert np.array_equal(oa, ob) and ra == rb and np.array_equal(a.acc[0], b.acc[0]) and np.array_equal(a.a[0], b.a[0]), (k, cfg)


def test_acc_needs_no_clamp_and_every_product_fits_int32():
    """acc' lies between acc and xs << 8, xs in 0..255, so acc stays in 0 .. 255 << 8; the two largest products are below 2^31."""
    assert 255 * 256 * 256 + 32768 < 2 ** 31 and 65280 * 256 + 128 < 2 ** 31
    rng = np.random.default_rng(5120)
    for cfg in DC.VARIANTS + [dict(spatial_thr=255), dict(spatial_thr=0), dict(motion_lo=0, motion_hi=1), dict(motion_lo=2294, motion_hi=2295)]:
        c = DR.config(**cfg)
        acc, seen = np.zeros((7, 9, 3), np.int64), 0
        for f in random_frames(7, 9, 10, rng):
            d = {}
            _, new, a, _ = DR.frame_step(f, acc, seen, c, detail=d)
            xs = d["xs"]
            assert xs.min() >= 0 and xs.max() <= 255 and d["w"].min() >= 256 >> c["temporal_shift"] and d["w"].max() <= 256
            assert new.min() >= 0 and new.max() <= DR.MAX_ACC
            if seen:
                assert (np.minimum(acc, xs << 8) <= new).all() and (new <= np.maximum(acc, xs << 8)).all()
            else:
                assert np.array_equal(new, xs << 8) and (a == 256).all()
            acc, seen = new, seen + 1


def test_identity_settings_return_the_input_bytes():
    rng = np.random.default_rng(5130)
    ref = DR.Ref(1, 6, 8, temporal_shift=0, spatial=0)
    for f in random_frames(6, 8, 8, rng):
        out, _ = ref.step(0, f)
        assert np.array_equal(out, f) and np.array_equal(ref.acc[0], f.astype(np.int64) << 8)


def test_a_constant_frame_is_a_fixed_point():
    for cfg in DC.VARIANTS[::3]:
        ref = DR.Ref(1, 5, 6, **cfg)
        f = np.zeros((5, 6, 3), np.uint8) + np.array([7, 200, 91], np.uint8)
        for i in range(5):
            out, row = ref.step(0, f)
            assert np.array_equal(out, f) and np.array_equal(ref.acc[0], f.astype(np.int64) << 8)
            assert (row["n_static"], row["n_moving"], row["absdiff_static"]) == ((0, 30, 0) if i == 0 else (30, 0, 0))


def test_every_gpu_case_sees_every_branch():
    """What tests/test_gpu_denoise.py compares must not be one branch only: over each case's run there are static pixels, moving pixels
    after the first frame, and pixels between the thresholds."""
    for h, w, _, v, seed in DC.sequence_cases():
        ref = DR.Ref(DC.N_STREAMS, h, w, **DC.VARIANTS[v])
        for frames in DC.sequence(h, w, DC.N_FRAMES, DC.N_STREAMS, seed):
            for s, f in enumerate(frames):
                ref.step(s, f)
        assert DC.saw_every_branch(ref.history) == (True, True, True), (h, w, DC.VARIANTS[v])
    assert {v for *_, v, _ in DC.sequence_cases()} == set(range(len(DC.VARIANTS)))


# ---- the rule header through a stand-alone program ----------------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("denoise_rule_check_san" if sanitize else "denoise_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built denoise_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def frame_cases():
    """(h, w, pitch, base, wide, variant): a pitch of 3w puts the frame's last pixel at the buffer's last byte; partial runs, one pixel,
    one row, one column, the dword path only with an aligned pitch and base."""
    return [(1, 1, 3, 0, 0, 0), (1, 9, 27, 0, 0, 5), (9, 1, 3, 0, 0, 9), (5, 9, 27, 0, 0, 14), (5, 9, 29, 1, 0, 2), (4, 8, 24, 0, 1, 7), (4, 8, 24, 4, 1, 11),
            (3, 37, 111, 3, 0, 16), (3, 36, 108, 0, 1, 18), (6, 5, 16, 0, 1, 21), (2, 70, 212, 8, 1, 23), (1, 4, 12, 0, 1, 3)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_denoise_rule_header_equals_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    rng = np.random.default_rng(5140)
    lines, want = [], []
    for h, w, pitch, base, wide, v in frame_cases():
        cfg = DR.config(**DC.VARIANTS[v])
        frames = random_frames(h, w, 5, rng) if h * w < 20 else [f[0] for f in DC.sequence(h, w, 5, 1, 5141 + v)]
        lines.append(f"F {h} {w} {pitch} {base} {wide} {cfg['motion_lo']} {cfg['motion_hi']} {cfg['temporal_shift']} {cfg['spatial']} {cfg['spatial_thr']} {len(frames)} "
                     + " ".join(str(int(b)) for f in frames for b in f.ravel()))
        ref = DR.Ref(1, h, w, **DC.VARIANTS[v])
        for f in frames:
            out, row = ref.step(0, f)
            vals = out.ravel().tolist() + ref.acc[0].ravel().tolist() + [row["n_static"], row["n_moving"], row["absdiff_static"], row["frames_seen"]]
            want += [" ".join(str(int(x)) for x in vals), "pad 0"]
    for _ in range(300):
        lo = int(rng.integers(0, 2295))
        hi = int(rng.integers(lo + 1, 2296))
        d, seen = int(rng.choice([0, lo, lo + 1, hi - 1, hi, 2295, int(rng.integers(0, 2296))])), int(rng.choice([0, 1, 2 ** 30]))
        lines.append(f"a {lo} {hi} {d} {seen}")
        want.append(f"{256 if seen == 0 else int(DR.alpha_of(d, dict(motion_lo=lo, motion_hi=hi)))} {min(seen + 1, 2 ** 30)}")
    for n in range(1, 10):
        for total in (0, 1, n // 2, n, 255 * n - 1, 255 * n, int(rng.integers(0, 255 * n + 1))):
            lines.append(f"m {total} {n}")
            want.append(str((total + n // 2) // n))
    n_lines = len(lines)
    one = "F 1 1 3 0 0 {} {} {} {} {} 1 7 7 7"
    extra = [one.format(18, 18, 3, 256, 6), one.format(-1, 54, 3, 256, 6), one.format(18, 2296, 3, 256, 6), one.format(18, 54, 7, 256, 6), one.format(18, 54, -1, 256, 6),
             one.format(18, 54, 3, 257, 6), one.format(18, 54, 3, 256, 256), "F 4 8 24 2 1 18 54 3 256 6 0", "F 4 8 23 0 0 18 54 3 256 6 0", "a 5 5 0 1", "a 0 1 2296 1",
             "m 10 0", "m 10 10", "m 256 1"]
    out = subprocess.run([exe], input="\n".join(lines + extra) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == f"done {n_lines + len(extra)}" and len(got) == len(want) + len(extra) + 1
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert g_.strip() == w_, (i, g_[:300], w_[:300])
    assert got[len(want):-1] == ["bad"] * len(extra)


# ---- the library: the host-only entry point, defaults, refusals, exports ------------------------------------------------------------------------
def test_pixel_entry_point_equals_restatement(pkg):
    DN = pkg.ingestion.denoise
    rng = np.random.default_rng(5150)
    for k in range(400):
        v = DC.VARIANTS[k % len(DC.VARIANTS)]
        cfg = DN.make_cfg(motion=(v["motion_lo"], v["motion_hi"]), temporal_shift=v["temporal_shift"], spatial=v["spatial"], spatial_thr=int(rng.choice([0, 6, 255])))
        c = DR.config(**dict(v, spatial_thr=cfg.spatial_thr))
        level = int(rng.integers(0, 256))
        cur = np.clip(level + rng.integers(-8, 9, (3, 3, 3)), 0, 255).astype(np.uint8) if k % 3 else rng.integers(0, 256, (3, 3, 3), dtype=np.uint8)
        acc = np.clip((level << 8) + rng.integers(-1500, 1500, (3, 3, 3)), 0, DR.MAX_ACC).astype(np.uint16) if k % 4 else rng.integers(0, DR.MAX_ACC + 1, (3, 3, 3)).astype(np.uint16)
        inside = int(rng.integers(0, 512)) | 16
        seen = int(rng.choice([0, 1, 5, 2 ** 30]))
        out, new, a, d = DN.pixel(cur, acc, inside, seen, cfg)
        w_out, w_new, w_a, w_d = DR.pixel(cur, acc, [(inside >> q) & 1 for q in range(9)], seen, c)
        assert (out.tolist(), new.tolist(), a, d) == (w_out.tolist(), w_new.tolist(), w_a, w_d), (k, v)
    # the issue's literal through the library: 119 on acc 29696
    out, new, a, d = DN.pixel(np.full((3, 3, 3), 119, np.uint8), np.full((3, 3, 3), 29696, np.uint16))
    assert (out.tolist(), new.tolist(), a, d) == ([117] * 3, [29960] * 3, 64, 27)
    E, ok = pkg._ffi.RtmodtError, (np.zeros((3, 3, 3), np.uint8), np.zeros((3, 3, 3), np.uint16))
    over = ok[1].copy()
    over[2, 2, 2] = 65281
    for bad in (dict(inside=0x1EF), dict(inside=512), dict(frames_seen=-1), dict(frames_seen=2 ** 30 + 1), dict(cfg=DN.make_cfg(motion=(5, 5))),
                dict(cfg=DN.make_cfg(temporal_shift=7)), dict(acc=over)):
        with pytest.raises(E) as e:
            DN.pixel(**dict(dict(cur=ok[0], acc=ok[1]), **bad))
        assert e.value.code == pkg._ffi.E_INVALID, bad
    with pytest.raises(ValueError):
        DN.pixel(np.zeros((3, 3), np.uint8), ok[1])


def test_denoise_cfg_defaults_refusals_and_exports(pkg):
    import ctypes as C
    import inspect
    DN = pkg.ingestion.denoise
    L = pkg._ffi.lib()
    cfg = DN.make_cfg()
    assert {k: getattr(cfg, k) for k in DR.DEFAULTS} == DR.DEFAULTS and (cfg.streams, cfg.height, cfg.width, cfg.device) == (1, 0, 0, 0)
    assert DR.DEFAULTS == dict(motion_lo=18, motion_hi=54, temporal_shift=3, spatial=256, spatial_thr=6)
    assert (DN.MAX_THRESHOLD, DN.MAX_ACC) == (DR.MAX_THRESHOLD, DR.MAX_ACC) == (2295, 65280)
    sig = inspect.signature(DN.FrameDenoiser.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[4:]] == [("motion", (18, 54)), ("temporal_shift", 3), ("spatial", 256), ("spatial_thr", 6), ("device", 0)]
    ok = dict(streams=2, height=37, width=70)
    # a parameter outside its range is refused before the device is touched, and the message names it; the defaults lack a frame size
    for kw, word in ((dict(), "height"), (dict(ok, streams=0), "streams"), (dict(ok, streams=1025), "streams"), (dict(ok, height=16385), "height"),
                     (dict(ok, width=0), "width"), (dict(ok, motion=(18, 18)), "motion_hi"), (dict(ok, motion=(54, 18)), "motion_hi"), (dict(ok, motion=(-1, 18)), "motion_lo"),
                     (dict(ok, motion=(18, 2296)), "motion_hi"), (dict(ok, motion=(2296, 2297)), "motion_lo"), (dict(ok, spatial_thr=-1), "spatial_thr"),
                     (dict(ok, spatial_thr=256), "spatial_thr"), (dict(ok, spatial=-1), "spatial"), (dict(ok, spatial=257), "spatial"),
                     (dict(ok, temporal_shift=-1), "temporal_shift"), (dict(ok, temporal_shift=7), "temporal_shift")):
        h = C.c_void_p()
        bad = DN.make_cfg(**kw)
        assert L.rtmodt_denoise_create(C.byref(bad), C.byref(h)) == pkg._ffi.E_INVALID and not h.value, kw
        assert word.encode() in L.rtmodt_last_error(), (kw, L.rtmodt_last_error())
    h = C.c_void_p()
    many = DN.make_cfg(streams=1024, height=2048, width=2048)                           # 2^32 pixels over all streams
    assert L.rtmodt_denoise_create(C.byref(many), C.byref(h)) == pkg._ffi.E_CAPACITY and not h.value
    assert L.rtmodt_denoise_create(None, C.byref(h)) == pkg._ffi.E_INVALID
    assert L.rtmodt_denoise_process(None, None, 0, 0, None, 0, 0, None, 0, 1, 1, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_denoise_reset(None, 0) == pkg._ffi.E_INVALID and L.rtmodt_denoise_last_ms(None, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_denoise_read_state(None, 0, None, None) == pkg._ffi.E_INVALID and L.rtmodt_denoise_load_state(None, 0, None, 0, 0) == pkg._ffi.E_INVALID
    assert L.rtmodt_denoise_pixel(None, None, None, 0, 0, None, None, None, None) == pkg._ffi.E_INVALID
    L.rtmodt_denoise_destroy(None)
    with pytest.raises(ValueError):
        DN.make_cfg(**dict(ok, motion=(1, 2, 3)))
    assert pkg.ingestion.FrameDenoiser is DN.FrameDenoiser is pkg.FrameDenoiser
    declared = [s for s in pkg._ffi.header_symbols() if s.startswith("rtmodt_denoise_")]
    assert len(declared) == 9 and all(hasattr(L, s) and s in L._signatures for s in declared)
    assert inspect.signature(pkg.pipeline.run).parameters["denoise"].default is None
    r = DN.DenoiseResult(0, 3, 7, 0, 10)
    assert r.noise_q8 == 2560 // 7 == DR.noise_q8(r._asdict()) and DN.DenoiseResult(0, 1, 0, 5, 0).noise_q8 == 0


def test_create_on_a_device_that_cannot_exist(pkg):
    """As tests/test_handle_lifecycle_cpu.py does for the other handles: the create fails at hipSetDevice inside the shared open, the
    half-built handle is released, and what is left of the Python object closes twice and is collected without a sound."""
    E = pkg._ffi.RtmodtError
    shell = None
    with pytest.raises(E) as info:
        try:
            pkg.ingestion.denoise.FrameDenoiser(1, 8, 8, device=1 << 20)
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
def night(amplitude, lift, **cfg):
    """The noisy night scene through the restatement -> (frames, clean, boxes, outputs)"""
    frames, clean, boxes = DC.noisy_night(amplitude, lift)
    ref = DR.Ref(1, EC.NIGHT_H, EC.NIGHT_W, **cfg)
    return frames, clean, boxes, [ref.step(0, f)[0] for f in frames]


def psnr(a, b):
    return 10 * math.log10(255 * 255 / ((a.astype(np.float64) - b) ** 2).mean())


@pytest.mark.parametrize("shift,derived", [(3, 11.76), (2, 8.45)])
@pytest.mark.parametrize("amplitude", [4, 8])
def test_premise_psnr_gain_reaches_the_derived_steady_state(amplitude, shift, derived):
    """A first-order filter of weight w = 2^-shift on white noise leaves w / (2 - w) of its variance: 10 log10((2 - w) / w) dB.
    Measured at the defaults' thresholds (frame 29, lift 60, 320 x 240): +-4: 10.99 dB at shift 3 and 8.11 dB at shift 2; +-8: 11.07 dB
    and 8.20 dB -- 0.25 to 0.8 dB short of the derived figure, from the quantisation and the clip at 0."""
    w = 2.0 ** -shift
    assert abs(10 * math.log10((2 - w) / w) - derived) < 0.005
    frames, clean, _, outs = night(amplitude, 60, temporal_shift=shift)
    gain = psnr(outs[29], clean[29]) - psnr(frames[29], clean[29])
    print(f"+-{amplitude} shift {shift}: raw {psnr(frames[29], clean[29]):.2f} dB, filtered {psnr(outs[29], clean[29]):.2f} dB, gain {gain:.2f} dB, derived {derived}")
    assert gain >= derived - 2.0


@pytest.mark.parametrize("amplitude", [4, 8])
def test_premise_every_jpeg_from_the_tenth_frame_on_is_smaller(amplitude):
    """Measured ratios filtered / raw at quality 85, still frames: 0.91 at +-4 and 0.77 at +-8."""
    frames, _, _, outs = night(amplitude, 60)
    ratios = [len(jpeg_ref.encode(o, 85)) / len(jpeg_ref.encode(f, 85)) for o, f in zip(outs[9:], frames[9:])]
    print(f"+-{amplitude}: ratio on frame 29 {ratios[20]:.3f}, least {min(ratios):.3f}, largest {max(ratios):.3f}")
    assert len(ratios) == 41 and max(ratios) < 1


@pytest.mark.parametrize("amplitude", [4, 8])
def test_premise_a_bright_moving_box_leaves_no_trail(amplitude):
    """Behind the box (the 40 columns it has just left) and inside it the filtered frame is nearer the clean one than the raw frame
    is; a filter that treats every pixel as static (the defect `static`) drags the box along and fails both."""
    i = DC.NIGHT_STILL + 15
    frames, clean, boxes, outs = night(amplitude, 60)
    y, x = boxes[i]
    regions = dict(left=(slice(y, y + EC.BOX_H), slice(x - 40, x)), inside=(slice(y, y + EC.BOX_H), slice(x, x + EC.BOX_W)))
    mae = lambda img, r: float(np.abs(img[r].astype(np.int64) - clean[i][r]).mean())       # noqa: E731
    ref = DR.Ref(1, EC.NIGHT_H, EC.NIGHT_W, defect="static")
    dragged = [ref.step(0, f)[0] for f in frames[:i + 1]][-1]
    for name, r in regions.items():
        print(f"+-{amplitude} {name}: raw {mae(frames[i], r):.2f}, filtered {mae(outs[i], r):.2f}, static defect {mae(dragged, r):.2f}")
        assert mae(outs[i], r) < mae(frames[i], r), name
        assert mae(dragged, r) > mae(frames[i], r), name


@pytest.mark.parametrize("amplitude", [4, 8])
def test_premise_motion_statuses_do_not_change(amplitude):
    """enhance_ref -> motion_ref on the lift-8 sequence: the same status on all 50 frames with and without the filter ahead, and MOTION
    on all 20 frames in which the dim box moves."""
    frames, _, boxes, outs = night(amplitude, EC.BOX_LIFT)
    h, w = EC.NIGHT_H, EC.NIGHT_W
    statuses = []
    for seq in (frames, outs):
        en, mo = ER.Ref(1, h, w), MR.Ref(1, h, w)
        statuses.append([mo.step(0, en.step(0, f)[0])["status"] for f in seq])
    assert statuses[0] == statuses[1]
    assert [s for s, b in zip(statuses[1], boxes) if b is not None] == [MR.MOTION] * DC.NIGHT_MOVING
