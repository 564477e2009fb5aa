"""Inputs shared by ``tests/test_stab_cpu.py`` (which establishes on the restatements what each input is here for) and
``tests/test_gpu_stab.py`` (which runs them on the kernels of ``csrc/stab.hip``).  Plain NumPy; no GPU, no library.

Shapes (h, w): 37 x 23, 131 x 77 and 1 x 1 stay inside the warp kernel's first tile (256 output pixels x 4 rows a workgroup, a run of 4
pixels a thread); 523 x 9 is three tiles wide and three high with a partial run at each row's end.  37, 131 and 523 are odd: a
multiple of no vector width."""
import math

import numpy as np

import gmc_ref as G
import stab_ref as S
from lens_cases import SENT, image, padded

BORDER = (17, 200, 93)
SHAPES = {"37x23": (23, 37), "131x77": (77, 131), "1x1": (1, 1), "523x9": (9, 523)}
CFG = dict(leak_shift=3, max_shift_px=12, max_rot_milli=20, max_zoom_milli=30, reset_after=4)      # small limits: a dozen calls reach every one
N_STREAMS, N_CALLS = 4, 12


def warp(deg=0.0, scale=1.0, tx=0.0, ty=0.0):
    """float32 [a, -b, tx; b, a, ty]."""
    a, b = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return np.float32([a, -b, tx, b, a, ty])


def schedule(seed=5):
    """-> per call (warps float32 [4, 6], valid [4]).  Stream 0 jitters by a few pixels and a fraction of a degree (status OK
    throughout); stream 1 drifts by 5 px and 0.4 degrees a call until the shift and rotation limits clamp it; stream 2 loses its input
    for calls 3..9 (HOLD, HOLD, HOLD, RESET, HOLD, ...; a NaN warp stands behind an invalid flag) and recovers; stream 3 zooms by 1.5 % a
    call into the zoom limit and shifts in y only."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(N_CALLS):
        w0 = warp(rng.uniform(-0.3, 0.3), 1.0 + rng.uniform(-0.002, 0.002), rng.uniform(-3, 3), rng.uniform(-3, 3))
        w1 = warp(0.4, 1.0, 5.0, -2.25)
        lost = 3 <= k <= 9
        w2 = np.float32([np.nan] * 6) if lost and k % 2 else warp(-0.1, 1.0, 1.5, 0.5)
        w3 = warp(0.0, 1.015, 0.0, 0.75 * (-1) ** k)
        out.append((np.stack([w0, w1, w2, w3]), [True, True, not lost, True]))
    return out


def run(st, pkg, frames, *, warps=None, valid=None, streams=None, src_kind="host", dst_kind="host", spitch=None, dpitch=None, offset=0):
    """One process call in the given memory kinds and pitches -> the output frames; asserts that no byte outside them changed."""
    F = pkg._ffi
    n, (h, w) = len(frames), frames[0].shape[:2]
    spitch, dpitch = spitch or 3 * w, dpitch or 3 * w
    if src_kind == "host":
        src, kw = [padded(f, spitch, i)[1] for i, f in enumerate(frames)], {}
    else:
        src = F.DeviceBuffer(offset + n * h * spitch + 8)
        src.upload(image(frames, spitch, offset))
        kw = dict(stride=spitch, offset=offset)
    blank = [np.full((h, w, 3), SENT, np.uint8)] * n
    if dst_kind == "host":
        bufs = [padded(b, dpitch, 3 + i) for i, b in enumerate(blank)]
        got = st.process(src, warps, valid, streams=streams, out=[v for _, v in bufs], **kw)
        for i, (buf, view) in enumerate(bufs):
            assert np.array_equal(buf, padded(view, dpitch, 3 + i)[0]), f"frame {i}: a byte outside the pixels changed"
        return [np.array(g) for g in got]
    dst = F.DeviceBuffer(offset + n * h * dpitch + 8)
    dst.upload(image(blank, dpitch, offset))
    assert st.process(src, warps, valid, streams=streams, out=dst, out_stride=dpitch, out_offset=offset, **kw) is dst
    raw = dst.download()
    got = [np.array(np.lib.stride_tricks.as_strided(raw[offset + i * h * dpitch:], (h, w, 3), (dpitch, 3, 1))) for i in range(n)]
    assert np.array_equal(raw, image(got, dpitch, offset)), "a byte outside the pixels changed"
    return got


def same_state(st, ref, tag=""):
    """The device's paths (bit patterns), statuses, HOLD runs and coefficients against the restatement's."""
    for s, r in enumerate(st.result()):
        assert np.array_equal(np.float64(r.path).view(np.uint64), np.float64(ref.path[s]).view(np.uint64)), (tag, s, r.path, ref.path[s])
        assert (r.status, r.hold, tuple(r.coef)) == (ref.status[s], ref.hold[s], tuple(ref.coef[s])), (tag, s, r, ref.status[s], ref.hold[s], ref.coef[s])


# ---------------------------------------------------------------------------------------------------------------- the shaking camera
# A textured scene (gmc_ref's canvas) seen by a camera that shakes by integer pixels: frame k is the crop at JITTER[k], so the content of
# frame k - 1 is found in frame k moved by JITTER[k - 1] - JITTER[k], exactly.
GATE_SIZE = (96, 128)
JITTER = [(0, 0), (2, -1), (-3, 2), (1, 3), (-2, -3), (3, 1), (-1, -2), (2, 2), (-3, -1), (0, 3), (3, -3), (-2, 1), (1, -2), (-1, 2)]
GATE_MOTION = dict(warmup=4, scale=4)
GATE_STAB = dict(leak_shift=0, max_shift_px=8, crop_zoom_milli=1100)          # the enlargement hides the 3-pixel band (1 + 2 x 3 / 96 < 1.1)
GATE_MARGIN = 16


def gate_frames(seed=91):
    h, w = GATE_SIZE
    cv = G.canvas(h + 2 * GATE_MARGIN, w + 2 * GATE_MARGIN, seed)
    return [G.crop(cv, GATE_MARGIN + dx, GATE_MARGIN + dy, h, w) for dx, dy in JITTER]


def gate_warps():
    """Per frame the float32 warp previous frame -> this frame (the identity for the first)."""
    out = [S.IDENTITY_WARP.copy()]
    for (px, py), (qx, qy) in zip(JITTER, JITTER[1:]):
        out.append(np.float32([1, 0, px - qx, 0, 1, py - qy]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the estimator form
# downscale 1, coarse_search 2: level 1 needs 2 x 2 + 4 = 8 columns and rows, and min_blocks blocks of 16 x 16 whose search window stays
# inside the frame: 96 x 112 has 6 x 7 blocks, 4 x 5 of them interior.  Smaller frames leave fewer than min_blocks = 12 of them.
EST_SIZE = (96, 112)
EST_CFG = dict(downscale=1, coarse_search=2, search=4, min_blocks=12, min_inliers=8, min_sep=16.0)
EST_STEPS = [(3, -2), (-5, 1), (2, 4), (-1, -3), (4, 2)]                       # camera steps; content moves by their negatives
EST_STAB = dict(leak_shift=0, max_shift_px=16)


def est_frames(seed=17):
    return G.pan_sequence(EST_SIZE[0], EST_SIZE[1], seed, EST_STEPS, margin=24)


def est_interior():
    """Rows and columns every stabilised frame shows of the first frame: the running sum of the steps stays inside +-m."""
    x = y = m = 0
    for sx, sy in EST_STEPS:
        x, y = x + sx, y + sy
        m = max(m, abs(x), abs(y))
    return m + 1
