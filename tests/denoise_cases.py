"""Shared cases of the frame-denoiser tests (tests/test_denoise_cpu.py, tests/test_gpu_denoise.py): the geometries, the rule variants,
the scene generator (a textured base, fresh noise per frame, a block that moves) and the noisy night scene that shows what the module
is for."""
import numpy as np

import enhance_cases as EC

#: the kernel's tile: 256 columns x 16 rows
TILE_W, TILE_H = 256, 16
#: (h, w, stride): the enhancer's geometries, frames of one pixel, one row and one column, and frames one pixel past a tile both ways
TINY = ((1, 1, 3), (1, 9, 27), (9, 1, 7))
PAST_TILE = ((TILE_H + 1, TILE_W + 1, 3 * (TILE_W + 1) + 2), (2 * TILE_H + 1, TILE_W + 4, 3 * (TILE_W + 4)))
GEOMETRIES = EC.GEOMETRIES + EC.WIDE_GEOMETRIES + TINY + PAST_TILE
#: every spatial x temporal_shift x threshold pair
VARIANTS = [dict(spatial=sp, temporal_shift=ts, motion_lo=lo, motion_hi=hi) for lo, hi in ((18, 54), (6, 200)) for sp in (0, 128, 256) for ts in (0, 1, 3, 6)]
N_STREAMS, N_FRAMES = 3, 6


def sequence_cases():
    """(h, w, stride, variant index, seed): every geometry twice, every variant at least once"""
    out = []
    for rep in range(2):
        for g, (h, w, stride) in enumerate(GEOMETRIES):
            k = len(out)
            out.append((h, w, stride, k * 7 % len(VARIANTS), 5200 + k))
    return out


# ---- the generator --------------------------------------------------------------------------------------------------------------------
NOISE, LIFT = 2, 40
#: added to every pixel of frame f: a change of a few levels everywhere puts whole frames between the thresholds
FLICKER = (0, 0, 0, 3, 0, 5)


def scene(h, w, rng):
    """A textured base: blocks of 8 x 8 pixels at random levels (edges for the sigma filter) under a fine texture of +-3."""
    coarse = rng.integers(50, 180, ((h + 7) // 8, (w + 7) // 8))
    img = np.kron(coarse, np.ones((8, 8), np.int64))[:h, :w, None] + rng.integers(-3, 4, (h, w, 1))
    return img + np.array([0, 4, -4])


def block_at(f, h, w):
    """-> (y, x, bh, bw) of the block in frame f, or None: it is absent in every third frame and elsewhere in every other"""
    if f % 3 == 0:
        return None
    bh, bw = max(1, h // 3), max(1, w // 4)
    return (5 * f) % (h - bh + 1), (7 * f) % (w - bw + 1), bh, bw


def frame(base, f, rng):
    img = base + FLICKER[f % len(FLICKER)]
    at = block_at(f, *base.shape[:2])
    if at is not None:
        y, x, bh, bw = at
        img = img.copy()
        img[y:y + bh, x:x + bw] += LIFT
    return np.clip(img + rng.integers(-NOISE, NOISE + 1, img.shape), 0, 255).astype(np.uint8)


def sequence(h, w, n_frames, n_streams, seed):
    """-> frames[frame][stream], a scene of its own per stream"""
    rng = np.random.default_rng(seed)
    bases = [scene(h, w, rng) for _ in range(n_streams)]
    return [[frame(bases[s], f + s, rng) for s in range(n_streams)] for f in range(n_frames)]


def saw_every_branch(ref_a_maps):
    """Over the `a` maps of a run: static pixels, moving pixels after the first frame, and pixels between the thresholds."""
    later = [a for a, first in ref_a_maps if not first]
    return (any((a == 0).any() for a in later), any((a == 256).any() for a in later), any(((a > 0) & (a < 256)).any() for a in later))


# ---- what it is for: the enhancer's night scene under sensor noise ---------------------------------------------------------------------
NIGHT_STILL, NIGHT_MOVING = 30, 20


def noisy_night(amplitude, lift, seed=5101):
    """-> (frames, clean, boxes): `NIGHT_STILL` frames of enhance_cases.night_scene() under uniform noise of +-amplitude on every
    channel, then `NIGHT_MOVING` in which a box `lift` levels brighter moves enhance_cases.BOX_STEP pixels a frame; `clean` are the
    same frames without the noise and boxes[i] is (y, x) or None."""
    rng = np.random.default_rng(seed)
    base = EC.night_scene()
    frames, clean, boxes = [], [], []
    for i in range(NIGHT_STILL + NIGHT_MOVING):
        img = base.copy()
        at = None
        if i >= NIGHT_STILL:
            at = (100, 16 + EC.BOX_STEP * (i - NIGHT_STILL))
            img[at[0]:at[0] + EC.BOX_H, at[1]:at[1] + EC.BOX_W] += lift
        clean.append(np.clip(img, 0, 255).astype(np.uint8))
        frames.append(np.clip(img + rng.integers(-amplitude, amplitude + 1, img.shape), 0, 255).astype(np.uint8))
        boxes.append(at)
    return frames, clean, boxes
