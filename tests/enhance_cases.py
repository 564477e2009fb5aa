"""Shared cases of the frame-enhancer tests (tests/test_enhance_cpu.py, tests/test_gpu_enhance.py): the geometries and tile grids, the
frame contents, and the dark scene with a dim moving box that shows what the module is for."""
import numpy as np

#: (h, w, stride): odd sizes with a pitch that forces the byte path, and a variant of each whose pitch (and base) allow dword access
GEOMETRIES = ((37, 70, 211), (70, 37, 117), (19, 150, 452), (150, 530, 1601), (5, 9, 29))
WIDE_GEOMETRIES = ((36, 72, 216), (72, 36, 108), (20, 152, 460), (152, 532, 1600), (4, 8, 24))
#: (tiles_y, tiles_x)
GRIDS = ((1, 1), (2, 3), (8, 8), (16, 16))
CONTENTS = ("uniform", "constant", "night", "binary", "ramp")
#: clip_limit 0 (no clipping), OpenCV's 2.0, and one whose clip is forced to 1 on every tile of the geometries above
CLIP_Q8 = (0, 512, 1)


def fits(grid, h, w):
    return grid[0] <= h and grid[1] <= w


def content(kind, h, w, rng):
    """One uint8 (h, w, 3) frame."""
    if kind == "uniform":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "constant":                      # every pixel in one bin: the count must be exactly n
        return np.full((h, w, 3), int(rng.integers(0, 256)), np.uint8) + np.zeros((h, w, 3), np.uint8)
    if kind == "night":                         # 40 levels
        g = rng.integers(8, 48, (h, w, 1))
        return np.clip(g + rng.integers(-2, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 1), dtype=np.uint8) * 255).repeat(3, 2)
    if kind == "ramp":
        return np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)[None, :, None], (h, w, 3)).copy()
    raise KeyError(kind)


def sequence(h, w, n_frames, n_streams, seed):
    """-> frames[frame][stream]: every content in turn, a different one per stream"""
    rng = np.random.default_rng(seed)
    return [[content(CONTENTS[(f + 2 * s) % len(CONTENTS)], h, w, rng) for s in range(n_streams)] for f in range(n_frames)]


def padded(frame, stride, fill=0xA5, lead=0):
    """A copy of `frame` as a view into a buffer whose rows are `stride` bytes apart and whose padding holds `fill`; `lead` bytes
    before the first pixel (an odd number forces an odd base address) -> (view, buffer)"""
    h, w, _ = frame.shape
    buf = np.full(lead + h * stride, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[lead:], (h, w, 3), (stride, 3, 1))
    view[...] = frame
    return view, buf


# ---- what it is for: a dark, noisy, static scene and a dim moving box -----------------------------------------------------------------
#: the scene: luma around NIGHT_BASE with a fixed texture of +-NIGHT_TEXTURE, fresh noise of +-NIGHT_NOISE per frame and pixel, and a
#: box BOX_LIFT levels brighter than what it covers.  BOX_LIFT is below motion_ref's default threshold of 12 levels, which a raw cell
#: difference must exceed; the enhancer at its defaults stretches the scene's 20-odd levels over several times as many.
NIGHT_H, NIGHT_W = 240, 320
NIGHT_BASE, NIGHT_TEXTURE, NIGHT_NOISE = 18, 6, 1
BOX_LIFT, BOX_H, BOX_W, BOX_STEP = 8, 40, 32, 8
NIGHT_WARM, NIGHT_MOVING = 30, 20           # frames without the box, then frames in which it moves BOX_STEP pixels a frame


def night_scene(seed=4101):
    rng = np.random.default_rng(seed)
    img = NIGHT_BASE + rng.integers(-NIGHT_TEXTURE, NIGHT_TEXTURE + 1, (NIGHT_H, NIGHT_W))
    return np.stack([img, img + 1, img - 1], -1)


def night_frame(base, rng, box_at=None):
    img = base.copy()
    if box_at is not None:
        y, x = box_at
        img[y:y + BOX_H, x:x + BOX_W] += BOX_LIFT
    return np.clip(img + rng.integers(-NIGHT_NOISE, NIGHT_NOISE + 1, img.shape), 0, 255).astype(np.uint8)


def night_sequence(with_box=True, n_still=NIGHT_WARM, n_moving=NIGHT_MOVING, seed=4102):
    """-> (frames, moving): `moving[i]` says that the box is in frame i at another place than in frame i - 1"""
    rng = np.random.default_rng(seed)
    base = night_scene()
    frames = [night_frame(base, rng) for _ in range(n_still)]
    moving = [False] * n_still
    for i in range(n_moving):
        frames.append(night_frame(base, rng, (100, 16 + BOX_STEP * i) if with_box else None))
        moving.append(with_box)
    return frames, moving
