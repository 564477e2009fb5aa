"""Deterministic scenes for the left-object detector's tests (tests/test_leftobj_cpu.py, tests/test_gpu_leftobj.py)."""
import numpy as np

from motion_cases import background, cells_to_frame  # noqa: F401

#: the scripted sequence: warm-up, a bright block put down at PLACE, a dark walker in front of its left part for WALK_FRAMES frames
#: from WALK_FIRST, the alarm, the absorb, the block taken away at TAKE (the REMOVED alarm), a global +STEP from STEP_AT
N_FRAMES, PLACE, WALK_FIRST, WALK_FRAMES, TAKE, STEP_AT, STEP = 63, 6, 9, 2, 46, 60, 60
#: the small timers the sequence is written for
SEQ_CFG = dict(warmup=4, static_frames=5, alarm_frames=8, absorb_frames=30, occlusion=2, miss_frames=3)


def block_box(h, w):
    """The block's pixel box (x0, y0, x1, y1), exclusive."""
    return w * 3 // 10, h * 3 // 10, w * 6 // 10, h * 7 // 10


def walker_box(h, w):
    """The walker's: the left third of the block and a strip beside it."""
    x0, y0, x1, y1 = block_box(h, w)
    return max(0, x0 - (x1 - x0) // 3), y0, x0 + (x1 - x0) // 3, y1


def sequence(h, w, seed, n=N_FRAMES):
    """``n`` frames (h, w, 3) uint8: noise of +-3 on the smooth background, the block, the walker, then the global +STEP."""
    rng = np.random.default_rng(seed)
    bgd = background(h, w)
    out = []
    for f in range(n):
        fr = bgd + rng.integers(-3, 4, (h, w, 3))
        if PLACE <= f < TAKE:
            x0, y0, x1, y1 = block_box(h, w)
            fr[y0:y1, x0:x1] = 215 + rng.integers(-3, 4, (y1 - y0, x1 - x0, 3))
        if WALK_FIRST <= f < WALK_FIRST + WALK_FRAMES:
            x0, y0, x1, y1 = walker_box(h, w)
            fr[y0:y1, x0:x1] = 15 + rng.integers(-3, 4, (y1 - y0, x1 - x0, 3))
        if f >= STEP_AT:
            fr = fr + STEP
        out.append(np.clip(fr, 0, 255).astype(np.uint8))
    return out


def blob_cells(gh, gw, n, size=3, gap=2, base=100, lift=100):
    """Cell lumas: ``base`` with the first ``n`` of a raster of ``size x size`` blobs, ``gap`` cells apart, raised by ``lift``
    -> (cells, the blobs' cell boxes (cx0, cy0, cx1, cy1) in raster order)."""
    cells = np.full((gh, gw), base, np.uint8)
    boxes = []
    pitch = size + gap
    for by in range(1, gh - size, pitch):
        for bx in range(1, gw - size, pitch):
            if len(boxes) == n:
                return cells, boxes
            cells[by:by + size, bx:bx + size] = base + lift
            boxes.append((bx, by, bx + size - 1, by + size - 1))
    assert len(boxes) == n, (len(boxes), n)
    return cells, boxes
