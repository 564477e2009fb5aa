"""Deterministic scenarios for the modules that share the cell-grid reader (csrc/cell_grid.h), the launch geometry (csrc/grid_host.h)
and the component labelling with its chunk ranking (csrc/ccl_dev.h): motion detection, left / removed objects and camera health, at
the sizes those headers are written for.  No device code: tests/test_grid_limit_cases_cpu.py proves on the restatements alone that
every scenario reaches what it was written for, tests/test_gpu_grid_limits.py drives the same scenarios on the kernels.

The big grid is 1025 x 1024 px at scale 1: 1 049 600 cells in 257 chunks of 4096, so that the scan of the per-chunk region counts
takes a second pass of 256; chunk c is the cell rows 4c .. 4c + 3, chunk 256 the single row 1024 (a quarter full) and cell 2^20 is
cell (0, 1024)."""
import functools

import numpy as np

import health_cases as HC
import leftobj_cases as LC
import motion_cases as MC

CHUNK = 4096                                     # CCL_CHUNK
READER_ROWS, FILTER_TW, FILTER_TH = 4, 64, 16    # CG_ROWS, GRID_TW, GRID_TH
BIG_H, BIG_W = 1025, 1024
MID_H, MID_W = 150, 530
PROD_H, PROD_W = 1080, 1920
MAX_SIDE = 32768                                 # MO_MAX_DIM
FLAT, LIT = 100, 200


def geometry(h, w, scale):
    """What grid_host.h's GridGeom makes of a frame size: the grid, its chunks, the reader's and the filter's tiles (x, y)."""
    gh, gw = -(-h // scale), -(-w // scale)
    cpt = 1 if scale >= 4 else 4 // scale
    return dict(gh=gh, gw=gw, cells=gh * gw, n_chunks=-(-gh * gw // CHUNK), reader_tiles=(-(-gw // (64 * cpt)), -(-gh // READER_ROWS)),
                filter_tiles=(-(-gw // FILTER_TW), -(-gh // FILTER_TH)))


# ---- masks into the motion detector: a flat model and a frame whose mask cells are 100 levels above it ---------------------
#: mask = raw: no neighbour test, no dilation, and nothing absorbed between the frames of a test
MOTION_MASK_CFG = dict(min_neighbors=1, dilate=0, learn_shift_fg=0)


def motion_load(model, gh, gw, s=0):
    """A flat background of FLAT with no deviation, past the warm-up, into stream ``s`` of a ``MotionDetector`` or a ``motion_ref.Ref``."""
    flat = np.full((gh, gw), FLAT << 8, np.uint16)
    model.load_state(flat, np.zeros_like(flat), 8, s)


def motion_frame(mask, scale, h, w):
    return MC.cells_to_frame(FLAT + (LIT - FLAT) * (np.asarray(mask) != 0).astype(np.uint8), scale, h, w)


# ---- masks into the left-object detector: a model whose mask cells are one frame short of static ---------------------------
#: mask = static: no neighbour test; two rows may alarm (alarm_frames 2) and clear (miss_frames 1) within a test's few frames
LO_MASK_CFG = dict(scale=1, warmup=1, static_frames=4, alarm_frames=2, min_neighbors=1, miss_frames=1)


def lo_base(gh, gw):
    """The background's cell lumas: FLAT .. FLAT + 4 in a pattern, so that the background's edge sums are not zero."""
    y, x = np.mgrid[0:gh, 0:gw]
    return (FLAT + (7 * x + 3 * y) % 5).astype(np.uint8)


def lo_model(mask, static_frames):
    """-> dict of int64 (gh, gw) arrays bg, cand, age, miss, flags and the uint8 luma grid: the background is ``lo_base``, the mask
    cells hold a candidate of LIT aged ``static_frames - 1 + (x + 2 y) % 5``, so that one frame of ``lo_frame`` makes exactly them
    static with ages ``static_frames .. static_frames + 4``."""
    m = np.asarray(mask) != 0
    gh, gw = m.shape
    y, x = np.mgrid[0:gh, 0:gw]
    base = lo_base(gh, gw)
    bg = base.astype(np.int64) << 8
    return dict(bg=bg, cand=np.where(m, LIT << 8, bg), age=np.where(m, static_frames - 1 + (x + 2 * y) % 5, 0).astype(np.int64),
                miss=np.zeros((gh, gw), np.int64), flags=np.zeros((gh, gw), np.int64), luma=base)


def lo_load_ref(ref, model, s=0):
    """The model into stream ``s`` of a ``leftobj_ref.Ref``, past the warm-up; the mask and the ledger stay."""
    for k in ("bg", "cand", "age", "miss", "flags"):
        getattr(ref, k)[s] = model[k].copy()
    ref.luma[s] = model["luma"].astype(np.int64)
    ref.seen[s] = ref.c["warmup"]


def lo_cells(model, dtype):
    """The model as the detector's array of 8-byte cells (``dtype``: its CELL_DTYPE)."""
    cells = np.zeros(model["bg"].shape, dtype)
    for k in ("bg", "cand", "age", "miss", "flags"):
        cells[k] = model[k]
    return cells


def lo_frame(mask, h, w):
    return LC.cells_to_frame(np.where(np.asarray(mask) != 0, LIT, lo_base(h, w)).astype(np.uint8), 1, h, w)


# ---- 1. chunk_edges ----------------------------------------------------------------------------------------------------------
KINDS = {"dot": [(0, 0)], "h2": [(0, 0), (1, 0)], "v2": [(0, 0), (0, 1)], "sq3": [(dx, dy) for dy in range(3) for dx in range(3)],
         "h9": [(dx, 0) for dx in range(9)], "bar5": [(0, dy) for dy in range(5)]}
#: (x, y, kind) of the first cell: regions of 2 and 5 cells, decoys of 1 cell (below min_area 2) and of 9 cells (above the left-object
#: max_area 8; a region for motion) directly before and after them.  Cell 0, cell 4095 (its region reaches into chunk 1) and cell
#: 4096; chunk 100; chunk 255, with the bar over rows 1020 .. 1024 whose root is in chunk 255 and whose last cell is in chunk 256;
#: chunk 256: cell 2^20, the region that ends on the grid's last cell, and more
EDGE_PIECES = (
    (0, 0, "h2"), (10, 0, "dot"), (20, 0, "sq3"), (1023, 3, "v2"),
    (0, 4, "h2"),
    (5, 400, "dot"), (10, 400, "h2"), (15, 400, "dot"), (20, 400, "sq3"), (30, 401, "h2"), (40, 401, "dot"), (50, 403, "h2"),
    (5, 1020, "dot"), (10, 1020, "h2"), (20, 1020, "sq3"), (30, 1020, "dot"), (500, 1020, "bar5"), (40, 1021, "h2"), (60, 1023, "h2"), (70, 1023, "dot"),
    (0, 1024, "h2"), (10, 1024, "dot"), (20, 1024, "h2"), (25, 1024, "dot"), (100, 1024, "h2"), (200, 1024, "h9"), (600, 1024, "dot"), (1022, 1024, "h2"))
EDGE_MOTION = dict(min_area=2)
EDGE_LEFTOBJ = dict(min_area=2, max_area=8)


@functools.lru_cache(maxsize=None)
def edge_mask():
    m = np.zeros((BIG_H, BIG_W), np.uint8)
    for x, y, kind in EDGE_PIECES:
        for dx, dy in KINDS[kind]:
            m[y + dy, x + dx] = 1
    m.setflags(write=False)
    return m


def edge_roots(min_area, max_area=2 ** 24):
    """-> [(first cell index, area)] of the qualifying pieces in raster order, from the table alone."""
    return sorted((y * BIG_W + x, len(KINDS[k])) for x, y, k in EDGE_PIECES if min_area <= len(KINDS[k]) <= max_area)


def chunk_counts(roots, n_chunks):
    """The qualifying roots per chunk (what ccl_count_chunk writes) from a list of first cell indices."""
    return np.bincount(np.asarray(roots, np.int64) // CHUNK, minlength=n_chunks)


def edge_cuts(min_area, max_area=2 ** 24):
    """max_regions such that the cut falls (a) exactly before chunk 255, (b) exactly before chunk 256, (c) inside chunk 256, (d)
    beyond the total."""
    per = chunk_counts([r for r, _ in edge_roots(min_area, max_area)], 257)
    return dict(a=int(per[:255].sum()), b=int(per[:256].sum()), c=int(per[:256].sum()) + 2, d=int(per.sum()) + 3)


# ---- 2. speckle_wide ---------------------------------------------------------------------------------------------------------
SPECKLE_CFG = dict(scale=1, threshold=6, dev_gain=0, min_neighbors=1, dilate=0, min_area=1)     # test_sparse_speckle's first
SPECKLE_MAX_REGIONS = (32, 256)
SPECKLE_FRAMES = 2


def speckle_cells(frame_no, frac=0.02, h=BIG_H, w=BIG_W):
    """Cell lumas of frame ``frame_no``: ``motion_cases.speckle`` over the whole grid."""
    return MC.speckle(h, w, np.random.default_rng(7000 + frame_no), frac=frac)


# ---- 3. shapes_big -----------------------------------------------------------------------------------------------------------
SHAPES = ("spiral", "comb", "diagonal", "full")


@functools.lru_cache(maxsize=None)
def big_shape(name):
    m = MC.SHAPES[name](BIG_H, BIG_W)
    m.setflags(write=False)
    return m


def shape_frames(name):
    """The shape, its complement, the shape again."""
    m = big_shape(name)
    return (m, 1 - m, m)


# ---- 4. dense ----------------------------------------------------------------------------------------------------------------
FILLS = (0.30, 0.42, 0.50, 0.70)
SEEDS = (0, 1, 2)
DENSE_MOTION = dict(scale=1, min_area=2, max_regions=256, **MOTION_MASK_CFG)
DENSE_LEFTOBJ = dict(LO_MASK_CFG, min_area=2, max_regions=256)


@functools.lru_cache(maxsize=None)
def dense_mask(fill, seed):
    m = (np.random.default_rng(1000 * round(100 * fill) + seed).random((MID_H, MID_W)) < fill).astype(np.uint8)
    m.setflags(write=False)
    return m


# ---- 5. streams_big ----------------------------------------------------------------------------------------------------------
STREAM_LISTS = ([2, 0, 1], [1], [2, 0], [0, 1, 2])
STREAMS_MOTION = dict(scale=1, min_area=2, max_regions=64, **MOTION_MASK_CFG)
STREAMS_LEFTOBJ = dict(LO_MASK_CFG, min_area=2, max_regions=32, max_objects=32)


def stream_mask_big(call, s):
    """Stream 0: the chunk_edges mask; streams 1 and 2: speckle of 2 % and 0.3 %, new on every call."""
    if s == 0:
        return edge_mask()
    return (np.random.default_rng(100 * call + s).random((BIG_H, BIG_W)) < (0.02, 0.003)[s - 1]).astype(np.uint8)


def stream_mask_mid(call, s):
    """Fills of 2 %, 30 % and 50 % on the 150 x 530 grid, new on every call."""
    return (np.random.default_rng(200 * call + s).random((MID_H, MID_W)) < (0.02, 0.30, 0.50)[s]).astype(np.uint8)


# ---- 6. production -----------------------------------------------------------------------------------------------------------
PROD_PITCH = 3 * PROD_W                          # 5760: a multiple of 4, the reader's dword path
PROD_ODD = (3 * PROD_W + 5, 1)                   # (pitch, offset) of the device frames: the byte path
#: frames of ``motion_cases.sequence`` by their number there: the warm-up, still, the rectangle's first two frames, still again
MOTION_PICK = tuple(range(9)) + (MC.RECT_FIRST, MC.RECT_FIRST + 1, MC.RECT_FIRST + MC.RECT_FRAMES, MC.RECT_FIRST + MC.RECT_FRAMES + 1)
MOTION_SCALE1 = dict(scale=1, warmup=2)
MOTION_SCALE1_PICK = (0, 1, 2, MC.RECT_FIRST, MC.RECT_FIRST + MC.RECT_FRAMES)
#: frames of ``leftobj_cases.sequence``: the warm-up, the block put down at PLACE and the walker, static, the alarm (alarm_frames 3);
#: then the block is taken away and the scene is clear again after ``occlusion`` frames.  These run under the sequence's own small
#: timers (the defaults need 100 frames to call a cell static, health's 25 to end the warm-up); the first DEFAULT_FRAMES frames run
#: under the default configuration as well
LEFTOBJ_PROD = dict(LC.SEQ_CFG, scale=4, alarm_frames=3)
LEFTOBJ_PICK = tuple(range(LC.PLACE + 8)) + tuple(range(LC.TAKE, LC.TAKE + 4))
HEALTH_STRETCHES = (("healthy", 4), ("covered", 4), ("healthy", 3))
DEFAULT_FRAMES = 10


def motion_frames(h, w, seed, pick, low=False):
    """The frames ``pick`` of ``motion_cases.sequence``'s script (its background, noise and rectangle; noise drawn per frame made).
    ``low``: a second rectangle in the picture's last quarter on the same frames."""
    rng = np.random.default_rng(seed)
    bgd = MC.background(h, w)
    out = []
    for f in pick:
        fr = bgd + rng.integers(-3, 4, (h, w, 3))
        if MC.RECT_FIRST <= f < MC.RECT_FIRST + MC.RECT_FRAMES:
            x0, y0, x1, y1 = MC.rect_at(h, w, f - MC.RECT_FIRST)
            fr[y0:y1, x0:x1] = 220 + rng.integers(-3, 4, (y1 - y0, x1 - x0, 3))
            if low:
                fr[h * 3 // 4:h * 3 // 4 + 20, 100:160] = 220
        out.append(np.clip(fr, 0, 255).astype(np.uint8))
    return out


def leftobj_frames(h, w, seed, pick):
    """The frames ``pick`` of ``leftobj_cases.sequence``'s script (its background, noise, block and walker)."""
    rng = np.random.default_rng(seed)
    bgd = LC.background(h, w)
    out = []
    for f in pick:
        fr = bgd + rng.integers(-3, 4, (h, w, 3))
        if LC.PLACE <= f < LC.TAKE:
            x0, y0, x1, y1 = LC.block_box(h, w)
            fr[y0:y1, x0:x1] = 215 + rng.integers(-3, 4, (y1 - y0, x1 - x0, 3))
        if LC.WALK_FIRST <= f < LC.WALK_FIRST + LC.WALK_FRAMES:
            x0, y0, x1, y1 = LC.walker_box(h, w)
            fr[y0:y1, x0:x1] = 15 + rng.integers(-3, 4, (y1 - y0, x1 - x0, 3))
        out.append(np.clip(fr, 0, 255).astype(np.uint8))
    return out


def health_frames(h, w, seed, stretches=HEALTH_STRETCHES):
    return HC.sequence(h, w, seed, stretches)[0]


# ---- 7. max_side -------------------------------------------------------------------------------------------------------------
SIDE_SHAPES = ((4, MAX_SIDE), (MAX_SIDE, 4))
SIDE_SCALES = (1, 8)
SIDE_MOTION = dict(warmup=2)
SIDE_LEFTOBJ = dict(warmup=1, static_frames=2, alarm_frames=2, min_neighbors=2, occlusion=0, miss_frames=0)
SIDE_HEALTH = dict(HC.TIMERS, warmup=2, hold_frames=2, clear_frames=1)
#: the rectangles along the long side in pixels, (first, last + 1).  The first lies across pixel 512: at scale 1 cell 512, an edge of the
#: reader's tiles (256 cells along x, 4 rows along y) and of the filter's (64 along x, 16 along y); at scale 8 cell 64, an edge of
#: both again (64 cells along x).  The second ends on the last pixel, which at a short side of 4 px and scale 8 lies in a partial cell
SIDE_RECTS = ((480, 560), (MAX_SIDE - 70, MAX_SIDE))


def side_frame(h, w, rect=None, level=220):
    """The smooth background, with ``rect`` along the long side (over the whole short side) at ``level``."""
    fr = np.clip(MC.background(h, w), 0, 255).astype(np.uint8)
    if rect is not None:
        if w >= h:
            fr[:, rect[0]:rect[1]] = level
        else:
            fr[rect[0]:rect[1], :] = level
    return fr


def side_motion_frames(h, w):
    """Two frames of warm-up, still, the first rectangle, the second, still."""
    return [side_frame(h, w), side_frame(h, w), side_frame(h, w), side_frame(h, w, SIDE_RECTS[0]), side_frame(h, w, SIDE_RECTS[1]), side_frame(h, w)]


def side_leftobj_frames(h, w):
    """One frame of warm-up, clear, both rectangles for four frames (static from the second on, the alarm), clear again."""
    both = side_frame(h, w, SIDE_RECTS[0])
    if w >= h:
        both[:, SIDE_RECTS[1][0]:] = 220
    else:
        both[SIDE_RECTS[1][0]:, :] = 220
    return [side_frame(h, w)] * 2 + [both] * 4 + [side_frame(h, w)] * 2


def side_health_frames(h, w, seed=3):
    return HC.sequence(h, w, seed, (("healthy", 3), ("covered", 3), ("healthy", 2), ("repeated", 3)))[0]
