"""The layouts and frames ``tests/test_gpu_compose.py`` runs, shared with ``tests/test_compose_cpu.py`` (whose discrimination test must
show that deliberately wrong restatements differ on exactly these inputs).  Sizes are the smallest that reach every path of
``csrc/compose.hip``: tiles are 32 x 8 pixels, a footprint is staged in 32 KiB and a source row in chunks of 10240 pixels."""
import functools

import numpy as np

import compose_ref as R

O, C = R.Output, R.Cell


def frame(h: int, w: int, seed: int) -> np.ndarray:
    """Uniform noise: every rounding rule and every chroma rule shows on it."""
    return np.random.default_rng(1000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _many_cells():
    # 64 cells on a 100 x 70 output: an 8 x 8 grid of 11 x 7 rectangles that start off every tile boundary, alternating sources and fits
    cells = []
    for i in range(64):
        cells.append(C(0, i % 3, (3 + (i % 8) * 12, 2 + (i // 8) * 8, 11, 7), fit=i % 3, pad=(i, 2 * i, 3 * i)))
    return cells


# name -> (sources [(h, w)], outputs, cells, indices of the sources that are down)
CASES = {
    # ---- the kinds of axis
    "shrink": ([(37, 53)], [O(9, 16)], [C(0, 0, (0, 0, 16, 9), fit=R.STRETCH)], ()),
    "copy": ([(9, 33)], [O(9, 33)], [C(0, 0, (0, 0, 33, 9), fit=R.STRETCH)], ()),
    "enlarge": ([(4, 5)], [O(11, 12)], [C(0, 0, (0, 0, 12, 11), fit=R.STRETCH)], ()),
    "mixed": ([(10, 40)], [O(23, 13)], [C(0, 0, (0, 0, 13, 23), fit=R.STRETCH)], ()),
    "fit_fill": ([(30, 50)], [O(40, 90, background=(9, 8, 7))],
                 [C(0, 0, (1, 1, 40, 37), fit=R.FIT, pad=(50, 60, 70)), C(0, 0, (45, 3, 44, 20), fit=R.FILL), C(0, 0, (50, 25, 7, 13), fit=R.FIT, pad=(1, 2, 3))], ()),
    # ---- limits and ratios
    "one": ([(5, 7), (1, 1)], [O(3, 4, background=(200, 100, 50))], [C(0, 0, (1, 1, 1, 1), fit=R.STRETCH), C(0, 1, (3, 2, 1, 1), fit=R.STRETCH)], ()),
    "long": ([(3, 16384)], [O(1, 1)], [C(0, 0, (0, 0, 1, 1), fit=R.STRETCH)], ()),
    "band": ([(300, 1100)], [O(5, 20)], [C(0, 0, (0, 0, 20, 5), fit=R.STRETCH)], ()),
    "max_w": ([(3, 16384)], [O(3, 16384)], [C(0, 0, (0, 0, 16384, 3), fit=R.STRETCH), C(0, 0, (5000, 1, 333, 2), fit=R.STRETCH)], ()),
    "max_h": ([(16384, 3)], [O(16384, 3)], [C(0, 0, (0, 0, 3, 16384), fit=R.STRETCH), C(0, 0, (1, 9000, 2, 777), fit=R.STRETCH)], ()),
    # ---- tile seams: 130 x 35 is 5 x 5 tiles; rectangles start and end off tile boundaries, touch all four borders of the output,
    # and the crops touch all four borders of the source
    "seams": ([(80, 300), (41, 67)], [O(35, 130, background=(3, 2, 1))],
              [C(0, 0, (0, 0, 97, 21), crop=(0, 0, 250, 60), fit=R.STRETCH), C(0, 1, (61, 5, 69, 30), crop=(10, 0, 57, 41), fit=R.STRETCH),
               C(0, 0, (0, 19, 70, 16), crop=(37, 22, 263, 58), fit=R.STRETCH), C(0, 1, (33, 9, 45, 17), crop=(0, 3, 30, 38), fit=R.FIT, pad=(90, 91, 92))], ()),
    # ---- order: three overlapping cells, the top-most wins, cell 1 is fully covered by cell 2; source 1 is down; source 0 feeds two cells
    "order": ([(20, 30), (8, 8), (16, 24)], [O(40, 70, background=(10, 20, 30))],
              [C(0, 0, (2, 3, 40, 30), fit=R.STRETCH), C(0, 2, (10, 10, 12, 9), fit=R.STRETCH), C(0, 2, (8, 8, 30, 20), fit=R.FIT, pad=(5, 6, 7)),
               C(0, 1, (30, 1, 25, 25), fit=R.STRETCH, offline=(0, 0, 255)), C(0, 0, (20, 20, 45, 18), crop=(5, 5, 10, 4), fit=R.STRETCH)], (1,)),
    # ---- several outputs in one launch
    "many_cells": ([(20, 31), (9, 9), (64, 48)], [O(70, 100, background=(7, 7, 7))], _many_cells(), ()),
    "many_outputs": ([(24, 40), (17, 13)], [O(6 + i, 20 + 3 * i, fmt=(R.BGR24, R.NV12, R.I420)[i % 3] if i % 2 == 0 else R.BGR24, background=(i, i, i))
                                          for i in range(16)],
                     [C(i, i % 2, (2 * (i % 3), 0, 12 + 2 * (i % 4), 6), fit=R.STRETCH) for i in range(16)], ()),
    # ---- 4:2:0
    "nv12": ([(37, 53), (4, 5)], [O(36, 70, fmt=R.NV12, background=(40, 200, 90))],
             [C(0, 0, (2, 4, 40, 30), fit=R.FIT, pad=(250, 10, 10)), C(0, 1, (34, 2, 30, 22), fit=R.STRETCH), C(0, 0, (44, 20, 26, 16), crop=(7, 5, 39, 30), fit=R.FILL)], ()),
    "i420": ([(37, 53), (4, 5)], [O(36, 70, fmt=R.I420, background=(40, 200, 90))],
             [C(0, 0, (2, 4, 40, 30), fit=R.FIT, pad=(250, 10, 10)), C(0, 1, (34, 2, 30, 22), fit=R.STRETCH), C(0, 0, (44, 20, 26, 16), crop=(7, 5, 39, 30), fit=R.FILL)], ()),
}
RESAMPLING = ("shrink", "enlarge", "mixed", "fit_fill", "band", "seams", "order", "many_cells", "nv12", "i420")   # both axes of some cell are not copies
YUV = ("nv12", "i420", "many_outputs")


@functools.lru_cache(maxsize=None)
def frames(name: str):
    sources, _, _, down = CASES[name]
    return tuple(None if i in down else frame(h, w, 17 * i + len(name)) for i, (h, w) in enumerate(sources))


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """The restatement's BGR pictures of a case, computed once and shared (callers must not write into them)."""
    sources, outputs, cells, _ = CASES[name]
    out = R.compose(sources, outputs, cells, list(frames(name)))
    for a in out:
        a.setflags(write=False)
    return tuple(out)
