"""Scenes for the camera-motion estimator (csrc/gmc.hip) at its default downscale and at its limits, shared by
``tests/test_gmc_cases_cpu.py`` (which proves on the restatement that every case reaches the code it is here for) and
``tests/test_gpu_gmc_limits.py`` (which runs them on the kernels).  Plain NumPy on the scenes of ``tests/gmc_ref.py``; no GPU.

A case is a name, the estimator's parameters, one list of frames per stream and, optionally, one set of mask boxes per stream (the
same boxes with every frame).  Each shape is the smallest at which the code in question can go wrong:

  d4, d4-odd-p*, d4-streams   downscale = 4, the default: the only value that takes gmc_luma_l0's three-dword read, on the rows whose
                              address is a multiple of 4; the other rows take the byte loop.  Tight rows of 3 x 384 bytes are all
                              dwords; pitches that are 1, 2, 3 mod 4 mix the two inside one cell; three staged frames of an odd size
                              start at three different alignments
  d8                          downscale = 8
  widest                      W1 = 960 with coarse_search = 16: gmc_coarse_sad's LDS full to its last column and row
  blocks-4096-d1 / -d2        64 x 64 blocks: gmc_fit's four blocks a thread on all 1024 threads, ord_s / qx_s / qy_s to their ends
  masks-200 / -1024 / -edges  hits that only a later pass of gmc_blocks's 64-lane mask loop sees; the limit; the float edges
  reasons                     every block reason 0..4 and sub-pixel offsets of both signs in one frame
  few-inliers-*               the FEW_INLIERS exits of gmc_fit that pixels can reach (see FEW_INLIERS EXITS below)
  mixed                       FEW_INLIERS, OK and FEW_BLOCKS in one call: workgroups that return early beside one that does not
  crop-view / crop-copy       a host frame that ends on its buffer's last byte, and the same pixels contiguous

FEW_INLIERS EXITS.  gmc_fit has three: (A) after the hypotheses, best score < min_inliers; (B) in refit round 0 and (C) in refit round
1, N < min_inliers or D <= 0.  (A) is min_inliers = best score + 1 and (C) is min_inliers = best score on a scene whose refitted model
keeps fewer blocks than the winning pair did, both with min_inliers read from the restatement's own debug output.  (B) cannot be
reached: round 0 counts the inliers of the winning hypothesis's own model over the same points with the same arithmetic, so its N is
the best score exactly, which exit (A) has already found to be >= min_inliers (tests/test_gmc_cases_cpu.py asserts that equality on
every estimate of every case, and search_refit_0_exit() below, 300 (seed, n_hyp) candidates of the reasons scene, found none); and D = N
S|P|^2 - |SP|^2 is positive by Cauchy-Schwarz as soon as two of the N >= 2 inliers differ, which block centres always do.  So D <= 0
has no case in either round.  BAD_SCALE has none either: a shift inside a search square of +-8 level-0 pixels around one common
coarse shift moves two block centres that are min_sep >= 16 pixels apart by a few percent of their distance, nowhere near a scale of
0.5 or 2.  Both stay covered by reading, and by tests/test_gmc_cpu.py on the restatement's fit() fed points directly."""
import functools
from collections import namedtuple

import numpy as np

import gmc_ref as G

F32 = np.float32
GUARD = 0x5A                                                 # what stands in row padding and around device frames

Boxes = namedtuple("Boxes", "xyxy confidence")               # what CameraMotionEstimator.estimate reads of a Detections
Case = namedtuple("Case", "name cfg streams masks extra", defaults=(None, None))


def padded(frame, pitch):
    """The frame as a view with rows ``pitch`` bytes apart of a buffer of exactly (h - 1) pitch + 3w bytes, GUARD in the padding."""
    h, w, _ = frame.shape
    buf = np.full((h - 1) * pitch + 3 * w, GUARD, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (pitch, 3, 1))
    view[...] = frame
    return view


def frame_bytes(frame):
    """The (h - 1) pitch + 3w bytes a frame (a view with any row pitch) owns, padding included, as they stand in memory."""
    h, w, _ = frame.shape
    return np.lib.stride_tricks.as_strided(frame, ((h - 1) * frame.strides[0] + 3 * w,), (1,)).copy()


def row_residues(frame, d, base):
    """{address % 4} over the rows gmc_luma_l0 reads of a frame at address ``base`` (every read starts 12 x bytes into its row)."""
    h = frame.shape[0] // d * d
    return {(base + r * frame.strides[0]) % 4 for r in range(h)}


def staged_bases(case):
    """Where FrameStage puts the host frames of one call, relative to its (256-byte aligned) allocation: frame i at i h pitch."""
    f = case.streams[0][0]
    return [s * f.shape[0] * f.strides[0] for s in range(len(case.streams))]


def blocks_of(rect, d, bx_n):
    """The blocks the pixel rectangle (x1, y1, x2, y2), integers, x2 / y2 exclusive, meets, by integer arithmetic."""
    x1, y1, x2, y2 = rect
    return {by * bx_n + bx for by in range(y1 // (16 * d), (y2 - 1) // (16 * d) + 1) for bx in range(x1 // (16 * d), (x2 - 1) // (16 * d) + 1)}


# ---------------------------------------------------------------------------------------------------------------- downscale 4 and 8
D4_ODD = (331, 389)                                          # W0 = 97, H0 = 82: a partial cell column and row, 6 x 5 blocks
# content moves by -(step): (-17, -15) then (+18, -14) full-resolution pixels, (-4.25, -3.75) and (4.5, -3.5) level-0 pixels
D4_ODD_STEPS = ((17, 15), (-18, 14))


def _d4():
    return Case("d4", dict(downscale=4), [G.pan_sequence(336, 384, 71, [(16, 0), (-16, 4)], margin=32)])


def _d4_odd(extra):
    h, w = D4_ODD
    pitch = 3 * w + extra
    return Case(f"d4-odd-p{pitch % 4}", dict(downscale=4), [[padded(f, pitch) for f in G.pan_sequence(h, w, 72, D4_ODD_STEPS, margin=40)]])


def _d4_streams():
    h, w = D4_ODD
    steps = (D4_ODD_STEPS, ((-15, 17), (19, 13)), ((-19, 16), (13, 18)))
    return Case("d4-streams", dict(downscale=4), [[padded(f, 3 * w + 2) for f in G.pan_sequence(h, w, 73 + s, steps[s], margin=40)] for s in range(3)])


def _d8():
    return Case("d8", dict(downscale=8, coarse_search=2), [G.pan_sequence(768, 1024, 74, [(32, -32), (-40, 24)], margin=64)])


# ---------------------------------------------------------------------------------------------------------------- the limits
def _widest():
    return Case("widest", dict(downscale=1, coarse_search=16), [G.pan_sequence(160, 3840, 75, [(40, -8), (-52, 12)], margin=64)])


def _blocks_4096(d):
    return Case(f"blocks-4096-d{d}", dict(downscale=d), [G.pan_sequence(1024 * d, 1024 * d, 76 + d, [(4 * d, 4 * d), (-4 * d, -4 * d)], margin=16 * d)])


# ---------------------------------------------------------------------------------------------------------------- masks
MASK_SIZE = (96, 160)                                        # d = 1: 10 x 6 blocks
MASK_RECTS = ((40, 40, 70, 60), (100, 50, 120, 70))          # 3 x 2 and 2 x 2 blocks


def _mask_frames():
    return G.pan_sequence(*MASK_SIZE, 1, [(3, -2), (-5, 4)], margin=32)


def _outside(n):
    """n boxes that meet no block of a 160 x 96 frame: right of it, below it, left of and above it, in turn."""
    i = np.arange(n, dtype=np.float64)
    out = np.stack([200 + i, 10 + 0 * i, 230 + i, 40 + 0 * i], 1)
    out[1::3] = np.stack([10 + i, 100 + i, 60 + i, 140 + i], 1)[1::3]
    out[2::3] = np.stack([-90 - i, -80 - i, -1 - 0 * i, -2 - 0 * i], 1)[2::3]
    return out.astype(F32)


def _masks_many(n, hits):
    """n boxes of confidence 1, all outside the frame except ``hits``: {box index: rectangle}."""
    xy = _outside(n)
    for i, r in hits.items():
        xy[i] = r
    extra = {i: blocks_of(r, 1, MASK_SIZE[1] // 16) for i, r in hits.items()}
    return Case(f"masks-{n}", dict(downscale=1), [_mask_frames()], [Boxes(xy, np.ones(n, F32))], extra)


def _masks_edges():
    """Box 0: confidence == mask_conf, masks.  Box 1: one float32 step below, does not.  Box 2: x2 == X0 of block column 7, box 3: y2 ==
    Y0 of block row 2: neither meets the block it touches (the comparison is strict).  Boxes 4, 5: a NaN coordinate, no hit anywhere."""
    at = F32(G.DEFAULTS["mask_conf"])
    nan = np.nan
    xy = np.asarray([[40, 40, 60, 60], [100, 40, 120, 60], [100, 66, 112, 78], [130, 20, 140, 32], [nan, 0, 160, 96], [0, 0, 160, nan]], F32)
    conf = np.asarray([at, np.nextafter(at, F32(0)), 1, 1, 1, 1], F32)
    bx_n = MASK_SIZE[1] // 16
    extra = {0: blocks_of((40, 40, 60, 60), 1, bx_n), 1: set(), 2: {4 * bx_n + 6}, 3: {1 * bx_n + 8}, 4: set(), 5: set(),
             "below": blocks_of((100, 40, 120, 60), 1, bx_n), "touched": {4 * bx_n + 7, 2 * bx_n + 8}}
    return Case("masks-edges", dict(downscale=1), [_mask_frames()], [Boxes(xy, conf)], extra)


# ---------------------------------------------------------------------------------------------------------------- reasons, statuses
REASONS_SIZE = (192, 320)                                    # d = 1: 20 x 12 blocks
REASONS_CFG = dict(downscale=1, search=4)
REASONS_SEED = 31


def reasons_frames(seed=REASONS_SEED):
    """Three frames.  The background pans by (3, -2) a frame; a 96 x 64 rectangle of another texture moves by (+8, -4) a frame against
    it, beyond search = 4 (reasons 3 and 4); in the second frame a 64 x 64 patch is fresh noise (reason 3 in the second and third
    estimate's eyes); a 64 x 48 patch is flat in every frame (reason 2).  The frame's border blocks are reason 1."""
    h, w = REASONS_SIZE
    m = 48
    bg, fg = G.canvas(h + 2 * m, w + 2 * m, seed), G.canvas(h + 2 * m, w + 2 * m, seed + 1, smooth=5)
    noise = np.random.default_rng(seed + 2).integers(0, 256, (64, 64, 3)).astype(np.uint8)
    out = []
    for k in range(3):
        f = G.crop(bg, m + 3 * k, m - 2 * k, h, w)
        x, y = 176 + 5 * k, 112 - 2 * k                      # content moves by (-3, +2) with the pan, the rectangle by (+8, -4) against it
        f[y:y + 64, x:x + 96] = fg[112:176, 176:272]
        if k == 1:
            f[32:96, 32:96] = noise
        f[16:64, 208:272] = 90
        out.append(f)
    return out


def _reasons():
    return Case("reasons", dict(REASONS_CFG), [reasons_frames()])


@functools.lru_cache(maxsize=None)
def reasons_best_score(seed=REASONS_SEED, n_hyp=G.DEFAULTS["n_hyp"]):
    """The best hypothesis score of the reasons scene's first estimate, from the restatement's debug output."""
    ref = G.GmcRef(**REASONS_CFG, n_hyp=n_hyp)
    fr = reasons_frames(seed)
    ref.estimate(fr[0])
    return int(ref.estimate(fr[1])[2]["scores"].max())


def _few_inliers(which):
    """after-hypotheses: min_inliers = best score + 1.  refit-1: min_inliers = best score."""
    best = reasons_best_score()
    return Case(f"few-inliers-{which}", dict(REASONS_CFG, min_inliers=best + (1 if which == "after-hypotheses" else 0)), [reasons_frames()[:2]])


def _mixed():
    h, w = REASONS_SIZE
    streams = [reasons_frames()[:2], G.pan_sequence(h, w, 77, [(3, -2)], margin=32), [np.full((h, w, 3), 90, np.uint8)] * 2]
    return Case("mixed", dict(REASONS_CFG, min_inliers=reasons_best_score() + 1), streams)


def fit_exit(dbg, min_inliers):
    """Which way fit() left: 'few-blocks', 'after-hypotheses', 'refit-0', 'refit-1' (the three FEW_INLIERS exits) or 'end'."""
    if dbg["status"] == G.FEW_BLOCKS:
        return "few-blocks"
    if dbg["scores"].max() < min_inliers:
        return "after-hypotheses"
    for r in range(2):
        if dbg["sums"][r][0] < min_inliers:
            return f"refit-{r}"
    return "end"


def search_refit_0_exit(seeds=range(31, 56), n_hyps=(1, 2, 3, 5, 8, 16, 32, 64, 100, 128, 200, 256)):
    """The case search the module docstring quotes (25 x 12 = 300 candidates, half a minute; no test runs it): the (seed, n_hyp) of the
    reasons scene at which refit round 0 counts another N than the best score.  It returns []."""
    found = []
    for seed in seeds:
        fr = reasons_frames(seed)
        for n_hyp in n_hyps:
            ref = G.GmcRef(**REASONS_CFG, n_hyp=n_hyp, min_inliers=2)
            ref.estimate(fr[0])
            dbg = ref.estimate(fr[1])[2]
            if dbg["status"] != G.FEW_BLOCKS and dbg["scores"].max() >= 2 and int(dbg["sums"][0][0]) != int(dbg["scores"].max()):
                found.append((seed, n_hyp))
    return found


# ---------------------------------------------------------------------------------------------------------------- crops
def _crop(view):
    frames = G.pan_sequence(96, 160, 78, [(3, -2), (-5, 4)], margin=32)
    if not view:
        return Case("crop-copy", dict(downscale=1), [frames])
    out = []
    for f in frames:
        big = np.full((96 + 3, 165, 3), GUARD, np.uint8)
        big[-96:, 5:] = f
        out.append(big[-96:, 5:])                            # its last pixel is the buffer's last: nothing is owned behind it
    return Case("crop-view", dict(downscale=1), [out])


_BUILDERS = {
    "d4": _d4, "d4-odd-p1": lambda: _d4_odd(2), "d4-odd-p2": lambda: _d4_odd(3), "d4-odd-p3": lambda: _d4_odd(4), "d4-streams": _d4_streams,
    "d8": _d8, "widest": _widest, "blocks-4096-d1": lambda: _blocks_4096(1), "blocks-4096-d2": lambda: _blocks_4096(2),
    "masks-200": lambda: _masks_many(200, {130: MASK_RECTS[0], 199: MASK_RECTS[1]}), "masks-1024": lambda: _masks_many(1024, {1023: MASK_RECTS[0]}),
    "masks-edges": _masks_edges, "reasons": _reasons, "few-inliers-after-hypotheses": lambda: _few_inliers("after-hypotheses"),
    "few-inliers-refit-1": lambda: _few_inliers("refit-1"), "mixed": _mixed, "crop-view": lambda: _crop(True), "crop-copy": lambda: _crop(False),
}
NAMES = tuple(_BUILDERS)
D4_NAMES = ("d4", "d4-odd-p1", "d4-odd-p2", "d4-odd-p3", "d4-streams")


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    for st in c.streams:
        for f in st:
            f.setflags(write=False)
    return c


def geometry(c):
    h, w = c.streams[0][0].shape[:2]
    d = c.cfg["downscale"]
    w0, h0 = w // d, h // d
    return dict(h=h, w=w, W0=w0, H0=h0, W1=w0 // 4, H1=h0 // 4, BX=w0 // 16, BY=h0 // 16, nb=(w0 // 16) * (h0 // 16))


@functools.lru_cache(maxsize=None)
def reference(name, masked=True):
    """The restatement's (warp, status, debug) of a case, computed once: [frame][stream].  ``masked`` False: without the case's boxes."""
    c = case(name)
    refs = [G.GmcRef(**c.cfg) for _ in c.streams]
    out = []
    for f in range(len(c.streams[0])):
        row = []
        for s, ref in enumerate(refs):
            m = c.masks[s] if masked and c.masks is not None else None
            row.append(ref.estimate(c.streams[s][f], None if m is None else m.xyxy, None if m is None else m.confidence))
        out.append(row)
    return out
