"""Geometry cases for the lens corrector beyond its first tile, shared by ``tests/test_lens_cases_cpu.py`` (which proves on the
restatement that every case reaches the paths it is here for) and ``tests/test_gpu_lens_tiles.py`` (which runs them), and the helpers
that lay frames out in padded buffers for both them and ``tests/test_gpu_lens.py``.

``lens_remap`` makes a tile of TILE_W = 256 output pixels x TILE_H = 4 rows per workgroup; a lane makes a run of RUN = 4 pixels, so a
wave covers one row of a tile.  A case names its source and output size as ``(height, width)``, its lens (or a caller's map) and the
extra bytes of destination pitch it is run with; ``promise`` is what the census must find in it."""
import functools
from collections import namedtuple

import numpy as np

import lens_ref as R

TILE_W, TILE_H, RUN = 256, 4, 4
MAX_DIM = 16384
SENT = 0xA5
BORDER = (17, 200, 93)

# promise: the least number of (whole, partial, OUTSIDE) pixels in EVERY 256-pixel tile column; ``last``: the same for the last tile
# column where it is too narrow for the general figure (None: the general one holds there too)
Promise = namedtuple("Promise", "each last", defaults=(None,))
Case = namedtuple("Case", "name src out lens map dextras promise")
GENERIC = Promise((8, 8, 8))


def axis_lens(name, src, out, step_x, step_y, dcx=0.3, dcy=-0.2, ncx=None, ncy=None, f=None):
    """One of R.LENSES on a ``src`` picture: on the axis one output pixel is ``step_x`` x ``step_y`` source pixels, the output pixel
    (ncx, ncy) (default: the output's centre) sees the source's centre moved by (dcx, dcy)."""
    (sh, sw), (oh, ow) = src, out
    f = 0.9 * max(sw, sh) if f is None else f
    return R.Lens(f, f * 1.01, (sw - 1) / 2 + dcx, (sh - 1) / 2 + dcy, R.COEFFS[name], f / step_x, f * 1.01 / step_y,
                  (ow - 1) / 2 if ncx is None else ncx, (oh - 1) / 2 if ncy is None else ncy)


def hostile_map_wide(src=(11, 300), out=(9, 521)):
    """R.hostile_map's NaN, infinities and +-2^20 stand in its first 45 columns only: here they are repeated in the second and third
    tile column."""
    mx, my = R.hostile_map(src, out)
    for at in range(TILE_W, out[1], TILE_W):
        n = min(45, out[1] - at)
        mx[:, at:at + n], my[:, at:at + n] = mx[:, :n], my[:, :n]
    return mx, my


def one_row_map(src=(5, 400), ow=1030):
    """sx runs along the source from before its first column to its last but one; sy steps through above, straddling the top, inside, straddling the bottom and
    below, with period 6: the six pixels of the last tile column (1024..1029) hold every kind."""
    u = np.arange(ow)
    sy = np.array([-1.5, -0.5, 1.0, 2.25, src[0] - 0.5, src[0] + 1.0])[u % 6]
    return (0.388 * u - 1.3).astype(np.float32)[None], sy.astype(np.float32)[None]


def _cases():
    c = []
    add = lambda name, src, out, lens, dextras=(7,), promise=GENERIC, map=None: c.append(Case(name, src, out, lens, map, dextras, promise))
    # 9 columns x 9 rows are too few for 8 of each kind in one tile column: the lone pixel column has every kind
    add("two_tiles_plus_1", (11, 300), (9, 257), axis_lens("barrel", (11, 300), (9, 257), 1.2, 1.9), promise=Promise((8, 8, 8), (1, 1, 1)))
    add("three_tiles_odd", (11, 300), (9, 521), axis_lens("tangential", (11, 300), (9, 521), 0.62, 1.9, dcy=-0.9), dextras=(7, 9))     # pitch 1570, 1572 (wide)
    add("exact_tiles", (13, 523), (8, 512), axis_lens("rational", (13, 523), (8, 512), 1.05, 2.4), dextras=(0,))               # pitch 1536: wide
    add("wide_260", (13, 523), (6, 260), axis_lens("pincushion", (13, 523), (6, 260), 1.9, 4.3, f=940.0), dextras=(0, 1))              # pitch 780: wide; 781: bytes
    # one row of a model lens crosses the source's edge once per side: a map that steps through every kind of pixel within 6 columns
    add("one_row", (5, 400), (1, 1030), None, map=one_row_map(), promise=Promise((8, 8, 8), (1, 1, 1)))
    add("tall", (300, 7), (1030, 5), axis_lens("barrel", (300, 7), (1030, 5), 1.9, 0.31))
    add("tiny_src_1x1", (1, 1), (5, 300), axis_lens("barrel", (1, 1), (5, 300), 0.02, 0.55, ncx=258.0, f=40.0), promise=Promise((0, 8, 8)))
    add("tiny_src_2x2", (2, 2), (4, 264), axis_lens("barrel", (2, 2), (4, 264), 0.02, 1.6, dcx=0.0, dcy=-0.3, ncx=258.0, f=40.0), promise=Promise((0, 8, 8)))
    add("max_width", (3, MAX_DIM), (3, MAX_DIM), axis_lens("barrel", (3, MAX_DIM), (3, MAX_DIM), 1.15, 1.4), dextras=(0,), promise=Promise((0, 0, 0)))
    add("max_height", (MAX_DIM, 3), (MAX_DIM, 3), axis_lens("barrel", (MAX_DIM, 3), (MAX_DIM, 3), 1.4, 1.15), dextras=(1,), promise=Promise((0, 0, 0)))
    add("hostile_map_wide", (11, 300), (9, 521), None, map=hostile_map_wide())
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
MAX_CASES = ("max_width", "max_height")


@functools.lru_cache(maxsize=None)
def table(name):
    """The restated table of a case, built once: (qx, qy, outside), read-only."""
    c = BY_NAME[name]
    t = R.build_model(c.lens, c.src, c.out) if c.lens is not None else R.build_from_map(c.map[0], c.map[1], c.src)
    for a in t:
        a.setflags(write=False)
    return t


def kinds(case, t=None):
    """-> (whole, partial, outside) boolean arrays of the output size: four taps on the source, some off it, OUTSIDE."""
    qx, qy, o = table(case.name) if t is None else t
    sh, sw = case.src
    x0, y0 = qx >> R.BITS, qy >> R.BITS
    outside = o != 0
    whole = ~outside & (x0 >= 0) & (x0 + 1 < sw) & (y0 >= 0) & (y0 + 1 < sh)
    return whole, ~outside & ~whole, outside


def census(case):
    """[(whole, partial, outside)] counts per 256-pixel tile column."""
    ks = kinds(case)
    return [tuple(int(k[:, at:at + TILE_W].sum()) for k in ks) for at in range(0, case.out[1], TILE_W)]


def geometry(case):
    """(tile columns, row bands, the most live lanes a wave has, the live lanes of a wave of the last tile column)."""
    oh, ow = case.out
    tiles_x = -(-ow // TILE_W)
    last = -(-(ow - (tiles_x - 1) * TILE_W) // RUN)
    return tiles_x, -(-oh // TILE_H), min(64, -(-ow // RUN)), last


# ---------------------------------------------------------------------------------------------------------------- frames in buffers
def random_frames(n, size, seed):
    return list(np.random.default_rng(seed).integers(0, 256, (n,) + tuple(size) + (3,), np.uint8))


def smooth_frame(size):
    """Integer ramps per channel -> (frame, G): G is the largest step between horizontally or vertically adjacent pixels of any
    channel (7 for these).  Blue is one ramp across the picture's middle, clipped to 0..255; green and red are ramps folded back at 0
    and 255 (a clipped ramp is flat over most of a wide frame, and a flat region hides a wrong position)."""
    h, w = size
    y, x = np.mgrid[0:h, 0:w]
    fold = lambda t: 255 - np.abs(t % 510 - 255)
    f = np.stack([np.clip(7 * (x - w // 2) + 3 * y + 128, 0, 255), fold(2 * x + 7 * y), fold(7 * x - 5 * y + 40)], -1).astype(np.uint8)
    g = f.astype(np.int64)
    G = int(max(np.abs(np.diff(g, axis=0)).max() if h > 1 else 0, np.abs(np.diff(g, axis=1)).max() if w > 1 else 0))
    return f, G


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def float64_reference(lens, src_size, out_size, frame):
    """Plain float64 bilinear interpolation of ``frame`` at the unquantised positions of R.lens_map; nothing of rules 2 and 3 is used.
    -> (reference [oh, ow, 3] float64, ``inner``: the pixels whose taps, moved by the kernel's rounding of the position or not, all lie
    on the source, ``off``: the pixels whose position is off the source by more than that rounding can bring back)."""
    (sh, sw), (oh, ow) = src_size, out_size
    v, u = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    sx, sy, inside = R.lens_map(lens.resolved(), u, v)
    x0, y0 = np.floor(sx), np.floor(sy)
    inner = inside & (x0 >= 1) & (x0 + 2 <= sw - 1) & (y0 >= 1) & (y0 + 2 <= sh - 1)          # a one-pixel margin on every side
    xi, yi = np.clip(x0, 0, sw - 2).astype(np.int64), np.clip(y0, 0, sh - 2).astype(np.int64)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
    f = frame.astype(np.float64)
    ref = (1 - fy) * ((1 - fx) * f[yi, xi] + fx * f[yi, xi + 1]) + fy * ((1 - fx) * f[yi + 1, xi] + fx * f[yi + 1, xi + 1])
    eps = 1.0 / 64
    off = ~inside | (sx <= -1 - eps) | (sx >= sw + eps) | (sy <= -1 - eps) | (sy >= sh + eps)
    return ref, inner, off


def float64_bound(G):
    """Rule 2 rounds the position to the nearest 1 / 32 pixel, a move of at most 1 / 64 pixel per axis; a bilinear surface changes by at
    most G per pixel along an axis, so the move costs at most 2 G / 64; rule 3's (sum + 512) >> 10 rounds the exact blend by at most 0.5."""
    return 0.5 + G / 32


def float64_check(lens, src_size, out_size, frame, G, out, border):
    """``out`` (the kernel's or the restatement's bytes) against the float64 reference -> (worst error over the inner pixels, how many
    they are, how many pixels are off the source); asserts the bound and that every pixel off the source is exactly the border colour."""
    ref, inner, off = float64_reference(lens, src_size, out_size, frame)
    err = np.abs(out.astype(np.float64) - ref).max(axis=2)
    worst = float(err[inner].max())
    assert worst <= float64_bound(G), (worst, float64_bound(G), np.argwhere(inner & (err > float64_bound(G)))[:8].tolist())
    assert (out[off] == np.asarray(border, np.uint8)).all(), np.argwhere(off & (out != np.asarray(border, np.uint8)).any(axis=2))[:8].tolist()
    return worst, int(inner.sum()), int(off.sum())


def padded(frame, pitch, lead=0):
    """A host frame with rows ``pitch`` bytes apart ``lead`` bytes into its buffer, everything else SENT -> (buffer, view)."""
    h, w, _ = frame.shape
    buf = np.full(lead + h * pitch, SENT, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[lead:], (h, w, 3), (pitch, 3, 1))
    view[...] = frame
    return buf, view


def image(frames, pitch, offset):
    """The bytes of a device buffer that holds ``frames`` one after another from ``offset``, rows ``pitch`` apart, SENT elsewhere."""
    h, w, _ = frames[0].shape
    buf = np.full(offset + len(frames) * h * pitch + 8, SENT, np.uint8)
    for i, f in enumerate(frames):
        np.lib.stride_tricks.as_strided(buf[offset + i * h * pitch:], (h, w, 3), (pitch, 3, 1))[...] = f
    return buf


def rectify(lc, pkg, frames, streams, out_size, *, src_kind, dst_kind, spitch, dpitch, offset=0):
    """One process call in the given memory kinds and pitches -> the output frames; asserts that no byte outside them changed."""
    F = pkg._ffi
    n, (sh, sw), (oh, ow) = len(frames), frames[0].shape[:2], out_size
    if src_kind == "host":
        src, kw = [padded(f, spitch, i)[1] for i, f in enumerate(frames)], {}
    else:
        src = F.DeviceBuffer(offset + n * sh * spitch + 8)
        src.upload(image(frames, spitch, offset))
        kw = dict(stride=spitch, offset=offset)
    blank = [np.full((oh, ow, 3), SENT, np.uint8)] * n
    if dst_kind == "host":
        bufs = [padded(b, dpitch, 3 + i) for i, b in enumerate(blank)]
        got = lc.process(src, streams, [v for _, v in bufs], **kw)
        for i, (buf, view) in enumerate(bufs):
            want = padded(view, dpitch, 3 + i)[0]
            assert np.array_equal(buf, want), f"frame {i}: a byte outside the pixels changed"
        return [np.array(g) for g in got]
    dst = F.DeviceBuffer(offset + n * oh * dpitch + 8)
    dst.upload(image(blank, dpitch, offset))
    assert lc.process(src, streams, dst, out_stride=dpitch, out_offset=offset, **kw) is dst
    raw = dst.download()
    got = [np.array(np.lib.stride_tricks.as_strided(raw[offset + i * oh * dpitch:], (oh, ow, 3), (dpitch, 3, 1))) for i in range(n)]
    assert np.array_equal(raw, image(got, dpitch, offset)), "a byte outside the pixels changed"
    return got


# ---------------------------------------------------------------------------------------------------------------- the kernel's indexing, emulated
# Faults of the tile, wave and run arithmetic of lens_remap, each emulated below on the kernel's own indexing scheme:
#   tile_ignored   u0 without the tile column's term when the table is read: pixel u >= 256 takes table entry u % 256
#   band_swapped   the row band from blockIdx.x % tiles_x and the tile column from blockIdx.x / tiles_x
#   stride_out_w   table rows out_w entries apart where the table has align_up(out_w, 4)
#   full_last_run  the partial run at a row's end written in full: pixels past out_w land in the padding
#   wide_swapped   a full run packed with pixels 1 and 2 exchanged
MUTATIONS = ("tile_ignored", "band_swapped", "stride_out_w", "full_last_run", "wide_swapped")
GUARD = 16                                                   # bytes behind the last row, for full_last_run to land in


def emulate(case, frame, fault=None, dextra=12, border=BORDER):
    """The destination buffer (rows ``3 * out_w + dextra`` bytes apart, SENT elsewhere, GUARD bytes behind) as lens_remap's grid of
    blocks, waves and lanes fills it from the packed table, with ``fault`` (one of MUTATIONS, None: none) built in."""
    assert fault is None or fault in MUTATIONS
    (oh, ow), (qx, qy, o) = case.out, table(case.name)
    tpitch = -(-ow // RUN) * RUN
    tiles_x, bands = -(-ow // TILE_W), -(-oh // TILE_H)
    pq = np.zeros((3, oh, tpitch), np.int64)
    pq[2] = 1                                                # the pad entries are OUTSIDE
    pq[:, :, :ow] = qx, qy, o
    pq = pq.reshape(3, -1)
    b, r, lane = np.meshgrid(np.arange(tiles_x * bands), np.arange(TILE_H), np.arange(64), indexing="ij")
    tx, band = (b // tiles_x, b % tiles_x) if fault == "band_swapped" else (b % tiles_x, b // tiles_x)
    row, u0 = band * TILE_H + r, (tx * 64 + lane) * RUN
    live = (row < oh) & (u0 < ow)
    row, u0, lane = row[live], u0[live], lane[live]
    tu0 = lane * RUN if fault == "tile_ignored" else u0
    at = (row * (ow if fault == "stride_out_w" else tpitch) + tu0)[:, None] + np.arange(RUN)
    px = R.sample(frame, (pq[0][at], pq[1][at], pq[2][at]), border)                        # [threads, RUN, 3]
    npx = np.full(len(row), RUN) if fault == "full_last_run" else np.minimum(RUN, ow - u0)
    if fault == "wide_swapped":
        full = npx == RUN
        px[full, 1], px[full, 2] = px[full, 2].copy(), px[full, 1].copy()
    dpitch = 3 * ow + dextra
    buf = np.full(oh * dpitch + GUARD, SENT, np.uint8)
    for i in range(RUN):
        w = i < npx
        buf[(row[w] * dpitch + 3 * (u0[w] + i))[:, None] + np.arange(3)] = px[w, i]
    return buf


def expected_buffer(case, frame, dextra=12, border=BORDER):
    """What ``emulate`` must give without a fault: R.sample's bytes in the rows, SENT everywhere else."""
    ow = case.out[1]
    return np.concatenate([image([R.sample(frame, table(case.name), border)], 3 * ow + dextra, 0)[:-8], np.full(GUARD, SENT, np.uint8)])
