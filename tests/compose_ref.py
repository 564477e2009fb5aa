"""Plain NumPy / Python restatement of the compositor (``csrc/compose_rule.h``, ``csrc/compose.hip``): the plan of a cell (crop, fit,
inner picture, kind of each axis), the taps and weights of the three kinds of axis, the one-rounding pixel, the painting order and
the forward BT.601 conversion of the 4:2:0 outputs.  Written from the rules, not from the kernel: whole pictures are resampled with
gathered tap arrays and painted over one another in list order, there are no tiles, no staging and no bands.  The kernel must equal
it exactly: every output byte.

Sizes are ``(height, width)``; rectangles are ``(x, y, w, h)``; colours are ``(b, g, r)``."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

STRETCH, FIT, FILL = 0, 1, 2
SHRINK, COPY, ENLARGE = 0, 1, 2
BGR24, NV12, I420 = 0, 1, 2
ENLARGE_TOTAL = 2048
F32 = np.float32


@dataclasses.dataclass
class Output:
    h: int
    w: int
    fmt: int = BGR24
    background: tuple = (0, 0, 0)


@dataclasses.dataclass
class Cell:
    output: int
    source: int
    rect: tuple                       # x, y, w, h inside the output
    crop: tuple = (0, 0, 0, 0)        # x, y, w, h inside the source; zeros: all of it
    fit: int = FIT
    pad: tuple = (0, 0, 0)
    offline: tuple = (0, 0, 0)


@dataclasses.dataclass
class Plan:
    crop: tuple
    inner: tuple
    kind_x: int
    kind_y: int


def fit_size(sw: int, sh: int, tw: int, th: int):
    """sw x sh fitted into tw x th with the aspect kept: the relatively longer axis fills, the other is rounded to nearest, >= 1."""
    if sw * th >= sh * tw:
        return tw, max(1, (sh * tw + sw // 2) // sw)
    return max(1, (sw * th + sh // 2) // sh), th


def kind(S: int, D: int) -> int:
    return SHRINK if S > D else COPY if S == D else ENLARGE


def total(k: int, S: int) -> int:
    return S if k == SHRINK else 1 if k == COPY else ENLARGE_TOTAL


def plan(src_size, cell: Cell, yuv420: bool) -> Plan:
    sh, sw = src_size
    cx, cy, cw, ch = cell.crop
    if (cx, cy, cw, ch) == (0, 0, 0, 0):
        cx, cy, cw, ch = 0, 0, sw, sh
    rx, ry, rw, rh = cell.rect
    inner = (rx, ry, rw, rh)
    if cell.fit == FIT:
        dw, dh = fit_size(cw, ch, rw, rh)
        if yuv420:
            dw, dh = dw + (dw & 1), dh + (dh & 1)
        ox, oy = (rw - dw) // 2, (rh - dh) // 2
        if yuv420:
            ox, oy = ox & ~1, oy & ~1
        inner = (rx + ox, ry + oy, dw, dh)
    elif cell.fit == FILL:
        nw, nh = fit_size(rw, rh, cw, ch)
        cx, cy, cw, ch = cx + (cw - nw) // 2, cy + (ch - nh) // 2, nw, nh
    return Plan((cx, cy, cw, ch), inner, kind(cw, inner[2]), kind(ch, inner[3]))


def enlarge_table(D: int, S: int):
    """cv::resize's INTER_LINEAR 8-bit table of one axis (csrc/letterbox.h: resize_table): source index and two 11-bit weights."""
    scale = 1.0 / (D / S)
    ofs, c0, c1 = np.empty(D, np.int64), np.empty(D, np.int64), np.empty(D, np.int64)
    for d in range(D):
        f = F32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = F32(f - F32(s))
        if s < 0:
            s, f = 0, F32(0)
        if s >= S - 1:
            s, f = S - 1, F32(0)
        ofs[d] = s
        c0[d] = int(np.rint(F32(F32(1.0) - f) * F32(2048)))
        c1[d] = int(np.rint(f * F32(2048)))
    return ofs, c0, c1


def taps(S: int, D: int):
    """``(idx [D][K], w [D][K], T)``: destination j reads source ``idx[j][k]`` with weight ``w[j][k]`` (0 where a row has fewer taps)."""
    k = kind(S, D)
    if k == COPY:
        return np.arange(D, dtype=np.int64)[:, None], np.ones((D, 1), np.int64), 1
    if k == ENLARGE:
        ofs, c0, c1 = enlarge_table(D, S)
        return np.stack([ofs, np.minimum(ofs + 1, S - 1)], 1), np.stack([c0, c1], 1), ENLARGE_TOTAL
    j = np.arange(D, dtype=np.int64)
    i0, i1 = j * S // D, ((j + 1) * S - 1) // D
    K = int((i1 - i0).max()) + 1
    i = i0[:, None] + np.arange(K, dtype=np.int64)[None, :]
    w = np.minimum((j[:, None] + 1) * S, (i + 1) * D) - np.maximum(j[:, None] * S, i * D)
    w = np.where(i <= i1[:, None], w, 0)
    assert (w >= 0).all() and (w.sum(1) == S).all()
    return np.minimum(i, S - 1), w, S


def resample(crop: np.ndarray, dh: int, dw: int, round_between: bool = False) -> np.ndarray:
    """``crop`` (sh x sw x 3 uint8) at dh x dw: per axis the taps of its kind, ONE rounding for both axes.  ``round_between``: the
    deliberately wrong variant that rounds after the horizontal pass (the discrimination test needs it to differ)."""
    sh, sw = crop.shape[:2]
    xi, xw, tx = taps(sw, dw)
    yi, yw, ty = taps(sh, dh)
    src = crop.astype(np.int64)
    hor = np.zeros((sh, dw, 3), np.int64)
    for k in range(xi.shape[1]):
        hor += src[:, xi[:, k], :] * xw[None, :, k, None]
    if round_between:
        hor = (hor + tx // 2) // tx
        tx = 1
    acc = np.zeros((dh, dw, 3), np.int64)
    for k in range(yi.shape[1]):
        acc += hor[yi[:, k]] * yw[:, k, None, None]
    tot = tx * ty
    return ((acc + tot // 2) // tot).astype(np.uint8)


def pixel(src: np.ndarray, p: Plan, dx: int, dy: int, ch: int) -> int:
    """One channel the slow way, tap by tap (csrc/compose_rule.h: cp_pixel)."""
    cx, cy, cw, chh = p.crop
    xi, xw, tx = taps(cw, p.inner[2])
    yi, yw, ty = taps(chh, p.inner[3])
    acc = 0
    for a in range(yi.shape[1]):
        row = 0
        for b in range(xi.shape[1]):
            row += int(xw[dx, b]) * int(src[cy + int(yi[dy, a]), cx + int(xi[dx, b]), ch])
        acc += row * int(yw[dy, a])
    tot = tx * ty
    return (acc + tot // 2) // tot


def compose(sources, outputs, cells, frames, round_between: bool = False):
    """The BGR pictures of all outputs: ``sources`` [(h, w)], ``frames`` [h x w x 3 uint8 or None (camera down)]."""
    out = []
    for o in outputs:
        img = np.empty((o.h, o.w, 3), np.uint8)
        img[:] = np.asarray(o.background, np.uint8)
        out.append(img)
    for c in cells:
        o = outputs[c.output]
        rx, ry, rw, rh = c.rect
        view = out[c.output][ry:ry + rh, rx:rx + rw]
        f = frames[c.source]
        if f is None:
            view[:] = np.asarray(c.offline, np.uint8)
            continue
        assert f.shape[:2] == tuple(sources[c.source])
        p = plan(sources[c.source], c, o.fmt != BGR24)
        view[:] = np.asarray(c.pad, np.uint8)
        cx, cy, cw, ch = p.crop
        ix, iy, iw, ih = p.inner
        out[c.output][iy:iy + ih, ix:ix + iw] = resample(f[cy:cy + ch, cx:cx + cw, :3], ih, iw, round_between)
    return out


# ---- 4:2:0 ----------------------------------------------------------------------------------------------------------------------
def yuv_y(b, g, r):
    return (269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20


def yuv_u(b, g, r):
    return (-155188 * r - 305135 * g + 460324 * b + (1 << 19) + (128 << 20)) >> 20


def yuv_v(b, g, r):
    return (460324 * r - 385875 * g - 74448 * b + (1 << 19) + (128 << 20)) >> 20


def to_yuv420(img: np.ndarray, chroma_top_left: bool = False):
    """``(Y [h][w], U [h/2][w/2], V [h/2][w/2])`` of an even-sized BGR picture: Y per pixel, U and V of the 2 x 2 block's rounded mean.
    ``chroma_top_left``: the deliberately wrong variant that takes the block's top-left pixel instead."""
    h, w = img.shape[:2]
    assert h % 2 == 0 and w % 2 == 0
    p = img.astype(np.int64)
    Y = yuv_y(p[..., 0], p[..., 1], p[..., 2])
    m = p[0::2, 0::2] if chroma_top_left else (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    U, V = yuv_u(m[..., 0], m[..., 1], m[..., 2]), yuv_v(m[..., 0], m[..., 1], m[..., 2])
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def yuv_to_bgr(Y, U, V):
    """The conversion ``csrc/preprocess.hip`` applies to 4:2:0 input (cv2's integer BT.601 limited range), elementwise on int arrays."""
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    uu, vv, yv = U - 128, V - 128, np.maximum(0, Y - 16) * 1220542 + (1 << 19)
    r = np.clip((yv + 1673527 * vv) >> 20, 0, 255)
    g = np.clip((yv - 852492 * vv - 409993 * uu) >> 20, 0, 255)
    b = np.clip((yv + 2116026 * uu) >> 20, 0, 255)
    return b, g, r


def resolve_format(fmt: int, h: int, w: int, pitch: int = 0, chroma_pitch: int = 0, u_offset: int = 0, v_offset: int = 0):
    """``rtmodt_frame_format``'s zero defaults -> (pitch, chroma pitch, u offset, v offset, span in bytes)."""
    if fmt == BGR24:
        pitch = pitch or 3 * w
        return pitch, 0, 0, 0, pitch * (h - 1) + 3 * w
    pitch = pitch or w
    cp = chroma_pitch or (pitch if fmt == NV12 else pitch // 2)
    uo = u_offset or pitch * h
    crow = w if fmt == NV12 else w // 2
    vo = 0 if fmt == NV12 else (v_offset or uo + cp * (h // 2))
    span = max(pitch * (h - 1) + w, uo + cp * (h // 2 - 1) + crow, vo + cp * (h // 2 - 1) + crow if fmt == I420 else 0)
    return pitch, cp, uo, vo, span


def write_output(buf: np.ndarray, img: np.ndarray, fmt: int, pitch: int = 0, chroma_pitch: int = 0, u_offset: int = 0, v_offset: int = 0,
                 chroma_top_left: bool = False) -> None:
    """Writes picture ``img`` into the flat uint8 buffer ``buf`` the way a run writes a destination: only the rows' own bytes."""
    h, w = img.shape[:2]
    pitch, cp, uo, vo, span = resolve_format(fmt, h, w, pitch, chroma_pitch, u_offset, v_offset)
    assert buf.ndim == 1 and buf.size >= span
    if fmt == BGR24:
        for y in range(h):
            buf[y * pitch:y * pitch + 3 * w] = img[y].reshape(-1)
        return
    Y, U, V = to_yuv420(img, chroma_top_left)
    for y in range(h):
        buf[y * pitch:y * pitch + w] = Y[y]
    for y in range(h // 2):
        if fmt == NV12:
            buf[uo + y * cp:uo + y * cp + w] = np.stack([U[y], V[y]], 1).reshape(-1)
        else:
            buf[uo + y * cp:uo + y * cp + w // 2] = U[y]
            buf[vo + y * cp:vo + y * cp + w // 2] = V[y]


# ---- point mapping (float64, from the plan) -------------------------------------------------------------------------------------
def map_points(p: Plan, xy):
    """Source pixel coordinates (pixel centres at integers) -> output coordinates through the plan of a cell."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    cx, cy, cw, ch = p.crop
    ix, iy, iw, ih = p.inner
    x = (xy[:, 0] + 0.5 - cx) * (iw / cw) - 0.5 + ix
    y = (xy[:, 1] + 0.5 - cy) * (ih / ch) - 0.5 + iy
    return np.stack([x, y], 1)
