"""The stabiliser's rules (``csrc/stab_rule.h``) restated: Python floats (IEEE float64, one rounding per operation, in the header's
order) and Python / NumPy integers.  ``csrc/stab.hip`` is pinned to this bit for bit: path, status, HOLD run, coefficients, bytes.
The four-tap blend is ``lens_ref.sample`` (the restatement of ``lens_model.h`` rule 3), used, not restated.  No GPU, no library."""
from dataclasses import dataclass

import numpy as np

import lens_ref as LR

OK, HOLD, CLAMPED, RESET = 0, 1, 2, 3
ROUND = 6755399441055744.0                                   # 1.5 x 2^52
MIN_DET = 1e-6
MAX_HOLD = 1 << 30
IDENTITY = (1.0, 0.0, 0.0, 0.0)
IDENTITY_WARP = np.float32([1, 0, 0, 0, 1, 0])


@dataclass(frozen=True)
class Rule:
    h: int
    w: int
    leak_shift: int = 6
    max_shift_px: int = 32
    max_rot_milli: int = 35
    max_zoom_milli: int = 50
    crop_zoom_milli: int = 1000
    reset_after: int = 30


def centre(r):
    return float(r.w - 1) / 2.0, float(r.h - 1) / 2.0


def input_ok(W):
    W = [float(np.float32(v)) for v in np.asarray(W).reshape(6)]
    if not all(np.isfinite(v) for v in W):
        return False
    p, q = W[0] * W[4], W[1] * W[3]
    det = p - q
    return det >= MIN_DET or det <= -MIN_DET


def _clamp(v, lo, hi):
    if v > hi:
        return hi, True
    if v < lo:
        return lo, True
    return v, False


def step(r, path, hold, W=None, valid=True):
    """Rules 1 to 5 -> (path, hold, status)."""
    cx, cy = centre(r)
    a, b, t0, t1 = 1.0, 0.0, 0.0, 0.0
    ok = bool(valid) and (W is None or input_ok(W))
    if ok and W is not None:
        W = [float(np.float32(v)) for v in np.asarray(W).reshape(6)]
        a, b, t0, t1 = W[0], W[3], W[2], W[5]
    hold = 0 if ok else (hold + 1 if hold < MAX_HOLD else hold)
    wtx = ((a * cx - b * cy) + t0) - cx
    wty = ((b * cx + a * cy) + t1) - cy
    za, zb, tx, ty = path
    if r.leak_shift > 0:
        k = 1.0 - 1.0 / float(1 << r.leak_shift)
        za, zb, tx, ty = 1.0 + (za - 1.0) * k, zb * k, tx * k, ty * k
    nza, nzb = a * za - b * zb, b * za + a * zb
    ntx, nty = (a * tx - b * ty) + wtx, (b * tx + a * ty) + wty
    if r.reset_after > 0 and hold >= r.reset_after:
        return IDENTITY, 0, RESET
    M, R, Z = float(r.max_shift_px), float(r.max_rot_milli) / 1000.0, float(r.max_zoom_milli) / 1000.0
    ntx, c0 = _clamp(ntx, -M, M)
    nty, c1 = _clamp(nty, -M, M)
    nzb, c2 = _clamp(nzb, -R, R)
    nza, c3 = _clamp(nza, 1.0 - Z, 1.0 + Z)
    return (nza, nzb, ntx, nty), hold, (HOLD if not ok else CLAMPED if (c0 or c1 or c2 or c3) else OK)


def path_ok(r, path):
    za, zb, tx, ty = path
    M, R, Z = float(r.max_shift_px), float(r.max_rot_milli) / 1000.0, float(r.max_zoom_milli) / 1000.0
    return -M <= tx <= M and -M <= ty <= M and -R <= zb <= R and 1.0 - Z <= za <= 1.0 + Z


def affine(r, path):
    """Rule 6 before the rounding -> (sa, sb, U, V)."""
    cx, cy = centre(r)
    z = float(r.crop_zoom_milli) / 1000.0
    za, zb, tx, ty = path
    sa, sb = za / z, zb / z
    U = ((tx + cx) - sa * cx) + sb * cy
    V = ((ty + cy) - sb * cx) - sa * cy
    return sa, sb, U, V


def q16(v):
    return int((v * 65536.0 + ROUND) - ROUND)


def quantise(r, path):
    return tuple(q16(v) for v in affine(r, path))


def positions(coef, h, w):
    """Rule 7's (qx, qy) of every output pixel, int64 [h, w]."""
    A, B, U, V = coef
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return (A * x - B * y + U + 1024) >> 11, (B * x + A * y + V + 1024) >> 11


def sample(src, coef, border=(0, 0, 0)):
    h, w = src.shape[:2]
    qx, qy = positions(coef, h, w)
    return LR.sample(src, (qx, qy, np.zeros((h, w), np.int64)), border)


def point(r, path, to_source, x, y):
    """Rule 8."""
    sa, sb, U, V = affine(r, path)
    if to_source:
        return (sa * x - sb * y) + U, (sb * x + sa * y) + V
    d = sa * sa + sb * sb
    ex, ey = x - U, y - V
    return (sa * ex + sb * ey) / d, (sa * ey - sb * ex) / d


class Ref:
    """What a ``Stabilizer(streams, size, **cfg)`` holds and answers."""

    def __init__(self, streams, size, border=(0, 0, 0), **cfg):
        self.rule = Rule(size[0], size[1], **cfg)
        self.border = border
        self.path = [IDENTITY] * streams
        self.hold = [0] * streams
        self.status = [OK] * streams
        self.coef = [quantise(self.rule, IDENTITY)] * streams

    def process(self, frames, warps=None, valid=None, streams=None):
        out = []
        for i, f in enumerate(frames):
            s = i if streams is None else streams[i]
            W = None if warps is None else np.asarray(warps, np.float32).reshape(-1, 6)[i]
            v = True if valid is None else bool(valid[i])
            self.path[s], self.hold[s], self.status[s] = step(self.rule, self.path[s], self.hold[s], W, v)
            self.coef[s] = quantise(self.rule, self.path[s])
            out.append(sample(np.asarray(f), self.coef[s], self.border))
        return out

    def reset(self, s=None):
        for k in (range(len(self.path)) if s is None else [s]):
            self.path[k], self.hold[k], self.status[k], self.coef[k] = IDENTITY, 0, OK, quantise(self.rule, IDENTITY)

    def load_state(self, s, path, hold=0):
        self.path[s], self.hold[s], self.status[s] = tuple(float(v) for v in path), int(hold), OK
        self.coef[s] = quantise(self.rule, self.path[s])
