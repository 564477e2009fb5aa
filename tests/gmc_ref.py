"""Plain restatement of the camera-motion estimator (csrc/gmc.hip) and the scenes its tests run on.

The rules, per stream and frame (everything a sum is taken over is an integer, so the order of a sum is free):

  luma      Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 of a BGR24 pixel (csrc/jpeg.hip's Y)
  L0        (sum of Y over a d x d cell + d*d // 2) // (d*d); W0 = w // d, H0 = h // d, partial cells dropped
  L1        (sum of L0 over a 4 x 4 cell + 8) >> 4; W1 = W0 // 4, H1 = H0 // 4
  coarse    SAD(dx, dy) = sum |L1prev(x, y) - L1cur(x + dx, y + dy)| over cs <= x < W1 - cs, cs <= y < H1 - cs, |dx|, |dy| <= cs;
            argmin with ties to the smallest dx^2 + dy^2, then the smaller dy, then the smaller dx.  W1, H1 >= 2 cs + 4
  blocks    L0prev in 16 x 16 blocks, raster order, BX = W0 // 16, BY = H0 // 16; block (bx, by) at x0 = 16 bx, y0 = 16 by is searched
            in L0cur at (x0, y0) + 4 coarse + (dx, dy), |dx|, |dy| <= sr, same SAD and tie rule.  reason, the first that holds:
            1 the search window leaves the image (nothing is searched: dx = dy = off = sad = 0), 2 a gradient sum of the previous
            block below min_texture, 3 best SAD > max_sad, 4 best shift on the border of the search square, 5 the block's rectangle
            in full-resolution pixels [16 d bx, 16 d (bx + 1)) x [...] meets a mask box with conf >= mask_conf; 0 valid
  sub-pixel per axis from S-, S0, S+ around the best shift (not on the border): den = S- - 2 S0 + S+; off = 0 when den <= 0 or
            S0 == 0 (an exact match has no sub-pixel part), else 8 (S- - S+) / den rounded half away from zero, clamped to +-8
  points    P = 16 d x0 + 128 d - 8, Q = P + d (16 (4 coarse + shift) + off), per axis, in 1/16 full-resolution pixel
  fit       see fit() below; the result is float32 of [a, 0 - b, tx / 16; b, a, ty / 16] (0 - b: a zero rotation gives +0)
"""
from __future__ import annotations

import math

import numpy as np

OK, FIRST, FEW_BLOCKS, FEW_INLIERS, BAD_SCALE = 0, 1, 2, 3, 4
R_VALID, R_WINDOW, R_TEXTURE, R_SAD, R_BORDER, R_MASK = 0, 1, 2, 3, 4, 5
IDENTITY = np.asarray([1, 0, 0, 0, 1, 0], np.float32)
MAX_STREAMS, MAX_BLOCKS, MAX_W, MAX_H, MAX_HYP = 64, 4096, 3840, 2160, 256

DEFAULTS = dict(downscale=4, coarse_search=8, search=4, min_texture=256, max_sad=4096, mask_conf=0.1, n_hyp=128, seed=1, min_sep=32.0,
                inlier_px=1.5, min_blocks=16, min_inliers=12)


def luma(frame):
    f = np.asarray(frame, np.uint8).astype(np.int64)
    return (19595 * f[..., 2] + 38470 * f[..., 1] + 7471 * f[..., 0] + 32768) >> 16


def pyramid(frame, d):
    y = luma(frame)
    h0, w0 = y.shape[0] // d, y.shape[1] // d
    l0 = (y[:h0 * d, :w0 * d].reshape(h0, d, w0, d).sum((1, 3)) + d * d // 2) // (d * d)
    h1, w1 = h0 // 4, w0 // 4
    l1 = (l0[:h1 * 4, :w1 * 4].reshape(h1, 4, w1, 4).sum((1, 3)) + 8) >> 4
    return l0.astype(np.uint8), l1.astype(np.uint8)


def geometry_ok(h, w, d, cs):
    w1, h1 = w // d // 4, h // d // 4
    return w1 >= 2 * cs + 4 and h1 >= 2 * cs + 4


def tie_key(sad, dx, dy):
    return (int(sad), dx * dx + dy * dy, dy, dx)


def argmin_shift(table, r):
    """table[dy + r][dx + r] -> (dx, dy) by the tie rule."""
    best = None
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            k = tie_key(table[dy + r][dx + r], dx, dy)
            if best is None or k < best:
                best = k
    return best[3], best[2]


def coarse_table(l1p, l1c, cs):
    h1, w1 = l1p.shape
    p = l1p[cs:h1 - cs, cs:w1 - cs].astype(np.int64)
    t = np.zeros((2 * cs + 1, 2 * cs + 1), np.int64)
    for dy in range(-cs, cs + 1):
        for dx in range(-cs, cs + 1):
            t[dy + cs, dx + cs] = np.abs(p - l1c[cs + dy:h1 - cs + dy, cs + dx:w1 - cs + dx].astype(np.int64)).sum()
    return t


def subpixel(sm, s0, sp):
    den = sm - 2 * s0 + sp
    if den <= 0 or s0 == 0:
        return 0
    num = 8 * (sm - sp)
    q = (2 * abs(num) + den) // (2 * den)
    return max(-8, min(8, q if num >= 0 else -q))


def block_motion(l0p, l0c, coarse, d, sr, min_texture, max_sad, mask_xyxy=None, mask_conf_v=None, mask_conf=0.1):
    h0, w0 = l0p.shape
    bx_n, by_n = w0 // 16, h0 // 16
    nb = bx_n * by_n
    cx, cy = 4 * coarse[0], 4 * coarse[1]
    p = l0p.astype(np.int64)
    c = l0c.astype(np.int64)
    n = 2 * sr + 1
    sads = np.zeros((n, n, by_n, bx_n), np.int64)          # per shift, every block at once where the shifted image exists
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            sx, sy = cx + dx, cy + dy
            x_lo, x_hi = max(0, -sx), min(16 * bx_n, w0 - sx)
            y_lo, y_hi = max(0, -sy), min(16 * by_n, h0 - sy)
            diff = np.zeros((16 * by_n, 16 * bx_n), np.int64)
            if x_hi > x_lo and y_hi > y_lo:
                diff[y_lo:y_hi, x_lo:x_hi] = np.abs(p[y_lo:y_hi, x_lo:x_hi] - c[y_lo + sy:y_hi + sy, x_lo + sx:x_hi + sx])
            sads[dy + sr, dx + sr] = diff.reshape(by_n, 16, bx_n, 16).sum((1, 3))
    pb = p[:16 * by_n, :16 * bx_n].reshape(by_n, 16, bx_n, 16)
    gx = np.abs(pb[:, :, :, 1:] - pb[:, :, :, :-1]).sum((1, 3))
    gy = np.abs(pb[:, 1:, :, :] - pb[:, :-1, :, :]).sum((1, 3))
    mask_conf = np.float32(mask_conf)
    boxes = []
    if mask_xyxy is not None:
        for b, cf in zip(np.asarray(mask_xyxy, np.float32).reshape(-1, 4), np.asarray(mask_conf_v, np.float32).reshape(-1)):
            if cf >= mask_conf:
                boxes.append(b)
    out = {k: np.zeros(nb, np.int32) for k in ("reason", "dx", "dy", "offx", "offy", "sad")}
    for by in range(by_n):
        for bx in range(bx_n):
            i = by * bx_n + bx
            x0, y0 = 16 * bx, 16 * by
            if x0 + cx - sr < 0 or y0 + cy - sr < 0 or x0 + cx + sr + 16 > w0 or y0 + cy + sr + 16 > h0:
                out["reason"][i] = R_WINDOW
                continue
            t = sads[:, :, by, bx]
            dx, dy = argmin_shift(t, sr)
            s0 = int(t[dy + sr, dx + sr])
            border = abs(dx) == sr or abs(dy) == sr
            out["dx"][i], out["dy"][i], out["sad"][i] = dx, dy, s0
            if not border:
                out["offx"][i] = subpixel(int(t[dy + sr, dx + sr - 1]), s0, int(t[dy + sr, dx + sr + 1]))
                out["offy"][i] = subpixel(int(t[dy + sr - 1, dx + sr]), s0, int(t[dy + sr + 1, dx + sr]))
            X0, Y0, X1, Y1 = np.float32(16 * d * bx), np.float32(16 * d * by), np.float32(16 * d * (bx + 1)), np.float32(16 * d * (by + 1))
            if gx[by, bx] < min_texture or gy[by, bx] < min_texture:
                r = R_TEXTURE
            elif s0 > max_sad:
                r = R_SAD
            elif border:
                r = R_BORDER
            elif any(b[0] < X1 and b[2] > X0 and b[1] < Y1 and b[3] > Y0 for b in boxes):
                r = R_MASK
            else:
                r = R_VALID
            out["reason"][i] = r
    out["gx"], out["gy"] = gx.reshape(-1), gy.reshape(-1)
    return out


def correspondences(blk, order, bx_n, coarse, d):
    order = np.asarray(order, np.int64)
    bx, by = order % bx_n, order // bx_n
    P = np.stack([16 * d * 16 * bx + 128 * d - 8, 16 * d * 16 * by + 128 * d - 8], 1).astype(np.int64)
    sh = np.stack([16 * (4 * coarse[0] + blk["dx"][order].astype(np.int64)) + blk["offx"][order],
                   16 * (4 * coarse[1] + blk["dy"][order].astype(np.int64)) + blk["offy"][order]], 1)
    return P, P + d * sh


def lcg_pair(seed, k, n):
    """Hypothesis k of n >= 2 correspondences: x = seed + 0x9E3779B9 k; x = 1664525 x + 1013904223; i = (x >> 16) % n; once more;
    j = (x >> 16) % (n - 1), j += 1 when j >= i; all mod 2^32."""
    m = 0xFFFFFFFF
    x = (seed + 0x9E3779B9 * k) & m
    x = (1664525 * x + 1013904223) & m
    i = (x >> 16) % n
    x = (1664525 * x + 1013904223) & m
    j = (x >> 16) % (n - 1)
    if j >= i:
        j += 1
    return i, j


def two_point_model(pi, pj, qi, qj):
    """float64, one rounding per operation: a = num_a / den, b = num_b / den from exact integers; tx = Qix - (a Pix - b Piy);
    ty = Qiy - (b Pix + a Piy)."""
    dpx, dpy, dqx, dqy = int(pj[0] - pi[0]), int(pj[1] - pi[1]), int(qj[0] - qi[0]), int(qj[1] - qi[1])
    den = np.float64(dpx * dpx + dpy * dpy)
    a = np.float64(dpx * dqx + dpy * dqy) / den
    b = np.float64(dpx * dqy - dpy * dqx) / den
    px, py = np.float64(int(pi[0])), np.float64(int(pi[1]))
    tx = np.float64(int(qi[0])) - (a * px - b * py)
    ty = np.float64(int(qi[1])) - (b * px + a * py)
    return a, b, tx, ty


def inliers(model, P, Q, thr2):
    a, b, tx, ty = (np.float64(v) for v in model)
    px, py, qx, qy = (v.astype(np.float64) for v in (P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]))
    rx = ((a * px - b * py) + tx) - qx
    ry = ((b * px + a * py) + ty) - qy
    return (rx * rx + ry * ry) <= thr2


def int_sums(P, Q, m):
    """N, sum Px, sum Py, sum Qx, sum Qy, sum P.Q, sum P x Q, sum |P|^2 over the inliers, as Python integers."""
    px, py, qx, qy = ([int(v) for v in col[m]] for col in (P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]))
    return [len(px), sum(px), sum(py), sum(qx), sum(qy), sum(a * c + b * e for a, b, c, e in zip(px, py, qx, qy)),
            sum(a * e - b * c for a, b, c, e in zip(px, py, qx, qy)), sum(a * a + b * b for a, b in zip(px, py))]


def sums_model(s):
    """Closed-form least-squares similarity from the eight sums; None when it is degenerate.  A = N S(P.Q) - (SPx SQx + SPy SQy),
    B = N S(PxQ) - (SPx SQy - SPy SQx), D = N S|P|^2 - (SPx^2 + SPy^2), exact in int64; a = A / D, b = B / D;
    tx = (SQx - (a SPx - b SPy)) / N, ty = (SQy - (b SPx + a SPy)) / N in float64."""
    n, spx, spy, sqx, sqy, dot, cross, pp = s
    A = n * dot - (spx * sqx + spy * sqy)
    B = n * cross - (spx * sqy - spy * sqx)
    D = n * pp - (spx * spx + spy * spy)
    assert max(abs(A), abs(B), abs(D)) < 2 ** 63
    if D <= 0:
        return None
    a, b = np.float64(A) / np.float64(D), np.float64(B) / np.float64(D)
    fx, fy, nn = np.float64(spx), np.float64(spy), np.float64(n)
    tx = (np.float64(sqx) - (a * fx - b * fy)) / nn
    ty = (np.float64(sqy) - (b * fx + a * fy)) / nn
    return a, b, tx, ty


def fit(P, Q, n_hyp, seed, min_sep, inlier_px, min_blocks, min_inliers):
    """The deterministic robust fit.  Stages not reached leave zeros (scores -1, best_k -1)."""
    n = len(P)
    out = dict(scores=np.full(MAX_HYP, -1, np.int32), best_k=-1, inl=np.zeros((2, n), np.uint8), sums=np.zeros((2, 8), np.int64),
               model=np.zeros((3, 4), np.float64), warp=IDENTITY.copy(), status=OK)
    if n < min_blocks:
        out["status"] = FEW_BLOCKS
        return out
    t = np.float64(16.0) * np.float64(np.float32(inlier_px))
    thr2 = t * t
    s = np.float64(16.0) * np.float64(np.float32(min_sep))
    sep2 = s * s
    best = -1
    for k in range(n_hyp):
        i, j = lcg_pair(seed, k, n)
        dx, dy = int(P[j, 0] - P[i, 0]), int(P[j, 1] - P[i, 1])
        if np.float64(dx * dx + dy * dy) < sep2:
            continue
        sc = int(inliers(two_point_model(P[i], P[j], Q[i], Q[j]), P, Q, thr2).sum())
        out["scores"][k] = sc
        if sc > best:
            best, out["best_k"] = sc, k
    if best < min_inliers:
        out["status"] = FEW_INLIERS
        return out
    i, j = lcg_pair(seed, out["best_k"], n)
    model = two_point_model(P[i], P[j], Q[i], Q[j])
    out["model"][0] = model
    for rnd in range(2):
        m = inliers(model, P, Q, thr2)
        out["inl"][rnd] = m
        sm = int_sums(P, Q, m)
        out["sums"][rnd] = sm
        model = sums_model(sm) if sm[0] >= min_inliers else None
        if model is None:
            out["status"] = FEW_INLIERS
            return out
        out["model"][1 + rnd] = model
    a, b, tx, ty = model
    s2 = a * a + b * b
    if not (s2 >= 0.25 and s2 <= 4.0):
        out["status"] = BAD_SCALE
        return out
    out["warp"] = np.asarray([a, np.float64(0.0) - b, tx / np.float64(16.0), b, a, ty / np.float64(16.0)], np.float64).astype(np.float32)
    return out


class GmcRef:
    """One stream of the estimator."""

    def __init__(self, **cfg):
        self.cfg = dict(DEFAULTS)
        self.cfg.update(cfg)
        self.prev = None

    def reset(self):
        self.prev = None

    def estimate(self, frame, mask_xyxy=None, mask_conf=None):
        """-> (warp float32[6], status, debug dict)."""
        c = self.cfg
        d, cs, sr = c["downscale"], c["coarse_search"], c["search"]
        h, w = frame.shape[:2]
        assert geometry_ok(h, w, d, cs)
        l0, l1 = pyramid(frame, d)
        dbg = dict(l0=l0, l1=l1)
        prev, self.prev = self.prev, (l0, l1)
        if prev is None:
            dbg.update(warp=IDENTITY.copy(), status=FIRST)
            return IDENTITY.copy(), FIRST, dbg
        assert prev[0].shape == l0.shape, "a changed size needs a reset"
        table = coarse_table(prev[1], l1, cs)
        coarse = argmin_shift(table, cs)
        blk = block_motion(prev[0], l0, coarse, d, sr, c["min_texture"], c["max_sad"], mask_xyxy, mask_conf, c["mask_conf"])
        order = np.nonzero(blk["reason"] == R_VALID)[0].astype(np.int32)
        P, Q = correspondences(blk, order, l0.shape[1] // 16, coarse, d)
        f = fit(P, Q, c["n_hyp"], c["seed"], c["min_sep"], c["inlier_px"], c["min_blocks"], c["min_inliers"])
        dbg.update(table=table, coarse=coarse, blk=blk, order=order, P=P, Q=Q, **f)
        return f["warp"], f["status"], dbg


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def canvas(h, w, seed, smooth=9):
    """A seeded uint8 BGR canvas, box-filtered (`smooth` x `smooth`, twice) and stretched back to full contrast, so that its
    texture survives the 4 x 4 average of d = 4."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (h + 4 * smooth, w + 4 * smooth, 3)).astype(np.float64)
    for _ in range(2):
        c = np.cumsum(np.cumsum(np.pad(x, ((1, 0), (1, 0), (0, 0))), 0), 1)
        x = (c[smooth:, smooth:] - c[:-smooth, smooth:] - c[smooth:, :-smooth] + c[:-smooth, :-smooth]) / (smooth * smooth)
    x = x[:h, :w]
    lo, hi = x.min(), x.max()
    return np.clip(np.rint((x - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)


def crop(cv, x, y, h, w):
    return np.ascontiguousarray(cv[y:y + h, x:x + w])


def sample(cv, warp, h, w, origin):
    """The frame a camera sees when frame pixel p shows canvas point origin + M^-1 (p - t) (so that content moves by `warp` = [M | t]
    from the frame at `origin` to this one), float64 bilinear."""
    m = np.asarray(warp, np.float64).reshape(2, 3)
    inv = np.linalg.inv(m[:, :2])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    u = inv[0, 0] * (xs - m[0, 2]) + inv[0, 1] * (ys - m[1, 2]) + origin[0]
    v = inv[1, 0] * (xs - m[0, 2]) + inv[1, 1] * (ys - m[1, 2]) + origin[1]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() + 1 < cv.shape[1] and y0.max() + 1 < cv.shape[0], "the canvas is too small"
    fx, fy = (u - x0)[..., None], (v - y0)[..., None]
    c = cv.astype(np.float64)
    out = (c[y0, x0] * (1 - fx) + c[y0, x0 + 1] * fx) * (1 - fy) + (c[y0 + 1, x0] * (1 - fx) + c[y0 + 1, x0 + 1] * fx) * fy
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def similarity(deg=0.0, scale=1.0, tx=0.0, ty=0.0, centre=(0.0, 0.0)):
    """float64 2x3 [R | t] rotating and scaling about `centre`, then translating."""
    c, s = math.cos(math.radians(deg)) * scale, math.sin(math.radians(deg)) * scale
    cx, cy = centre
    return np.asarray([[c, -s, cx - (c * cx - s * cy) + tx], [s, c, cy - (s * cx + c * cy) + ty]], np.float64)


def corner_error(warp, truth, h, w):
    """The largest displacement error over the four frame corners, pixels."""
    a, b = np.asarray(warp, np.float64).reshape(2, 3), np.asarray(truth, np.float64).reshape(2, 3)
    pts = np.asarray([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], np.float64).T
    return float(np.sqrt((((a - b) @ pts) ** 2).sum(0)).max())


def assert_textured(dbg, min_texture):
    """Every block whose window is inside the frame and that no box masks passes min_texture: nothing passes by being unmeasured."""
    blk = dbg["blk"]
    inside = blk["reason"] != R_WINDOW
    assert inside.any()
    assert (blk["gx"][inside] >= min_texture).all() and (blk["gy"][inside] >= min_texture).all(), "scene too flat for min_texture"


def paint(frame, boxes, colours):
    """Filled rectangles (xyxy, rounded to pixels, clipped)."""
    out = frame.copy()
    h, w = out.shape[:2]
    for b, col in zip(boxes, colours):
        x1, y1, x2, y2 = (int(round(float(v))) for v in b)
        out[max(0, y1):min(h, y2), max(0, x1):min(w, x2)] = col
    return out


def pan_sequence(h, w, seed, steps, margin=160):
    """Frames that are crops of one canvas: frame k sits at margin + the running sum of steps[:k] (content moves by -step)."""
    cv = canvas(h + 2 * margin, w + 2 * margin, seed)
    x, y, out = margin, margin, []
    for k, (sx, sy) in enumerate([(0, 0)] + list(steps)):
        x, y = x + sx, y + sy
        out.append(crop(cv, x, y, h, w))
    return out


def gmc_scene_frames(scene, h=360, w=480, seed=7, margin=120, colours=((40, 200, 90), (200, 60, 180))):
    """botsort_ref.gmc_scene rendered: the camera's path is the running sum of the scene's (negated) warps over one canvas, the two
    objects are filled rectangles at the frame's detection boxes."""
    cv = canvas(h + 2 * margin, w + 2 * margin, seed)
    off, out = np.zeros(2), []
    for b, _, _, _, warp in scene:
        off = off - np.asarray([warp[2], warp[5]], np.float64)
        x, y = int(round(off[0])), int(round(off[1]))
        assert abs(x) <= margin and abs(y) <= margin
        out.append(paint(crop(cv, margin + x, margin + y, h, w), b, colours))
    return out
