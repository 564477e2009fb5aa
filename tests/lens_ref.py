"""The lens corrector's rules restated with NumPy float64 and integers: the parity surface of ``csrc/lens_model.h`` (the table, the
points) and of ``csrc/lens.hip`` (the output bytes).  Every float64 step is one of + - x / in the header's order, each rounded on its
own, so the header, the library and the kernel's table equal this bit for bit; sampling is integer arithmetic.

Sizes are ``(height, width)``; a lens is a ``Lens``; tables are ``(qx, qy, outside)`` of the output size."""
import numpy as np

BITS, ONE, ITERS = 5, 32, 20
LIMIT = 1048576.0                                           # 2^20

# The largest undistort_points residual (pixels) over grid_1080() for the four LENSES at F_1080, measured once with this restatement:
# barrel 5.15e-10, pincushion 6.95e-07, tangential 1.86e-10, rational 2.00e-09 (20 iterations contract slowest on the pincushion
# lens at the corners).  The constant is the largest of them; the tests assert 8 x it, the margin this tree uses for fit_plane.
MEASURED_RESIDUAL_PX = 6.95e-07
RESIDUAL_BOUND_PX = 8 * MEASURED_RESIDUAL_PX

COEFFS = {                                                  # k1 k2 p1 p2 k3 k4 k5 k6
    "barrel": (-0.30, 0.10, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "pincushion": (0.25, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "tangential": (-0.20, 0.05, 0.01, -0.008, 0.01, 0.0, 0.0, 0.0),
    "rational": (0.50, 0.10, 0.001, 0.001, 0.01, 0.70, 0.15, 0.02),
}
LENSES = tuple(COEFFS)


class Lens:
    def __init__(self, fx, fy, cx, cy, k=(0.0,) * 8, nfx=0.0, nfy=0.0, ncx=0.0, ncy=0.0, r2_limit=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k = tuple(float(v) for v in k) + (0.0,) * (8 - len(k))
        self.nfx, self.nfy, self.ncx, self.ncy, self.r2_limit = float(nfx), float(nfy), float(ncx), float(ncy), float(r2_limit)

    def resolved(self):
        if self.nfx == 0.0:
            return Lens(self.fx, self.fy, self.cx, self.cy, self.k, self.fx, self.fy, self.cx, self.cy, self.r2_limit)
        return self

    def as_list(self):                                      # the 17 doubles of rtmodt_lens_params, in order
        return [self.fx, self.fy, self.cx, self.cy, *self.k, self.nfx, self.nfy, self.ncx, self.ncy, self.r2_limit]

    @property
    def K(self):
        return (self.fx, self.fy, self.cx, self.cy)

    @property
    def new_K(self):
        return None if self.nfx == 0.0 else (self.nfx, self.nfy, self.ncx, self.ncy)


def lens_for(name, src_size, out_size=None, zoom=0.6, r2_limit=0.0):
    """One of LENSES on a ``src_size`` picture, seen through output intrinsics that zoom out (borders on every side)."""
    (sh, sw), (oh, ow) = src_size, out_size or src_size
    f = 0.9 * sw
    return Lens(f, f * 1.01, (sw - 1) / 2 + 0.3, (sh - 1) / 2 - 0.2, COEFFS[name], zoom * f, zoom * f * 1.01, (ow - 1) / 2, (oh - 1) / 2, r2_limit)


def fold_lens(r2_limit=0.0):
    """k1 = -0.6 seen from far out on 37 x 23 -> 41 x 19: r (1 - 0.6 r^2) turns back at r^2 = 1 / 1.8, so the rim of the output folds
    back onto the source unless ``r2_limit`` cuts it off."""
    base = lens_for("barrel", (23, 37), (19, 41), zoom=0.3)
    return Lens(base.fx, base.fy, base.cx, base.cy, (-0.6,), base.nfx, base.nfy, base.ncx, base.ncy, r2_limit)


F_1080 = 1100.0


def lens_1080(name):
    return Lens(F_1080, F_1080, 959.5, 539.5, COEFFS[name])


def grid_1080(step=60):
    xs, ys = np.arange(0, 1920, step, dtype=np.float64), np.arange(0, 1080, step, dtype=np.float64)
    g = np.stack(np.meshgrid(np.append(xs, 1919.0), np.append(ys, 1079.0)), -1).reshape(-1, 2)
    return np.ascontiguousarray(g)


# ---------------------------------------------------------------------------------------------------------------- rule 1
def terms(m, x, y):
    """-> (r2, den, rad, dx, dy) at the normalised point(s) (x, y), in lens_model.h's order."""
    k1, k2, p1, p2, k3, k4, k5, k6 = m.k
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    a = r2 * k3
    a = k2 + a
    a = r2 * a
    a = k1 + a
    a = r2 * a
    num = 1.0 + a
    b = r2 * k6
    b = k5 + b
    b = r2 * b
    b = k4 + b
    b = r2 * b
    den = 1.0 + b
    rad = num / den
    two_p1, two_p2 = 2.0 * p1, 2.0 * p2
    e0 = two_p1 * xy
    e1 = 2.0 * xx
    e2 = r2 + e1
    e3 = p2 * e2
    dx = e0 + e3
    g0 = 2.0 * yy
    g1 = r2 + g0
    g2 = p1 * g1
    g3 = two_p2 * xy
    dy = g2 + g3
    return r2, den, rad, dx, dy


def lens_map(m, u, v):
    """Resolved lens, output position(s) -> (sx, sy, inside) with inside False where den or r2_limit say OUTSIDE."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        x, y = (u - m.ncx) / m.nfx, (v - m.ncy) / m.nfy
        r2, den, rad, dx, dy = terms(m, x, y)
        xr, yr = x * rad, y * rad
        xd, yd = xr + dx, yr + dy
        fxd, fyd = m.fx * xd, m.fy * yd
        sx, sy = fxd + m.cx, fyd + m.cy
        inside = den > 0.0
        if m.r2_limit > 0.0:
            inside = inside & ~(r2 > m.r2_limit)
    return sx, sy, inside


# ---------------------------------------------------------------------------------------------------------------- rule 2
def axis_hit(q, size):
    p0, a = q >> BITS, q & (ONE - 1)
    return ((p0 >= 0) & (p0 < size)) | ((a > 0) & (p0 + 1 >= 0) & (p0 + 1 < size))


def quantise(sx, sy, src_size, inside=None):
    """float64 positions -> the canonical (qx, qy, outside)."""
    sh, sw = src_size
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    with np.errstate(all="ignore"):
        ok = (sx > -LIMIT) & (sx < LIMIT) & (sy > -LIMIT) & (sy < LIMIT)
        if inside is not None:
            ok = ok & inside
        tx, ty = np.where(ok, sx, 0.0) * 32.0, np.where(ok, sy, 0.0) * 32.0
        qx, qy = np.floor(tx + 0.5).astype(np.int64), np.floor(ty + 0.5).astype(np.int64)
    ok = ok & axis_hit(qx, sw) & axis_hit(qy, sh)
    return np.where(ok, qx, 0).astype(np.int32), np.where(ok, qy, 0).astype(np.int32), (~ok).astype(np.uint8)


def build_model(lens, src_size, out_size=None):
    m = lens.resolved()
    oh, ow = out_size or src_size
    v, u = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    sx, sy, inside = lens_map(m, u, v)
    return quantise(sx, sy, src_size, inside)


def build_from_map(map_x, map_y, src_size):
    return quantise(np.asarray(map_x, np.float32).astype(np.float64), np.asarray(map_y, np.float32).astype(np.float64), src_size)


# ---------------------------------------------------------------------------------------------------------------- rule 3
def sample(src, table, border=(0, 0, 0)):
    """``src`` (h, w, c) uint8 through the table -> (out_h, out_w, c) uint8."""
    qx, qy, outside = (np.asarray(t).astype(np.int64) for t in table)
    src = np.asarray(src)
    sh, sw, ch = src.shape
    s = src.astype(np.int64)
    bd = np.asarray(border, np.int64).reshape(1, 1, ch)
    x0, y0, ax, ay = qx >> BITS, qy >> BITS, qx & (ONE - 1), qy & (ONE - 1)
    total = np.zeros(qx.shape + (ch,), np.int64)
    for j in (0, 1):
        for i in (0, 1):
            x, y = x0 + i, y0 + j
            w = (ax if i else ONE - ax) * (ay if j else ONE - ay)
            inb = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
            tap = np.where(inb[..., None], s[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)], bd)
            total += w[..., None] * tap
    out = (total + 512) >> 10
    out = np.where(outside[..., None] != 0, bd, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- rule 4
def distort_points(lens, xy):
    m = lens.resolved()
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    sx, sy, _ = lens_map(m, xy[:, 0], xy[:, 1])
    return np.stack([sx, sy], 1)


def undistort_points(lens, xy):
    """-> (rectified points, residuals)."""
    m = lens.resolved()
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    px, py = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        xd, yd = (px - m.cx) / m.fx, (py - m.cy) / m.fy
        x, y = xd, yd
        for _ in range(ITERS):
            _, _, rad, dx, dy = terms(m, x, y)
            nx, ny = xd - dx, yd - dy
            x, y = nx / rad, ny / rad
        ux, vy = m.nfx * x, m.nfy * y
        u, v = ux + m.ncx, vy + m.ncy
        bx, by, _ = lens_map(m, u, v)
        ex, ey = np.abs(bx - px), np.abs(by - py)
        e = np.where(ey > ex, ey, ex)
        res = np.where((ex == ex) & (ey == ey), e, np.inf)
    return np.stack([u, v], 1), res


# ---------------------------------------------------------------------------------------------------------------- shared cases
SIZES = [((23, 37), (19, 41)), ((1, 1), (1, 1))]            # (src, out): 37 x 23 -> 41 x 19 and 1 x 1 -> 1 x 1


def table_cases():
    """[(name, lens, src_size, out_size)]: the four lenses at SIZES."""
    return [(f"{name}_{sw}x{sh}", lens_for(name, (sh, sw), (oh, ow)), (sh, sw), (oh, ow)) for name in LENSES for (sh, sw), (oh, ow) in SIZES]


def hostile_map(src_size=(23, 37), out_size=(19, 41)):
    """A caller's map with NaN, +-inf, +-1e30 and values at +-2^20 among ordinary ones."""
    oh, ow = out_size
    rng = np.random.default_rng(7)
    mx = rng.uniform(-3, src_size[1] + 3, (oh, ow)).astype(np.float32)
    my = rng.uniform(-3, src_size[0] + 3, (oh, ow)).astype(np.float32)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 20, -2.0 ** 20, np.nextafter(np.float32(2.0 ** 20), np.float32(0)),
           -np.nextafter(np.float32(2.0 ** 20), np.float32(0)), -0.0, src_size[1] - 1.0, src_size[1] - 1.0 + 1 / 64, -1.0, -1.0 + 1 / 64, -1 / 64]
    for k, b in enumerate(bad):
        mx[k % oh, (3 * k) % ow] = b
        my[(k + 5) % oh, (3 * k + 1) % ow] = b
        mx[(k + 9) % oh, (3 * k + 2) % ow] = b
        my[(k + 9) % oh, (3 * k + 2) % ow] = b
    return mx, my


def point_cases():
    """[(lens, x, y)] x 64: 16 points for each lens, inside and outside a 1920 x 1080 picture."""
    rng = np.random.default_rng(11)
    out = []
    for name in LENSES:
        lens = Lens(F_1080, F_1080 * 0.99, 961.25, 538.5, COEFFS[name], 900.0, 905.0, 950.0, 545.0)
        pts = rng.uniform((-100, -100), (2020, 1180), (16, 2))
        out += [(lens, float(p[0]), float(p[1])) for p in pts]
    return out
