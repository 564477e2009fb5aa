"""NumPy restatement of the re-identification embedder (csrc/reid.hip), written from its header's rules and from the OSNet paper /
torchreid's module definitions, sharing no code with the package:

* the box rule and the fixed-point bilinear resize (integers: the device's crop tap agrees bit for bit),
* the normalisation table (float32 expression, checked against the package's exactly),
* the network in float64, NHWC, one function per tap so that a tap can be computed from the device's own previous tap
  (teacher forcing) -- with ``emulate=True`` it rounds to fp16 wherever the contract says a value is stored, and with ``mutate=``
  it computes one deliberately wrong network (the defects the tolerances must see),
* the int8 quantiser (float64, sequential norm: tests/deepsort_ref.py's ``quantize_rows``, the rule of rtmodt_appearance_quantize).

PARITY UNPINNED: torchreid and cv2 are installed nowhere this runs; what is pinned is this restatement.
"""
import numpy as np

from deepsort_ref import box_region, quantize_rows  # noqa: F401  (re-exported: the quantiser and the box rule are app_coord's)

H, W, DIM = 256, 128, 512
TAPS = ("crop", "conv1", "maxpool", "conv2.0", "conv2.1", "conv2.2", "conv3.0", "conv3.1", "conv3.2", "conv4.0", "conv4.1", "conv5", "feat")
MUTATIONS = ("bgr", "no_gate", "d3", "no_residual", "maxpool_for_avg", "eps1e-3")
#: first tap each mutation changes
FIRST_TAP = {"bgr": "conv1", "no_gate": "conv2.0", "d3": "conv2.0", "no_residual": "conv2.0", "maxpool_for_avg": "conv2.2", "eps1e-3": "conv1"}

# Tolerances, relative to max|ref64| of the tap.  A tap that is ONE conv from stored inputs (conv1 from the crop, the 1x1 conv of
# conv5, fc from conv5's pooled map) is held to the project's conv bound (tests/conv_ref64.py: 2e-3 * max|ref|); maxpool is exact.
# The others are several stored tensors deep (a block stores 23 fp16 tensors between its input and its output): the bound is
# the emulator's worst error against float64 over the inputs of tests/test_gpu_reid.py (emulator = package torch_forward,
# float32, emulate=True, teacher-forced from the same previous tap), times 2 for the accumulation order it cannot reproduce.
# Measured emulator errors (profiles/reid/README.md has the run): see MEASURED_EMULATOR_ERROR.
TOL_CONV = 2e-3
MEASURED_EMULATOR_ERROR = {"conv2.0": 8.9e-4, "conv2.1": 6.6e-4, "conv2.2": 5.2e-4, "conv3.0": 6.1e-4, "conv3.1": 5.8e-4, "conv3.2": 6.3e-4,
                           "conv4.0": 6.0e-4, "conv4.1": 5.5e-4}
TOL_TAP = {"conv1": TOL_CONV, "maxpool": 0.0, "conv5": TOL_CONV, "feat": TOL_CONV}
TOL_TAP.update({k: 2 * v for k, v in MEASURED_EMULATOR_ERROR.items()})
# free-running feature against float64 end to end: emulator's worst error 2.0e-4 * max|feat| over the same inputs, times 2
MEASURED_EMULATOR_ERROR_FEAT = 2.0e-4
TOL_FEAT = 2 * MEASURED_EMULATOR_ERROR_FEAT


# ---------------------------------------------------------------------------------------------------------------- crop
def axis_map(n_out: int, n_src: int, shift: int):
    """(lo, hi, w0, w1) per output index: f = (2 o + 1) * n_src * shift - 1024 (11 fractional bits; shift = 2048 / (2 n_out))."""
    o = np.arange(n_out, dtype=np.int64)
    f = np.maximum((2 * o + 1) * n_src * shift - 1024, 0)
    lo, w1 = f >> 11, f & 2047
    edge = lo >= n_src - 1
    lo = np.where(edge, n_src - 1, lo)
    w1 = np.where(edge, 0, w1)
    return lo, np.minimum(lo + 1, n_src - 1), 2048 - w1, w1


def resize(rect_bgr: np.ndarray) -> np.ndarray:
    """uint8 BGR rectangle (h, w, 3) -> uint8 RGB crop (256, 128, 3)."""
    src = np.asarray(rect_bgr, np.uint8).astype(np.int64)
    yl, yh, wy0, wy1 = axis_map(H, src.shape[0], 4)
    xl, xh, wx0, wx1 = axis_map(W, src.shape[1], 8)
    top = wx0[None, :, None] * src[yl][:, xl] + wx1[None, :, None] * src[yl][:, xh]
    bot = wx0[None, :, None] * src[yh][:, xl] + wx1[None, :, None] * src[yh][:, xh]
    out = (wy0[:, None, None] * top + wy1[:, None, None] * bot + (1 << 21)) >> 22
    return out[..., ::-1].astype(np.uint8)


def crop(frame: np.ndarray, box):
    """The crop of one box, or None for an empty one (all-zero descriptor, no network work)."""
    reg = box_region(box, frame.shape[0], frame.shape[1])
    if reg is None:
        return None
    x0, y0, x1, y1 = reg
    return resize(frame[y0:y1, x0:x1])


MEAN = np.asarray([0.485, 0.456, 0.406], np.float32)
STD = np.asarray([0.229, 0.224, 0.225], np.float32)


def norm_table() -> np.ndarray:
    v = (np.arange(256, dtype=np.float32) / np.float32(255.0))[:, None]
    return ((v - MEAN[None]) / STD[None]).astype(np.float16)


def network_input(crops_u8: np.ndarray, bgr: bool = False) -> np.ndarray:
    """(n, 256, 128, 3) uint8 RGB -> float64 NHWC input values."""
    t = norm_table().astype(np.float64)
    c = np.asarray(crops_u8)
    if bgr:
        c = c[..., ::-1]
    return np.stack([t[c[..., k], k] for k in range(3)], -1)


# ------------------------------------------------------------------------------------------------------------- network
def _r(x, emulate):
    return x.astype(np.float16).astype(np.float64) if emulate else x


def _pw(x, wb):
    w, b = wb
    return x @ w.astype(np.float64).T + b.astype(np.float64)


def _dw(x, wb):
    w, b = wb
    n, h, ww, c = x.shape
    p = np.zeros((n, h + 2, ww + 2, c))
    p[:, 1:-1, 1:-1] = x
    out = np.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            out += p[:, ky:ky + h, kx:kx + ww] * w[:, ky, kx].astype(np.float64)
    return out + b.astype(np.float64)


def _conv1(x, wb):
    w, b = wb                                            # [16, 7, 7, 3]
    n, h, ww, _ = x.shape
    p = np.zeros((n, h + 6, ww + 6, 3))
    p[:, 3:-3, 3:-3] = x
    out = np.zeros((n, h // 2, ww // 2, 16))
    for ky in range(7):
        for kx in range(7):
            out += p[:, ky:ky + h:2, kx:kx + ww:2] @ w[:, ky, kx, :].astype(np.float64).T
    return out + b.astype(np.float64)


def _maxpool3(x):
    n, h, w, c = x.shape
    p = np.full((n, h + 2, w + 2, c), -np.inf)
    p[:, 1:-1, 1:-1] = x
    return np.max([p[:, ky:ky + h:2, kx:kx + w:2] for ky in range(3) for kx in range(3)], 0)


def _pool2(x, use_max=False):
    q = np.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]])
    return q.max(0) if use_max else q.mean(0)


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def _block(p, x, wts, emulate, mutate):
    relu = lambda t: np.maximum(t, 0.0)  # noqa: E731
    x1 = _r(relu(_pw(x, wts[p + ".conv1"])), emulate)
    f1, f2 = wts[p + ".gate.fc1"], wts[p + ".gate.fc2"]
    x2 = 0.0
    for s, n in (("a", 1), ("b", 2), ("c", 3), ("d", 4)):
        if s == "d" and mutate == "d3":
            n = 3
        u = x1
        for i in range(n):
            u = _r(relu(_dw(_r(_pw(u, wts[f"{p}.conv2{s}.{i}.pw"]), emulate), wts[f"{p}.conv2{s}.{i}.dw"])), emulate)
        if mutate == "no_gate":
            x2 = x2 + u
            continue
        g = _sigmoid(_pw(relu(_pw(u.mean((1, 2)), f1)), f2))
        x2 = x2 + u * g[:, None, None, :]
    x2 = _r(x2, emulate)
    idn = _r(_pw(x, wts[p + ".downsample"]), emulate) if (p + ".downsample") in wts else x
    y = _pw(x2, wts[p + ".conv3"])
    return _r(relu(y if mutate == "no_residual" else y + idn), emulate)


def step(name: str, prev: np.ndarray, wts: dict, emulate: bool = False, mutate=None) -> np.ndarray:
    """Tap ``name`` from the previous tap, float64 NHWC.  For ``conv1`` ``prev`` is the uint8 RGB crop tap; for ``feat`` it is the
    ``conv5`` tap.  ``wts``: the fused dict (for the ``eps1e-3`` mutation pass the dict folded with that eps)."""
    relu = lambda t: np.maximum(t, 0.0)  # noqa: E731
    if name == "conv1":
        return _r(relu(_conv1(network_input(prev, bgr=mutate == "bgr"), wts["conv1"])), emulate)
    x = np.asarray(prev, np.float64)
    if name == "maxpool":
        return _maxpool3(x)
    if name in ("conv2.2", "conv3.2"):
        return _r(_pool2(_r(relu(_pw(x, wts[name])), emulate), use_max=mutate == "maxpool_for_avg"), emulate)
    if name == "conv5":
        return _r(relu(_pw(x, wts["conv5"])), emulate)
    if name == "feat":
        return relu(_pw(_r(x.mean((1, 2)), emulate), wts["fc"]))
    return _block(name, x, wts, emulate, mutate)


def forward(crops_u8: np.ndarray, wts: dict, emulate: bool = False, mutate=None) -> dict:
    """Every tap after the crop, free-running from the uint8 RGB crops."""
    out, x = {}, crops_u8
    for name in TAPS[1:]:
        x = step(name, x, wts, emulate, mutate)
        out[name] = x
    return out


def lsb_bound(feat64: np.ndarray, eps: float) -> int:
    """How many int8 steps the quantised device feature may lie from the quantised float64 feature when every component of the
    device feature is within ``eps`` (= tol * max|feat64| of the test) of it.  With q = 127 f / ||f||, e the error vector (|e_k| <= eps,
    ||e|| <= sqrt(n) eps): |dq_k| <= 127 (|e_k| / ||f|| + |f_k| ||e|| / ||f||^2) <= 127 eps (1 + sqrt(n) max|f| / ||f||) / ||f||
    to first order; the second-order term is below 1e-3 of it for tol <= 1e-2.  Rounding both sides adds one step."""
    f = np.asarray(feat64, np.float64)
    worst = 0.0
    for row in f:
        nrm = float(np.sqrt((row * row).sum()))
        if nrm == 0.0:
            continue
        m = float(np.abs(row).max())
        worst = max(worst, 127.0 * eps * (1.0 + np.sqrt(row.size) * m / nrm) / nrm * 1.001)
    return int(np.ceil(worst)) + 1


# ------------------------------------------------------------------------------------------------- inputs of the GPU tests
def scene_frame(h: int, w: int, pad: int, seed: int):
    """(buffer (h, pitch) uint8, view (h, w, 3)): smooth colour structure plus noise, so that crops differ and no tap is flat."""
    rng = np.random.default_rng(seed)
    pitch = 3 * w + pad
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / (5.0 + c)) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    buf = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (pitch, 3, 1))
    view[...] = np.clip(img, 0, 255).astype(np.uint8)
    return buf, view


def scene_boxes(h: int, w: int, seed: int) -> np.ndarray:
    """17 boxes: inside, overhanging each edge, 1 pixel wide, 1 pixel high, larger than the frame, zero area, NaN, negative, and
    random ones."""
    rng = np.random.default_rng(seed)
    fixed = [[w * 0.11, h * 0.1, w * 0.53, h * 0.89], [-20, h * 0.12, w * 0.3, h * 0.75], [w * 0.2, -15, w * 0.6, h * 0.5],
             [w * 0.7, h * 0.25, w + 34, h * 0.94], [w * 0.15, h * 0.6, w * 0.57, h + 40], [w * 0.4 + 0.2, 5, w * 0.4 + 1.1, h * 0.9],
             [5, h * 0.4, w * 0.9, h * 0.4 + 1.5], [-1e9, -1e9, 1e9, 1e9], [w * 0.3, h * 0.3, w * 0.3, h * 0.7], [float("nan"), 1, 9, 9],
             [-50, -50, -10, -10]]
    rnd = []
    while len(fixed) + len(rnd) < 17:
        x0, y0 = rng.uniform(-5, w - 4), rng.uniform(-5, h - 4)
        rnd.append([x0, y0, x0 + rng.uniform(2, w / 2), y0 + rng.uniform(2, h / 2)])
    return np.asarray(fixed + rnd, np.float32)


EMPTY_ROWS = (8, 9, 10)            # of scene_boxes: zero area, NaN, negative
