"""Weights of the DeepSORT re-identification network: OSNet x0.25 (Zhou et al., "Omni-Scale Feature Learning for Person
Re-Identification"; torchreid's ``osnet_x0_25``, eval mode, output = the 512-value feature after ``fc``), the model the reference's
``tracking.deepsort.embedder: "weights/osnet_x0_25.onnx"`` (config/default.yaml:60) names.  ``csrc/reid.hip`` runs it.

An ``.onnx`` file is NOT read (no ONNX package anywhere this runs, and an exported graph has lost the key names): convert the
torchreid checkpoint instead, ``python tools/convert_weights.py --reid osnet_x0_25.pth osnet_x0_25.rtreid``.

Fused dict ``{name: (w float32, b float32)}`` (BatchNorm folded, eps 1e-5):

    conv1                        w[16, 7, 7, 3] (RGB), stride 2, ReLU
    conv{2,3,4}.{0,1}.conv1      w[mid, cin], ReLU                      mid = cout / 4 = 16 / 24 / 32
    ....conv2{a,b,c,d}.{i}.pw    w[mid, mid], no bias (b = 0)           stream a: i = 0; b: 0..1; c: 0..2; d: 0..3
    ....conv2{a,b,c,d}.{i}.dw    w[mid, 3, 3] depthwise, ReLU
    ....gate.fc1 / gate.fc2      w[mid / 16, mid] ReLU / w[mid, mid / 16] sigmoid      (float32 in the file: is_fp32)
    ....conv3                    w[cout, mid], linear
    ....downsample               w[cout, cin], linear (first block of a stage)
    conv{2,3}.2                  w[c, c], ReLU, then a 2x2 average pool
    conv5                        w[128, 128], ReLU
    fc                           w[512, 128] (Linear + BatchNorm1d), ReLU

``RTREID01`` layout (little endian): ``char[8] magic, u32 version (1), u32 n_records, u32 crc32, u32 0`` -- the CRC-32 (zlib's) of
every byte after these 24 -- then ``n_records`` x 96 bytes ``char[48] name, u32 dtype (0 fp16 / 1 fp32), u32 ndim, u32 shape[4],
u64 w_offset, u64 b_offset`` (byte offsets from the start of the file, 64-B aligned; the bias is ``shape[0]`` float32), then the
payloads.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from .weights import fold_bn, read_pt

MAGIC = b"RTREID01"
SUFFIX = ".rtreid"
_HDR = struct.Struct("<8s4I")
_REC = struct.Struct("<48s6I2Q8x")
IN_H, IN_W, FEAT_DIM = 256, 128, 512
MEAN = (0.485, 0.456, 0.406)            # ImageNet, RGB
STD = (0.229, 0.224, 0.225)
STAGES = ((2, 16, 64), (3, 64, 96), (4, 96, 128))      # (torchreid index, cin, cout)
STREAMS = (("a", 1), ("b", 2), ("c", 3), ("d", 4))
#: the 13 tensors csrc/reid.hip keeps in HBM (rtmodt_reid_tap), in network order
TAPS = ("crop", "conv1", "maxpool", "conv2.0", "conv2.1", "conv2.2", "conv3.0", "conv3.1", "conv3.2", "conv4.0", "conv4.1", "conv5", "feat")
#: synthetic(): standard deviation of every tap after conv1 .. feat, over the calibration crops, lies in this range
SYNTHETIC_TAP_STD = (0.05, 8.0)


def is_fp32(name: str) -> bool:
    """The gate's two tiny layers run on the vector ALU in float32 and are stored so; everything else is fp16."""
    return ".gate." in name


def block_names(prefix: str, first: bool) -> list:
    out = [prefix + ".conv1"]
    for s, n in STREAMS:
        for i in range(n):
            out += [f"{prefix}.conv2{s}.{i}.pw", f"{prefix}.conv2{s}.{i}.dw"]
    out += [prefix + ".gate.fc1", prefix + ".gate.fc2", prefix + ".conv3"]
    if first:
        out.append(prefix + ".downsample")
    return out


def layer_shapes() -> dict:
    """``{name: shape of w}`` of every record, in file order."""
    out = {"conv1": (16, 7, 7, 3)}
    for idx, cin, cout in STAGES:
        mid = cout // 4
        for j in (0, 1):
            ci = cin if j == 0 else cout
            for n in block_names(f"conv{idx}.{j}", j == 0):
                leaf = n.rsplit(".", 1)[1]
                out[n] = {"conv1": (mid, ci), "pw": (mid, mid), "dw": (mid, 3, 3), "fc1": (mid // 16, mid), "fc2": (mid, mid // 16),
                          "conv3": (cout, mid), "downsample": (cout, ci)}[leaf]
        if idx != 4:
            out[f"conv{idx}.2"] = (cout, cout)
    out["conv5"] = (128, 128)
    out["fc"] = (FEAT_DIM, 128)
    return out


# ------------------------------------------------------------------------------------------------------------ input side
def norm_table() -> np.ndarray:
    """``table[v][c] = RNE16((v / 255 - mean_c) / std_c)`` evaluated in float32, c in R, G, B: the network's input values."""
    v = np.arange(256, dtype=np.float32)[:, None] / np.float32(255.0)
    t = (v - np.asarray(MEAN, np.float32)[None, :]) / np.asarray(STD, np.float32)[None, :]
    return t.astype(np.float32).astype(np.float16)


def normalize(crop_rgb_u8: np.ndarray) -> np.ndarray:
    """uint8 RGB crops ``(n, 256, 128, 3)`` -> the float32 values of the fp16 input, NHWC."""
    t = norm_table().astype(np.float32)
    c = np.asarray(crop_rgb_u8)
    return np.stack([t[c[..., k], k] for k in range(3)], -1)


# --------------------------------------------------------------------------------------------------------------- forward
def torch_step(name: str, x, weights: dict, dtype=None, emulate: bool = False, on_layer=None):
    """One tap from the previous one, torch CPU, NCHW.  ``x``: the previous tap (for ``"conv1"`` the normalised input
    ``(n, 3, 256, 128)``; for ``"feat"`` the ``conv5`` tap).  ``emulate`` rounds to fp16 wherever csrc/reid.hip stores or
    forms an fp16 value (its header states the contract); arithmetic runs in ``dtype``.  ``on_layer(name, pre) -> scale``
    may rescale a layer's weights in place (calibration)."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    x = x.to(dtype)

    def r(t):
        return t.to(torch.float16).to(dtype) if emulate else t

    def wb(n):
        w, b = weights[n]
        return torch.from_numpy(np.ascontiguousarray(w)).to(dtype), torch.from_numpy(np.ascontiguousarray(b)).to(dtype)

    def lin(n, t, conv):
        w, b = wb(n)
        pre = conv(t, w)
        if on_layer is not None:
            s = on_layer(n, pre)
            if s != 1.0:
                weights[n] = (weights[n][0] * np.float32(s), weights[n][1])
                pre = pre * s
        return pre + b.view(1, -1, *([1] * (pre.dim() - 2)))

    def pw(n, t):
        return lin(n, t, lambda u, w: F.conv2d(u, w[:, :, None, None]))

    def dw(n, t):
        return lin(n, t, lambda u, w: F.conv2d(u, w[:, None], padding=1, groups=w.shape[0]))

    def block(p, t):
        x1 = r(F.relu(pw(p + ".conv1", t)))
        x2 = 0
        fc1w, fc1b = wb(p + ".gate.fc1")
        fc2w, fc2b = wb(p + ".gate.fc2")
        for s, n in STREAMS:
            u = x1
            for i in range(n):
                u = r(F.relu(dw(f"{p}.conv2{s}.{i}.dw", r(pw(f"{p}.conv2{s}.{i}.pw", u)))))
            g = u.mean((2, 3))
            g = torch.sigmoid(F.relu(g @ fc1w.T + fc1b) @ fc2w.T + fc2b)
            x2 = x2 + u * g[:, :, None, None]
        x2 = r(x2)
        idn = r(pw(p + ".downsample", t)) if (p + ".downsample") in weights else t
        return r(F.relu(pw(p + ".conv3", x2) + idn))

    if name == "conv1":
        return r(F.relu(lin("conv1", x, lambda u, w: F.conv2d(u, w.permute(0, 3, 1, 2), stride=2, padding=3))))
    if name == "maxpool":
        return F.max_pool2d(x, 3, 2, 1)
    if name in ("conv2.2", "conv3.2"):
        return r(F.avg_pool2d(r(F.relu(pw(name, x))), 2))
    if name == "conv5":
        return r(F.relu(pw("conv5", x)))
    if name == "feat":
        v = r(x.mean((2, 3)))
        return F.relu(lin("fc", v, lambda u, w: u @ w.T))
    return block(name, x)


def torch_forward(x, weights: dict, dtype=None, emulate: bool = False, on_layer=None) -> dict:
    """All taps after the crop, ``{name: tensor}`` (NCHW; ``feat`` is ``(n, 512)``), from the normalised input ``x``
    ``(n, 3, 256, 128)``.  ``dtype=torch.float64`` is the reference; ``dtype=torch.float32, emulate=True`` the CPU emulator."""
    out = {}
    for name in TAPS[1:]:
        x = torch_step(name, x, weights, dtype, emulate, on_layer)
        out[name] = x
    return out


# ------------------------------------------------------------------------------------------------------ synthetic weights
_BN = ("weight", "bias", "running_mean", "running_var")


def _sd_layers():
    """(fused name, torchreid prefix, kind) of every layer; kind: conv+bn | light | gate | fc."""
    out = [("conv1", "conv1", "convbn")]
    for idx, _, _ in STAGES:
        for j in (0, 1):
            p = f"conv{idx}.{j}"
            out.append((p + ".conv1", p + ".conv1", "convbn"))
            for s, n in STREAMS:
                for i in range(n):
                    # torchreid: conv2a is one LightConv3x3, conv2b..d are nn.Sequential of them
                    out.append((f"{p}.conv2{s}.{i}", f"{p}.conv2{s}" + ("" if s == "a" else f".{i}"), "light"))
            out.append((p + ".gate", p + ".gate", "gate"))
            out.append((p + ".conv3", p + ".conv3", "convbn"))
            if j == 0:
                out.append((p + ".downsample", p + ".downsample", "convbn"))
        if idx != 4:
            out.append((f"conv{idx}.2", f"conv{idx}.2.0", "convbn"))
    out += [("conv5", "conv5", "convbn"), ("fc", "fc", "fc")]
    return out


def from_state_dict(sd: dict, eps: float = 1e-5, dtype=np.float32) -> dict:
    """torchreid ``osnet_x0_25`` ``state_dict`` (values anything ``np.asarray`` accepts; a ``module.`` prefix is accepted) -> the
    fused dict.  ``classifier.*`` and ``num_batches_tracked`` are dropped.  ``weights.fold_bn`` folds BatchNorm in float64 and
    casts once to ``dtype``: float32 is what :func:`round_stored` and :func:`save` take; ``dtype=np.float64`` returns the fold
    itself, which equals the unfolded graph to float64 rounding."""
    sd = {(k[7:] if k.startswith("module.") else k): np.asarray(v) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    sd = {k: v for k, v in sd.items() if not k.startswith("classifier.")}
    shapes = layer_shapes()
    out = {}

    def bn(p):
        return [sd[f"{p}.{k}"] for k in _BN]

    for name, p, kind in _sd_layers():
        if kind == "convbn":
            w, b = fold_bn(sd[p + ".conv.weight"], *bn(p + ".bn"), eps=eps, dtype=dtype)
            out[name] = (w if name == "conv1" else w[:, 0, 0, :], b)
        elif kind == "light":
            w1 = np.asarray(sd[p + ".conv1.weight"], np.float64)[:, :, 0, 0]
            out[name + ".pw"] = (w1, np.zeros(w1.shape[0], np.float64))
            w, b = fold_bn(sd[p + ".conv2.weight"], *bn(p + ".bn"), eps=eps, dtype=dtype)      # (c, 1, 3, 3) -> [c, 3, 3, 1]
            out[name + ".dw"] = (w[..., 0], b)
        elif kind == "gate":
            for f in ("fc1", "fc2"):
                out[f"{name}.{f}"] = (np.asarray(sd[f"{p}.{f}.weight"], np.float64)[:, :, 0, 0], np.asarray(sd[f"{p}.{f}.bias"], np.float64))
        else:                                                                        # Linear (bias) + BatchNorm1d
            g, be, mu, var = bn(p + ".1")
            lb = np.asarray(sd[p + ".0.bias"], np.float64)                           # BN(W v + lb) = fold of W, with the mean moved by lb
            w, b = fold_bn(np.asarray(sd[p + ".0.weight"])[:, :, None, None], g, be, np.asarray(mu, np.float64) - lb, var, eps=eps, dtype=dtype)
            out[name] = (w[:, 0, 0, :], b)
    out = {n: (np.ascontiguousarray(w, dtype=dtype), np.ascontiguousarray(b, dtype=dtype)) for n, (w, b) in out.items()}
    for n, (w, b) in out.items():
        if w.shape != shapes[n] or b.shape != (shapes[n][0],):
            raise ValueError(f"{n}: weight {w.shape} / bias {b.shape}, osnet_x0_25 has {shapes[n]}")
    return {n: out[n] for n in shapes}


def calibration_crops(n: int = 4) -> np.ndarray:
    """uint8 RGB crops ``(n, 256, 128, 3)``: white noise and smooth structure, alternating."""
    from . import synth
    a = synth.frames((n + 1) // 2, IN_H, IN_W, 4321)
    b = synth.structured_frames((n + 1) // 2, IN_H, IN_W, 7)
    return np.stack([(a, b)[i % 2][i // 2] for i in range(n)])


def synthetic_state_dict(seed: int = 0, calibrate: bool = True) -> dict:
    """A seeded torchreid-named ``state_dict`` with BatchNorm left unfolded (small running variances, as real BN layers behind
    small-magnitude convs have: the fold depends visibly on eps).  ``calibrate``: every layer's BN gain is rescaled layer by
    layer, as ``weights.calibrate_`` does, so that its pre-activation has unit standard deviation on :func:`calibration_crops`
    -- random weights through 6 gated residual blocks otherwise die or overflow fp16."""
    rng = np.random.default_rng(seed)
    sd = {}

    def put_bn(p, c):
        sd[p + ".weight"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        sd[p + ".bias"] = rng.normal(0, 0.1, c).astype(np.float32)
        sd[p + ".running_mean"] = rng.normal(0, 0.05, c).astype(np.float32)
        sd[p + ".running_var"] = rng.uniform(0.002, 0.02, c).astype(np.float32)

    shapes = layer_shapes()
    for name, p, kind in _sd_layers():
        if kind == "convbn":
            sh = shapes[name]
            oihw = (sh[0], 3, 7, 7) if name == "conv1" else (sh[0], sh[1], 1, 1)
            sd[p + ".conv.weight"] = rng.normal(0, np.sqrt(1.0 / np.prod(oihw[1:])), oihw).astype(np.float32)
            put_bn(p + ".bn", sh[0])
        elif kind == "light":
            c = shapes[name + ".pw"][0]
            sd[p + ".conv1.weight"] = rng.normal(0, np.sqrt(1.0 / c), (c, c, 1, 1)).astype(np.float32)
            sd[p + ".conv2.weight"] = rng.normal(0, 1.0 / 3.0, (c, 1, 3, 3)).astype(np.float32)
            put_bn(p + ".bn", c)
        elif kind == "gate":
            hid, c = shapes[name + ".fc1"]
            sd[p + ".fc1.weight"] = rng.normal(0, np.sqrt(1.0 / c), (hid, c, 1, 1)).astype(np.float32)
            sd[p + ".fc1.bias"] = rng.normal(0.5, 0.1, hid).astype(np.float32)
            sd[p + ".fc2.weight"] = rng.normal(0, 1.0, (c, hid, 1, 1)).astype(np.float32)
            sd[p + ".fc2.bias"] = rng.normal(0, 0.5, c).astype(np.float32)
        else:
            sd[p + ".0.weight"] = rng.normal(0, np.sqrt(1.0 / 128), (FEAT_DIM, 128)).astype(np.float32)
            sd[p + ".0.bias"] = rng.normal(0, 0.05, FEAT_DIM).astype(np.float32)
            put_bn(p + ".1", FEAT_DIM)
    sd["classifier.weight"] = rng.normal(0, 0.01, (1000, FEAT_DIM)).astype(np.float32)      # dropped by from_state_dict
    sd["classifier.bias"] = np.zeros(1000, np.float32)
    if calibrate:
        _calibrate_sd(sd)
    return sd


def _calibrate_sd(sd: dict) -> None:
    import torch
    fused = from_state_dict(sd)
    x = torch.from_numpy(np.ascontiguousarray(normalize(calibration_crops()).transpose(0, 3, 1, 2)))
    scales = {}

    def on_layer(name, pre):
        if ".pw" in name and ".conv2" in name:
            return 1.0                                   # LightConv's 1x1 has no BN of its own: its depthwise conv's BN absorbs the scale
        sd_ = float(pre.flatten(2).std(dim=2).mean(0).max()) if pre.dim() == 4 else float(pre.std(dim=0).max())
        target = 0.5 if name.endswith((".conv3", ".downsample")) else 1.0           # two of them are added before the block's ReLU
        # keep 5 mantissa bits of the scale: every machine derives the SAME weights from the same seed (see weights.calibrate_)
        m, e = np.frexp(target / max(sd_, 1e-12))
        scales[name] = float(np.ldexp(np.round(m * 32.0) / 32.0, e))
        return scales[name]

    with torch.no_grad():
        torch_forward(x, fused, torch.float32, on_layer=on_layer)
    for name, p, kind in _sd_layers():                   # fused w' = s w, b unchanged  <=>  gamma' = s gamma, beta' = b + mu gamma' / sigma
        bnp = {"convbn": p + ".bn", "light": p + ".bn", "fc": p + ".1"}.get(kind)
        s = scales.get(name + ".dw" if kind == "light" else name)
        if bnp is None or s is None:
            continue
        g, be, mu, var = (np.asarray(sd[f"{bnp}.{k}"], np.float64) for k in _BN)
        sig = np.sqrt(var + 1e-5)
        b = be - mu * g / sig
        if kind == "fc":
            b = be + (np.asarray(sd[p + ".0.bias"], np.float64) - mu) * g / sig
            sd[bnp + ".bias"] = (b - (np.asarray(sd[p + ".0.bias"], np.float64) - mu) * s * g / sig).astype(np.float32)
        else:
            sd[bnp + ".bias"] = (b + mu * s * g / sig).astype(np.float32)
        sd[bnp + ".weight"] = (s * g).astype(np.float32)


def round_stored(weights: dict) -> dict:
    """The values the file holds: fp16 weights (float32 for the gate), float32 biases."""
    return {n: (w.astype(np.float32) if is_fp32(n) else w.astype(np.float16).astype(np.float32), b.astype(np.float32)) for n, (w, b) in weights.items()}


def synthetic(seed: int = 0) -> dict:
    """Seeded synthetic fused weights, rounded as stored: ``from_state_dict(synthetic_state_dict(seed))``.  Guarantee: over
    :func:`calibration_crops`, every tap from ``conv1`` to ``feat`` has a standard deviation inside ``SYNTHETIC_TAP_STD`` -- no tap
    dies, none nears fp16's range."""
    return round_stored(from_state_dict(synthetic_state_dict(seed)))


# ------------------------------------------------------------------------------------------------------------------ file
def _payload(weights: dict) -> bytes:
    shapes = layer_shapes()
    off = _HDR.size + _REC.size * len(shapes)
    recs, blobs = [], []

    def place(blob: bytes):
        nonlocal off
        pad = (-off) % 64
        blobs.append(b"\0" * pad + blob)
        off += pad + len(blob)
        return off - len(blob)

    for n, sh in shapes.items():
        w, b = weights[n]
        if tuple(w.shape) != sh or tuple(b.shape) != (sh[0],):
            raise ValueError(f"{n}: weight {w.shape} / bias {b.shape}, osnet_x0_25 has {sh}")
        f32 = is_fp32(n)
        w_at = place(np.ascontiguousarray(w, dtype=np.float32 if f32 else np.float16).tobytes())
        b_at = place(np.ascontiguousarray(b, dtype=np.float32).tobytes())
        recs.append(_REC.pack(n.encode(), int(f32), len(sh), *(list(sh) + [1] * (4 - len(sh))), w_at, b_at))
    return b"".join(recs) + b"".join(blobs)


def digest(weights: dict) -> str:
    """The file's CRC-32 as 8 hex digits: two machines that print the same digest run the same network."""
    return f"{zlib.crc32(_payload(weights)) & 0xFFFFFFFF:08x}"


def save(path: str, weights: dict) -> str:
    body = _payload(weights)
    crc = zlib.crc32(body) & 0xFFFFFFFF
    with open(path, "wb") as f:
        f.write(_HDR.pack(MAGIC, 1, len(layer_shapes()), crc, 0))
        f.write(body)
    return f"{crc:08x}"


def load(path: str):
    """Returns ``(weights dict (float32 views of what is stored), digest)``; ``ValueError`` on a foreign or damaged file."""
    raw = open(path, "rb").read()
    if len(raw) < _HDR.size:
        raise ValueError(f"{path}: not an RTREID01 weight file")
    magic, ver, n, crc, _ = _HDR.unpack_from(raw, 0)
    if magic != MAGIC or ver != 1:
        raise ValueError(f"{path}: not an RTREID01 weight file")
    if zlib.crc32(raw[_HDR.size:]) & 0xFFFFFFFF != crc:
        raise ValueError(f"{path}: digest mismatch (the file is damaged)")
    out = {}
    for i in range(n):
        name, f32, nd, s0, s1, s2, s3, w_at, b_at = _REC.unpack_from(raw, _HDR.size + i * _REC.size)
        sh = (s0, s1, s2, s3)[:nd]
        w = np.frombuffer(raw, dtype=np.float32 if f32 else np.float16, count=int(np.prod(sh)), offset=w_at).reshape(sh)
        out[name.rstrip(b"\0").decode()] = (w.astype(np.float32), np.frombuffer(raw, dtype=np.float32, count=s0, offset=b_at).copy())
    return out, f"{crc:08x}"


def convert_pt(pt_path: str, out_path: str) -> str:
    """torchreid ``osnet_x0_25`` checkpoint (``.pth`` / ``.pt`` holding the ``state_dict``) -> ``.rtreid``,
    through the restricted reader of ``weights.read_pt`` (no code of the checkpoint runs).  Returns the digest."""
    sd = read_pt(pt_path)
    return save(out_path, round_stored(from_state_dict(sd)))
