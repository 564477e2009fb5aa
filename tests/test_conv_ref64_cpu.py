"""CPU: the float64 conv check of tests/conv_ref64.py against an emulator of the kernels' rounding contract.

The emulator accumulates fp32 in 32-wide K blocks (one MFMA-like rounding per block, then a serial fp32 sum of the blocks),
evaluates csrc/common.h ``silu2`` in float32 (``x * k``, exp2, ``1 + t``, reciprocal, ``x * d``) and stores RNE16.  Run over
the network's shape classes it must pass the bracket and the exact_frac floors; each planted bug must fail the check.  For
each bug the test also prints whether the old ``2e-3 * max|ref| + 2e-3`` tolerance against an fp32 oracle would have caught it."""
import zlib

import numpy as np
import pytest

from oracle import yolo_oracle as Y
from tests import conv_ref64 as C

F32, F16 = np.float32, np.float16


def im2col(x, k, stride):
    h, w, cin = x.shape
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1
    xp = np.zeros((h + 2 * p, w + 2 * p, cin), np.float64)
    xp[p:p + h, p:p + w] = x
    cols = np.empty((ho, wo, k, k, cin), np.float64)
    for kh in range(k):
        for kw in range(k):
            cols[:, :, kh, kw, :] = xp[kh:kh + stride * (ho - 1) + 1:stride, kw:kw + stride * (wo - 1) + 1:stride, :]
    return cols.reshape(ho * wo, k * k * cin), (ho, wo)


def silu2_f32(z):
    z = z.astype(F32)
    with np.errstate(over="ignore"):
        t = (z * F32(C.K32)).astype(F32)
        e = np.exp2(t).astype(F32)
        d = (F32(1) + e).astype(F32)
        r = (F32(1) / d).astype(F32)
    return (z * r).astype(F32)


def rtz16(v):
    """fp32 -> fp16 rounded toward zero."""
    h = v.astype(F16)
    over = np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))
    return np.where(over, np.nextafter(h, F16(0)), h)


def emulate(x, w, b, stride=1, act=1, res=None, bug=None):
    """The contract in fp32 (or one planted bug): returns the stored fp16 tensor (H, W, cout) as float64."""
    cout, k = w.shape[0], w.shape[1]
    w = w.copy()
    b = b.astype(F32).copy()
    if bug == "drop8":
        w[..., -8:] = 0
    if bug == "bias_lost":
        b[int(np.argmax(np.abs(b)))] = 0
    cols, (ho, wo) = im2col(np.asarray(x, np.float64), k, stride)
    wm = w.reshape(cout, -1).astype(np.float64)
    if bug == "tap_drop":                                      # the centre tap missing for the last (partial) 16-pixel tile
        tail = (ho * wo) % 16 or 16
        c = (k * k // 2) * w.shape[3]
        cols[-tail:, c:c + w.shape[3]] = 0
    K = cols.shape[1]
    nb = -(-K // 32)
    cp = np.zeros((cols.shape[0], nb * 32)); cp[:, :K] = cols
    wp = np.zeros((cout, nb * 32)); wp[:, :K] = wm
    blk = np.einsum("mbk,nbk->mnb", cp.reshape(-1, nb, 32), wp.reshape(cout, nb, 32))
    acc = np.zeros(blk.shape[:2], F32)
    for j in range(nb):
        if bug == "psum16":
            acc = (acc.astype(F32) + blk[:, :, j].astype(F32)).astype(F16).astype(F32)
        else:
            acc = (acc + blk[:, :, j].astype(F32)).astype(F32)
    if bug == "bias_after16":
        acc = acc.astype(F16).astype(F32)
    z = (acc + b[None, :]).astype(F32)
    if act and bug == "silu16":
        z16 = z.astype(F16)
        with np.errstate(over="ignore"):
            s = (z16 / (F16(1) + np.exp(-z16).astype(F16)).astype(F16)).astype(F16).astype(F32)
    elif act:
        s = silu2_f32(z)
    else:
        s = z
    s = s.reshape(ho, wo, cout)
    if res is not None:
        r = np.asarray(res, F32)
        if bug == "res_shift":
            r = np.concatenate([r[:, 1:], r[:, :1]], axis=1)
        if bug == "res_double":
            return (s.astype(F16).astype(F32) + r).astype(F16).astype(np.float64)
        s = (s + r).astype(F32)
    return (rtz16(s) if bug == "rtz" else s.astype(F16)).astype(np.float64)


def data(rng, h, w, cin, cout, k, image=False):
    if image:
        x = (rng.integers(0, 256, (h, w, cin)) / 255.0).astype(F16)
    else:
        x = Y.silu(rng.normal(0.0, 1.5, (h, w, cin)).astype(F32)).astype(F16)
    wt = (rng.normal(0.0, 1.0, (cout, k, k, cin)) * np.sqrt(2.0 / (k * k * cin))).astype(F16).astype(F32)
    b = rng.normal(0.0, 0.3, cout).astype(F32)
    return x.astype(np.float64), wt, b


def old_ok(x, w, b, stride, act, res, got):
    """The old check: |got - ref_fp32| <= 2e-3 max|ref| + 2e-3 (fp32 oracle on the same fp16 inputs)."""
    ref = Y.conv2d_nhwc(x.astype(F32), w, b, stride=stride, act=act)
    if res is not None:
        ref = (ref + res.astype(F32)).astype(F32)
    return float(np.abs(ref - got).max()) <= 2e-3 * float(np.abs(ref).max()) + 2e-3


# name: (h, w, cin, cout, k, stride, residual, image input)
CLASSES = {
    "stem K=27 s2": (70, 58, 3, 32, 3, 2, False, True),
    "3x3 cin16": (37, 29, 16, 16, 3, 1, False, False),
    "3x3 cin48 s2": (45, 33, 48, 96, 3, 2, False, False),
    "3x3 cin128 s1 + res": (40, 40, 128, 64, 3, 1, True, False),
    "3x3 cin64 s1 partial tiles": (23, 19, 64, 64, 3, 1, False, False),
    "1x1 cin96": (30, 26, 96, 64, 1, 1, False, False),
}


def new_ok(r, got, floor):
    ok, frac, worst = r.check(got)
    return ok and frac >= floor, ok, frac, worst


@pytest.mark.parametrize("cls", list(CLASSES))
def test_emulated_contract_passes(cls):
    h, w, cin, cout, k, s, has_res, image = CLASSES[cls]
    rng = np.random.default_rng(zlib.crc32(cls.encode()))
    x, wt, b = data(rng, h, w, cin, cout, k, image)
    res = None
    if has_res:
        res = Y.silu(rng.normal(0.0, 1.5, ((h + s - 1) // s, (w + s - 1) // s, cout)).astype(F32)).astype(F16).astype(np.float64)
    got = emulate(x, wt, b, s, 1, res)
    r = C.conv64(x, wt, b, s, 1, res)
    ok, frac, worst = r.check(got)
    print(f"{cls}: K={r.K} exact_frac {frac:.4f}, worst {worst['ratio']:.3f} of bracket, median bracket {np.median((r.hi16 - r.lo16) / np.spacing(np.abs(r.t16).astype(F16)).astype(np.float64)):.1f} ulp16")
    assert ok, worst
    assert frac >= C.FLOOR_STORED, frac


@pytest.mark.parametrize("pair", ["1x1 tail (3x3 s2 -> 1x1)", "bottleneck (3x3 -> 3x3 + x)", "front end (stem -> 3x3 s2 -> 1x1)"])
def test_emulated_pair_behind_fp16_intermediate(pair):
    """The consumer of an LDS-resident fp16 intermediate: reference from RNE16(t64), bound widened by the flip term."""
    rng = np.random.default_rng(len(pair))
    if pair.startswith("1x1"):
        x, w1, b1 = data(rng, 41, 35, 64, 128, 3)
        _, w2, b2 = data(rng, 1, 1, 128, 64, 1)
        chain = [(w1, b1, 2, None), (w2, b2, 1, None)]
    elif pair.startswith("bottleneck"):
        x, w1, b1 = data(rng, 40, 36, 64, 64, 3)
        _, w2, b2 = data(rng, 1, 1, 64, 64, 3)
        chain = [(w1, b1, 1, None), (w2, b2, 1, "x")]
    else:
        x, w1, b1 = data(rng, 66, 62, 3, 32, 3, image=True)
        _, w2, b2 = data(rng, 1, 1, 32, 64, 3)
        _, w3, b3 = data(rng, 1, 1, 64, 64, 1)
        chain = [(w1, b1, 2, None), (w2, b2, 2, None), (w3, b3, 1, None)]
    t, ref = x, None
    for wt, b, s, res in chain:
        rr = x if res == "x" else None
        t = emulate(t, wt, b, s, 1, rr)
        ref = C.conv64(x if ref is None else ref.t16, wt, b, s, 1, rr, dx=None if ref is None else ref.dev)
    ok, frac, worst = ref.check(t)
    print(f"{pair}: consumer exact_frac {frac:.4f} (floor {C.FLOOR_BEHIND}), worst {worst['ratio']:.3f} of bracket")
    assert ok, worst
    assert ref.behind and frac >= C.FLOOR_BEHIND, frac


MUTATIONS = ["rtz", "silu16", "bias_after16", "psum16", "drop8", "bias_lost", "res_shift", "tap_drop", "res_double"]


@pytest.mark.parametrize("bug", MUTATIONS)
def test_planted_bug_is_rejected(bug):
    """3x3x128 (K = 1152) with a residual on a 40 x 38 map (not a multiple of 16 pixels): each planted bug fails the bracket or the floor."""
    rng = np.random.default_rng(7)
    x, wt, b = data(rng, 40, 38, 128, 64, 3)
    res = Y.silu(rng.normal(0.0, 1.5, (40, 38, 64)).astype(F32)).astype(F16).astype(np.float64)
    r = C.conv64(x, wt, b, 1, 1, res)
    good = emulate(x, wt, b, 1, 1, res)
    assert new_ok(r, good, C.FLOOR_STORED)[0]
    got = emulate(x, wt, b, 1, 1, res, bug=bug)
    passed, bracket, frac, worst = new_ok(r, got, C.FLOOR_STORED)
    print(f"{bug}: bracket {'ok' if bracket else 'VIOLATED'}, exact_frac {frac:.4f}; old 2e-3 tolerance: {'passes (missed)' if old_ok(x, wt, b, 1, 1, res, got) else 'caught'}")
    assert not passed, (bug, frac, worst)


# Detect's class-branch shapes at class counts other than 80: name: (h, w, cin, cout, k, act).  cv3.l.2 has cout = align4(nc)
# (4 for nc 1..4, 8 for nc 5..8) and no activation; on n, ccls = max(64, min(nc, 100)) is the cin of cv3.l.1 (3x3) and cv3.l.2
HEAD_CLASSES = {
    "head 1x1 cin64 cout4 (n, nc 1..4)": (24, 22, 64, 4, 1, 0),
    "head 1x1 cin128 cout8 (s, nc 5..8)": (24, 22, 128, 8, 1, 0),
    "head 1x1 cin88 cout88 (n, nc 88)": (24, 22, 88, 88, 1, 0),
    "head 3x3 cin88 (n, nc 88)": (24, 22, 88, 88, 3, 1),
    "head 3x3 cin100 (ccls 100)": (24, 22, 100, 100, 3, 1),
}


@pytest.mark.parametrize("cls", list(HEAD_CLASSES))
def test_emulated_contract_passes_head_widths(cls):
    h, w, cin, cout, k, act = HEAD_CLASSES[cls]
    rng = np.random.default_rng(zlib.crc32(cls.encode()))
    x, wt, b = data(rng, h, w, cin, cout, k)
    got = emulate(x, wt, b, 1, act)
    r = C.conv64(x, wt, b, 1, act)
    ok, frac, worst = r.check(got)
    print(f"{cls}: K={r.K} exact_frac {frac:.4f}, worst {worst['ratio']:.3f} of bracket")
    assert ok, worst
    assert frac >= C.FLOOR_STORED, frac


@pytest.mark.parametrize("cls,bug", [(c, m) for c, v in HEAD_CLASSES.items() for m in MUTATIONS
                                     if not m.startswith("res_") and not (m == "tap_drop" and v[4] == 1) and not (m == "silu16" and not v[5])])
def test_planted_bug_is_rejected_at_head_widths(cls, bug):
    """The planted bugs that apply to a conv without a residual (and, for tap_drop, with taps; silu16, with an activation) are
    rejected at the narrow head couts and the cin 88 / 100 K-chunk shapes too."""
    h, w, cin, cout, k, act = HEAD_CLASSES[cls]
    rng = np.random.default_rng(zlib.crc32(cls.encode()))
    x, wt, b = data(rng, h, w, cin, cout, k)
    r = C.conv64(x, wt, b, 1, act)
    assert new_ok(r, emulate(x, wt, b, 1, act), C.FLOOR_STORED)[0]
    passed, bracket, frac, worst = new_ok(r, emulate(x, wt, b, 1, act, bug=bug), C.FLOOR_STORED)
    print(f"{cls} {bug}: bracket {'ok' if bracket else 'VIOLATED'}, exact_frac {frac:.4f}")
    assert not passed, (cls, bug, frac, worst)



# ---------------------------------------------------------------------------------------------------------------- decode
def decode_f32(maps, bug=None, strides=(8, 16, 32), nc=80):
    """decode_row in float32 (NumPy): the kernel's operation order; ``bug`` plants a half-pixel anchor shift or an fp16 softmax."""
    cols = []
    for m, st in zip(maps, strides):
        h, w, _ = m.shape
        box = m[..., :64].reshape(h * w, 4, 16).astype(F32)
        d = (box - box.max(axis=2, keepdims=True)).astype(F32)
        if bug == "softmax16":
            e = np.exp(d.astype(F16)).astype(F16)
            p = (e / e.sum(axis=2, keepdims=True, dtype=F16)).astype(F16).astype(F32)
        else:
            e = np.exp(d).astype(F32)
            sm = np.zeros(e.shape[:2], F32)
            for k in range(16):
                sm = (sm + e[..., k]).astype(F32)
            p = (e / sm[..., None]).astype(F32)
        dist = np.zeros(p.shape[:2], F32)
        for k in range(16):
            dist = (dist + (p[..., k] * F32(k)).astype(F32)).astype(F32)
        yy, xx = np.mgrid[0:h, 0:w]
        off = F32(0.0 if bug == "anchor" else 0.5)
        ax, ay = xx.reshape(-1).astype(F32) + off, yy.reshape(-1).astype(F32) + off
        x1, y1, x2, y2 = ax - dist[:, 0], ay - dist[:, 1], ax + dist[:, 2], ay + dist[:, 3]
        xywh = np.stack([((x1 + x2) / F32(2)) * F32(st), ((y1 + y2) / F32(2)) * F32(st), (x2 - x1) * F32(st), (y2 - y1) * F32(st)])
        z = m[..., 64:64 + nc].reshape(h * w, nc).T.astype(F32)
        with np.errstate(over="ignore"):
            sg = (F32(1) / (F32(1) + np.exp(-z))).astype(F32)
        cols.append(np.concatenate([xywh, sg]).astype(F32))
    return np.concatenate(cols, axis=1)


def _head_maps(rng, size=160):
    return [(rng.normal(0.0, 3.0, (size // s, size // s, 144))).astype(F16).astype(F32) for s in (8, 16, 32)]


@pytest.mark.parametrize("bug", [None, "anchor", "softmax16"])
def test_decode_bound(bug):
    maps = _head_maps(np.random.default_rng(3))
    ref, e = C.decode64(maps)
    got = decode_f32(maps, bug)
    ok = bool(np.all(np.abs(got - ref) <= e))
    old = bool(np.allclose(got, Y.decode(maps), rtol=2e-4, atol=2e-4))
    print(f"decode {bug or 'correct'}: float64 bound {'holds' if ok else 'VIOLATED'} (worst {float((np.abs(got - ref) / e).max()):.3f}); "
          f"old rtol 2e-4: {'passes' if old else 'caught'}")
    assert ok == (bug is None)
    if bug is None:
        C.check_decode(got, maps, "emulated")


def test_capture_hook_and_graph():
    """forward(inputs=...) captures each computed conv's input and residual; conv_graph's provenance matches their widths;
    NetCheck recomputes an unstored producer (the front end: 0 and 1 behind 2.cv1) in float64, and the oracle's own fp32
    emulated front end passes behind its two intermediates, the emulated Bottleneck from stored inputs."""
    rng = np.random.default_rng(11)
    w = {n: ((rng.normal(0.0, 1.0, (co, k, k, ci)) * np.sqrt(2.0 / (k * k * ci))).astype(F16).astype(F32), rng.normal(0.0, 0.1, co).astype(F32))
         for n, ci, co, k, s, a in Y.fused_convs("n")}
    x = (rng.integers(0, 256, (64, 64, 3)) / 255.0).astype(F16).astype(F32)
    taps, inputs = {}, {}
    plain = Y.forward(x, w, "n")
    outs = Y.forward(x, w, "n", taps=taps, inputs=inputs)
    assert all(np.array_equal(a, b) for a, b in zip(plain, outs))        # the hook changes nothing
    g = C.conv_graph("n")
    assert set(inputs) == set(g) == {n for n, *_ in Y.fused_convs("n")}
    for n, (xin, res) in inputs.items():
        segs, rsegs, _, _ = g[n]
        assert sum(c1 - c0 for _, c0, c1, _ in segs) == xin.shape[-1], n
        assert (rsegs is None) == (res is None), n
    # teacher-forced: the engine would have stored fp16; every stored output is the oracle's rounded to fp16 here
    stored = {n: taps[n].astype(F16).astype(F32) for n in taps if isinstance(n, str) and n not in ("0", "1")}
    t = x.astype(np.float64)
    for n, s in (("0", 2), ("1", 2), ("2.cv1", 1)):                        # the fused front end, emulated
        t = emulate(t, *w[n], s, 1)
    stored["2.cv1"] = t.astype(F32)
    c = t.shape[2] // 2
    stored["2.m.0.cv1"] = emulate(t[..., c:], *w["2.m.0.cv1"], 1, 1).astype(F32)
    stored["2.m.0.cv2"] = emulate(stored["2.m.0.cv1"].astype(np.float64), *w["2.m.0.cv2"], 1, 1, t[..., c:]).astype(F32)
    taps2, inputs2 = {}, {}
    Y.forward(x, w, "n", taps=taps2, force=stored, only={"0", "1", "2.cv1", "2.m.0.cv1", "2.m.0.cv2"}, inputs=inputs2)
    assert set(inputs2) == {"0", "1", "2.cv1", "2.m.0.cv1", "2.m.0.cv2"}
    res = C.check_layers(w, "n", inputs2, stored, names=["2.cv1", "2.m.0.cv1", "2.m.0.cv2"], what="n @ 64, emulated")
    assert res["2.cv1"][2] and not res["2.m.0.cv1"][2]
