"""Float64 restatement of the conv kernels' rounding contract, with a rigorous per-element error bound -- the check the GPU
tests hold every stored conv layer to, next to the ``2e-3 * max|ref|`` tolerance.

The contract (csrc/conv_dev.h ``store_tile`` / ``epilogue_lds``, every fused epilogue the same):

    out16 = RNE16( fp32( silu32(acc + b) ) + res16 )

with fp16 weights and inputs (products exact in fp32), fp32 bias and fp32 accumulation in any order.  Fused pairs (the front
end's stem and layer 1, a fused Bottleneck's ``m.j.cv1``, a 1x1 tail's producer, bneck32's two convs) round their LDS
intermediate to fp16 exactly once; those are recomputed here in float64 and rounded with RNE16.

For one conv fed exact fp16 ``x`` (and ``res``), :func:`conv64` returns ``y64`` (the float64 value before the final rounding)
and a bound ``e`` such that the fp32 value the kernel rounds lies in ``[y64 - e, y64 + e]``:

* accumulation: K products, the bias and the zero the accumulator starts from are K + 2 terms summed in some order, so
  ``|acc + b - fl(acc + b)| <= gamma(K + 1) * (sum|w||x| + |b|)``, ``gamma(n) = n u / (1 - n u)`` with ``u = 2^-23``
  (``sum|w||x|`` itself bounded from above by a float32 conv, see ``_conv_upper``):
  2^-23, not 2^-24, so the bound holds for round-to-nearest and for truncating accumulation (the MFMA f16 accumulate mode
  is not documented).  Whether the bias is added in the epilogue (store_tile) or preloaded into the accumulator is covered.
* an unstored fp16 intermediate ``t``: the kernel's t is RNE16 of a value in t's own bracket, so it lies in
  ``[RNE16(t64 - e_t), RNE16(t64 + e_t)]``; ``dev = max distance of that interval from RNE16(t64)`` (one ulp16 when the
  bracket spans two fp16 values, zero when it does not) adds ``sum|w| dev`` to the consumer's accumulation error.
* SiLU (csrc/common.h ``silu2``: ``t = x * k``, ``v_exp_f32``, ``1 + t``, ``v_rcp_f32``, ``x * d``), evaluated at the
  fp32 pre-activation z' in ``[z - ez, z + ez]``:
  - propagation: ``|silu(z') - silu(z)| <= L ez`` with L the maximum of ``|silu'|`` on the interval (silu' is monotone
    between its two extrema at +-2.3994, so L is read at the end points and at any extremum inside);
  - ``t = fl(z' k32)``, ``k32 = fp32(-log2 e)``: ``|t + z' log2 e| <= dt = |z'| log2 e ((1 + dk)(1 + 2^-24) - 1)``;
  - ``E = v_exp_f32(t) = e^-z' 2^dt' (1 + a)``, |a| <= 2^-23 (1 ulp, ISA): ``E = e^-z' (1 + eta)``,
    ``eta = 2^dt (1 + 2^-23) - 1``;
  - ``d = fl(1 + E) = (1 + e^-z')(1 + eta theta)(1 + 2^-24)``, ``theta = e^-z' / (1 + e^-z') <= 1 - sigmoid(z - ez)``;
  - ``r = v_rcp_f32(d)`` (1 ulp, 2^-23) and ``y = fl(z' r)`` (2^-24): relative error of y at most
    ``(1 + 2^-23)(1 + 2^-24) / ((1 - eta theta)(1 - 2^-24)) - 1``;
  - flushing of fp32 denormals anywhere in that sequence: at most ``4 * 2^-126`` absolute.
  Where ``2^-t`` overflows (z' < -88) the kernel returns ``z' * 0``; the true value is below 2^-120 there, covered by the
  absolute term.
* residual add: one fp32 rounding, ``2^-24 (|y| + e)``; an unstored residual adds its ``dev``.

The stored element must then lie in ``[RNE16(y64 - e), RNE16(y64 + e)]`` (``bracket_ok``: rigorous for any summation
order, it cannot be flaky) and ``exact_frac`` -- the share of elements equal to ``RNE16(y64)`` -- catches the systematic
errors that hide inside the bracket (an fp16 rounding of the accumulator before the bias, round-toward-zero stores, ...).

:func:`decode64` does the same for the Detect decode (csrc/postprocess.hip ``decode_row``) on the engine's own fp16 logits.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

U24 = 2.0 ** -24                     # fp32 round to nearest
U23 = 2.0 ** -23                     # fp32 truncation / 1 ulp transcendental
TINY = 4 * 2.0 ** -126               # fp32 denormal flushes
LOG2E = 1.4426950408889634
K32 = float(np.float32(-LOG2E))
DK = abs(K32 + LOG2E) / LOG2E        # relative error of the fp32 constant in silu2
# floors of exact_frac (tests/test_conv_ref64_cpu.py measures them on the CPU emulator of the contract)
FLOOR_STORED = 0.98                  # every input a stored fp16 tensor
# behind an unstored fp16 intermediate.  Emulator (test_conv_ref64_cpu.py, and the fused Bottleneck pairs of the synthetic
# n @ 320 / s @ 288 nets at c = 16 .. 256): 0.983 - 0.999.  On the MI355X the lowest seen is 0.970 (n @ 320, 21.m.0.cv2,
# a 10 x 10 map), every element inside its bracket and every stored layer at the emulator's 0.998 - 0.9995; 0.95 sits
# below both and far above the mutations (bias after an fp16 rounding: 0.80, the highest of them).
FLOOR_BEHIND = 0.95


def rne16(a):
    """float64 -> nearest fp16 (ties to even), returned as float64 (NumPy's double -> half conversion is correctly rounded)."""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def _rne16_t(v):
    """rne16 on a float64 torch tensor, multi-threaded: the fp16 grid's quantum at |v| is 2^(max(floor(log2|v|), -14) - 10);
    v / quantum is exact, torch.round rounds half to even, and anything that rounds above 65504 is inf.  (Not
    ``.to(torch.float16)``: torch converts double -> float -> half, a double rounding.)"""
    _, ex = torch.frexp(v)
    q = torch.ldexp(torch.ones_like(v), torch.clamp(ex - 1, min=-14) - 10)
    r = torch.round(v / q) * q
    return torch.where(r.abs() > 65504.0, torch.copysign(torch.full_like(v, math.inf), v), r)


def _ulp16_t(t16):
    """Spacing of the fp16 grid above |t16| (np.spacing on float16)."""
    _, ex = torch.frexp(t16.abs())
    ex = torch.where(t16 == 0, torch.full_like(ex, -13), ex)           # (frexp(0) has exponent 0; 0 sits on the subnormal grid)
    return torch.ldexp(torch.ones_like(t16), torch.clamp(ex - 1, min=-14) - 10)


def gamma(n, u=U23):
    return n * u / (1.0 - n * u)


def _silu_crit():
    """x > 0 where silu'' = 0 (silu' has its maximum there, its minimum at -x)."""
    x = 2.4
    for _ in range(60):                   # 2 + x (1 - 2 s) = 0, Newton
        s = 1.0 / (1.0 + math.exp(-x))
        f = 2.0 + x * (1.0 - 2.0 * s)
        df = (1.0 - 2.0 * s) - 2.0 * x * s * (1.0 - s)
        x -= f / df
    return x


XC = _silu_crit()


def dsilu(x):
    """silu' (NumPy or torch float64)."""
    if isinstance(x, torch.Tensor):
        sg = torch.sigmoid(x)
    else:
        sg = 1.0 / (1.0 + np.exp(-np.clip(x, -700, 700)))
    return sg * (1.0 + x * (1.0 - sg))


SILU_MAX = float(dsilu(np.float64(XC)) * (1 + 1e-12))     # 1.0998...
SILU_MIN = float(dsilu(np.float64(-XC)))                  # -0.0998...


def silu_bound(z, ez):
    """(silu(z), bound on |kernel silu2(z') - silu(z)| for any fp32 z' within ez of z); float64 torch tensors."""
    lo, hi = z - ez, z + ez
    L = torch.maximum(dsilu(lo).abs(), dsilu(hi).abs())
    L = torch.where((lo <= XC) & (hi >= XC), torch.full_like(L, SILU_MAX), L)
    L = torch.where((lo <= -XC) & (hi >= -XC), torch.clamp(L, min=abs(SILU_MIN)), L)
    s = z * torch.sigmoid(z)
    dt = (z.abs() + ez) * (LOG2E * ((1 + DK) * (1 + U24) - 1))
    eta = torch.exp2(torch.clamp(dt, max=1.0)) * (1 + U23) - 1
    theta = torch.sigmoid(-lo)                             # e^-z' / (1 + e^-z') <= its value at z - ez
    rel = (1 + U23) * (1 + U24) / ((1 - eta * theta) * (1 - U24)) - 1
    Lez = L * ez
    e = Lez + rel * (s.abs() + Lez) + TINY
    big = -lo > 80.0                                      # 2^-t may overflow: kernel gives z' * 0, the truth is below 2^-100
    return s, torch.where(big, s.abs() + Lez + TINY, e)


def _nchw(x):
    """(H,W,C) float64 array -> a (1,C,H,W) view (channels-last memory, no copy)."""
    return torch.from_numpy(np.asarray(x, np.float64)).permute(2, 0, 1)[None]


def _conv(x, w, stride):
    """x (1,C,H,W) float64, w (cout,k,k,cin) -> (Ho,Wo,cout) float64 torch tensor, zero padding k//2."""
    k = w.shape[1]
    wt = torch.from_numpy(np.asarray(w, np.float64)).permute(0, 3, 1, 2)
    return Fn.conv2d(x, wt, stride=stride, padding=k // 2)[0].permute(1, 2, 0)


def _up32(a):
    """float64 tensor >= 0 -> the smallest float32 not below it."""
    a32 = a.float()
    return torch.where(a32.double() < a, torch.nextafter(a32, torch.tensor(math.inf)), a32)


def _conv_upper(x, w, stride):
    """An upper bound on the conv of nonnegative x (1,C,H,W) and w (cout,k,k,cin), from a float32 conv (50x faster than
    float64 on the CPU): inputs rounded up to float32, products of fp16 weights exact, and a sum of K nonnegative terms in
    any order is at most gamma(K, 2^-24) below the truth, so dividing by 1 - gamma(K, 2^-24) bounds it from above."""
    k = w.shape[1]
    K = k * k * w.shape[3]
    wt = _up32(torch.from_numpy(np.asarray(w, np.float64)).permute(0, 3, 1, 2))
    y = Fn.conv2d(_up32(x), wt, stride=stride, padding=k // 2)[0].permute(1, 2, 0).double()
    return y / (1.0 - gamma(K, U24))


class Conv64:
    """One conv's float64 value and bound.  ``t16`` / ``dev``: its fp16 output as a downstream input (RNE16(y64)) and how
    far the kernel's fp16 value may sit from it."""

    def __init__(self, x, w, b, stride=1, act=1, res=None, dx=None, dres=None):
        xt = _nchw(x)
        w = np.asarray(w, np.float64)
        bt = torch.from_numpy(np.asarray(b, np.float64))
        K = w.shape[1] * w.shape[2] * w.shape[3]
        flip = dx is not None and bool(np.any(dx))
        ax = xt.abs() + _nchw(dx) if flip else xt.abs()
        z = _conv(xt, w, stride) + bt
        ez = gamma(K + 1) * (_conv_upper(ax, np.abs(w), stride) + bt.abs())
        if flip:
            ez = ez + _conv_upper(_nchw(dx), np.abs(w), stride)
        y, e = silu_bound(z, ez) if act else (z, ez)
        if res is not None:
            if dres is not None:
                e = e + torch.from_numpy(np.asarray(dres, np.float64))
            y = y + torch.from_numpy(np.asarray(res, np.float64))
            e = e + U24 * (y.abs() + e)
        lo16, hi16, t16 = _rne16_t(y - e), _rne16_t(y + e), _rne16_t(y)
        self._t = (y, e, lo16, hi16, t16)
        self.y64, self.e, self.K = y.numpy(), e.numpy(), K
        self.lo16, self.hi16, self.t16 = lo16.numpy(), hi16.numpy(), t16.numpy()
        self.dev = torch.maximum(hi16 - t16, t16 - lo16).numpy()
        self.behind = flip or (dres is not None and bool(np.any(dres)))

    def check(self, got):
        """(bracket_ok, exact_frac, worst) for the stored tensor ``got`` (fp16 values, any float dtype).  ``worst``: the
        element with the largest bracket ratio -- its distance from RNE16(y64) over the distance of the bracket's end on
        that side (0 when exactly rounded, <= 1 inside the bracket)."""
        y, e, lo16, hi16, t16 = self._t
        g = torch.from_numpy(np.ascontiguousarray(np.asarray(got, np.float64)))
        assert g.shape == y.shape, (tuple(g.shape), tuple(y.shape))
        ok = (g >= lo16) & (g <= hi16)
        same = g == t16
        exact = float(same.double().mean())
        end = torch.where(g >= t16, hi16, lo16)
        ratio = torch.nan_to_num((g - t16).abs() / (end - t16).abs(), nan=0.0, posinf=1.0)
        ratio = torch.where(same, torch.zeros_like(ratio), ratio)
        ratio = torch.where(ok, ratio, torch.full_like(ratio, 1e300))
        i = np.unravel_index(int(torch.argmax(ratio)), tuple(g.shape))
        worst = {"pixel": tuple(int(v) for v in i[:-1]), "channel": int(i[-1]), "got": float(g[i]), "y64": float(y[i]),
                 "e": float(e[i]), "ratio": float(ratio[i]) if bool(ok[i]) else math.inf,
                 "ulp16": float((g[i] - t16[i]).abs() / _ulp16_t(t16[i]))}
        return bool(ok.all()), exact, worst


def conv64(x, w, b, stride=1, act=1, res=None, dx=None, dres=None):
    return Conv64(x, w, b, stride, act, res, dx, dres)


# ---------------------------------------------------------------------------------------------------------------- the network
def conv_graph(scale="s", nc=80, reg_max=16):
    """For every fused conv: (input segments, residual segments or None, stride, act).  A segment (producer, c0, c1, how)
    is channels [c0, c1) of conv ``producer``'s output ("input": the image), ``how`` None or "up" / "pool" when an
    Upsample / MaxPool lies between -- the order of forward() in oracle/yolo_oracle.py."""
    from oracle import yolo_oracle as Y
    mods, head = Y.arch(scale, nc, reg_max)
    fc = {n: (co, s, a) for n, ci, co, k, s, a in Y.fused_convs(scale, nc, reg_max)}
    g = {}

    def cv(name, src, res=None):
        g[name] = (src, res, fc[name][1], fc[name][2])
        return [(name, 0, fc[name][0], None)]

    def width(t):
        return sum(c1 - c0 for _, c0, c1, _ in t)

    def sl(t, a, bnd):
        out, off = [], 0
        for p, c0, c1, how in t:
            lo, hi = max(a, off), min(bnd, off + c1 - c0)
            if lo < hi:
                out.append((p, c0 + lo - off, c0 + hi - off, how))
            off += c1 - c0
        return out

    def via(t, how):
        return [(p, c0, c1, how) for p, c0, c1, _ in t]

    saved = {}
    cur = [("input", 0, 3, None)]
    for i, m in enumerate(mods):
        kind = m[0]
        if kind == "conv":
            cur = cv(f"{i}", cur)
        elif kind == "c2f":
            n, shortcut = m[4], m[5]
            y = cv(f"{i}.cv1", cur)
            c = width(y) // 2
            ys = [sl(y, 0, c), sl(y, c, 2 * c)]
            for j in range(n):
                t = cv(f"{i}.m.{j}.cv1", ys[-1])
                ys.append(cv(f"{i}.m.{j}.cv2", t, res=ys[-1] if shortcut else None))
            cur = cv(f"{i}.cv2", [s for y_ in ys for s in y_])
        elif kind == "sppf":
            y = cv(f"{i}.cv1", cur)
            cur = cv(f"{i}.cv2", y + via(y, "pool") * 3)
        elif kind == "up":
            cur = via(cur, "up")
        elif kind == "cat":
            a, bidx = m[1]
            cur = (cur if a == -1 else saved[a]) + saved[bidx]
        saved[i] = cur
    for lvl, src in enumerate((15, 18, 21)):
        for br in ("cv2", "cv3"):
            t = cv(f"22.{br}.{lvl}.0", saved[src])
            t = cv(f"22.{br}.{lvl}.1", t)
            cv(f"22.{br}.{lvl}.2", t)
    return g


class NetCheck:
    """Every conv of one image, from the inputs ``Y.forward(..., inputs=...)`` captured and the set of convs whose outputs
    the engine stored (and the oracle was forced with).  A conv fed by an unstored producer recomputes that producer in
    float64 from its own captured input (recursively: the front end's stem -> 1 -> 2.cv1)."""

    def __init__(self, weights, scale, inputs, stored, nc=80):
        self.w, self.inputs, self.stored = weights, inputs, set(stored)
        self.g = conv_graph(scale, nc)
        self.cache = {}

    def _operand(self, segs, captured):
        x = np.asarray(captured, np.float64)
        dx = np.zeros_like(x)
        off = 0
        for p, c0, c1, how in segs:
            wdt = c1 - c0
            if p != "input" and p not in self.stored:
                assert how is None, f"conv {p} feeds through {how} but was not stored: cannot be recomputed here"
                r = self.conv(p)
                x[..., off:off + wdt] = r.t16[..., c0:c1]
                dx[..., off:off + wdt] = r.dev[..., c0:c1]
            off += wdt
        assert off == x.shape[-1], (off, x.shape)
        xt = torch.from_numpy(x)
        assert bool(((xt == _rne16_t(xt)) | torch.from_numpy(dx != 0)).all()), "a conv input that should hold the engine's fp16 values does not"
        return x, (dx if np.any(dx) else None)

    def conv(self, name):
        if name not in self.cache:
            assert name in self.inputs, f"conv {name}: its input was not captured (not computed by this forward)"
            segs, rsegs, stride, act = self.g[name]
            xc, rc = self.inputs[name]
            x, dx = self._operand(segs, xc)
            r = dr = None
            if rsegs is not None:
                r, dr = self._operand(rsegs, rc)
            w, b = self.w[name]
            self.cache[name] = Conv64(x, w, b, stride, act, r, dx, dr)
        return self.cache[name]


def check_layers(weights, scale, inputs, gpu, names=None, stored=None, what="", nc=80, verbose=False):
    """Applies the float64 check to every conv in ``names`` (default: every stored conv the forward computed): bracket on
    every element, exact_frac >= FLOOR_STORED (FLOOR_BEHIND behind an unstored intermediate).  Returns
    ``{name: (exact_frac, worst)}``; prints one line per layer with ``verbose`` and the lowest fraction always."""
    net = NetCheck(weights, scale, inputs, gpu.keys() if stored is None else stored, nc)
    names = [n for n in gpu if n in inputs] if names is None else list(names)
    out = {}
    for n in names:
        r = net.conv(n)
        ok, frac, worst = r.check(gpu[n])
        floor = FLOOR_BEHIND if r.behind else FLOOR_STORED
        out[n] = (frac, worst, r.behind)
        if verbose:
            print(f"  {what} {n}: K={r.K} exact {frac:.4f}{' (behind fp16 intermediate)' if r.behind else ''}, worst element {worst['ratio']:.3f} "
                  f"of its bracket at pixel {worst['pixel']}, channel {worst['channel']}: got {worst['got']!r}, y64 {worst['y64']!r}, "
                  f"e {worst['e']:.3g}, {worst['ulp16']:.0f} ulp16")
        assert ok, f"{what} layer {n}: element outside its float64 bracket: {worst}"
        assert frac >= floor, f"{what} layer {n}: exact_frac {frac:.4f} < {floor} (worst {worst})"
    if out:
        lo = min(out, key=lambda k: out[k][0])
        hi = max(out, key=lambda k: out[k][1]["ratio"])
        wv = out[hi][1]
        print(f"{what}: {len(out)} layers in their float64 brackets; lowest exact_frac {out[lo][0]:.4f} ({lo}); worst element "
              f"{wv['ratio']:.3f} of its bracket: layer {hi}, pixel {wv['pixel']}, channel {wv['channel']}, got {wv['got']!r}, "
              f"y64 {wv['y64']!r}, e {wv['e']:.3g}, {wv['ulp16']:.0f} ulp16")
    return out


# ---------------------------------------------------------------------------------------------------------------- decode
def decode64(head_maps, nc=80, reg_max=16, strides=(8, 16, 32)):
    """Float64 decode of fp16 logits and a bound on csrc/postprocess.hip ``decode_row``'s fp32 result, per element of
    ``pred[(4 + nc), A]``.  The kernel: ``d_k = fl(v_k - max)`` (one rounding), ``e_k = expf(d_k)`` (1 ulp), a serial fp32
    sum of 16, ``q_k = e_k / sum`` (1 ulp allowed), ``dist = serial sum of fl(q_k k)``; then ``x1 = fl(ax - dl)`` ...,
    ``cx = fl(x1 + x2) / 2 * stride`` (exact scalings), ``bw = fl(x2 - x1) * stride``; classes ``1 / (1 + expf(-x))``.
    Per term: ``q_k k`` carries relative error R_k = (1 + A_k)(1 + u_div)(1 + u)(1 + g15) / (1 - S) - 1 with
    ``A_k = e^(u |d_k|)(1 + u_e) - 1`` and S = max_k (1 + A_k)(1 + g15) - 1 the sum's; ``|dist' - dist| <= sum p_k k R_k``."""
    g15 = gamma(15, U24)
    cols, errs = [], []
    proj = np.arange(reg_max, dtype=np.float64)
    for m, s in zip(head_maps, strides):
        h, w, _ = m.shape
        m = np.asarray(m, np.float64)
        box = m[..., :4 * reg_max].reshape(h * w, 4, reg_max)
        d = box - box.max(axis=2, keepdims=True)
        e = np.exp(d)
        p = e / e.sum(axis=2, keepdims=True)
        dist = (p * proj).sum(axis=2)
        A = np.exp(U24 * np.abs(d)) * (1 + U23) - 1
        S = ((1 + A) * (1 + g15)).max(axis=2, keepdims=True) - 1
        R = (1 + A) * (1 + U23) * (1 + U24) * (1 + g15) / (1 - S) - 1
        ed = (p * proj * R).sum(axis=2)
        yy, xx = np.mgrid[0:h, 0:w]
        ax, ay = xx.reshape(-1) + 0.5, yy.reshape(-1) + 0.5

        def sub(a, ea, b, eb):
            v = a - b
            return v, ea + eb + U24 * (np.abs(v) + ea + eb)

        def add(a, ea, b, eb):
            v = a + b
            return v, ea + eb + U24 * (np.abs(v) + ea + eb)

        x1, ex1 = sub(ax, 0.0, dist[:, 0], ed[:, 0])
        y1, ey1 = sub(ay, 0.0, dist[:, 1], ed[:, 1])
        x2, ex2 = add(ax, 0.0, dist[:, 2], ed[:, 2])
        y2, ey2 = add(ay, 0.0, dist[:, 3], ed[:, 3])
        cx, ecx = add(x1, ex1, x2, ex2)
        cy, ecy = add(y1, ey1, y2, ey2)
        bw, ebw = sub(x2, ex2, x1, ex1)
        bh, ebh = sub(y2, ey2, y1, ey1)
        xywh = np.stack([cx / 2, cy / 2, bw, bh]) * s
        exywh = np.stack([ecx / 2, ecy / 2, ebw, ebh]) * s
        z = m[..., 4 * reg_max:4 * reg_max + nc].reshape(h * w, nc).T
        sg = 1.0 / (1.0 + np.exp(-z))
        esg = ((1 + U23) / ((1 - U23) * (1 - U24)) - 1) * sg + TINY
        cols.append(np.concatenate([xywh, sg]))
        errs.append(np.concatenate([exywh, esg]))
    return np.concatenate(cols, axis=1), np.concatenate(errs, axis=1)


def check_decode(pred, head_maps, what="", nc=80):
    """Every element of the engine's pre-NMS tensor within its decode64 bound of the float64 decode of the same logits."""
    ref, e = decode64(head_maps, nc)
    g = np.asarray(pred, np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    ratio = np.abs(g - ref) / e
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what} decode: worst element {ratio[i]:.3f} of its bound (row {i[0]}, anchor {i[1]}: got {g[i]!r}, f64 {ref[i]!r}, e {e[i]:.3g})")
    assert ratio[i] <= 1.0, f"{what} decode: pred[{i}] = {g[i]!r}, float64 {ref[i]!r}, bound {e[i]:.3g}"
    return float(ratio[i])
