"""Times Stabilizer.process (csrc/stab.hip) on 8 x 1080p BGR24 frames in device memory -- the frames tools/lens_time.py and
tools/render_time.py time their kernels on -- device to device: with supplied warps of a few pixels and a fraction of a degree, and
with the warps estimated by a CameraMotionEstimator from the same frames (the estimator's part separated by its own last_ms); beside
the call's byte floor -- source read once, destination written once, at the best copy rate of profiles/r01/bandwidth_probe.txt --
and, in the same run, LensCorrector.process with the identity lens and render_batch's kernel on the same frames.  Device times are
HIP-event times (rtmodt_stab_last_ms: the step and the warp launch together), medians after a warm-up.  Writes stab_time.json into
--out-dir and prints the JSON line.

    python tools/stab_time.py [--iters 200] [--out-dir profiles/stabilize]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import rtmodt_amd  # noqa: E402,F401
import gmc_ref  # noqa: E402
import render_time  # noqa: E402
import stab_ref  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402
from lens_time import timed  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
SHAKE = [(4, -4), (-8, 4), (4, 8), (0, -8)]                   # camera steps of the estimator leg, multiples of its downscale


def shake_warps(rng, calls):
    """Per call N warps: up to 3 px and 0.3 degrees, 0.2 % of zoom."""
    out = []
    for _ in range(calls):
        deg, s = np.radians(rng.uniform(-0.3, 0.3, N)), 1.0 + rng.uniform(-0.002, 0.002, N)
        a, b = s * np.cos(deg), s * np.sin(deg)
        out.append(np.stack([a, -b, rng.uniform(-3, 3, N), b, a, rng.uniform(-3, 3, N)], 1).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    F = pkg._ffi
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    src, dst = F.DeviceBuffer(frames.nbytes), F.DeviceBuffer(frames.nbytes)
    src.upload(frames)
    tbs, probe_line = hbm_rate()
    floor_bytes = 2 * frames.nbytes
    res = {"tool": "tools/stab_time.py", "streams": N, "size": f"{W}x{H}", "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs,
           "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "floor_bytes": floor_bytes, "floor_us": floor_bytes / (tbs * 1e12) * 1e6}

    # ---- supplied warps ----
    cfg = dict(leak_shift=6, max_shift_px=32)
    st, ref = pkg.ingestion.Stabilizer(N, (H, W), **cfg), stab_ref.Ref(N, (H, W), **cfg)
    warps = shake_warps(rng, a.warmup + a.iters)
    calls = iter(warps)
    row = timed(lambda: st.process(src, next(calls), out=dst), st.last_ms, a.warmup, a.iters)
    for w in warps:                                                           # the restatement follows stream 0 and samples its last frame
        ref.path[0], ref.hold[0], ref.status[0] = stab_ref.step(ref.rule, ref.path[0], ref.hold[0], w[0], True)
    want = stab_ref.sample(frames[0], stab_ref.quantise(ref.rule, ref.path[0]))
    r0 = st.result()[0]
    row["bit_exact"] = bool(r0.path == ref.path[0] and np.array_equal(dst.download(H * W * 3).reshape(H, W, 3), want))
    row["over_floor"] = row["ms"] * 1e3 / res["floor_us"]
    res["process"] = row
    identity = timed(lambda: (st.reset(), st.process(src, out=dst)), st.last_ms, a.warmup, a.iters)
    identity["bit_exact"] = bool(np.array_equal(dst.download(), frames.ravel()))
    identity["over_floor"] = identity["ms"] * 1e3 / res["floor_us"]
    res["process_identity"] = identity
    st.close()

    # ---- the estimator form: a textured scene under a camera that steps by SHAKE, the same scene on every stream ----
    margin = 16
    cv = gmc_ref.canvas(H + 2 * margin, W + 2 * margin, 3)
    pos, x, y = [], 0, 0
    for sx, sy in SHAKE:
        x, y = x + sx, y + sy
        pos.append((x, y))
    bufs = []
    for x, y in pos:
        f = gmc_ref.crop(cv, margin + x, margin + y, H, W)
        b = F.DeviceBuffer(frames.nbytes)
        b.upload(np.broadcast_to(f, (N, H, W, 3)).copy())
        bufs.append(b)
    est = pkg.tracking.gmc.CameraMotionEstimator(n_streams=N)
    st = pkg.ingestion.Stabilizer(N, (H, W), gmc=est, **cfg)
    k = [0]
    est_ms, statuses = [], []

    def call():
        st.process(bufs[k[0] % len(bufs)], out=dst)
        k[0] += 1
        est_ms.append(est.last_ms())

    row = timed(call, st.last_ms, a.warmup, a.iters)
    statuses = sorted({int(s) for s in est.result()[1]})
    row["estimator_ms"] = float(np.median(est_ms[a.warmup:]))
    row["estimator_status_last"] = statuses
    row["stab_status_last"] = sorted({r.status for r in st.result()})
    row["over_floor"] = row["ms"] * 1e3 / res["floor_us"]
    res["process_gmc"] = row
    st.close(); est.close()

    # ---- the yardsticks on the same frames ----
    lc = pkg.ingestion.LensCorrector(N, (H, W))
    for s in range(N):
        lc.set_model(s, (1100.0, 1100.0, (W - 1) / 2, (H - 1) / 2), (0.0, 0.0, 0.0, 0.0))
    lens = timed(lambda: lc.process(src, out=dst), lc.last_ms, a.warmup, a.iters)
    lens["floor_us"] = (floor_bytes + 8 * N * H * W) / (tbs * 1e12) * 1e6     # its floor carries the 8 B table entry per pixel
    lens["over_floor"] = lens["ms"] * 1e3 / lens["floor_us"]
    res["lens_identity"] = lens
    lc.close()
    r = pkg.FrameRenderer()
    lists = [render_time.scene(rng) for _ in range(N)]
    rk = []
    for i in range(a.warmup + a.iters):
        r.render_batch(src, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if i >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    res["process_over_lens"] = res["process"]["ms"] / lens["ms"]
    res["bit_exact"] = bool(res["process"]["bit_exact"] and identity["bit_exact"])
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "stab_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["bit_exact"] else 1


if __name__ == "__main__":
    sys.exit(main())
