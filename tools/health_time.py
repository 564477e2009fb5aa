"""Times CameraHealth.process (csrc/health.hip) on 8 x 1080p BGR24 frames in device memory -- the frames tools/render_time.py times
the renderer on -- at scale 4, 2 and 1, beside each call's floor -- the bytes it must move, each once, at the best copy rate of
profiles/r01/bandwidth_probe.txt -- and, in the same run, MotionDetector.process on the same still scene at the same scale and
render_batch's kernel on the same frames.  Device times are HIP-event times around the launches of one call (rtmodt_health_last_ms:
the memset and all four launches together), medians after a warm-up.  Nothing is gated on these numbers.  Writes health_time.json
and README.md into --out-dir (a health_time_run1.json found there is quoted as the first of two runs) and prints the JSON line.

    python tools/health_time.py [--iters 30] [--out-dir profiles/health]
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
import health_ref  # noqa: E402
import render_time  # noqa: E402
from heatmap_time import hbm_rate  # noqa: E402
from motion_time import timed  # noqa: E402

pkg = sys.modules["rtmodt_amd"]
N, H, W = render_time.N, render_time.H, render_time.W
SCALES = (4, 2, 1)
#: bytes per cell besides the pixels: health_pixels reads and writes Y (2), health_edges reads Y and R and writes G (1 + 2 + 1),
#: health_learn reads G and R and writes R (1 + 2 + 2)
CELL_BYTES = 11

README = """# Camera health: timings (`tools/health_time.py`)

What is measured: one `CameraHealth.process` call on {n} streams of 1080p, BGR24 frames already in device memory ({frames_mb:.1f} MB:
the frames `tools/render_time.py` times the renderer on), at scale 4 ({cells4:.2f} M cells per stream), 2 ({cells2:.2f} M) and 1
({cells1:.2f} M), with the default configuration, on the same frames call after call.  Beside it, in the same process,
`MotionDetector.process` on the same still scene at the same scale and `render_batch`'s kernel on the same frames.  Everything below
comes from ONE process on one MI355X.

How: device times are HIP-event times around the memset and all four launches of one call together (`rtmodt_health_last_ms`;
`rtmodt_motion_last_ms` for the motion detector's memset and seven launches), medians of {iters} calls after {warmup} warm-up calls
(the motion detector after its own warm-up frames besides).  No profiler was attached, nothing was fixed in advance and nothing is
gated on these numbers.

    python tools/health_time.py --out-dir profiles/health

## Figures (`health_time.json`)

| scale | health call | floor | x floor | motion call, still scene | health / motion |
|---|---|---|---|---|---|
{rows}

A floor is the bytes the call must move, each once, at the {hbm:.2f} TB/s of the best `copy` line of
`profiles/r01/bandwidth_probe.txt` ({probe_line}): {frames_mb:.1f} MB of pixels plus {cell_bytes} B per cell (Y read and written by the
pixel pass; Y and R read and G written by the edge pass; G and R read and R written by the learn pass).  It leaves out the halo
cells a tile of the edge pass reads twice and the three bytes a row that lane 63 of a wave reads again for the fine-detail term.

`render_batch`'s kernel on the same frames: {render_ms:.3f} ms.

{verdict}

{spread}

## Parity

PINNED, exactly: the kernels against `tests/health_ref.py` (stream 0's result and state after the first two calls were compared again
in this run at every scale: {exact}).  UNPINNED: parity with any camera's or NVR's tamper detection, and every default: none has been
validated on real footage.  The guess that this call costs about what a still-scene motion call costs was a guess; the ratio above
is what was measured.  Which launch bounds each figure was not profiled: no kernel trace was taken.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lists = [render_time.scene(rng) for _ in range(N)]
    still = pkg._ffi.DeviceBuffer(frames.nbytes)
    still.upload(frames)
    tbs, probe_line = hbm_rate()
    res = {"tool": "tools/health_time.py", "streams": N, "size": f"{W}x{H}", "iters": a.iters, "warmup": a.warmup, "hbm_tbs": tbs,
           "hbm_source": f"profiles/r01/bandwidth_probe.txt: {probe_line}", "cell_bytes": CELL_BYTES, "scales": {}}
    exact = True
    for scale in SCALES:
        gh, gw = -(-H // scale), -(-W // scale)
        mon = pkg.ingestion.CameraHealth(N, H, W, scale=scale)
        ref = health_ref.Ref(1, H, W, scale=scale)
        ok = True
        for _ in range(2):                                          # the first two calls against the restatement: set, then average and n_changed 0
            g, want = mon.process(still)[0], ref.step(0, frames[0])
            ok = ok and all(getattr(g, k) == want[k] for k in health_ref.COUNTS + ("raw", "active", "frames_seen", "ref_sharp", "learned"))
            st, rs = mon.state(0), ref.state(0)
            ok = ok and bool(np.array_equal(st.r, rs["r"])) and bool(np.array_equal(st.prev, rs["prev"])) and (st.run, st.off) == (rs["run"], rs["off"])
        row = {"grid": f"{gw}x{gh}", "cells_per_stream": gh * gw, "floor_bytes": frames.nbytes + CELL_BYTES * N * gh * gw, "bit_exact": bool(ok)}
        exact &= bool(ok)
        row["floor_us"] = row["floor_bytes"] / (tbs * 1e12) * 1e6
        row["health"] = timed(lambda k: mon.process(still), mon.last_kernel_ms, a.warmup, a.iters)
        row["health"]["over_floor"] = row["health"]["ms"] * 1e3 / row["floor_us"]
        row["last_call"] = {"active": sorted({n_ for r in mon.process(still) for n_ in r.names})}
        mon.close()
        det = pkg.MotionDetector(N, H, W, scale=scale)
        for _ in range(det._cfg.warmup):
            det.process(still)
        row["motion_still"] = timed(lambda k: det.process(still), det.last_kernel_ms, a.warmup, a.iters)
        row["health_over_motion"] = row["health"]["ms"] / row["motion_still"]["ms"]
        det.close()
        res["scales"][str(scale)] = row
    r = pkg.FrameRenderer()
    rk = []
    for k in range(a.warmup + a.iters):
        r.render_batch(still, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if k >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    res["bit_exact"] = exact
    still.free()

    rows = []
    for scale in SCALES:
        row = res["scales"][str(scale)]
        rows.append(f"| {scale} | {row['health']['ms']:.3f} ms | {row['floor_us']:.1f} us | {row['health']['over_floor']:.1f} x | "
                    f"{row['motion_still']['ms']:.3f} ms | {row['health_over_motion']:.2f} x |")
    s4 = res["scales"]["4"]
    res["verdict"] = (f"At the default scale 4 the health call takes {s4['health']['ms']:.3f} ms for {N} streams, {s4['health_over_motion']:.2f} x the motion "
                      f"detector's still-scene call and {s4['health']['ms'] / res['render_kernel_ms']:.2f} x the render kernel's time; it is "
                      f"{s4['health']['over_floor']:.1f} x its byte floor.  The frames never change here (a stream would be FROZEN after freeze_frames such "
                      f"calls); the launches do the same work whatever the frames show.  Reported as measured, not tuned.")
    print(json.dumps(res))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        prev_path = os.path.join(a.out_dir, "health_time_run1.json")
        spread = "Only one run was made."
        if os.path.exists(prev_path):
            prev = json.load(open(prev_path))
            parts = [f"scale {s}: health {prev['scales'][str(s)]['health']['ms']:.3f} ms, motion still {prev['scales'][str(s)]['motion_still']['ms']:.3f} ms "
                     f"(this run: {res['scales'][str(s)]['health']['ms']:.3f} / {res['scales'][str(s)]['motion_still']['ms']:.3f})" for s in SCALES]
            spread = ("The same command was run twice on this code, one run after the other; the figures above are the second run, "
                      "`health_time_run1.json` the first: " + "; ".join(parts) + f"; render kernel {prev['render_kernel_ms']:.3f} ms "
                      f"(this run {res['render_kernel_ms']:.3f}).  Within a run the extremes of each figure are in `minmax_ms`.")
        with open(os.path.join(a.out_dir, "health_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        sc = res["scales"]
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(n=N, frames_mb=frames.nbytes / 1e6, cells1=sc["1"]["cells_per_stream"] / 1e6, cells2=sc["2"]["cells_per_stream"] / 1e6,
                                  cells4=sc["4"]["cells_per_stream"] / 1e6, iters=a.iters, warmup=a.warmup, rows="\n".join(rows), hbm=tbs,
                                  probe_line=probe_line, cell_bytes=CELL_BYTES, render_ms=res["render_kernel_ms"], verdict=res["verdict"], spread=spread,
                                  exact="equal" if exact else "NOT EQUAL"))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
