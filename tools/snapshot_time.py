"""Times the snapshot gallery (csrc/snapshot.hip: snapshot_decide + snapshot_resample) on 8 x 1080p device frames with 200 tracks
per stream, straight on the device-resident state of one ByteTrack handle, beside render_batch's kernel on the same frames in the
same run.  Nothing is asserted: the numbers are reported, not gated.

  first call     every track takes its shot: 1600 crops are resampled (the ledgers are reset before each repetition);
  steady state   the boxes drift and the confidence of a rotating few per cent of the tracks rises, so that those are rewritten;
  kept only      no track improves: the decision runs and the resampler finds an empty work list -- the steady state's configuration
                 and outputs, once with the boxes as they are and once with boxes of nine times the area, to check that the cost of a
                 call does not grow with the crop area of tracks whose thumbnail is kept; and once more with no output asked for.

Device times are HIP events around the two launches (rtmodt_snapshot_last_ms), medians after a warm-up; the raw series of the first
two runs are kept in the JSON.  The floor is the bytes of the rewritten crops read once plus their slots written once, over the
measured copy bandwidth of the chip.  Writes snapshot_time.json and README.md into --out-dir and prints the JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
from importlib import import_module
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import render_time  # noqa: E402

S, H, W, N_TRACKS, THUMB = 8, 1080, 1920, 200, (96, 96)
HBM_COPY_BYTES_PER_S = 6.29e12            # measured float4 copy on the MI355X (8.0e12 on the datasheet)

README = """# Snapshot gallery: device time of a call

`tools/snapshot_time.py`, {S} x {W}x{H} BGR24 device frames, {n} tracks per stream on one ByteTrack handle (boxes of {bw}x{bh} px on a
grid, drifting), thumbnails of {tw}x{th}, margin 100 per mille.  HIP events around the two launches of a call
(`snapshot_decide`, `snapshot_resample`), medians of the calls after {warmup} warm-up calls; `render_batch`'s kernel is timed the
same way on the same frames in the same run.  Raw series: `snapshot_time.json` (`first_call_ms_raw`, `steady_ms_raw`).

| run | thumbnails written per call | device time | / render kernel | / floor |
|---|---|---|---|---|
| first call (every track takes its shot) | {first_n:.0f} | {first_ms:.3f} ms | {first_over_render:.2f} x | {first_over_floor:.1f} x |
| steady state ({steady_share:.1%} rewritten; the {steady_calls} calls of the run that rewrote something) | {steady_n:.1f} | {steady_ms:.3f} ms | {steady_over_render:.2f} x | {steady_over_floor:.1f} x |
| ... the {tail_calls} calls at the end of that run that rewrote nothing | 0 | {tail_ms:.3f} ms | - | - |
| kept only, boxes as above | {kept_small_n} | {kept_small_ms:.3f} ms | {kept_small_over_render:.2f} x | - |
| kept only, boxes of 9 x the area | {kept_large_n} | {kept_large_ms:.3f} ms | {kept_large_over_render:.2f} x | - |
| kept only, boxes as above, no output asked for | 0 | {kept_quiet_ms:.3f} ms | {kept_quiet_over_render:.2f} x | - |

Every row but the last is the default configuration (occlusion test on) with the outputs fetched; the device time is the two
launches, not the copy of the results.  The kept-only rows are runs of their own on a fresh tracker and a fresh gallery in which no
confidence ever rises; the last one passes a null output struct, so the call neither copies nor waits.

`render_batch`'s kernel on the same frames ({n} tracks per frame, trails and zones as `tools/render_time.py`): {render_ms:.3f} ms.
The floor -- the rewritten crops read once and their slots written once, {first_floor_mb:.2f} MB for the first call and
{steady_floor_kb:.1f} kB for a steady-state call, at the {bw_tb:.2f} TB/s a float4 copy reaches on this chip -- is
{first_floor_us:.2f} us and {steady_floor_us:.3f} us.  Both runs are far from it: the first call moves its bytes at a small fraction of the
copy bandwidth, and a steady-state call is two launches around a few dozen thumbnails.  What bounds the resampler (the two barriers
per staged tile, the 64-bit division per value, its occupancy) was not profiled; reported as measured, not tuned.

The structural expectation holds or fails on the two kept-only rows with outputs: a call in which every thumbnail is kept costs
{kept_small_ms:.3f} ms with the boxes as they are and {kept_large_ms:.3f} ms with boxes of nine times the area ({kept_ratio:.2f} x), under the configuration
the steady state uses.  (Larger boxes overlap more, so more of the occlusion sweep's early exits are taken; the sweep itself is
quadratic in the sampled tracks of a stream, whatever their size.)

Not profiled: no kernel trace and no counters were collected (the split between the two kernels, LDS conflicts of the staged tile,
occupancy of the resampler at 184 VGPRs), no host-side cost of the call, host frames, the other three trackers, thumbnails other
than {tw}x{th}, and no real footage -- the share of rewritten tracks is the tool's own choice.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--first", type=int, default=12)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    import rtmodt_amd as pkg
    F = pkg._ffi
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8)
    dev = F.DeviceBuffer(frames.nbytes)
    dev.upload(frames)
    new_core = lambda: import_module(pkg.__name__ + ".tracking.tracker")._ByteTrackCore(n_streams=S, max_tracks=256, max_dets=256)
    bt = new_core()
    bw, bh = 60, 120
    base = np.asarray([[(k % 20) * 90 + 10, (k // 20) * 100 + 10] for k in range(N_TRACKS)], np.float32)
    cls = np.zeros((S, 256), np.int32)
    cnt = np.full(S, N_TRACKS, np.int32)
    fid = [0]

    def update(bt, t, conf_of, scale=1):
        phase = t % 60
        dx = 2 * (phase if phase < 30 else 60 - phase)
        xy = np.zeros((S, 256, 4), np.float32)
        conf = np.zeros((S, 256), np.float32)
        c = conf_of(t)
        for s in range(S):
            xy[s, :N_TRACKS, 0] = base[:, 0] + dx + s; xy[s, :N_TRACKS, 1] = base[:, 1]
            xy[s, :N_TRACKS, 2] = xy[s, :N_TRACKS, 0] + bw * scale; xy[s, :N_TRACKS, 3] = xy[s, :N_TRACKS, 1] + bh * scale
            conf[s, :N_TRACKS] = c
        bt.update_batch(xy, conf, cls, cnt)

    def call(g, bt, want=True):
        fid[0] += 1
        if want:
            g.process_tracker(SimpleNamespace(_core=bt, report="matched"), dev, fid[0], height=H, width=W)
        else:                                            # no outputs: nothing crosses to the host
            fids = np.full(S, fid[0], np.int64)
            fp = (C.c_void_p * S)(*[dev.ptr + i * H * W * 3 for i in range(S)])
            F.check(F.lib().rtmodt_snapshot_process_tracker(g._h, bt._h, fp, H, W, 3 * W, F.MEM_DEVICE, F.ptr(fids), 1, None))
        return g.last_kernel_ms()

    def floor_bytes(g, bt):
        total = 0
        plan = F.SnapshotPlan()
        snaps = {}
        for u in g.updated:
            st = snaps.setdefault(u.stream, bt.snapshot(u.stream))
            xy = np.ascontiguousarray(st["xyxy"][u.track], np.float32)
            F.check(F.lib().rtmodt_snapshot_plan(C.byref(g.cfg), F.ptr(xy), H, W, C.byref(plan)))
            total += 3 * plan.sw * plan.sh + THUMB[0] * ((3 * THUMB[1] + 15) // 16 * 16)
        return total

    g = pkg.visualization.SnapshotGallery(THUMB, n_streams=S, max_tracks=256, max_updated=256, max_retired=512, retire_after=30)
    flat = lambda t: np.full(N_TRACKS, 0.6, np.float32)
    res = {"tool": "tools/snapshot_time.py", "streams": S, "size": f"{W}x{H}", "tracks_per_stream": N_TRACKS, "thumb": list(THUMB), "box": [bw, bh],
           "warmup": a.warmup, "repeat": a.repeat}
    # ---- first call: every track takes its shot ----
    update(bt, 0, flat)
    first, first_n, first_bytes = [], [], []
    for r in range(a.first):
        g.reset()
        first.append(call(g, bt))
        first_n.append(len(g.updated))
        if r == 0:
            first_bytes.append(floor_bytes(g, bt))
    res["first_call_ms_raw"] = first
    res["first_call_ms"] = float(np.median(first[2:]))
    res["first_call_thumbnails"] = float(np.mean(first_n))
    res["first_call_floor_bytes"] = int(first_bytes[0])
    # ---- steady state: a rotating 3 % of the tracks improve by 15 % each time their turn comes ----
    turns = np.zeros(N_TRACKS, np.int64)

    def rising(t):
        turns[np.arange(N_TRACKS) % 33 == t % 33] += 1
        return np.minimum(0.99, 0.6 * 1.15 ** turns).astype(np.float32)

    steady, steady_n, steady_bytes = [], [], []
    for t in range(1, a.warmup + a.repeat + 1):
        update(bt, t, rising)
        ms = call(g, bt)
        if t > a.warmup:
            steady.append(ms)
            steady_n.append(len(g.updated))
            steady_bytes.append(floor_bytes(g, bt))
    # the confidences saturate towards the end of the run: calls that rewrote something and calls that rewrote nothing are two
    # populations, and every steady-state figure (time, thumbnails, share, floor) is taken over the first one alone
    wrote = np.asarray(steady_n) > 0
    res["steady_ms_raw"] = steady
    res["steady_thumbnails_raw"] = steady_n
    res["steady_calls"] = int(wrote.sum())
    res["steady_ms"] = float(np.median(np.asarray(steady)[wrote]))
    res["steady_thumbnails"] = float(np.mean(np.asarray(steady_n)[wrote]))
    res["steady_share"] = res["steady_thumbnails"] / (S * N_TRACKS)
    res["steady_floor_bytes"] = float(np.mean(np.asarray(steady_bytes)[wrote]))
    res["steady_tail_calls"] = int((~wrote).sum())
    res["steady_tail_ms"] = float(np.median(np.asarray(steady)[~wrote])) if (~wrote).any() else float("nan")
    # ---- kept only: the steady state's configuration and outputs, fresh trackers, two box sizes; then without outputs ----
    cfg_kw = dict(n_streams=S, max_tracks=256, max_updated=256, max_retired=512, retire_after=30)
    for name, scale, want in (("kept_small", 1, True), ("kept_large", 3, True), ("kept_quiet", 1, False)):
        g2 = pkg.visualization.SnapshotGallery(THUMB, **cfg_kw)
        b2 = new_core()
        ms, n_upd = [], 0
        for t in range(a.warmup + a.repeat):
            update(b2, t, flat, scale)
            v = call(g2, b2, want=want or t == 0)
            if t >= a.warmup:
                ms.append(v)
                n_upd += len(g2.updated) if want else 0
        res[name + "_ms"] = float(np.median(ms))
        res[name + "_thumbnails"] = n_upd
        res[name + "_rows"] = len(g2.snapshot(0)["rows"])
        g2.close(); b2.close()
    # ---- the render kernel on the same frames ----
    lists = [render_time.scene(rng) for _ in range(S)]
    r = pkg.FrameRenderer()
    rk = []
    for i in range(a.warmup + 20):
        r.render_batch(dev, lists, zones=render_time.ZONES, fps=30.0, latency_ms=5.0, height=H, width=W)
        if i >= a.warmup:
            rk.append(r.last_kernel_ms())
    res["render_kernel_ms"] = float(np.median(rk))
    res["floor_us"] = {"first_call": res["first_call_floor_bytes"] / HBM_COPY_BYTES_PER_S * 1e6, "steady": res["steady_floor_bytes"] / HBM_COPY_BYTES_PER_S * 1e6}
    for k in ("first_call", "steady", "kept_small", "kept_large", "kept_quiet"):
        res[k + "_over_render"] = res[k + "_ms"] / res["render_kernel_ms"]
    res["first_call_over_floor"] = res["first_call_ms"] * 1e3 / res["floor_us"]["first_call"]
    res["steady_over_floor"] = res["steady_ms"] * 1e3 / max(res["floor_us"]["steady"], 1e-9)
    res["kept_large_over_small"] = res["kept_large_ms"] / res["kept_small_ms"]
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_raw")}))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "snapshot_time.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "README.md"), "w") as f:
            f.write(README.format(S=S, W=W, H=H, n=N_TRACKS, bw=bw, bh=bh, tw=THUMB[1], th=THUMB[0], warmup=a.warmup, first_n=res["first_call_thumbnails"],
                                  first_ms=res["first_call_ms"], first_over_render=res["first_call_over_render"], first_over_floor=res["first_call_over_floor"],
                                  steady_share=res["steady_share"], steady_n=res["steady_thumbnails"], steady_ms=res["steady_ms"],
                                  steady_over_render=res["steady_over_render"], steady_over_floor=res["steady_over_floor"], kept_small_ms=res["kept_small_ms"],
                                  kept_small_over_render=res["kept_small_over_render"], kept_large_ms=res["kept_large_ms"],
                                  kept_large_over_render=res["kept_large_over_render"], render_ms=res["render_kernel_ms"],
                                  first_floor_mb=res["first_call_floor_bytes"] / 1e6, steady_floor_kb=res["steady_floor_bytes"] / 1e3,
                                  bw_tb=HBM_COPY_BYTES_PER_S / 1e12, first_floor_us=res["floor_us"]["first_call"], steady_floor_us=res["floor_us"]["steady"],
                                  kept_ratio=res["kept_large_over_small"], steady_calls=res["steady_calls"], tail_calls=res["steady_tail_calls"],
                                  tail_ms=res["steady_tail_ms"], kept_small_n=res["kept_small_thumbnails"], kept_large_n=res["kept_large_thumbnails"],
                                  kept_quiet_ms=res["kept_quiet_ms"], kept_quiet_over_render=res["kept_quiet_over_render"]))
    g.close(); r.close(); bt.close(); dev.free()


if __name__ == "__main__":
    main()
