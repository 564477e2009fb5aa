"""Times the cross-camera linker per call: device time (HIP events around the launches of one rtmodt_crosscam_process_botsort) at
8 streams x 200 tracks, dim 512, on one BoT-SORT handle, beside that handle's own update in the same run.  Three regimes:
  births   the first two calls of a fresh linker on a warm tracker: 1600 queries, 1024 born in the first call and 576 in the second;
  steady   3 % of every stream's objects are replaced per frame, so about 3 % of the entries are queries against a table of about
           1600 identities plus the ones not yet retired;
  bound    a still scene: every entry is bound, no query.
Nothing is asserted: the numbers are reported, not gated.  The GEMM's floors are computed from the shapes (bytes over the HBM peak,
operations over the int8 MFMA peak); its own device time comes from a kernel trace of this script (profiles/crosscam/README.md).

    python tools/crosscam_time.py [--repeat 30] [--out profiles/crosscam/crosscam_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rtmodt_amd  # noqa: E402

S, N, DIM = 8, 200, 512
HBM_PEAK, I8_PEAK = 8.0e12, 5.0e15                         # bytes/s and int8 operations/s, dense (the data sheet's)
GRID = 40                                                   # cells per row of the 96-px grid; 1600 cells for 200 objects and their successors


class Scene:
    """200 objects per stream on a grid, each with a descriptor of its own; replace(k) moves k objects per stream to fresh cells
    with fresh descriptors (the old tracks go lost, the new ones are tracked one frame later)."""

    def __init__(self, seed=1):
        self.rng = np.random.default_rng(seed)
        self.cell = np.tile(np.arange(N), (S, 1))
        self.next_cell = N
        self.rows = self.rng.integers(-127, 128, (S, N, DIM)).astype(np.int8)
        self.wh = np.round(self.rng.uniform(28, 40, (S, N, 2)) * 4) / 4

    def replace(self, k):
        for s in range(S):
            for i in self.rng.choice(N, k, replace=False):
                self.cell[s, i] = self.next_cell
                self.next_cell = self.next_cell + 1 if self.next_cell + 1 < GRID * GRID else 0
                self.rows[s, i] = self.rng.integers(-127, 128, DIM)
        taken = set()                                       # a recycled cell may still be in use: move on until it is free
        for s in range(S):
            taken.clear()
            for i in range(N):
                while int(self.cell[s, i]) in taken:
                    self.cell[s, i] = (self.cell[s, i] + 1) % (GRID * GRID)
                taken.add(int(self.cell[s, i]))

    def frame(self):
        p = np.stack([(self.cell % GRID) * 96.0 + 8, (self.cell // GRID) * 96.0 + 8], 2)
        return np.concatenate([p, p + self.wh], 2).astype(np.float32)


def step(bot, scene):
    xy = scene.frame()
    bot.update_batch(xy, np.full((S, N), 0.9, np.float32), np.zeros((S, N), np.int32), np.full(S, N, np.int32), embeddings=scene.rows)
    return float(sum(bot.last_ms()[1:]))


def gemm_floor(n_q, n_t):
    by = n_q * DIM + (n_t + n_q) * DIM + 4 * n_q * (n_t + n_q)
    ops = 2 * n_q * (n_t + n_q) * DIM
    return {"queries": n_q, "columns": n_t + n_q, "bytes": by, "int8_ops": ops, "byte_floor_us": by / HBM_PEAK * 1e6, "mfma_floor_us": ops / I8_PEAK * 1e6}


def med(v):
    return float(np.median(np.asarray(v, np.float64))) if len(v) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crosscam", "crosscam_time.json"))
    a = ap.parse_args()
    T = import_module(rtmodt_amd.__name__ + ".tracking")
    bot = T.botsort._BotSortCore(track_buffer=5, embedder="colorhist", dim=DIM, n_streams=S, max_tracks=256, max_dets=N)   # 200 + 6 x 6 lost tracks fit
    mk = lambda **kw: T.CrossCameraLinker(S, DIM, **kw)     # noqa: E731  (the caps: 256 tracks, 4096 identities, 1024 queries)
    scene = Scene()
    for _ in range(4):                                      # a warm tracker: every object tracked
        step(bot, scene)
    out = {"setup": {"streams": S, "tracks_per_stream": N, "dim": DIM, "max_identities": 4096, "max_queries": 1024}}
    # ---- births
    first, second, bot_ms, counters = [], [], [], None
    for _ in range(max(3, a.repeat // 3)):
        link = mk()
        bot_ms.append(step(bot, scene))
        r1 = link.process_tracker(bot); first.append(link.last_ms())
        bot_ms.append(step(bot, scene))
        r2 = link.process_tracker(bot); second.append(link.last_ms())
        counters = [r1.counters, r2.counters]
        link.close()
    out["births"] = {"first_call_ms": med(first), "second_call_ms": med(second), "botsort_update_ms": med(bot_ms), "counters": counters,
                     "gemm": [gemm_floor(c["n_queries"], c["n_identities"] - (c["n_queries"] - c["n_table_full"])) for c in counters]}
    # ---- steady: 3 % replaced per frame
    link = mk(max_age=8)
    for _ in range(2):
        step(bot, scene); link.process_tracker(bot)
    t, bt, nq, nid = [], [], [], []
    for k in range(10 + a.repeat):
        scene.replace(6)
        b = step(bot, scene)
        r = link.process_tracker(bot)
        if k >= 10:
            t.append(link.last_ms()); bt.append(b); nq.append(r.counters["n_queries"]); nid.append(r.counters["n_identities"])
    out["steady"] = {"call_ms": med(t), "botsort_update_ms": med(bt), "queries_per_call": med(nq), "identities": med(nid),
                     "gemm": gemm_floor(int(med(nq)), int(med(nid)))}
    # ---- bound: a still scene
    for _ in range(3):
        step(bot, scene); link.process_tracker(bot)
    t, bt, nq = [], [], []
    for _ in range(a.repeat):
        b = step(bot, scene)
        r = link.process_tracker(bot)
        t.append(link.last_ms()); bt.append(b); nq.append(r.counters["n_queries"])
    out["bound"] = {"call_ms": med(t), "botsort_update_ms": med(bt), "queries_per_call": med(nq), "identities": r.counters["n_identities"]}
    link.close(); bot.close()
    out["how"] = ("median over the repeats of the HIP-event time around the memset and the ten launches of one rtmodt_crosscam_process_botsort call "
                  "(rtmodt_crosscam_last_ms), all streams together, and of the BoT-SORT handle's own distance + update launches of the frame before it "
                  "(rtmodt_botsort_last_ms); caller descriptors of 512 values; peaks for the floors: 8.0 TB/s, 5 Pop/s int8 dense")
    out["command"] = "python tools/crosscam_time.py --repeat %d" % a.repeat
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
