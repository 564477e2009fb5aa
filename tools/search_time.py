"""Times the appearance index: device time (HIP events around the two launches of one rtmodt_index_search) on an archive of 2^20
rows of dim 512 -- random int8 with planted near-duplicates of the queries, so that hits exist -- at k = 16 for 1, 16 and 64
queries, beside the scan's byte floor (rows plus metadata read once at the measured copy rate of the card) and the time of an add
of 1600 rows (one frame set of 8 streams x 200 tracks).  Nothing is asserted: the numbers are reported, not gated.

    python tools/search_time.py [--rows 1048576] [--repeat 30] [--out profiles/search/search_time.json]
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

DIM, K = 512, 16
COPY_RATE = 6.29e12                                         # bytes/s, the card's measured device-to-device copy rate
META_BYTES = 3 * 8 + 4 * 4                                  # rid, key, t; stream, cls, n2, dead


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "search_time.json"))
    a = ap.parse_args()
    S = import_module(rtmodt_amd.__name__ + ".tracking.search")
    rng = np.random.default_rng(1)
    n = a.rows
    queries = rng.integers(-128, 128, (64, DIM)).astype(np.int8)
    idx = S.AppearanceIndex(DIM, n, max_add=65536)
    add_ms = []
    for b in range(0, n, 65536):                             # the archive, 65536 rows per add
        m = min(65536, n - b)
        rows = rng.integers(-128, 128, (m, DIM)).astype(np.int8)
        at = rng.integers(0, m, 64 * 24)                     # 24 near-duplicates of every query per batch
        rows[at] = np.clip(np.repeat(queries, 24, axis=0).astype(np.int32) + rng.integers(-48, 49, (64 * 24, DIM)), -128, 127)
        idx.add(rows, np.arange(b, b + m), (np.arange(m) % 64), 0, np.arange(b, b + m))
        add_ms.append(idx.last_ms()[0])
    floor_ms = n * (DIM + META_BYTES) / COPY_RATE * 1e3
    out = {"setup": {"rows": n, "dim": DIM, "k": K, "chunk_rows": (-(-n // 256) + 63) // 64 * 64, "planted_per_query": 24 * -(-n // 65536)},
           "scan_floor": {"bytes": n * (DIM + META_BYTES), "rate_bytes_per_s": COPY_RATE, "ms": floor_ms},
           "add_65536_rows": stats(add_ms), "search": {}}
    for label, ppm in (("min_ppm_500000", 500000), ("min_ppm_1", 1)):
        out["search"][label] = {}
        for nq in (1, 16, 64):
            t, hits = [], 0
            for r in range(3 + a.repeat):
                res = idx.search(queries[:nq], K, min_ppm=ppm)
                if r >= 3:
                    t.append(idx.last_ms()[1])
                hits = sum(len(h) for h in res)
            e = stats(t)
            e.update(hits=hits, times_floor=e["median_ms"] / floor_ms)
            out["search"][label]["nq_%d" % nq] = e
        s = out["search"][label]
        s["nq_64_over_nq_16"] = s["nq_64"]["median_ms"] / s["nq_16"]["median_ms"]
    t = []
    rows = rng.integers(-128, 128, (1600, DIM)).astype(np.int8)
    for r in range(3 + a.repeat):                            # one frame set: 8 streams x 200 tracks
        idx.add(rows, np.arange(1600), np.arange(1600) % 8, 0, r)
        if r >= 3:
            t.append(idx.last_ms()[0])
    out["add_1600_rows"] = stats(t)
    idx.close()
    out["how"] = ("median over the repeats of the HIP-event time around ix_scan + ix_merge of one rtmodt_index_search call, and around ix_add + "
                  "ix_advance of one rtmodt_index_add call (rtmodt_index_last_ms); the copies of the queries in and of the hits out are outside "
                  "the events; floor = (rows + metadata) bytes once at 6.29 TB/s")
    out["command"] = "python tools/search_time.py --rows %d --repeat %d" % (n, a.repeat)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
