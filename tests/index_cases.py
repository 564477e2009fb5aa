"""The archives and queries the appearance-index tests share: ``tests/test_index_cpu.py`` asserts on the restatement alone that they
reach what they are meant to reach (a buffer that overflows inside a chunk, hits spread over chunks, ties across a chunk boundary,
short and empty answers), ``tests/test_gpu_index.py`` holds ``csrc/index.hip`` to the restatement on them."""
from __future__ import annotations

import numpy as np

import index_ref as R


def metadata(n, seed=0):
    """keys (50 distinct), streams (all 64), classes (3), times (ascending) for n rows."""
    rng = np.random.default_rng(1000 + seed)
    return (1000 + rng.integers(0, 50, n)).astype(np.int64), (np.arange(n) * 7 % 64).astype(np.int32), rng.integers(0, 3, n).astype(np.int32), \
        (100 + np.arange(n)).astype(np.int64)


def random_rows(n, dim, seed):
    return np.random.default_rng(seed).integers(-128, 128, (n, dim)).astype(np.int8)


def fill(ref_or_idx, rows, meta, batch=4096):
    """The same adds for the restatement and for a handle (both have ``add(rows, keys, streams, cls, t)``)."""
    k, s, c, t = meta
    for b in range(0, len(rows), batch):
        e = min(len(rows), b + batch)                       # (the metadata may be longer than the rows: a prefix of a case)
        ref_or_idx.add(rows[b:e], k[b:e], s[b:e], c[b:e], t[b:e])


DUP_SLOTS = [3, 63, 64, 65, 127, 128, 130, 190, 191, 192, 250, 300, 319, 320, 321, 400, 447, 448, 449, 500, 511, 512, 560, 575, 576, 600, 639, 640,
             700, 703, 704, 767, 768, 800, 831, 832, 895, 896, 960, 999]


def selection():
    """1000 rows of dim 64 in chunks of 64 (16 chunks), 40 exact duplicates of one row scattered over them (pairs across chunk
    boundaries: 63 | 64, 127 | 128, 191 | 192, ...).  -> (kw, rows, meta, queries, filters)."""
    dim, n = 64, 1000
    rows = random_rows(n, dim, 11)
    dup = random_rows(1, dim, 12)[0]
    assert len(DUP_SLOTS) == 40
    rows[DUP_SLOTS] = dup
    near = np.clip(rows[77].astype(np.int32) + np.random.default_rng(13).integers(-6, 7, dim), -128, 127).astype(np.int8)
    queries = np.stack([dup, dup, near, np.zeros(dim, np.int8), random_rows(1, dim, 14)[0], dup])
    filters = [R.filt(1), R.filt(R.PPM), R.filt(900000), R.filt(1), R.filt(1), R.filt(200000, t_range=(100 + 60, 100 + 700), cls=1)]
    return dict(dim=dim, capacity=n, chunk_rows=64), rows, metadata(n, 1), queries, filters


def crowded():
    """1000 rows of dim 64 in chunks of 512: every row is one base row plus noise, so that nearly every row is eligible for the base
    as a query and a buffer of 128 overflows several times inside a chunk at k = 64.  -> (kw, rows, meta, queries, filters)."""
    dim, n = 64, 1000
    rng = np.random.default_rng(21)
    base = rng.integers(-90, 91, dim)
    rows = np.clip(base[None, :] + rng.integers(-60, 61, (n, dim)), -128, 127).astype(np.int8)
    queries = np.stack([base.astype(np.int8), rows[5], (-base).astype(np.int8)])
    return dict(dim=dim, capacity=n, chunk_rows=512), rows, metadata(n, 2), queries, [R.filt(1), R.filt(500000), R.filt(1)]


def chunk_of(ref, rid):
    return ((rid - 1) % ref.N) // ref.chunk


def eligible_per_chunk(ref, query, f):
    """How many rows of each chunk are eligible for the query."""
    r = ref.ranks(query[None, :], [f])[0]
    n_chunks = -(-ref.N // ref.chunk)
    return [int((r[c * ref.chunk:(c + 1) * ref.chunk] > 0).sum()) for c in range(n_chunks)]
