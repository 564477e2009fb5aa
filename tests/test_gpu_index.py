"""GPU: the appearance index (csrc/index.hip) against its restatement (tests/index_ref.py), through the C ABI and with exact
equality: every hit (rid, key, stream, class, time, ppm), every n_hits, the unused entries, and the whole archive in slot order
after the calls that change it.  tests/test_index_cpu.py checks the restatement itself against hand-worked literals and a
brute-force double loop, and that the shared cases of tests/index_cases.py reach what they are meant to reach.  PARITY UNPINNED:
no published vector index is installed; the restatement is the rule set of include/rtmodt.h as this project states it."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crosscam_ref as CR  # noqa: E402
import index_cases as K  # noqa: E402
import index_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def mod(pkg):
    return import_module(pkg.__name__ + ".tracking.search")


def pair(pkg, dim, capacity, chunk_rows=0, max_add=4096, **kw):
    """A handle and the restatement with the same configuration."""
    return mod(pkg).AppearanceIndex(dim, capacity, chunk_rows=chunk_rows, max_add=max_add, **kw), R.IndexRef(dim, capacity, chunk_rows_req=chunk_rows, max_add=max_add, **kw)


def ffi_filter(pkg, f):
    return pkg._ffi.IndexFilter(f["t0"], f["t1"], f["mask"], f["excl"], f["cls"], f["min_ppm"])


def check_search(pkg, idx, ref, queries, filters, k, tag):
    want = ref.search(queries, filters, k)
    assert want != R.E_INVALID, tag
    got = idx.search(queries, k, filters=[ffi_filter(pkg, f) for f in filters])
    assert [[(h.rid, h.key, h.stream, h.cls, h.t, h.similarity_ppm) for h in hits] for hits in got] == want, tag
    nh, raw = idx.last_raw
    assert nh.tolist() == [len(w) for w in want], tag
    for i, w in enumerate(want):                               # the unused entries are zero
        assert not raw[i, len(w):].tobytes().strip(b"\0"), (tag, i)
    return want


def check_state(idx, ref, tag):
    assert R.snapshots_equal(idx.snapshot(), ref.snapshot()) is None, (tag, R.snapshots_equal(idx.snapshot(), ref.snapshot()))
    assert len(idx) == len(ref) and idx.next_rid == ref.next_rid, tag


# ---------------------------------------------------------------------------------------------------------------- 1. fragment and tile edges
@pytest.mark.parametrize("dim", [64, 192, 512])
def test_fragment_and_tile_edges(pkg, dim):
    """One, three and eight k-chunks; archive sizes and query counts at the edges of the 16 x 16 fragment, of the 64-row step and of
    the chunk (chunk_rows 64: 129 rows are three chunks); rows of -128, of 127 and of zeros; k 1, 5, 64; min_ppm 1, 500000, 1000000."""
    rng = np.random.default_rng(dim)
    rows = rng.integers(-128, 128, (129, dim)).astype(np.int8)
    rows[0], rows[14], rows[15], rows[16], rows[64], rows[128] = -128, 127, 0, 127, -128, 0
    rows[70:76] = np.clip(rows[3].astype(np.int32) + rng.integers(-20, 21, (6, dim)), -128, 127)       # some sims between the thresholds
    queries = rng.integers(-128, 128, (64, dim)).astype(np.int8)
    queries[0], queries[1], queries[2], queries[3], queries[14], queries[16], queries[63] = -128, 127, 0, rows[3], rows[70], rows[71], rows[128 - 1]
    meta = K.metadata(129, dim)
    n_hits = 0
    for n in (1, 15, 16, 17, 63, 64, 65, 129):
        idx, ref = pair(pkg, dim, 129, chunk_rows=64)
        K.fill(idx, rows[:n], meta)
        K.fill(ref, rows[:n], meta)
        check_state(idx, ref, (dim, n))
        for nq, k, ppm in ((1, 1, 1), (15, 5, 500000), (16, 64, 1), (17, 5, 1000000), (63, 1, 500000), (64, 64, 1), (64, 5, 1000000), (16, 1, 1)):
            want = check_search(pkg, idx, ref, queries[:nq], [R.filt(ppm)] * nq, k, (dim, n, nq, k, ppm))
            n_hits += sum(len(w) for w in want)
        idx.close()
    assert n_hits > 1000


# ---------------------------------------------------------------------------------------------------------------- 2. selection
def loaded(pkg, case, **kw):
    cfg, rows, meta, queries, filters = case
    idx, ref = pair(pkg, cfg["dim"], cfg["capacity"], chunk_rows=cfg["chunk_rows"], **kw)
    K.fill(idx, rows, meta, batch=300)
    K.fill(ref, rows, meta, batch=300)
    return idx, ref, queries, filters


@pytest.mark.parametrize("k", [16, 64])
def test_selection_across_chunks(pkg, k):
    """1000 rows in 16 chunks with 40 exact duplicates scattered over them: at k = 16 a buffer overflows several times inside a chunk,
    and the merge breaks the duplicates' ties by rid across chunks."""
    idx, ref, queries, filters = loaded(pkg, K.selection())
    check_state(idx, ref, "selection")
    want = check_search(pkg, idx, ref, queries, filters, k, ("selection", k))
    assert [h[0] for h in want[1]] == sorted((s + 1 for s in K.DUP_SLOTS), reverse=True)[:k]
    idx.close()


def test_selection_inside_a_crowded_chunk(pkg):
    """Chunks of 512 rows, nearly all of them eligible: the buffer of 128 overflows several times inside a chunk at k = 64, and much
    more often at k = 1 and 5."""
    idx, ref, queries, filters = loaded(pkg, K.crowded())
    for k in (64, 5, 1):
        check_search(pkg, idx, ref, queries, filters, k, ("crowded", k))
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- 3. filters
def test_filters_one_at_a_time_and_together(pkg):
    idx, ref, queries, _ = loaded(pkg, K.selection())
    q = queries[[0, 4]]
    key0 = int(ref.key[K.DUP_SLOTS[0]])
    singles = [R.filt(1, t_range=(163, 164)), R.filt(1, t_range=(100 + 63, 100 + 65)), R.filt(1, streams=[63]), R.filt(1, streams=[0, 63]),
               R.filt(1, cls=2), R.filt(1, exclude_key=key0), R.filt(1, t_range=(5000, 6000)), R.filt(1, streams=[])]
    for i, f in enumerate(singles):
        check_search(pkg, idx, ref, q, [f, f], 64, ("single", i))
    both = R.filt(150000, t_range=(150, 900), streams=list(range(0, 64, 3)) + [63], cls=1, exclude_key=key0)
    want = check_search(pkg, idx, ref, q, [both, R.filt(1)], 64, "together")
    assert 1 <= len(want[0]) < 64 and len(want[1]) == 64
    # keys forgotten between two searches
    keys = sorted({h[1] for h in want[1]})[:5] + [999999]
    n_ref = ref.forget(keys)
    assert idx.forget(keys) == n_ref and n_ref >= 5
    check_state(idx, ref, "forget")
    after = check_search(pkg, idx, ref, q, [both, R.filt(1)], 64, "after forget")
    assert not {h[1] for h in after[1]} & set(keys) and after != want
    assert idx.forget(keys) == 0 and idx.forget([]) == 0
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the ring
def test_ring_wraps_and_restores(pkg, tmp_path):
    """capacity 100, 250 rows in batches of 37: the state after every batch, a search after the wrap, load(snapshot()) into a fresh
    handle, and save / restore through a file."""
    rng = np.random.default_rng(4)
    rows = rng.integers(-128, 128, (250, 64)).astype(np.int8)
    rows[::9] = rows[0]
    keys, streams, cls, t = K.metadata(250, 4)
    idx, ref = pair(pkg, 64, 100, chunk_rows=64)
    for b in range(0, 250, 37):
        sl = slice(b, min(250, b + 37))
        assert idx.add(rows[sl], keys[sl], streams[sl], cls[sl], t[sl]) == ref.add(rows[sl], keys[sl], streams[sl], cls[sl], t[sl]) == b + 1
        check_state(idx, ref, b)
    assert len(idx) == 100 and idx.next_rid == 251
    queries, fs = np.stack([rows[0], rows[249], rows[100]]), [R.filt(1), R.filt(1), R.filt(400000)]
    want = check_search(pkg, idx, ref, queries, fs, 64, "wrapped")
    assert all(151 <= h[0] <= 250 for w in want for h in w) and len(want[0]) >= 12    # live rids only; the copies of row 0 among them
    idx.forget([int(keys[249])])
    ref.forget([int(keys[249])])
    fresh = mod(pkg).AppearanceIndex(64, 100, chunk_rows=64)
    fresh.load(idx.snapshot())
    check_state(fresh, ref, "loaded")
    path = str(tmp_path / "archive.npz")
    idx.save(path)
    restored = mod(pkg).AppearanceIndex.restore(path, chunk_rows=64)
    check_state(restored, ref, "restored")
    for k in (1, 64):
        w = check_search(pkg, idx, ref, queries, fs, k, ("before", k))
        assert check_search(pkg, fresh, ref, queries, fs, k, ("fresh", k)) == w == check_search(pkg, restored, ref, queries, fs, k, ("restored", k))
    more = rng.integers(-128, 128, (5, 64)).astype(np.int8)                                 # a restart goes on where the other stopped
    assert fresh.add(more, [1, 2, 3, 4, 5], 1, 1, 9) == ref.add(more, [1, 2, 3, 4, 5], 1, 1, 9) == 251
    check_state(fresh, ref, "after restart")
    for h in (idx, fresh, restored):
        h.close()


def test_a_list_longer_than_the_ring(pkg):
    idx, ref = pair(pkg, 64, 10, max_add=64)
    rows = np.random.default_rng(6).integers(-128, 128, (25, 64)).astype(np.int8)
    meta = K.metadata(25, 6)
    assert idx.add(rows, *meta) == ref.add(rows, *meta) == 1
    check_state(idx, ref, "long list")
    check_search(pkg, idx, ref, rows[[24, 3]], [R.filt(1)] * 2, 5, "long list")
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- 5. device rows
def test_device_rows_equal_host_rows(pkg):
    rows = np.random.default_rng(7).integers(-128, 128, (70, 192)).astype(np.int8)
    meta = K.metadata(70, 7)
    a, ref = pair(pkg, 192, 80, chunk_rows=64)
    b = mod(pkg).AppearanceIndex(192, 80, chunk_rows=64)
    buf = pkg._ffi.DeviceBuffer(rows.nbytes)
    buf.upload(rows)
    assert a.add(rows, *meta) == b.add(buf, *meta) == ref.add(rows, *meta) == 1
    check_state(a, ref, "host")
    check_state(b, ref, "device")
    buf.free(); a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 6. from a linker
@pytest.mark.parametrize("every", [1, 3])
def test_add_from_linker(pkg, every):
    """A CrossCameraLinker driven with crosscam_ref.random_site(); after every call its sighted identities are appended on the device.
    The archive equals the restatement fed from link.snapshot(); then every identity's own s8 finds its gid first."""
    frames, _, _ = CR.random_site()
    link = import_module(pkg.__name__ + ".tracking.crosscam").CrossCameraLinker(3, 64, max_tracks=64, max_identities=256, max_queries=256, max_age=300)
    for tr in [(0, 2, 1, 0), (2, 0, 2, 300)]:
        link.set_transit(*tr)
    idx, ref = pair(pkg, 64, 300, chunk_rows=64)
    total = 0
    for c, lists in enumerate(frames):
        link.process(lists)
        n = idx.add_from_linker(link, t=1000 + c, every=every)
        assert n == ref.add_from_snapshot(link.snapshot(), 1000 + c, every), c
        total += n
        check_state(idx, ref, ("linker", c))
    assert total > (300 if every == 1 else 60) and len(idx) == min(total, 300)
    snap = link.snapshot()
    live = sorted(set(ref.key[ref.rid > 0].tolist()))
    sel = [i for i, g in enumerate(snap["gid"]) if int(g) in live][:64]
    want = check_search(pkg, idx, ref, snap["s8"][sel], [R.filt(500000)] * len(sel), 10, "own feature")
    assert len(sel) >= 10 and all(w and w[0][1] == int(snap["gid"][i]) for w, i in zip(want, sel))
    idx.close(); link.close()


# ---------------------------------------------------------------------------------------------------------------- 7. auto chunking
def test_large_archive_with_chosen_chunks(pkg):
    """20000 rows of dim 512 (chunks of 128 rows chosen by the library: 157 of them), 64 queries, k 64, against one NumPy int32
    product."""
    rng = np.random.default_rng(8)
    n, dim = 20000, 512
    rows = rng.integers(-128, 128, (n, dim)).astype(np.int8)
    queries = rng.integers(-128, 128, (64, dim)).astype(np.int8)
    for i in range(32):                                        # planted near-duplicates and exact copies of half the queries
        at = rng.integers(0, n, 12)
        rows[at[:10]] = np.clip(queries[i].astype(np.int32) + rng.integers(-40, 41, (10, dim)), -128, 127)
        rows[at[10:]] = queries[i]
    idx, ref = pair(pkg, dim, n)
    assert ref.chunk == 128
    meta = K.metadata(n, 8)
    K.fill(idx, rows, meta)
    K.fill(ref, rows, meta)
    filters = [R.filt(1 if i % 2 else 300000, cls=None if i % 3 else 1) for i in range(64)]
    want = check_search(pkg, idx, ref, queries, filters, 64, "large")
    assert all(len(w) == 64 for w in want[1::2]) and all(1 <= len(w) < 64 for w in want[0:32:6]) and sum(len(w) for w in want) > 2000
    nh, raw = idx.last_raw
    assert np.array_equal(idx.snapshot()["n2"], ref.n2)
    add_ms, search_ms = idx.last_ms()
    assert add_ms > 0 and search_ms > 0
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_change_nothing(pkg):
    ffi, S = pkg._ffi, mod(pkg)
    for kw in (dict(dim=96), dict(dim=576), dict(capacity=0), dict(capacity=(1 << 22) + 1), dict(max_queries=65), dict(max_k=65), dict(max_k=0),
               dict(max_add=65537), dict(chunk_rows=96), dict(capacity=16385, chunk_rows=64)):
        with pytest.raises(ffi.RtmodtError) as e:
            S.AppearanceIndex(**{**dict(dim=64, capacity=100), **kw})
        assert e.value.code == ffi.E_INVALID and "index" in str(e.value), kw
    idx, ref = pair(pkg, 64, 100, chunk_rows=64, max_add=8, max_queries=4, max_k=8)
    rows = np.random.default_rng(9).integers(-128, 128, (9, 64)).astype(np.int8)
    idx.add(rows[:5], [1, 2, 3, 4, 5], 0, 0, 0)
    ref.add(rows[:5], [1, 2, 3, 4, 5], 0, 0, 0)
    before = idx.snapshot()

    def refused(fn, *a, **k):
        with pytest.raises(ffi.RtmodtError) as e:
            fn(*a, **k)
        assert e.value.code == ffi.E_INVALID, str(e.value)
        assert R.snapshots_equal(idx.snapshot(), before) is None
        return str(e.value)

    assert "max_add" in refused(idx.add, rows, np.arange(9), 0, 0, 0)                      # n > max_add
    assert "stream" in refused(idx.add, rows[:2], [1, 2], [0, 64], 0, 0)                   # a stream of 64
    refused(idx.add, rows[:2], [1, 2], [-1, 0], 0, 0)
    assert "dim" in refused(idx.add, rows[:2, :32], [1, 2], 0, 0, 0)                       # rows of another dim
    assert "max_queries" in refused(idx.search, rows[:5], 3, min_ppm=1)                    # nq > max_queries
    assert "max_k" in refused(idx.search, rows[:2], 9, min_ppm=1)                          # k > max_k
    refused(idx.search, rows[:2], 0, min_ppm=1)
    assert "min_ppm" in refused(idx.search, rows[:2], 3, min_ppm=0)
    refused(idx.search, rows[:2], 3, min_ppm=1000001)
    assert "dim" in refused(idx.search, rows[:2, :32], 3, min_ppm=1)
    refused(idx.forget, np.arange(4097))
    crosscam = import_module(pkg.__name__ + ".tracking.crosscam").CrossCameraLinker
    for kw, word in ((dict(dim=128, max_identities=8), "dim"), (dict(dim=64, max_identities=9), "max_add")):     # a foreign linker
        link = crosscam(1, kw["dim"], max_tracks=4, max_identities=kw["max_identities"], max_queries=4)
        assert word in refused(idx.add_from_linker, link, 0)
        link.close()
    link = crosscam(1, 64, max_tracks=4, max_identities=8, max_queries=4)
    assert "every" in refused(idx.add_from_linker, link, 0, 0)
    assert idx.add_from_linker(link, 0) == 0                                               # a linker that has seen nothing yet
    link.close()
    for field, slot, value in (("rid", 0, 2), ("rid", 5, 6), ("rid", 4, 105), ("stream", 0, 64), ("dead", 1, 2)):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
        bad[field][slot] = value
        assert ref.load(bad) == R.E_INVALID
        assert "load" in refused(idx.load, bad), field
    bad = dict(before)
    bad["next_rid"] = 5                                                                    # rid 5 >= next_rid
    refused(idx.load, bad)
    check_state(idx, ref, "after the refusals")
    idx.close()
