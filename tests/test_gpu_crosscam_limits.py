"""GPU: the cross-camera linker (csrc/crosscam.hip) at its default dim and past one workgroup, against its restatement
(tests/crosscam_ref.py), through the C ABI and with exact equality after every call (test_gpu_crosscam.py: check_call).  The
scenarios are those of tests/crosscam_limit_cases.py; tests/test_crosscam_cases_cpu.py proves on the restatement alone that each of
them reaches the code it is meant for: more than one 64-wide k-chunk in every kernel, a retirement wave across table row 1024 and
ledger index 256, JOINs past the 64th birth of a call and with a full table, 64 streams."""
import ctypes as C
import os
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crosscam_limit_cases as LC  # noqa: E402
import crosscam_ref as R  # noqa: E402
from test_gpu_crosscam import check_call, linker  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def pair(pkg, scn):
    """-> (a handle, the restatement), both with the scenario's transit and snapshot."""
    kw, transit, snap, _ = scn
    link, ref = linker(pkg, **kw), R.CrossCamRef(**kw)
    for t in transit:
        link.set_transit(*t)
        ref.set_transit(*t)
    if snap is not None:
        link.load(snap)
        ref.load(snap)
        assert R.snapshots_equal(link.snapshot(), ref.snapshot()) is None
    return link, ref


def drive(pkg, scn, tag):
    link, ref = pair(pkg, scn)
    for c, lists in enumerate(scn[3]):
        check_call(link, ref, link.process(lists), ref.process(lists), (tag, c))
    return link, ref


# ---------------------------------------------------------------------------------------------------------------- 1. the scenarios
@pytest.mark.parametrize("dim", [128, 192, 512])
def test_wide(pkg, dim):
    """Two, three and eight k-chunks in cc_gather, cc_update, cc_compact, cc_bound and the in-pipeline GEMM; rows that are zero in
    chunk 0, rows of -128 and of 127 under the EMA, pairs equal in chunk 0 alone."""
    link, ref = drive(pkg, LC.wide(dim), f"wide{dim}")
    assert len(ref.table) == 20 and ref.err == [0, 0, 0]
    link.close()


def test_retire_wave(pkg):
    """A loaded table of 1300 rows: 406, 138 and 122 leave in three calls on both sides of row 1024, so cc_retire carries both counts
    between chunks and cc_compact moves rows to other ranks; ledgers of 790 / 770 bindings lose, keep, displace and gain bindings past
    index 256."""
    link, ref = drive(pkg, LC.retire_wave(), "retire_wave")
    assert ref.counters["n_retired"] > 100 and ref.err == [0, 0]
    link.close()


def test_join_fan(pkg):
    """90 births in one call: JOINs of founders past lane 63 of cc_births, three equal founders joined in gid order, JOINs with the
    table full, a stream that may join through one of two streams only."""
    link, ref = drive(pkg, LC.join_fan(), "join_fan")
    assert ref.counters["n_table_full"] > 0 and ref.counters["n_events"] > 100
    link.close()


def test_sixty_four_streams(pkg):
    """The stream limit: bit 63 of stream_mask and of cc_births' live masks, transit windows 63 <-> 0."""
    link, ref = drive(pkg, LC.sixty_four_streams(), "streams64")
    assert len(ref.table) == 0
    link.close()


# ---------------------------------------------------------------------------------------------------------------- 2. a device source
def test_botsort_handle_at_dim_128(pkg):
    """cc_stage's row copy with D / 16 = 8: process_tracker equals the restatement fed from snapshot()."""
    core_cls = import_module(pkg.__name__ + ".tracking.botsort")._BotSortCore
    params, streams = LC.botsort_streams(128, 8)
    S, N, dim = 2, 16, 128
    core = core_cls(n_streams=S, max_tracks=32, max_dets=N, embedder="colorhist", dim=dim, **params)
    link, ref = linker(pkg, S, dim, min_sim_milli=600), R.CrossCamRef(S, dim, min_sim_milli=600)
    n_entries = 0
    for f in range(8):
        xy, cf, cl = np.zeros((S, N, 4), F32), np.zeros((S, N), F32), np.zeros((S, N), np.int32)
        emb, cnt = np.zeros((S, N, dim), np.int8), np.zeros(S, np.int32)
        for s, fr in enumerate(streams):
            b, c, k, d = fr[f]
            n = len(b)
            xy[s, :n], cf[s, :n], cl[s, :n], cnt[s] = b, c, k, n
            if n:
                emb[s, :n] = d
        core.update_batch(xy, cf, cl, cnt, embeddings=emb)
        res = link.process_tracker(core)
        lists = []
        for s in range(S):
            st = core.snapshot(s)
            sel = np.nonzero((st["flag"] == 2) & (st["tsu"] == 0))[0]
            assert st["feat8"].shape[1] == dim
            lists.append((st["ids"][sel], st["cls"][sel], st["feat8"][sel]))
            n_entries += len(sel)
        check_call(link, ref, res, ref.process(lists), ("botsort128", f))
    assert n_entries > 20 and len(ref.table) > 0
    core.close(); link.close()


# ---------------------------------------------------------------------------------------------------------------- 3. no outputs
def raw_process(pkg, link, lists, out):
    """rtmodt_crosscam_process as CrossCameraLinker.process calls it, with the caller's `out`."""
    ffi = pkg._ffi
    S, D = link.n_streams, link.dim
    counts = np.asarray([len(l[0]) for l in lists], np.int32)
    stride = max(1, int(counts.max()))
    ids, cls, rows = np.zeros((S, stride), np.int64), np.zeros((S, stride), np.int32), np.zeros((S, stride, D), np.int8)
    for s, (i, k, r) in enumerate(lists):
        n = counts[s]
        if n:
            ids[s, :n], cls[s, :n], rows[s, :n] = np.asarray(i, np.int64), np.asarray(k, np.int32), np.asarray(r, np.int8).reshape(n, D)
    ffi.check(ffi.lib().rtmodt_crosscam_process(link._h, ffi.ptr(ids), ffi.ptr(cls), ffi.ptr(rows), ffi.ptr(counts), stride, out))


def test_calls_without_outputs(pkg):
    """out = NULL: nothing is copied back and nothing waits, the state moves on all the same; then a struct of null pointers."""
    frames, _, _ = R.random_site(seed=8, calls=10)
    scn = (dict(n_streams=3, dim=64), [(0, 2, 1, 0)], None, frames)
    link, ref = pair(pkg, scn)
    for lists in frames[:3]:
        raw_process(pkg, link, lists, None)
        ref.process(lists)
    assert R.snapshots_equal(link.snapshot(), ref.snapshot()) is None and link.errors() == ref.err
    assert ref.c == 3 and len(ref.table) > 0
    check_call(link, ref, link.process(frames[3]), ref.process(frames[3]), ("after null", 3))
    raw_process(pkg, link, frames[4], C.byref(pkg._ffi.CrossCamOut()))
    ref.process(frames[4])
    assert R.snapshots_equal(link.snapshot(), ref.snapshot()) is None
    for c in range(5, 10):
        check_call(link, ref, link.process(frames[c]), ref.process(frames[c]), ("after null", c))
    link.close()


# ---------------------------------------------------------------------------------------------------------------- 4. load at size
def test_load_at_size_into_two_handles(pkg):
    """The retire_wave snapshot (1300 rows, 790 / 770 bindings) loaded into two fresh handles: both equal each other and the
    restatement after every call."""
    scn = LC.retire_wave()
    a, ref = pair(pkg, scn)
    b, _ = pair(pkg, scn)
    assert all(a.global_id(int(l), s) == int(g) for s, led in enumerate(scn[2]["ledgers"]) for l, g, _ in led[::37])
    for c, lists in enumerate(scn[3]):
        want = ref.process(lists)
        ra, rb = a.process(lists), b.process(lists)
        check_call(a, ref, ra, want, ("first", c))
        check_call(b, ref, rb, want, ("second", c))
        assert ra == rb and R.snapshots_equal(a.snapshot(), b.snapshot()) is None
    a.close(); b.close()
