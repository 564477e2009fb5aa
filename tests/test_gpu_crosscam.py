"""GPU: the cross-camera linker (csrc/crosscam.hip) against its restatement (tests/crosscam_ref.py), through the C ABI and with
exact equality.  After every call: the per-entry outputs, the events, the retired list and the counters; the whole table (gids,
classes, s16, s8, last_seen, first_seen); every ledger; the sticky errors.  tests/test_crosscam_cpu.py checks the restatement
itself against hand-worked literals and the scenario generators on the restatement alone.  PARITY UNPINNED: no published
multi-camera tracker is installed; the restatement is the rule set of include/rtmodt.h as this project states it."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import botsort_ref as BR  # noqa: E402
import crosscam_cases as K  # noqa: E402
import crosscam_ref as R  # noqa: E402
import deepsort_ref as DR  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def linker(pkg, n_streams, dim, max_tracks=64, max_identities=256, max_queries=256, min_sim_milli=700, max_age=300, bind_age=None, match_class=True):
    """A handle with the restatement's defaults."""
    cls = import_module(pkg.__name__ + ".tracking.crosscam").CrossCameraLinker
    return cls(n_streams, dim, max_tracks=max_tracks, max_identities=max_identities, max_queries=max_queries, min_similarity=min_sim_milli / 1000,
               max_age=max_age, bind_age=bind_age, match_class=match_class)


def check_call(link, ref, res, want, tag):
    assert want != R.E_INVALID, tag
    assert res.gid == want["gid"], (tag, "gid")
    assert res.status == want["status"], (tag, "status")
    assert res.sim == want["sim"], (tag, "sim")
    assert [(e.gid, e.stream, e.local_id, e.from_stream, e.gap, e.sim) for e in res.events] == want["events"], (tag, "events")
    assert [(r.gid, r.first_seen, r.last_seen, sum(1 << s for s in r.streams)) for r in res.retired] == want["retired"], (tag, "retired")
    assert res.counters == ref.counters, (tag, "counters")
    assert R.snapshots_equal(link.snapshot(), ref.snapshot()) is None, (tag, R.snapshots_equal(link.snapshot(), ref.snapshot()))
    assert link.errors() == ref.err, (tag, "errors")


def drive(pkg, scn, tag=""):
    kw, transit, calls = scn
    link, ref = linker(pkg, **kw), R.CrossCamRef(**kw)
    for t in transit:
        link.set_transit(*t)
        ref.set_transit(*t)
    for c, lists in enumerate(calls):
        check_call(link, ref, link.process(lists), ref.process(lists), (tag, c))
    return link, ref


# ---------------------------------------------------------------------------------------------------------------- 1. the hand cases
@pytest.mark.parametrize("name", sorted(K.HAND))
def test_hand_case_equals_restatement(pkg, name):
    link, ref = drive(pkg, K.HAND[name](), name)
    if name == "lap_limit":
        assert link.errors() == [0, 2]
        link.clear_errors()
        assert link.errors() == [0, 0]
    if name == "fragment":
        assert (link.global_id(7), link.global_id(9), link.label(9), link.label(8)) == (2, 1, "G1", "")
    link.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the GEMM alone
@pytest.mark.parametrize("dim", [64, 192, 512])
def test_similarity_equals_numpy(pkg, dim):
    """One, three and eight k-chunks; query counts and table sizes at the edges of the 16 x 16 fragment and of the 64 x 64 workgroup
    tile; rows of -128 and of 127."""
    mod = import_module(pkg.__name__ + ".tracking.crosscam")
    rng = np.random.default_rng(dim)
    Q, T = rng.integers(-128, 128, (129, dim)).astype(np.int8), rng.integers(-128, 128, (129, dim)).astype(np.int8)
    Q[0], T[0], Q[14], T[14], Q[16], T[64] = -128, -128, 127, 127, -128, 127
    for nq in (1, 15, 16, 17, 63, 64, 65, 129):
        for nt in (1, 15, 16, 17, 65, 128, 129):
            dots, sim = mod.similarity(Q[:nq], T[:nt])
            want = Q[:nq].astype(np.int32) @ T[:nt].astype(np.int32).T
            assert np.array_equal(dots, want), (nq, nt)
            q64, t64 = Q[:nq].astype(np.int64), T[:nt].astype(np.int64)
            assert np.array_equal(sim, R.sim_matrix(want, (q64 * q64).sum(axis=1), (t64 * t64).sum(axis=1))), (nq, nt)
    assert dots[0, 0] == dim * 128 * 128 and sim[0, 0] == 1000 and sim[0, 14] == 0


# ---------------------------------------------------------------------------------------------------------------- 3. a random site
def test_random_site(pkg):
    """3 streams, 40 calls, 12 people who cross between the cameras while their tracks fragment and their local ids change; the
    pair 0 -> 2 is closed and 2 -> 0 needs two calls."""
    frames, _, _ = R.random_site()
    link, ref = drive(pkg, (dict(n_streams=3, dim=64), [(0, 2, 1, 0), (2, 0, 2, 300)], frames), "site")
    assert len(ref.table) == 12
    link.close()


# ---------------------------------------------------------------------------------------------------------------- 4. past one workgroup
def test_eight_streams_of_200_entries(pkg):
    """1600 queries against max_queries = 1024: the births spread over two calls; six steady calls; then the lap-limit case, which
    sets error 2 on its stream and leaves the state as the restatement has it."""
    link, ref = drive(pkg, K.big_site(), "big")
    assert ref.err == [0, 0, 2, 0, 0, 0, 0, 0] and len(ref.table) > 1600
    link.close()


# ---------------------------------------------------------------------------------------------------------------- 5. device sources
def test_botsort_handle_read_on_the_device(pkg):
    """Two streams with caller embeddings, 12 frames: process_tracker equals the restatement fed from snapshot(): the tracks with
    flag 2 and tsu 0, each with its feat8."""
    core_cls = import_module(pkg.__name__ + ".tracking.botsort")._BotSortCore
    names = ["stream0", "stream1"]
    inputs = [BR.sequence_inputs(n) for n in names]
    params, dim = inputs[0][0], inputs[0][1]
    S, N = 2, 16
    core = core_cls(n_streams=S, max_tracks=32, max_dets=N, embedder="colorhist", dim=dim, **params)
    link, ref = linker(pkg, S, dim, min_sim_milli=600), R.CrossCamRef(S, dim, min_sim_milli=600)
    n_entries = 0
    for f in range(12):
        xy, cf, cl = np.zeros((S, N, 4), F32), np.zeros((S, N), F32), np.zeros((S, N), np.int32)
        emb, cnt = np.zeros((S, N, dim), np.int8), np.zeros(S, np.int32)
        for s, (_, _, fr) in enumerate(inputs):
            b, c, k, d, _, _ = fr[f]
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
            lists.append((st["ids"][sel], st["cls"][sel], st["feat8"][sel]))
            n_entries += len(sel)
        check_call(link, ref, res, ref.process(lists), ("botsort", f))
    assert n_entries > 20 and len(ref.table) > 0
    other = core_cls(n_streams=S, max_tracks=32, max_dets=N, embedder="colorhist", dim=128, **params)
    with pytest.raises(pkg._ffi.RtmodtError) as e:              # a tracker of another dim
        link.process_tracker(other)
    assert e.value.code == pkg._ffi.E_INVALID and "dim" in str(e.value)
    assert R.snapshots_equal(link.snapshot(), ref.snapshot()) is None
    other.close(); core.close(); link.close()


def test_deepsort_handle_read_on_the_device(pkg):
    """The same on a DeepSORT handle: the confirmed tracks matched this frame, each with the newest row of its gallery ring (the
    ring wraps: nn_budget 6, 12 frames)."""
    core_cls = import_module(pkg.__name__ + ".tracking.deepsort")._DeepSortCore
    params, dim, frames = DR.embedded_inputs("embed64")
    S, N = 2, 8
    core = core_cls(n_streams=S, max_tracks=16, max_dets=N, dim=dim, **params)
    link, ref = linker(pkg, S, dim), R.CrossCamRef(S, dim)
    n_entries = n_events = 0
    for f in range(12):
        xy, cf, cl = np.zeros((S, N, 4), F32), np.zeros((S, N), F32), np.zeros((S, N), np.int32)
        emb, cnt = np.zeros((S, N, dim), np.int8), np.zeros(S, np.int32)
        for s in range(S):                                      # stream 1 sees the same people two frames later
            if f - 2 * s < 0:
                continue
            x, b, c, k, _ = frames[f - 2 * s]
            n = len(b)
            xy[s, :n], cf[s, :n], cl[s, :n], cnt[s], emb[s, :n] = b, c, k, n, DR.quantize_rows(x)
        core.update_batch(xy, cf, cl, cnt, embeddings=emb)
        res = link.process_tracker(core)
        lists = []
        for s in range(S):
            st = core.snapshot(s)
            sel = np.nonzero((st["state"] == 2) & (st["tsu"] == 0))[0]
            lists.append((st["ids"][sel], st["cls"][sel], np.asarray([st["gallery"][i, st["gallery_count"][i] - 1] for i in sel], np.int8).reshape(-1, dim)))
            n_entries += len(sel)
        check_call(link, ref, res, ref.process(lists), ("deepsort", f))
        n_events += len(res.events)
    assert n_entries > 20 and len(ref.ledgers[1]) > 0 and n_events > 0                    # stream 1's tracks found stream 0's identities
    core.close(); link.close()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing(pkg):
    ffi = pkg._ffi
    for kw in (dict(dim=96), dict(n_streams=65), dict(max_identities=4097), dict(max_queries=1025), dict(max_tracks=257), dict(dim=576)):
        with pytest.raises(ffi.RtmodtError) as e:
            linker(pkg, **{**dict(n_streams=2, dim=64), **kw})
        assert e.value.code == ffi.E_INVALID and "crosscam" in str(e.value), kw
    link = linker(pkg, 2, 64)
    link.process([K.entries((1, 0, K.A)), K.EMPTY])
    before = link.snapshot()
    with pytest.raises(ffi.RtmodtError) as e:                   # a local id twice in one list
        link.process([K.entries((4, 0, K.A), (4, 0, K.A2)), K.EMPTY])
    assert e.value.code == ffi.E_INVALID and "twice" in str(e.value)
    with pytest.raises(ffi.RtmodtError) as e:                   # more entries than max_tracks
        link.process([K.entries(*[(i, 0, K.A) for i in range(65)]), K.EMPTY])
    assert e.value.code == ffi.E_INVALID
    with pytest.raises(ffi.RtmodtError) as e:
        link.set_transit(0, 2, 0, 5)
    assert e.value.code == ffi.E_INVALID
    assert R.snapshots_equal(link.snapshot(), before) is None and before["call"] == 1
    bad = dict(before)
    bad["gid"] = before["gid"] + 5                              # a gid past next_gid
    with pytest.raises(ffi.RtmodtError) as e:
        link.load(bad)
    assert e.value.code == ffi.E_INVALID and R.snapshots_equal(link.snapshot(), before) is None
    link.close()


# ---------------------------------------------------------------------------------------------------------------- 7. snapshot / load
def test_load_snapshot_into_a_fresh_handle(pkg):
    frames, _, _ = R.random_site(seed=8, calls=25)
    tr = [(0, 2, 1, 0)]
    a, ref = drive(pkg, (dict(n_streams=3, dim=64), tr, frames[:20]), "before")
    b = linker(pkg, 3, 64)
    for t in tr:
        b.set_transit(*t)
    b.load(a.snapshot())
    assert R.snapshots_equal(b.snapshot(), ref.snapshot()) is None
    assert all(b.global_id(int(l), s) == int(g) for s, led in enumerate(ref.snapshot()["ledgers"]) for l, g, _ in led)
    for c, lists in enumerate(frames[20:]):
        want = ref.process(lists)
        check_call(a, ref, a.process(lists), want, ("uninterrupted", c))
        check_call(b, ref, b.process(lists), want, ("restarted", c))
    a.close(); b.close()
