"""CPU: the scenarios of tests/crosscam_limit_cases.py on the restatement alone.  Every test states the conditions under which its
scenario reaches the kernel code it was written for (tests/test_gpu_crosscam_limits.py drives the same scenarios on the kernels), so
that an edit of a generator cannot quietly empty it; and ``CrossCamRef.load`` against an uninterrupted run."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crosscam_limit_cases as LC  # noqa: E402
import crosscam_ref as R  # noqa: E402


@functools.lru_cache(maxsize=None)
def ran(name, dim=64):
    scn = getattr(LC, name)(dim)
    return scn, LC.run_ref(scn)


def clean(ref, outs):
    """Nothing hides behind UNBOUND or DEFERRED (run_ref asserts n_deferred == 0 after every call)."""
    assert ref.err == [0] * ref.S
    assert all(o != R.E_INVALID for o in outs)
    assert not any(st in (R.UNBOUND, R.DEFERRED, R.NONE) for o in outs for s in o["status"] for st in s)


def entry_of(scn, outs, call, stream, lid):
    """-> (gid, status, sim) of the entry with that local id."""
    e = list(scn[3][call][stream][0]).index(lid)
    return outs[call]["gid"][stream][e], outs[call]["status"][stream][e], outs[call]["sim"][stream][e]


# ---------------------------------------------------------------------------------------------------------------- wide
@pytest.mark.parametrize("dim", [128, 192, 512])
def test_wide(dim):
    scn, (ref, outs, before) = ran("wide", dim)
    clean(ref, outs)
    rows = LC.wide_rows(dim)
    assert ref.D == dim and scn[0]["n_streams"] == 3 and all(r.shape[1] == dim for fr in scn[3] for _, _, r in fr)
    assert not rows["TAIL"][:dim - 16].any() and rows["TAIL"][dim - 16:].all()
    assert not rows["MID"][:64].any() and not rows["MID"][80:].any() and rows["MID"][64:80].all()
    for c, s, lid, name, want in LC.WIDE_HAND:
        assert entry_of(scn, outs, c, s, lid)[1] == want, (c, s, lid, name)
    gid = {lid: entry_of(scn, outs, c, s, lid)[0] for c, s, lid, _, want in LC.WIDE_HAND if want == R.BORN}
    assert len(set(gid.values())) == 8                                          # TAIL, MID, M128, P127, X1, X2, Y1, Y2
    for x, y in (("X1", "Y1"), ("X2", "Y2")):                                    # chunk 0 alone would link them; the whole row must not
        assert R.sim_rows(rows[x][:64], R.feat_step(None, rows[y][:64])[1]) == 1000
        assert R.sim_rows(rows[y], R.feat_step(None, rows[x])[1]) < 200
    assert [entry_of(scn, outs, 7, 1, lid)[0] for lid in (9103, 9104, 9105, 9106)] == [gid[9005], gid[9001], gid[9002], gid[9006]]
    assert all(entry_of(scn, outs, 7, 1, lid)[2] >= 900 for lid in (9103, 9104, 9105, 9106))
    # the EMA moved the rows of -128 and of 127 when ALT came, and the bound TAIL2 / MID2 moved theirs
    row = lambda snap, g: snap["s16"][list(snap["gid"]).index(g)].tolist()      # noqa: E731
    for lid in (9003, 9004):
        assert row(before[7], gid[lid]) == row(before[6], gid[lid]) != row(before[8], gid[lid])
    for lid in (9001, 9002):
        assert row(before[6], gid[lid]) != row(before[7], gid[lid])
    assert abs(row(before[6], gid[9003])[0]) == round(R.FEAT_NORM / dim ** 0.5)
    assert len(ref.table) == 12 + 8


# ---------------------------------------------------------------------------------------------------------------- retire_wave
def test_retire_wave():
    scn, (ref, outs, before) = ran("retire_wave")
    clean(ref, outs)
    kw, _, snap, calls = scn
    assert kw["n_streams"] == 2 and kw["max_identities"] == 2048 and kw["max_tracks"] == 256 and kw["bind_age"] < kw["max_age"]
    assert len(snap["gid"]) == 1300 > 1024 and all(700 <= len(l) <= 800 for l in snap["ledgers"])
    assert (np.diff(snap["gid"]) > 0).all() and (np.diff(snap["gid"]) > 1).any()
    gone = np.isin(snap["gid"], [r[0] for r in outs[0]["retired"]])
    assert 0.30 <= gone.mean() <= 0.40 and gone.sum() >= 100
    for part in (gone[:1024], gone[1024:]):                                     # both carries of cc_retire move on both sides of row 1024
        assert part.any() and not part.all()
    assert np.abs(np.diff(gone.astype(int))).sum() > 200                        # irregularly interleaved
    assert [len(o["retired"]) for o in outs] == [406, 138, 122]                 # at least 100 in every call
    snaps = before + [ref.snapshot()]
    assert all(len(l) > 512 for l in snaps[0]["ledgers"]) and all(len(l) > 256 for s in snaps for l in s["ledgers"])
    assert all(sum(map(len, o["status"])) == 320 and len(o["events"]) >= 140 for o in outs)
    every = []
    for k, (out, lists) in enumerate(zip(outs, calls)):
        c = snaps[k]["call"] + 1
        dead = {r[0] for r in out["retired"]}
        for s in range(2):
            old, new = snaps[k]["ledgers"][s], snaps[k + 1]["ledgers"][s]
            at = {int(l): j for j, l in enumerate(old[:, 0])}
            new_at = {int(l): j for j, l in enumerate(new[:, 0])}
            dropped = {j for j, (_, g, t) in enumerate(old.tolist()) if g in dead or c - t > kw["bind_age"]}
            by_age = {j for j, (_, g, t) in enumerate(old.tolist()) if g not in dead and c - t > kw["bind_age"]}
            kept_of = {g: j for j, (_, g, _) in enumerate(old.tolist()) if j not in dropped}
            st, gid, ids = out["status"][s], out["gid"][s], [int(v) for v in lists[s][0]]
            bound = {at[l] for l, x in zip(ids, st) if x == R.BOUND}
            displaced = {kept_of[g] for l, x, g in zip(ids, st, gid) if x == R.LINKED and g in kept_of}
            inserted = {new_at[l] for l, x in zip(ids, st) if x in (R.LINKED, R.JOINED, R.BORN)}
            reused = {at[l] for l, x in zip(ids, st) if x == R.BORN and l in at}
            assert reused <= dropped and not (displaced & bound)
            assert all(int(old[j, 0]) not in new_at for j in displaced)
            every.append([max(v, default=-1) >= 256 for v in (dropped, by_age, displaced, bound, inserted, reused)])
            assert ids != sorted(ids) and st != sorted(st)                      # a mixed entry order
    assert all(every[0]) and all(every[1])                                      # asked of one stream; both have all of it in the first call
    assert all(v[2] and v[3] and v[4] for v in every)                           # ... and a displaced, a bound and a new binding in every call


# ---------------------------------------------------------------------------------------------------------------- join_fan
def test_join_fan():
    scn, p1, p2, cls = LC.join_fan_plan()
    ref, outs, _ = LC.run_ref(scn)
    clean(ref, outs)
    out = outs[0]
    assert scn[0]["max_identities"] == 90 and [len(s) for s in out["status"]] == [100, 100, 100]
    assert out["status"][0] == [R.BORN] * 90 + [R.TABLE_FULL] * 10 and out["gid"][0] == list(range(1, 91)) + [0] * 10
    rows0 = scn[3][0][0][2]
    a, b, c = LC.JF_EQUAL
    assert a < 64 <= b < c < 90 and np.array_equal(rows0[a], rows0[b]) and np.array_equal(rows0[a], rows0[c]) and cls[a] == cls[b] == cls[c]
    assert [p for p in p1 if p in LC.JF_EQUAL] != list(LC.JF_EQUAL)             # gid order is not the order the people come in
    for s, perm, ok in ((1, p1, lambda e: True), (2, p2, lambda e: e % 2 == 0)):
        nxt = iter(LC.JF_EQUAL)
        want = [(next(nxt) if p in LC.JF_EQUAL else p) + 1 if p < 90 and ok(e) else 0 for e, p in enumerate(perm)]
        assert out["gid"][s] == want, s                                         # the equal founders in gid order, lowest first
        assert out["status"][s] == [R.JOINED if g else R.TABLE_FULL for g in want]
        assert any(g - 1 >= 64 for g in want)                                   # a founder past the first 64 births
        assert all(v == 1000 for g, v in zip(want, out["sim"][s]) if g - 1 in LC.JF_EQUAL)
    flat = [st for s in out["status"] for st in s]                              # the query order
    assert flat[flat.index(R.TABLE_FULL):].count(R.JOINED) == flat.count(R.JOINED) > 100
    assert ref.counters["n_table_full"] == flat.count(R.TABLE_FULL) and ref.counters["n_identities"] == 90
    assert all(e[3] == 0 and e[4] == 0 for e in out["events"]) and len(out["events"]) == flat.count(R.JOINED)
    assert all(ref.table[p].last_seen[:2] == [1, 1] for p in LC.JF_EQUAL)


# ---------------------------------------------------------------------------------------------------------------- sixty_four_streams
def test_sixty_four_streams():
    scn, (ref, outs, _) = ran("sixty_four_streams")
    clean(ref, outs)
    kw, transit, _, calls = scn
    assert kw["n_streams"] == 64 and kw["max_tracks"] == 8 and len(calls) == 12 and sorted(transit) == [(0, 63, 1, 3), (63, 0, 1, 3)]
    assert all(len(i) <= 8 for fr in calls for i, _, _ in fr) and {s for fr in calls for s, l in enumerate(fr) if len(l[0])} == set(range(64))
    ev = [e for o in outs for e in o["events"]]                                 # (gid, stream, local id, from_stream, gap, sim)
    assert any(e[1] == 63 and e[3] == 0 and 1 <= e[4] <= 3 for e in ev) and any(e[1] == 0 and e[3] == 63 and 1 <= e[4] <= 3 for e in ev)
    assert not any({e[1], e[3]} == {0, 63} and not 1 <= e[4] <= 3 for e in ev)  # `late` and `both` were not linked across the window
    assert any(e[1] == 63 and e[3] == 62 and e[4] == 0 for e in outs[1]["events"])         # `pair` JOINED into stream 63
    st = lambda c, s: outs[c]["status"][s][-1]                                  # noqa: E731  (the specials are a stream's last entry)
    assert (st(2, 63), st(6, 0), st(3, 0), st(3, 63), st(1, 62), st(1, 63)) == (R.BORN, R.BORN, R.BORN, R.BORN, R.BORN, R.JOINED)
    retired = [r for o in outs for r in o["retired"]]
    masks = [r[3] for r in retired]
    assert any(m >> 63 & 1 for m in masks) and any(m == 1 << 63 for m in masks) and any(m >> 63 & 1 and m & 1 for m in masks)
    assert len(ref.table) == 0 and len(retired) == ref.next_gid - 1 > 40


# ---------------------------------------------------------------------------------------------------------------- CrossCamRef.load
@pytest.mark.parametrize("name,cut", [("retire_wave", 1), ("sixty_four_streams", 5)])
def test_load_equals_the_uninterrupted_run(name, cut):
    (kw, transit, snap, calls), (ref, outs, before) = ran(name)
    ref2 = R.CrossCamRef(**kw)
    for t in transit:
        ref2.set_transit(*t)
    ref2.err = [2] * ref2.S
    ref2.load(before[cut])
    assert ref2.err == [0] * ref2.S and R.snapshots_equal(ref2.snapshot(), before[cut]) is None
    for c in range(cut, len(calls)):
        assert ref2.process(calls[c]) == outs[c], c
        assert R.snapshots_equal(ref2.snapshot(), (before + [ref.snapshot()])[c + 1]) is None, c
    assert ref2.counters == ref.counters and ref2.next_gid == ref.next_gid
    if snap is not None:                                                        # a snapshot built by hand, not taken: load then snapshot gives it back
        ref3 = R.CrossCamRef(**kw)
        ref3.load(snap)
        assert R.snapshots_equal(ref3.snapshot(), snap) is None


# ---------------------------------------------------------------------------------------------------------------- the device source
def test_botsort_streams_bring_entries_at_dim_128():
    """The input of the GPU test of cc_stage at dim 128, on the BoT-SORT restatement: how many entries the linker is handed."""
    import botsort_ref as BR
    params, streams = LC.botsort_streams(128, 8)
    n_entries = 0
    for fr in streams:
        ref = BR.BotSortRef(dim=128, **params)
        assert len(fr) == 8
        for xy, cf, cl, d in fr:
            assert d.shape == (len(xy), 128) and d.dtype == np.int8
            ref.update(xy, cf, cl, d, None)
            st = ref.snapshot()
            n_entries += int(((st["flag"] == 2) & (st["tsu"] == 0)).sum())
    assert n_entries == 24
