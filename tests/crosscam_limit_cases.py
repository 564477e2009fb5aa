"""Scenarios of the cross-camera linker at its limits, shared by tests/test_crosscam_cases_cpu.py (the restatement alone: does every
scenario reach the code it is meant for?) and tests/test_gpu_crosscam_limits.py (the kernels against the restatement).  A scenario
is ``(kwargs of CrossCamRef, transit settings, snapshot to load or None, calls)`` with ``calls[c][s] = (ids, classes, rows)``.  Every
builder is deterministic and takes ``dim``.
  wide                 dim above 64: the k-chunk loops, the D / 8 and D / 16 copies, rows that are zero in chunk 0
  retire_wave          a loaded table past 1024 rows and ledgers past 512 bindings, a third of which leave in one call
  join_fan             more than 64 births in one call, equal founders, JOIN while the table is full
  sixty_four_streams   the stream limit: bit 63 of every stream mask, transit windows between streams 63 and 0"""
import numpy as np

import crosscam_ref as R


def entries(dim, *e):
    """(id, class, row), ... -> one stream's list."""
    return ([i for i, _, _ in e], [k for _, k, _ in e], np.asarray([r for _, _, r in e], np.int8).reshape(-1, dim))


def run_ref(scn):
    """-> (the restatement after the last call, the outputs of every call, the snapshot before every call)."""
    kw, transit, snap, calls = scn
    ref = R.CrossCamRef(**kw)
    for t in transit:
        ref.set_transit(*t)
    if snap is not None:
        ref.load(snap)
    outs, before = [], []
    for c in calls:
        before.append(ref.snapshot())
        outs.append(ref.process(c))
        assert ref.counters["n_deferred"] == 0
    return ref, outs, before


# ---------------------------------------------------------------------------------------------------------------- wide
def wide_rows(dim):
    """The hand rows by name.  TAIL / MID are zero in chunk 0 (MID in all but bytes 64..79, TAIL in all but the last 16); the X / Y
    of a pair are equal in chunk 0 and orthogonal in the rest, and the signs alternate so that every dot with a constant row is 0;
    the chunk-0 patterns of the two pairs are orthogonal to each other."""
    assert dim >= 128 and dim % 64 == 0
    z = lambda: np.zeros(dim, np.int32)                                                                      # noqa: E731
    alt, alt2 = np.where(np.arange(dim) % 2 == 0, 1, -1), np.where(np.arange(dim) % 4 < 2, 1, -1)
    rest, half = dim - 64, (dim - 64) // 2
    r = dict(ZERO=z(), M128=z() - 128, P127=z() + 127, ALT=np.where(np.arange(dim) % 2 == 0, -128, 127))
    r["TAIL"], r["TAIL2"], r["MID"], r["MID2"] = z(), z(), z(), z()
    r["TAIL"][dim - 16:] = 100
    r["TAIL2"][dim - 16:] = [100] * 8 + [50] * 8
    r["MID"][64:80] = 100
    r["MID2"][64:80] = [50] * 8 + [100] * 8
    for name, sign in (("1", alt), ("2", alt2)):
        x, y = z(), z()
        x[:64], y[:64] = 30, 30
        x[64:64 + half], y[64 + half:64 + rest] = 120, 120
        r["X" + name], r["Y" + name] = x * sign, y * sign
    return {k: v.astype(np.int8) for k, v in r.items()}


# (call, stream, local id, row, the status intended); all of class 1, the people of random_site are of class 0
WIDE_HAND = [
    (5, 0, 9001, "TAIL", R.BORN), (5, 0, 9002, "MID", R.BORN), (5, 0, 9003, "M128", R.BORN), (5, 0, 9004, "P127", R.BORN),
    (5, 0, 9005, "X1", R.BORN), (5, 0, 9007, "ZERO", R.NO_DESCRIPTOR),
    (6, 0, 9001, "TAIL2", R.BOUND), (6, 0, 9002, "MID2", R.BOUND), (6, 0, 9003, "M128", R.BOUND), (6, 0, 9004, "P127", R.BOUND),
    (6, 0, 9006, "X2", R.BORN), (6, 1, 9101, "Y1", R.BORN), (6, 1, 9102, "Y2", R.BORN),
    (7, 0, 9003, "ALT", R.BOUND), (7, 0, 9004, "ALT", R.BOUND), (7, 0, 9001, "ZERO", R.BOUND),
    (7, 1, 9103, "X1", R.LINKED), (7, 1, 9104, "TAIL", R.LINKED), (7, 1, 9105, "MID", R.LINKED), (7, 1, 9106, "X2", R.LINKED),
]


def wide(dim):
    """3 streams: the frames of random_site(dim=dim) under the transit of GPU case 3, with WIDE_HAND appended to calls 5..7."""
    frames, _, _ = R.random_site(dim=dim)
    rows = wide_rows(dim)
    calls = [[(list(i), list(k), np.asarray(r, np.int8)) for i, k, r in fr] for fr in frames]
    for c, s, lid, name, _ in WIDE_HAND:
        i, k, r = calls[c][s]
        assert lid not in i
        calls[c][s] = (i + [lid], k + [1], np.concatenate([r, rows[name][None, :]]))
    return dict(n_streams=3, dim=dim), [(0, 2, 1, 0), (2, 0, 2, 300)], None, calls


# ---------------------------------------------------------------------------------------------------------------- retire_wave
RW_CALL, RW_MAX_AGE, RW_BIND_AGE, RW_N = 100, 40, 25, 1300


def retire_wave(dim=64, seed=21):
    """2 streams.  A snapshot of 1300 identities at call 100 with 790 / 770 bindings, then three calls.  An identity whose greatest
    last_seen is 60 or less leaves in the first call (about a third, at random rows), 61 in the second, 62 in the third; a binding
    last sighted before call 76 is past bind_age 25.  Every call shows, per stream and in a shuffled order: 50 bound tracks (40 of
    them from ledger index 256 up), 45 table people whose binding is absent, under a fresh local id (the LINK displaces the binding),
    25 table people the stream holds no binding of, 40 new people (10 of them under a local id whose binding is dropped in this very
    call, the others under ids between old ones), and in stream 1 five of stream 0's new people once more (JOINED)."""
    rng = np.random.default_rng(seed)
    n, S, C0 = RW_N, 2, RW_CALL
    kw = dict(n_streams=S, dim=dim, max_tracks=256, max_identities=2048, max_queries=256, max_age=RW_MAX_AGE, bind_age=RW_BIND_AGE)
    base = R.person_rows(n, dim, seed + 1)
    feats = [R.feat_step(None, row) for row in base]
    gid = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
    u = rng.random(n)
    top = np.where(u < 0.32, rng.integers(45, 61, n), np.where(u < 0.44, 61, np.where(u < 0.54, 62, np.where(u < 0.62, rng.integers(63, 78, n),
                                                                                                         rng.integers(78, C0 + 1, n)))))
    where = rng.integers(0, 10, n)                                             # 0..2 stream 0 alone, 3..5 stream 1 alone, else both
    last = np.zeros((n, S), np.int64)
    for i in range(n):
        a = 0 if where[i] < 3 else (1 if where[i] < 6 else int(rng.integers(0, 2)))
        last[i, a] = top[i]
        if where[i] >= 6:
            last[i, 1 - a] = top[i] - int(rng.integers(0, 12))
    first = np.asarray([int(rng.integers(1, min(v for v in last[i] if v > 0) + 1)) for i in range(n)], np.int64)
    ledgers = []
    for s, nb in enumerate((790, 770)):
        who = rng.permutation(np.nonzero(last[:, s] > 0)[0])[:nb]
        lids = np.cumsum(rng.integers(2, 5, nb)).astype(np.int64) + 10
        ledgers.append(np.stack([lids, gid[who], last[who, s]], 1).astype(np.int64).reshape(-1, 3))
    snap = dict(call=C0, next_gid=int(gid[-1]) + 5, gid=gid, cls=np.zeros(n, np.int32), first_seen=first, last_seen=last,
                s16=np.asarray([f[0] for f in feats], np.int16), s8=np.asarray([f[1] for f in feats], np.int8), ledgers=ledgers)
    # the calls, generated along the restatement's state
    ref = R.CrossCamRef(**kw)
    ref.load(snap)
    row_of = {int(g): base[i] for i, g in enumerate(gid)}
    calls, n_new = [], 0
    for k in range(3):
        c = ref.c + 1
        alive = {g.gid: g for g in ref.table if c - max(g.last_seen) <= RW_MAX_AGE}
        lists, shared = [], []
        for s in range(S):
            led = sorted(ref.ledgers[s].items())                                # (lid, [gid, last]) in ledger order
            keeps = [(j, lid, b[0]) for j, (lid, b) in enumerate(led) if b[0] in alive and c - b[1] <= RW_BIND_AGE]
            drops = [(j, lid) for j, (lid, b) in enumerate(led) if not (b[0] in alive and c - b[1] <= RW_BIND_AGE)]
            hi, lo = [x for x in keeps if x[0] >= 256], [x for x in keeps if x[0] < 256]
            pick = lambda pool, m: [pool[int(t)] for t in rng.permutation(len(pool))[:m]]                   # noqa: E731
            ent = []
            bound = pick(hi, 40) + pick(lo, 10)
            ent += [(lid, 0, R.noisy(row_of[g], rng, 6)) for _, lid, g in bound]
            shown = {g for _, _, g in bound}
            absent = [x for x in hi if x[2] not in shown]
            used = {lid for lid, _ in led}
            between = [lid + 1 for lid, _ in led if lid + 1 not in used]
            fresh = iter(pick(between, 45 + 25 + 40))
            displaced = pick(absent, 45)
            ent += [(next(fresh), 0, R.noisy(row_of[g], rng, 6)) for _, _, g in displaced]
            shown |= {g for _, _, g in displaced}
            held = {b[0] for _, b in led}
            others = [g for g in alive if g not in held and g in row_of and alive[g].last_seen[s] == 0]
            ent += [(next(fresh), 0, R.noisy(row_of[g], rng, 6)) for g in pick(others, 25)]
            reuse = [lid for _, lid in pick([d for d in drops if d[0] >= 256], 10)]
            for t in range(40):
                if s == 1 and t < 5:
                    row = R.noisy(shared[t], rng, 6)
                else:
                    row = R.person_rows(1, dim, 7000 + n_new)[0]
                    n_new += 1
                    if s == 0 and len(shared) < 5:
                        shared.append(row)
                ent.append((reuse[t] if t < len(reuse) else next(fresh), 0, row))
            order = rng.permutation(len(ent))
            lists.append(entries(dim, *[ent[int(t)] for t in order]))
        calls.append(lists)
        out = ref.process(lists)
        assert out != R.E_INVALID
        for s in range(S):                                                     # the people born in this call can be bound or linked later
            for lid, g, row in zip(lists[s][0], out["gid"][s], lists[s][2]):
                if g and g not in row_of:
                    row_of[g] = row
    return kw, [], snap, calls


# ---------------------------------------------------------------------------------------------------------------- join_fan
JF_EQUAL = (10, 70, 80)                                    # stream 0's entries of one row: the founders at these birth positions


def join_fan_plan(dim=64, seed=31):
    """-> (the scenario, stream 1's and stream 2's person per entry, every person's class).

    3 streams x 100 entries, one call, a table of 90.  Stream 0: 100 people of class (entry % 2), three of them (JF_EQUAL, all of
    class 0) with one row: 90 BORN, 10 TABLE_FULL.  Stream 1: the same people permuted, each with its class: JOINED to a founder at any
    birth position while the table is full; the three equal rows join the three equal founders in gid order.  Stream 2: the people
    permuted again, every odd entry with the other class; 0 -> 2 is closed for overlap, so it joins through stream 1 alone."""
    rng = np.random.default_rng(seed)
    n = 100
    base = R.person_rows(n, dim, seed + 1)
    for p in JF_EQUAL[1:]:
        base[p] = base[JF_EQUAL[0]]
    cls = [p % 2 for p in range(n)]
    row = lambda p: base[p] if p in JF_EQUAL else R.noisy(base[p], rng, 6)                                   # noqa: E731
    p1, p2 = rng.permutation(n), rng.permutation(n)
    s0 = entries(dim, *[(p + 1, cls[p], base[p]) for p in range(n)])
    s1 = entries(dim, *[(200 + e, cls[int(p)], row(int(p))) for e, p in enumerate(p1)])
    s2 = entries(dim, *[(400 + e, cls[int(p)] ^ (e & 1), row(int(p))) for e, p in enumerate(p2)])
    kw = dict(n_streams=3, dim=dim, max_tracks=n, max_identities=90, max_queries=512)
    return (kw, [(0, 2, 1, 300)], None, [[s0, s1, s2]]), p1.tolist(), p2.tolist(), cls


def join_fan(dim=64):
    return join_fan_plan(dim)[0]


# ---------------------------------------------------------------------------------------------------------------- sixty_four_streams
def sixty_four_streams(dim=64, seed=41):
    """64 streams x at most 8 entries, 12 calls, max_age 4; 63 -> 0 and 0 -> 63 take 1..3 calls.  A walker is in one stream per call
    and steps to the next (or the previous) stream every call, each time under a fresh local id: walkers cross 63 -> 0 and 0 -> 63
    inside the window; `late` is in 63 at call 2 and in 0 at call 6 (4 calls: past the window, born again), `both` is in 63 and 0
    in one call (0 calls: below the window, two identities), `pair` is in 62 and 63 in one call (JOINED into 63); everybody is gone
    by call 7 and retires before the last call."""
    rng = np.random.default_rng(seed)
    S, n_calls = 64, 12
    walkers = [(61, +1, 0, 7), (2, -1, 0, 7), (63, +1, 1, 5), (0, -1, 1, 5), (60, +1, 2, 7), (5, -1, 0, 6)]
    walkers += [(s, int(rng.choice([-1, 1])), int(rng.integers(0, 3)), int(rng.integers(4, 8))) for s in range(S) if s not in (61, 2, 63, 0, 60, 5)]
    base = R.person_rows(len(walkers) + 3, dim, seed + 1)
    late, both, pair = base[-3], base[-2], base[-1]
    next_id = [1] * S
    calls = []
    for c in range(n_calls):
        ent = [[] for _ in range(S)]

        def show(s, row, k=0):
            if len(ent[s]) < 8:
                ent[s].append((next_id[s], k, R.noisy(row, rng, 6)))
                next_id[s] += 1
        for w, (s0, d, t0, t1) in enumerate(walkers):
            if t0 <= c < t1:
                show((s0 + d * (c - t0)) % S, base[w], w % 2)
        if c == 2:
            show(63, late)
        if c == 6:
            show(0, late)
        if c == 3:
            show(63, both)
            show(0, both)
        if c == 1:
            show(62, pair)
            show(63, pair)
        calls.append([entries(dim, *e) for e in ent])
    kw = dict(n_streams=S, dim=dim, max_tracks=8, max_identities=256, max_queries=256, max_age=4)
    return kw, [(63, 0, 1, 3), (0, 63, 1, 3)], None, calls


# ---------------------------------------------------------------------------------------------------------------- a device source
def botsort_streams(dim=128, n_frames=8):
    """-> (tracker parameters, per stream the frames (xyxy, conf, cls, int8 rows of dim values)): the boxes of botsort_ref's stream0
    and stream1 with caller embeddings of `dim` values."""
    import botsort_ref as BR
    params = BR.SEQUENCES["stream0"][0]
    out = []
    for k in range(2):
        scene = BR._stream(k)[:n_frames]
        desc = BR.object_descriptors(scene, dim, seed=600 + k)
        out.append([(f[0], f[1], f[2], d) for f, d in zip(scene, desc)])
    return params, out
