"""Scenarios of the cross-camera linker shared by tests/test_crosscam_cpu.py (the restatement against hand-worked literals) and
tests/test_gpu_crosscam.py (the kernels against the restatement): a scenario is ``(kwargs of CrossCamRef, transit settings, calls)``
with ``calls[c][s] = (ids, classes, rows)``.  All rows have 64 values."""
import numpy as np

import crosscam_ref as R

D = 64
A = np.full(D, 100, np.int8)                               # its birth feature is 16 everywhere: sim(A, A) = 1000
A2 = np.asarray([60] * 8 + [100] * 56, np.int8)            # sim(A2, birth of A) = 990
G1 = np.asarray([100] * 32 + [0] * 32, np.int8)
G2 = np.asarray([60] * 32 + [80] * 32, np.int8)            # cos(G1, G2) = 0.6
Q1 = np.asarray([90] * 32 + [-44] * 32, np.int8)           # cos(Q1, G1) = 0.898, cos(Q1, G2) = 0.188


def unit(k, v=100):
    """Rows of distinct k are orthogonal."""
    r = np.zeros(D, np.int8)
    r[4 * k:4 * k + 4] = v
    return r


def entries(*e):
    """(id, class, row), ... -> one stream's list."""
    return ([i for i, _, _ in e], [k for _, k, _ in e], np.asarray([r for _, _, r in e], np.int8).reshape(-1, D))


EMPTY = entries()


def handoff(tmin01=0):
    calls = [[entries((7, 0, A)), EMPTY]] + [[EMPTY, EMPTY]] * 4 + [[EMPTY, entries((3, 0, A))]]
    return dict(n_streams=2, dim=D), ([(0, 1, tmin01, 300)] if tmin01 else []), calls


def overlap(tmin=0):
    return dict(n_streams=2, dim=D), ([(0, 1, tmin, 300)] if tmin else []), [[entries((1, 0, A)), entries((5, 0, A))]]


def near_equal():
    return dict(n_streams=2, dim=D), [], [[entries((1, 0, A)), EMPTY], [EMPTY, entries((10, 0, A2), (11, 0, A))]]


def greedy_loses():
    return dict(n_streams=2, dim=D, min_sim_milli=400), [], [[entries((1, 0, G1), (2, 0, G2)), EMPTY], [EMPTY, entries((20, 0, G1), (21, 0, Q1))]]


def fragment():
    return dict(n_streams=1, dim=D), [], [[entries((7, 0, A))], [entries((9, 0, A))], [entries((7, 0, A), (9, 0, A))]]


def retirement():
    return dict(n_streams=1, dim=D, max_age=3), [], [[entries((1, 0, A))]] + [[EMPTY]] * 4 + [[entries((2, 0, A))]]


def full_table():
    return dict(n_streams=1, dim=D, max_identities=2), [], [[entries((1, 0, unit(0)), (2, 0, unit(1)), (3, 0, unit(2)))]]


def deferral():
    c = [entries((1, 0, A), (2, 0, unit(3))), entries((5, 0, A))]
    return dict(n_streams=2, dim=D, max_queries=2), [], [c, c]


def lap_limit():
    """50 queries x 50 identities of one row: 2500 contested pairs."""
    first = entries(*[(i + 1, 0, A) for i in range(50)])
    second = entries(*[(i + 101, 0, A) for i in range(50)])
    return dict(n_streams=2, dim=D, max_identities=256), [], [[first, EMPTY], [first, second], [first, second]]


def mixed():
    """Classes, a zero row, a bound entry whose row is zero, match_class, a restricted pair, two streams linking one identity."""
    z = np.zeros(D, np.int8)
    calls = [
        [entries((1, 0, A), (2, 1, unit(1)), (3, 0, z)), EMPTY, EMPTY],
        [entries((1, 0, z), (2, 1, unit(1))), entries((4, 1, A), (5, 1, unit(1))), entries((6, 0, A))],
        [EMPTY, entries((4, 1, A), (7, 0, A)), entries((6, 0, A2), (8, 1, unit(1, 90)))],
        [entries((3, 0, unit(5))), entries((9, 0, unit(5))), entries((8, 1, unit(1)))],
    ]
    return dict(n_streams=3, dim=D, max_age=50, bind_age=2), [(0, 2, 0, -1), (1, 2, 1, 50)], calls


HAND = dict(handoff=handoff, handoff_blocked=lambda: handoff(6), overlap=overlap, overlap_disjoint=lambda: overlap(1), near_equal=near_equal,
            greedy_loses=greedy_loses, fragment=fragment, retirement=retirement, full_table=full_table, deferral=deferral, lap_limit=lap_limit, mixed=mixed)


def run_ref(scn):
    """-> (the restatement after the last call, the outputs of every call)."""
    kw, transit, calls = scn
    ref = R.CrossCamRef(**kw)
    for t in transit:
        ref.set_transit(*t)
    return ref, [ref.process(c) for c in calls]


def big_site(seed=11, n_streams=8, n=200, calls=8):
    """GPU case 4: 8 streams x 200 entries, dim 64.  Every entry is a person of its own (a random sign pattern), so the first call
    brings 1600 queries; afterwards a few per cent of every stream's tracks are replaced each call, by new people or by people another camera sees too; the two last calls are the lap-limit case."""
    rng = np.random.default_rng(seed)
    new_row = lambda: (rng.integers(0, 2, D) * 200 - 100).astype(np.int8)                                   # noqa: E731
    cur = [[(i + 1, 0, new_row()) for i in range(n)] for _ in range(n_streams)]
    nxt = [n + 1] * n_streams
    out = []
    for c in range(calls):
        if c >= 2:
            for s in range(n_streams):
                for j, k in enumerate(rng.choice(n, 5, replace=False)):          # three new people, two seen by another camera as well
                    other = cur[(s + 1 + int(rng.integers(0, n_streams - 1))) % n_streams]
                    cur[s][int(k)] = (nxt[s], 0, new_row() if j < 3 else other[int(rng.integers(0, n))][2])
                    nxt[s] += 1
        out.append([entries(*[(i, k, R.noisy(r, rng, 6)) for i, k, r in cur[s]]) for s in range(n_streams)])
    # the lap-limit case: 50 tracks of one row are born in stream 1, then 50 more of that row appear in stream 2 (2500 contested pairs)
    x = new_row()
    for s in (1, 2):
        cur[s] = cur[s] + [(nxt[s] + i, 0, x) for i in range(50)]
        out.append([entries(*cur[t]) for t in range(n_streams)])
    return dict(n_streams=n_streams, dim=D, max_tracks=n + 50, max_identities=4096, max_queries=1024), [], out
