"""The call sequence of the ledger modules' workgroup-boundary cases (test_gpu_zones.py, test_gpu_crossing.py, test_gpu_speed.py):
one stream, max_tracks 600, so a ledger of 1200 rows.  Both scans of the merge -- over the list and over the old rows -- end exactly
at, one before and one after a pass of the 256-thread workgroup, in the same call:

    step  0   255 ids                                     255 rows
    step  1   255 new ids                                 255 in the list, 255 idle rows
    step  2   254 of those 510 come back + 2 new ids      256 in the list, 256 idle rows
    step  3   255 of those 512 come back + 2 new ids      257 in the list, 257 idle rows
    step 20   (GAP = 10 steps: every row has expired) 10 of the old ids come back after the gap: fresh rows
    step 21   600 new ids                                 600 + 10 idle
    step 22   590 new ids                                 590 + 610 idle = 1200: exactly full
    step 23   1 new id                                    1 + 1200 idle: the ledger overflows by one row

The ids are drawn at random, so list entries and idle rows interleave everywhere in the merge, and every list comes shuffled.  The
idle counts are worked out here from the ids alone; each test asserts them again on its restatement's own state."""
import numpy as np

MAX_TRACKS = 600
GAP = 10
LAST_STEP = 23


def calls(seed=11):
    """``[(step, ids, idle)]``: the list of a call in the caller's (shuffled) order and the idle rows the ledger keeps beside it."""
    rng = np.random.default_rng(seed)
    pool = [int(v) for v in rng.permutation(20000)[:3000] + 1]
    fresh = iter(pool)
    take = lambda n: [next(fresh) for _ in range(n)]
    pick = lambda ids, n: [ids[i] for i in rng.permutation(len(ids))[:n]]
    last = {}                                                   # id -> the step it was last in a list
    out = []

    def call(step, ids):
        live = set(i for i, s in last.items() if step - s <= GAP)
        for i in list(last):
            if i not in live:
                del last[i]
        ids = [ids[i] for i in rng.permutation(len(ids))]
        out.append((step, ids, len(live - set(ids))))
        for i in ids:
            last[i] = step

    call(0, take(255))
    call(1, take(255))
    call(2, pick(sorted(last), 254) + take(2))
    call(3, pick(sorted(last), 255) + take(2))
    old = sorted(last)
    call(20, pick(old, 10))
    call(21, take(600))
    call(22, take(590))
    call(LAST_STEP, take(1))
    return out


def guards(seq):
    """The sequence does what the docstring says (asserted where the ids are made and again by every test that uses them)."""
    shape = [(step, len(ids), idle) for step, ids, idle in seq]
    assert shape == [(0, 255, 0), (1, 255, 255), (2, 256, 256), (3, 257, 257), (20, 10, 0), (21, 600, 10), (22, 590, 610), (23, 1, 1200)], shape
    seen2, seen3 = set(seq[0][1]) | set(seq[1][1]), set(seq[0][1]) | set(seq[1][1]) | set(seq[2][1])
    assert len(seen2 & set(seq[2][1])) == 254 and len(seen3 & set(seq[3][1])) == 255          # ids return inside the gap
    assert set(seq[4][1]) <= seen3 | set(seq[3][1])                                            # and after it
    assert max(len(ids) for _, ids, _ in seq) <= MAX_TRACKS
