"""GPU: ``assoc_sparse<double>`` (track_dev.h) -- the compaction of the contested rows, columns and edges into the fixed LDS
arrays of lap.h (256 / 256 / 2048) and the exact solve -- through ``rtmodt_assign_lapjv`` on planted matrices, at each limit
and one past it, beyond the first 1024-thread pass, at every lane-group width, in large components and at other thresholds;
then the tracker's lapjv branch over sequences whose frames do reach the solver.  The reference is the oracle's assign_lapjv
(scipy on lap's extended matrix); planted values are generic, so the optimum is unique and the four lists are equal."""
import numpy as np
import pytest

import lap_ref as LR
from oracle import tracker_oracle as T
from test_gpu_tracker import contested_boxes, gain

pytestmark = pytest.mark.gpu
TH = 0.8


def planted(iou, thresh=TH):
    return LR.counts(LR.admissible(iou, thresh))


def equal_to_oracle(pkg, iou, thresh=TH, ref=None):
    ref = T.assign_lapjv(iou, thresh) if ref is None else ref
    got = pkg._ffi.assign_lapjv(iou, thresh)
    LR.check_lists(iou, thresh, got)
    assert got == ref, (len(got[0]), len(ref[0]), gain(iou, got[0], got[1], thresh) - gain(iou, ref[0], ref[1], thresh))


def refused(pkg, iou, thresh=TH):
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        pkg._ffi.assign_lapjv(iou, thresh)
    assert e.value.code == pkg._ffi.E_CAPACITY
    ok = LR.embed(np.random.default_rng(1), LR.complete(np.random.default_rng(2), 5, 4), 20, 20, isolated=6)
    equal_to_oracle(pkg, ok)                                   # the device still answers a valid call


def limit_cases():
    rng = np.random.default_rng(256)
    rows256 = LR.embed(rng, LR.pairs_of_rows(rng, 128), 300, 300, isolated=30)       # 128 columns with two degree-1 rows each
    col = int(LR.contested(LR.admissible(rows256, TH))[1][5])
    free = int(np.flatnonzero(rows256.sum(axis=1) == 0)[0])
    rows257 = rows256.copy()
    rows257[free, col] = 0.9                                   # a third row on one of those columns
    blk = np.zeros((128, 256), np.float32)                     # 128 rows of degree 2 on disjoint column pairs
    blk[np.repeat(np.arange(128), 2), np.arange(256)] = LR.generic(rng, 256)
    cols256 = LR.embed(rng, blk, 300, 300, isolated=30)
    r = int(LR.contested(LR.admissible(cols256, TH))[0][7])
    freec = int(np.flatnonzero(cols256.sum(axis=0) == 0)[0])
    cols257 = cols256.copy()
    cols257[r, freec] = 0.9                                    # one row gets a third column
    edges2048 = LR.embed(rng, LR.complete(rng, 32, 64), 100, 100, isolated=20)
    col = int(LR.contested(LR.admissible(edges2048, TH))[1][3])
    free = int(np.flatnonzero(edges2048.sum(axis=1) == 0)[0])
    edges2049 = edges2048.copy()
    edges2049[free, col] = 0.9                                 # one more row with a single edge into a contested column
    return {"rows256": (rows256, (256, 128, 256), True), "rows257": (rows257, (257, 128, 257), False),
            "cols256": (cols256, (128, 256, 256), True), "cols257": (cols257, (128, 257, 257), False),
            "edges2048": (edges2048, (32, 64, 2048), True), "edges2049": (edges2049, (33, 64, 2049), False),
            # two limits at once
            "rows256_edges2048": (LR.embed(rng, LR.complete(rng, 256, 8), 300, 40, isolated=10), (256, 8, 2048), True),
            "rows256_cols256": (LR.embed(rng, LR.chain(256, rng), 300, 300, isolated=30), (256, 256, 511), True)}


@pytest.mark.parametrize("case", ["rows256", "rows257", "cols256", "cols257", "edges2048", "edges2049", "rows256_edges2048", "rows256_cols256"])
def test_each_limit_and_one_past_it(pkg, case):
    iou, want, fits = limit_cases()[case]
    assert planted(iou) == want
    if fits:
        equal_to_oracle(pkg, iou)
    else:
        refused(pkg, iou)


def test_contested_rows_beyond_the_first_thread_pass(pkg):
    """2500 x 2700 with 2000 isolated pairs; 240 contested rows and columns in runs across 1023/1024 and 2047/2048 (both
    compaction scans advance 1024 indices per pass and carry the running count into the next)."""
    rng = np.random.default_rng(1024)
    m, n = 2500, 2700
    rows = np.concatenate([np.arange(3, 43), np.arange(984, 1064), np.arange(2008, 2088), np.arange(2455, 2495)])
    cols = np.concatenate([np.arange(990, 1070), np.arange(2000, 2100), np.arange(2640, 2700)])
    assert len(rows) == 240 and len(cols) == 240
    iou = LR.embed(rng, LR.sparse(rng, 240, 240, 2), m, n, rows=rows, cols=cols[rng.permutation(240)], isolated=2000)
    cr, cc, ce = LR.contested(LR.admissible(iou, TH))
    assert np.array_equal(cr, rows) and np.array_equal(cc, np.sort(cols)) and ce == 720
    for edge in (1024, 2048):
        assert (cr < edge).any() and (cr >= edge).any() and (cc < edge).any() and (cc >= edge).any()
        assert edge - 1 in cr and edge in cr and edge - 1 in cc and edge in cc
    equal_to_oracle(pkg, iou, ref=LR.oracle_by_components(T.assign_lapjv, iou, TH))


def width_matrix(rng, m, n):
    """A block on up to 6 rows x 6 columns that include the first and last index, its first row and column full (contested
    unless the matrix is 1 x 1), and isolated pairs elsewhere."""
    br, bc = min(m, 6), min(n, 6)
    rows = np.unique(np.concatenate([[0, m - 1], rng.choice(m, br, replace=False)]))[:br] if m > 1 else np.array([0])
    cols = np.unique(np.concatenate([[0, n - 1], rng.choice(n, bc, replace=False)]))[:bc] if n > 1 else np.array([0])
    if m > 1 and m - 1 not in rows:
        rows[-1] = m - 1
    if n > 1 and n - 1 not in cols:
        cols[-1] = n - 1
    blk = np.where(rng.random((len(rows), len(cols))) < 0.5, LR.generic(rng, (len(rows), len(cols))), 0).astype(np.float32)
    blk[0, :] = LR.generic(rng, len(cols))
    blk[:, 0] = LR.generic(rng, len(rows))
    return LR.embed(rng, blk, m, n, rows=rows, cols=cols, isolated=min(m - len(rows), n - len(cols), 12))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("m", [1, 16, 17, 32, 33, 1024, 1025])
def test_group_width_switch_points(pkg, m, n):
    """The degree scan gives each row a group of R lanes: R halves while m * R > 1024 or R / 2 >= n."""
    iou = width_matrix(np.random.default_rng(1000 * m + n), m, n)
    nr, nc, ne = planted(iou)
    assert iou.shape == (m, n) and ((m, n) == (1, 1) or (nr >= 1 and nc >= 1 and ne >= 2))
    equal_to_oracle(pkg, iou)


@pytest.mark.parametrize("case", ["chain256", "chain256_evict", "star256", "star256_transposed", "complete45", "complete256x8"])
def test_large_components(pkg, case):
    rng = np.random.default_rng(45)
    blk, want = {"chain256": lambda: (LR.chain(256, rng), (256, 256, 511)),
                 "chain256_evict": lambda: (LR.chain_evict(256, rng), (256, 255, 510)),
                 "star256": lambda: (LR.star(256, rng), (256, 1, 256)),
                 "star256_transposed": lambda: (LR.star(256, rng).T.copy(), (1, 256, 256)),
                 "complete45": lambda: (LR.complete(rng, 45, 45), (45, 45, 2025)),
                 "complete256x8": lambda: (LR.complete(rng, 256, 8), (256, 8, 2048))}[case]()
    iou = LR.embed(rng, blk, blk.shape[0] + 40, blk.shape[1] + 50, isolated=25)
    assert planted(iou) == want
    ref = T.assign_lapjv(iou, TH)
    pos = {int(r): k for k, r in enumerate(LR.contested(LR.admissible(iou, TH))[0])}
    pc = {int(c): k for k, c in enumerate(LR.contested(LR.admissible(iou, TH))[1])}
    x = {pos[r]: pc[c] for r, c in zip(ref[0], ref[1]) if r in pos}
    if case == "chain256":                                     # the planted optimum: the chain re-routed / its first row evicted
        assert x == {i: i for i in range(256)}
    if case == "chain256_evict":
        assert x == {i: i - 1 for i in range(1, 256)}
    equal_to_oracle(pkg, iou, ref=ref)


def test_all_equal_gains_same_total(pkg):
    """Ties on purpose: every optimum has the same gain; the lists may differ, the total and the validity may not."""
    rng = np.random.default_rng(9)
    for blk in (np.full((45, 45), 0.9, np.float32), np.where(LR.chain(256) > 0, np.float32(0.9), np.float32(0))):
        iou = LR.embed(rng, blk, blk.shape[0] + 10, blk.shape[1] + 10, isolated=5)
        ref = T.assign_lapjv(iou, TH)
        got = pkg._ffi.assign_lapjv(iou, TH)
        LR.check_lists(iou, TH, got)
        assert len(got[0]) == len(ref[0])
        assert abs(gain(iou, got[0], got[1], TH) - gain(iou, ref[0], ref[1], TH)) < 1e-12


BOX_N = 150                                                    # found on the CPU: 131 / 227 / 498 contested at 0.5, 144 / 240 / 844 at 0.3


@pytest.mark.parametrize("thresh", [0.5, 0.3])
def test_other_thresholds_on_box_matrices(pkg, thresh):
    t, d = contested_boxes(np.random.default_rng(11), BOX_N)
    iou = T.batch_iou(t, d)
    nr, nc, ne = planted(iou, thresh)
    assert nr >= 100 and nr <= LR.LAP_ROWS and nc <= LR.LAP_COLS and ne <= LR.LAP_EDGES, (nr, nc, ne)
    ref = T.assign_lapjv(iou, thresh)
    got = pkg._ffi.assign_lapjv(iou, thresh)
    LR.check_lists(iou, thresh, got)
    assert abs(gain(iou, got[0], got[1], thresh) - gain(iou, ref[0], ref[1], thresh)) < 1e-12
    assert got == ref


@pytest.mark.parametrize("thresh,floor", [(0.5, 50), (0.3, 100)])
def test_tracker_sequences_where_the_solver_works(pkg, thresh, floor):
    """_ByteTrackCore's lapjv branch against the oracle, digest by digest, at thresholds where the frames' own track x
    detection matrices put up to 81 rows / 191 pairs (0.5) and 137 rows / 515 pairs (0.3) through the exact solver (the
    oracle's counts for this seed, well clear of the floors asserted), all within the limits."""
    core = pkg.tracking.tracker._ByteTrackCore(assign_mode=pkg._ffi.ASSIGN_LAPJV, match_thresh=thresh)
    ora = T.TrackerOracle(assign="lapjv", match_thresh=thresh)
    inner, seen = ora._assign, []

    def recording(iou, th):
        seen.append(planted(iou, th))
        return inner(iou, th)
    ora._assign = recording
    xy, cf, cl = pkg.synth.box_sequence(200, 640, 30, 21)
    for f in range(30):
        ora.update(xy[f], cf, cl)
        top = np.array(seen + [(0, 0, 0)]).max(axis=0)         # the oracle's matrices are the kernel's while the states agree
        assert top[0] <= LR.LAP_ROWS and top[1] <= LR.LAP_COLS and top[2] <= LR.LAP_EDGES, (f, top)
        core.update(xy[f], cf, cl)
        assert np.array_equal(T.state_digest(core.snapshot()), T.state_digest(ora.snapshot())), f"frame {f}"
    assert top[0] >= floor, top
    core.close()
