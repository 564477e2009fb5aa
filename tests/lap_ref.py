"""Shared by the assignment-solver tests: the row / column degree rule by which ``assoc_sparse`` (track_dev.h) and
``mot_accumulate`` (eval.hip) split a bipartite graph into isolated pairs and the "contested" remainder that goes to
``lap_solve``, restated in numpy, and generators of float32 matrices with planted structures (a value above the threshold
is an admissible pair, 0 is not).  Every test asserts its planted counts with :func:`contested` before it runs the GPU,
so a case cannot pass by missing its target."""
import numpy as np

F32 = np.float32
LAP_ROWS, LAP_COLS, LAP_EDGES = 256, 256, 2048


def admissible(iou, thresh):
    """tracker.hip assoc_lap: ``double(float32(1 - iou)) < 1 - thresh``."""
    return (F32(1) - np.asarray(iou, F32)).astype(np.float64) < float(1 - thresh)


def contested(adj):
    """-> (contested row indices, contested column indices, number of contested edges).  A row is contested when it has two
    or more admissible columns, or one whose column has another admissible row; the contested columns and edges are those
    of the contested rows."""
    adj = np.asarray(adj, bool)
    rdeg, cdeg = adj.sum(axis=1), adj.sum(axis=0)
    only = adj.shape[1] - 1 - np.argmax(adj[:, ::-1], axis=1)          # a degree-1 row's column
    hard = (rdeg >= 2) | ((rdeg == 1) & (cdeg[only] != 1))
    return np.nonzero(hard)[0], np.nonzero(adj[hard].any(axis=0))[0], int(rdeg[hard].sum())


def counts(adj):
    r, c, e = contested(adj)
    return len(r), len(c), e


def within_limits(adj):
    r, c, e = counts(adj)
    return r <= LAP_ROWS and c <= LAP_COLS and e <= LAP_EDGES


def generic(rng, shape, lo=0.82, hi=0.999):
    """Generic float32 values above the 0.8 threshold: the optimum of a planted structure is unique."""
    return rng.uniform(lo, hi, size=shape).astype(F32)


def complete(rng, nr, nc):
    return generic(rng, (nr, nc))


def sparse(rng, nr, nc, extra):
    """Row i has column i % nc and `extra` more random ones: every row and column is contested when extra >= 1 (nr >= nc > extra)."""
    a = np.zeros((nr, nc), F32)
    for i in range(nr):
        cols = np.concatenate([[i % nc], rng.choice(np.setdiff1d(np.arange(nc), [i % nc]), size=extra, replace=False)])
        a[i, cols] = generic(rng, len(cols))
    return a


def chain(n, rng=None):
    """n rows, n columns, edges r_i - c_i (about 0.9000) and r_i - c_{i+1} (about 0.9002), the last row's only edge 0.99: rows
    0..n-2 take c_{i+1} first (they are solved in order), and solving the last row re-routes all of them along one augmenting
    path of n rows.  The identity is the only perfect matching and any other matching loses 0.1 - (n - 1) * 0.0002 or more."""
    rng = rng or np.random.default_rng(0)
    a = np.zeros((n, n), F32)
    i = np.arange(n)
    a[i, i] = 0.9000 + rng.uniform(0, 1e-5, n)
    a[i[:-1], i[:-1] + 1] = 0.9002 + rng.uniform(0, 1e-5, n - 1)
    a[n - 1, n - 1] = 0.99
    return a


def chain_evict(n, rng=None):
    """n rows, n - 1 columns.  In units of 1e-4 above the 0.8 threshold: r_0 - c_0 300; r_i - c_{i-1} 501 and r_i - c_i 500; the
    last row's only edge r_{n-1} - c_{n-2} 600.  Rows 0..n-2 take c_i (shifting the rows before gains 202 + i - 1 < 500); the
    last row then shifts every row down one column and evicts row 0 to its dummy (600 + (n - 2) - 300, against 354 - k at most
    for stopping at row k > 0): the solver's to_dummy branch with a path through all n rows.  Jitter is below 0.1 unit."""
    rng = rng or np.random.default_rng(0)
    assert 3 <= n <= 256
    a = np.zeros((n, n - 1), F32)
    i = np.arange(1, n)
    a[i, i - 1] = 0.8501
    a[i[:-1], i[:-1]] = 0.85
    a[0, 0] = 0.83
    a[n - 1, n - 2] = 0.86
    return np.where(a > 0, a + rng.uniform(0, 1e-5, a.shape), 0).astype(F32)


def star(n, rng):
    """n rows on one column, distinct gains."""
    v = (0.82 + 0.17 * (rng.permutation(n) + rng.uniform(0.1, 0.9, n)) / n).astype(F32)
    assert len(np.unique(v)) == n
    return v.reshape(n, 1)


def pairs_of_rows(rng, ncols):
    """2 * ncols rows, ncols columns: every column has two rows of degree 1."""
    a = np.zeros((2 * ncols, ncols), F32)
    a[np.arange(2 * ncols), np.arange(2 * ncols) // 2] = generic(rng, 2 * ncols)
    return a


def embed(rng, block, m, n, rows=None, cols=None, isolated=0):
    """The block at the given (default: random, ascending) rows / columns of an m x n matrix of zeros, plus `isolated` pairs
    on rows and columns of their own."""
    br, bc = block.shape
    free_r, free_c = np.arange(m), np.arange(n)
    rows = np.sort(rng.choice(m, br, replace=False)) if rows is None else np.asarray(rows)
    cols = np.sort(rng.choice(n, bc, replace=False)) if cols is None else np.asarray(cols)
    assert len(rows) == br and len(cols) == bc and len(set(rows.tolist())) == br and len(set(cols.tolist())) == bc
    a = np.zeros((m, n), F32)
    a[np.ix_(rows, cols)] = block
    free_r, free_c = np.setdiff1d(free_r, rows), np.setdiff1d(free_c, cols)
    k = isolated
    assert k <= len(free_r) and k <= len(free_c)
    a[rng.choice(free_r, k, replace=False), rng.choice(free_c, k, replace=False)] = generic(rng, k)
    return a


def check_lists(iou, thresh, res):
    """The four lists are a valid answer: a one-to-one matching over admissible pairs, and the complements."""
    mr, mc, ur, uc = res
    adj = admissible(iou, thresh)
    assert len(mr) == len(mc) and len(set(mr)) == len(mr) and len(set(mc)) == len(mc)
    assert all(adj[r, c] for r, c in zip(mr, mc))
    assert sorted(mr + ur) == list(range(iou.shape[0])) and sorted(mc + uc) == list(range(iou.shape[1]))


def oracle_by_components(assign, iou, thresh):
    """``assign`` (the oracle's assign_lapjv) applied to each connected component of the admissible graph: the optimum of
    a block-diagonal problem is the union of its blocks' optima, exactly, and the oracle's (rows + columns)^2 embedding of
    a 2500 x 2700 matrix takes half a minute.  Rows and columns without an admissible pair stay unmatched."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    iou = np.asarray(iou, F32)
    m, n = iou.shape
    adj = admissible(iou, thresh)
    rr, cc = np.nonzero(adj)
    g = csr_matrix((np.ones(len(rr)), (rr, m + cc)), shape=(m + n, m + n))
    _, lab = connected_components(g, directed=False)
    x = np.full(m, -1, np.int64)
    order = np.argsort(lab, kind="stable")
    bounds = np.flatnonzero(np.diff(lab[order])) + 1
    for comp in np.split(order, bounds):
        rows, cols = comp[comp < m], comp[comp >= m] - m
        if len(rows) == 0 or len(cols) == 0:
            continue
        mr, mc, _, _ = assign(iou[np.ix_(rows, cols)], thresh)
        x[rows[mr]] = cols[mc]
    mr = [int(i) for i in range(m) if x[i] >= 0]
    mc = [int(x[i]) for i in mr]
    used = np.zeros(n, bool)
    used[mc] = True
    return mr, mc, [int(i) for i in range(m) if x[i] < 0], [int(c) for c in np.nonzero(~used)[0]]


# ---------------------------------------------------------------------------------------------------------------------
# CLEAR-MOT frames (eval.hip's own compaction): fast equivalents of eval_ref.assign_lex / max_weight, frames from boxes
# ---------------------------------------------------------------------------------------------------------------------
LEX_W = 1024.0                                                 # > the largest distance sum of a frame: 0.5 * 1024 rows


def assign_lex_scipy(dist, valid):
    """eval_ref.assign_lex by scipy: a valid pair costs d - 1024, every row has a private dummy column of cost 0.  One more
    pair always wins (d <= 0.5, at most 1024 rows a frame: a matching's distances sum to 512 at most), then the smaller sum
    of d.  d - 1024 rounds d to 2^-43, so sums that differ by less than about 1e-10 are not told apart; generic boxes have
    none, and the counts compared exactly depend on the cardinality alone."""
    from scipy.optimize import linear_sum_assignment
    dist, valid = np.asarray(dist, np.float64), np.asarray(valid, bool)
    r, c = valid.shape
    if r == 0 or c == 0 or not valid.any():
        return []
    assert r <= 1024 and dist[valid].max() <= 0.5
    cost = np.full((r, c + r), 1e6)
    cost[:, :c][valid] = dist[valid] - LEX_W
    cost[np.arange(r), c + np.arange(r)] = 0.0
    rows, cols = linear_sum_assignment(cost)
    return [(int(i), int(j)) for i, j in zip(rows, cols) if j < c and valid[i, j]]


def max_weight_scipy(w):
    """eval_ref.max_weight by scipy (integer weights: exact in float64)."""
    from scipy.optimize import linear_sum_assignment
    w = np.asarray(w, np.int64)
    if w.size == 0 or not (w > 0).any():
        return 0
    rows, cols = linear_sum_assignment(w.astype(np.float64), maximize=True)
    return int(w[rows, cols].sum())


def frame_valid(g, h):
    """The valid-pair matrix of one frame's GT and hypothesis rows (``frame, id, x, y, w, h``), in id order."""
    import eval_ref as ER
    g, h = g[np.argsort(g[:, 1], kind="stable")], h[np.argsort(h[:, 1], kind="stable")]
    return np.array([[1.0 - ER.box_iou(a[2:6], b[2:6]) <= 0.5 for b in h] for a in g], bool).reshape(len(g), len(h))


def _rows(frame, first_id, xs, ys, w=100.0, h=40.0):
    return np.array([[frame, first_id + k, x, y, w, h] for k, (x, y) in enumerate(zip(xs, ys))], np.float64).reshape(-1, 6)


def mot_clusters(rng, frame, sizes, pitch=400.0, first_gt=1, first_hyp=1):
    """One cluster per (n_gt, n_hyp) of `sizes`, far apart on a grid; inside a cluster every box is the same 100 x 40 box
    moved by up to 4 px (IoU > 0.8: every GT x hypothesis pair of a cluster is valid, none across clusters)."""
    g, h = [], []
    for k, (ng, nh) in enumerate(sizes):
        cx, cy = pitch * (k % 16), pitch * (k // 16)
        g.append(_rows(frame, first_gt + sum(s[0] for s in sizes[:k]), cx + rng.uniform(-4, 4, ng), cy + rng.uniform(-4, 4, ng)))
        h.append(_rows(frame, first_hyp + sum(s[1] for s in sizes[:k]), cx + rng.uniform(-4, 4, nh), cy + rng.uniform(-4, 4, nh)))
    return np.concatenate(g), np.concatenate(h)


def mot_chain(rng, frame, n, cols=None):
    """GT i at x = 50 i, hypothesis j at x = 50 j - 25 (100 x 40, +-1 px): GT i is valid with hypotheses i and i + 1 only
    (offset 25 +- 2: IoU 0.53 or more; offset 75 -+ 2: 0.16 or less).  `cols` hypotheses (default n: the last GT has one edge)."""
    cols = n if cols is None else cols
    g = _rows(frame, 1, 50.0 * np.arange(n) + rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    h = _rows(frame, 1, 50.0 * np.arange(cols) - 25.0 + rng.uniform(-1, 1, cols), rng.uniform(-1, 1, cols))
    return g, h


def mot_edges(rng, frame, extra):
    """32 GTs x 64 hypotheses of one cluster (2048 valid pairs); hypothesis 64 sits 30 px to the right (IoU 0.54 with every
    GT).  With `extra`, GT 33 sits 62 px to the right: valid with hypothesis 64 alone (IoU 0.52; 0.23 with the others)."""
    g, h = mot_clusters(rng, frame, [(32, 64)])
    h[-1, 2:4] = (30.0, 0.0)
    g[:, 2:4] = rng.uniform(-0.5, 0.5, (32, 2))
    h[:-1, 2:4] = rng.uniform(-0.5, 0.5, (63, 2))
    if extra:
        g = np.concatenate([g, _rows(frame, 33, [62.0], [0.0])])
    return g, h
