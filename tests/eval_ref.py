"""NumPy restatement of the evaluation rules, written loop by loop as the rules read, for the
tests of ``rtmodt_amd.evaluation``.  Plain Python / NumPy only; slow by design.

* ``coco_ref``      -- COCO bbox evaluate + accumulate (pycocotools >= 2.0.7 rules): precision[T,R,K,A,M], recall[T,K,A,M]
* ``mot_ref``       -- CLEAR MOT + IDF1 counts of one sequence (motmetrics >= 1.4.0 rules, 'iou' distance, 0.5)
* ``assign_lex``    -- the exact "maximum cardinality, then minimum sum of d" assignment (Hungarian method on
                       lexicographic costs), used per frame by ``mot_ref``
* ``max_weight``    -- exact maximum-weight bipartite matching of integer weights (IDTP)
"""
from __future__ import annotations

import numpy as np

# the parameters as the rules state them
IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
FP, TP, IGN = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# COCO (rules §1)
# ---------------------------------------------------------------------------------------------------------------------
def iou_rows(db, gb, crowd):
    """IoU of every detection (rows) with every GT (columns), boxes x, y, w, h, float64: the overlap width / height are
    min(right) - max(left), zero when <= 0; the union is the detection's box area for a crowd GT, else
    (det area + GT area) - intersection."""
    db = np.asarray(db, np.float64).reshape(-1, 1, 4)
    gb = np.asarray(gb, np.float64).reshape(1, -1, 4)
    w = np.minimum(db[..., 0] + db[..., 2], gb[..., 0] + gb[..., 2]) - np.maximum(db[..., 0], gb[..., 0])
    h = np.minimum(db[..., 1] + db[..., 3], gb[..., 1] + gb[..., 3]) - np.maximum(db[..., 1], gb[..., 1])
    inter = w * h
    da = db[..., 2] * db[..., 3]
    union = np.where(np.asarray(crowd, bool).reshape(1, -1), da, (da + gb[..., 2] * gb[..., 3]) - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = inter / union
    return np.where((w <= 0) | (h <= 0), 0.0, out)


def match_cell(g, d, lo, hi, thrs, keep):
    """One cell at one area range.  g: dict of the cell's GT arrays (file order), d: its detections (file order).
    Returns (scores of the kept detections in rank order, codes[T, D] in {FP, TP, IGN}, number of non-ignored GTs)."""
    rank = np.argsort(-d["score"], kind="stable")[:keep]
    score, dbox = d["score"][rank], d["bbox"][rank]
    ign = (g["iscrowd"] != 0) | (g["area"] < lo) | (g["area"] > hi)
    pos = np.argsort(ign, kind="stable")                   # non-ignored GTs first, stable
    ign, crowd, gid = ign[pos], g["iscrowd"][pos] != 0, g["id"][pos]
    iou = iou_rows(dbox, g["bbox"][pos], crowd)
    darea = dbox[:, 2] * dbox[:, 3]
    codes = np.zeros((len(thrs), len(rank)), np.int8)
    for ti, t in enumerate(thrs):
        floor = min(t, 1 - 1e-10)
        used = np.zeros(len(pos), bool)
        for r in range(len(rank)):
            ok = ~(used & ~crowd) & (iou[r] >= floor)
            m = -1
            for group in (ok & ~ign, ok & ign):            # the last GT with the best IoU, non-ignored ones first
                if group.any():
                    best = iou[r][group].max()
                    m = int(np.nonzero(group & (iou[r] == best))[0][-1])
                    break
            matched, ignored = False, False
            if m >= 0:
                used[m] = True
                ignored = bool(ign[m])
                matched = gid[m] != 0
            if not matched and (darea[r] < lo or darea[r] > hi):
                ignored = True
            codes[ti, r] = IGN if ignored else (TP if matched else FP)
    return score, codes, int((~ign).sum())


def precision_curve(codes, npig, rec_thrs):
    """Codes of one (category, area, maxDets, threshold) in accumulation order -> (precision at rec_thrs, recall)."""
    tp = np.cumsum(codes == TP).astype(np.float64)
    fp = np.cumsum(codes == FP).astype(np.float64)
    nd = len(codes)
    if nd == 0:
        return np.zeros(len(rec_thrs)), 0.0
    rc = tp / npig
    pr = tp / ((fp + tp) + np.spacing(1))
    pr = np.maximum.accumulate(pr[::-1])[::-1]
    at = np.searchsorted(rc, rec_thrs, side="left")
    return np.where(at < nd, pr[np.minimum(at, nd - 1)], 0.0), rc[-1]


def coco_ref(gt, dt, img_ids=None, cat_ids=None, iou_thrs=None):
    """Arrays in ``coco_eval``'s form -> (precision[T,R,K,A,M], recall[T,K,A,M])."""
    thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, np.float64).reshape(-1)
    gimg, gcat = np.asarray(gt["image_id"]), np.asarray(gt["category_id"])
    dimg, dcat = np.asarray(dt["image_id"]), np.asarray(dt["category_id"])
    imgs = np.unique(gimg if img_ids is None else np.asarray(img_ids))
    cats = np.unique(gcat if cat_ids is None else np.asarray(cat_ids))
    G = {k: np.asarray(gt[k]) for k in ("bbox", "area", "iscrowd", "id")}
    G["bbox"] = G["bbox"].astype(np.float64).reshape(-1, 4)
    D = {"bbox": np.asarray(dt["bbox"], np.float64).reshape(-1, 4), "score": np.asarray(dt["score"], np.float64)}
    T, R, K, A, M = len(thrs), len(REC_THRS), len(cats), len(AREA_RNG), len(MAX_DETS)
    precision = np.full((T, R, K, A, M), -1.0)
    recall = np.full((T, K, A, M), -1.0)
    for k, c in enumerate(cats):
        cells = []                                         # (image index, GT rows, detection rows) of the existing cells
        for i, im in enumerate(imgs):
            gr = np.nonzero((gcat == c) & (gimg == im))[0]
            dr = np.nonzero((dcat == c) & (dimg == im))[0]
            if len(gr) or len(dr):
                cells.append((i, gr, dr))
        if not cells:
            continue
        for a, (lo, hi) in enumerate(AREA_RNG):
            per = [(i, match_cell({n: v[gr] for n, v in G.items()}, {n: v[dr] for n, v in D.items()}, lo, hi, thrs, MAX_DETS[-1]))
                   for i, gr, dr in cells]
            npig = sum(res[2] for _, res in per)
            if npig == 0:
                continue
            for m, md in enumerate(MAX_DETS):
                score = np.concatenate([res[0][:md] for _, res in per])
                img = np.concatenate([np.full(min(len(res[0]), md), i) for i, res in per])
                rnk = np.concatenate([np.arange(min(len(res[0]), md)) for _, res in per])
                codes = np.concatenate([res[1][:, :md] for _, res in per], axis=1)
                order = np.lexsort((rnk, img, -score))     # key (-score, image index, rank in cell)
                for t in range(T):
                    precision[t, :, k, a, m], recall[t, k, a, m] = precision_curve(codes[t, order], npig, REC_THRS)
    return precision, recall


# ---------------------------------------------------------------------------------------------------------------------
# exact assignment
# ---------------------------------------------------------------------------------------------------------------------
class Lex:
    """(count, distance) compared lexicographically."""
    __slots__ = ("n", "d")

    def __init__(self, n, d=0.0):
        self.n, self.d = n, d

    def __add__(self, o):
        return Lex(self.n + o.n, self.d + o.d)

    def __sub__(self, o):
        return Lex(self.n - o.n, self.d - o.d)

    def __lt__(self, o):
        return self.n < o.n or (self.n == o.n and self.d < o.d)

    def __le__(self, o):
        return not o < self


def _hungarian(cost, zero, inf):
    """Minimum-cost perfect matching of a square matrix of ``Lex`` (shortest augmenting paths with potentials).
    Returns row -> column."""
    n = len(cost)
    u = [zero] * (n + 1)
    v = [zero] * (n + 1)
    p = [0] * (n + 1)
    way = [0] * (n + 1)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = [inf] * (n + 1)
        used = [False] * (n + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], inf, -1
            for j in range(1, n + 1):
                if not used[j]:
                    cur = cost[i0 - 1][j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(n + 1):
                if used[j]:
                    u[p[j]] = u[p[j]] + delta
                    v[j] = v[j] - delta
                else:
                    minv[j] = minv[j] - delta
            j0 = j1
            if p[j0] == 0:
                break
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    r2c = [-1] * n
    for j in range(1, n + 1):
        if p[j]:
            r2c[p[j] - 1] = j - 1
    return r2c


def assign_lex(dist, valid):
    """Rows x columns: the pairs of a matching of maximum cardinality and, among those, minimum sum of ``dist`` over
    ``valid`` pairs.  Embedding: (r + c) square, a valid pair costs (-1, d), an invalid one (1, 0) (never worth taking),
    every dummy 0."""
    dist = np.asarray(dist, np.float64)
    valid = np.asarray(valid, bool)
    r, c = valid.shape
    if r == 0 or c == 0 or not valid.any():
        return []
    n = r + c
    zero = Lex(0, 0.0)
    cost = [[zero] * n for _ in range(n)]
    for i in range(r):
        for j in range(c):
            cost[i][j] = Lex(-1, float(dist[i, j])) if valid[i, j] else Lex(1, 0.0)
    r2c = _hungarian(cost, zero, Lex(1 << 40, float("inf")))
    return [(i, r2c[i]) for i in range(r) if r2c[i] < c and valid[i, r2c[i]]]


def max_weight(w):
    """Exact maximum total weight of a one-to-one pairing of rows and columns (integer weights >= 0)."""
    w = np.asarray(w, np.int64)
    r, c = w.shape
    if r == 0 or c == 0 or not (w > 0).any():
        return 0
    n = r + c
    zero = Lex(0, 0.0)
    cost = [[zero] * n for _ in range(n)]
    for i in range(r):
        for j in range(c):
            cost[i][j] = Lex(-int(w[i, j]), 0.0)
    r2c = _hungarian(cost, zero, Lex(1 << 60, 0.0))
    return int(sum(w[i, r2c[i]] for i in range(r) if r2c[i] < c))


# ---------------------------------------------------------------------------------------------------------------------
# MOT
# ---------------------------------------------------------------------------------------------------------------------
def box_iou(a, b):
    iw = max(min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]), 0.0)
    i = iw * ih
    u = (a[2] * a[3] + b[2] * b[3]) - i
    return 0.0 if i == 0 else i / u


def mot_ref(gt, hyp, assign=assign_lex, weight=max_weight):
    """``(n, 6)`` rows ``frame, id, x, y, w, h`` (0-based boxes) -> dict of counts (+ ``dist_sum``, ``events``: per
    frame the list of (kind, oid, hid)).  ``assign`` / ``weight``: the per-frame assignment and the IDTP matching; crowded
    frames pass faster equivalents (tests/test_gpu_eval_lap.py), the pure-Python ones being cubic in rows + columns."""
    gt = np.asarray(gt, np.float64).reshape(-1, 6)
    hyp = np.asarray(hyp, np.float64).reshape(-1, 6)
    frames = np.union1d(gt[:, 0], hyp[:, 0])
    m, last_match, present, tracked = {}, {}, {}, {}
    last_update = None
    c = dict(num_frames=len(frames), num_objects=0, num_predictions=0, num_matches=0, num_switches=0, num_misses=0,
             num_false_positives=0)
    dist_sum = 0.0
    events = []
    n_oh = {}
    for f in frames:
        O = gt[gt[:, 0] == f]
        H = hyp[hyp[:, 0] == f]
        O = O[np.argsort(O[:, 1], kind="stable")]
        H = H[np.argsort(H[:, 1], kind="stable")]
        oids, hids = O[:, 1].tolist(), H[:, 1].tolist()
        D = np.array([[1.0 - box_iou(o[2:6], h[2:6]) for h in H] for o in O], np.float64).reshape(len(O), len(H))
        V = D <= 0.5
        for i, o in enumerate(oids):
            for j, h in enumerate(hids):
                if V[i, j]:
                    n_oh[(o, h)] = n_oh.get((o, h), 0) + 1
        om = [None] * len(O)
        hm = [False] * len(H)
        ev = []
        if len(O) and len(H):
            for i, o in enumerate(oids):
                if o in m and last_match[o] == last_update and m[o] in hids:
                    j = hids.index(m[o])
                    if V[i, j]:
                        om[i] = ("MATCH", j)
                        hm[j] = True
                        last_match[o] = f
        ri = [i for i in range(len(O)) if om[i] is None]
        cj = [j for j in range(len(H)) if not hm[j]]
        if ri and cj:
            pairs = assign(D[np.ix_(ri, cj)], V[np.ix_(ri, cj)])
            for a, b in pairs:
                i, j = ri[a], cj[b]
                o, h = oids[i], hids[j]
                kind = "SWITCH" if (o in m and m[o] != h) else "MATCH"
                om[i] = (kind, j)
                hm[j] = True
                m[o] = h
                last_match[o] = f
        for i, o in enumerate(oids):
            present[o] = present.get(o, 0) + 1
            if om[i] is None:
                c["num_misses"] += 1
                ev.append(("MISS", o, None))
            else:
                kind, j = om[i]
                tracked[o] = tracked.get(o, 0) + 1
                c["num_matches" if kind == "MATCH" else "num_switches"] += 1
                dist_sum += D[i, j]
                ev.append((kind, o, hids[j]))
        for j, h in enumerate(hids):
            if not hm[j]:
                c["num_false_positives"] += 1
                ev.append(("FP", None, h))
        c["num_objects"] += len(O)
        c["num_predictions"] += len(H)
        last_update = f
        events.append(ev)
    c["mostly_tracked"] = sum(1 for o in present if tracked.get(o, 0) / present[o] >= 0.8)
    c["mostly_lost"] = sum(1 for o in present if tracked.get(o, 0) / present[o] < 0.2)
    c["num_unique_objects"] = len(present)
    go = sorted(set(gt[:, 1].tolist()))
    ho = sorted(set(hyp[:, 1].tolist()))
    W = np.zeros((len(go), len(ho)), np.int64)
    for (o, h), n in n_oh.items():
        W[go.index(o), ho.index(h)] = n
    c["idtp"] = weight(W)
    c["idfp"] = c["num_predictions"] - c["idtp"]
    c["idfn"] = c["num_objects"] - c["idtp"]
    c["dist_sum"] = dist_sum
    c["events"] = events
    with np.errstate(divide="ignore", invalid="ignore"):
        c["mota"] = 1.0 - float(np.float64(c["num_misses"] + c["num_switches"] + c["num_false_positives"]) / np.float64(c["num_objects"]))
        c["motp"] = float(np.float64(dist_sum) / np.float64(c["num_matches"] + c["num_switches"]))
        c["idf1"] = float(np.float64(2 * c["idtp"]) / np.float64(c["num_objects"] + c["num_predictions"]))
    return c
