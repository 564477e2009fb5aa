"""Plain Python / NumPy restatement of the HOTA rules (csrc/hota.hip's header), written loop by
loop as the rules read, for the tests of ``rtmodt_amd.evaluation.hota_eval``.  Slow by design, and it shares no code with
the package: the similarity, the solver, the summation orders and the final formulae are all stated again here.

* ``hota_ref``     -- one sequence's sums per alpha (+ per frame: the scored edges and the matching)
* ``match_frame``  -- the frame's maximum-weight matching: isolated edges directly, the contested rest by ``lap_solve``
* ``lap_solve``    -- csrc/lap.h's sparse shortest-augmenting-path solver for float costs, line by line, with the same
                      row, edge and column order, so that assignments agree on ties too
* ``record`` / ``combine`` -- TrackEval's final formulae and ``combine_sequences``
"""
from __future__ import annotations

import numpy as np

EPS = float(np.finfo(float).eps)
ALPHAS = np.arange(0.05, 0.99, 0.05)
LAP_ROWS, LAP_COLS, LAP_EDGES = 256, 256, 2048
MAX_ROWS = 1024
INF = float("inf")
FLOAT_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
SUM_FIELDS = ("HOTA_TP", "HOTA_FN", "HOTA_FP", "loc_sum", "ass_a_sum", "ass_re_sum", "ass_pr_sum")


class Capacity(Exception):
    """A frame past the limits; ``frame`` is its id."""

    def __init__(self, frame, what):
        super().__init__(f"frame {frame}: {what}")
        self.frame = frame


def box_iou(a, b):
    """The evaluator's float64 IoU of two boxes x, y, w, h (mot_eval's distance is 1 - this)."""
    iw = max(min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]), 0.0)
    i = iw * ih
    u = (a[2] * a[3] + b[2] * b[3]) - i
    return 0.0 if i == 0.0 else i / u


def lap_solve(estart, ecol, ecost, ncols):
    """Rows 0..n-1, each with a private dummy column of cost 0 and real edges (CSR) of cost < 0 -> row -> column or -1."""
    nhr = len(estart) - 1
    u, rm = [0.0] * nhr, [-1] * nhr
    v, minv, p, wayrow, used = [0.0] * ncols, [INF] * ncols, [-1] * ncols, [0] * ncols, [False] * ncols
    for h0 in range(nhr):
        touched, usedl = [], []
        i0, jend, drow, dmin, to_dummy = h0, -1, -1, INF, False
        while True:
            ui = u[i0]
            for e in range(estart[i0], estart[i0 + 1]):        # relax the real edges of row i0
                j = ecol[e]
                if used[j]:
                    continue
                cur = ecost[e] - ui - v[j]
                if minv[j] == INF:
                    touched.append(j)
                if cur < minv[j]:
                    minv[j], wayrow[j] = cur, i0
            if 0.0 - ui < dmin:                                 # ... and its dummy edge
                dmin, drow = 0.0 - ui, i0
            delta, j1 = dmin, -1
            for j in touched:
                if not used[j] and minv[j] < delta:
                    delta, j1 = minv[j], j
            u[h0] += delta
            for j in usedl:
                u[p[j]] += delta
                v[j] -= delta
            for j in touched:
                if not used[j]:
                    minv[j] -= delta
            dmin -= delta
            if j1 < 0:
                to_dummy = True
                break
            if p[j1] < 0:
                jend = j1
                break
            used[j1] = True
            usedl.append(j1)
            i0 = p[j1]
        if to_dummy:                                            # row drow gives up its column; shift the path back to h0
            i, jfree = drow, rm[drow]
            rm[i] = -1
            while i != h0:
                j = jfree
                ip = wayrow[j]
                jfree = rm[ip]
                p[j] = ip
                rm[ip] = j
                i = ip
        else:
            j = jend
            while True:
                ip = wayrow[j]
                jn = rm[ip]
                p[j] = ip
                rm[ip] = j
                if ip == h0:
                    break
                j = jn
        for j in touched:
            minv[j], used[j] = INF, False
    return rm


def split_edges(edges):
    """``edges``: (GT row, hyp row, score > 0) in ascending (row, column) order -> (isolated pairs, contested rows in
    ascending order, each contested row's edges).  An edge is isolated when it is the only one of its row and of its column."""
    odeg, hdeg = {}, {}
    for o, h, _ in edges:
        odeg[o] = odeg.get(o, 0) + 1
        hdeg[h] = hdeg.get(h, 0) + 1
    isolated, rows = [], {}
    for o, h, sc in edges:
        if odeg[o] == 1 and hdeg[h] == 1:
            isolated.append((o, h))
        else:
            rows.setdefault(o, []).append((h, sc))
    return isolated, sorted(rows), rows


def match_frame(edges, frame=0):
    """One maximum-weight one-to-one matching of the frame's edges -> the (GT row, hyp row) pairs in ascending GT row."""
    isolated, order, rows = split_edges(edges)
    pairs = list(isolated)
    if order:
        if len(order) > LAP_ROWS:
            raise Capacity(frame, f"{len(order)} contested rows")
        colmap, hcol, estart, ecol, ecost = {}, [], [0], [], []
        for o in order:                                         # rows ascending, a row's edges in ascending hypothesis row
            for h, sc in rows[o]:
                if h not in colmap:                             # contested columns in first-touch order
                    if len(hcol) == LAP_COLS:
                        raise Capacity(frame, "more than 256 contested columns")
                    colmap[h] = len(hcol)
                    hcol.append(h)
                if len(ecol) == LAP_EDGES:
                    raise Capacity(frame, "more than 2048 contested edges")
                ecol.append(colmap[h])
                ecost.append(-sc)
            estart.append(len(ecol))
        rm = lap_solve(estart, ecol, ecost, len(hcol))
        pairs += [(o, hcol[rm[k]]) for k, o in enumerate(order) if rm[k] >= 0]
    return sorted(pairs)


def hota_ref(gt, hyp, alphas=None, match=match_frame):
    """``(n, 6)`` rows ``frame, id, x, y, w, h`` (0-based boxes) of one sequence -> dict: per alpha ``HOTA_TP, HOTA_FN,
    HOTA_FP`` (int64) and ``loc_sum, ass_a_sum, ass_re_sum, ass_pr_sum`` (float64); ``frames``: per frame its id, row counts,
    scored ``edges`` (GT row, hyp row, score) and ``pairs``; ``pmc``: the (o, h) -> potential-match sums."""
    alphas = ALPHAS if alphas is None else np.asarray(alphas, np.float64).reshape(-1)
    al = [float(x) for x in alphas]
    gt = np.asarray(gt, np.float64).reshape(-1, 6)
    hyp = np.asarray(hyp, np.float64).reshape(-1, 6)
    frames = np.union1d(gt[:, 0], hyp[:, 0])
    per = []
    pmc, gtc, trc = {}, {}, {}
    # ---- pass 1 ----
    for f in frames:
        O = gt[gt[:, 0] == f]
        H = hyp[hyp[:, 0] == f]
        O = O[np.argsort(O[:, 1], kind="stable")]
        H = H[np.argsort(H[:, 1], kind="stable")]
        if len(O) > MAX_ROWS or len(H) > MAX_ROWS:
            raise Capacity(int(f), "more than 1024 rows")
        oids, hids = O[:, 1].tolist(), H[:, 1].tolist()
        ob, hb = O[:, 2:6].tolist(), H[:, 2:6].tolist()
        S = {}
        for i in range(len(O)):
            for j in range(len(H)):
                s = box_iou(ob[i], hb[j])
                if s > 0.0:
                    S[(i, j)] = s
        r, c = [0.0] * len(O), [0.0] * len(H)
        for (i, j), s in S.items():                              # (i, j) ascend: each r[i] in ascending j, each c[j] in ascending i
            r[i] += s
            c[j] += s
        for (i, j), s in S.items():
            den = (r[i] + c[j]) - s
            q = s / den if den > EPS else 0.0
            k = (oids[i], hids[j])
            pmc[k] = pmc.get(k, 0.0) + q                        # frames ascend
        for o in oids:
            gtc[o] = gtc.get(o, 0) + 1
        for h in hids:
            trc[h] = trc.get(h, 0) + 1
        per.append({"frame": int(f), "nO": len(O), "nH": len(H), "oids": oids, "hids": hids, "S": S})
    gas = {k: v / ((float(gtc[k[0]]) + float(trc[k[1]])) - v) for k, v in pmc.items()}
    # ---- pass 2 ----
    A = len(al)
    tp, loc = [0] * A, [0.0] * A
    mc = {}
    for fr in per:
        S, oids, hids = fr["S"], fr["oids"], fr["hids"]
        edges = [(i, j, gas[(oids[i], hids[j])] * s) for (i, j), s in S.items()]
        edges = [e for e in edges if e[2] > 0.0]
        pairs = match(edges, fr["frame"])
        fr["edges"], fr["pairs"] = edges, pairs
        for i, j in pairs:                                      # ascending GT row
            s = S[(i, j)]
            for a in range(A):
                if s >= al[a] - EPS:
                    tp[a] += 1
                    loc[a] += s
                    m = mc.setdefault((oids[i], hids[j]), [0] * A)
                    m[a] += 1
    # ---- finish ----
    aa, ar, ap = [0.0] * A, [0.0] * A, [0.0] * A
    for k in sorted(mc):
        g, t = float(gtc[k[0]]), float(trc[k[1]])
        for a in range(A):
            m = float(mc[k][a])
            if m > 0:
                aa[a] += m * (m / ((g + t) - m))
                ar[a] += m * (m / max(1.0, g))
                ap[a] += m * (m / max(1.0, t))
    tp = np.array(tp, np.int64)
    return {"HOTA_TP": tp, "HOTA_FN": len(gt) - tp, "HOTA_FP": len(hyp) - tp, "loc_sum": np.array(loc, np.float64),
            "ass_a_sum": np.array(aa, np.float64), "ass_re_sum": np.array(ar, np.float64), "ass_pr_sum": np.array(ap, np.float64),
            "frames": per, "pmc": pmc, "alphas": np.array(al, np.float64)}


def record(c, combined=False):
    """The sums -> TrackEval's fields per alpha, their means over alpha and the three ``(0)`` values."""
    tp, fn, fp = (np.asarray(c[k], np.int64) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP"))
    r = {k: np.asarray(c[k]) for k in SUM_FIELDS}
    tpf = tp.astype(np.float64)
    r["DetRe"] = tpf / np.maximum(1, tp + fn)
    r["DetPr"] = tpf / np.maximum(1, tp + fp)
    r["DetA"] = tpf / np.maximum(1, tp + fn + fp)
    r["AssA"] = r["ass_a_sum"] / np.maximum(1, tp)
    r["AssRe"] = r["ass_re_sum"] / np.maximum(1, tp)
    r["AssPr"] = r["ass_pr_sum"] / np.maximum(1, tp)
    r["HOTA"] = np.sqrt(r["DetA"] * r["AssA"])
    if combined:                                                # combine_sequences: LocA weighted by TP
        r["LocA"] = r["loc_sum"] / np.maximum(1e-10, tpf)
    else:
        r["LocA"] = np.maximum(1e-10, r["loc_sum"]) / np.maximum(1e-10, tpf)
    r["mean"] = {k: float(np.mean(r[k])) for k in FLOAT_FIELDS}
    r["HOTA(0)"], r["LocA(0)"] = float(r["HOTA"][0]), float(r["LocA"][0])
    r["HOTALocA(0)"] = r["HOTA(0)"] * r["LocA(0)"]
    return r


def combine(counts):
    """TrackEval's combine_sequences on the sums: everything added, then the final formulae."""
    counts = list(counts)
    return record({k: sum(np.asarray(c[k]) for c in counts) for k in SUM_FIELDS}, combined=True)


# ---------------------------------------------------------------------------------------------------------------------
# sequences for the tests
# ---------------------------------------------------------------------------------------------------------------------
def synth_sequence(rng, n_frames, n_obj, *, miss=0.1, fp=0.1, switch=0.05, jitter=3.0, split=True, grid=None):
    """Seeded drift, misses, false positives, id switches and (``split``) two fragments per object.  ``grid``: round every
    coordinate to a multiple of it (tie-heavy inputs).  -> (gt, hyp) rows ``frame, id, x, y, w, h``, frames from 1."""
    gt, hyp = [], []
    hid = 1
    for o in range(n_obj):
        t0 = int(rng.integers(0, n_frames // 3))
        t1 = int(rng.integers(2 * n_frames // 3, n_frames + 1))
        x, y = rng.uniform(0, 600, 2)
        vx, vy = rng.uniform(-4, 4, 2)
        w, h = rng.uniform(40, 120, 2)
        cut = (t0 + t1) // 2 if split else -1
        for f in range(t0, t1):
            if f == cut:
                hid += 1
            b = np.array([x + vx * (f - t0), y + vy * (f - t0), w, h])
            gt.append([f + 1.0, o + 1.0, *b])
            if rng.random() < switch:
                hid += 1
            if rng.random() >= miss:
                hyp.append([f + 1.0, float(hid), *(b + rng.normal(0, jitter, 4))])
        hid += 1
    for f in range(n_frames):
        for _ in range(int(rng.poisson(fp * n_obj))):
            hyp.append([f + 1.0, float(hid), rng.uniform(0, 600), rng.uniform(0, 600), rng.uniform(40, 120), rng.uniform(40, 120)])
            hid += 1
    gt, hyp = np.array(gt, np.float64).reshape(-1, 6), np.array(hyp, np.float64).reshape(-1, 6)
    if grid:
        gt[:, 2:] = np.maximum(np.round(gt[:, 2:] / grid), 1) * grid
        hyp[:, 2:] = np.maximum(np.round(hyp[:, 2:] / grid), 1) * grid
    hyp[:, 4:] = np.maximum(hyp[:, 4:], 1.0)
    return gt, hyp


def tie_sequence(rng, n_frames, groups, m, first_id=1, grid=10.0):
    """``groups`` clusters of ``m`` GT ids and ``m`` hypothesis ids that all carry the cluster's one integer-grid box in every
    frame (a hypothesis id skips a frame now and then, the same frame for the whole cluster): inside a cluster every
    similarity is 1 and every alignment score is equal, so every score ties."""
    gt, hyp = [], []
    for g in range(groups):
        x, y = 400.0 * g, 0.0
        w, h = grid * rng.integers(3, 9, 2)
        skip = set(rng.choice(n_frames, size=max(1, n_frames // 8), replace=False).tolist())
        for f in range(n_frames):
            b = [x + grid * (f % 5), y + grid * (f // 5), float(w), float(h)]
            for k in range(m):
                gt.append([f + 1.0, float(first_id + g * m + k), *b])
                if f not in skip:
                    hyp.append([f + 1.0, float(first_id + g * m + k), *b])
    return np.array(gt, np.float64).reshape(-1, 6), np.array(hyp, np.float64).reshape(-1, 6)
