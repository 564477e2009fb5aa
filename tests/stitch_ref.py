"""Track stitching (csrc/stitch.hip) restated in plain Python loops: the definition the GPU tests
compare against.  Two parts, so that a result can be checked without assuming how a tie between equal optima is broken:

* :func:`candidates` -- the admissible links of a sequence with their exit points and ``d2``;
* :func:`apply_links` -- what a set of chosen links does: roots, new ids, fill rows and the record ``stitch_tracks`` returns.

Between them :func:`solve` picks the links: the maximum number and, among those, the minimum sum of ``d2``.  It does not
mirror lap.h: the graph is split into connected components and each is solved by successive shortest augmenting paths
(Bellman-Ford on the residual graph, every augmentation the cheapest one over all free rows) in exact arithmetic -- ``4 d2``
as Python integers when every ``d2`` is a multiple of 1/4 (boxes on an integer grid), fractions otherwise.
:func:`solve_exhaustive` enumerates every one-to-one choice of a small problem and checks the solver.

Every float operation is a Python float operation in the order the rules state it, one rounding each."""
from fractions import Fraction

import numpy as np


def tracklets(rows):
    """``(n, 6)`` rows ``frame, id, x, y, w, h`` -> ``(ids ascending, {id: [row, ...] by frame})``."""
    rows = np.asarray(rows, np.float64).reshape(-1, 6)
    by = {}
    for r in rows:
        by.setdefault(int(r[1]), []).append([float(v) for v in r])
    for t in by.values():
        t.sort(key=lambda r: r[0])
        assert all(a[0] < b[0] for a, b in zip(t, t[1:])), "a (frame, id) pair occurs twice"
    return sorted(by), by


def centre(r):
    return (r[2] + 0.5 * r[4], r[3] + 0.5 * r[5])


def exit_velocity(trk, velocity_window):
    if velocity_window == 0 or len(trk) == 1:
        return (0.0, 0.0)
    last, ref = trk[-1], trk[-1 - min(velocity_window, len(trk) - 1)]
    ce, cr = centre(last), centre(ref)
    df = float(int(last[0]) - int(ref[0]))
    return ((ce[0] - cr[0]) / df, (ce[1] - cr[1]) / df)


def candidates(rows, max_gap=30, max_dist=20.0, velocity_window=0):
    """The admissible links ``(id_A, id_B, gap, d2, (p.x, p.y))`` in the order the library keeps them: A in id order, then
    B by (first frame, id)."""
    ids, by = tracklets(rows)
    lim = max_dist * max_dist
    out = []
    by_start = sorted(ids, key=lambda i: (by[i][0][0], i))
    for a in ids:
        A = by[a]
        ce, v, e = centre(A[-1]), exit_velocity(A, velocity_window), int(A[-1][0])
        for b in by_start:
            g = int(by[b][0][0]) - e
            if not 1 <= g <= max_gap:
                continue
            gf = float(g)
            p = (ce[0] + v[0] * gf, ce[1] + v[1] * gf)
            cs = centre(by[b][0])
            dx, dy = p[0] - cs[0], p[1] - cs[1]
            d2 = dx * dx + dy * dy
            if d2 < lim:
                out.append((a, b, g, d2, p))
    return out


def degree_counts(cands):
    """-> (isolated pairs, contested rows, contested columns, contested links, largest component (rows, columns, links)) by
    the degree rule: a row of degree 1 whose column has degree 1 is an isolated pair."""
    rdeg, cdeg = {}, {}
    for a, b, *_ in cands:
        rdeg[a] = rdeg.get(a, 0) + 1
        cdeg[b] = cdeg.get(b, 0) + 1
    iso = [(a, b) for a, b, *_ in cands if rdeg[a] == 1 and cdeg[b] == 1]
    hard = [c for c in cands if not (rdeg[c[0]] == 1 and cdeg[c[1]] == 1)]
    big = (0, 0, 0)
    for comp in _components(hard):
        big = max(big, (len({c[0] for c in comp}), len({c[1] for c in comp}), len(comp)))
    return len(iso), len({c[0] for c in hard}), len({c[1] for c in hard}), len(hard), big


def _components(edges):
    """Connected components of the bipartite graph: lists of edges, rows and columns being different nodes."""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for e in edges:
        ra, rb = find(("r", e[0])), find(("c", e[1]))
        if ra != rb:
            parent[ra] = rb
    comps = {}
    for e in edges:
        comps.setdefault(find(("r", e[0])), []).append(e)
    return list(comps.values())


def _exact(d2s):
    """Exact costs: 4 d2 as integers for grid boxes, fractions otherwise."""
    if all(float(d * 4.0).is_integer() for d in d2s):
        return [int(d * 4.0) for d in d2s]
    return [Fraction(d) for d in d2s]


def _ssap(edges, cost):
    """One component: successive shortest augmenting paths.  edges: (row, column); cost: exact.  Nodes: rows, columns; a free
    row is a source (distance 0), a free column a sink.  Residual arcs: row -> column over an unused edge (+cost), column ->
    its matched row over the used edge (-cost)."""
    rows = sorted({e[0] for e in edges})
    adj = {r: [] for r in rows}
    for k, (r, c) in enumerate(edges):
        adj[r].append((c, k))
    match_r, match_c = {}, {}                              # row -> edge index, column -> edge index
    while True:
        dist_r = {r: 0 for r in rows if r not in match_r}
        dist_c, via = {}, {}
        queue = list(dist_r)
        while queue:                                       # Bellman-Ford by a work list; no negative cycle in a residual graph of an optimal flow
            nxt = []
            for r in queue:
                dr = dist_r[r]
                for c, k in adj[r]:
                    if match_r.get(r) == k:
                        continue
                    d = dr + cost[k]
                    if c not in dist_c or d < dist_c[c]:
                        dist_c[c] = d
                        via[c] = k
                        if c in match_c:
                            k2 = match_c[c]
                            r2 = edges[k2][0]
                            d2 = d - cost[k2]
                            if r2 not in dist_r or d2 < dist_r[r2]:
                                dist_r[r2] = d2
                                nxt.append(r2)
            queue = nxt
        free = [c for c in dist_c if c not in match_c]
        if not free:
            break
        c = min(free, key=lambda x: (dist_c[x], x))
        while True:                                        # flip the path back to its source
            k = via[c]
            r = edges[k][0]
            prev = match_r.get(r)
            match_r[r] = k
            match_c[c] = k
            if prev is None:
                break
            c = edges[prev][1]
    return sorted(match_r.values())


def solve(cands):
    """The chosen links of a candidate list (entries start ``id_A, id_B``; ``d2`` at index 3): maximum count, then minimum
    sum of d2.  Returns the chosen entries in A order and the objective ``(count, exact sum of d2)``."""
    chosen = []
    for comp in _components(cands):
        cost = _exact([c[3] for c in comp])
        chosen += [comp[k] for k in _ssap([(c[0], c[1]) for c in comp], cost)]
    chosen.sort(key=lambda c: c[0])
    return chosen, objective(chosen)


def objective(links):
    """(count, exact sum of d2) of a set of links (d2 at index 3)."""
    return len(links), sum((Fraction(c[3]) for c in links), Fraction(0))


def solve_exhaustive(cands):
    """The optimal objective by enumerating every one-to-one subset (small problems only)."""
    rows = sorted({c[0] for c in cands})
    by_row = {r: [c for c in cands if c[0] == r] for r in rows}
    best = [(0, Fraction(0))]

    def rec(i, used, n, s):
        if i == len(rows):
            if n > best[0][0] or (n == best[0][0] and s < best[0][1]):
                best[0] = (n, s)
            return
        rec(i + 1, used, n, s)
        for c in by_row[rows[i]]:
            if c[1] not in used:
                rec(i + 1, used | {c[1]}, n + 1, s + Fraction(c[3]))

    rec(0, frozenset(), 0, Fraction(0))
    return best[0]


def check_links(links, cands):
    """The links are admissible and one-to-one."""
    ok = {(c[0], c[1]): (c[2], c[3]) for c in cands}
    assert all(ok.get((l[0], l[1])) == (l[2], l[3]) for l in links), "a link is not an admissible candidate"
    assert len({l[0] for l in links}) == len(links) and len({l[1] for l in links}) == len(links), "links are not one-to-one"


def apply_links(rows, links, interpolate=False):
    """What the chosen links ``(id_A, id_B, gap, d2)`` do to a sequence -> the record ``stitch_tracks`` returns, plus
    ``fill``: the fill rows in the library's order (A in id order, then k)."""
    ids, by = tracklets(rows)
    links = sorted((int(l[0]), int(l[1]), int(l[2]), float(l[3])) for l in links)
    pred = {b: a for a, b, _, _ in links}
    id_map = {}
    for i in ids:
        r = i
        while r in pred:                                   # the serial walk to the head of the chain
            r = pred[r]
        id_map[i] = r
    out = [[r[0], float(id_map[i])] + r[2:] for i in ids for r in by[i]]
    fill = []
    if interpolate:
        for a, b, g, _ in links:
            la, fb = by[a][-1], by[b][0]
            assert g == int(fb[0]) - int(la[0])
            for k in range(1, g):
                t = float(k) / float(g)
                fill.append([float(int(la[0]) + k), float(id_map[a])] + [la[q] + (fb[q] - la[q]) * t for q in range(2, 6)])
    allrows = np.array(out + fill, np.float64).reshape(-1, 6)
    allrows = allrows[np.lexsort((allrows[:, 1], allrows[:, 0]))]
    return {"rows": allrows, "id_map": id_map, "links": links, "n_tracks_before": len(ids), "n_tracks_after": len(set(id_map.values())),
            "fill": np.array(fill, np.float64).reshape(-1, 6)}


def stitch(rows, max_gap=30, max_dist=20.0, velocity_window=0, interpolate=False):
    """The whole step on one sequence."""
    chosen, _ = solve(candidates(rows, max_gap, max_dist, velocity_window))
    return apply_links(rows, [c[:4] for c in chosen], interpolate)


def same_record(got, want):
    """Exact equality of two records (``fill`` compared when both carry it)."""
    assert got["rows"].shape == want["rows"].shape and np.array_equal(got["rows"], want["rows"]), (got["rows"], want["rows"])
    assert got["id_map"] == want["id_map"], (got["id_map"], want["id_map"])
    assert [tuple(l) for l in got["links"]] == [tuple(l) for l in want["links"]], (got["links"], want["links"])
    assert (got["n_tracks_before"], got["n_tracks_after"]) == (want["n_tracks_before"], want["n_tracks_after"])
    if "fill" in got and "fill" in want:
        assert got["fill"].shape == want["fill"].shape and np.array_equal(got["fill"], want["fill"]), (got["fill"], want["fill"])
