"""Hand-worked track-stitching cases shared by tests/test_stitch_cpu.py (against the restatement) and
tests/test_gpu_stitch.py (against the library).  Every case states its input as tracklets, its parameters, and -- as
literals -- the links ``(id_A, id_B, gap, d2)``, the id map and, where it has any, the fill rows.  Boxes are 10 x 10 on an
integer grid unless a case says otherwise, so a box at (x, y) has its centre at (x + 5, y + 5) and every d2 is exact."""
import numpy as np


def trk(tid, f0, f1, x, y, vx=0.0, vy=0.0, w=10.0, h=10.0):
    """Rows of id `tid` on frames f0..f1, the box at (x, y) on f0 and moving by (vx, vy) a frame."""
    return [[float(f), float(tid), x + vx * (f - f0), y + vy * (f - f0), w, h] for f in range(f0, f1 + 1)]


def rows(*tracklets):
    return np.array([r for t in tracklets for r in t], np.float64).reshape(-1, 6)


def relabel(r, id_map):
    """The input rows under the new ids, sorted by (frame, id)."""
    out = np.array(r, np.float64).reshape(-1, 6).copy()
    out[:, 1] = [id_map[int(i)] for i in out[:, 1]]
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def case(name, r, links, id_map, fill=(), rows_out=None, **params):
    fill = np.array(fill, np.float64).reshape(-1, 6)
    want = np.concatenate([relabel(r, id_map), fill])
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    if rows_out is not None:                               # a case that also writes its rows out must agree with itself
        assert np.array_equal(want, np.array(rows_out, np.float64).reshape(-1, 6)), name
    return {"name": name, "rows": r, "params": params, "links": [tuple(l) for l in links], "id_map": dict(id_map), "fill": fill,
            "want_rows": want, "n_before": len(id_map), "n_after": len(set(id_map.values()))}


CASES = [
    # the gap: s_B - e_A = 30 = max_gap is linked (centres (105, 105) and (108, 109): 9 + 16), 31 is not
    case("gap_equal_max", rows(trk(1, 1, 5, 100, 100), trk(2, 35, 40, 103, 104)), [(1, 2, 30, 25.0)], {1: 1, 2: 1}),
    case("gap_max_plus_one", rows(trk(1, 1, 5, 100, 100), trk(2, 36, 40, 103, 104)), [], {1: 1, 2: 2}),
    case("gap_at_custom_max", rows(trk(1, 1, 5, 100, 100), trk(2, 9, 12, 100, 100), trk(3, 17, 18, 100, 100)), [(1, 2, 4, 0.0)],
         {1: 1, 2: 1, 3: 3}, max_gap=4),
    # gap 0 (B starts on A's last frame) and overlapping tracklets are never linked, however close
    case("gap_zero_and_overlap", rows(trk(1, 1, 5, 100, 100), trk(2, 5, 9, 100, 100), trk(3, 3, 8, 101, 100)), [], {1: 1, 2: 2, 3: 3}),
    # the distance is strict: dx 12, dy 16 -> d2 = 400 = 20^2 is not linked; dy 15 -> 369 is
    case("d2_exactly_limit", rows(trk(1, 1, 5, 100, 100), trk(2, 8, 9, 112, 116)), [], {1: 1, 2: 2}),
    case("d2_one_step_below", rows(trk(1, 1, 5, 100, 100), trk(2, 8, 9, 112, 115)), [(1, 2, 3, 369.0)], {1: 1, 2: 1}),
    # four fragments in time order 5, 9, 2, 7, each 3 px on: the only choice of three links is the chain (5 -> 2, 5 -> 7,
    # 9 -> 7 are admissible too, but any of them leaves at most two links); everything collapses to id 5
    case("chain_of_four", rows(trk(5, 1, 3, 0, 0), trk(9, 6, 8, 3, 0), trk(2, 10, 12, 6, 0), trk(7, 15, 16, 9, 0)),
         [(2, 7, 3, 9.0), (5, 9, 3, 9.0), (9, 2, 2, 9.0)], {2: 5, 5: 5, 7: 5, 9: 5},
         rows_out=[[1, 5, 0, 0, 10, 10], [2, 5, 0, 0, 10, 10], [3, 5, 0, 0, 10, 10], [6, 5, 3, 0, 10, 10], [7, 5, 3, 0, 10, 10],
                   [8, 5, 3, 0, 10, 10], [10, 5, 6, 0, 10, 10], [11, 5, 6, 0, 10, 10], [12, 5, 6, 0, 10, 10], [15, 5, 9, 0, 10, 10],
                   [16, 5, 9, 0, 10, 10]]),
    # two tracklets end on frame 5 at x = 0 and x = 10; one starts on frame 8 at x = 4: d2 16 beats 36
    case("two_compete_for_one", rows(trk(1, 1, 5, 0, 0), trk(2, 2, 5, 10, 0), trk(3, 8, 9, 4, 0)), [(1, 3, 3, 16.0)], {1: 1, 2: 2, 3: 1},
         rows_out=[[1, 1, 0, 0, 10, 10], [2, 1, 0, 0, 10, 10], [2, 2, 10, 0, 10, 10], [3, 1, 0, 0, 10, 10], [3, 2, 10, 0, 10, 10],
                   [4, 1, 0, 0, 10, 10], [4, 2, 10, 0, 10, 10], [5, 1, 0, 0, 10, 10], [5, 2, 10, 0, 10, 10], [8, 1, 4, 0, 10, 10],
                   [9, 1, 4, 0, 10, 10]]),
    # max_dist 5.  A1 at x = 0, A2 at x = 4 end on frame 3; B1 at x = 1, B2 at x = -2 start on frame 5.  d2: A1-B1 1, A1-B2 4,
    # A2-B1 9, A2-B2 36 (not admissible).  Nearest-first takes A1-B1 and leaves A2 nothing: one link.  The optimum has two.
    case("greedy_one_optimum_two", rows(trk(1, 1, 3, 0, 0), trk(2, 1, 3, 4, 0), trk(3, 5, 6, 1, 0), trk(4, 5, 6, -2, 0)),
         [(1, 4, 2, 4.0), (2, 3, 2, 9.0)], {1: 1, 2: 2, 3: 2, 4: 1}, max_dist=5.0),
    # max_dist 20.  A1 at x = 0, A2 at x = 3; B1 at x = 1, B2 at x = -2.  d2: A1-B1 1, A1-B2 4, A2-B1 4, A2-B2 25.  Nearest-first:
    # A1-B1 then A2-B2, sum 26; the optimum crosses them: sum 8.
    case("greedy_two_larger_sum", rows(trk(1, 1, 3, 0, 0), trk(2, 1, 3, 3, 0), trk(3, 5, 6, 1, 0), trk(4, 5, 6, -2, 0)),
         [(1, 4, 2, 4.0), (2, 3, 2, 4.0)], {1: 1, 2: 2, 3: 2, 4: 1}),
    # single-row tracklets link like any other, and have no velocity whatever the window
    case("single_rows", rows(trk(1, 1, 1, 0, 0), trk(2, 3, 3, 2, 0), trk(3, 40, 40, 2, 0)), [(1, 2, 2, 4.0)], {1: 1, 2: 1, 3: 3},
         velocity_window=3),
    # 8 px a frame: A ends on frame 5 at x = 40, B starts 10 frames later at x = 120.  Window 0: 80 px apart.  Window 3:
    # v = (40 - 16) / 3 = 8, p = 40 + 8 * 10 = 120, d2 = 0
    case("velocity_window_0", rows(trk(1, 1, 5, 8, 0, vx=8.0), trk(2, 15, 18, 120, 0, vx=8.0)), [], {1: 1, 2: 2}),
    case("velocity_window_3", rows(trk(1, 1, 5, 8, 0, vx=8.0), trk(2, 15, 18, 120, 0, vx=8.0)), [(1, 2, 10, 0.0)], {1: 1, 2: 1},
         velocity_window=3),
    # the window clamps to the tracklet: two rows on frames 1 and 3 at x = 0 and 16, window 5 -> v = 16 / 2 = 8; B on frame 6
    # at x = 16 + 8 * 3 = 40
    case("velocity_window_clamps", np.array([[1, 1, 0, 0, 10, 10], [3, 1, 16, 0, 10, 10], [6, 2, 40, 0, 10, 10]], np.float64),
         [(1, 2, 3, 0.0)], {1: 1, 2: 1}, velocity_window=5),
    # gap filling: A's last box (0, 0, 10, 10) on frame 2, B's first box (8, 4, 14, 12) on frame 6: centres (5, 5) and (15, 10),
    # d2 = 125; t = 1/4, 2/4, 3/4
    case("fill_rows", np.array([[1, 1, 0, 0, 10, 10], [2, 1, 0, 0, 10, 10], [6, 2, 8, 4, 14, 12], [7, 2, 8, 4, 14, 12]], np.float64),
         [(1, 2, 4, 125.0)], {1: 1, 2: 1}, fill=[[3, 1, 2, 1, 11, 10.5], [4, 1, 4, 2, 12, 11], [5, 1, 6, 3, 13, 11.5]],
         rows_out=[[1, 1, 0, 0, 10, 10], [2, 1, 0, 0, 10, 10], [3, 1, 2, 1, 11, 10.5], [4, 1, 4, 2, 12, 11], [5, 1, 6, 3, 13, 11.5],
                   [6, 1, 8, 4, 14, 12], [7, 1, 8, 4, 14, 12]], interpolate=True),
    # a gap of one frame links and has nothing to fill
    case("fill_gap_one", rows(trk(4, 1, 2, 0, 0), trk(3, 3, 4, 1, 0)), [(4, 3, 1, 1.0)], {3: 4, 4: 4}, interpolate=True),
    case("empty_sequence", np.zeros((0, 6)), [], {}),
]
BY_NAME = {c["name"]: c for c in CASES}


def check(rec, c):
    """A record (the library's or the restatement's) equals the case's literals."""
    assert [tuple(l) for l in rec["links"]] == c["links"], (c["name"], rec["links"])
    assert rec["id_map"] == c["id_map"], (c["name"], rec["id_map"])
    assert rec["rows"].shape == c["want_rows"].shape and np.array_equal(rec["rows"], c["want_rows"]), (c["name"], rec["rows"])
    assert np.array_equal(rec["fill"], c["fill"]), (c["name"], rec["fill"])
    assert (rec["n_tracks_before"], rec["n_tracks_after"]) == (c["n_before"], c["n_after"]), c["name"]


# correct_id_switches on the design document's dict form: ids 7 and 12 are one object, 9 is another
HISTORY = {7: [(1, 0.0, 0.0, 10.0, 10.0), (2, 1.0, 0.0, 10.0, 10.0)], 12: [(5, 4.0, 0.0, 10.0, 10.0), (6, 5.0, 0.0, 10.0, 10.0)],
           9: [(1, 200.0, 50.0, 10.0, 10.0), (2, 200.0, 50.0, 10.0, 10.0)]}
HISTORY_OUT = {7: [(1, 0.0, 0.0, 10.0, 10.0), (2, 1.0, 0.0, 10.0, 10.0), (5, 4.0, 0.0, 10.0, 10.0), (6, 5.0, 0.0, 10.0, 10.0)],
               9: [(1, 200.0, 50.0, 10.0, 10.0), (2, 200.0, 50.0, 10.0, 10.0)]}


def raw_call(pkg, seq_trk_start, trk_row_start, row_frame, row_box, *, max_gap=30, max_dist=20.0, velocity_window=0, interpolate=0,
             fill_cap=0, guard=0, null=(), params_null=False, n_seq=None, fill_cap_arg=None):
    """rtmodt_stitch_tracks through ctypes on the caller's own arrays.  The fill buffers get `guard` extra rows of a sentinel
    behind fill_cap.  `null`: argument names passed as NULL.  Returns (return code, message, outputs)."""
    import ctypes as C
    F = pkg._ffi
    sts = np.ascontiguousarray(seq_trk_start, np.int32)
    trs = np.ascontiguousarray(trk_row_start, np.int32)
    rf = np.ascontiguousarray(row_frame, np.int64)
    rb = np.ascontiguousarray(row_box, np.float64).reshape(-1, 4)
    n_seq = len(sts) - 1 if n_seq is None else n_seq
    n_trk = max(len(trs) - 1, 0)
    o = {"trk_succ": np.full(n_trk, -7, np.int32), "trk_root": np.full(n_trk, -7, np.int32), "trk_link_d2": np.full(n_trk, -7.0),
         "seq_links": np.full(max(n_seq, 0), -7, np.int64), "seq_cost": np.full(max(n_seq, 0), -7.0),
         "fill_trk": np.full(fill_cap + guard, -7, np.int32), "fill_frame": np.full(fill_cap + guard, -7, np.int64),
         "fill_box": np.full((fill_cap + guard, 4), -7.0)}
    n_fill = C.c_int64(-7)
    a = {"seq_trk_start": sts, "trk_row_start": trs, "row_frame": rf, "row_box": rb, **o}
    P = lambda k: None if k in null else F.ptr(a[k])       # noqa: E731
    params = F.StitchParams(max_gap, max_dist, velocity_window, interpolate)
    rc = F.lib().rtmodt_stitch_tracks(0, None if params_null else C.byref(params), n_seq, P("seq_trk_start"), P("trk_row_start"),
                                      P("row_frame"), P("row_box"), P("trk_succ"), P("trk_root"), P("trk_link_d2"), P("seq_links"),
                                      P("seq_cost"), fill_cap if fill_cap_arg is None else fill_cap_arg, P("fill_trk"), P("fill_frame"),
                                      P("fill_box"), None if "n_fill" in null else C.byref(n_fill), 0, None, None, None, None, None)
    o["n_fill"] = n_fill.value
    return rc, F.lib().rtmodt_last_error().decode(errors="replace") if rc else "", o


def csr_of(sequences):
    """Sequences of (n, 6) rows -> (seq_trk_start, trk_row_start, row_frame, row_box, ids per sequence), as the wrapper lays them out."""
    sts, trs, frames, boxes, ids = [0], [0], [], [], []
    for r in sequences:
        r = np.asarray(r, np.float64).reshape(-1, 6)
        r = r[np.lexsort((r[:, 0], r[:, 1]))]
        u, cnt = np.unique(r[:, 1], return_counts=True)
        for c in cnt:
            trs.append(trs[-1] + int(c))
        sts.append(sts[-1] + len(u))
        frames.append(r[:, 0].astype(np.int64)); boxes.append(r[:, 2:6]); ids.append(u.astype(np.int64))
    return (np.array(sts, np.int32), np.array(trs, np.int32), np.concatenate(frames) if frames else np.zeros(0, np.int64),
            np.concatenate(boxes) if boxes else np.zeros((0, 4)), ids)
