"""GPU: track stitching (csrc/stitch.hip) against the plain-Python restatement tests/stitch_ref.py and
the hand-worked literals of tests/stitch_cases.py.  Every comparison is exact; boxes lie on an integer grid (every d2 is a
multiple of 1/4 and every sum of them exact) unless a test says otherwise."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import stitch_cases as SC
import stitch_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def EV():
    import rtmodt_amd
    return rtmodt_amd.evaluation


def ref_record(rows, **params):
    p = dict(params)
    return SR.stitch(rows, p.get("max_gap", 30), p.get("max_dist", 20.0), p.get("velocity_window", 0), p.get("interpolate", False))


# ---------------------------------------------------------------------------------------------------------------------
# 1. hand cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_hand_case_alone(EV, name):
    c = SC.BY_NAME[name]
    rec = EV.stitch_tracks([c["rows"]], **c["params"])[0]
    SC.check(rec, c)
    SR.same_record(rec, ref_record(c["rows"], **c["params"]))


def test_hand_cases_as_sequences_of_one_call(EV):
    """Cases that share their parameters travel together: every sequence of the call equals its literals."""
    groups = {}
    for c in SC.CASES:
        groups.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    assert max(len(g) for g in groups.values()) >= 8
    for params, cases in groups.items():
        recs = EV.stitch_tracks([c["rows"] for c in cases], **dict(params))
        assert len(recs) == len(cases)
        for rec, c in zip(recs, cases):
            SC.check(rec, c)
    assert EV.correct_id_switches(SC.HISTORY) == SC.HISTORY_OUT
    assert EV.correct_id_switches(SC.HISTORY, 2, 20) == {k: SC.HISTORY[k] for k in sorted(SC.HISTORY)}      # gap 3 > max_gap 2


# ---------------------------------------------------------------------------------------------------------------------
# 2. random sequences
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 17, 64, 100, 150, 200, 250, 300, 300, 300)


def random_sequence(rng, n, side):
    """n tracklets of 1..20 rows (frames may skip inside a tracklet) starting on frames 1..200 at integer positions in a
    side x side field, moving by an integer step a frame; ids are a random subset of 1..4n in random order."""
    ids = rng.choice(np.arange(1, 4 * n + 2), n, replace=False)
    out = []
    for i in ids:
        k = int(rng.integers(1, 21))
        frames = int(rng.integers(1, 201)) + np.cumsum(np.concatenate([[0], rng.integers(1, 3, k - 1)]))
        x0, y0, vx, vy = rng.integers(0, side), rng.integers(0, side), rng.integers(-2, 3), rng.integers(-2, 3)
        w, h = 2 * rng.integers(4, 12), 2 * rng.integers(4, 12)
        for j, f in enumerate(frames):
            out.append([f, i, x0 + vx * j, y0 + vy * j, w, h])
    r = np.array(out, np.float64).reshape(-1, 6)
    return r[rng.permutation(len(r))]


@pytest.fixture(scope="module")
def random_batch():
    rng = np.random.default_rng(1830)
    seqs = [random_sequence(rng, n, side=max(40, int(16 * np.sqrt(n)))) for n in SIZES]
    cands = [SR.candidates(s) for s in seqs]
    opt = [SR.solve(c) for c in cands]
    return seqs, cands, opt


def test_random_sequences_equal_restatement(EV, random_batch):
    seqs, cands, opt = random_batch
    # the planted mix, asserted before the GPU runs: isolated pairs, contested components and unlinkable tracklets all occur
    iso = hard = big_rows = unlinkable = 0
    for s, c in zip(seqs, cands):
        i, hr, hc, he, big = SR.degree_counts(c)
        assert big[0] <= 256 and big[1] <= 256 and big[2] <= 2048
        iso += i; hard += hr; big_rows = max(big_rows, big[0])
        unlinkable += len(set(s[:, 1].astype(int).tolist()) - {x[0] for x in c} - {x[1] for x in c})
    assert iso >= 50 and hard >= 300 and big_rows >= 8 and unlinkable >= 50, (iso, hard, big_rows, unlinkable)
    runs = [EV.stitch_tracks(seqs, interpolate=True, return_candidates=True) for _ in range(2)]
    for k, (s, c, (chosen, obj), rec) in enumerate(zip(seqs, cands, opt, runs[0])):
        assert rec["candidates"] == c, k                                     # the candidate set, every d2 and every exit point
        SR.check_links(rec["links"], c)                                      # one-to-one and admissible
        assert SR.objective(rec["links"]) == obj, (k, SR.objective(rec["links"]), obj)
        assert Fraction(rec["cost"]) == obj[1] and len(rec["links"]) == obj[0]   # seq_links / seq_cost: exact sums on the grid
        SR.same_record(rec, SR.apply_links(s, rec["links"], interpolate=True))    # everything downstream of the GPU's own links
    for a, b in zip(*runs):                                                  # twice: identical
        SR.same_record(a, b)
        assert a["candidates"] == b["candidates"] and a["cost"] == b["cost"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. planted unique optima
# ---------------------------------------------------------------------------------------------------------------------
def chain(n, first_id=1, y=0.0, frame=10):
    """lap_ref.chain as tracklet geometry.  A_i (ids first_id + i) end on `frame` at x = 30 i; B_j (ids first_id + n + j) start
    two frames later at x = 30 j - 16.  A_i reaches B_i (16 px, d2 256) and B_{i+1} (14 px, d2 196) and nothing else (the next
    are 44 and 46 px away); the last A reaches B_{n-1} alone.  B_0 has only A_0, so a matching of all n rows is forced step by
    step to the identity: the only one of n links, hence the unique optimum.  Rows are solved in id order: every A_i takes
    the cheaper B_{i+1} first, and the last row re-routes all of them along one augmenting path through the 2n tracklets."""
    t = [SC.trk(first_id + i, frame - 2, frame, 30.0 * i, y) for i in range(n)]
    t += [SC.trk(first_id + n + j, frame + 2, frame + 3, 30.0 * j - 16.0, y) for j in range(n)]
    return t, [(first_id + i, first_id + n + i, 2, 256.0) for i in range(n)]


def star(n, first_id, y, frame=10):
    """n tracklets end at x = 0, 1, .. n-1 (n <= 19), one starts at x = -1: distinct d2 1, 4, 9, ..; the nearest one wins."""
    t = [SC.trk(first_id + i, frame - 1, frame, float(i), y) for i in range(n)] + [SC.trk(first_id + n, frame + 3, frame + 4, -1.0, y)]
    return t, [(first_id, first_id + n, 3, 1.0)]


def planted_sequence():
    """One component of 64 tracklets (chain 32) and four more components, 200 px apart in y: a chain of 5 and of 9, two stars."""
    parts = [chain(32, 1, 0.0), chain(5, 100, 200.0), star(7, 200, 400.0), chain(9, 300, 600.0, frame=50), star(19, 400, 800.0)]
    return SC.rows(*[t for p, _ in parts for t in p]), sorted(l for _, ls in parts for l in ls)


def test_planted_unique_optima(EV):
    """The optimum of every component is unique by construction (see chain / star), so the links must equal the
    restatement's exactly, whatever order either solver works in."""
    rows, want = planted_sequence()
    cand = SR.candidates(rows)
    assert SR.degree_counts(cand) == (0, 32 + 5 + 7 + 9 + 19, 32 + 5 + 1 + 9 + 1, 63 + 9 + 7 + 17 + 19, (32, 32, 63))
    ref = SR.stitch(rows)
    assert ref["links"] == want
    hand = SC.BY_NAME["chain_of_four"]
    recs = EV.stitch_tracks([rows, hand["rows"], rows, np.zeros((0, 6)), rows])
    for k in (0, 2, 4):                                    # the same sequence at three positions of one call
        assert recs[k]["links"] == want
        SR.same_record(recs[k], ref)
    SC.check(recs[1], hand)
    assert recs[3]["links"] == [] and len(recs[3]["rows"]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. limits
# ---------------------------------------------------------------------------------------------------------------------
def block(na, nb, extra=False):
    """na tracklets end on frame 10 on an 8-wide patch, nb start on frame 12 on the patch below: all na x nb pairs admissible
    (at most 7 px across, 11 down).  extra: one more A at x = 30 and B number nb - 1 moved to (12, 0): the new A reaches it
    alone (18 px), every other A still does (at most 12 px)."""
    t = [SC.trk(1 + i, 9, 10, float(i % 8), float(i // 8)) for i in range(na)]
    t += [SC.trk(1000 + j, 12, 13, float(j % 8), 4.0 + float(j // 8)) for j in range(nb)]
    if extra:
        t[-1] = SC.trk(1000 + nb - 1, 12, 13, 12.0, 0.0)
        t.append(SC.trk(500, 9, 10, 30.0, 0.0))
    return SC.rows(*t)


def disc(n):
    """n distinct grid points within 19 px of the origin."""
    pts = [(x, y) for x in range(-19, 20) for y in range(-19, 20) if x * x + y * y < 361]
    assert len(pts) >= n
    return pts[:n]


def many_to_one(n):
    return SC.rows(*[SC.trk(1 + i, 9, 10, float(x), float(y)) for i, (x, y) in enumerate(disc(n))], SC.trk(5000, 12, 13, 0.0, 0.0))


def one_to_many(n):
    return SC.rows(SC.trk(1, 9, 10, 0.0, 0.0), *[SC.trk(10 + i, 12, 13, float(x), float(y)) for i, (x, y) in enumerate(disc(n))])


def test_components_at_the_solver_limits(EV):
    cases = {"chain256": (SC.rows(*chain(256)[0]), (256, 256, 511)), "edges2048": (block(32, 64), (32, 64, 2048)),
             "rows256": (many_to_one(256), (256, 1, 256)), "cols256": (one_to_many(256), (1, 256, 256))}
    cands = {k: SR.candidates(r) for k, (r, _) in cases.items()}
    for k, (_, want) in cases.items():
        assert SR.degree_counts(cands[k])[4] == want, k
    recs = EV.stitch_tracks([r for r, _ in cases.values()], return_candidates=True)
    for (k, (r, _)), rec in zip(cases.items(), recs):
        chosen, obj = SR.solve(cands[k])
        assert rec["candidates"] == cands[k], k
        SR.check_links(rec["links"], cands[k])
        assert SR.objective(rec["links"]) == obj and Fraction(rec["cost"]) == obj[1], k
        SR.same_record(rec, SR.apply_links(r, rec["links"]))
    assert recs[0]["links"] == chain(256)[1] and SR.stitch(cases["chain256"][0])["links"] == chain(256)[1]      # the unique optimum
    assert len(recs[1]["links"]) == 32 and len(recs[2]["links"]) == 1 and len(recs[3]["links"]) == 1


@pytest.mark.parametrize("case", ["rows257", "cols257", "edges2049"])
def test_one_past_each_limit_is_refused_and_names_the_sequence(EV, case):
    import rtmodt_amd
    rows, want = {"rows257": (many_to_one(257), (257, 1, 257)), "cols257": (one_to_many(257), (1, 257, 257)),
                  "edges2049": (block(32, 64, extra=True), (33, 64, 2049))}[case]
    assert SR.degree_counts(SR.candidates(rows))[4] == want
    ok = SC.BY_NAME["two_compete_for_one"]
    with pytest.raises(rtmodt_amd._ffi.RtmodtError) as e:
        EV.stitch_tracks([ok["rows"], np.zeros((0, 6)), rows, ok["rows"]])
    assert e.value.code == rtmodt_amd._ffi.E_CAPACITY, e.value
    msg = str(e.value)
    assert "sequence 2" in msg and "256 rows / 256 columns / 2048 links" in msg, msg
    SC.check(EV.stitch_tracks([ok["rows"]])[0], ok)         # the process goes on working


def test_fill_rows_one_short_of_the_need(EV):
    import rtmodt_amd
    c = SC.BY_NAME["fill_rows"]
    sts, trs, rf, rb, _ = SC.csr_of([c["rows"], c["rows"]])
    rc, msg, o = SC.raw_call(rtmodt_amd, sts, trs, rf, rb, interpolate=1, fill_cap=5, guard=3)
    assert rc == rtmodt_amd._ffi.E_CAPACITY and "6 fill rows do not fit fill_cap 5" in msg, (rc, msg)
    assert o["n_fill"] == 6
    assert o["trk_succ"].tolist() == [1, -1, 3, -1] and o["trk_root"].tolist() == [0, 0, 2, 2] and o["trk_link_d2"].tolist() == [125.0, 0, 125.0, 0]
    assert o["seq_links"].tolist() == [1, 1] and o["seq_cost"].tolist() == [125.0, 125.0]
    assert o["fill_trk"][:5].tolist() == [0, 0, 0, 2, 2] and o["fill_frame"][:5].tolist() == [3, 4, 5, 3, 4]
    assert np.array_equal(o["fill_box"][:5], np.concatenate([c["fill"][:, 2:], c["fill"][:2, 2:]]))
    assert (o["fill_trk"][5:] == -7).all() and (o["fill_frame"][5:] == -7).all() and (o["fill_box"][5:] == -7.0).all()     # the sentinel
    rc, _, o = SC.raw_call(rtmodt_amd, sts, trs, rf, rb, interpolate=1, fill_cap=6, guard=3)
    assert rc == 0 and o["n_fill"] == 6 and o["fill_frame"][:6].tolist() == [3, 4, 5, 3, 4, 5] and (o["fill_frame"][6:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. velocity and gap filling off the grid
# ---------------------------------------------------------------------------------------------------------------------
def test_velocity_and_fill_per_element_on_float_boxes(EV):
    """Generic float64 boxes, velocity_window 3, interpolate: the exit point p, d2 and every fill box equal the restatement's
    Python floats element by element -- one division, one multiply, one add, none contracted into an FMA."""
    rng = np.random.default_rng(5)
    out = []
    for i in range(160):
        k = int(rng.integers(1, 9))
        frames = int(rng.integers(1, 60)) + np.cumsum(np.concatenate([[0], rng.integers(1, 4, k - 1)]))
        p0, v = rng.uniform(0, 150, 2), rng.uniform(-3, 3, 2)
        for j, f in enumerate(frames):
            out.append([f, 3 * i + 1, *(p0 + v * j + rng.normal(0, 0.3, 2)), *rng.uniform(8, 30, 2)])
    rows = np.array(out, np.float64)
    cand = SR.candidates(rows, 12, 25.5, 3)
    by = SR.tracklets(rows)[1]
    assert len(cand) >= 150 and sum(c[4] != SR.centre(by[c[0]][-1]) for c in cand) >= 100      # the velocity moves most exit points
    assert not any(float(c[3] * 4.0).is_integer() for c in cand)                              # nothing here is on the grid
    rec = EV.stitch_tracks([rows], max_gap=12, max_dist=25.5, velocity_window=3, interpolate=True, return_candidates=True)[0]
    assert len(rec["candidates"]) == len(cand)
    for got, want in zip(rec["candidates"], cand):
        assert got == want, (got, want)                    # ids, gap, d2 and p, bit for bit
    SR.check_links(rec["links"], cand)
    assert len(rec["links"]) == SR.solve(cand)[1][0]
    want = SR.apply_links(rows, rec["links"], interpolate=True)
    assert len(want["fill"]) >= 50
    SR.same_record(rec, want)


# ---------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------
def fragmented_scene():
    """8 objects on parallel lines 100 px apart (2 px a frame in x, 1 in y) for 120 frames: never closer than 100 px.  Each is
    cut into 2..4 fragments with fresh ids across gaps of 2..6 frames; the hypothesis boxes are the GT boxes."""
    rng = np.random.default_rng(6)
    gt, hyp, next_id, n_frag = [], [], 100, 0
    for o in range(8):
        path = [[f, o + 1, 10.0 + 2.0 * f, 100.0 * o + 1.0 * f, 40.0, 80.0] for f in range(1, 121)]
        gt += path
        cuts = np.sort(rng.choice(np.arange(15, 105, 12), int(rng.integers(1, 4)), replace=False))
        lo = 1
        for c in list(cuts) + [None]:
            hi = 120 if c is None else int(c)
            hyp += [[r[0], next_id] + r[2:] for r in path if lo <= r[0] <= hi]
            next_id += 1; n_frag += 1
            lo = hi + int(rng.integers(2, 7))                  # the next fragment starts 2..6 frames after this one ends
    return np.array(gt, np.float64), np.array(hyp, np.float64), n_frag


def test_end_to_end_stitch_then_evaluate(EV, tmp_path):
    gt, hyp, n_frag = fragmented_scene()
    assert 16 <= n_frag <= 32 and len(np.unique(hyp[:, 1])) == n_frag
    before = EV.mot_eval([(gt, hyp)])[0]
    assert before["idf1"] < 1.0 and before["num_switches"] > 0
    rec = EV.stitch_tracks([hyp], interpolate=True)[0]
    assert rec["n_tracks_before"] == n_frag and rec["n_tracks_after"] == 8 and len(rec["links"]) == n_frag - 8
    after = EV.mot_eval([(gt, rec["rows"])])[0]
    assert after["idfp"] == 0 and after["idfn"] == 0 and after["idf1"] == 1.0 and after["num_switches"] == 0
    assert after["num_misses"] == 0 and after["num_false_positives"] == 0 and len(np.unique(rec["rows"][:, 1])) == 8
    # the same through the command-line tool, in a fresh process, on files
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from stitch_tracks import write_mot
    finally:
        sys.path.pop(0)
    write_mot(tmp_path / "gt.txt", gt)
    write_mot(tmp_path / "hyp.txt", hyp)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stitch_tracks.py"), str(tmp_path / "hyp.txt"), str(tmp_path / "out.txt"),
                        "--gt", str(tmp_path / "gt.txt"), "--interpolate"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["tracks_before"] == n_frag and out["tracks_after"] == 8 and out["before"]["idf1"] == before["idf1"]
    assert out["after"] == {"idf1": 1.0, "num_switches": 0, "mota": 1.0, "idfp": 0, "idfn": 0}
    stitched = EV.load_mot(str(tmp_path / "out.txt"))
    assert np.array_equal(stitched[np.lexsort((stitched[:, 1], stitched[:, 0]))], rec["rows"])
