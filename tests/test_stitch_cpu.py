"""CPU: the track-stitching rules.  The plain-Python restatement tests/stitch_ref.py is checked
against the hand-worked literal cases of tests/stitch_cases.py, its solver against exhaustive enumeration, and the parts of
the library that need no GPU are run: the Python-side input checks and every argument check of rtmodt_stitch_tracks (they
all precede the first HIP call)."""
import numpy as np
import pytest

import stitch_cases as SC
import stitch_ref as SR


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_restatement_equals_the_hand_cases(name):
    c = SC.BY_NAME[name]
    SC.check(SR.stitch(c["rows"], **c["params"]), c)


def test_hand_cases_cover_what_they_claim():
    """The greedy cases really separate nearest-first from the optimum; the competing case really has two candidates."""
    def greedy(cands):
        used_a, used_b, out = set(), set(), []
        for c in sorted(cands, key=lambda c: (c[3], c[0], c[1])):
            if c[0] not in used_a and c[1] not in used_b:
                used_a.add(c[0]); used_b.add(c[1]); out.append(c)
        return out
    c = SC.BY_NAME["greedy_one_optimum_two"]
    cand = SR.candidates(c["rows"], max_dist=5.0)
    assert [(x[0], x[1], x[3]) for x in cand] == [(1, 3, 1.0), (1, 4, 4.0), (2, 3, 9.0)]
    assert len(greedy(cand)) == 1 and SR.solve(cand)[1] == (2, 13)
    c = SC.BY_NAME["greedy_two_larger_sum"]
    cand = SR.candidates(c["rows"])
    assert len(cand) == 4 and SR.objective(greedy(cand)) == (2, 26) and SR.solve(cand)[1] == (2, 8)
    cand = SR.candidates(SC.BY_NAME["two_compete_for_one"]["rows"])
    assert [(x[0], x[1], x[3]) for x in cand] == [(1, 3, 16.0), (2, 3, 36.0)]
    cand = SR.candidates(SC.BY_NAME["chain_of_four"]["rows"])
    assert len(cand) == 6 and SR.degree_counts(cand)[4] == (3, 3, 6)
    cand = SR.candidates(SC.BY_NAME["velocity_window_3"]["rows"], velocity_window=3)
    assert cand == [(1, 2, 10, 0.0, (125.0, 5.0))]


def random_problem(rng, n):
    """n tracklets of 1..3 rows on a coarse grid in a short time span: dense, tie-rich candidate graphs."""
    t = []
    for i in range(n):
        f0 = int(rng.integers(1, 7))
        t.append(SC.trk(i + 1, f0, f0 + int(rng.integers(0, 3)), float(rng.integers(0, 5) * 4), float(rng.integers(0, 3) * 4)))
    return SC.rows(*t)


def test_solver_equals_exhaustive_enumeration():
    rng = np.random.default_rng(18)
    contested = 0
    for _ in range(200):
        r = random_problem(rng, int(rng.integers(3, 9)))
        cand = SR.candidates(r, max_gap=int(rng.integers(2, 8)), max_dist=float(rng.integers(5, 14)))
        chosen, obj = SR.solve(cand)
        SR.check_links(chosen, cand)
        assert obj == SR.solve_exhaustive(cand), (r, cand)
        contested += SR.degree_counts(cand)[3] > 0
    assert contested >= 100                                 # most problems leave the solver something to decide


def test_solver_on_non_grid_costs_uses_fractions():
    rng = np.random.default_rng(19)
    for _ in range(20):
        r = random_problem(rng, 7)
        r[:, 2:4] += rng.uniform(-1, 1, (len(r), 2))
        cand = SR.candidates(r, max_gap=6, max_dist=9.0, velocity_window=2)
        assert SR.solve(cand)[1] == SR.solve_exhaustive(cand)


def test_correct_id_switches_on_a_dict(pkg):
    """The adapter's two conversions around the restatement: the design document's dict in, the merged dict out."""
    from rtmodt_amd.evaluation import stitch as ST
    r = ST.history_to_rows(SC.HISTORY)
    assert r.shape == (6, 6) and sorted(set(r[:, 1].tolist())) == [7.0, 9.0, 12.0]
    rec = SR.stitch(r, 30, 20.0)
    assert rec["links"] == [(7, 12, 3, 9.0)]
    assert ST.rows_to_history(rec["rows"]) == SC.HISTORY_OUT
    assert ST.rows_to_history(r) == {k: SC.HISTORY[k] for k in sorted(SC.HISTORY)}
    import inspect
    sig = inspect.signature(pkg.evaluation.correct_id_switches)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[:3]] == [("tracks_history", inspect.Parameter.empty), ("max_gap", 30), ("max_dist", 20)]


def test_python_side_value_errors(pkg):
    st = pkg.evaluation.stitch_tracks
    ok = SC.rows(SC.trk(1, 1, 3, 0, 0))
    with pytest.raises(ValueError, match=r"\(frame, id\) pair occurs twice"):
        st([np.concatenate([ok, ok[:1]])])
    bad = ok.copy(); bad[1, 0] = 2.5
    with pytest.raises(ValueError, match="frame number is not an integer"):
        st([bad])
    bad = ok.copy(); bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="frame number is not an integer"):
        st([bad])
    bad = ok.copy(); bad[:, 1] = 1.5
    with pytest.raises(ValueError, match="track id is not an integer"):
        st([ok, bad])
    assert st([]) == []


GOOD = dict(seq_trk_start=[0, 2], trk_row_start=[0, 2, 3], row_frame=[1, 2, 5], row_box=[[0, 0, 10, 10]] * 3)


def invalid(pkg, match, **kw):
    a = {k: kw.pop(k, v) for k, v in GOOD.items()}
    rc, msg, _ = SC.raw_call(pkg, a["seq_trk_start"], a["trk_row_start"], a["row_frame"], a["row_box"], **kw)
    assert rc == pkg._ffi.E_INVALID, (rc, msg)
    assert msg.startswith("stitch_tracks:") and match in msg, msg


def test_every_invalid_argument_is_refused_before_any_hip_call(pkg):
    """No GPU here: a call that got past its checks would fail with RTMODT_E_HIP, not RTMODT_E_INVALID."""
    invalid(pkg, "null params", params_null=True)
    invalid(pkg, "null params or n_fill", null=("n_fill",))
    for name in ("seq_trk_start", "seq_links", "seq_cost"):
        invalid(pkg, "null sequence arrays", null=(name,))
    for name in ("trk_row_start", "row_frame", "row_box", "trk_succ", "trk_root", "trk_link_d2"):
        invalid(pkg, "null tracklet or row arrays", null=(name,))
    for name in ("fill_trk", "fill_frame", "fill_box"):
        invalid(pkg, "null fill arrays", null=(name,), fill_cap=4, interpolate=1)
    invalid(pkg, "max_gap 0", max_gap=0)
    invalid(pkg, "max_gap 1048577", max_gap=(1 << 20) + 1)
    for d in (0.0, -1.0, float("inf"), float("nan")):
        invalid(pkg, "max_dist", max_dist=d)
    invalid(pkg, "velocity_window -1", velocity_window=-1)
    invalid(pkg, "interpolate 2", interpolate=2)
    invalid(pkg, "n_seq -1", n_seq=-1)
    invalid(pkg, "fill_cap -1", fill_cap_arg=-1)
    invalid(pkg, "must start at 0", seq_trk_start=[1, 2])
    invalid(pkg, "sequence 1: the tracklet CSR is not monotone", seq_trk_start=[0, 2, 1])
    invalid(pkg, "row CSR must start at 0", trk_row_start=[1, 2, 3])
    invalid(pkg, "sequence 0 tracklet 1 (row 2): the row CSR is not monotone", trk_row_start=[0, 2, 2])
    invalid(pkg, "sequence 0 row 1: frames must ascend strictly", row_frame=[1, 1, 5])
    invalid(pkg, "sequence 0 row 1: frames must ascend strictly", row_frame=[2, 1, 5])
    invalid(pkg, "sequence 0 row 2: frame", row_frame=[1, 2, 1 << 60])
    for q, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan)):
        box = np.array(GOOD["row_box"], np.float64)
        box[2, q] = v
        invalid(pkg, "sequence 0 row 2 has a NaN or infinite box", row_box=box)
    # the second sequence is named as such
    invalid(pkg, "sequence 1 row 4: frames must ascend strictly", seq_trk_start=[0, 2, 3], trk_row_start=[0, 2, 3, 5], row_frame=[1, 2, 5, 7, 7],
            row_box=[[0, 0, 10, 10]] * 5)


def test_nothing_to_do_is_success_without_a_device(pkg):
    rc, _, o = SC.raw_call(pkg, [0], [0], [], np.zeros((0, 4)))
    assert rc == 0 and o["n_fill"] == 0
    rc, _, o = SC.raw_call(pkg, [0, 0, 0], [0], [], np.zeros((0, 4)), interpolate=1)
    assert rc == 0 and o["n_fill"] == 0 and o["seq_links"].tolist() == [0, 0] and o["seq_cost"].tolist() == [0.0, 0.0]
    recs = pkg.evaluation.stitch_tracks([np.zeros((0, 6)), np.zeros((0, 6))])
    assert [r["rows"].shape for r in recs] == [(0, 6), (0, 6)] and recs[0]["links"] == [] and recs[0]["id_map"] == {}
