"""GPU: rtmodt_amd.evaluation.hota_eval (csrc/hota.hip) against the restatement tests/hota_ref.py, which shares no code
with it and is itself checked against hand-worked literals and scipy in tests/test_hota_cpu.py.  Integers are compared with
==, doubles bit for bit through .view(np.int64).  The cases are the smallest that reach each mechanism."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hota_ref as HR  # noqa: E402
import lap_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

INTS = ("HOTA_TP", "HOTA_FN", "HOTA_FP")
SUMS = ("loc_sum", "ass_a_sum", "ass_re_sum", "ass_pr_sum")


@pytest.fixture(scope="module")
def EV(pkg):
    return pkg.evaluation


def same(got, want, what=""):
    """One record of hota_eval against the restatement's record: exact."""
    for k in INTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in SUMS + HR.FLOAT_FIELDS:
        g, w = np.ascontiguousarray(got[k], np.float64), np.ascontiguousarray(want[k], np.float64)
        assert np.array_equal(g.view(np.int64), w.view(np.int64)), (what, k, g, w)
    assert got["mean"] == want["mean"], what
    for k in ("HOTA(0)", "LocA(0)", "HOTALocA(0)"):
        assert got[k] == want[k], (what, k)


def adjacency(fr):
    a = np.zeros((fr["nO"], fr["nH"]), bool)
    for i, j, _ in fr["edges"]:
        a[i, j] = True
    return a


def drop_frame(rows, frame):
    return rows[rows[:, 0] != frame]


@pytest.fixture(scope="module")
def several():
    """Three sequences of 30-40 frames with 5-12 objects (drift, misses, false positives, id switches, two fragments per
    object) with a frame without GT, one without hypotheses and one with neither, and a sequence with no hypotheses at all;
    the restatement's sums, computed once."""
    rng = np.random.default_rng(2021)
    seqs = []
    for n_frames, n_obj in ((30, 5), (36, 9), (40, 12)):
        g, h = HR.synth_sequence(rng, n_frames, n_obj)
        g = drop_frame(drop_frame(g, 12), 20)                  # frame 12: no GT; frame 20: neither; frame 16: no hypotheses
        h = drop_frame(drop_frame(h, 16), 20)
        assert len(g[g[:, 0] == 16]) and len(h[h[:, 0] == 12])
        seqs.append((g, h))
    seqs.append((HR.synth_sequence(rng, 30, 5)[0], np.zeros((0, 6))))
    return seqs, [HR.hota_ref(g, h) for g, h in seqs]


def test_several_sequences_in_one_call(EV, several):
    seqs, want = several
    got = EV.hota_eval(seqs)
    assert len(got["sequences"]) == 4 and np.array_equal(got["alphas"], HR.ALPHAS)
    for s, (r, c) in enumerate(zip(got["sequences"], want)):
        same(r, HR.record(c), f"sequence {s}")
    same(got["combined"], HR.combine(want), "combined")
    assert all(0 < w["HOTA_TP"][0] and w["HOTA_TP"][-1] < w["HOTA_TP"][0] and w["HOTA_FP"][0] > 0 for w in want[:3])
    assert not want[3]["HOTA_TP"].any() and want[3]["HOTA_FN"][0] == len(seqs[3][0])
    assert any(len(HR.split_edges(fr["edges"])[1]) for w in want for fr in w["frames"])      # the solver ran


def test_each_sequence_alone_equals_its_record_in_the_batch(EV, several):
    """The key bases, the id-count slices and the row offsets of a batch: every sequence's record is that of the sequence alone."""
    seqs, want = several
    for s in (1, 2, 3):
        same(EV.hota_eval([seqs[s]])["sequences"][0], HR.record(want[s]), f"sequence {s} alone")


def test_a_frame_wider_than_one_wave_pass(EV):
    """70 GT x 70 hypotheses on a jittered grid with overlapping neighbours: 4900 candidate pairs (77 passes of a wave), rows
    beyond one wave in the sums, one connected contested component."""
    rng = np.random.default_rng(70)
    cx, cy = np.meshgrid(np.arange(10) * 70.0, np.arange(7) * 70.0)
    base = np.stack([cx.ravel(), cy.ravel(), np.full(70, 100.0), np.full(70, 100.0)], 1)
    g, h = [], []
    for f in (1, 2, 3):
        perm = rng.permutation(70) if f == 3 else np.arange(70)                # frame 3: other ids on the same places
        g.append(np.column_stack([np.full(70, f), np.arange(70) + 1, base + rng.uniform(-6, 6, (70, 4))]))
        h.append(np.column_stack([np.full(70, f), perm + 1, base + rng.uniform(-6, 6, (70, 4))]))
    g, h = np.concatenate(g), np.concatenate(h)
    want = HR.hota_ref(g, h)
    for fr in want["frames"]:
        nr, nc, ne = LR.counts(adjacency(fr))
        assert (fr["nO"], fr["nH"]) == (70, 70) and nr == 70 and nc == 70 and 500 < ne <= LR.LAP_EDGES
    same(EV.hota_eval([(g, h)])["sequences"][0], HR.record(want))


def test_a_contested_component_inside_the_limits(EV):
    """A planted overlapping cluster of 100 GT rows and 100 hypothesis rows in a line, each overlapping about 10 of the other
    side, among isolated pairs: the contested counts are asserted first, so the case cannot pass by missing its target."""
    rng = np.random.default_rng(100)
    n = 100
    g, h = [], []
    for f in (1, 2):
        gx = 20.0 * np.arange(n) + rng.uniform(-3, 3, n)
        hx = 20.0 * np.arange(n) + rng.uniform(-3, 3, n)
        far = 5000.0 + 300.0 * np.arange(30)
        g.append(np.column_stack([np.full(n + 30, f), np.arange(n + 30) + 1, np.concatenate([gx, far]), rng.uniform(-3, 3, n + 30),
                                  np.full(n + 30, 100.0), np.full(n + 30, 60.0)]))
        h.append(np.column_stack([np.full(n + 30, f), np.arange(n + 30) + 1, np.concatenate([hx, far + rng.uniform(-5, 5, 30)]),
                                  rng.uniform(-3, 3, n + 30), np.full(n + 30, 100.0), np.full(n + 30, 60.0)]))
    g, h = np.concatenate(g), np.concatenate(h)
    want = HR.hota_ref(g, h)                                   # raises hota_ref.Capacity outside 256 / 256 / 2048
    for fr in want["frames"]:
        nr, nc, ne = LR.counts(adjacency(fr))
        assert (nr, nc) == (100, 100) and 800 <= ne <= LR.LAP_EDGES, (nr, nc, ne)
        assert LR.within_limits(adjacency(fr)) and len(fr["edges"]) == ne + 30
    same(EV.hota_eval([(g, h)])["sequences"][0], HR.record(want))


def test_ties(EV):
    """Identical boxes for several ids (every score of a cluster equal) and integer-grid boxes: all outputs exact."""
    rng = np.random.default_rng(5)
    tg, th = HR.tie_sequence(rng, 16, 3, 4)
    gg, gh = HR.synth_sequence(rng, 16, 8, jitter=8.0, fp=0.4, grid=20.0)
    gh = np.concatenate([gh, gh[::2] + np.array([0, 1000, 20.0, 0, 0, 0])])
    want = [HR.hota_ref(tg, th), HR.hota_ref(gg, gh)]
    sc = [e[2] for fr in want[0]["frames"] for e in fr["edges"]]
    assert len(sc) - len(set(sc)) > 500
    assert any(len(HR.split_edges(fr["edges"])[1]) >= 4 for fr in want[0]["frames"])
    got = EV.hota_eval([(tg, th), (gg, gh)])
    for r, c in zip(got["sequences"], want):
        same(r, HR.record(c))
    same(got["combined"], HR.combine(want))


def test_pmc_is_summed_in_frame_order(EV):
    """One (o, h) pair meeting in 200 frames with distinct IoUs; a second hypothesis id overlaps the GT in every frame, so each
    frame's q is a different number below 1 and the matching's scores carry pmc's last bit.  The reversed sum differs: asserted
    on the CPU side first."""
    rng = np.random.default_rng(200)
    F = 200
    g = np.column_stack([np.arange(F) + 1.0, np.ones(F), np.zeros(F), np.zeros(F), np.full(F, 100.0), np.full(F, 100.0)])
    h = g.copy()
    h[:, 4] = 100.0 - rng.uniform(1, 60, F)                    # IoU = width / 100, distinct
    h2 = g.copy()
    h2[:, 1] = 2.0
    h2[:, 2] = 50.0 + rng.uniform(0, 30, F)
    hyp = np.concatenate([h, h2])
    want = HR.hota_ref(g, hyp)
    q = []
    for fr in want["frames"]:
        S = fr["S"]
        r = sum(s for (i, j), s in S.items())
        c = S[(0, 0)]
        q.append(S[(0, 0)] / ((r + c) - S[(0, 0)]))
    fwd = 0.0
    for x in q:
        fwd += x
    rev = 0.0
    for x in reversed(q):
        rev += x
    assert fwd == want["pmc"][(1.0, 1.0)] and fwd != rev and abs(fwd - rev) < 1e-12
    assert len(set(q)) == F
    same(EV.hota_eval([(g, hyp)])["sequences"][0], HR.record(want))


def test_limits_are_refused_cleanly(EV):
    """257 mutually overlapping rows per side: a capacity error naming the sequence and frame; 1025 rows in a frame: refused
    before launch.  Argument checks, and the device answers a valid call afterwards."""
    from rtmodt_amd import _ffi
    rng = np.random.default_rng(257)
    g, h = LR.mot_clusters(rng, 5, [(257, 257)])
    adj = np.array([[HR.box_iou(a[2:], b[2:]) > 0 for b in h] for a in g])
    assert LR.counts(adj) == (257, 257, 257 * 257)
    g1, h1 = LR.mot_clusters(np.random.default_rng(1), 1, [(1, 1), (2, 2)], first_gt=5000, first_hyp=5000)
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.hota_eval([(g1, h1), (np.concatenate([g1, g]), np.concatenate([h1, h]))])
    assert e.value.code == _ffi.E_CAPACITY and "sequence 1 frame 5" in e.value.msg, e.value.msg
    wide = np.column_stack([np.full(1025, 3.0), np.arange(1025) + 1.0, 300.0 * np.arange(1025), np.zeros(1025), np.full(1025, 50.0),
                            np.full(1025, 50.0)])
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.hota_eval([(g1, h1), (wide, h1)])
    assert e.value.code == _ffi.E_CAPACITY and "sequence 1 frame 3" in e.value.msg and "1025" in e.value.msg, e.value.msg
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.hota_eval([(g1, h1)], alphas=np.linspace(0.01, 0.99, 33))
    assert e.value.code == _ffi.E_CAPACITY
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.hota_eval([(g1, h1)], alphas=[0.5, 0.25])
    assert e.value.code == _ffi.E_INVALID
    same(EV.hota_eval([(g1, h1)])["sequences"][0], HR.record(HR.hota_ref(g1, h1)))


def test_empty_input_and_one_alpha(EV, several):
    got = EV.hota_eval([])
    assert got["sequences"] == [] and not got["combined"]["HOTA_TP"].any() and len(got["combined"]["HOTA"]) == 19
    seqs, _ = several
    g, h = seqs[0]
    for al in ([0.5], [0.3, 0.30000000000000004, 0.9]):
        got = EV.hota_eval([(g, h)], alphas=al)
        want = HR.hota_ref(g, h, al)
        same(got["sequences"][0], HR.record(want))
        assert len(got["sequences"][0]["HOTA"]) == len(al) and want["HOTA_TP"][0] > 0
    assert EV.hota_eval([(np.zeros((0, 6)), np.zeros((0, 6)))])["sequences"][0]["HOTA_FN"].tolist() == [0] * 19


def test_stitching_raises_association_not_detection(EV):
    """The metric does its job: tracks split into two ids each, exact boxes.  stitch_tracks joins them: DetA is unchanged bit
    for bit and AssA rises at every alpha to 1."""
    rng = np.random.default_rng(9)
    gt, _ = HR.synth_sequence(rng, 30, 6, split=False)
    hyp = gt.copy()
    for o in np.unique(gt[:, 1]):
        fr = gt[gt[:, 1] == o, 0]
        late = (hyp[:, 1] == o) & (hyp[:, 0] > fr[len(fr) // 2])
        hyp[late, 1] = 100 + o
    assert len(np.unique(hyp[:, 1])) == 12
    before = EV.hota_eval([(gt, hyp)])["sequences"][0]
    st = EV.stitch_tracks([hyp], max_gap=2, max_dist=20.0, interpolate=False)[0]
    assert st["n_tracks_after"] == 6 and len(st["rows"]) == len(hyp)
    after = EV.hota_eval([(gt, st["rows"])])["sequences"][0]
    assert np.array_equal(before["DetA"].view(np.int64), after["DetA"].view(np.int64)) and np.array_equal(before["DetA"], np.ones(19))
    assert np.all(before["AssA"] < 1.0) and np.all(after["AssA"] > before["AssA"]) and np.array_equal(after["AssA"], np.ones(19))
    assert np.array_equal(after["HOTA"], np.ones(19))
    same(before, HR.record(HR.hota_ref(gt, hyp)))
