"""GPU: the CLEAR-MOT assignment of crowded frames.  ``mot_accumulate`` (eval.hip) has its own copy of the compaction that feeds
lap.h's solver (LexCost); test_gpu_eval.py never gives it more than 13 objects a frame.  Here: one-frame sequences (the counts
are exactly that frame's optimum) at each limit of the solver's arrays and one past it, a crowd, the long chain and the
stars, and a two-frame sequence in which the continuation step makes an over-limit frame fit.  The reference is
``eval_ref.mot_ref`` with scipy in place of its pure-Python assignment (shown equal in tests/test_lap_cpu.py)."""
import numpy as np
import pytest

import eval_ref as ER
import lap_ref as LR
from test_gpu_eval import KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def EV():
    import rtmodt_amd
    return rtmodt_amd.evaluation


def ref(g, h):
    return ER.mot_ref(g, h, assign=LR.assign_lex_scipy, weight=LR.max_weight_scipy)


def passing_frames():
    rng = np.random.default_rng(2048)
    crowd = [(2, 2)] * 60 + [(1, 2)] * 40 + [(2, 1)] * 30 + [(1, 1)] * 40
    crowd = [crowd[i] for i in rng.permutation(len(crowd))]
    return {"crowd": (LR.mot_clusters(rng, 1, crowd), (220, 230, 380)),
            "chain256": (LR.mot_chain(rng, 1, 256), (256, 256, 511)),
            "chain255_cols256": (LR.mot_chain(rng, 1, 255, cols=256), (255, 256, 510)),
            "rows256_star": (LR.mot_clusters(rng, 1, [(256, 1)] + [(1, 1)] * 7), (256, 1, 256)),
            "cols256_star": (LR.mot_clusters(rng, 1, [(1, 1)] * 3 + [(1, 256)]), (1, 256, 256)),
            "cols256": (LR.mot_clusters(rng, 1, [(1, 2)] * 128 + [(1, 1)] * 9), (128, 256, 256)),
            "edges2048": (LR.mot_edges(rng, 1, extra=False), (32, 64, 2048))}


def refused_frames():
    rng = np.random.default_rng(2049)
    return {"rows257": (LR.mot_clusters(rng, 5, [(257, 1)]), (257, 1, 257)),
            "cols257": (LR.mot_clusters(rng, 5, [(1, 2)] * 127 + [(1, 3)]), (128, 257, 257)),
            "edges2049": (LR.mot_edges(rng, 5, extra=True), (33, 64, 2049))}


def test_crowded_frames_at_the_limits_equal_reference(EV):
    frames = passing_frames()
    for name, ((g, h), want) in frames.items():
        assert LR.counts(LR.frame_valid(g, h)) == want, name
    got = EV.mot_eval([gh for gh, _ in frames.values()])
    for (name, ((g, h), _)), r in zip(frames.items(), got):
        want = ref(g, h)
        for k in KEYS:
            assert r[k] == want[k], (name, k, r[k], want[k])
        assert abs(r["dist_sum"] - want["dist_sum"]) <= 1e-12 * max(1.0, want["dist_sum"]), name
    assert got[1]["num_matches"] == 256 and got[3]["num_matches"] == 8 and got[6]["num_matches"] == 32


@pytest.mark.parametrize("case", ["rows257", "cols257", "edges2049"])
def test_one_past_each_limit_is_refused_and_names_the_frame(EV, case):
    from rtmodt_amd import _ffi
    (g, h), want = refused_frames()[case]
    assert LR.counts(LR.frame_valid(g, h)) == want
    g1, h1 = LR.mot_clusters(np.random.default_rng(1), 1, [(1, 1), (2, 2)], first_gt=5000, first_hyp=5000)    # ids of its own: no continuation
    ok = (g1, h1)
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.mot_eval([ok, (np.concatenate([g1, g]), np.concatenate([h1, h]))])
    assert e.value.code == _ffi.E_CAPACITY and "sequence 1 frame 5" in e.value.msg, e.value.msg
    r = EV.mot_eval([ok])[0]                                   # the device still answers a valid call
    want = ref(g1, h1)
    for k in KEYS:
        assert r[k] == want[k], k


def test_continuation_makes_an_over_limit_frame_fit(EV):
    """Frame 2 has 129 hypotheses with two GTs each: 258 contested rows, refused by itself.  Frame 1 pairs five of the
    hypotheses with one of their GTs; in frame 2 those five pairs continue (step 1 of the kernel), their hypotheses are
    taken, the five other GTs have nothing left, and 248 contested rows remain."""
    from rtmodt_amd import _ffi
    rng = np.random.default_rng(258)
    g2, h2 = LR.mot_clusters(rng, 2, [(2, 1)] * 129)
    V = LR.frame_valid(g2, h2)
    assert LR.counts(V) == (258, 129, 258)
    g1, h1 = g2[np.isin(g2[:, 1], [1, 3, 5, 7, 9])].copy(), h2[np.isin(h2[:, 1], [1, 2, 3, 4, 5])].copy()
    g1[:, 0] = h1[:, 0] = 1
    assert LR.counts(LR.frame_valid(g1, h1)) == (0, 0, 0) and LR.frame_valid(g1, h1).sum() == 5
    rest = np.ix_(~np.isin(g2[:, 1], [1, 3, 5, 7, 9]), ~np.isin(h2[:, 1], [1, 2, 3, 4, 5]))
    assert LR.counts(V[rest]) == (248, 124, 248)
    with pytest.raises(_ffi.RtmodtError) as e:
        EV.mot_eval([(g2, h2)])
    assert e.value.code == _ffi.E_CAPACITY and "frame 2" in e.value.msg
    g, h = np.concatenate([g1, g2]), np.concatenate([h1, h2])
    r = EV.mot_eval([(g, h)])[0]
    want = ref(g, h)
    for k in KEYS:
        assert r[k] == want[k], (k, r[k], want[k])
    assert r["num_matches"] == 5 + 129 and r["num_switches"] == 0 and r["num_misses"] == 129
