"""CPU: the cross-camera linker's rules without a GPU.  ``tests/crosscam_ref.py`` (the restatement the kernels of
``csrc/crosscam.hip`` are pinned to) against hand-worked literals; ``csrc/crosscam_rule.h`` against the restatement through
``tests/native/crosscam_rule_check.cpp``, a stand-alone program built plain and with the address / undefined-behaviour sanitizers
(nothing is loaded into Python under a sanitizer); the generator of the GPU test's random site, on the restatement alone."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import botsort_ref as BR  # noqa: E402
import crosscam_cases as K  # noqa: E402
import crosscam_ref as R  # noqa: E402
import lap_ref as LR  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "crosscam_rule_check.cpp")
B, L, J, N = R.BOUND, R.LINKED, R.JOINED, R.BORN


def flat(out, key):
    return [v for s in out[key] for v in s]


# ---------------------------------------------------------------------------------------------------------------- 1. literals
def test_sim_worked_pairs():
    assert R.sim_milli(50, 100, 100) == 500
    assert R.sim_milli(0, 100, 100) == 0 and R.sim_milli(-7, 100, 100) == 0                # dot <= 0
    # cos = 99 / sqrt(9900) = 0.99499; isqrt(9900) = 99 (99.4987 floored), so 1000 * 99 / 99 = 1000: the floor pushes it to the cap
    assert R.sim_milli(99, 100, 99) == 1000
    assert R.sim_milli(3, 2, 4) == 1000                                                    # 1500 before the cap
    assert R.sim_milli(5, 0, 0) == 1000                                                    # max(1, isqrt(0))
    assert R.sim_rows(K.A, [16] * 64) == 1000 and R.sim_rows(K.A2, [16] * 64) == 990
    p = np.asarray([0, 1, 2, 3, 4, 8, 9, 15, 16, 17, 9899, 9900, 9801, (512 * 128 * 128) ** 2, (512 * 128 * 128) ** 2 - 1], np.int64)
    assert R.isqrt_vec(p).tolist() == [0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 99, 99, 99, 512 * 128 * 128, 512 * 128 * 128 - 1]


def test_handoff_and_transit_window():
    _, outs = K.run_ref(K.handoff())
    assert (outs[0]["gid"], outs[0]["status"], outs[0]["events"]) == ([[1], []], [[N], []], [])
    assert all(o["gid"] == [[], []] and o["events"] == [] for o in outs[1:5])
    assert (outs[5]["gid"], outs[5]["status"], outs[5]["sim"]) == ([[], [1]], [[], [L]], [[], [1000]])
    assert outs[5]["events"] == [(1, 1, 3, 0, 5, 1000)]                                    # gid, stream, local id, from_stream, gap, sim
    ref, outs = K.run_ref(K.handoff(6))                                                    # tmin[0][1] = 6 > the gap of 5
    assert (outs[5]["gid"], outs[5]["status"], outs[5]["events"]) == ([[], [2]], [[], [N]], [])
    assert [g.gid for g in ref.table] == [1, 2]


def test_overlapping_streams_join_on_the_first_call():
    ref, outs = K.run_ref(K.overlap())
    assert (outs[0]["gid"], outs[0]["status"], outs[0]["sim"]) == ([[1], [1]], [[N], [J]], [[0], [1000]])
    assert outs[0]["events"] == [(1, 1, 5, 0, 0, 1000)]
    assert len(ref.table) == 1 and ref.table[0].last_seen == [1, 1]
    assert ref.table[0].s8 == R.feat_step(R.feat_step(None, K.A)[0], K.A)[1]               # the founder's row, then the joiner's
    ref, outs = K.run_ref(K.overlap(1))                                                    # disjoint views: two identities
    assert (outs[0]["gid"], outs[0]["status"], outs[0]["events"]) == ([[1], [2]], [[N], [N]], [])


def test_two_near_equal_queries_for_one_identity():
    ref, outs = K.run_ref(K.near_equal())
    assert (outs[1]["gid"], outs[1]["status"], outs[1]["sim"]) == ([[], [2, 1]], [[], [N, L]], [[], [0, 1000]])     # 990 loses to 1000
    assert outs[1]["events"] == [(1, 1, 11, 0, 1, 1000)]
    assert ref.ledgers[1] == {10: [2, 2], 11: [1, 2]}


def test_best_pair_first_loses_to_the_optimum():
    ref, outs = K.run_ref(K.greedy_loses())
    # gains over min_sim 400: (20, g1) 601, (20, g2) 186, (21, g1) 499; taking 601 first leaves 21 with nothing: 186 + 499 > 601
    assert R.sim_rows(K.G1, R.feat_step(None, K.G1)[1]) == 1000
    assert (outs[1]["gid"], outs[1]["status"], outs[1]["sim"]) == ([[], [2, 1]], [[], [L, L]], [[], [585, 898]])
    assert outs[1]["events"] == [(2, 1, 20, 0, 1, 585), (1, 1, 21, 0, 1, 898)]


def test_matching_objective_equals_scipy_on_random_sparse_gains():
    rng = np.random.default_rng(42)
    for _ in range(200):
        nr, nc = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        gain = np.where(rng.random((nr, nc)) < 0.35, rng.integers(1, 302, (nr, nc)), 0)
        x, ok = R.max_gain_rows(gain)
        assert ok
        cols = [c for c in x if c >= 0]
        assert len(set(cols)) == len(cols) and all(gain[r, c] > 0 for r, c in enumerate(x) if c >= 0)
        assert sum(int(gain[r, c]) for r, c in enumerate(x) if c >= 0) == LR.max_weight_scipy(gain)


def test_fragmented_local_track():
    ref, outs = K.run_ref(K.fragment())
    assert (outs[1]["gid"], outs[1]["status"], outs[1]["events"]) == ([[1]], [[L]], [(1, 0, 9, 0, 1, 1000)])
    assert (outs[2]["gid"], outs[2]["status"]) == ([[2, 1]], [[N, B]])                    # 7 comes back: a query again, 1 is live here
    assert ref.ledgers[0] == {7: [2, 3], 9: [1, 3]}
    r2 = R.CrossCamRef(**K.fragment()[0])
    r2.process(K.fragment()[2][0])
    r2.process(K.fragment()[2][1])
    assert r2.ledgers[0] == {9: [1, 2]}                                                     # the old binding 7 -> 1 is gone


def test_retirement_and_gids_never_reused():
    ref, outs = K.run_ref(K.retirement())
    assert [o["retired"] for o in outs] == [[], [], [], [], [(1, 1, 1, 1)], []]            # c - last_seen = 4 > max_age 3 at call 5
    assert (outs[5]["gid"], outs[5]["status"]) == ([[2]], [[N]])
    assert [g.gid for g in ref.table] == [2] and ref.next_gid == 3 and ref.ledgers[0] == {2: [2, 6]}


def test_full_table():
    ref, outs = K.run_ref(K.full_table())
    assert (outs[0]["gid"], outs[0]["status"]) == ([[1, 2, 0]], [[N, N, R.TABLE_FULL]])
    assert ref.counters["n_table_full"] == 1 and ref.counters["n_identities"] == 2 and 3 not in ref.ledgers[0]


def test_deferral_past_max_queries():
    ref, outs = K.run_ref(K.deferral())
    assert (outs[0]["gid"], outs[0]["status"]) == ([[1, 2], [0]], [[N, N], [R.DEFERRED]])
    assert (outs[1]["gid"], outs[1]["status"], outs[1]["events"]) == ([[1, 2], [1]], [[B, B], [L]], [(1, 1, 5, 0, 1, 1000)])
    assert ref.counters["n_deferred"] == 0 and ref.counters["n_queries"] == 1


def test_lap_limit_error():
    ref, outs = K.run_ref(K.lap_limit())
    assert flat(outs[0], "status") == [N] * 50 and flat(outs[0], "gid") == list(range(1, 51))
    for o in outs[1:]:
        assert o["status"] == [[B] * 50, [R.UNBOUND] * 50] and o["gid"][1] == [0] * 50 and o["events"] == []
    assert ref.err == [0, 2] and ref.ledgers[1] == {} and len(ref.table) == 50 and ref.next_gid == 51


def test_duplicate_ids_are_refused():
    ref = R.CrossCamRef(1, 64)
    assert ref.process([K.entries((1, 0, K.A), (1, 0, K.A2))]) == R.E_INVALID and ref.c == 0


def test_feature_update_equals_botsort():
    rng = np.random.default_rng(3)
    for dim in (64, 192, 512):
        s16 = None
        for _ in range(6):
            f = rng.integers(-128, 128, dim)
            a, b = R.feat_step(s16, f), BR.feat_step(s16, f)
            assert a == (list(b[0]), list(b[1]))
            s16 = a[0]
    assert R.feat_step(None, [0] * 64) == ([0] * 64, [0] * 64)
    assert R.FEAT_NORM == BR.FEAT_NORM


# ---------------------------------------------------------------------------------------------------------------- 2. the generator
def test_random_site_generator():
    frames, truth, base = R.random_site()
    rows = {p: [] for p in range(len(base))}
    for fr, tr in zip(frames, truth):
        for (_, _, r), who in zip(fr, tr):
            for row, p in zip(r, who):
                rows[p].append(row)
    assert all(len(v) >= 2 for v in rows.values())
    for p, v in rows.items():
        assert min(R.sim_rows(a, b) for a in v[:6] for b in v[-6:]) >= 850
        for q in range(p):
            assert max(R.sim_rows(a, b) for a in v[:4] for b in rows[q][:4]) <= 500
    ref = R.CrossCamRef(3, 64)
    ref.set_transit(0, 2, 1, 0)
    ref.set_transit(2, 0, 2, 300)
    person_gids, gid_people = {}, {}
    n_links = 0
    for fr, tr in zip(frames, truth):
        out = ref.process(fr)
        n_links += len(out["events"])
        for s in range(3):
            for g, p in zip(out["gid"][s], tr[s]):
                assert g > 0
                person_gids.setdefault(p, set()).add(g)
                gid_people.setdefault(g, set()).add(p)
    assert all(len(v) == 1 for v in person_gids.values()) and all(len(v) == 1 for v in gid_people.values())
    assert len(person_gids) == 12 and n_links >= 12 and ref.err == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 3. the header
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("crosscam_rule_check_san" if sanitize else "crosscam_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built crosscam_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def requests():
    """-> (the program's input, the restatement's answers)."""
    rng = np.random.default_rng(9)
    req, want = [], []
    for dot, nq, ng in [(50, 100, 100), (0, 1, 1), (-5, 9, 9), (99, 100, 99), (3, 2, 4), (5, 0, 0), (512 * 128 * 128, 512 * 128 * 128, 512 * 128 * 128),
                        (2 ** 31 - 1, 1, 1)] + [(int(rng.integers(-10 ** 6, 10 ** 7)), int(rng.integers(0, 2 ** 23)), int(rng.integers(0, 2 ** 23))) for _ in range(300)]:
        req.append(f"sim {dot} {nq} {ng}")
        want.append(str(R.sim_milli(dot, nq, ng)))
    for n in [0, 1, 2, 3, 4, 2 ** 46, 2 ** 46 - 1, (2 ** 23) ** 2 + 1, 2 ** 62, 2 ** 63 - 1] + [int(v) for v in rng.integers(0, 2 ** 62, 50)]:
        req.append(f"isqrt {n}")
        want.append(str(math.isqrt(n)))
    for c, last, lo, hi in [(6, 1, 0, 300), (6, 1, 6, 300), (6, 1, 5, 5), (6, 0, 0, 300), (6, 6, 0, -1), (6, 6, 0, 0), (9, 3, 1, 5), (9, 3, 7, 5)]:
        req.append(f"transit {c} {last} {lo} {hi}")
        want.append("1" if last > 0 and lo <= c - last <= hi else "0")
    for dim in (64, 192, 512):
        s16 = None
        for k in range(5):
            f = rng.integers(-128, 128, dim) if k != 3 else np.full(dim, -128)
            req.append(f"feat {1 if s16 is None else 0} {dim} " + " ".join(str(v) for v in (s16 or [0] * dim)) + " " + " ".join(str(int(v)) for v in f))
            s16, s8 = R.feat_step(s16, f)
            want.append(" ".join(str(v) for v in s16 + s8))
    req.append("feat 1 64 " + " ".join(["0"] * 128))
    want.append(" ".join(["0"] * 128))
    return "\n".join(req) + "\n", want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_rule_header_equals_the_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    text, want = requests()
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want
