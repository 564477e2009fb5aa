"""CPU: the appearance index's rules without a GPU.  ``tests/index_ref.py`` (the restatement the kernels of ``csrc/index.hip`` are
pinned to) against hand-worked literals and against a brute-force double loop; its similarity against the cross-camera linker's
(``crosscam_ref.sim_matrix``: ppm // 1000 is that per-mille value, so the two modules cannot drift apart); ``csrc/index_rule.h``
against the restatement through ``tests/native/index_rule_check.cpp``, a stand-alone program built plain and with the address /
undefined-behaviour sanitizers (nothing is loaded into Python under a sanitizer); and the shared cases of ``tests/index_cases.py``
on the restatement alone, so that the GPU tests cannot pass by reaching little."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crosscam_ref as CR  # noqa: E402
import index_cases as K  # noqa: E402
import index_ref as R  # noqa: E402
from test_lap_cpu import CSRC, ROOT, host_compilers  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "index_rule_check.cpp")
A = np.asarray([16] * 64, np.int8)
ORTH = np.asarray([16, -16] * 32, np.int8)


def small(capacity=8, **kw):
    return R.IndexRef(64, capacity, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. literals
def test_ppm_worked_values():
    assert R.ppm_of(64 * 256, 64 * 256, 64 * 256) == 1000000                               # an identical row
    assert R.ppm_of(0, 100, 100) == 0 and R.ppm_of(-7, 100, 100) == 0                      # orthogonal, negative
    assert R.ppm_of(50, 100, 100) == 500000
    assert R.ppm_of(99, 100, 99) == 1000000                                                # isqrt(9900) = 99: the floor pushes it to the cap
    assert R.ppm_of(98, 100, 99) == 989898                                                 # 98000000 // 99
    assert R.ppm_of(5, 0, 0) == 1000000                                                    # max(1, isqrt(0))
    assert R.ppm_of(512 * 128 * 128, 512 * 128 * 128, 512 * 128 * 128) == 1000000


def test_identical_orthogonal_and_negative_rows():
    ref = small()
    assert ref.add(np.stack([A, ORTH, -A]), [7, 8, 9], 0, 0, [1, 2, 3]) == 1
    assert ref.search(A[None], [R.filt(1)], 5) == [[(1, 7, 0, 0, 1, 1000000)]]             # rid, key, stream, cls, t, ppm
    assert ref.search(-A[None], [R.filt(1)], 5) == [[(3, 9, 0, 0, 3, 1000000)]]
    assert ref.search(np.zeros((1, 64), np.int8), [R.filt(1)], 5) == [[]]                  # a zero query: every dot is 0


def test_a_zero_row_is_never_eligible():
    ref = small()
    ref.add(np.zeros((1, 64), np.int8), [1], 0, 0, 0)
    assert ref.n2[0] == 0 and ref.search(A[None], [R.filt(1)], 5) == [[]]


def test_tie_in_ppm_is_won_by_the_larger_rid():
    ref = small()
    ref.add(np.stack([A, A, 2 * A, ORTH, A]), [1, 2, 3, 4, 5], 0, 0, 0)                    # 2A has the same direction: 1000000 too
    assert [h[0] for h in ref.search(A[None], [R.filt(1)], 3)[0]] == [5, 3, 2]
    assert [h[0] for h in ref.search(A[None], [R.filt(1)], 8)[0]] == [5, 3, 2, 1]


def test_ring_overwrite():
    ref = small(4)
    for i in range(6):
        assert ref.add(A[None], [10 + i], i, 0, i) == i + 1
    assert ref.rid.tolist() == [5, 6, 3, 4] and ref.next_rid == 7 and len(ref) == 4        # rids 1 and 2 are gone
    assert [h[0] for h in ref.search(A[None], [R.filt(1)], 8)[0]] == [6, 5, 4, 3]
    assert [R.slot_rid(s, 4, 7) for s in range(4)] == [5, 6, 3, 4] and [R.slot_rid(s, 4, 3) for s in range(4)] == [1, 2, 0, 0]
    big = small(4)
    assert big.add(np.stack([A] * 6), np.arange(6), 0, 0, 0) == 1                          # a list longer than the ring
    assert big.rid.tolist() == [5, 6, 3, 4] and big.key.tolist() == [4, 5, 2, 3] and big.next_rid == 7


def test_every_filter_rejects_on_its_own():
    ref = small()
    ref.add(np.stack([A, A, A, A]), [1, 2, 3, 4], [0, 63, 5, 5], [0, 1, 1, 1], [10, 20, 30, 40])
    rids = lambda f: [h[0] for h in ref.search(A[None], [f], 8)[0]]                         # noqa: E731
    assert rids(R.filt(1)) == [4, 3, 2, 1]
    assert rids(R.filt(1, t_range=(20, 30))) == [3, 2]                                     # inclusive at both ends
    assert rids(R.filt(1, streams=[63])) == [2] and rids(R.filt(1, streams=[0, 5])) == [4, 3, 1] and rids(R.filt(1, streams=[])) == []
    assert rids(R.filt(1, cls=0)) == [1] and rids(R.filt(1, cls=2)) == []
    assert rids(R.filt(1, exclude_key=3)) == [4, 2, 1]
    assert ref.forget([2, 4, 99]) == 2 and rids(R.filt(1)) == [3, 1] and ref.forget([2]) == 0
    half = np.asarray([16] * 32 + [0] * 32, np.int8)                                       # cos = 1 / sqrt 2: 10^6 * 8192 // isqrt(16384 * 8192) = 8192000000 // 11585
    assert R.ppm_of(32 * 256, 64 * 256, 32 * 256) == 707121
    assert ref.search(half[None], [R.filt(707121)], 8)[0][0][5] == 707121 and ref.search(half[None], [R.filt(707122)], 8) == [[]]
    assert ref.search(A[None], [R.filt(0)], 8) == R.E_INVALID and ref.search(A[None], [R.filt(1)], 65) == R.E_INVALID


def test_refusals_change_nothing_and_load_checks_its_input():
    ref = small(4, max_add=3)
    ref.add(np.stack([A, A]), [1, 2], 0, 0, 0)
    before = ref.snapshot()
    assert ref.add(np.stack([A] * 4), [1] * 4, 0, 0, 0) == R.E_INVALID                     # n > max_add
    assert ref.add(A[None], [1], 64, 0, 0) == R.E_INVALID and ref.add(A[None], [1], -1, 0, 0) == R.E_INVALID
    assert R.snapshots_equal(ref.snapshot(), before) is None
    for field, slot, value in (("rid", 0, 2), ("rid", 2, 3), ("rid", 1, 6), ("stream", 0, 64), ("dead", 1, 2)):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
        bad[field][slot] = value
        assert ref.load(bad) == R.E_INVALID and R.snapshots_equal(ref.snapshot(), before) is None, field
    other = small(4)
    assert other.load(before) is None and R.snapshots_equal(other.snapshot(), before) is None


def test_chunk_rows_rule():
    assert R.chunk_rows(1000) == 64 and R.chunk_rows(16384) == 64 and R.chunk_rows(16385) == 128 and R.chunk_rows(20000) == 128
    assert R.chunk_rows(1 << 20) == 4096 and R.chunk_rows(1 << 22) == 16384
    assert R.chunk_rows(129, 64) == 64 and R.chunk_rows(16385, 64) == 0 and R.chunk_rows(1000, 96) == 0 and R.chunk_rows(0) == 0


# ---------------------------------------------------------------------------------------------------------------- 2. brute force
@pytest.mark.parametrize("seed", range(4))
def test_search_equals_a_double_loop(seed):
    rng = np.random.default_rng(seed)
    n, cap = int(rng.integers(20, 90)), int(rng.integers(16, 60))
    ref = R.IndexRef(64, cap, chunk_rows_req=64)
    rows = rng.integers(-128, 128, (n, 64)).astype(np.int8)
    rows[rng.integers(0, n, 6)] = rows[0]                                                   # ties
    K.fill(ref, rows, K.metadata(n, seed), batch=17)
    ref.forget([1003, 1017])
    queries = np.stack([rows[0], rows[n - 1], rng.integers(-128, 128, 64).astype(np.int8)])
    for f in (R.filt(1), R.filt(300000, t_range=(110, 160)), R.filt(1, streams=range(0, 64, 2), cls=1, exclude_key=int(ref.key[0]))):
        for k in (1, 5, 64):
            assert ref.search(queries, [f] * 3, k) == [R.brute_force(ref, q, f, k) for q in queries]


# ---------------------------------------------------------------------------------------------------------------- 3. against crosscam
def test_ppm_agrees_with_the_linkers_similarity():
    rng = np.random.default_rng(5)
    for dim in (64, 512):
        q, t = rng.integers(-128, 128, (40, dim)).astype(np.int8), rng.integers(-128, 128, (50, dim)).astype(np.int8)
        q[0], t[0], q[1], t[1], t[2] = -128, -128, 127, 127, 0
        t[3:10] = np.clip(q[3:10].astype(np.int32) + rng.integers(-9, 10, (7, dim)), -128, 127)       # near pairs: sims near 1000
        dots = q.astype(np.int32) @ t.astype(np.int32).T
        nq, nt = (q.astype(np.int64) ** 2).sum(axis=1), (t.astype(np.int64) ** 2).sum(axis=1)
        ppm = R.ppm_matrix(dots, nq, nt)
        assert np.array_equal(ppm // 1000, CR.sim_matrix(dots, nq, nt))
        assert ppm[0, 0] == 1000000 and ppm[1, 1] == 1000000 and ppm[0, 1] == 0 and (ppm[:, 2] == 0).all()
        assert all(int(ppm[i, j]) == R.ppm_of(dots[i, j], nq[i], nt[j]) for i in range(40) for j in range(0, 50, 7))


# ---------------------------------------------------------------------------------------------------------------- 4. the header
def build(tmp_path, sanitize):
    exe = str(tmp_path / ("index_rule_check_san" if sanitize else "index_rule_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built index_rule_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def requests():
    """-> (the program's input, the restatement's answers)."""
    rng = np.random.default_rng(9)
    req, want = [], []
    for dot, nq, n2 in [(50, 100, 100), (0, 1, 1), (-5, 9, 9), (99, 100, 99), (98, 100, 99), (5, 0, 0), (512 * 128 * 128,) * 3, (2 ** 31 - 1, 1, 1)] + \
            [(int(rng.integers(-10 ** 6, 2 ** 23)), int(rng.integers(0, 2 ** 23)), int(rng.integers(0, 2 ** 23))) for _ in range(300)]:
        req.append(f"ppm {dot} {nq} {n2}")
        want.append(f"{R.ppm_of(dot, nq, n2)} {R.ppm_of(dot, nq, n2) // 1000}")       # beside it the header prints cc_sim of crosscam_rule.h
    for rid, cap in [(1, 1), (1, 4), (4, 4), (5, 4), (2 ** 40 - 1, 1 << 22), (2 ** 40 - 1, 1000)]:
        req.append(f"slot {rid} {cap}")
        want.append(str((rid - 1) % cap))
    for cap, nxt in [(4, 1), (4, 3), (4, 5), (4, 7), (7, 100), (1, 9)]:
        for s in range(cap):
            req.append(f"slotrid {s} {cap} {nxt}")
            want.append(str(R.slot_rid(s, cap, nxt)))
    for cap, rq in [(1000, 0), (16384, 0), (16385, 0), (1 << 22, 0), (129, 64), (16385, 64), (1000, 96), (0, 0), ((1 << 22) + 1, 0), (100, -64)]:
        req.append(f"chunk {cap} {rq}")
        want.append(str(R.chunk_rows(cap, rq)))
    for ppm, rid in [(1, 1), (1000000, 2 ** 40 - 1), (707121, 12345)]:
        req.append(f"rank {ppm} {rid}")
        want.append(f"{ppm << 40 | rid} {ppm} {rid}")
    for seed in range(3):                                  # whole searches: the brute force of the header against the restatement's
        r2 = np.random.default_rng(100 + seed)
        n, cap, k = 70, 50, (1, 5, 64)[seed]
        ref = R.IndexRef(64, cap, chunk_rows_req=64)
        rows = r2.integers(-128, 128, (n, 64)).astype(np.int8)
        rows[r2.integers(0, n, 8)] = rows[n - 1]
        K.fill(ref, rows, K.metadata(n, seed), batch=23)
        ref.forget([1001, 1002])
        queries = np.stack([rows[n - 1], r2.integers(-128, 128, 64).astype(np.int8), np.zeros(64, np.int8)])
        fs = [R.filt(1), R.filt(200000, t_range=(125, 165), streams=range(1, 64), cls=2, exclude_key=1005), R.filt(1)]
        req.append(f"search 64 {cap} 3 {k}")
        for s in range(cap):
            req.append(" ".join(str(int(v)) for v in (ref.rid[s], ref.dead[s], ref.t[s], ref.stream[s], ref.cls[s], ref.key[s], *ref.rows[s])))
        for q, f in zip(queries, fs):
            req.append(" ".join(str(int(v)) for v in (f["t0"], f["t1"], f["mask"], f["cls"], f["excl"], f["min_ppm"], *q)))
        for hits in ref.search(queries, fs, k):
            want.append(" ".join([str(len(hits))] + [f"{h[0]}:{h[5]}" for h in hits]))
    return "\n".join(req) + "\n", want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_rule_header_equals_the_restatement(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    text, want = requests()
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want


# ---------------------------------------------------------------------------------------------------------------- 5. the shared cases
def loaded(case):
    kw, rows, meta, queries, filters = case
    ref = R.IndexRef(kw["dim"], kw["capacity"], chunk_rows_req=kw["chunk_rows"])
    K.fill(ref, rows, meta, batch=300)
    return ref, queries, filters


def test_selection_case_reaches_what_it_is_meant_to():
    ref, queries, filters = loaded(K.selection())
    assert ref.chunk == 64 and -(-ref.N // ref.chunk) == 16
    res16, res64 = ref.search(queries, filters, 16), ref.search(queries, filters, 64)
    # more eligible rows than k inside a single chunk (so a buffer of 2k = 32 overflows there, more than once where there are > 48)
    per = K.eligible_per_chunk(ref, queries[0], filters[0])
    assert max(per) > 16 and sum(1 for v in per if v > 16) >= 8
    # the 40 duplicates tie at 1000000 ppm over 14 chunks, in pairs across chunk boundaries, and rid alone orders them
    assert [h[5] for h in res64[1]] == [1000000] * 40 and [h[0] for h in res64[1]] == sorted((s + 1 for s in K.DUP_SLOTS), reverse=True)
    assert len({K.chunk_of(ref, h[0]) for h in res64[1]}) >= 3 and len({K.chunk_of(ref, h[0]) for h in res16[0]}) >= 3
    assert any(K.chunk_of(ref, a[0]) != K.chunk_of(ref, b[0]) and a[5] == b[5] and a[0] == b[0] + 1 for a, b in zip(res16[0], res16[0][1:]))
    assert len(res16[1]) == 16 and 1 <= len(res64[1]) <= 63                                # 40 of 64: a short answer
    assert 1 <= len(res16[2]) <= 15 and res16[2][0][0] == 78                               # the noisy copy of row 77 finds it (rid 78)
    assert res16[3] == [] and res64[3] == []                                               # the zero query: none
    assert len(res64[4]) == 64 and 1 <= len(res64[5]) <= 63
    assert all(61 <= h[0] <= 701 and h[3] == 1 for h in res64[5])


def test_crowded_case_overflows_a_buffer_of_128_inside_a_chunk():
    ref, queries, filters = loaded(K.crowded())
    per = K.eligible_per_chunk(ref, queries[0], filters[0])
    assert len(per) == 2 and min(per) > 112 + 3 * 64                                       # k = 64: at least four compactions per chunk
    res = ref.search(queries, filters, 64)
    assert len(res[0]) == 64 and len(res[1]) == 64 and res[2] == []
