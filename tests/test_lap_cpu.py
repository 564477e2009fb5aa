"""``csrc/lap.h``'s ``lap_solve`` -- the one exact assignment solver behind the tracker's lapjv branch, both DeepSORT stages, the
CLEAR-MOT assignment and the IDF1 pairing -- is ``__host__ __device__``; ``tests/native/lap_check.cpp`` runs it on the host for
``double``, ``LexCost`` and ``long long`` with every solver array allocated at exactly its documented size: against every matching on
small graphs, against its own duals on limit-sized and long-path graphs, and (here) against scipy on generic double costs.  The
program is built twice, plain and with the address / undefined-behaviour sanitizers; it runs by itself (no GPU)."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "real-time-multi-object-detection---tracking-system_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "lap_check.cpp")
FAMILIES = 10                                                  # per cost type, see lap_check.cpp's check_type


def rocm_root():
    for r in (os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"):
        if r and os.path.isfile(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return r
    raise AssertionError("no ROCm headers (hip/hip_runtime.h) found")


def host_compilers(sanitize):
    """Compilers to try, in order: g++ first for the plain build; for the sanitizer build whichever links its runtime."""
    rocm = rocm_root()
    clang = [p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.isfile(p)]
    gxx = [p for p in (shutil.which("g++"),) if p]
    return clang + gxx if sanitize else gxx + clang


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("lap_check_san" if sanitize else "lap_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        cmd = [cxx, "-x", "c++", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(rocm_root(), "include"), SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built lap_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def generic_problems():
    """Sparse problems with generic double costs in (-1, 0): many small ones, some at the solver's limits."""
    rng = np.random.default_rng(20240611)
    probs = []
    for _ in range(60):
        nr, nc = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        adj = rng.random((nr, nc)) < rng.uniform(0.05, 0.6)
        probs.append((adj, np.where(adj, -rng.uniform(1e-3, 1.0, size=(nr, nc)), 0.0)))
    for nr, nc in ((45, 45), (256, 8), (8, 256)):
        probs.append((np.ones((nr, nc), bool), -rng.uniform(1e-3, 1.0, size=(nr, nc))))
    for _ in range(3):                                         # 256 rows / 256 columns / 2048 edges
        adj = np.zeros((256, 256), bool)
        for r in range(256):
            adj[r, r * 97 % 256] = True
            adj[r, rng.choice(np.setdiff1d(np.arange(256), [r * 97 % 256]), size=7, replace=False)] = True
        probs.append((adj, np.where(adj, -rng.uniform(1e-3, 1.0, size=adj.shape), 0.0)))
    adj = lap_ref.chain(256) > 0                               # the long augmenting path, generic costs
    probs.append((adj, np.where(adj, -rng.uniform(1e-3, 1.0, size=adj.shape), 0.0)))
    return probs


def scipy_objective(adj, cost):
    """Each row gets a private zero-cost dummy column; a missing edge costs more than any matching can gain."""
    from scipy.optimize import linear_sum_assignment
    nr, nc = adj.shape
    big = 1e3
    ext = np.full((nr, nc + nr), big)
    ext[:, :nc] = np.where(adj, cost, big)
    ext[np.arange(nr), nc + np.arange(nr)] = 0.0
    rows, cols = linear_sum_assignment(ext)
    assert all(c >= nc or adj[r, c] for r, c in zip(rows, cols))
    return math.fsum(cost[r, c] for r, c in zip(rows, cols) if c < nc)


def write_problems(path, probs):
    with open(path, "w") as f:
        f.write(f"{len(probs)}\n")
        for adj, cost in probs:
            nr, nc = adj.shape
            deg = adj.sum(axis=1)
            rr, cc = np.nonzero(adj)                           # row-major: CSR order
            f.write(f"{nr} {nc} {len(rr)}\n")
            f.write(" ".join(str(int(x)) for x in np.concatenate([[0], np.cumsum(deg)])) + "\n")
            f.write(" ".join(str(int(c)) for c in cc) + "\n")
            f.write(" ".join(float(cost[r, c]).hex() for r, c in zip(rr, cc)) + "\n")


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    probs = generic_problems()
    path = str(tmp_path_factory.mktemp("lap") / "problems.txt")
    write_problems(path, probs)
    return path, [scipy_objective(adj, cost) for adj, cost in probs]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_lap_solve_on_the_host(tmp_path, problems, sanitize):
    path, ref = problems
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    sys.stdout.write("\n".join(l for l in out.stdout.splitlines() if l.startswith("ok ")) + "\n")
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    for typ in ("double", "LexCost", "longlong"):
        assert sum(1 for l in out.stdout.splitlines() if l.startswith("ok ") and l.split()[2] == typ) == FAMILIES + (typ == "double"), typ
    got = {int(l.split()[1]): float(l.split()[2]) for l in out.stdout.splitlines() if l.startswith("obj ")}
    assert sorted(got) == list(range(len(ref)))
    for i, r in enumerate(ref):                                # costs in (-1, 0): the bound test_gpu_tracker.py uses for this comparison
        assert abs(got[i] - r) < 1e-12, (i, got[i], r)


def test_contested_rule_on_a_hand_made_graph():
    #        c0 c1 c2 c3 c4
    adj = [[1, 0, 0, 0, 0],        # r0 - c0 isolated
           [0, 1, 1, 0, 0],        # r1 has two columns: contested, with c1 and c2
           [0, 0, 0, 1, 0],        # r2 and r3 share c3: both contested
           [0, 0, 0, 1, 0],
           [0, 0, 0, 0, 0]]        # r4 has nothing; c4 has nothing
    r, c, e = lap_ref.contested(np.array(adj, bool))
    assert r.tolist() == [1, 2, 3] and c.tolist() == [1, 2, 3] and e == 4
    assert lap_ref.counts(lap_ref.admissible(lap_ref.chain(256), 0.8)) == (256, 256, 511)
    assert lap_ref.counts(lap_ref.admissible(lap_ref.chain_evict(256), 0.8)) == (256, 255, 510)


def test_component_wise_oracle_equals_the_oracle():
    from oracle import tracker_oracle as T
    rng = np.random.default_rng(3)
    for _ in range(3):
        a = lap_ref.embed(rng, lap_ref.sparse(rng, 40, 40, 2), 200, 230, isolated=120)
        assert lap_ref.oracle_by_components(T.assign_lapjv, a, 0.8) == T.assign_lapjv(a, 0.8)


def test_scipy_stand_ins_equal_the_pure_python_reference():
    """The crowded-frame GPU tests replace eval_ref.assign_lex / max_weight (cubic, pure Python) by scipy; on small cases,
    generic and tied, both give the same cardinality and distance sum, and on generic ones the same pairs."""
    import eval_ref as ER
    rng = np.random.default_rng(8)
    for t in range(60):
        r, c = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        D = rng.uniform(0, 1, (r, c)) if t % 2 else rng.integers(0, 5, (r, c)) / 8.0
        V = D <= 0.5
        a, b = ER.assign_lex(D, V), lap_ref.assign_lex_scipy(D, V)
        assert len(a) == len(b) and abs(sum(D[i, j] for i, j in a) - sum(D[i, j] for i, j in b)) <= 1e-12
        if t % 2:
            assert sorted(a) == sorted(b)
        W = rng.integers(0, 4, (r, c)) * (rng.random((r, c)) < 0.5)
        assert ER.max_weight(W) == lap_ref.max_weight_scipy(W)
    g, h = lap_ref.mot_clusters(rng, 1, [(2, 2), (1, 2), (2, 1), (1, 1)] * 2)
    g2, h2 = lap_ref.mot_chain(rng, 2, 9)
    g, h = np.concatenate([g, g2]), np.concatenate([h, h2])
    a, b = ER.mot_ref(g, h), ER.mot_ref(g, h, assign=lap_ref.assign_lex_scipy, weight=lap_ref.max_weight_scipy)
    assert {k: v for k, v in a.items() if k != "dist_sum"} == {k: v for k, v in b.items() if k != "dist_sum"}
    assert abs(a["dist_sum"] - b["dist_sum"]) <= 1e-12 * a["dist_sum"]
