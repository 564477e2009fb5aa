"""``csrc/launch_plan.h`` -- the one value that says how a detector launch runs (tiles, tail tile, form), its tune-cache record, the
derived ``skip`` flags and the A/B hooks -- is host code; ``tests/native/launch_plan_check.cpp`` drives it over the committed
``profiles/bench_tune_cache.txt`` (every record must decode and encode back to the same three integers) and over hand-built op lists.
The program is built twice with the host compiler, plain and with the address / undefined-behaviour sanitizers; it runs by itself,
with or without a GPU."""
import os
import subprocess
import sys

import pytest

from test_lap_cpu import CSRC, ROOT, host_compilers

SRC = os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp")
CACHE = os.path.join(ROOT, "profiles", "bench_tune_cache.txt")
STEPS = ("ok round trip", "ok literals", "ok mark_skips", "ok apply_hooks", "ok finish_plan", "ok for_each_view")


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("launch_plan_check_san" if sanitize else "launch_plan_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built launch_plan_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_launch_plan_on_the_host(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, CACHE], capture_output=True, text=True, timeout=120, env=env)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    for step in STEPS:
        assert any(l.startswith(step) for l in lines), step
    assert lines[-1] == "all ok" and not any(l.startswith("FAIL") for l in lines)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    with open(CACHE) as f:                                         # the count the program printed is the file's record count
        records = sum(1 for l in f.read().splitlines()[1:] if l.strip())
    assert records > 100 and lines[0].startswith(f"ok round trip {records} of {records} records"), lines[0]
