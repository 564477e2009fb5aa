"""``csrc/handle_host.h`` -- the open / close frame, the event timer and the tail of a create that every module's handle shares --
is host code; ``tests/native/handle_host_check.cpp`` drives a toy handle through the failure paths on a device ordinal that exists
nowhere: open failing at ``hipSetDevice`` and the created-tail after it, close of an empty and of a half-built handle, the timer
before anything was recorded.  The program is built twice with the host compiler and linked to the HIP runtime, plain and with the
address / undefined-behaviour sanitizers (the leak checker included: a tail that lost the handle would be reported); it runs by
itself, with or without a GPU."""
import os
import subprocess
import sys

import pytest

from test_lap_cpu import CSRC, ROOT, host_compilers, rocm_root

SRC = os.path.join(ROOT, "tests", "native", "handle_host_check.cpp")
STEPS = ("ok open fails", "ok check fails", "ok close of an empty handle", "ok close after a failed open", "ok timer")


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("handle_host_check_san" if sanitize else "handle_host_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    rocm = rocm_root()
    errors = []
    for cxx in host_compilers(sanitize):
        cmd = [cxx, "-x", "c++", "-std=c++17", "-Wall", "-Wno-unused-result", *flags, "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(rocm, "include"), SRC, "-o", exe,
               "-L", os.path.join(rocm, "lib"), "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lamdhip64"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built handle_host_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_handle_skeleton_on_the_host(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    for step in STEPS:
        assert any(l.startswith(step) for l in lines), step
    assert lines[-1] == "all ok" and not any(l.startswith("FAIL") for l in lines)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
