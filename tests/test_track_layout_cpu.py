"""``csrc/track_layout.h`` -- the pool carver, the three trackers' state layouts and the Kalman read-back -- includes no HIP header;
``tests/native/track_layout_check.cpp`` runs it on the host: measuring pass == assigning pass, 16-byte starts, no overlap, the
DeepSORT / OC-SORT sizes against the formulas the library used to carry, and the unpack against hand-made values.  The program is
built twice, plain and with the address / undefined-behaviour sanitizers, as ``test_lap_cpu.py`` builds ``lap_check.cpp``; it runs
by itself (no GPU)."""
import os
import subprocess
import sys

import pytest

from test_lap_cpu import CSRC, ROOT, host_compilers

SRC = os.path.join(ROOT, "tests", "native", "track_layout_check.cpp")
CASES = 6 * 2                                                  # max_tracks x n_streams, see track_layout_check.cpp's main


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("track_layout_check_san" if sanitize else "track_layout_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built track_layout_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_track_layout_on_the_host(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert sum(1 for l in lines if l.startswith("ok layouts ")) == CASES
    assert "ok kalman_unpack" in lines and lines[-1] == "all ok" and not any(l.startswith("FAIL") for l in lines)
