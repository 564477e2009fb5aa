"""``csrc/track_ledger.h`` -- the arithmetic of the id-sorted ledgers of zones, crossing, speed and snapshot: rank encoding, members
below an id (binary search or, after the swap guard, counting), old-row match, new positions, overflow, the meta row, the staging
sort -- includes no HIP header; ``tests/native/track_ledger_check.cpp`` runs the whole merge serially on the host against a sort,
at the sizes around one and two passes of the 256-thread workgroup and at 600 rows.  The program is built twice, plain and with the
address / undefined-behaviour sanitizers, as ``test_track_layout_cpu.py`` builds its program; it runs by itself (no GPU)."""
import os
import subprocess
import sys

import pytest

from test_lap_cpu import CSRC, ROOT, host_compilers

SRC = os.path.join(ROOT, "tests", "native", "track_ledger_check.cpp")
SIZES = 9                                                      # old rows x list lengths, see track_ledger_check.cpp's main


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("track_ledger_check_san" if sanitize else "track_ledger_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in host_compilers(sanitize):
        r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built track_ledger_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_track_ledger_on_the_host(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert sum(1 for l in lines if l.startswith("ok merge ") and l.endswith("(144 cases)")) == SIZES * SIZES
    assert "ok meta" in lines and "ok staging" in lines and lines[-1] == "all ok" and not any(l.startswith("FAIL") for l in lines)
