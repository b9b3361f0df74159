"""CPU: the row-pair-interleaved weight layout's helpers (csrc/w_layout.hpp) as a stand-alone host program.

tests/w_layout_check.cpp includes only that header, so compiling it with the host compiler shows the helpers
have no HIP dependency.  It checks, for N in {1, 2, 7, 255, 256, 257, 258} and K in {32, 64, 96, 2560}, every
tile column, tile row, chunk and k-tile: the staged 8 halves lie inside the helper's allocation size, and the
copy read back through the staging formula is w[n][k], the partner row of an odd N zero.  Run plain, and once
with the address and undefined-behaviour sanitizers, which watch the same indexing on a heap buffer of exactly
the allocation's size.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "task-vector-replication_amd" / "csrc"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_w_layout_check(tmp_path, flags):
    cxx = shutil.which("g++")
    assert cxx, "the layout check needs the host compiler (g++)"
    exe = tmp_path / "w_layout_check"
    build = subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Werror", "-I", str(CSRC),
                            str(ROOT / "tests" / "w_layout_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "w_layout_check: ok" in run.stdout
