"""The head / body / tail plan of mi_reduce_bcast_mixed (plan_mixed_grid,
oneccl_amd/csrc/vec_grid.hpp), checked exhaustively on the CPU by
tests/cpp/mixed_grid_check.cpp: both element-size pairs, every output and
input misalignment, accumulators, counts 0..600, unaligned vectors on and off,
against the split's invariants, the alignment of every body store and the
documented conditions of the element loop.  Once as a plain build, once under
AddressSanitizer and UBSan; both are stand-alone programs."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan-ubsan"])
def test_mixed_grid_plan(tmp_path, san):
    exe = tmp_path / "mixed_grid_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *san, "-o",
                        str(exe), str(ROOT / "tests" / "cpp" / "mixed_grid_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "failures 0" in r.stdout
    assert int(r.stdout.split()[1]) > 2_000_000
