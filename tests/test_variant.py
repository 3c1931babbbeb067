"""The variant rule (oneccl_amd/csrc/variant.hpp) of the host fold, checked
exhaustively on the CPU by tests/cpp/variant_check.cpp: canon_flags against
copies of mi_reduce.hip's canon_flags and of host_reduce.cpp's former canon
over every dtype, op, flag word and input count, valid_variant against the
image of canon_flags and against a copy of mi_reduce.hip's valid_v, the 94
variants per dtype class, dtype_size and
tail_trunc_from.  Under both standards the header is compiled with: gnu++11
(the in-tree build of host_reduce.cpp) and c++17 (the libraries)."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# (dtype -1..12) x (op -1..4): flag words x input counts, and the 32 five-bit values;
# (dtype, op) variant counts and their total; dtype sizes; tail thresholds
CASES = 14 * 6 * (256 * 4 + 32) + 12 * 4 + 1 + 14 + 6


@pytest.mark.parametrize("std", ["gnu++11", "c++17"])
def test_variant_rule(tmp_path, std):
    exe = tmp_path / "variant_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", f"-std={std}", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "variant_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "failures 0" in r.stdout
    assert int(r.stdout.split()[1]) == CASES
