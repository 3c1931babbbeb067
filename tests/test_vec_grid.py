"""The vector-grid plan (oneccl_amd/csrc/vec_grid.hpp) that every reduce
launcher shares, checked exhaustively on the CPU by tests/cpp/vec_grid_check.cpp:
element sizes 1..8, every output and input misalignment, counts 0..70, one and
two outputs, unaligned vectors on and off, against the split's invariants and
against the formulas the launchers held before they shared it."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_vec_grid_plan(tmp_path):
    exe = tmp_path / "vec_grid_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "vec_grid_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "failures 0" in r.stdout
    assert int(r.stdout.split()[1]) > 2_000_000
