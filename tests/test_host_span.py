"""The host-span arithmetic (oneccl_amd/csrc/host_span.hpp) under every staged
copy of mi_reduce.hip, checked exhaustively on the CPU by
tests/cpp/host_span_check.cpp: every address offset within a page pair times
lengths 0..80, around a page and around a staging chunk, against the
invariants of the aligned hull, the head / interior / tail split and the
staging buffer's size, and against the formulas h2d_stage, d2h_pageable,
copy_geometry and reduce_issue held before they shared the header."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_host_span(tmp_path):
    exe = tmp_path / "host_span_check"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "host_span_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "failures 0" in r.stdout
    assert int(r.stdout.split()[1]) == 4112 * (81 + 5 + 4)  # offsets x (lengths + chunk checks per element size)
