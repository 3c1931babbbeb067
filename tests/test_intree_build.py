"""The drop-in's in-tree half, proven against the reference's own sources.

INTEGRATION.md §2a swaps src/comp/{comp,bf16/bf16,fp16/fp16}.cpp for
oneccl_amd/csrc/comp.cpp built with -DMI_ONECCL_TREE.  This test compiles
that translation unit exactly as oneCCL's build would — the reference's
headers (src/, include/ with its shipped oneapi/ccl/config.h, deps/*/include),
its flags (CMakeLists.txt:178-195: -std=gnu++11 -Wall -Wextra
-Wno-unused-parameter -Werror -fvisibility=internal; the BF16/FP16/AVX
defines SURVEY.md §8c records) — and compares the symbols of the resulting
object with the objects it replaces, compiled from the reference's own
sources with the same command.  No stand-ins: every header resolves from
the reference tree.  Runs where /root/reference exists (this container).

Checked:
  * every global symbol the three replaced objects define is defined by ours,
    with the same mangled name (so every caller in src/sched, src/atl and
    src/common/env links unchanged);
  * every symbol ours needs is one the replaced objects already needed, one
    the rest of libccl defines (checked on the compiled reference object that
    holds it), a libmi_reduce.so export, or a C/C++ runtime symbol;
  * the MPI fp16 user op (atl_mpi_ctx.cpp:58-64, inline ccl_fp16_reduce_impl)
    still links: the fp16/bf16 SIMD wrappers it needs come from the kept
    *_intrisics.cpp objects, which the swap leaves in the build.
"""
from __future__ import annotations

import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")

pytestmark = pytest.mark.skipif(not os.path.isdir(REF / "src" / "comp"),
                                reason="reference tree absent (GPU box): checked in the build container")

DEFS = ["-D_GNU_SOURCE", "-DCCL_BF16_COMPILER", "-DCCL_BF16_AVX512BF_COMPILER", "-DCCL_BF16_TARGET_ATTRIBUTES",
        "-DCCL_FP16_COMPILER", "-DCCL_FP16_TARGET_ATTRIBUTES", "-DCCL_AVX_COMPILER", "-DCCL_AVX_TARGET_ATTRIBUTES",
        "-DCCL_ENABLE_ITT=1", "-DCCL_ENABLE_MPI"]
WARN = ["-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-implicit-fallthrough", "-Werror"]
INCS = [f"-I{REF}/include", f"-I{REF}/src", f"-I{REF}/src/atl"] + \
       [f"-I{REF}/deps/{d}/include" for d in ("hwloc", "itt", "ofi", "pmix", "mpi", "level_zero")]
FLAGS = ["-std=gnu++11", "-O2", "-fPIC", "-fvisibility=internal", *WARN, *DEFS, *INCS]

REPLACED = {"comp": "src/comp/comp.cpp", "bf16": "src/comp/bf16/bf16.cpp", "fp16": "src/comp/fp16/fp16.cpp"}
KEPT = {"bf16_intrisics": "src/comp/bf16/bf16_intrisics.cpp", "fp16_intrisics": "src/comp/fp16/fp16_intrisics.cpp"}
OTHER = {"datatype": "src/common/datatype/datatype.cpp", "atl_mpi_ctx": "src/atl/mpi/atl_mpi_ctx.cpp"}


def _compile(src: Path, out: Path, extra=()) -> subprocess.CompletedProcess:
    return subprocess.run(["g++", *FLAGS, *extra, "-c", str(src), "-o", str(out)], capture_output=True, text=True)


def _nm(path: Path, *args) -> list[tuple[str, str]]:
    r = subprocess.run(["nm", *args, str(path)], capture_output=True, text=True, check=True)
    out = []
    for line in r.stdout.splitlines():
        m = re.match(r"^\s*(?:[0-9a-fA-F]+\s+)?([A-Za-z])\s+(\S+)$", line)
        if m:
            out.append((m.group(1), m.group(2)))
    return out


def _global_defs(obj: Path) -> set[str]:
    return {s for t, s in _nm(obj, "--defined-only") if t in "TBDR"}


def _undefs(obj: Path) -> set[str]:
    return {s for t, s in _nm(obj, "-u")}


def _dyn_defs(lib: str) -> set[str]:
    return {s.split("@")[0] for t, s in _nm(Path(lib), "-D", "--defined-only")}


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("intree")
    jobs = {name: (REF / rel, d / f"{name}.o", ()) for name, rel in {**REPLACED, **KEPT, **OTHER}.items()}
    jobs["ours"] = (ROOT / "oneccl_amd" / "csrc" / "comp.cpp", d / "ours.o",
                    ("-DMI_ONECCL_TREE", f"-I{ROOT / 'include'}"))
    # the host reduce, with the per-source ISA options of INTEGRATION.md §2a
    jobs["ours_host"] = (ROOT / "oneccl_amd" / "csrc" / "host_reduce.cpp", d / "ours_host.o",
                         ("-mavx2", "-mf16c", "-mfma"))
    jobs["ours_host512"] = (ROOT / "oneccl_amd" / "csrc" / "host_reduce_avx512.cpp", d / "ours_host512.o",
                            ("-mavx2", "-mf16c", "-mfma", "-mavx512f", "-mavx512bw", "-mavx512vl", "-mavx512bf16"))
    with ThreadPoolExecutor(4) as ex:
        res = dict(zip(jobs, ex.map(lambda j: _compile(*j), jobs.values())))
    return {name: (jobs[name][1], r) for name, r in res.items()}


def test_intree_translation_unit_compiles_with_reference_flags(objs):
    for name in ("ours", "ours_host", "ours_host512"):
        out, r = objs[name]
        assert r.returncode == 0, (name, r.stderr[-3000:])
    for name in (*REPLACED, *KEPT, *OTHER):  # the same command builds the reference's own sources
        assert objs[name][1].returncode == 0, (name, objs[name][1].stderr[-2000:])


def test_intree_object_defines_every_replaced_symbol(objs):
    ours = _global_defs(objs["ours"][0])
    replaced = set().union(*(_global_defs(objs[n][0]) for n in REPLACED))
    assert len(replaced) >= 17
    missing = sorted(replaced - ours)
    assert not missing, missing


def test_intree_object_needs_nothing_the_tree_does_not_provide(objs):
    ours = ("ours", "ours_host", "ours_host512")
    need = set().union(*(_undefs(objs[n][0]) for n in ours)) - set().union(*(_global_defs(objs[n][0]) for n in ours))
    provided = set().union(*(_undefs(objs[n][0]) for n in REPLACED))  # already resolved inside libccl
    provided |= _global_defs(objs["datatype"][0])  # ccl_datatype's constructor
    provided |= _dyn_defs(str(ROOT / "oneccl_amd" / "lib" / "libmi_reduce.so"))
    # ld.so: __tls_get_addr, which libccl's own thread_locals need as well
    # (src/common/log/log.cpp, src/common/global/global.cpp)
    for lib in ("/lib/x86_64-linux-gnu/libc.so.6", "/lib/x86_64-linux-gnu/libstdc++.so.6",
                "/lib/x86_64-linux-gnu/libgcc_s.so.1", "/lib/x86_64-linux-gnu/libm.so.6",
                "/lib64/ld-linux-x86-64.so.2"):
        if Path(lib).exists():
            provided |= _dyn_defs(lib)
    libgcc = subprocess.run(["g++", "-print-libgcc-file-name"], capture_output=True, text=True).stdout.strip()
    if libgcc and Path(libgcc).exists():  # the compiler's static runtime (__builtin_cpu_supports' data)
        provided |= {s for t, s in _nm(Path(libgcc), "--defined-only") if t in "TBDRC"}
    provided |= {"_GLOBAL_OFFSET_TABLE_", "__dso_handle"}
    missing = sorted(need - provided)
    assert not missing, missing


def test_mpi_fp16_user_op_still_links(objs):
    """atl_mpi_ctx.o (ATL_MPI_FP16/BF16 user ops) after the swap: what it
    needs from src/comp is defined by our object or the kept SIMD objects."""
    need = _undefs(objs["atl_mpi_ctx"][0])
    all_comp = set().union(*(_global_defs(objs[n][0]) for n in (*REPLACED, *KEPT)))
    from_comp = need & all_comp
    assert any("fp16_sum_wrap_256" in s for s in from_comp)  # the inline ccl_fp16_reduce_impl path
    after_swap = _global_defs(objs["ours"][0]) | set().union(*(_global_defs(objs[n][0]) for n in KEPT))
    missing = sorted(from_comp - after_swap)
    assert not missing, missing
