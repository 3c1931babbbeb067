#!/usr/bin/env python3
"""Per-kernel register table of a built libmi_reduce.so, from the gfx950 code
object's metadata (as tests/test_kernel_resources.py reads it; no GPU):

  python tools/kernel_table.py LIB > table.tsv
  python tools/kernel_table.py LIB_A LIB_B      # both tables side by side, differing rows marked
  python tools/kernel_table.py LIB_A LIB_B --text   # kernels whose instruction text differs, or in one library only

Columns: vgpr, sgpr, scratch bytes, vgpr spills, sgpr spills, demangled name."""
from __future__ import annotations

import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests.test_kernel_resources import LLVM, _code_object  # noqa: E402

KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def table(lib: Path) -> dict[str, tuple[int, ...]]:
    with tempfile.TemporaryDirectory() as tmp:
        co = _code_object(lib, Path(tmp))
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
    rows = {}
    for block in re.split(r"\n\s+- \.", notes):
        name = re.search(r"\.name:\s+(\S+)", "." + block)
        if not name or "private_segment_fixed_size" not in block:
            continue
        rows[name.group(1)] = tuple(int(m.group(1)) if (m := re.search(rf"\.{k}:\s+(\d+)", block)) else 0
                                    for k in KEYS)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=str(LLVM))
    if not filt:
        return rows  # mangled names
    names = list(rows)
    dem = subprocess.run([filt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"^void ", "", d): rows[n] for n, d in zip(names, dem)}


def text(lib: Path) -> dict[str, str]:
    """Instruction text per symbol of the code object: the disassembly without
    addresses, encodings and the trailing `//` comments."""
    with tempfile.TemporaryDirectory() as tmp:
        dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(_code_object(lib, Path(tmp)))], check=True,
                             capture_output=True, text=True).stdout
    out, fn = {}, None
    for line in dis.splitlines():
        if m := re.match(r"^[0-9a-f]+ <(\S+)>:$", line):
            fn = m.group(1)
            out[fn] = ""
        elif fn and line.strip():
            out[fn] += line.split("//")[0].strip() + "\n"
    return out


def main():
    if sys.argv[3:] == ["--text"]:
        a, b = text(Path(sys.argv[1])), text(Path(sys.argv[2]))
        for name in sorted(a.keys() | b.keys()):
            if a.get(name) != b.get(name):
                print(("differs" if name in a and name in b else "only in A" if name in a else "only in B") + "\t" + name)
        print(f"# kernels: {len(a)} -> {len(b)}; only in A: {len(a.keys() - b.keys())}; only in B: "
              f"{len(b.keys() - a.keys())}; instruction text differs: "
              f"{sum(1 for n in a.keys() & b.keys() if a[n] != b[n])}")
        return
    if len(sys.argv) == 2:
        print("vgpr\tsgpr\tscratch\tvspill\tsspill\tkernel")
        for name, r in sorted(table(Path(sys.argv[1])).items()):
            print("\t".join(map(str, r)) + "\t" + name)
        return
    a, b = table(Path(sys.argv[1])), table(Path(sys.argv[2]))
    print(f"# kernels: {len(a)} -> {len(b)}; only in A: {len(a.keys() - b.keys())}; only in B: {len(b.keys() - a.keys())}")
    print(f"# scratch or spills in A: {sum(1 for r in a.values() if any(r[2:]))}, in B: "
          f"{sum(1 for r in b.values() if any(r[2:]))}")
    print(f"# max vgpr: {max(r[0] for r in a.values())} -> {max(r[0] for r in b.values())}")
    # Both tables side by side.  Every kernel is listed: one row per kernel
    # template and set of figures, with the template arguments of all the
    # instantiations that have them; `*` marks rows whose figures differ.
    print("A:vgpr\tsgpr\tscratch\tB:vgpr\tsgpr\tscratch\tdiffers\tn\ttemplate\targuments")
    none = (0,) * len(KEYS)
    rows = {}
    for name in sorted(a.keys() | b.keys()):
        m = re.match(r"([\w:]+)<(.*)>\(", name)
        family, args = (m.group(1), m.group(2)) if m else (name, "")
        rows.setdefault((family, a.get(name, none)[:3] + b.get(name, none)[:3], a.get(name) != b.get(name)),
                        []).append(args)
    for (family, figs, differs), args in sorted(rows.items()):
        print("\t".join(map(str, figs)) + ("\t*\t" if differs else "\t\t") + f"{len(args)}\t{family}\t" + " | ".join(args))


if __name__ == "__main__":
    main()
