"""The CPU host path (host_reduce.cpp / host_reduce_avx512.cpp) writes nothing
outside its output: full-width vector bodies with scalar tails, folded
between guards (tests/guard.py) at every count around the 8-, 16- and
32-lane steps, with the output at 0, 1 and 3 elements off its natural
alignment, out of place and aliasing inputs[0].  The same for the host
conversions, the host copy and the drop-in's keep-precision batch reduce,
whose fp32 scratch fold must not run past `out`.  The bits are the oracle's
as everywhere else; the bounds check is on top.  The file runs again in a
child process under each narrower ISA form (MI_HOST_ISA).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
from oneccl_amd import _lib, comp
from oneccl_amd.comp import F_ACC_FP32, F_BF16_RNE, F_BF16_TAIL_TRUNC16, F_MINMAX_INOUT_FIRST, bf16_flags
from tests.guard import Arena, arena_bytes, oracle_fold
from tests.util import ALL_DTYPES, BF16, DT_NAME, FP16, FP32, OP_NAME, OPS, assert_same, convert_expected, rand_array

pytestmark = pytest.mark.skipif(not _lib.shim().mi_host_supported(), reason="CPU lacks AVX2/F16C: no host path")

COUNTS = [0, 1, 15, 16, 17, 31, 63, 64, 65, 511, 513, 4099]
OUT_MIS = [0, 1, 3]  # elements
KS = [1, 2, 3, 16]


def _variants(dt):
    if dt == BF16:
        return [bf16_flags(2), bf16_flags(0), F_ACC_FP32, F_ACC_FP32 | F_BF16_RNE | F_MINMAX_INOUT_FIRST]
    if dt == FP16:
        return [F_MINMAX_INOUT_FIRST, F_ACC_FP32 | F_MINMAX_INOUT_FIRST]
    return [0]


def _run_host_cases(dt, op, k, flags):
    """Every count x output misalignment x {out of place, out = inputs[0]}
    of one kind of fold in one arena: the calls are synchronous CPU code, so
    one snapshot before and one comparison after cover them all."""
    es = np.dtype(oracle.NP_DTYPE[dt]).itemsize
    cases = [(n, m, inplace) for n in COUNTS for m in OUT_MIS for inplace in (False, True)]
    total = sum((k + 1) * n * es for n, _, _ in cases)
    ar = Arena(arena_bytes(total, len(cases) * (k + 1)), "pageable", seed=dt * 64 + op * 16 + k)
    placed = []
    for c, (n, m, inplace) in enumerate(cases):
        ins = [rand_array(dt, n, seed=7000 + 31 * c + j, op=op) for j in range(k)]
        # inputs at their own element offsets: host code takes any element-aligned pointer
        mis = [((m + j) * es) % 16 for j in range(k)]
        mis[0] = (m * es) % 16
        pin, pout = ar.place_reduce(ins, dt, op, flags, mis, inplace, out_mis=(m * es) % 16, tag=f"c{c}.")
        exp = oracle_fold(ins, dt, op, flags) if n else ins[0].copy()
        placed.append((pin, pout, exp, n))
    ar.snapshot()
    hr = _lib.shim().mi_host_reduce
    for pin, pout, exp, n in placed:
        arr = _lib.void_ptr_array([o.ptr for o in pin])
        assert hr(arr, k, pout.ptr, n, dt, op, flags) == 0
    ar.check(what=f"mi_host_reduce {DT_NAME[dt]} {OP_NAME[op]} k={k} flags={flags:#x}")
    for (pin, pout, exp, n), case in zip(placed, cases):
        if n:
            assert_same(ar.read(pout), exp, dt, f"count, out misalignment, in place = {case}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
@pytest.mark.parametrize("dt", ALL_DTYPES, ids=[DT_NAME[d] for d in ALL_DTYPES])
def test_host_reduce_between_guards(dt, op, k):
    _run_host_cases(dt, op, k, _variants(dt)[0])


LP_VARIANTS = [(dt, f) for dt in (BF16, FP16) for f in _variants(dt)[1:]]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
@pytest.mark.parametrize("dt,flags", LP_VARIANTS, ids=[f"{DT_NAME[d]}-f{f:x}" for d, f in LP_VARIANTS])
def test_host_reduce_lp_variants_between_guards(dt, flags, op, k):
    """bf16 truncating (scalar impl) and the fp32-accumulate fan-in of both
    low-precision types."""
    _run_host_cases(dt, op, k, flags)


CONV = [(FP32, BF16, 0), (FP32, BF16, F_BF16_RNE), (FP32, BF16, F_BF16_RNE | F_BF16_TAIL_TRUNC16), (FP32, FP16, 0),
        (BF16, FP32, 0), (FP16, FP32, 0)]


@pytest.mark.parametrize("sdt,ddt,flags", CONV, ids=["f32-bf16trunc", "f32-bf16rne", "f32-bf16rne-tail", "f32-f16",
                                                     "bf16-f32", "f16-f32"])
def test_host_convert_between_guards(sdt, ddt, flags):
    ds = np.dtype(oracle.NP_DTYPE[ddt]).itemsize
    cases = [(n, m) for n in COUNTS for m in OUT_MIS]
    ar = Arena(arena_bytes(sum(6 * n for n, _ in cases), 2 * len(cases)), "pageable", seed=sdt * 16 + ddt)
    placed = []
    for c, (n, m) in enumerate(cases):
        src = rand_array(sdt, n, seed=100 + c)
        ps = ar.place(src, (c * src.itemsize) % 16, "in", f"c{c}.src")
        noise = np.full(n * ds, 0x5A, np.uint8).view(np.uint32 if ds == 4 else np.uint16)
        pd = ar.place(noise, (m * ds) % 16, "out", f"c{c}.dst")
        placed.append((ps, pd, convert_expected(src, sdt, ddt, flags), n))
    ar.snapshot()
    for ps, pd, exp, n in placed:
        assert _lib.shim().mi_host_convert(ps.ptr, sdt, pd.ptr, ddt, n, flags) == 0
    ar.check(what="mi_host_convert")
    for (ps, pd, exp, n), case in zip(placed, cases):
        got = ar.read(pd)
        assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), case


@pytest.mark.parametrize("nt", [0, 1])
def test_host_copy_between_guards(nt):
    """mi_host_copy over non-zero guards (test_host_copy_offsets_and_sizes
    checks zero pads): streaming stores from the first 64-byte boundary."""
    cases = [(n, so, do) for n in (0, 1, 63, 255, 256, 257, 383, 4096 + 5) for so in (0, 1, 33) for do in (0, 1, 31, 60)]
    ar = Arena(arena_bytes(sum(2 * n for n, _, _ in cases), 2 * len(cases)) + 128 * len(cases), "pageable", seed=nt)
    rng = np.random.default_rng(4)
    placed = []
    for c, (n, so, do) in enumerate(cases):
        src = rng.integers(0, 256, n, dtype=np.uint8)
        # misalignments beyond 16 bytes: pad the operand's front inside its own range
        ps = ar.place(np.concatenate([np.zeros(so // 16 * 16, np.uint8), src]), so % 16, "in", f"c{c}.src")
        pd_all = ar.place(rng.integers(1, 255, do // 16 * 16 + n, dtype=np.uint8), do % 16, "in", f"c{c}.dstpad")
        pd = ar.sub(pd_all, do // 16 * 16, n, "out", f"c{c}.dst")
        placed.append((ps.ptr + so // 16 * 16, pd, src))
    ar.snapshot()
    for sp, pd, src in placed:
        if src.size:
            assert _lib.shim().mi_host_copy(pd.ptr, sp, src.size, nt) == 0
    ar.check(what="mi_host_copy")
    for (sp, pd, src), case in zip(placed, cases):
        assert np.array_equal(ar.read(pd), src), case


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in ("CCL_BF16", "CCL_FP16", "CCL_COMP_HOST_MAX_BYTES")}

    def set_(**kv):
        for k, v in kv.items():
            os.environ[k] = v
        comp.env_reload()

    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    comp.env_reload()


@pytest.mark.parametrize("setting,bimpl", [("scalar", 0), ("avx512f", 1), ("avx512bf", 2)])
@pytest.mark.parametrize("keep", [0, 1])
def test_dropin_host_batch_reduce_between_guards(keep, setting, bimpl, env):
    """ccl_comp_batch_reduce on host buffers (the CPU path): k peer chunks
    packed in one tmp_buf at element offsets j * n, folded into inout.  With
    keep-precision the fold runs in fp32 scratch and rounds once: it must not
    write past inout, and tmp_buf stays as it was."""
    env(CCL_BF16=setting, CCL_COMP_HOST_MAX_BYTES=str(1 << 20))
    _, f_impl = comp.impl_types()
    cases = [(n, k, m) for n in (1, 15, 16, 17, 513, 4099) for k in (1, 3, 16) for m in (0, 1, 3)]
    ar = Arena(arena_bytes(sum(2 * n * (k + 1) for n, k, _ in cases), 2 * len(cases)), "pageable", seed=keep)
    placed = []
    for c, (n, k, m) in enumerate(cases):
        chunks = [rand_array(BF16, n, seed=40 * c + j) for j in range(k)]
        inout = rand_array(BF16, n, seed=40 * c + 39)
        packed = np.concatenate(chunks)
        pt = ar.place(packed, (2 * c) % 16, "in", f"c{c}.tmp_buf")
        po = ar.place(inout, (2 * m) % 16, "inout", f"c{c}.inout")
        exp = inout.copy()
        oracle.batch_reduce(packed, [j * n for j in range(k)], n, exp, BF16, 0, keep, bimpl, int(f_impl))
        placed.append((pt, po, exp, n, k))
    ar.snapshot()
    for pt, po, exp, n, k in placed:
        comp.comp_batch_reduce(pt.ptr, [j * n for j in range(k)], n, po.ptr, comp.datatype.bfloat16,
                               comp.reduction.sum, keep)
    ar.check(what=f"ccl_comp_batch_reduce keep={keep} CCL_BF16={setting}")
    for (pt, po, exp, n, k), case in zip(placed, cases):
        assert_same(ar.read(po), exp, BF16, f"{case}")


@pytest.mark.parametrize("dt", ALL_DTYPES, ids=[DT_NAME[d] for d in ALL_DTYPES])
def test_dropin_host_reduce_between_guards(dt, env):
    """ccl_comp_reduce on host buffers below the dispatcher's threshold."""
    env(CCL_COMP_HOST_MAX_BYTES=str(1 << 20))
    b_impl, f_impl = comp.impl_types()
    es = np.dtype(oracle.NP_DTYPE[dt]).itemsize
    flags = bf16_flags(int(b_impl)) if dt == BF16 else (F_MINMAX_INOUT_FIRST if dt == FP16 else 0)
    cases = [(n, m, op) for n in (1, 17, 63, 513, 4099) for m in OUT_MIS for op in OPS]
    ar = Arena(arena_bytes(sum(2 * n * es for n, _, _ in cases), 2 * len(cases)), "pageable", seed=dt)
    placed = []
    for c, (n, m, op) in enumerate(cases):
        a = rand_array(dt, n, seed=2 * c, op=op)
        b = rand_array(dt, n, seed=2 * c + 1, op=op)
        (pb, pa), _ = ar.place_reduce([b, a], dt, op, flags, [(m * es) % 16, ((m + 1) * es) % 16], True, tag=f"c{c}.")
        exp = b.copy()
        oracle.comp_reduce(a, exp, dt, op, int(b_impl), int(f_impl))
        placed.append((pa, pb, exp, n, op))
    ar.snapshot()
    for pa, pb, exp, n, op in placed:
        comp.comp_reduce(pa.ptr, n, pb.ptr, comp.datatype(dt), comp.reduction(op))
    ar.check(what="ccl_comp_reduce on host buffers")
    for (pa, pb, exp, n, op), case in zip(placed, cases):
        assert_same(ar.read(pb), exp, dt, f"{case}")


@pytest.mark.parametrize("isa", ["avx2", "avx512"])
def test_narrower_isa_forms_between_guards(isa):
    """The narrower forms of the host fold (8 AVX2 lanes, 16 AVX-512 lanes
    with the integer bf16 rounding), forced with MI_HOST_ISA in a fresh child
    process, keep to their outputs as well.  MI_HOST_ISA changes the bf16 /
    fp16 fold only (host_reduce.cpp pick_lp), so the child runs this file's
    low-precision cases: reduces, conversions and the drop-in batch reduce."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", str(Path(__file__)),
                        "-k", "(float16 or bf16 or f16 or batch_reduce) and not narrower_isa"],
                       cwd=str(root), env=dict(os.environ, MI_HOST_ISA=isa), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
