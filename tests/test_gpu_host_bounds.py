"""Host outputs of the GPU paths stay inside their range.

mi_reduce.hip promises "Nothing outside the destination is written" for the
staged pipeline's D2H (d2h_pageable / Edges); the bounce buffers, the
zero-copy kernels on pinned memory and the cooperative split make the same
promise without saying so.  Here the output (for in-place calls, inout) lies
in a pinned or pageable arena between guards (tests/guard.py) at
misalignments 0, es and 16 - es, ending on and off a 16-byte boundary, and
the whole arena is compared after the call: the up to 15 bytes between a
misaligned operand and the next 16-byte boundary included.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import oracle
from oneccl_amd import _lib, comp
from oneccl_amd.comp import F_BF16_RNE, F_BF16_TAIL_TRUNC16, F_MINMAX_INOUT_FIRST, bf16_flags
from tests.guard import DT_OP, DT_OP_IDS, T_LEAN, Arena, arena_bytes, oracle_fold
from tests.guard import es_of as _es
from tests.guard import ref_flags as _flags
from tests.guard import tile_shapes as shapes
from tests.util import BF16, FP16, FP32, FP64, assert_same, convert_expected, rand_array

pytestmark = pytest.mark.gpu

MIB = 1 << 20
FOUR = [(FP32, 0), (BF16, 3), (0, 2), (FP64, 1)]
FOUR_IDS = ["f32-sum", "bf16-max", "i8-min", "f64-prod"]


def _mis3(es):
    return sorted({0, es % 16, 16 - es})


def run_sync(kind, cases, what, seed=0):
    """cases: (dt, op, flags, k, count, misalignment, inplace).  k = 2 in
    place goes through mi_reduce_sync, everything else through
    mi_reduce_multi_sync.  The calls return when the output is final, so one
    snapshot before and one comparison after cover them all."""
    total = sum((c[3] + 1) * c[4] * _es(c[0]) for c in cases)
    ar = Arena(arena_bytes(total, sum(c[3] + 1 for c in cases)), kind, seed=seed)
    placed = []
    for i, (dt, op, flags, k, n, m, inplace) in enumerate(cases):
        ins = [rand_array(dt, n, seed=2000 * seed + 17 * i + j, op=op) for j in range(k)]
        pin, pout = ar.place_reduce(ins, dt, op, flags, [m] * k, inplace, m, tag=f"c{i}.")
        placed.append((pin, pout, oracle_fold(ins, dt, op, flags) if n else ins[0]))
    ar.snapshot()
    m_ = _lib.mi()
    for (dt, op, flags, k, n, m, inplace), (pin, pout, _) in zip(cases, placed):
        if k == 2 and inplace:
            _lib.check(m_.mi_reduce_sync(pin[1].ptr, pin[0].ptr, n, dt, op, flags, -1), "mi_reduce_sync")
        else:
            arr = _lib.void_ptr_array([o.ptr for o in pin])
            _lib.check(m_.mi_reduce_multi_sync(arr, k, pout.ptr, n, dt, op, flags, -1), "mi_reduce_multi_sync")
    ar.check(what=what)
    for c, (pin, pout, exp) in zip(cases, placed):
        if c[4]:
            assert_same(ar.read(pout), exp, c[0], f"{what}: (dt, op, flags, k, count, mis, inplace) = {c}")


# ---- zero-copy: the kernels write pinned host memory in place -------------------

@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_zero_copy_pinned(dt, op):
    """Pinned operands: the lean and fan kernels read and write host memory
    over PCIe, at the tile-edge shapes of test_gpu_bounds.py."""
    cases = []
    for n, m in shapes(_es(dt), T_LEAN):
        cases.append((dt, op, _flags(dt), 2, n, m, True))
        cases.append((dt, op, _flags(dt), 3, n, m, False))
        cases.append((dt, op, _flags(dt), 9, n, m, True))
        cases.append((dt, op, _flags(dt), 16, n, m, False))
    run_sync("pinned", cases, "zero-copy", seed=dt)


# ---- bounce buffers: pageable operands of at most 1 MiB --------------------------

@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_bounce_buffers(dt, op):
    es = _es(dt)
    cases = []
    for n in (1, 17, MIB // es - 1):
        for m in _mis3(es):
            cases.append((dt, op, _flags(dt), 2, n, m, True))
            cases.append((dt, op, _flags(dt), 3, n, m, False))
    run_sync("pageable", cases, "bounce buffers", seed=20 + dt)


# ---- the staged pipeline: pageable operands above 1 MiB ---------------------------

@pytest.mark.parametrize("dt,op", FOUR, ids=FOUR_IDS)
def test_staged_pipeline_one_chunk(dt, op):
    """Just over the bounce size: one staging chunk, whose < 16-byte head and
    tail go through d2h_pageable's pinned scratch and the CPU's memcpy."""
    es = _es(dt)
    cases = []
    for m in _mis3(es):
        n_on = (MIB + 4096 + (16 - m) % 16) // es  # m + n_on * es is a multiple of 16: ends on a boundary
        cases.append((dt, op, _flags(dt), 2, n_on + 1, m, True))  # ends off one
        cases.append((dt, op, _flags(dt), 3, n_on, m, False))
    run_sync("pageable", cases, "staged pipeline, one chunk", seed=40 + dt)


def test_staged_pipeline_two_chunks():
    """32 MiB + 4 KiB + 6 B of bf16 with the output 2 bytes off alignment:
    two staging chunks, so the drain thread and its Edges slot are used."""
    n = (32 * MIB + 4096 + 6) // 2
    run_sync("pageable", [(BF16, 0, bf16_flags(2), 2, n, 2, True)], "staged pipeline, two chunks", seed=60)


# ---- mi_convert_sync / mi_copy_sync --------------------------------------------

SIZES = [5, 4096 + 13, MIB + 4096 + 9]


@pytest.mark.parametrize("src_kind", ["same", "device"])
@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_copy_sync_into_host(kind, src_kind):
    """mi_copy_sync into a host destination at byte misalignments 0, 1 and 15
    from a host source of the same kind or from device memory."""
    import torch
    rng = np.random.default_rng(3)
    cases = [(n, m) for n in SIZES for m in (0, 1, 15)]
    ar = Arena(arena_bytes(2 * sum(n for n, _ in cases), 2 * len(cases)), kind, seed=1)
    placed, keep = [], []
    for c, (n, m) in enumerate(cases):
        src = rng.integers(0, 256, n, dtype=np.uint8)
        if src_kind == "device":
            full = np.concatenate([src, rng.integers(0, 256, 16, dtype=np.uint8)])
            t = torch.from_numpy(full).cuda()
            keep.append(t)
            sp = t.data_ptr() + c % 16  # the source at its own byte offset
            src = full[c % 16:c % 16 + n]
        else:
            sp = ar.place(src, (5 * c) % 16, "in", f"c{c}.src").ptr
        pd = ar.place(rng.integers(1, 255, n, dtype=np.uint8), m, "out", f"c{c}.dst")
        placed.append((sp, pd, src))
    ar.snapshot()
    torch.cuda.synchronize()
    for nt, (sp, pd, src) in enumerate(placed):
        _lib.check(_lib.mi().mi_copy_sync(sp, pd.ptr, src.size, nt & 1, -1), "mi_copy_sync")
    ar.check(what=f"mi_copy_sync into {kind} memory")
    for (sp, pd, src), case in zip(placed, cases):
        assert np.array_equal(ar.read(pd), src), case


CONV = [(FP32, BF16, F_BF16_RNE | F_BF16_TAIL_TRUNC16), (FP32, FP16, 0), (BF16, FP32, 0), (FP16, FP32, 0)]


@pytest.mark.parametrize("sdt,ddt,flags", CONV, ids=["f32-bf16rne-tail", "f32-f16", "bf16-f32", "f16-f32"])
@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_convert_sync_into_host(kind, sdt, ddt, flags):
    ss, ds = _es(sdt), _es(ddt)
    cases = [(max(nb // ds, 1), m) for nb in SIZES for m in _mis3(ds)]
    ar = Arena(arena_bytes(sum(n * (ss + ds) for n, _ in cases), 2 * len(cases)), kind, seed=2)
    placed = []
    for c, (n, m) in enumerate(cases):
        src = rand_array(sdt, n, seed=300 + c)
        ps = ar.place(src, (c * ss) % 16, "in", f"c{c}.src")
        noise = np.full(n * ds, 0x5A, np.uint8).view(np.uint32 if ds == 4 else np.uint16)
        pd = ar.place(noise, m, "out", f"c{c}.dst")
        placed.append((ps, pd, convert_expected(src, sdt, ddt, flags), n))
    ar.snapshot()
    for ps, pd, exp, n in placed:
        _lib.check(_lib.mi().mi_convert_sync(ps.ptr, sdt, pd.ptr, ddt, n, flags, -1), "mi_convert_sync")
    ar.check(what=f"mi_convert_sync into {kind} memory")
    for (ps, pd, exp, n), case in zip(placed, cases):
        assert np.array_equal(ar.read(pd).view(np.uint8), exp.view(np.uint8)), case


@pytest.mark.parametrize("sdt,ddt,flags,smis,dmis", [(FP32, BF16, F_BF16_RNE | F_BF16_TAIL_TRUNC16, 4, 2),
                                                     (BF16, FP32, 0, 2, 4)], ids=["f32-bf16rne-tail", "bf16-f32"])
def test_convert_sync_two_chunks(sdt, ddt, flags, smis, dmis):
    """A staged conversion across a chunk boundary.  The chunk is 32 MiB of
    the larger element, 8388608 elements; 23 more make a second chunk whose
    first 16 elements are rounded and whose last 7 are truncated under
    F_BF16_TAIL_TRUNC16 (count // 16 * 16 lies inside it): the smallest count
    that crosses the boundary and puts the split into the second chunk's
    window.  Source and destination sit off 16-byte alignment by different
    amounts, so both chunks' staged copies have unaligned ends."""
    n = 8388608 + 23
    ss, ds = _es(sdt), _es(ddt)
    ar = Arena(arena_bytes(n * (ss + ds), 2), "pageable", seed=4)
    src = rand_array(sdt, n, seed=400)
    ps = ar.place(src, smis, "in", "src")
    pd = ar.place(np.full(n * ds, 0x5A, np.uint8).view(np.uint32 if ds == 4 else np.uint16), dmis, "out", "dst")
    exp = convert_expected(src, sdt, ddt, flags)
    ar.snapshot()
    _lib.check(_lib.mi().mi_convert_sync(ps.ptr, sdt, pd.ptr, ddt, n, flags, -1), "mi_convert_sync")
    ar.check(what="mi_convert_sync over two chunks")
    assert np.array_equal(ar.read(pd).view(np.uint8), exp.view(np.uint8))


# ---- requests -----------------------------------------------------------------

def _host_fold_ptr():
    """mi_host_reduce (the shim's CPU fold) as a C function pointer."""
    return ctypes.cast(_lib.shim().mi_host_reduce, ctypes.c_void_p).value


def _one_inplace(kind, dt, op, n, m, seed):
    flags = _flags(dt)
    a = rand_array(dt, n, seed=seed, op=op)
    b = rand_array(dt, n, seed=seed + 1, op=op)
    ar = Arena(arena_bytes(2 * a.nbytes, 2), kind, seed=seed)
    (pb, pa), _ = ar.place_reduce([b, a], dt, op, flags, [m, m], True)
    ar.snapshot()
    return ar, pa, pb, oracle_fold([b, a], dt, op, flags), flags


@pytest.mark.parametrize("kind,n", [("pinned", 4099), ("pageable", MIB // 2 + 4099)], ids=["direct", "staged"])
def test_start_wait(kind, n):
    """mi_reduce_start / mi_wait: a direct request (pinned operands: a launch
    on the caller's thread) and a staged one (pageable operands above the
    bounce size: the staging worker)."""
    m = _lib.mi()
    ar, pa, pb, exp, flags = _one_inplace(kind, BF16, 0, n, 2, seed=70)
    req = ctypes.c_void_p()
    _lib.check(m.mi_reduce_start(_lib.void_ptr_array([pb.ptr, pa.ptr]), 2, pb.ptr, n, BF16, 0, flags, -1,
                                 ctypes.byref(req)), "mi_reduce_start")
    _lib.check(m.mi_wait(req), "mi_wait")
    _lib.check(m.mi_request_free(req))
    ar.check(what=f"mi_reduce_start ({kind})")
    assert_same(ar.read(pb), exp, BF16)


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("dt,op", FOUR, ids=FOUR_IDS)
def test_split_start(dt, op, kind):
    """The cooperative split: the CPU folds [0, 256) through mi_host_reduce
    while the GPU folds the other 4099 elements.  The guard before the CPU's
    head and the one after the GPU's tail are intact and the whole output is
    the oracle's."""
    m = _lib.mi()
    es = _es(dt)
    n = 256 + 4099
    for mis in _mis3(es):
        ar, pa, pb, exp, flags = _one_inplace(kind, dt, op, n, mis, seed=80 + mis)
        req = ctypes.c_void_p()
        _lib.check(m.mi_reduce_split_start(_lib.void_ptr_array([pb.ptr, pa.ptr]), 2, pb.ptr, n, dt, op, flags, -1, 256,
                                           _host_fold_ptr(), ctypes.byref(req)), "mi_reduce_split_start")
        _lib.check(m.mi_wait(req), "mi_wait")
        _lib.check(m.mi_request_free(req))
        ar.check(what=f"mi_reduce_split_start ({kind}, misalignment {mis})")
        assert_same(ar.read(pb), exp, dt, f"misalignment {mis}")


# ---- the drop-in on host buffers ---------------------------------------------------

@pytest.fixture(params=["gpu-paths", "default-threshold"])
def dispatch(request):
    """CCL_COMP_HOST_MAX_BYTES=0 sends host buckets of any size to the GPU
    paths; at the default the small ones here stay on the CPU path."""
    saved = os.environ.get("CCL_COMP_HOST_MAX_BYTES")
    if request.param == "gpu-paths":
        os.environ["CCL_COMP_HOST_MAX_BYTES"] = "0"
    else:
        os.environ.pop("CCL_COMP_HOST_MAX_BYTES", None)
    comp.env_reload()
    yield request.param
    if saved is None:
        os.environ.pop("CCL_COMP_HOST_MAX_BYTES", None)
    else:
        os.environ["CCL_COMP_HOST_MAX_BYTES"] = saved
    comp.env_reload()


@pytest.mark.parametrize("dt,op", FOUR, ids=FOUR_IDS)
def test_dropin_reduce_on_host_buffers(dt, op, dispatch):
    b_impl, f_impl = comp.impl_types()
    es = _es(dt)
    flags = bf16_flags(int(b_impl)) if dt == BF16 else (F_MINMAX_INOUT_FIRST if dt == FP16 else 0)
    cases = [(n, m) for n in (1, 17, 4099, MIB // es + 5) for m in _mis3(es)]
    ar = Arena(arena_bytes(2 * sum(n for n, _ in cases) * es, 2 * len(cases)), "pageable", seed=90)
    placed = []
    for c, (n, m) in enumerate(cases):
        a = rand_array(dt, n, seed=2 * c, op=op)
        b = rand_array(dt, n, seed=2 * c + 1, op=op)
        (pb, pa), _ = ar.place_reduce([b, a], dt, op, flags, [m, (m + es) % 16], True, tag=f"c{c}.")
        exp = b.copy()
        oracle.comp_reduce(a, exp, dt, op, int(b_impl), int(f_impl))
        placed.append((pa, pb, exp, n))
    ar.snapshot()
    for pa, pb, exp, n in placed:
        comp.comp_reduce(pa.ptr, n, pb.ptr, comp.datatype(dt), comp.reduction(op))
    ar.check(what=f"ccl_comp_reduce on host buffers ({dispatch})")
    for (pa, pb, exp, n), case in zip(placed, cases):
        assert_same(ar.read(pb), exp, dt, f"{case}")


@pytest.mark.parametrize("keep", [0, 1])
def test_dropin_batch_reduce_on_host_buffers(keep, dispatch):
    """ccl_comp_batch_reduce: k peer chunks packed in tmp_buf at element
    offsets j * n (n odd), folded into inout; tmp_buf stays as it was."""
    b_impl, f_impl = comp.impl_types()
    cases = [(n, k, m) for n in (1, 17, 4099, MIB // 8 + 1) for k in (1, 4, 16) for m in (0, 2, 14)]
    ar = Arena(arena_bytes(sum(2 * n * (k + 1) for n, k, _ in cases), 2 * len(cases)), "pageable", seed=91)
    placed = []
    for c, (n, k, m) in enumerate(cases):
        chunks = [rand_array(BF16, n, seed=40 * c + j) for j in range(k)]
        inout = rand_array(BF16, n, seed=40 * c + 39)
        packed = np.concatenate(chunks)
        pt = ar.place(packed, (2 * c) % 16, "in", f"c{c}.tmp_buf")
        po = ar.place(inout, m, "inout", f"c{c}.inout")
        exp = inout.copy()
        oracle.batch_reduce(packed, [j * n for j in range(k)], n, exp, BF16, 0, keep, int(b_impl), int(f_impl))
        placed.append((pt, po, exp, n, k))
    ar.snapshot()
    for pt, po, exp, n, k in placed:
        comp.comp_batch_reduce(pt.ptr, [j * n for j in range(k)], n, po.ptr, comp.datatype.bfloat16,
                               comp.reduction.sum, keep)
    ar.check(what=f"ccl_comp_batch_reduce keep={keep} ({dispatch})")
    for (pt, po, exp, n, k), case in zip(placed, cases):
        assert_same(ar.read(po), exp, BF16, f"{case}")
