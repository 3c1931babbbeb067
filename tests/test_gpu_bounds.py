"""No device kernel writes outside its output.

The parity tests pin what each kernel writes inside its output; here every
kernel family runs between guards (tests/guard.py) at the edges of its tile:
body lengths of 0, 1, T-1, T, T+1 and 2T+1 16-byte vectors (T = 64 for the
lean, batch, fan and lean copy kernels, 1024 for the grid-stride general and
copy kernels), crossed with scalar heads and tails of 0, 1 and 16/es - 1
elements, and one element at misalignment es.  Since the 2-input and fan-in
kernels take every operand through a per-tile buffer descriptor, the
descriptor's range is all that keeps the last tile's extra lanes from
storing; a lane that got through would load zeros and store op(0, 0), or, in
place, fold its neighbours.  The guards are non-zero and drawn so that either
changes bits (guard_elems).  Many cases share one arena and one snapshot, so
a test is a few hundred launches and one comparison of the whole arena; the
output bits are checked against the oracle as well.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

from oneccl_amd import _lib, comp
from oneccl_amd.comp import F_ACC_FP32, F_BF16_RNE, F_BF16_TAIL_TRUNC16, F_MINMAX_INOUT_FIRST
from tests.guard import DT_OP, DT_OP_IDS, T_GENERAL, T_LEAN, Arena, arena_bytes, oracle_fold
from tests.guard import es_of as _es
from tests.guard import ref_flags as _flags
from tests.guard import tile_shapes as shapes
from tests.util import BF16, FP16, FP32, FP64, assert_same, convert_expected, rand_array

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def Knobs(max_blocks=0, unaligned=1):
    """mi_set_max_blocks / mi_set_unaligned_vectors for a block; both are put
    back to what was in force before, whichever of the two calls fails."""
    m = _lib.mi()
    blk, unr, prev_cap = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(m.mi_get_launch_config(ctypes.byref(blk), ctypes.byref(unr), ctypes.byref(prev_cap)))
    prev_un = m.mi_set_unaligned_vectors(unaligned)
    try:
        _lib.check(m.mi_set_max_blocks(max_blocks))
        yield
    finally:
        m.mi_set_unaligned_vectors(prev_un)
        _lib.check(m.mi_set_max_blocks(prev_cap.value))


def _launch(entry, ins, out, n, dt, op, flags):
    m = _lib.mi()
    if entry == "reduce":  # inout = op(in, inout)
        assert out is ins[0] and len(ins) == 2
        _lib.check(m.mi_reduce(ins[1].ptr, ins[0].ptr, n, dt, op, flags, _stream()))
    elif entry == "reduce_out":  # out = op(in1 [in role], in2 [inout role])
        assert len(ins) == 2
        _lib.check(m.mi_reduce_out(ins[1].ptr, ins[0].ptr, out.ptr, n, dt, op, flags, _stream()))
    else:
        arr = _lib.void_ptr_array([o.ptr for o in ins])
        _lib.check(m.mi_reduce_multi(arr, len(ins), out.ptr, n, dt, op, flags, _stream()))


def run_reduces(cases, what, seed=0, **knobs):
    """cases: (dt, op, flags, k, count, [input misalignments], out
    misalignment, inplace, entry).  All placed in one arena, launched on the
    current stream under `knobs`, then one bounds check and a bit-exact
    comparison of every output with the oracle."""
    import torch
    total = sum((c[3] + 1) * c[4] * _es(c[0]) for c in cases)
    ar = Arena(arena_bytes(total, sum(c[3] + 1 for c in cases)), "device", seed=seed)
    placed = []
    for i, (dt, op, flags, k, n, mis, out_mis, inplace, entry) in enumerate(cases):
        ins = [rand_array(dt, n, seed=1000 * seed + 17 * i + j, op=op) for j in range(k)]
        pin, pout = ar.place_reduce(ins, dt, op, flags, mis, inplace, out_mis, tag=f"c{i}.")
        placed.append((pin, pout, oracle_fold(ins, dt, op, flags) if n else ins[0]))
    ar.snapshot()
    with Knobs(**knobs):
        for (dt, op, flags, k, n, mis, out_mis, inplace, entry), (pin, pout, _) in zip(cases, placed):
            _launch(entry, pin, pout, n, dt, op, flags)
        torch.cuda.synchronize()
    ar.check(what=what)
    for c, (pin, pout, exp) in zip(cases, placed):
        if c[4]:
            assert_same(ar.read(pout), exp, c[0], f"{what}: case (dt, op, flags, k, count, mis, out_mis, inplace, "
                                                  f"entry) = {c}")


def _common(dt, op, k, T, entries, flags=None):
    """Cases with every operand at the output's misalignment."""
    flags = _flags(dt) if flags is None else flags
    return [(dt, op, flags, k, n, [m] * k, m, inplace, entry) for n, m in shapes(_es(dt), T)
            for inplace, entry in entries]


# ---- the device and pinned arenas can fail ------------------------------------------

@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_arena_flags_a_stray_store(kind):
    """tests/test_guard_selftest.py shows on pageable memory that check()
    flags every kind of spill; the same for the two arena kinds that need a
    GPU, with the stray store done by a torch slice assignment."""
    import torch
    a = rand_array(FP32, 1003, seed=1)
    b = rand_array(FP32, 1003, seed=2)
    exp = oracle_fold([b, a], FP32, 0, 0)
    ar = Arena(arena_bytes(2 * a.nbytes, 2), kind, seed=3)
    (pb, pa), _ = ar.place_reduce([b, a], FP32, 0, 0, [4, 4], True)
    ar.snapshot()
    skip = ar.base - ar.t.data_ptr()
    ar.t[skip + pb.off:skip + pb.end] = torch.from_numpy(exp.view(np.uint8)).to(ar.t.device)  # the output only
    torch.cuda.synchronize()
    ar.check()
    assert_same(ar.read(pb), exp, FP32)
    ar.t[skip + pb.end:skip + pb.end + 16] = 0  # one vector of zeros past the end
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="16 bytes outside the output changed.*0 bytes after the end of inout"):
        ar.check()


# ---- reduce2_kernel --------------------------------------------------------

@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_lean_two_input_kernel(dt, op):
    """reduce2_kernel: mi_reduce in place and mi_reduce_out with the output's
    guards separate from both inputs'."""
    run_reduces(_common(dt, op, 2, T_LEAN, [(True, "reduce"), (False, "reduce_out")]), "reduce2_kernel",
                seed=dt * 4 + op)


# ---- reduce2_batch_kernel --------------------------------------------------

@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_batch_kernel(dt, op):
    """reduce2_batch_kernel: 3, 64 and 65 descriptors (one launch, one full
    launch, a full one and a second) of ragged counts, empty ones and ones
    without a vector body among them."""
    import torch
    es, flags = _es(dt), _flags(dt)
    shp = shapes(es, T_LEAN)
    ndesc = (3, 64, 65)
    ar = Arena(arena_bytes(2 * sum(ndesc) * (2 * T_LEAN + 3) * 16, 2 * sum(ndesc)), "device", seed=100 + dt)
    batches = []
    i = 0
    for nd in ndesc:
        batch = []
        for _ in range(nd):
            n, m = shp[(7 * i) % len(shp)]
            i += 1
            a = rand_array(dt, n, seed=5000 + 2 * i, op=op)
            b = rand_array(dt, n, seed=5001 + 2 * i, op=op)
            (pb, pa), _ = ar.place_reduce([b, a], dt, op, flags, [m, m], True, tag=f"d{i}.")
            batch.append((pa, pb, n, oracle_fold([b, a], dt, op, flags) if n else b))
        batches.append(batch)
    ar.snapshot()
    for batch in batches:
        descs = _lib.desc_array([(pa.ptr, pb.ptr, n) for pa, pb, n, _ in batch])
        _lib.check(_lib.mi().mi_reduce_batch(descs, len(batch), dt, op, flags, _stream()), "mi_reduce_batch")
    torch.cuda.synchronize()
    ar.check(what="reduce2_batch_kernel")
    for batch in batches:
        for pa, pb, n, exp in batch:
            if n:
                assert_same(ar.read(pb), exp, dt, f"descriptor {pb.name} count {n}")


# ---- fan_kernel<..., 8> / <..., 16> ------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 8, 9, 16])
@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_fan_kernel(dt, op, k):
    """fan_kernel with 8 and 16 input slots (k <= 8 / k > 8), in place and out
    of place: the packed 8- and 16-bit integer fold and the widened fold.
    k = 1 out of place is a device copy, in place nothing."""
    run_reduces(_common(dt, op, k, T_LEAN, [(True, "multi"), (False, "multi")]), f"fan_kernel k={k}",
                seed=300 + dt * 4 + op)


@pytest.mark.parametrize("dt,flags", [(BF16, F_ACC_FP32), (BF16, F_ACC_FP32 | F_BF16_RNE | F_MINMAX_INOUT_FIRST),
                                      (FP16, F_ACC_FP32 | F_MINMAX_INOUT_FIRST)],
                         ids=["bf16-acc32-trunc", "bf16-acc32-rne", "fp16-acc32"])
def test_fan_kernel_fp32_accumulate(dt, flags):
    cases = []
    for k, op in ((3, 0), (9, 3)):
        cases += _common(dt, op, k, T_LEAN, [(True, "multi"), (False, "multi")], flags)
    run_reduces(cases, "fan_kernel fp32-accumulate", seed=400 + dt)


# ---- reduce_kernel: grid-stride tiles under a grid cap ---------------------------

@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_general_kernel_under_grid_cap(dt, op, cap):
    """mi_set_max_blocks(1) / (3): one block of reduce_kernel strides over
    several 16 KiB tiles and ends in the guarded partial tile."""
    cases = _common(dt, op, 2, T_GENERAL, [(True, "reduce"), (False, "reduce_out")])
    cases += _common(dt, op, 3, T_GENERAL, [(True, "multi"), (False, "multi")])
    run_reduces(cases, f"reduce_kernel max_blocks={cap}", seed=500 + dt, max_blocks=cap)


# ---- operands at differing misalignments ------------------------------------------

def _differing(dt, op, k, T, entries):
    es = _es(dt)
    per = 16 // es
    out = []
    for i, (n, m) in enumerate(shapes(es, T)):
        mis = [((m // es + 1 + j + i) % per) * es for j in range(k)]
        for inplace, entry in entries:
            mm = list(mis)
            if inplace:
                mm[0] = m
            if all(x == m for x in mm):
                mm[-1] = (m + es) % 16
            out.append((dt, op, _flags(dt), k, n, mm, m, inplace, entry))
    return out


@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_unaligned_vector_loads(dt, op):
    """mi_set_unaligned_vectors(1): the vector kernels on the output's 16-byte
    grid with each input at its own misalignment, k = 2 (lean) and k = 5 (fan)."""
    cases = _differing(dt, op, 2, T_LEAN, [(True, "reduce"), (False, "reduce_out")])
    cases += _differing(dt, op, 5, T_LEAN, [(True, "multi"), (False, "multi")])
    run_reduces(cases, "unaligned vectors", seed=600 + dt, unaligned=1)


@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_element_loop(dt, op):
    """mi_set_unaligned_vectors(0) with differing misalignments: the general
    kernel's element loop, k = 2 and k = 5."""
    cases = _differing(dt, op, 2, T_LEAN, [(True, "reduce"), (False, "reduce_out")])
    cases += _differing(dt, op, 5, T_LEAN, [(True, "multi"), (False, "multi")])
    run_reduces(cases, "element loop", seed=700 + dt, unaligned=0)


@pytest.mark.parametrize("unaligned", [0, 1])
def test_element_loop_byte_misaligned_fp32(unaligned):
    """fp32 operands at odd byte offsets are not element-aligned: the element
    loop whatever the knob says."""
    cases = []
    for n in (1, 3, 255, 256, 257, 4 * T_LEAN + 1, 8 * T_LEAN + 5):
        for mis, om in (([1, 1], 1), ([1, 3], 7), ([0, 5], 0), ([2, 0], 15)):
            for op in (0, 3):
                cases.append((FP32, op, 0, 2, n, [om, mis[1]], om, True, "reduce"))
                cases.append((FP32, op, 0, 2, n, mis, om, False, "reduce_out"))
                cases.append((FP32, op, 0, 3, n, mis + [9], om, False, "multi"))
    run_reduces(cases, "element loop, byte-misaligned fp32", seed=800 + unaligned, unaligned=unaligned)


# ---- convert_kernel --------------------------------------------------------

CONV_PAIRS = [(FP32, BF16, F_BF16_RNE | F_BF16_TAIL_TRUNC16), (FP32, BF16, 0), (FP32, FP16, 0), (BF16, FP32, 0),
              (FP16, FP32, 0)]
CONV_COUNTS = [1, 7, 8, 9, 511, 512, 513, 1024 + 8 * 3 + 5]


@pytest.mark.parametrize("mode", ["default", "one-block", "element-loop"])
@pytest.mark.parametrize("sdt,ddt,flags", CONV_PAIRS, ids=["f32-bf16rne-tail", "f32-bf16trunc", "f32-f16", "bf16-f32",
                                                           "f16-f32"])
def test_convert_kernel(sdt, ddt, flags, mode):
    """The non-streaming convert_kernel: counts around the 512-element wave
    chunk (two runs of 4 per lane), the 8-per-lane remainder loop, the head
    and tail lanes; under mi_set_max_blocks(1) one block strides over the
    wave chunks and then the remainder; the element loop for sources off the
    vector path."""
    import torch
    ss, ds = _es(sdt), _es(ddt)
    cases = []
    for n in CONV_COUNTS:
        for head in sorted({0, 1, 16 // ds - 1}):
            for smis in sorted({0, ss, 16 - ss}):
                if mode == "element-loop" and head == 0 and smis == 0:
                    continue  # both 16-byte aligned: the vector path whatever the knob
                cases.append((n, (16 - head * ds) % 16, smis))
    ar = Arena(arena_bytes(sum(n * (ss + ds) for n, _, _ in cases), 2 * len(cases)), "device", seed=sdt * 16 + ddt)
    placed = []
    for c, (n, dmis, smis) in enumerate(cases):
        src = rand_array(sdt, n, seed=900 + c)
        ps = ar.place(src, smis, "in", f"c{c}.src")
        noise = np.full(n * ds, 0x5A, np.uint8).view(np.uint32 if ds == 4 else np.uint16)
        pd = ar.place(noise, dmis, "out", f"c{c}.dst")
        placed.append((ps, pd, convert_expected(src, sdt, ddt, flags), n))
    ar.snapshot()
    knobs = {"default": {}, "one-block": {"max_blocks": 1}, "element-loop": {"unaligned": 0}}[mode]
    with Knobs(**knobs):
        for ps, pd, exp, n in placed:
            _lib.check(_lib.mi().mi_convert(ps.ptr, sdt, pd.ptr, ddt, n, flags, _stream()), "mi_convert")
        torch.cuda.synchronize()
    ar.check(what=f"convert_kernel {mode}")
    for (ps, pd, exp, n), case in zip(placed, cases):
        assert np.array_equal(ar.read(pd).view(np.uint8), exp.view(np.uint8)), \
            f"(count, dst misalignment, src misalignment) = {case}"


# ---- copy_lean_kernel<1/3>, copy_kernel<1/3> -------------------------------------

@pytest.mark.parametrize("cap,T", [(0, T_LEAN), (3, T_GENERAL)], ids=["copy_lean_kernel", "copy_kernel-cap3"])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("entry", ["mi_copy", "comp_copy"])
def test_copy_kernels(entry, nt, cap, T):
    """Byte copies between random non-zero guards: head and tail bytes of 0,
    1 and 15, the source at its own byte offset; the lean kernel by default,
    the grid-stride one under mi_set_max_blocks(3).  comp_copy is the drop-in
    ccl_comp_copy on device pointers (the library's own stream)."""
    import torch
    cases = [(h + 16 * b + t, (16 - h) % 16, (3 * i + h) % 16) for i, (b, h, t) in enumerate(
        (b, h, t) for b in (0, 1, T - 1, T, T + 1, 2 * T + 1) for h in (0, 1, 15) for t in (0, 1, 15))]
    cases.append((1, 5, 0))
    ar = Arena(arena_bytes(2 * sum(c[0] for c in cases), 2 * len(cases)), "device", seed=nt + 2 * cap)
    rng = np.random.default_rng(11)
    placed = []
    for c, (n, dmis, smis) in enumerate(cases):
        src = rng.integers(0, 256, n, dtype=np.uint8)
        ps = ar.place(src, smis, "in", f"c{c}.src")
        pd = ar.place(rng.integers(1, 255, n, dtype=np.uint8), dmis, "out", f"c{c}.dst")
        placed.append((ps, pd, src))
    ar.snapshot()  # synchronises: comp_copy runs on the library's stream
    with Knobs(max_blocks=cap):
        for ps, pd, src in placed:
            if entry == "mi_copy":
                _lib.check(_lib.mi().mi_copy(ps.ptr, pd.ptr, src.size, nt, _stream()), "mi_copy")
            elif src.size:
                comp.comp_copy(ps.ptr, pd.ptr, src.size, bool(nt))
        torch.cuda.synchronize()
    ar.check(what=f"{entry} nontemporal={nt} max_blocks={cap}")
    for (ps, pd, src), case in zip(placed, cases):
        assert np.array_equal(ar.read(pd), src), f"(bytes, dst misalignment, src misalignment) = {case}"


# ---- workload shapes -------------------------------------------------------

CHUNKS = [1, 77, 3, 1025, 255, 129, 2049]  # odd counts: the starts fall on every element misalignment


@pytest.mark.parametrize("how", ["separate-calls", "one-batch"])
@pytest.mark.parametrize("in_shift", [0, 1], ids=["common-alignment", "in-shifted-one-element"])
@pytest.mark.parametrize("op", [0, 3], ids=["sum", "max"])
@pytest.mark.parametrize("dt", [FP32, BF16, 0], ids=["f32", "bf16", "i8"])
def test_contiguous_ragged_chunks_in_one_bucket(dt, op, in_shift, how):
    """The reduce-scatter layout: one inout bucket and one in bucket cut into
    7 touching chunks of odd counts, reduced chunk by chunk in a shuffled
    order or by one mi_reduce_batch of the 7 touching descriptors.  A spill
    into a neighbouring chunk changes that chunk's input or result, so the
    whole bucket must equal the oracle's reduce of the whole bucket, and the
    bucket's outer guards stay as they were."""
    import torch
    es, flags = _es(dt), _flags(dt)
    total = sum(CHUNKS)
    a = rand_array(dt, total, seed=31 + dt, op=op)
    b = rand_array(dt, total, seed=32 + dt, op=op)
    # the oracle chunk by chunk: the bf16 / fp16 folds do not depend on where a chunk is cut,
    # but this restates exactly what is asked of the library
    exp = b.copy()
    starts = np.concatenate([[0], np.cumsum(CHUNKS)[:-1]]).tolist()
    for s, n in zip(starts, CHUNKS):
        exp[s:s + n] = oracle_fold([b[s:s + n], a[s:s + n]], dt, op, flags)
    assert_same(exp, oracle_fold([b, a], dt, op, flags), dt, "oracle: chunked == whole")
    ar = Arena(arena_bytes(2 * a.nbytes, 2), "device", seed=dt + op)
    (pb, pa), _ = ar.place_reduce([b, a], dt, op, flags, [0, (in_shift * es) % 16], True)
    ar.snapshot()
    order = np.random.default_rng(5).permutation(len(CHUNKS)).tolist()
    trip = [(pa.ptr + starts[i] * es, pb.ptr + starts[i] * es, CHUNKS[i]) for i in order]
    if how == "one-batch":
        _lib.check(_lib.mi().mi_reduce_batch(_lib.desc_array(trip), len(trip), dt, op, flags, _stream()))
    else:
        for pin, pio, n in trip:
            _lib.check(_lib.mi().mi_reduce(pin, pio, n, dt, op, flags, _stream()))
    torch.cuda.synchronize()
    ar.check(what="ragged chunks in one bucket")
    assert_same(ar.read(pb), exp, dt, "whole bucket")


@pytest.mark.parametrize("inplace", [True, False], ids=["into-chunk-0", "out-of-place"])
@pytest.mark.parametrize("dt,op", [(FP32, 0), (BF16, 0), (0, 3), (FP64, 2)], ids=["f32-sum", "bf16-sum", "i8-max",
                                                                                 "f64-min"])
def test_packed_tmp_buf(dt, op, inplace):
    """ccl_comp_batch_reduce's layout: k = 4 peer chunks contiguous in one
    allocation at element offsets j * n with n odd, folded by mi_reduce_multi
    into chunk 0 or into a separate output.  Chunks 1 to 3 are unchanged."""
    import torch
    es, flags, k = _es(dt), _flags(dt), 4
    for n in (1, 63, 16 // es * T_LEAN + 1, 4099):
        chunks = [rand_array(dt, n, seed=70 + j, op=op) for j in range(k)]
        ar = Arena(arena_bytes((k + 1) * n * es, 2), "device", seed=n)
        ptmp = ar.place(np.concatenate(chunks), 0, "in", "tmp_buf")
        subs = [ar.sub(ptmp, j * n, n, "inout" if inplace and j == 0 else "in", f"chunk{j}") for j in range(k)]
        pout = subs[0] if inplace else ar.place(rand_array(dt, n, seed=99, op=op, specials=False), es, "out", "out")
        ar.snapshot()
        arr = _lib.void_ptr_array([s.ptr for s in subs])
        _lib.check(_lib.mi().mi_reduce_multi(arr, k, pout.ptr, n, dt, op, flags, _stream()))
        torch.cuda.synchronize()
        ar.check(what=f"packed tmp_buf n={n}")
        assert_same(ar.read(pout), oracle_fold(chunks, dt, op, flags), dt, f"n={n}")
        for j in range(1, k):
            assert_same(ar.read(subs[j]), chunks[j], dt, f"chunk {j} changed (n={n})")
