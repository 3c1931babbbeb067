"""The guard mechanism (tests/guard.py) can fail: on a pageable arena, with no
GPU, every kind of spill the bounds tests look for is performed here with
numpy writes and must be flagged, and a call that writes only its output must
not be.  guard_elems' conditions are checked for every dtype x op x input
count and the fp32-accumulate / bf16 truncate and RNE variants.
"""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd.comp import F_ACC_FP32, F_BF16_RNE, F_MINMAX_INOUT_FIRST, bf16_flags
from tests import guard
from tests.guard import GUARD, Arena, guard_conditions, guard_elems, oracle_fold
from tests.util import ALL_DTYPES, BF16, DT_NAME, FP16, FP32, OP_NAME, OPS, rand_array

import oracle

VARIANTS = [(dt, 0) for dt in ALL_DTYPES if dt not in (BF16, FP16)]
VARIANTS += [(BF16, bf16_flags(v)) for v in (0, 1, 2)] + [(FP16, F_MINMAX_INOUT_FIRST)]
VARIANTS += [(BF16, F_ACC_FP32), (BF16, F_ACC_FP32 | F_BF16_RNE | F_MINMAX_INOUT_FIRST),
             (FP16, F_ACC_FP32 | F_MINMAX_INOUT_FIRST)]


@pytest.mark.parametrize("dt,flags", VARIANTS, ids=[f"{DT_NAME[d]}-f{f:x}" for d, f in VARIANTS])
@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
def test_guard_elems_conditions(dt, flags, op):
    es = np.dtype(oracle.NP_DTYPE[dt]).itemsize
    n = GUARD // es
    for k in (2, 3, 16):
        for inplace in (False, True):
            ing, out = guard_elems(dt, op, k, n, flags, inplace, seed=k)
            assert len(ing) == k and all(g.size == n for g in ing) and out.size == n
            assert (out is ing[0]) == inplace
            # restated here rather than through guard_conditions()
            ob = guard._bits(out)
            assert (ob != 0).all()
            assert (ob != guard._bits(oracle_fold([np.zeros_like(out)] * k, dt, op, flags))).all()
            assert (ob != guard._bits(oracle_fold(ing, dt, op, flags))).all()
            assert not guard_conditions(ing, out, dt, op, flags, inplace).any()


def _setup(dt=FP32, op=3, n=1000 + 3, mis=4, inplace=True):
    """An in-place 2-input reduce placed in a pageable arena; returns the
    arena, operands and the expected output."""
    a = rand_array(dt, n, seed=1, op=op)
    b = rand_array(dt, n, seed=2, op=op)
    ar = Arena(guard.arena_bytes(3 * a.nbytes, 3), "pageable", seed=5)
    ins, out = ar.place_reduce([b, a], dt, op, 0, [mis, mis], inplace, out_mis=mis)
    ar.snapshot()
    exp = oracle_fold([b, a], dt, op, 0)
    return ar, ins, out, exp


def _write_output(ar, out, exp):
    ar.mem[out.off:out.end] = exp.view(np.uint8)


@pytest.mark.parametrize("inplace", [True, False])
def test_clean_call_passes(inplace):
    ar, ins, out, exp = _setup(inplace=inplace)
    _write_output(ar, out, exp)
    ar.check()
    assert np.array_equal(ar.read(out).view(np.uint32), exp.view(np.uint32))
    for o in ins:
        if o is not out:
            assert np.array_equal(ar.read(o).view(np.uint32), ar.original(o).view(np.uint32))


def test_zero_store_past_the_output_is_flagged():
    """A lane past the end that loaded zeros and stored op(0, 0): 16 zero
    bytes right after the output."""
    ar, ins, out, exp = _setup(inplace=False)
    _write_output(ar, out, exp)
    ar.mem[out.end:out.end + 16] = 0
    with pytest.raises(AssertionError, match=r"16 bytes outside the output changed.*0 bytes after the end of out operand out"):
        ar.check()


@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
@pytest.mark.parametrize("dt", [FP32, BF16, 0, 10], ids=["f32", "bf16", "i8", "f64"])
def test_rmw_spill_in_place_is_flagged(dt, op):
    """In place, a spilling lane folds its neighbours: the fold of the guard
    elements stored over the first guard element after the output.  For
    min/max over arbitrary guards that is often the identity; guard_elems
    makes it a change."""
    flags = bf16_flags(2) if dt == BF16 else 0
    n = 301
    a = rand_array(dt, n, seed=1, op=op)
    b = rand_array(dt, n, seed=2, op=op)
    ar = Arena(guard.arena_bytes(2 * a.nbytes, 2), "pageable", seed=9)
    ins, out = ar.place_reduce([b, a], dt, op, flags, [0, 0], True)
    ar.snapshot()
    _write_output(ar, out, oracle_fold([b, a], dt, op, flags))
    es = a.itemsize
    g_acc = ar.mem[ins[0].end:ins[0].end + es].view(a.dtype).copy()
    g_in = ar.mem[ins[1].end:ins[1].end + es].view(a.dtype).copy()
    ar.mem[out.end:out.end + es] = oracle_fold([g_acc, g_in], dt, op, flags).view(np.uint8)
    with pytest.raises(AssertionError, match="0 bytes after the end of inout operand in0"):
        ar.check()


def test_byte_before_the_output_is_flagged():
    ar, ins, out, exp = _setup()
    _write_output(ar, out, exp)
    ar.mem[out.off - 1] ^= 0x40
    with pytest.raises(AssertionError, match="1 bytes outside the output changed.*1 bytes before inout operand in0"):
        ar.check()


def test_changed_input_is_flagged():
    ar, ins, out, exp = _setup()
    _write_output(ar, out, exp)
    o = ins[1]
    ar.mem[o.off + 4 * 17:o.off + 4 * 18] ^= 0xFF
    with pytest.raises(AssertionError, match=f"byte {4 * 17} inside in operand in1"):
        ar.check()


def test_store_one_tile_past_the_end_is_flagged():
    """A store one lean tile (1 KiB) beyond the end: far from the output's
    edge, still inside its guard."""
    ar, ins, out, exp = _setup(inplace=False)
    _write_output(ar, out, exp)
    ar.mem[out.end + 1024:out.end + 1024 + 16] = ar.mem[out.end + 1024:out.end + 1024 + 16] ^ 0x81
    with pytest.raises(AssertionError, match="1024 bytes after the end of out operand out"):
        ar.check()


@pytest.mark.parametrize("dt,off", [(FP32, 3), (BF16, 0), (0, 15), (10, 1)])
def test_to_dev_guards(dt, off):
    """tests/util.py padded() / guards_intact(), what to_dev(guard_seed=...)
    and the fuzz sweeps use: non-zero pads, a changed pad byte on either side
    is flagged, the operand's own bytes are not looked at."""
    from tests.util import guards_intact, padded
    x = rand_array(dt, 1001, seed=1)
    es = x.itemsize
    raw = padded(x, 16, off, guard_seed=77)
    pads = np.concatenate([raw[:off], raw[off + x.size:]]).view(np.uint8)
    assert pads.min() >= 1 and pads.max() <= 254
    assert np.array_equal(raw[off:off + x.size].view(np.uint8), x.view(np.uint8))
    assert not padded(x, 16, off)[:off].any()  # the default is still zeros
    guards_intact(raw, x, off, 77)
    inside = raw.copy()
    inside.view(np.uint8)[off * es:(off + x.size) * es] ^= 0xFF
    guards_intact(inside, x, off, 77)
    after = raw.copy()
    after.view(np.uint8)[(off + x.size) * es + 3] = 0
    with pytest.raises(AssertionError, match="first 3 bytes after its end"):
        guards_intact(after, x, off, 77)
    if off:
        before = raw.copy()
        before.view(np.uint8)[off * es - 1] = 0
        with pytest.raises(AssertionError, match="first 1 bytes before the operand"):
            guards_intact(before, x, off, 77)


def test_arena_has_no_zero_byte_and_places_at_the_asked_misalignment():
    ar = Arena(1 << 20, "pageable", seed=3)
    assert ar.mem.min() >= 1 and ar.mem.max() <= 254
    for mis in (0, 1, 2, 4, 8, 15):
        o = ar.place(np.arange(100, dtype=np.uint8), mis)
        assert o.ptr % 16 == mis
    offs = [(o.off, o.end) for o in ar.ops]
    assert offs[0][0] >= GUARD
    assert all(b[0] - a[1] >= GUARD for a, b in zip(offs, offs[1:]))
    assert ar.size - offs[-1][1] >= GUARD
