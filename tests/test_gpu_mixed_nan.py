"""NaN and Inf bits of mi_reduce_bcast_mixed, bit for bit, on each of its three
routes (the tile kernel, the grid-stride form, the element loop).

A dense table: every ordered pair of the 16 special values of the input dtype
(tests.nanvec.SPECIALS: quiet NaNs of both signs, signalling NaNs, payload
NaNs, +-inf, +-0, +-max, +-1, the smallest denormal and normal), 256 elements
per block, between two operand slots, every other slot 1.0.  At k = 1 the
table is the conversion of the specials; at k = 2 the pair is (inputs[0],
inputs[1]); at k = 3 the pair rotates through the three pairs of slots.  With
an accumulator, acc is one of the slots.  The blocks are concatenated and the
outputs placed so that the table crosses a scalar head, tile boundaries of the
body and a scalar tail.

The expectation is the composition (tests.mixed.expected_mixed).  What it
covers is asserted on the expectation itself, without a device, in
tests/test_mixed_expected.py: Inf - Inf gives x86's default
NaN 0xFFC00000; of two NaNs the accumulator's (the earlier operand's) comes
back, quieted; fp16 signalling NaNs come out quiet, at k = 1 too (bf16's do
not at k = 1: that conversion is a shift); fp32 -> fp16 overflows to Inf; the
bf16 round-to-nearest-even flushes denormals to signed zero."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.mixed import PAIR_IDS, PAIRS, call_mixed, expected_mixed, knobs
from tests.nanvec import I_ONE, SPECIALS
from tests.util import FP32, assert_same, from_dev, to_dev

pytestmark = pytest.mark.gpu

ROUTES = {"tile": dict(), "stride": dict(max_blocks=1), "elements": dict(unaligned=0)}


def _es(dt):
    return 4 if dt == FP32 else 2


@functools.lru_cache(maxsize=None)
def table(idt, k, with_acc):
    """(inputs, acc or None): the blocks of the module docstring, concatenated."""
    S = SPECIALS[idt].view(np.float32) if idt == FP32 else SPECIALS[idt]
    A, B = np.repeat(S, 16), np.tile(S, 16)
    one = np.full(256, S[I_ONE], S.dtype)
    slots = k + (1 if with_acc else 0)  # slot 0 is acc when there is one
    if slots == 1:
        cols = [[B]]
    else:
        cols = []
        for a in range(slots):
            for b in range(a + 1, slots):
                cols.append([A if s == a else B if s == b else one for s in range(slots)])
    ops = [np.concatenate([c[s] for c in cols]) for s in range(slots)]
    for o in ops:
        o.setflags(write=False)
    if not with_acc:
        return tuple(ops), None
    # acc is fp32: the same specials, in fp32 (SPECIALS[FP32] lines up with the 16-bit tables' order)
    S32 = SPECIALS[FP32].view(np.float32)
    A32, one32 = np.repeat(S32, 16), np.full(256, 1.0, np.float32)
    acc = np.concatenate([A32 if a == 0 else one32 for a in range(slots) for _ in range(a + 1, slots)])
    acc.setflags(write=False)
    return tuple(ops[1:]), acc


CASES = [(1, False), (2, False), (3, False), (1, True), (2, True)]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_special_table(idt, odt, flags, route):
    import torch
    esi, eso = _es(idt), _es(odt)
    head = 16 // eso - 1                       # the longest scalar head
    out_off = 16 // eso - head                 # elements into a 256-byte aligned buffer
    in_off = (16 // esi - head) % (16 // esi)  # element `head` on a 16-byte boundary
    acc_off = (4 - head) % 4
    if route == "elements":                    # one element off the grid, unaligned vectors off
        in_off, acc_off = in_off + 1, acc_off + 1
    stream = torch.cuda.current_stream().cuda_stream
    for k, with_acc in CASES:
        if with_acc and odt != FP32:
            continue
        ins, acc = table(idt, k, with_acc)
        n = ins[0].size
        assert (n - head) // 8 >= 1 and (n - head) % 8 != 0  # a body and a scalar tail
        exp = expected_mixed(list(ins), idt, odt, flags, acc)
        for inplace in ((False, True) if with_acc else (False,)):
            held = [to_dev(a, 64, in_off, guard_seed=11 + j) for j, a in enumerate(ins)]
            m = 2
            outs = [to_dev(np.full(n, 0x5A5A5A5A if eso == 4 else 0x5A5A, exp.dtype if eso == 2 else np.uint32)
                           .view(exp.dtype), 64, out_off, guard_seed=31 + o) for o in range(m)]
            pacc = None
            if with_acc:
                hacc = to_dev(acc, 64, out_off if inplace else acc_off, guard_seed=51)
                pacc = hacc[1]
                if inplace:
                    outs[0] = hacc
            with knobs(**ROUTES[route]):
                call_mixed([p for _, p in held], idt, [p for _, p in outs], odt, n, flags, pacc, stream)
                torch.cuda.synchronize()
            for o, (t, _) in enumerate(outs):
                assert_same(from_dev(t, exp, out_off), exp, odt,
                            f"{route} k={k} acc={with_acc} in place={inplace}: output {o}")
            for j, ((t, _), a) in enumerate(zip(held, ins)):
                assert_same(from_dev(t, a, in_off), a, idt, f"inputs[{j}] changed")
