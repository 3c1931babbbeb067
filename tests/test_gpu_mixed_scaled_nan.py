"""NaN and Inf bits of mi_reduce_bcast_mixed_scaled at scale -2.5, bit for bit,
on each of its three routes (the tile kernel, the grid-stride form, the
element loop).

The table is tests/test_gpu_mixed_nan.py's: every ordered pair of the 16
special values of the input dtype (tests.nanvec.SPECIALS) between two operand
slots, every other slot 1.0; k = 1, 2 and 3, with and without an accumulator
(acc one of the slots), placed so that it crosses a scalar head, tile
boundaries and a scalar tail.  The expectation is
tests.mixed_scaled.expected_mixed_scaled; what it has to say about the table is
asserted on the expectation itself, without a device, by the first tests here:
a NaN keeps its payload and its sign through the negative multiplier, a
signalling fp16 NaN comes out quiet, a NaN accumulator wins over a NaN product,
Inf times the scale added to the accumulator's opposite Inf is x86's default
NaN."""
from __future__ import annotations

import numpy as np
import pytest

from tests.mixed import PAIR_IDS, PAIRS, expected_mixed, knobs
from tests.mixed_scaled import call_mixed_scaled, expected_mixed_scaled
from tests.nanvec import SPECIALS
from tests.test_gpu_mixed_nan import ROUTES, _es, table
from tests.util import BF16, FP16, FP32, assert_same, from_dev, to_dev

pytestmark = pytest.mark.gpu

SCALE = -2.5
CASES = [(1, False), (2, False), (3, False), (1, True), (2, True), (3, True)]


def _u32(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("idt", [BF16, FP16], ids=["bf16", "fp16"])
def test_table_expectation_payloads(idt):
    S = SPECIALS[idt]
    top = 0x7F80 if idt == BF16 else 0x7C00
    nan = [i for i in range(16) if (int(S[i]) & 0x7FFF) > top]
    assert len(nan) == 6
    wide = _u32(expected_mixed([S], idt, FP32, 0))               # k = 1 unscaled: the conversion
    k1 = _u32(expected_mixed_scaled([S], idt, FP32, 0, SCALE))
    for i in nan:  # the NaN as the unscaled call stores it: payload and sign kept under a negative scale
        assert k1[i] == wide[i]
    if idt == FP16:  # signalling fp16 NaNs are quieted (bf16's are not at k = 1: that conversion is a shift)
        assert any(not int(S[i]) & 0x0200 for i in nan) and all(int(k1[i]) & 0x00400000 for i in nan)
    (a, b), _ = table(idt, 2, False)
    e = _u32(expected_mixed_scaled([a, b], idt, FP32, 0, SCALE))
    for i in nan:
        for j in nan:  # of two NaNs the earlier operand's, quieted, whatever the multiplier's sign
            assert e[i * 16 + j] == wide[i] | 0x00400000
    # with an accumulator: its NaN wins over a NaN product, and Inf * s + (the other Inf) is the default NaN
    (b1,), acc = table(idt, 1, True)
    ea = _u32(expected_mixed_scaled([b1], idt, FP32, 0, SCALE, acc))
    w = wide.view(np.float32)[np.arange(256) % 16]
    both = np.flatnonzero(np.isnan(acc) & np.isnan(w))
    assert both.size == 36 and (ea[both] == (_u32(acc)[both] | 0x00400000)).all()
    with np.errstate(all="ignore"):
        clash = np.flatnonzero(np.isinf(acc) & np.isinf(w) & (np.sign(acc) == np.sign(w)))  # -2.5 flips the product's
    assert clash.size == 2 and (ea[clash] == 0xFFC00000).all()


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
        exp = expected_mixed_scaled(list(ins), idt, odt, flags, SCALE, acc)
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
                call_mixed_scaled([p for _, p in held], idt, [p for _, p in outs], odt, n, flags, SCALE, pacc, stream)
                torch.cuda.synchronize()
            for o, (t, _) in enumerate(outs):
                assert_same(from_dev(t, exp, out_off), exp, odt,
                            f"{route} k={k} acc={with_acc} in place={inplace}: output {o}")
            for j, ((t, _), a) in enumerate(zip(held, ins)):
                assert_same(from_dev(t, a, in_off), a, idt, f"inputs[{j}] changed")
