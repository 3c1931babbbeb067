"""The CPU construction the GPU tests of mi_reduce_bcast_mixed compare against
(tests.mixed.expected_mixed), checked where it can be without a device.

The widened sum is the fp32 accumulator of the MI_F_ACC_FP32 fold before its
one rounding: narrowing it with the array conversion under the flags'
rounding bits gives the oracle's keep-precision fold of the 16-bit inputs, bit
for bit.  And for k = 1 both directions are the array conversion."""
from __future__ import annotations

import numpy as np
import pytest

from tests.guard import oracle_fold
from tests.mixed import F_RNE, NARROWING, SUM, expected_mixed
from tests.nanvec import SPECIALS
from tests.test_gpu_mixed_nan import table
from tests.util import BF16, FP16, FP32, assert_same, convert_expected, rand_array

N = 3 * 4096 + 5


def _inputs(dt, k, seed):
    return [rand_array(dt, N, seed=seed + 17 * j) for j in range(k)]


@pytest.mark.parametrize("dt,flags", [(BF16, 0x4), (BF16, 0x5), (BF16, 0x6), (BF16, 0x7), (FP16, 0x4), (FP16, 0x5)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
def test_narrowed_widening_is_the_acc_fp32_fold(dt, flags, k):
    assert N > 40  # rand_array's specials are present
    ins = _inputs(dt, k, 300 + k)
    wide = expected_mixed(ins, dt, FP32, flags)
    assert_same(convert_expected(wide, FP32, dt, flags), oracle_fold(ins, dt, SUM, flags), dt, f"k={k} flags={flags:#x}")


@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
def test_widening_k1_is_the_conversion(dt):
    x = _inputs(dt, 1, 41)
    assert_same(expected_mixed(x, dt, FP32, 0), convert_expected(x[0], dt, FP32, 0), FP32)


@pytest.mark.parametrize("idt,odt,flags", NARROWING, ids=lambda v: str(v))
def test_narrowing_k1_is_the_conversion(idt, odt, flags):
    x = _inputs(FP32, 1, 43)
    assert_same(expected_mixed(x, FP32, odt, flags), convert_expected(x[0], FP32, odt, flags), odt)


# ---- what the special-value table of tests/test_gpu_mixed_nan.py covers -----------------------------

def _u32(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("idt", [BF16, FP16], ids=["bf16", "fp16"])
def test_table_expectation_widening(idt):
    (a, b), _ = table(idt, 2, False)
    e = _u32(expected_mixed([a, b], idt, FP32, 0))
    S = SPECIALS[idt]
    pinf, ninf = int(np.flatnonzero(S == (0x7F80 if idt == BF16 else 0x7C00))[0]), \
        int(np.flatnonzero(S == (0xFF80 if idt == BF16 else 0xFC00))[0])
    assert e[pinf * 16 + ninf] == 0xFFC00000 and e[ninf * 16 + pinf] == 0xFFC00000  # inf - inf
    nan = [i for i in range(16) if (int(S[i]) & 0x7FFF) > (0x7F80 if idt == BF16 else 0x7C00)]
    assert len(nan) == 6
    wide = _u32(expected_mixed([S], idt, FP32, 0))  # k = 1: the conversion
    for i in nan:
        for j in nan:  # of two NaNs the earlier operand's, quieted
            assert e[i * 16 + j] == wide[i] | 0x00400000
        assert (e[i * 16:(i + 1) * 16] & 0x00400000).all() and (e[i::16] & 0x00400000).all()  # never signalling
    quiet_at_k1 = [(int(wide[i]) & 0x00400000) != 0 for i in nan]
    assert all(quiet_at_k1) if idt == FP16 else not all(quiet_at_k1)
    # with an accumulator, its NaN wins over an input's
    (b1,), acc = table(idt, 1, True)
    ea = _u32(expected_mixed([b1], idt, FP32, 0, acc))
    acc_nan = np.flatnonzero(np.isnan(acc) & np.isnan(wide.view(np.float32)[np.arange(256) % 16]))
    assert acc_nan.size == 36 and (ea[acc_nan] == (_u32(acc)[acc_nan] | 0x00400000)).all()


def test_table_expectation_narrowing():
    (a, b), _ = table(FP32, 2, False)
    S = SPECIALS[FP32]
    imax, izero, iden = (int(np.flatnonzero(S == v)[0]) for v in (0x7F7FFFFF, 0x00000000, 0x00000001))
    h = expected_mixed([a, b], FP32, FP16, 0)
    assert h[imax * 16 + izero] == 0x7C00  # fp32 max -> fp16 overflows to +inf
    r = expected_mixed([a, b], FP32, BF16, F_RNE)
    t = expected_mixed([a, b], FP32, BF16, 0)
    assert r[iden * 16 + izero] == 0x0000 and t[iden * 16 + izero] == 0x0000
    ineg = int(np.flatnonzero(S == 0x80000000)[0])
    nden = np.array([0x80000001], np.uint32).view(np.float32)
    assert expected_mixed([nden], FP32, BF16, F_RNE)[0] == 0x8000  # signed zero
    assert r[ineg * 16 + ineg] == 0x8000
