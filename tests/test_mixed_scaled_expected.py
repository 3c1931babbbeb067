"""The CPU construction the GPU tests of mi_reduce_bcast_mixed_scaled compare
against (tests.mixed_scaled.expected_mixed_scaled), checked where it can be
without a device: what it reduces to at scale 1, and that on the GPU test's own
inputs and scale it tells the right code from the two wrong ones that are
easiest to write (a fused multiply-add under an accumulator; a sum rounded to
storage before it is scaled)."""
from __future__ import annotations

import numpy as np
import pytest

from tests.guard import _bits, oracle_fold
from tests.mixed import NARROWING, PAIR_IDS, SUM, WIDENING, expected_mixed
from tests.mixed_scaled import expected_mixed_scaled
from tests.util import BF16, FP16, FP32, assert_same, convert_expected, rand_array

N = 3 * 4096 + 5
K = 3
SCALE = 1 / 3  # the GPU test's: not a power of two


def _inputs(dt, k=K):
    """The GPU test's inputs (tests/test_gpu_mixed_scaled.py)."""
    return [rand_array(dt, N, seed=7100 + 31 * dt + j) for j in range(k)]


def _acc():
    return rand_array(FP32, N, seed=7999)


def _u32(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("idt,odt,flags", WIDENING, ids=PAIR_IDS[:2])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_scale_one_widening_is_the_unscaled_call(idt, odt, flags, k):
    ins = _inputs(idt, k)
    assert_same(expected_mixed_scaled(ins, idt, odt, flags, 1.0), expected_mixed(ins, idt, odt, flags), FP32)


@pytest.mark.parametrize("idt,odt,flags", NARROWING, ids=PAIR_IDS[2:])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_scale_one_narrowing_is_the_unscaled_call(idt, odt, flags, k):
    ins = _inputs(idt, k)
    assert_same(expected_mixed_scaled(ins, idt, odt, flags, 1.0), expected_mixed(ins, idt, odt, flags), odt)


@pytest.mark.parametrize("idt", [BF16, FP16], ids=["bf16", "fp16"])
def test_scale_one_with_acc_is_one_add_not_the_left_fold(idt):
    ins, acc = _inputs(idt), _acc()
    S = expected_mixed(ins, idt, FP32, 0)
    e = expected_mixed_scaled(ins, idt, FP32, 0, 1.0, acc)
    assert_same(e, oracle_fold([acc, S], FP32, SUM, 0), FP32)
    differ = int((_u32(e) != _u32(expected_mixed(ins, idt, FP32, 0, acc))).sum())
    print(f"{idt}: acc + sum differs from the left fold from acc in {differ} of {N} elements")
    assert differ >= 1


@pytest.mark.parametrize("idt", [BF16, FP16], ids=["bf16", "fp16"])
def test_a_fused_multiply_add_would_be_caught(idt):
    """float32(float64(S) * float64(s) + float64(acc)) is v_fmac_f32's result
    wherever the double sum is exact enough to round as the infinitely precise
    one does; that it differs from the expectation at all is what matters."""
    ins, acc = _inputs(idt), _acc()
    S = expected_mixed(ins, idt, FP32, 0)
    e = expected_mixed_scaled(ins, idt, FP32, 0, SCALE, acc)
    with np.errstate(all="ignore"):
        fused = (S.astype(np.float64) * np.float64(np.float32(SCALE)) + acc.astype(np.float64)).astype(np.float32)
        finite = np.isfinite(e) & np.isfinite(fused)
        differ = int((_u32(e)[finite] != _u32(fused)[finite]).sum())
        print(f"{idt}: fused differs in {differ} of {int(finite.sum())} finite elements at scale 1/3")
        assert differ >= 1
        # a power of two scales exactly: no second rounding to tell the two apart
        e8 = expected_mixed_scaled(ins, idt, FP32, 0, 1 / 8, acc)
        fused8 = (S.astype(np.float64) * 0.125 + acc.astype(np.float64)).astype(np.float32)
        finite8 = np.isfinite(e8) & np.isfinite(fused8) & (np.abs(S) > 1e-30)  # the product is no denormal
        assert (_u32(e8)[finite8] == _u32(fused8)[finite8]).all()


@pytest.mark.parametrize("idt,odt,flags", [p for p in NARROWING if not p[2] & 0x8],
                         ids=["bf16-trunc", "bf16-rne", "fp16"])
def test_rounding_the_sum_to_storage_first_would_be_caught(idt, odt, flags):
    from tests.test_gpu_scaled import expected_scaled
    ins = _inputs(idt)
    e = expected_mixed_scaled(ins, idt, odt, flags, SCALE)
    twice = expected_scaled([expected_mixed(ins, idt, odt, flags)], odt, flags, SCALE)
    differ = int((e != twice).sum())
    print(f"{odt} flags {flags:#x}: two roundings differ in {differ} of {N} elements")
    assert differ >= 1


@pytest.mark.parametrize("idt,odt,flags", WIDENING + NARROWING, ids=PAIR_IDS)
def test_nan_elements_are_the_unscaled_expectation(idt, odt, flags):
    ins = _inputs(idt)
    u, e = expected_mixed(ins, idt, odt, flags), expected_mixed_scaled(ins, idt, odt, flags, -2.5)
    wide = u if odt == FP32 else convert_expected(u, odt, FP32, 0)
    nan = np.isnan(wide)
    assert nan.any()
    assert (_bits(e)[nan] == _bits(u)[nan]).all()
    if odt == FP32:  # under an accumulator too: the add is the oracle's, NaN rule included
        acc = _acc()
        ua = oracle_fold([acc, u], FP32, SUM, 0)
        ea = expected_mixed_scaled(ins, idt, odt, flags, -2.5, acc)
        nan = np.isnan(u) | np.isnan(acc)
        assert (_u32(ea)[nan] == _u32(ua)[nan]).all()
