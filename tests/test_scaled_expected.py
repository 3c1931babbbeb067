"""The CPU construction the GPU tests of mi_reduce_bcast_scaled compare
against (tests.test_gpu_scaled.expected_scaled), checked where it can be
without a device: at scale 1 it must give back the oracle's fold."""
from __future__ import annotations

import numpy as np
import pytest

from tests.guard import oracle_fold
from tests.test_gpu_scaled import F_ACC_FP32, N, SUM, VARIANT_IDS, VARIANTS, _inputs, expected_scaled
from tests.util import BF16, assert_same


@pytest.mark.parametrize("dt,flags", VARIANTS[:-1], ids=VARIANT_IDS[:-1])  # the oracle has no TAIL_TRUNC16 fold
def test_expected_at_scale_one_is_the_fold(dt, flags):
    """expected_scaled at scale 1 is oracle_fold (the input for k = 1 in
    storage precision), but for bf16 denormals through k = 1 under RNE
    without fp32 accumulation, which the narrowing flushes to signed zero."""
    assert N > 40  # rand_array's specials are present
    for k in (1, 2, 3, 8):
        ins = _inputs(dt, k, 500 + k)
        copied = k == 1 and not flags & F_ACC_FP32
        F = ins[0] if copied else oracle_fold(ins, dt, SUM, flags)
        got = expected_scaled(ins, dt, flags, 1.0)
        if dt == BF16 and copied and flags & 0x2:
            den = ((F & 0x7F80) == 0) & ((F & 0x007F) != 0)
            assert den.any() and (got[den] == (F[den] & 0x8000)).all()
            got[den] = F[den]
        assert_same(got, F, dt, f"k={k}")


def test_expected_keeps_the_unscaled_nan_bits():
    """Where the accumulator is a NaN the expected value is the fold's own
    element, whatever the scale; elsewhere a scale other than 1 changes it."""
    for (dt, flags) in VARIANTS[:-1]:
        ins = _inputs(dt, 3, 900)
        F = oracle_fold(ins, dt, SUM, flags)
        got = expected_scaled(ins, dt, flags, -2.5)
        iv = {2: np.uint16, 4: np.uint32, 8: np.uint64}[F.itemsize]
        same = got.view(iv) == F.view(iv)
        nan = (F.view(iv) & {2: 0x7FFF, 4: 0x7FFFFFFF, 8: 0x7FFFFFFFFFFFFFFF}[F.itemsize]) > \
            {2: 0x7F80 if dt == BF16 else 0x7C00, 4: 0x7F800000, 8: 0x7FF0000000000000}[F.itemsize]
        assert nan.any() and same[nan].all()
        assert (~same).sum() > F.size // 2
