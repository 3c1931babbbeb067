"""What the tests of mi_reduce_bcast_mixed_scaled share: the expectation, built
on the CPU from three helpers the suite already trusts (the unscaled mixed
composition, mi_reduce_bcast_scaled's expectation, the oracle's fp32 fold), and
the call itself.  The routes are tests.mixed.knobs."""
from __future__ import annotations

from tests.guard import oracle_fold
from tests.mixed import SUM, expected_mixed
from tests.test_gpu_scaled import expected_scaled
from tests.util import FP32, convert_expected


def expected_mixed_scaled(ins, idt, odt, flags, scale, acc=None):
    """The compositions the header defines, on numpy arrays.  The product is
    an fp32 array before anything is added to it or rounded from it: rounded
    once as fp32, never fused with the add."""
    if odt == FP32:
        S = expected_mixed(ins, idt, odt, flags)            # the wire inputs alone
        P = expected_scaled([S], FP32, 0, scale)            # mi_reduce_bcast_scaled, k = 1
        if acc is None:
            return P
        return oracle_fold([acc, P], FP32, SUM, 0)          # acc the accumulator, P in the `in` role
    assert acc is None
    P = expected_scaled(list(ins), FP32, 0, scale)          # the fp32 fold, scaled
    return convert_expected(P, FP32, odt, flags)


def call_mixed_scaled(pin, idt, pout, odt, n, flags, scale, acc=None, stream=None):
    from oneccl_amd import _lib
    _lib.check(_lib.mi().mi_reduce_bcast_mixed_scaled(_lib.void_ptr_array(pin), len(pin), idt, acc,
                                                      _lib.void_ptr_array(pout), len(pout), odt, n, SUM, flags,
                                                      scale, stream), "mi_reduce_bcast_mixed_scaled")
