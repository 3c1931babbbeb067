"""What the tests of mi_reduce_bcast_mixed share: the expectation, built on the
CPU from pieces the suite already trusts (the oracle's fp32 fold with the x86
NaN rule, the oracle's array conversions), the call itself and the three
kernel routes."""
from __future__ import annotations

import contextlib
import ctypes

from tests.guard import oracle_fold
from tests.util import BF16, FP16, FP32, convert_expected

SUM = 0
F_RNE, F_TAIL = 0x2, 0x8

# (in_dtype, out_dtype, flags): the two widenings; each narrowing variant
WIDENING = [(BF16, FP32, 0), (FP16, FP32, 0)]
NARROWING = [(FP32, BF16, 0), (FP32, BF16, F_RNE), (FP32, BF16, F_RNE | F_TAIL), (FP32, FP16, 0)]
PAIRS = WIDENING + NARROWING
PAIR_IDS = ["bf16-fp32", "fp16-fp32", "fp32-bf16-trunc", "fp32-bf16-rne", "fp32-bf16-rne-tail16", "fp32-fp16"]

# T: groups of 8 elements per tile of the kernel as built.  A one-wave block
# owns 64 * 2 runs of 4 elements (mixed_kernel, reduce_kernels.hpp; kMixedRuns
# = 2 in mi_reduce.hip), 512 elements.
T_GROUPS = 64


def expected_mixed(ins, idt, odt, flags, acc=None):
    """The composition the header defines, on numpy arrays."""
    if odt == FP32:
        cs = [convert_expected(x, idt, FP32, 0) for x in ins]
        return oracle_fold(([acc] if acc is not None else []) + cs, FP32, SUM, 0)
    assert acc is None
    return convert_expected(oracle_fold(list(ins), FP32, SUM, 0), FP32, odt, flags)


def call_mixed(pin, idt, pout, odt, n, flags, acc=None, stream=None):
    from oneccl_amd import _lib
    _lib.check(_lib.mi().mi_reduce_bcast_mixed(_lib.void_ptr_array(pin), len(pin), idt, acc, _lib.void_ptr_array(pout),
                                               len(pout), odt, n, SUM, flags, stream), "mi_reduce_bcast_mixed")


@contextlib.contextmanager
def knobs(max_blocks=0, unaligned=1):
    """Route a launch: max_blocks > 0 the grid-stride form, unaligned = 0 the
    element loop for inputs off the outputs' grid."""
    from oneccl_amd import _lib
    m = _lib.mi()
    mb = ctypes.c_int()
    assert m.mi_get_launch_config(None, None, ctypes.byref(mb)) == 0
    prev_u = m.mi_set_unaligned_vectors(unaligned)
    assert m.mi_set_max_blocks(max_blocks) == 0
    try:
        yield
    finally:
        assert m.mi_set_max_blocks(mb.value) == 0
        m.mi_set_unaligned_vectors(prev_u)
