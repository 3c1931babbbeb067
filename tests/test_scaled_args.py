"""mi_reduce_bcast_scaled's host-side refusals.  As for mi_reduce_bcast
(tests/test_bcast_args.py) every argument check runs before the first HIP
call, so none of this needs a device: the operands are pageable numpy
buffers, a refused call returns its code with a message naming the argument,
and no byte of any buffer is written.  A call that passes every check is
refused only for its pageable operands."""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd import _lib

FP16, FP32, FP64, BF16 = 8, 9, 10, 11
SUM, PROD, MIN, MAX, CUSTOM = 0, 1, 2, 3, 4
E_INVALID, E_UNSUPPORTED = -1, -2
N = 64


class Bufs:
    """`k` inputs and `m` outputs, separate pageable buffers of 8 bytes per
    element (room for any dtype) with a snapshot to compare against."""

    def __init__(self, k, m, n=N):
        self.ins = [np.full(n, 1000 + i, np.int64) for i in range(k)]
        self.outs = [np.full(n, 2000 + i, np.int64) for i in range(m)]
        self.snap = [a.copy() for a in self.ins + self.outs]

    def untouched(self):
        return all(np.array_equal(a, s) for a, s in zip(self.ins + self.outs, self.snap))


def _ptrs(arrays):
    return [a.ctypes.data for a in arrays]


def _call(ins, outs, scale=0.5, count=N, dt=FP32, op=SUM, flags=0, k=None, m=None):
    mi = _lib.mi()
    rc = mi.mi_reduce_bcast_scaled(_lib.void_ptr_array(ins), len(ins) if k is None else k, _lib.void_ptr_array(outs),
                                   len(outs) if m is None else m, count, dt, op, flags, scale, None)
    return rc, mi.mi_last_error().decode() if rc else ""


def test_binding():
    entry = [(res, args) for name, res, args in _lib.MI_API if name == "mi_reduce_bcast_scaled"]
    assert len(entry) == 1
    import ctypes
    assert entry[0][1][-2] is ctypes.c_double  # the scale, before the stream
    assert _lib.mi().mi_version() == 101


def test_python_wrapper_is_exported():
    import oneccl_amd
    from oneccl_amd import comp
    assert oneccl_amd.reduce_bcast_scaled is comp.reduce_bcast_scaled


# ---- what only the scaled entry refuses ------------------------------------------------

@pytest.mark.parametrize("op", [PROD, MIN, MAX])
def test_other_ops_are_unsupported(op):
    b = Bufs(2, 2)
    rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), op=op)
    assert rc == E_UNSUPPORTED and msg.startswith("op") and "sum" in msg
    assert b.untouched()


@pytest.mark.parametrize("dt", range(8), ids=["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_integer_dtypes_are_unsupported(dt):
    b = Bufs(2, 2)
    rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), dt=dt)
    assert rc == E_UNSUPPORTED and msg.startswith("dtype")
    assert b.untouched()


@pytest.mark.parametrize("dt", [FP16, FP32, FP64, BF16])
@pytest.mark.parametrize("scale", [float("nan"), float("inf"), float("-inf")])
def test_scale_not_finite(scale, dt):
    b = Bufs(3, 2)
    rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=scale, dt=dt)
    assert rc == E_INVALID and msg.startswith("scale") and "NaN or infinite" in msg
    assert b.untouched()


@pytest.mark.parametrize("dt", [FP16, FP32, FP64, BF16])
@pytest.mark.parametrize("scale", [0.0, -0.0])
def test_scale_zero(scale, dt):
    b = Bufs(3, 2)
    rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=scale, dt=dt)
    assert rc == E_INVALID and msg.startswith("scale") and "zero" in msg
    assert b.untouched()


@pytest.mark.parametrize("dt", [FP32, BF16, FP16])
def test_scale_underflowing_or_overflowing_float(dt):
    """The compute type of fp32, bf16 and fp16 is float: 1e-60 converts to
    zero and 1e300 to infinity, and both are refused; for fp64 they are
    ordinary multipliers (refused below only for the pageable operands)."""
    b = Bufs(2, 3)
    rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=1e-60, dt=dt)
    assert rc == E_INVALID and msg.startswith("scale") and "zero as a float" in msg
    for big in (1e300, -1e300):
        rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=big, dt=dt)
        assert rc == E_INVALID and msg.startswith("scale") and "infinite as a float" in msg
    # the smallest float denormal and the largest float are multipliers like any other
    for ok in (1.5e-45, 3.4e38):
        rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=ok, dt=dt)
        assert rc == E_INVALID and "pageable" in msg
    for ok in (1e-60, 1e300):
        rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=ok, dt=FP64)
        assert rc == E_INVALID and "pageable" in msg
    assert b.untouched()


def test_scale_is_checked_for_an_empty_call_too():
    b = Bufs(2, 2)
    rc, msg = _call(_ptrs(b.ins), _ptrs(b.outs), scale=0.0, count=0)
    assert rc == E_INVALID and "zero" in msg
    rc, _ = _call(_ptrs(b.ins), _ptrs(b.outs), count=0)
    assert rc == 0
    # fake non-null addresses: an empty call touches nothing, overlapping or not
    rc, _ = _call([0x1000, 0x1000], [0x1000, 0x1000], count=0)
    assert rc == 0


# ---- mi_reduce_bcast's refusals, through the new entry ------------------------------------

def _both(ins, outs, **kw):
    """The scaled call's (rc, message); the unscaled call on the same
    arguments must refuse with the same code and text."""
    mi = _lib.mi()
    rc, msg = _call(ins, outs, **kw)
    kw.pop("scale", None)
    k, m = kw.get("k"), kw.get("m")
    rc2 = mi.mi_reduce_bcast(_lib.void_ptr_array(ins), len(ins) if k is None else k, _lib.void_ptr_array(outs),
                             len(outs) if m is None else m, kw.get("count", N), kw.get("dt", FP32), kw.get("op", SUM),
                             0, None)
    assert rc == rc2 and msg == mi.mi_last_error().decode()
    return rc, msg


@pytest.mark.parametrize("k,m", [(0, 2), (17, 2), (2, 0), (2, 17)])
def test_counts_out_of_range(k, m):
    b = Bufs(17, 17)
    rc, msg = _both(_ptrs(b.ins), _ptrs(b.outs), k=k, m=m)
    assert rc == E_INVALID and "[1,16]" in msg and ("input count k" if k in (0, 17) else "output count m") in msg
    assert b.untouched()


def test_null_entries_and_lists():
    b = Bufs(3, 3)
    po = _ptrs(b.outs)
    po[1] = None
    rc, msg = _both(_ptrs(b.ins), po)
    assert rc == E_INVALID and "outs[1] is NULL" in msg
    pi = _ptrs(b.ins)
    pi[2] = None
    rc, msg = _both(pi, _ptrs(b.outs))
    assert rc == E_INVALID and "inputs[2] is NULL" in msg
    rc, msg = _both(_ptrs(b.ins), po, count=0)
    assert rc == E_INVALID and "outs[1] is NULL" in msg
    mi = _lib.mi()
    assert mi.mi_reduce_bcast_scaled(None, 2, _lib.void_ptr_array(_ptrs(b.outs)), 3, N, FP32, SUM, 0, 0.5,
                                     None) == E_INVALID
    assert b"input list" in mi.mi_last_error()
    assert mi.mi_reduce_bcast_scaled(_lib.void_ptr_array(_ptrs(b.ins)), 3, None, 2, N, FP32, SUM, 0, 0.5,
                                     None) == E_INVALID
    assert b"output list" in mi.mi_last_error()
    assert b.untouched()


def test_overlapping_outputs():
    b = Bufs(2, 3)
    po = _ptrs(b.outs)
    po[2] = po[0]
    rc, msg = _both(_ptrs(b.ins), po)
    assert rc == E_INVALID and "outs[0] and outs[2] overlap" in msg
    bucket = np.zeros(2 * N - 1, np.float32)
    base = bucket.ctypes.data
    rc, msg = _both(_ptrs(b.ins), [b.outs[0].ctypes.data, base, base + (N - 1) * 4])  # one element shared
    assert rc == E_INVALID and "outs[1] and outs[2] overlap" in msg
    assert b.untouched() and not bucket.any()


def test_output_overlapping_an_input_by_one_element():
    bucket = np.zeros(2 * N - 1, np.float32)
    base = bucket.ctypes.data
    b = Bufs(2, 1)
    rc, msg = _both([b.ins[0].ctypes.data, base], [b.outs[0].ctypes.data, base + (N - 1) * 4])
    assert rc == E_INVALID and "outs[1] overlaps inputs[1] without being equal to it" in msg
    rc, msg = _both([base + (N - 1) * 4, b.ins[0].ctypes.data], [base, b.outs[0].ctypes.data])
    assert rc == E_INVALID and "outs[0] overlaps inputs[0] without being equal to it" in msg
    assert b.untouched() and not bucket.any()


def test_bad_dtype_custom_op_and_count():
    b = Bufs(2, 2)
    rc, msg = _both(_ptrs(b.ins), _ptrs(b.outs), dt=42)
    assert rc == E_INVALID and "datatype" in msg
    rc, msg = _both(_ptrs(b.ins), _ptrs(b.outs), op=CUSTOM)
    assert rc == E_INVALID and "reduction" in msg
    rc, msg = _both([1 << 20, 2 << 20], [3 << 20, 4 << 20], count=(1 << 63))
    assert rc == E_INVALID and "overflows" in msg
    assert b.untouched()


def test_exact_alias_passes_validation():
    """outs[0] == inputs[2], and the in-place averaged allreduce
    (outs[i] == inputs[i]), get past every argument check in every supported
    dtype: what refuses them here is only that the buffers are pageable."""
    for dt in (FP16, FP32, FP64, BF16):
        b = Bufs(3, 1)
        rc, msg = _call(_ptrs(b.ins), [b.ins[2].ctypes.data, b.outs[0].ctypes.data], scale=1 / 3, dt=dt)
        assert rc == E_INVALID and "pageable" in msg and "overlap" not in msg
        rc, msg = _call(_ptrs(b.ins), _ptrs(b.ins), scale=1 / 3, dt=dt)
        assert rc == E_INVALID and "pageable" in msg and "overlap" not in msg
        # one output, one input: still the scaled entry's own path
        rc, msg = _call(_ptrs(b.ins)[:1], _ptrs(b.outs), scale=1 / 3, dt=dt)
        assert rc == E_INVALID and "pageable" in msg
        assert b.untouched()  # nothing ran
