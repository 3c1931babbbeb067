"""mi_reduce_bcast's host-side refusals.  Every argument check runs before the
first HIP call, so none of this needs a device: a refused call returns
MI_E_INVALID with a message naming the operands, and a call that passes the
checks on pageable host buffers goes on to the device-visibility check and is
refused there (as mi_reduce_multi refuses a pageable operand on a stream)."""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd import _lib

FP32, SUM, E_INVALID = 9, 0, -1
N = 64


def _bufs(count, n=N):
    """`count` separate pageable fp32 buffers of n elements (kept alive by the caller)."""
    return [np.full(n, float(i + 1), np.float32) for i in range(count)]


def _call(ins, outs, count=N, dt=FP32, op=SUM, k=None, m=None):
    mi = _lib.mi()
    rc = mi.mi_reduce_bcast(_lib.void_ptr_array(ins), len(ins) if k is None else k, _lib.void_ptr_array(outs),
                            len(outs) if m is None else m, count, dt, op, 0, None)
    return rc, mi.mi_last_error().decode() if rc else ""


def _ptrs(arrays):
    return [a.ctypes.data for a in arrays]


def test_binding_and_version():
    assert _lib.mi().mi_version() == 101
    assert any(name == "mi_reduce_bcast" for name, _, _ in _lib.MI_API)


@pytest.mark.parametrize("m", [0, 17])
def test_output_count_out_of_range(m):
    ins, outs = _bufs(2), _bufs(17)
    rc, msg = _call(_ptrs(ins), _ptrs(outs), m=m)
    assert rc == E_INVALID and "output count m" in msg and "[1,16]" in msg


@pytest.mark.parametrize("k", [0, 17])
def test_input_count_out_of_range(k):
    ins, outs = _bufs(17), _bufs(2)
    rc, msg = _call(_ptrs(ins), _ptrs(outs), k=k)
    assert rc == E_INVALID and "input count k" in msg and "[1,16]" in msg


def test_null_entries():
    ins, outs = _bufs(3), _bufs(3)
    po = _ptrs(outs)
    po[1] = None
    rc, msg = _call(_ptrs(ins), po)
    assert rc == E_INVALID and "outs[1] is NULL" in msg
    pi = _ptrs(ins)
    pi[2] = None
    rc, msg = _call(pi, _ptrs(outs))
    assert rc == E_INVALID and "inputs[2] is NULL" in msg
    # a NULL entry is refused for an empty call too; NULL lists as well
    rc, msg = _call(_ptrs(ins), po, count=0)
    assert rc == E_INVALID and "outs[1] is NULL" in msg
    mi = _lib.mi()
    assert mi.mi_reduce_bcast(None, 2, _lib.void_ptr_array(_ptrs(outs)), 3, N, FP32, SUM, 0, None) == E_INVALID
    assert b"input list" in mi.mi_last_error()
    assert mi.mi_reduce_bcast(_lib.void_ptr_array(_ptrs(ins)), 3, None, 2, N, FP32, SUM, 0, None) == E_INVALID
    assert b"output list" in mi.mi_last_error()


def test_two_equal_outputs():
    ins, outs = _bufs(2), _bufs(3)
    po = _ptrs(outs)
    po[2] = po[0]
    rc, msg = _call(_ptrs(ins), po)
    assert rc == E_INVALID and "outs[0] and outs[2] overlap" in msg


def test_outputs_overlapping_by_one_element():
    ins = _bufs(2)
    bucket = np.zeros(2 * N - 1, np.float32)
    base = bucket.ctypes.data
    other = _bufs(1)
    po = [other[0].ctypes.data, base, base + (N - 1) * 4]  # the last element of outs[1] is the first of outs[2]
    rc, msg = _call(_ptrs(ins), po)
    assert rc == E_INVALID and "outs[1] and outs[2] overlap" in msg
    # touching ranges do not overlap: on to the device-visibility check
    bucket2 = np.zeros(2 * N, np.float32)
    rc, msg = _call(_ptrs(ins), [other[0].ctypes.data, bucket2.ctypes.data, bucket2.ctypes.data + N * 4])
    assert rc == E_INVALID and "pageable" in msg


def test_output_overlapping_an_input_by_one_element():
    bucket = np.zeros(2 * N - 1, np.float32)
    base = bucket.ctypes.data
    ins, outs = _bufs(2), _bufs(1)
    # inputs[1] ends where outs[1] starts, one element shared; and the other way round
    rc, msg = _call([ins[0].ctypes.data, base], [outs[0].ctypes.data, base + (N - 1) * 4])
    assert rc == E_INVALID and "outs[1] overlaps inputs[1] without being equal to it" in msg
    rc, msg = _call([base + (N - 1) * 4, ins[0].ctypes.data], [base, outs[0].ctypes.data])
    assert rc == E_INVALID and "outs[0] overlaps inputs[0] without being equal to it" in msg


def test_bad_dtype_and_custom_op():
    ins, outs = _bufs(2), _bufs(2)
    rc, msg = _call(_ptrs(ins), _ptrs(outs), dt=42)
    assert rc == E_INVALID and "datatype" in msg
    rc, msg = _call(_ptrs(ins), _ptrs(outs), op=4)  # MI_OP_CUSTOM
    assert rc == E_INVALID and "reduction" in msg
    # both refused ahead of everything else, fake addresses never looked at
    rc, msg = _call([16, 32], [48, 64], dt=-1)
    assert rc == E_INVALID and "datatype" in msg


def test_count_overflowing_the_address_space():
    rc, msg = _call([1 << 20, 2 << 20], [3 << 20, 4 << 20], count=(1 << 63))
    assert rc == E_INVALID and "overflows" in msg
    # the limit is the dtype's: 2^61 elements wrap at 8 bytes each (int64), one fewer end past the top
    rc, msg = _call([1 << 20, 2 << 20], [3 << 20, 4 << 20], count=1 << 61, dt=6)
    assert rc == E_INVALID and msg == "count overflows the address space"
    rc, msg = _call([1 << 20, 2 << 20], [3 << 20, 4 << 20], count=(1 << 61) - 1, dt=6)
    assert rc == E_INVALID and msg == "inputs[0] + count overflows the address space"
    rc, msg = _call([1 << 20, 2 << 20], [3 << 20, 4 << 20], count=1 << 61)  # fp32: 2^63 bytes fit
    assert rc == E_INVALID and msg == "outs[0] overlaps inputs[0] without being equal to it"


def test_empty_call_with_valid_arguments_returns_zero():
    ins, outs = _bufs(3), _bufs(2)
    rc, _ = _call(_ptrs(ins), _ptrs(outs), count=0)
    assert rc == 0
    # fake non-null addresses: an empty call touches nothing, overlapping or not
    rc, _ = _call([0x1000, 0x1000], [0x1000, 0x1000], count=0)
    assert rc == 0


def test_exact_alias_passes_validation():
    """outs[0] == inputs[2] (and the in-place allreduce, outs[i] == inputs[i])
    get past every argument check: what refuses them here is only that the
    buffers are pageable host memory."""
    ins, outs = _bufs(3), _bufs(1)
    rc, msg = _call(_ptrs(ins), [ins[2].ctypes.data, outs[0].ctypes.data])
    assert rc == E_INVALID and "pageable" in msg and "overlap" not in msg
    rc, msg = _call(_ptrs(ins), _ptrs(ins))
    assert rc == E_INVALID and "pageable" in msg and "overlap" not in msg
    for a, i in zip(ins, range(3)):
        assert (a == float(i + 1)).all()  # nothing ran


def test_one_output_is_reduce_multi():
    """m = 1 routes to mi_reduce_multi's path: the same refusal text."""
    ins, outs = _bufs(3), _bufs(1)
    rc, msg = _call(_ptrs(ins), _ptrs(outs))
    mi = _lib.mi()
    rc2 = mi.mi_reduce_multi(_lib.void_ptr_array(_ptrs(ins)), 3, outs[0].ctypes.data, N, FP32, SUM, 0, None)
    assert rc == rc2 == E_INVALID and msg == mi.mi_last_error().decode()


def test_python_wrapper_is_exported():
    import oneccl_amd
    from oneccl_amd import comp
    assert oneccl_amd.reduce_bcast is comp.reduce_bcast
