"""mi_reduce_bcast_mixed's host-side refusals.  Every argument check runs
before the first HIP call, so none of this needs a device: the calls are driven
with fake non-NULL addresses (never dereferenced: a call that passed every
check would go on to the device-visibility check, which refuses pageable or
unknown memory), and each refusal returns its code with a message naming the
operand or argument."""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd import _lib

FP16, FP32, FP64, BF16 = 8, 9, 10, 11
SUM, E_INVALID, E_UNSUPPORTED = 0, -1, -2
N = 64
PAIRS = [(BF16, FP32), (FP16, FP32), (FP32, BF16), (FP32, FP16)]


def _call(ins, outs, idt=BF16, odt=FP32, acc=None, count=N, op=SUM, k=None, m=None, flags=0):
    mi = _lib.mi()
    rc = mi.mi_reduce_bcast_mixed(None if ins is None else _lib.void_ptr_array(ins), len(ins) if k is None else k, idt,
                                  acc, None if outs is None else _lib.void_ptr_array(outs),
                                  len(outs) if m is None else m, odt, count, op, flags, None)
    return rc, mi.mi_last_error().decode() if rc else ""


def _addrs(n, base=0x10000000, step=0x100000):
    """n fake, well separated, 256-byte aligned addresses."""
    return [base + i * step for i in range(n)]


def test_binding_and_version():
    assert _lib.mi().mi_version() == 101
    entry = [e for e in _lib.MI_API if e[0] == "mi_reduce_bcast_mixed"]
    assert len(entry) == 1 and len(entry[0][2]) == 11


def test_error_codes_match_the_header():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "mi_reduce.h").read_text()
    assert int(re.search(r"#define MI_E_INVALID \((-?\d+)\)", text).group(1)) == E_INVALID
    assert int(re.search(r"#define MI_E_UNSUPPORTED \((-?\d+)\)", text).group(1)) == E_UNSUPPORTED


@pytest.mark.parametrize("idt,odt", [(FP32, FP32), (BF16, BF16), (FP16, FP16), (BF16, FP16), (FP16, BF16), (FP64, FP32),
                                     (FP32, FP64), (4, FP32), (FP32, 4), (42, FP32), (FP32, -1)])
def test_dtype_pair_outside_the_four(idt, odt):
    rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), idt=idt, odt=odt)
    assert rc == E_UNSUPPORTED and "in_dtype" in msg and "out_dtype" in msg
    # ahead of everything else: NULL lists are never looked at
    rc, msg = _call(None, None, idt=idt, odt=odt, k=2, m=2)
    assert rc == E_UNSUPPORTED and "in_dtype" in msg


@pytest.mark.parametrize("idt,odt", PAIRS)
@pytest.mark.parametrize("op", [1, 2, 3, 4, -1])
def test_op_other_than_sum(idt, odt, op):
    rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), idt=idt, odt=odt, op=op)
    assert rc == E_UNSUPPORTED and msg.startswith("op")


@pytest.mark.parametrize("odt", [BF16, FP16])
def test_acc_refused_when_narrowing(odt):
    rc, msg = _call(_addrs(2), _addrs(1, 0x30000000), idt=FP32, odt=odt, acc=0x50000000)
    assert rc == E_UNSUPPORTED and msg.startswith("acc")


@pytest.mark.parametrize("m", [0, 17, -1])
def test_output_count_out_of_range(m):
    rc, msg = _call(_addrs(2), _addrs(17, 0x30000000), m=m)
    assert rc == E_INVALID and "output count m" in msg and "[1,16]" in msg


@pytest.mark.parametrize("k", [0, 17, -1])
def test_input_count_out_of_range(k):
    rc, msg = _call(_addrs(17), _addrs(2, 0x30000000), k=k)
    assert rc == E_INVALID and "input count k" in msg and "[1,16]" in msg


def test_acc_counts_against_max_inputs():
    rc, msg = _call(_addrs(16), _addrs(1, 0x30000000), acc=0x50000000)
    assert rc == E_INVALID and "input count k" in msg and "[1,15]" in msg and "acc" in msg
    # 15 inputs and an accumulator pass the count check: on to the visibility check
    rc, msg = _call(_addrs(15), _addrs(1, 0x30000000), acc=0x50000000)
    assert rc == E_INVALID and "pageable" in msg
    rc, msg = _call(_addrs(16), _addrs(1, 0x30000000))
    assert rc == E_INVALID and "pageable" in msg


@pytest.mark.parametrize("idt,odt", PAIRS)
def test_null_lists_and_entries(idt, odt):
    ins, outs = _addrs(3), _addrs(3, 0x30000000)
    rc, msg = _call(None, outs, idt=idt, odt=odt, k=3)
    assert rc == E_INVALID and "input list" in msg
    rc, msg = _call(ins, None, idt=idt, odt=odt, m=3)
    assert rc == E_INVALID and "output list" in msg
    rc, msg = _call(ins, [outs[0], None, outs[2]], idt=idt, odt=odt)
    assert rc == E_INVALID and "outs[1] is NULL" in msg
    rc, msg = _call([ins[0], ins[1], None], outs, idt=idt, odt=odt)
    assert rc == E_INVALID and "inputs[2] is NULL" in msg
    # a NULL entry is refused for an empty call too
    rc, msg = _call(ins, [outs[0], None, outs[2]], idt=idt, odt=odt, count=0)
    assert rc == E_INVALID and "outs[1] is NULL" in msg


def test_address_overflow():
    rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), count=1 << 63)
    assert rc == E_INVALID and "overflows" in msg
    # the limit is the wider side's, whichever side that is: 2^62 elements wrap as fp32 only
    for idt, odt in ((BF16, FP32), (FP32, BF16)):
        rc, msg = _call(_addrs(1), _addrs(1, 0x30000000), idt=idt, odt=odt, count=1 << 62)
        assert rc == E_INVALID and msg == "count overflows the address space"
        rc, msg = _call(_addrs(1), _addrs(1, 0x30000000), idt=idt, odt=odt, count=(1 << 62) - 1)
        assert rc == E_INVALID and msg == ("outs" if odt == FP32 else "inputs") + "[0] + count overflows the address space"
    top = (1 << 64) - 0x1000
    rc, msg = _call([0x10000000, top], _addrs(1, 0x30000000), count=0x1000)  # 2-byte inputs: 0x2000 bytes
    assert rc == E_INVALID and "inputs[1] + count overflows" in msg
    rc, msg = _call(_addrs(1), [0x30000000, top], count=0x1000)
    assert rc == E_INVALID and "outs[1] + count overflows" in msg
    rc, msg = _call(_addrs(1), _addrs(1, 0x30000000), acc=top, count=0x1000)
    assert rc == E_INVALID and "acc + count overflows" in msg
    # each side's own element size: 0x800 two-byte inputs end exactly at the top, fp32 outputs would not
    rc, msg = _call([top], _addrs(1, 0x30000000), count=0x7FF)
    assert rc == E_INVALID and "pageable" in msg
    rc, msg = _call([0x10000000], [top], idt=FP32, odt=BF16, count=0x7FF)
    assert rc == E_INVALID and "pageable" in msg
    rc, msg = _call([top], [0x30000000], idt=FP32, odt=BF16, count=0x7FF)
    assert rc == E_INVALID and "inputs[0] + count overflows" in msg


@pytest.mark.parametrize("idt,odt,eso", [(BF16, FP32, 4), (FP32, FP16, 2)])
def test_two_outputs_overlapping(idt, odt, eso):
    ins = _addrs(2)
    base = 0x30000000
    rc, msg = _call(ins, [base, 0x40000000, base], idt=idt, odt=odt)
    assert rc == E_INVALID and "outs[0] and outs[2] overlap" in msg
    rc, msg = _call(ins, [0x40000000, base, base + (N - 1) * eso], idt=idt, odt=odt)  # one element shared
    assert rc == E_INVALID and "outs[1] and outs[2] overlap" in msg
    rc, msg = _call(ins, [0x40000000, base, base + N * eso], idt=idt, odt=odt)  # touching: passes the checks
    assert rc == E_INVALID and "pageable" in msg


@pytest.mark.parametrize("idt,odt,esi,eso", [(BF16, FP32, 2, 4), (FP16, FP32, 2, 4), (FP32, BF16, 4, 2),
                                             (FP32, FP16, 4, 2)])
def test_output_overlapping_an_input_at_all(idt, odt, esi, eso):
    base = 0x30000000
    # equal addresses are no exception: there is no in-place form across element sizes
    rc, msg = _call([0x10000000, base], [0x40000000, base], idt=idt, odt=odt)
    assert rc == E_INVALID and "outs[1] overlaps inputs[1]" in msg
    # the input's last element is the output's first byte range, and the other way round,
    # each range with its own element size
    rc, msg = _call([base], [base + (N - 1) * esi], idt=idt, odt=odt)
    assert rc == E_INVALID and "outs[0] overlaps inputs[0]" in msg
    rc, msg = _call([base + (N - 1) * eso], [base], idt=idt, odt=odt)
    assert rc == E_INVALID and "outs[0] overlaps inputs[0]" in msg
    # touching on either side passes the overlap checks
    rc, msg = _call([base], [base + N * esi], idt=idt, odt=odt)
    assert rc == E_INVALID and "pageable" in msg
    rc, msg = _call([base + N * eso], [base], idt=idt, odt=odt)
    assert rc == E_INVALID and "pageable" in msg


def test_output_overlapping_acc_without_being_equal():
    base = 0x30000000
    rc, msg = _call(_addrs(2), [0x40000000, base + 4], acc=base)
    assert rc == E_INVALID and "outs[1] overlaps acc without being equal to it" in msg
    rc, msg = _call(_addrs(2), [base], acc=base + (N - 1) * 4)
    assert rc == E_INVALID and "outs[0] overlaps acc without being equal to it" in msg
    # acc exactly one output (main_grad += ...) passes every argument check
    rc, msg = _call(_addrs(2), [0x40000000, base], acc=base)
    assert rc == E_INVALID and "pageable" in msg and "overlap" not in msg
    # but not two of them: those two outputs overlap each other
    rc, msg = _call(_addrs(2), [base, base], acc=base)
    assert rc == E_INVALID and "outs[0] and outs[1] overlap" in msg


@pytest.mark.parametrize("idt,odt", PAIRS)
def test_empty_call_returns_zero(idt, odt):
    rc, _ = _call(_addrs(3), _addrs(2, 0x30000000), idt=idt, odt=odt, count=0)
    assert rc == 0
    # an empty call touches nothing, overlapping or not
    rc, _ = _call([0x1000, 0x1000], [0x1000, 0x1000], idt=idt, odt=odt, count=0)
    assert rc == 0
    if odt == FP32:
        rc, _ = _call([0x1000], [0x1000], idt=idt, odt=odt, acc=0x1000, count=0)
        assert rc == 0
    # the refusals still come first
    rc, msg = _call(_addrs(3), _addrs(2, 0x30000000), idt=idt, odt=odt, count=0, op=1)
    assert rc == E_UNSUPPORTED and msg.startswith("op")


def test_pageable_operands_are_refused_and_untouched():
    ins = [np.full(N, 0x3F80, np.uint16) for _ in range(2)]
    acc = np.full(N, 2.0, np.float32)
    out = np.full(N, 7.0, np.float32)
    rc, msg = _call([a.ctypes.data for a in ins], [out.ctypes.data], acc=acc.ctypes.data)
    assert rc == E_INVALID and "pageable" in msg
    assert (out == 7.0).all() and (acc == 2.0).all() and all((a == 0x3F80).all() for a in ins)


# ---- the Python wrapper's own checks (CPU tensors: each raises before any pointer is taken) ----

def test_python_wrapper_is_exported():
    import oneccl_amd
    from oneccl_amd import comp
    assert oneccl_amd.reduce_bcast_mixed is comp.reduce_bcast_mixed


def test_python_wrapper_checks():
    import torch
    import oneccl_amd as oa
    b = [torch.zeros(N, dtype=torch.bfloat16) for _ in range(2)]
    f = [torch.zeros(N, dtype=torch.float32) for _ in range(2)]
    h = torch.zeros(N, dtype=torch.float16)
    with pytest.raises(ValueError, match="at least one"):
        oa.reduce_bcast_mixed([], f)
    with pytest.raises(TypeError, match="all inputs must have one dtype"):
        oa.reduce_bcast_mixed([b[0], h], f)
    with pytest.raises(TypeError, match="all outputs must have one dtype"):
        oa.reduce_bcast_mixed(b, [f[0], h])
    with pytest.raises(TypeError, match="unsupported dtype pair"):
        oa.reduce_bcast_mixed(f, [torch.zeros(N, dtype=torch.float32)])
    with pytest.raises(TypeError, match="unsupported dtype pair"):
        oa.reduce_bcast_mixed(b, [h])
    with pytest.raises(TypeError, match="acc goes with fp32 outputs"):
        oa.reduce_bcast_mixed(f, [h], acc=torch.zeros(N, dtype=torch.float32))
    with pytest.raises(TypeError, match="acc must be float32"):
        oa.reduce_bcast_mixed(b, f, acc=torch.zeros(N, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="same numel"):
        oa.reduce_bcast_mixed(b, [f[0], torch.zeros(N + 1, dtype=torch.float32)])
    with pytest.raises(ValueError, match="same numel"):
        oa.reduce_bcast_mixed(b, f, acc=torch.zeros(N - 1, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        oa.reduce_bcast_mixed(b, [f[0], torch.zeros(2 * N, dtype=torch.float32)[::2]])
    with pytest.raises(ValueError, match="device tensors"):
        oa.reduce_bcast_mixed(b, f)
