"""mi_reduce_bcast_mixed_scaled's host-side refusals: those of
mi_reduce_bcast_mixed, code for code and in the same order (the dtype pair
first), and the scale's, after the list checks and before the operands'.  As
tests/test_mixed_args.py, none of this needs a device: the calls are driven
with fake non-NULL addresses that are never dereferenced (a call that passed
every check goes on to the device-visibility check, which refuses pageable or
unknown memory)."""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd import _lib

FP16, FP32, FP64, BF16 = 8, 9, 10, 11
SUM, E_INVALID, E_UNSUPPORTED = 0, -1, -2
N = 64
PAIRS = [(BF16, FP32), (FP16, FP32), (FP32, BF16), (FP32, FP16)]
BAD_SCALES = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e-60, 1e300, -1e300]


def _call(ins, outs, idt=BF16, odt=FP32, acc=None, count=N, op=SUM, k=None, m=None, flags=0, scale=1 / 3):
    mi = _lib.mi()
    rc = mi.mi_reduce_bcast_mixed_scaled(None if ins is None else _lib.void_ptr_array(ins),
                                         len(ins) if k is None else k, idt, acc,
                                         None if outs is None else _lib.void_ptr_array(outs),
                                         len(outs) if m is None else m, odt, count, op, flags, scale, None)
    return rc, mi.mi_last_error().decode() if rc else ""


def _unscaled(ins, outs, idt=BF16, odt=FP32, acc=None, count=N, op=SUM, k=None, m=None, flags=0):
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
    entry = [e for e in _lib.MI_API if e[0] == "mi_reduce_bcast_mixed_scaled"]
    assert len(entry) == 1 and len(entry[0][2]) == 12


# Every refusal of the unscaled call: (keyword arguments, code).  Fake addresses as tests/test_mixed_args.py's.
_B, _T = 0x30000000, (1 << 64) - 0x1000
REFUSALS = [
    (dict(ins=_addrs(2), outs=_addrs(2, _B), idt=FP32, odt=FP32), E_UNSUPPORTED),
    (dict(ins=_addrs(2), outs=_addrs(2, _B), idt=BF16, odt=FP16), E_UNSUPPORTED),
    (dict(ins=_addrs(2), outs=_addrs(2, _B), idt=FP64, odt=FP32), E_UNSUPPORTED),
    (dict(ins=None, outs=None, idt=42, odt=FP32, k=2, m=2), E_UNSUPPORTED),
    (dict(ins=_addrs(2), outs=_addrs(2, _B), op=1), E_UNSUPPORTED),
    (dict(ins=_addrs(2), outs=_addrs(2, _B), idt=FP32, odt=FP16, op=3), E_UNSUPPORTED),
    (dict(ins=_addrs(2), outs=_addrs(1, _B), idt=FP32, odt=BF16, acc=0x50000000), E_UNSUPPORTED),
    (dict(ins=_addrs(2), outs=_addrs(17, _B), m=0), E_INVALID),
    (dict(ins=_addrs(2), outs=_addrs(17, _B), m=17), E_INVALID),
    (dict(ins=_addrs(17), outs=_addrs(2, _B), k=0), E_INVALID),
    (dict(ins=_addrs(17), outs=_addrs(2, _B), k=17), E_INVALID),
    (dict(ins=_addrs(16), outs=_addrs(1, _B), acc=0x50000000), E_INVALID),
    (dict(ins=None, outs=_addrs(3, _B), k=3), E_INVALID),
    (dict(ins=_addrs(3), outs=None, m=3), E_INVALID),
    (dict(ins=_addrs(3), outs=[_B, None, _B + 0x100000]), E_INVALID),
    (dict(ins=[0x10000000, None], outs=_addrs(3, _B)), E_INVALID),
    (dict(ins=_addrs(3), outs=[_B, None], count=0), E_INVALID),
    (dict(ins=_addrs(2), outs=_addrs(2, _B), count=1 << 63), E_INVALID),
    (dict(ins=[0x10000000, _T], outs=_addrs(1, _B), count=0x1000), E_INVALID),
    (dict(ins=_addrs(1), outs=[_B, _T], count=0x1000), E_INVALID),
    (dict(ins=_addrs(1), outs=_addrs(1, _B), acc=_T, count=0x1000), E_INVALID),
    (dict(ins=_addrs(2), outs=[_B, 0x40000000, _B]), E_INVALID),
    (dict(ins=_addrs(2), outs=[0x40000000, _B, _B + (N - 1) * 4]), E_INVALID),
    (dict(ins=[0x10000000, _B], outs=[0x40000000, _B]), E_INVALID),
    (dict(ins=[_B], outs=[_B + (N - 1) * 2]), E_INVALID),
    (dict(ins=[_B + (N - 1) * 2], outs=[_B], idt=FP32, odt=FP16), E_INVALID),
    (dict(ins=_addrs(2), outs=[0x40000000, _B + 4], acc=_B), E_INVALID),
    (dict(ins=_addrs(2), outs=[_B], acc=_B + (N - 1) * 4), E_INVALID),
    (dict(ins=_addrs(2), outs=[_B, _B], acc=_B), E_INVALID),
    # these pass every argument check: the visibility check refuses the fake addresses
    (dict(ins=_addrs(15), outs=_addrs(1, _B), acc=0x50000000), E_INVALID),
    (dict(ins=_addrs(16), outs=_addrs(1, _B)), E_INVALID),
    (dict(ins=_addrs(2), outs=[0x40000000, _B], acc=_B), E_INVALID),
    (dict(ins=[_B], outs=[_B + N * 2]), E_INVALID),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_every_refusal_of_the_unscaled_call_is_kept(i):
    kw, code = REFUSALS[i]
    rc_u, msg_u = _unscaled(**kw)
    rc, msg = _call(**kw)
    assert rc_u == code, "the case is not a refusal of mi_reduce_bcast_mixed"
    assert rc == code
    assert msg.split()[0] == msg_u.split()[0]
    assert msg == msg_u  # the whole message, in fact


@pytest.mark.parametrize("idt,odt", PAIRS)
@pytest.mark.parametrize("scale", BAD_SCALES, ids=lambda s: repr(s))
def test_bad_scale(idt, odt, scale):
    rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), idt=idt, odt=odt, scale=scale)
    assert rc == E_INVALID and msg.startswith("scale")
    # for an empty call too, and with an accumulator
    rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), idt=idt, odt=odt, scale=scale, count=0)
    assert rc == E_INVALID and msg.startswith("scale")
    if odt == FP32:
        rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), idt=idt, odt=odt, scale=scale, acc=0x50000000)
        assert rc == E_INVALID and msg.startswith("scale")


def test_scale_messages():
    for s, word in ((float("nan"), "NaN or infinite"), (float("inf"), "NaN or infinite"), (0.0, "zero"),
                    (1e-60, "zero as a float"), (1e300, "infinite as a float")):
        rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), scale=s)
        assert rc == E_INVALID and word in msg, (s, msg)
    # the smallest and largest magnitudes that are still a float pass on to the visibility check
    for s in (1e-45, -3e38, 2.0 ** 100, 2.0 ** -130):
        rc, msg = _call(_addrs(2), _addrs(2, 0x30000000), scale=s)
        assert rc == E_INVALID and "pageable" in msg, (s, msg)


@pytest.mark.parametrize("scale", [float("nan"), 0.0, 1e300], ids=lambda s: repr(s))
def test_order_of_the_scale_refusal(scale):
    """After the dtype pair, the op, acc's direction, k, m and the lists;
    before the entries and the overlap checks (mi_reduce_bcast_scaled's order)."""
    ins, outs = _addrs(2), _addrs(2, 0x30000000)
    rc, msg = _call(ins, outs, idt=FP32, odt=FP32, scale=scale)
    assert rc == E_UNSUPPORTED and "in_dtype" in msg
    rc, msg = _call(None, None, idt=BF16, odt=BF16, k=2, m=2, scale=scale)
    assert rc == E_UNSUPPORTED and "in_dtype" in msg
    rc, msg = _call(ins, outs, op=2, scale=scale)
    assert rc == E_UNSUPPORTED and msg.startswith("op")
    rc, msg = _call(ins, outs, idt=FP32, odt=BF16, acc=0x50000000, scale=scale)
    assert rc == E_UNSUPPORTED and msg.startswith("acc")
    rc, msg = _call(ins, outs, k=0, scale=scale)
    assert rc == E_INVALID and "input count k" in msg
    rc, msg = _call(ins, outs, m=17, scale=scale)
    assert rc == E_INVALID and "output count m" in msg
    rc, msg = _call(None, outs, k=2, scale=scale)
    assert rc == E_INVALID and "input list" in msg
    rc, msg = _call(ins, None, m=2, scale=scale)
    assert rc == E_INVALID and "output list" in msg
    rc, msg = _call(ins, [outs[0], None], scale=scale)
    assert rc == E_INVALID and msg.startswith("scale")
    rc, msg = _call(ins, [outs[0], outs[0]], scale=scale)
    assert rc == E_INVALID and msg.startswith("scale")


@pytest.mark.parametrize("idt,odt", PAIRS)
def test_empty_call_returns_zero(idt, odt):
    rc, _ = _call(_addrs(3), _addrs(2, 0x30000000), idt=idt, odt=odt, count=0)
    assert rc == 0
    rc, _ = _call([0x1000, 0x1000], [0x1000, 0x1000], idt=idt, odt=odt, count=0)  # touches nothing, overlapping or not
    assert rc == 0
    if odt == FP32:
        rc, _ = _call([0x1000], [0x1000], idt=idt, odt=odt, acc=0x1000, count=0)
        assert rc == 0
    # the refusals still come first
    rc, msg = _call(_addrs(3), _addrs(2, 0x30000000), idt=idt, odt=odt, count=0, op=1)
    assert rc == E_UNSUPPORTED and msg.startswith("op")
    rc, msg = _call(_addrs(3), [0x30000000, None], idt=idt, odt=odt, count=0)
    assert rc == E_INVALID and "outs[1] is NULL" in msg


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
    assert oneccl_amd.reduce_bcast_mixed_scaled is comp.reduce_bcast_mixed_scaled


def test_python_wrapper_checks():
    import torch
    import oneccl_amd as oa
    b = [torch.zeros(N, dtype=torch.bfloat16) for _ in range(2)]
    f = [torch.zeros(N, dtype=torch.float32) for _ in range(2)]
    h = torch.zeros(N, dtype=torch.float16)
    with pytest.raises(ValueError, match="at least one"):
        oa.reduce_bcast_mixed_scaled([], f, 0.5)
    with pytest.raises(TypeError, match="all inputs must have one dtype"):
        oa.reduce_bcast_mixed_scaled([b[0], h], f, 0.5)
    with pytest.raises(TypeError, match="all outputs must have one dtype"):
        oa.reduce_bcast_mixed_scaled(b, [f[0], h], 0.5)
    with pytest.raises(TypeError, match="unsupported dtype pair"):
        oa.reduce_bcast_mixed_scaled(f, [torch.zeros(N, dtype=torch.float32)], 0.5)
    with pytest.raises(TypeError, match="acc goes with fp32 outputs"):
        oa.reduce_bcast_mixed_scaled(f, [h], 0.5, acc=torch.zeros(N, dtype=torch.float32))
    with pytest.raises(TypeError, match="acc must be float32"):
        oa.reduce_bcast_mixed_scaled(b, f, 0.5, acc=torch.zeros(N, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="same numel"):
        oa.reduce_bcast_mixed_scaled(b, f, 0.5, acc=torch.zeros(N - 1, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        oa.reduce_bcast_mixed_scaled(b, [f[0], torch.zeros(2 * N, dtype=torch.float32)[::2]], 0.5)
    with pytest.raises(ValueError, match="device tensors"):
        oa.reduce_bcast_mixed_scaled(b, f, 0.5)
