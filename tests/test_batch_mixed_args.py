"""mi_reduce_batch_mixed's host-side refusals, in the header's order.  As
tests/test_mixed_args.py, no device is needed: the descriptors hold fake
addresses that are never dereferenced (a batch that passes every argument
check goes on to the device-visibility check, which refuses them)."""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd import _lib

FP16, FP32, FP64, BF16 = 8, 9, 10, 11
E_INVALID, E_UNSUPPORTED, N = -1, -2, 64
A, B, C, D, TOP = 0x10000000, 0x20000000, 0x30000000, 0x40000000, (1 << 64) - 0x1000


def _call(descs, idt=BF16, odt=FP32, op=0, n=None, scale=1 / 3):
    mi = _lib.mi()
    rc = mi.mi_reduce_batch_mixed(None if descs is None else _lib.desc_array(descs),
                                  len(descs) if n is None else n, idt, odt, op, 0, scale, None)
    return rc, mi.mi_last_error().decode() if rc else ""


# (arguments, code, message fragment) in the order of the refusals; a case also holds what later refusals object to
REFUSALS = [
    (dict(descs=None, n=-1, idt=FP32, odt=FP32, op=1, scale=0.0), E_UNSUPPORTED, "in_dtype/out_dtype"),
    (dict(descs=None, n=-1, idt=FP64, odt=FP32), E_UNSUPPORTED, "in_dtype/out_dtype"),
    (dict(descs=None, n=-1, op=1, scale=0.0), E_UNSUPPORTED, "op:"),
    (dict(descs=None, n=-1, scale=0.0), E_INVALID, "n:"),
    (dict(descs=None, n=2, scale=0.0), E_INVALID, "descs:"),
    (dict(descs=[(0, B, N)], scale=float("nan")), E_INVALID, "scale is NaN or infinite"),
    (dict(descs=[(0, B, N)], scale=0.0), E_INVALID, "scale is zero"),
    (dict(descs=[(0, B, N)], scale=1e-60), E_INVALID, "zero as a float"),
    (dict(descs=[(0, B, N)], scale=1e300), E_INVALID, "infinite as a float"),
    (dict(descs=[(A, B, N), (0, TOP, N)]), E_INVALID, "descs[1].in is NULL"),
    (dict(descs=[(A, B, 1 << 63), (C, 0, N)]), E_INVALID, "descs[1].inout is NULL"),
    (dict(descs=[(A, A, N), (C, D, 1 << 63)]), E_INVALID, "descs[1].in + count overflows"),
    (dict(descs=[(A, B, N), (TOP, D, 0x1000)]), E_INVALID, "descs[1].in + count overflows"),   # 0x2000 bytes of bf16
    (dict(descs=[(A, B, N), (C, TOP, 0x7FF)]), E_INVALID, "descs[1].inout + count overflows"),  # fits as bf16, not fp32
    (dict(descs=[(A, TOP, 0x7FF)], idt=FP32, odt=BF16), E_INVALID, "pageable"),                 # each side's own size
    (dict(descs=[(A, B, N), (C, B + (N - 1) * 4, N)]), E_INVALID, "descs[0].inout and descs[1].inout overlap"),
    (dict(descs=[(A, B, N), (B + (N - 1) * 4, D, N)]), E_INVALID, "descs[1].in overlaps descs[0].inout"),
    (dict(descs=[(A, B, N), (C, C, N)]), E_INVALID, "descs[1].in overlaps descs[1].inout"),      # its own, equal
    (dict(descs=[(B + (N - 1) * 2, B, N)], idt=FP32, odt=BF16), E_INVALID, "descs[0].in overlaps descs[0].inout"),
    # touching ranges, and overlaps of empty descriptors, pass every argument check
    (dict(descs=[(A, B, N), (B + N * 4, B - N * 4, N), (B, B, 0)]), E_INVALID, "pageable"),
    (dict(descs=[(B + N * 2, B, N)], idt=FP32, odt=BF16), E_INVALID, "pageable"),
    # empty batches return 0: n == 0 ahead of the list and the scale; count == 0 with pointers not looked at
    (dict(descs=None, n=0, scale=0.0), 0, ""),
    (dict(descs=None, n=0, idt=FP32, odt=FP16, scale=0.0), 0, ""),
    (dict(descs=[(0, 0, 0), (A, A, 0), (TOP, 0, 0)], idt=FP16), 0, ""),
    (dict(descs=[(0, 0, 0), (A, A, 0), (TOP, 0, 0)], idt=FP32, odt=BF16), 0, ""),
]


@pytest.mark.parametrize("kw,code,frag", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_in_order_and_empty_batches(kw, code, frag):
    rc, msg = _call(**kw)
    assert rc == code and frag in msg, (rc, msg)


def test_pageable_batch_is_refused_and_untouched():
    src = [np.full(N, 0x3F80, np.uint16) for _ in range(2)]
    dst = [np.full(N, 7.0, np.float32) for _ in range(2)]
    rc, msg = _call([(s.ctypes.data, d.ctypes.data, N) for s, d in zip(src, dst)], scale=1.0)
    assert rc == E_INVALID and "pageable" in msg
    assert all((d == 7.0).all() for d in dst) and all((s == 0x3F80).all() for s in src)


def test_binding_and_python_wrapper_checks():
    """CPU tensors: each of the wrapper's checks raises before any pointer is taken."""
    import torch
    import oneccl_amd as oa
    assert _lib.mi().mi_version() == 101
    assert [len(e[2]) for e in _lib.MI_API if e[0] == "mi_reduce_batch_mixed"] == [8]
    b, h, f = torch.zeros(N, dtype=torch.bfloat16), torch.zeros(N, dtype=torch.float16), torch.zeros(N)
    oa.reduce_batch_mixed([])  # nothing to do
    for pairs, exc, match in [([(b, f), (h, f)], TypeError, "all sources must have one dtype"),
                              ([(f, b), (f, h)], TypeError, "all destinations must have one dtype"),
                              ([(f, f)], TypeError, "unsupported dtype pair"), ([(b, h)], TypeError, "unsupported dtype"),
                              ([(b, f), (b, torch.zeros(N + 1))], ValueError, "same numel"),
                              ([(b, torch.zeros(2 * N)[::2])], ValueError, "contiguous"),
                              ([(b, f)], ValueError, "device tensors")]:
        with pytest.raises(exc, match=match):
            oa.reduce_batch_mixed(pairs, scale=0.5)
