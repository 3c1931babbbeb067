"""The kernels and the host fold give the same bytes for every raw flag word.

comp.cpp sends a small host bucket to mi_host_reduce and a large one to the
kernels, and coop_fold splits one bucket between the two, so the two
libraries must canonicalise a flag word alike (the host fold with canon_flags
of oneccl_amd/csrc/variant.hpp, mi_reduce.hip with its own copy of that
text).  For every dtype, op and flags in 0..31 this
runs mi_reduce_multi on device buffers and mi_host_reduce on the same inputs
and compares return codes and, where they are 0, the outputs bit for bit:

  k = 1   the copy, or under MI_F_ACC_FP32 the widening and its rounding
  k = 2   the 2-input kernel, where min / max drop MI_F_ACC_FP32
  k = 3   the fan-in
  count 33  two whole 16-element groups and a one-element tail: the smallest
            count at which MI_F_BF16_TAIL_TRUNC16 truncates something (element
            32), with one scalar tail element beside whole vectors
  count 16  the threshold equals the count

Integers are drawn over their full range.  Floats are finite, of both signs,
with magnitudes in [2^-4, 2^4], so that three of them neither overflow nor go
denormal in fp16; elements 0 and 1 hold (+0, -0, +0) and (-0, +0, -0) across
the inputs, for the order of a min / max tie.  No NaNs: test_gpu_nan_paths.py,
test_gpu_nan.py and test_nanvec.py own those.  One synchronisation per
(dtype, op); each dtype takes well under a second.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from oneccl_amd import _lib
from tests.test_gpu_bounds import _stream
from tests.util import ALL_DTYPES, BF16, DT_NAME, FP16, FP32, FP64, INT_DTYPES, OP_NAME, OPS, assert_same, to_dev

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not _lib.shim().mi_host_supported(), reason="CPU lacks AVX2/F16C: no host path")]

SEED = 3  # 1 and 2 leave element 32's bf16 sum exact: flags 6 and 14 then agree (check_draw_tells_variants)
KS = (1, 2, 3)
COUNTS = (16, 33)
N = max(COUNTS)
SLOT = 48  # elements between two outputs: 16-byte multiples for every element size
CASES = [(flags, k, count) for flags in range(32) for k in KS for count in COUNTS]


@functools.lru_cache(maxsize=None)
def draw(dt: int):
    """The three inputs of a dtype, N elements each."""
    rng = np.random.default_rng(SEED + dt)
    st = oracle.NP_DTYPE[dt]
    if dt in INT_DTYPES:
        info = np.iinfo(st)
        return tuple(rng.integers(info.min, info.max, size=N, endpoint=True, dtype=st) for _ in KS)
    ins = []
    for j in range(len(KS)):
        f = np.ldexp(rng.uniform(1.0, 2.0, N), rng.integers(-4, 4, N)) * rng.choice([-1.0, 1.0], N)
        f[0], f[1] = (0.0, -0.0) if j % 2 == 0 else (-0.0, 0.0)
        f32 = f.astype(np.float32)
        ins.append(f if dt == FP64 else f32 if dt == FP32 else
                   oracle.f32_to_bf16(f32, rne=True) if dt == BF16 else oracle.f32_to_fp16(f32))
    return tuple(ins)


def host_fold(ins, k, count, dt, op, flags):
    out = np.zeros(count, ins[0].dtype)
    arr = _lib.void_ptr_array([x.ctypes.data for x in ins[:k]])
    return _lib.shim().mi_host_reduce(arr, k, out.ctypes.data, count, dt, op, flags), out


def check_draw_tells_variants():
    """Host outputs alone: the bf16 draw separates the variants a wrong
    canonicalisation would confuse (rounding, accumulation, the truncated
    tail).  If it does not, change SEED until it does."""
    out = {f: host_fold(draw(BF16), 3, N, BF16, 0, f)[1].tobytes() for f in (0, 2, 4, 6, 14)}
    assert len({out[4], out[6], out[14]}) == 3, "flags 4, 6 and 14 do not give three different bf16 sums"
    assert out[0] != out[2], "flags 0 and 2 give the same bf16 sum"


@pytest.mark.parametrize("dt", ALL_DTYPES, ids=[DT_NAME[d] for d in ALL_DTYPES])
def test_device_and_host_agree(dt):
    import torch
    if dt == BF16:
        check_draw_tells_variants()
    ins = draw(dt)
    for f in ins if dt not in INT_DTYPES else ():  # the draw is what the docstring says it is
        v = (oracle.bf16_to_f32(f) if dt == BF16 else oracle.fp16_to_f32(f) if dt == FP16 else f).astype(np.float64)
        assert np.all(v[:2] == 0) and np.all((np.abs(v[2:]) >= 2.0 ** -4) & (np.abs(v[2:]) <= 2.0 ** 4))
    dev = [to_dev(x) for x in ins]
    arr = _lib.void_ptr_array([p for _, p in dev])
    es = ins[0].itemsize
    m = _lib.mi()
    for op in OPS:
        outs = torch.zeros(len(CASES) * SLOT * es, dtype=torch.int8, device="cuda")
        rcs = [m.mi_reduce_multi(arr, k, outs.data_ptr() + i * SLOT * es, count, dt, op, flags, _stream())
               for i, (flags, k, count) in enumerate(CASES)]
        torch.cuda.synchronize()
        got = outs.cpu().numpy().view(ins[0].dtype).reshape(len(CASES), SLOT)
        for i, (flags, k, count) in enumerate(CASES):
            what = f"{DT_NAME[dt]} {OP_NAME[op]} flags={flags:#x} k={k} count={count}"
            rc, exp = host_fold(ins, k, count, dt, op, flags)
            assert rcs[i] == rc, f"{what}: mi_reduce_multi returned {rcs[i]}, mi_host_reduce {rc}"
            if rc == 0:
                assert_same(got[i, :count], exp, dt, what)
