"""mi_reduce_bcast above the kernel: the Python wrapper, graph capture, and
the sequence it replaces (mi_reduce_multi into the first output, then one
mi_copy per further output).  Bit-exact against the oracle's fold; bounds
and tile edges are tests/test_gpu_bcast_bounds.py's."""
from __future__ import annotations

import numpy as np
import pytest

import oneccl_amd
from oneccl_amd import _lib, comp
from tests.guard import oracle_fold, ref_flags
from tests.util import BF16, FP32, assert_same, rand_array

pytestmark = pytest.mark.gpu

INT32 = 4
SUM, MAX = 0, 3
_SIGNED = {2: np.int16, 4: np.int32}


def _tensor(a, torch_dtype):
    import torch
    return torch.from_numpy(a.view(_SIGNED[a.itemsize]).copy()).view(torch_dtype).cuda()


def _host(t, like):
    import torch
    st = {2: torch.int16, 4: torch.int32}[like.itemsize]
    return t.view(st).cpu().numpy().view(like.dtype)


# ---- comp.reduce_bcast ----------------------------------------------------------------

@pytest.mark.parametrize("dt,name,op", [(FP32, "float32", SUM), (BF16, "bfloat16", SUM), (INT32, "int32", MAX)],
                         ids=["f32-sum", "bf16-sum", "i32-max"])
def test_wrapper(dt, name, op):
    import torch
    td = getattr(torch, name)
    n, k = 3 * 4096 + 5, 3
    arrays = [rand_array(dt, n, seed=40 + j, op=op) for j in range(k)]
    ins = [_tensor(a, td) for a in arrays]
    outs = [torch.zeros(n, dtype=td, device="cuda") for _ in range(2)] + [ins[1]]  # the last one in place
    oneccl_amd.reduce_bcast(ins, outs, op=comp.reduction(op))
    torch.cuda.synchronize()
    exp = oracle_fold(arrays, dt, op, ref_flags(dt))  # the wrapper's default flags are the reference's
    for o, t in enumerate(outs):
        assert_same(_host(t, exp), exp, dt, f"output {o}")
    assert_same(_host(ins[0], exp), arrays[0], dt, "inputs[0] unchanged")
    assert_same(_host(ins[2], exp), arrays[2], dt, "inputs[2] unchanged")


def test_wrapper_refuses_mismatched_tensors():
    import torch
    a = torch.ones(64, dtype=torch.float32, device="cuda")
    b = torch.ones(64, dtype=torch.float32, device="cuda")
    o = torch.zeros(64, dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError, match="one dtype"):
        comp.reduce_bcast([a, b], [o, torch.zeros(64, dtype=torch.int32, device="cuda")])
    with pytest.raises(TypeError, match="one dtype"):
        comp.reduce_bcast([a, b.to(torch.bfloat16)], [o])
    with pytest.raises(ValueError, match="same numel"):
        comp.reduce_bcast([a, b], [o, torch.zeros(65, dtype=torch.float32, device="cuda")])
    with pytest.raises(ValueError, match="one device"):
        comp.reduce_bcast([a, b], [o, torch.zeros(64, dtype=torch.float32)])
    with pytest.raises(ValueError, match="contiguous"):
        comp.reduce_bcast([a, b], [o, torch.zeros(128, dtype=torch.float32, device="cuda")[::2]])
    with pytest.raises(ValueError, match="at least one"):
        comp.reduce_bcast([a, b], [])
    with pytest.raises(_lib.MiReduceError, match=r"outs\[0\] and outs\[1\] overlap"):
        comp.reduce_bcast([a, b], [o, o])
    torch.cuda.synchronize()
    assert bool((o == 0).all())  # no refused call wrote


# ---- graph capture -------------------------------------------------------------------

def test_captured_chain_replays():
    """Three mi_reduce_bcast launches in a row on one stream (a linear graph,
    no parallel branches), captured once and replayed twice on rewritten
    inputs: fold 3 inputs into two buffers; fold one of those with a fourth
    input into three; then the in-place allreduce of two of those."""
    import torch
    m = _lib.mi()
    n = 4097
    dev = lambda: torch.empty(n, dtype=torch.float32, device="cuda")  # noqa: E731
    a = [dev() for _ in range(4)]
    o1, o2, p1, p2, p3 = (dev() for _ in range(5))

    def fill(seed):
        arrays = [rand_array(FP32, n, seed=seed + j) for j in range(4)]
        for t, x in zip(a, arrays):
            t.copy_(torch.from_numpy(x))
        for t in (o1, o2, p1, p2, p3):
            t.fill_(-7.0)
        return arrays

    ptrs = lambda ts: _lib.void_ptr_array([t.data_ptr() for t in ts])  # noqa: E731
    fill(1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(m.mi_reduce_bcast(ptrs(a[:3]), 3, ptrs([o1, o2]), 2, n, FP32, SUM, 0, s), "mi_reduce_bcast 1")
        _lib.check(m.mi_reduce_bcast(ptrs([o1, a[3]]), 2, ptrs([p1, p2, p3]), 3, n, FP32, MAX, 0, s), "mi_reduce_bcast 2")
        _lib.check(m.mi_reduce_bcast(ptrs([p1, p2]), 2, ptrs([p1, p2]), 2, n, FP32, SUM, 0, s), "mi_reduce_bcast 3")
    for seed in (11, 23):
        arrays = fill(seed)
        g.replay()
        torch.cuda.synchronize()
        e1 = oracle_fold(arrays[:3], FP32, SUM, 0)
        e2 = oracle_fold([e1, arrays[3]], FP32, MAX, 0)
        e3 = oracle_fold([e2, e2], FP32, SUM, 0)
        for t, e, what in ((o1, e1, "o1"), (o2, e1, "o2"), (p3, e2, "p3"), (p1, e3, "p1"), (p2, e3, "p2")):
            assert_same(t.cpu().numpy(), e, FP32, f"{what}, seed {seed}")
        for t, x in zip(a, arrays):
            assert_same(t.cpu().numpy(), x, FP32, f"an input changed, seed {seed}")


# ---- the sequence it replaces ------------------------------------------------------------

@pytest.mark.parametrize("dt", [FP32, BF16], ids=["f32", "bf16"])
def test_equals_reduce_multi_then_copies(dt):
    """(8, 8) at 1 MiB + 3 elements per buffer (past one tile per CU): byte
    for byte what mi_reduce_multi into outs[0] and seven mi_copy calls leave,
    and the oracle's fold."""
    import torch
    m = _lib.mi()
    es = 4 if dt == FP32 else 2
    n, k, mo = (1 << 20) // es + 3, 8, 8
    flags = ref_flags(dt)
    arrays = [rand_array(dt, n, seed=60 + j) for j in range(k)]
    st = torch.int32 if es == 4 else torch.int16
    ins = [_tensor(x, st) for x in arrays]
    fused = [torch.zeros(n, dtype=st, device="cuda") for _ in range(mo)]
    seq = [torch.zeros(n, dtype=st, device="cuda") for _ in range(mo)]
    s = torch.cuda.current_stream().cuda_stream
    pin = _lib.void_ptr_array([t.data_ptr() for t in ins])
    _lib.check(m.mi_reduce_bcast(pin, k, _lib.void_ptr_array([t.data_ptr() for t in fused]), mo, n, dt, SUM, flags, s),
               "mi_reduce_bcast")
    _lib.check(m.mi_reduce_multi(pin, k, seq[0].data_ptr(), n, dt, SUM, flags, s), "mi_reduce_multi")
    for t in seq[1:]:
        _lib.check(m.mi_copy(seq[0].data_ptr(), t.data_ptr(), n * es, 1, s), "mi_copy")
    torch.cuda.synchronize()
    exp = oracle_fold(arrays, dt, SUM, flags)
    for o in range(mo):
        assert torch.equal(fused[o], seq[o]), f"output {o} differs from the sequence's"
        assert_same(_host(fused[o], exp), exp, dt, f"output {o}")
