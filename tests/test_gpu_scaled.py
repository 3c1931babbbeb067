"""mi_reduce_bcast_scaled on the GPU: every output bit for bit what the header
(include/mi_reduce.h) defines, NaN payloads included.

The expected value is built on the CPU from what the other tests already
trust (expected_scaled): the oracle's fold F, the accumulator A it implies
(F itself for fp32 / fp64, F widened for bf16 / fp16 in storage precision,
numpy's float32 left fold of the widened inputs under MI_F_ACC_FP32), one
numpy multiply in the compute type, the oracle's narrowing conversion, and
F's own bits wherever A is a NaN.  At scale 1 that construction reproduces
oracle_fold exactly except for bf16 denormals passing through k = 1 under
MI_F_BF16_RNE (tests/test_scaled_expected.py pins that on the CPU).
oracle_fold does not model MI_F_BF16_TAIL_TRUNC16, so for that variant F's
NaN elements come from the GPU's unscaled call.  Bounds and tile edges are
tests/test_gpu_scaled_bounds.py's."""
from __future__ import annotations

import numpy as np
import pytest

import oneccl_amd
from oneccl_amd import _lib, comp
from tests.guard import oracle_fold, ref_flags
from tests.util import BF16, FP16, FP32, FP64, assert_same, convert_expected, from_dev, rand_array, to_dev

pytestmark = pytest.mark.gpu

SUM = 0
F_ACC_FP32, F_TAIL = 0x4, 0x8
N = 3 * 4096 + 5  # > 40: rand_array's specials are present; a scalar tail of 5 (fp32: 1) elements
SCALES = [1 / 3, 1 / 8, -2.5, 1e-30]
VARIANTS = [(FP32, 0), (FP64, 0), (FP16, 0x1), (FP16, 0x5), (BF16, 0), (BF16, 0x3), (BF16, 0x7), (BF16, 0xF)]
VARIANT_IDS = ["f32", "f64", "f16-0x1", "f16-0x5", "bf16-0x0", "bf16-0x3", "bf16-0x7", "bf16-0xf"]


def expected_scaled(ins, dt, flags, scale, unscaled=None):
    """What mi_reduce_bcast_scaled stores for the numpy inputs `ins`.
    unscaled: the unscaled fold where the oracle has none (TAIL_TRUNC16)."""
    k = len(ins)
    if unscaled is not None:
        F = unscaled
    elif k == 1 and not flags & F_ACC_FP32:
        F = ins[0]
    else:
        F = oracle_fold(ins, dt, SUM, flags)
    with np.errstate(all="ignore"):
        if dt in (FP32, FP64):
            A = F
        elif flags & F_ACC_FP32:
            A = convert_expected(ins[0], dt, FP32, 0)
            for x in ins[1:]:
                A = convert_expected(x, dt, FP32, 0) + A
            assert A.dtype == np.float32
        else:
            A = convert_expected(F, dt, FP32, 0)
        s = np.float64(scale) if dt == FP64 else np.float32(scale)
        P = A * s
    assert P.dtype == A.dtype
    out = P if dt in (FP32, FP64) else convert_expected(P, FP32, dt, flags)
    nan = np.isnan(A)
    out = out.copy()
    out[nan] = F[nan]
    return out


def _inputs(dt, k, seed):
    return [rand_array(dt, N, seed=seed + j) for j in range(k)]


def _ptrs(ps):
    return _lib.void_ptr_array(list(ps))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _fresh(like, m):
    """m device buffers of `like`'s shape holding a non-zero pattern."""
    fill = np.full(like.nbytes, 0x5A, np.uint8).view(like.dtype)
    return [to_dev(fill) for _ in range(m)]


def _scaled(pin, pout, dt, flags, scale, n=N):
    _lib.check(_lib.mi().mi_reduce_bcast_scaled(_ptrs(pin), len(pin), _ptrs(pout), len(pout), n, dt, SUM, flags,
                                                scale, _stream()), "mi_reduce_bcast_scaled")


def _unscaled(pin, pout, dt, flags, n=N):
    _lib.check(_lib.mi().mi_reduce_bcast(_ptrs(pin), len(pin), _ptrs(pout), len(pout), n, dt, SUM, flags, _stream()),
               "mi_reduce_bcast")


def _gpu_unscaled(arrays, dev_ins, dt, flags):
    import torch
    (t, p), = _fresh(arrays[0], 1)
    _unscaled([q for _, q in dev_ins], [p], dt, flags)
    torch.cuda.synchronize()
    return from_dev(t, arrays[0])


# ---- every variant x (k, m) x scale ----------------------------------------------------

KM = [(1, 1), (1, 3), (2, 1), (2, 2), (3, 16), (8, 3), (9, 1), (9, 2), (16, 3), (16, 16)]


@pytest.mark.parametrize("k,m", KM, ids=[f"k{k}-m{m}" for k, m in KM])
@pytest.mark.parametrize("dt,flags", VARIANTS, ids=VARIANT_IDS)
def test_scaled_bits(dt, flags, k, m):
    """Separate outputs, each scale in turn on the same inputs; at scale 1.0
    (k >= 2) every output equals the GPU's own mi_reduce_bcast output byte for
    byte."""
    import torch
    arrays = _inputs(dt, k, 100 * k + m)
    ins = [to_dev(a) for a in arrays]
    pin = [p for _, p in ins]
    unscaled = _gpu_unscaled(arrays, ins, dt, flags)
    runs = [(s, _fresh(arrays[0], m)) for s in SCALES + ([1.0] if k >= 2 else [])]
    for s, outs in runs:
        _scaled(pin, [p for _, p in outs], dt, flags, s)
    torch.cuda.synchronize()
    if not flags & F_TAIL:  # the oracle models every other variant: the GPU's unscaled fold is its fold
        assert_same(unscaled, arrays[0] if (k == 1 and not flags & F_ACC_FP32) else oracle_fold(arrays, dt, SUM, flags),
                    dt, "unscaled")
    for s, outs in runs:
        exp = unscaled if s == 1.0 else expected_scaled(arrays, dt, flags, s, unscaled if flags & F_TAIL else None)
        for o, (t, _) in enumerate(outs):
            assert_same(from_dev(t, exp), exp, dt, f"scale {s!r}, output {o}")
    for (t, _), a in zip(ins, arrays):
        assert_same(from_dev(t, a), a, dt, "an input changed")


# ---- in place ----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("dt,flags", VARIANTS, ids=VARIANT_IDS)
def test_in_place_allreduce(dt, flags, k):
    """outs[i] == inputs[i] for all i: every buffer ends as the scaled sum."""
    import torch
    s = 1.0 / k
    arrays = _inputs(dt, k, 700 + k)
    ins = [to_dev(a) for a in arrays]
    pin = [p for _, p in ins]
    unscaled = _gpu_unscaled(arrays, ins, dt, flags) if flags & F_TAIL else None
    _scaled(pin, pin, dt, flags, s)
    torch.cuda.synchronize()
    exp = expected_scaled(arrays, dt, flags, s, unscaled)
    for i, (t, _) in enumerate(ins):
        assert_same(from_dev(t, exp), exp, dt, f"buffer {i}")


@pytest.mark.parametrize("dt,flags", VARIANTS, ids=VARIANT_IDS)
def test_one_output_in_place_others_separate(dt, flags):
    """(3, 2) with outs[0] == inputs[1]: both outputs hold the value, the
    inputs that are not outputs are unchanged."""
    import torch
    s = -2.5
    arrays = _inputs(dt, 3, 800)
    ins = [to_dev(a) for a in arrays]
    pin = [p for _, p in ins]
    unscaled = _gpu_unscaled(arrays, ins, dt, flags) if flags & F_TAIL else None
    (t_out, p_out), = _fresh(arrays[0], 1)
    _scaled(pin, [pin[1], p_out], dt, flags, s)
    torch.cuda.synchronize()
    exp = expected_scaled(arrays, dt, flags, s, unscaled)
    assert_same(from_dev(ins[1][0], exp), exp, dt, "the output that is inputs[1]")
    assert_same(from_dev(t_out, exp), exp, dt, "the separate output")
    for j in (0, 2):
        assert_same(from_dev(ins[j][0], exp), arrays[j], dt, f"inputs[{j}] unchanged")


# ---- graph capture -------------------------------------------------------------------------

def test_captured_chain_replays():
    """Three mi_reduce_bcast_scaled launches in a row on one stream (a linear
    graph, no parallel branches), captured once and replayed twice on
    rewritten inputs: the mean of 3 inputs into two buffers; one of those and
    a fourth input, times -2.5, into three; then the in-place averaged
    allreduce of two of those."""
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
        _lib.check(m.mi_reduce_bcast_scaled(ptrs(a[:3]), 3, ptrs([o1, o2]), 2, n, FP32, SUM, 0, 1 / 3, s), "launch 1")
        _lib.check(m.mi_reduce_bcast_scaled(ptrs([o1, a[3]]), 2, ptrs([p1, p2, p3]), 3, n, FP32, SUM, 0, -2.5, s),
                   "launch 2")
        _lib.check(m.mi_reduce_bcast_scaled(ptrs([p1, p2]), 2, ptrs([p1, p2]), 2, n, FP32, SUM, 0, 0.5, s), "launch 3")
    for seed in (11, 23):
        arrays = fill(seed)
        g.replay()
        torch.cuda.synchronize()
        e1 = expected_scaled(arrays[:3], FP32, 0, 1 / 3)
        e2 = expected_scaled([e1, arrays[3]], FP32, 0, -2.5)
        e3 = expected_scaled([e2, e2], FP32, 0, 0.5)
        for t, e, what in ((o1, e1, "o1"), (o2, e1, "o2"), (p3, e2, "p3"), (p1, e3, "p1"), (p2, e3, "p2")):
            assert_same(t.cpu().numpy(), e, FP32, f"{what}, seed {seed}")
        for t, x in zip(a, arrays):
            assert_same(t.cpu().numpy(), x, FP32, f"an input changed, seed {seed}")


# ---- comp.reduce_bcast_scaled ------------------------------------------------------------

_SIGNED = {2: np.int16, 4: np.int32}


@pytest.mark.parametrize("dt,name", [(FP32, "float32"), (BF16, "bfloat16")], ids=["f32", "bf16"])
def test_wrapper(dt, name):
    import torch
    td = getattr(torch, name)
    k = 3
    arrays = _inputs(dt, k, 40)
    ins = [torch.from_numpy(a.view(_SIGNED[a.itemsize]).copy()).view(td).cuda() for a in arrays]
    outs = [torch.zeros(N, dtype=td, device="cuda") for _ in range(2)] + [ins[1]]  # the last one in place
    oneccl_amd.reduce_bcast_scaled(ins, outs, 1 / k)
    torch.cuda.synchronize()
    exp = expected_scaled(arrays, dt, ref_flags(dt), 1 / k)  # the wrapper's default flags are the reference's
    host = lambda t: t.view({2: torch.int16, 4: torch.int32}[exp.itemsize]).cpu().numpy().view(exp.dtype)  # noqa: E731
    for o, t in enumerate(outs):
        assert_same(host(t), exp, dt, f"output {o}")
    assert_same(host(ins[0]), arrays[0], dt, "inputs[0] unchanged")
    assert_same(host(ins[2]), arrays[2], dt, "inputs[2] unchanged")


def test_wrapper_refuses_mismatched_tensors():
    import torch
    a = torch.ones(64, dtype=torch.float32, device="cuda")
    b = torch.ones(64, dtype=torch.float32, device="cuda")
    o = torch.zeros(64, dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError, match="one dtype"):
        comp.reduce_bcast_scaled([a, b], [o, torch.zeros(64, dtype=torch.int32, device="cuda")], 0.5)
    with pytest.raises(TypeError, match="one dtype"):
        comp.reduce_bcast_scaled([a, b.to(torch.bfloat16)], [o], 0.5)
    with pytest.raises(ValueError, match="same numel"):
        comp.reduce_bcast_scaled([a, b], [o, torch.zeros(65, dtype=torch.float32, device="cuda")], 0.5)
    with pytest.raises(ValueError, match="one device"):
        comp.reduce_bcast_scaled([a, b], [o, torch.zeros(64, dtype=torch.float32)], 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        comp.reduce_bcast_scaled([a, b], [o, torch.zeros(128, dtype=torch.float32, device="cuda")[::2]], 0.5)
    with pytest.raises(ValueError, match="at least one"):
        comp.reduce_bcast_scaled([a, b], [], 0.5)
    with pytest.raises(_lib.MiReduceError, match=r"outs\[0\] and outs\[1\] overlap"):
        comp.reduce_bcast_scaled([a, b], [o, o], 0.5)
    with pytest.raises(_lib.MiReduceError, match="scale is zero"):
        comp.reduce_bcast_scaled([a, b], [o], 0.0)
    ai = torch.ones(64, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.MiReduceError, match="dtype"):
        comp.reduce_bcast_scaled([ai, ai.clone()], [torch.zeros(64, dtype=torch.int32, device="cuda")], 0.5)
    torch.cuda.synchronize()
    assert bool((o == 0).all())  # no refused call wrote
