"""mi_reduce_bcast_mixed_scaled on the GPU: every output bit for bit the
composition the header defines (tests.mixed_scaled.expected_mixed_scaled) and
byte for byte what the GPU's own sequence of existing calls leaves: the
unscaled mixed call into a scratch buffer, mi_reduce_bcast_scaled with k = 1
over it and, under an accumulator, mi_reduce_multi({acc, P}); narrowing,
mi_reduce_bcast_scaled in fp32 into a scratch buffer and mi_convert x M.

The scales: 1/3 (no power of two: a fused multiply-add under the accumulator,
or a sum rounded to storage before the multiply, gives other bits,
tests/test_mixed_scaled_expected.py), 1.0 (the unscaled call's bytes without an
accumulator), -2.5 (signs; NaNs keep theirs), 2^100 (products overflow to Inf)
and 2^-130 (denormal products, which bf16 round-to-nearest-even flushes).
Bounds and tile edges are tests/test_gpu_mixed_scaled_bounds.py's, the dense
NaN table tests/test_gpu_mixed_scaled_nan.py's."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import oneccl_amd
from oneccl_amd import _lib
from tests.mixed import NARROWING, PAIR_IDS, SUM, WIDENING, call_mixed
from tests.mixed_scaled import call_mixed_scaled, expected_mixed_scaled
from tests.util import BF16, FP16, FP32, assert_same, rand_array

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 5  # > 40: rand_array's specials are present
KM = [(1, 1), (2, 1), (3, 16), (8, 3), (9, 2), (16, 3)]
SCALES = [1 / 3, 1.0, -2.5, 2.0 ** 100, 2.0 ** -130]
SCALE_IDS = ["third", "one", "minus2.5", "2^100", "2^-130"]
_SIGNED = {2: np.int16, 4: np.int32}


@functools.lru_cache(maxsize=None)
def _inputs(dt):
    """16 inputs of dtype dt, drawn once; never changed."""
    ins = tuple(rand_array(dt, N, seed=7100 + 31 * dt + j) for j in range(16))
    for a in ins:
        a.setflags(write=False)
    return ins


@functools.lru_cache(maxsize=None)
def _acc():
    a = rand_array(FP32, N, seed=7999)
    a.setflags(write=False)
    return a


def _dev(a):
    import torch
    return torch.from_numpy(a.view(_SIGNED[a.itemsize]).copy()).cuda()


def _host(t, np_dtype):
    return t.cpu().numpy().view(np_dtype)


def _filled(es):
    """An output buffer of N elements of es bytes, every byte 0x5A."""
    import torch
    return torch.full((N * es,), 0x5A, dtype=torch.uint8, device="cuda")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(dt):
    return np.float32 if dt == FP32 else np.uint16


def _ptrs(ts):
    return _lib.void_ptr_array([t.data_ptr() for t in ts])


def _sequence(dins, idt, odt, flags, scale, k, m, dacc):
    """The sequence the fused call replaces, from calls that exist without it;
    returns its m outputs."""
    mi, s = _lib.mi(), _stream()
    eso = 4 if odt == FP32 else 2
    outs = [_filled(eso) for _ in range(m)]
    scratch = _filled(4)
    if odt == FP32:
        call_mixed([t.data_ptr() for t in dins[:k]], idt, [scratch.data_ptr()], FP32, N, flags, None, s)
        if dacc is None:
            _lib.check(mi.mi_reduce_bcast_scaled(_ptrs([scratch]), 1, _ptrs(outs), m, N, FP32, SUM, 0, scale, s),
                       "mi_reduce_bcast_scaled")
        else:
            p = _filled(4)
            _lib.check(mi.mi_reduce_bcast_scaled(_ptrs([scratch]), 1, _ptrs([p]), 1, N, FP32, SUM, 0, scale, s),
                       "mi_reduce_bcast_scaled")
            for o in outs:
                _lib.check(mi.mi_reduce_multi(_ptrs([dacc, p]), 2, o.data_ptr(), N, FP32, SUM, 0, s), "mi_reduce_multi")
    else:
        _lib.check(mi.mi_reduce_bcast_scaled(_ptrs(dins[:k]), k, _ptrs([scratch]), 1, N, FP32, SUM, 0, scale, s),
                   "mi_reduce_bcast_scaled")
        for o in outs:
            _lib.check(mi.mi_convert(scratch.data_ptr(), FP32, o.data_ptr(), odt, N, flags, s), "mi_convert")
    return outs


def _run(idt, odt, flags, scale, acc_mode):
    """acc_mode: None, "separate" or "inplace" (acc == outs[0])."""
    import torch
    ins = _inputs(idt)
    dins = [_dev(a) for a in ins]
    eso = 4 if odt == FP32 else 2
    for k, m in KM:
        if acc_mode and k > 15:
            k = 15
        acc = _acc() if acc_mode else None
        what = f"{idt}->{odt} flags {flags:#x} scale {scale!r} k={k} m={m} acc={acc_mode}"
        outs = [_filled(eso) for _ in range(m)]
        dacc = None
        if acc_mode == "separate":
            dacc = _dev(acc)
        elif acc_mode == "inplace":
            dacc = _dev(acc)
            outs[0] = dacc.view(torch.uint8)
        call_mixed_scaled([t.data_ptr() for t in dins[:k]], idt, [t.data_ptr() for t in outs], odt, N, flags, scale,
                          dacc.data_ptr() if dacc is not None else None, _stream())
        seq = _sequence(dins, idt, odt, flags, scale, k, m, _dev(acc) if acc_mode else None)
        torch.cuda.synchronize()
        exp = expected_mixed_scaled(list(ins[:k]), idt, odt, flags, scale, acc)
        for o, t in enumerate(outs):
            assert_same(_host(t, _np(odt)), exp, odt, f"{what}: output {o}")
            assert torch.equal(t, seq[o]), f"{what}: output {o} differs from the sequence of existing calls"
        if acc_mode == "separate":
            assert_same(_host(dacc, np.float32), acc, FP32, f"{what}: acc changed")
    for j, (t, a) in enumerate(zip(dins, ins)):
        assert_same(_host(t, _np(idt)), a, idt, f"{idt}->{odt}: inputs[{j}] changed")


@pytest.mark.parametrize("scale", SCALES, ids=SCALE_IDS)
@pytest.mark.parametrize("idt,odt,flags", NARROWING, ids=PAIR_IDS[2:])
def test_narrowing(idt, odt, flags, scale):
    _run(idt, odt, flags, scale, None)


@pytest.mark.parametrize("scale", SCALES, ids=SCALE_IDS)
@pytest.mark.parametrize("acc_mode", [None, "separate", "inplace"], ids=["no-acc", "acc", "acc-in-place"])
@pytest.mark.parametrize("idt,odt,flags", WIDENING, ids=PAIR_IDS[:2])
def test_widening(idt, odt, flags, acc_mode, scale):
    _run(idt, odt, flags, scale, acc_mode)


@pytest.mark.parametrize("idt,odt,flags", WIDENING + NARROWING, ids=PAIR_IDS)
def test_scale_one_is_the_unscaled_call(idt, odt, flags):
    """Without an accumulator; against the unscaled call on the GPU."""
    import torch
    dins = [_dev(a) for a in _inputs(idt)[:5]]
    eso = 4 if odt == FP32 else 2
    a, b = _filled(eso), _filled(eso)
    call_mixed_scaled([t.data_ptr() for t in dins], idt, [a.data_ptr()], odt, N, flags, 1.0, None, _stream())
    call_mixed([t.data_ptr() for t in dins], idt, [b.data_ptr()], odt, N, flags, None, _stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_wrapper():
    """oneccl_amd.reduce_bcast_mixed_scaled: dtypes from the tensors,
    flags=None the reference's (bf16: round to nearest even), acc in place."""
    import torch
    b = _inputs(BF16)[:3]
    tb = [_dev(a).view(torch.bfloat16) for a in b]
    acc = _dev(_acc()).view(torch.float32)
    other = torch.zeros(N, dtype=torch.float32, device="cuda")
    oneccl_amd.reduce_bcast_mixed_scaled(tb, [acc, other], 1 / 3, acc=acc)
    plain = torch.zeros(N, dtype=torch.float32, device="cuda")
    oneccl_amd.reduce_bcast_mixed_scaled(tb, [plain], 1 / 3)
    f = _inputs(FP32)[:4]
    tf = [_dev(a).view(torch.float32) for a in f]
    ob = [torch.zeros(N, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    oh = torch.zeros(N, dtype=torch.float16, device="cuda")
    oneccl_amd.reduce_bcast_mixed_scaled(tf, ob, 0.25)
    oneccl_amd.reduce_bcast_mixed_scaled(tf, [oh], scale=1 / 3)
    oneccl_amd.reduce_bcast_mixed_scaled(tf, [ob[1]], 1 / 3, flags=0)  # truncation
    torch.cuda.synchronize()
    e = expected_mixed_scaled(list(b), BF16, FP32, 0, 1 / 3, _acc())
    assert_same(_host(acc.view(torch.int32), np.float32), e, FP32, "acc in place")
    assert_same(_host(other.view(torch.int32), np.float32), e, FP32, "second output")
    assert_same(_host(plain.view(torch.int32), np.float32), expected_mixed_scaled(list(b), BF16, FP32, 0, 1 / 3), FP32,
                "no acc")
    assert_same(_host(ob[0].view(torch.int16), np.uint16), expected_mixed_scaled(list(f), FP32, BF16, 0x2, 0.25), BF16,
                "bf16 rne")
    assert_same(_host(ob[1].view(torch.int16), np.uint16), expected_mixed_scaled(list(f), FP32, BF16, 0, 1 / 3), BF16,
                "bf16 trunc")
    assert_same(_host(oh.view(torch.int16), np.uint16), expected_mixed_scaled(list(f), FP32, FP16, 0, 1 / 3), FP16,
                "fp16")
    with pytest.raises(_lib.MiReduceError, match="scale is zero"):
        oneccl_amd.reduce_bcast_mixed_scaled(tf, [oh], 0.0)
    with pytest.raises(_lib.MiReduceError, match=r"outs\[0\] overlaps inputs\[1\]"):
        oneccl_amd.reduce_bcast_mixed_scaled(tf, [tf[1].view(torch.bfloat16)[:N]], 0.5)


# ---- graph capture (as tests/test_gpu_mixed.py) ----------------------------------------------

def _hip():
    """The HIP runtime this process already has loaded."""
    import torch
    torch.cuda.init()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "HIP runtime not loaded"
    return ctypes.CDLL(sorted(paths)[0])


@pytest.mark.parametrize("idt,odt,flags,with_acc", [(BF16, FP32, 0, True), (FP32, BF16, 0xA, False)],
                         ids=["widening-acc-in-place", "narrowing"])
def test_capture_is_one_kernel_node_and_replays(idt, odt, flags, with_acc):
    import torch
    hip = _hip()
    k, m, scale = 3, 2, 1 / 3
    ins = _inputs(idt)[:k]
    dins = [_dev(a) for a in ins]
    eso = 4 if odt == FP32 else 2
    outs = [_filled(eso) for _ in range(m)]
    dacc = None
    if with_acc:
        dacc = _dev(_acc())
        outs[0] = dacc.view(torch.uint8)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = ctypes.c_void_p(stream.cuda_stream)
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(s, 2) == 0  # hipStreamCaptureModeRelaxed
    try:
        call_mixed_scaled([t.data_ptr() for t in dins], idt, [t.data_ptr() for t in outs], odt, N, flags, scale,
                          dacc.data_ptr() if with_acc else None, stream.cuda_stream)
    finally:
        assert hip.hipStreamEndCapture(s, ctypes.byref(graph)) == 0
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    assert n.value == 1, f"{n.value} graph nodes"
    node, kind = ctypes.c_void_p(), ctypes.c_int(-1)
    assert hip.hipGraphGetNodes(graph, ctypes.byref(node), ctypes.byref(n)) == 0
    assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0
    assert kind.value == 0, "not a kernel node"  # hipGraphNodeTypeKernel
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, ctypes.c_size_t(0)) == 0
    try:
        torch.cuda.synchronize()
        for o in outs[1 if with_acc else 0:]:
            assert bool((o == 0x5A).all()), "the capture itself wrote"
        acc = _acc() if with_acc else None
        for rep in range(2):  # the second replay accumulates onto the first one's result
            assert hip.hipGraphLaunch(gexec, s) == 0
            stream.synchronize()
            exp = expected_mixed_scaled(list(ins), idt, odt, flags, scale, acc)
            for o, t in enumerate(outs):
                assert_same(_host(t, _np(odt)), exp, odt, f"replay {rep}: output {o}")
            if with_acc:
                acc = exp
    finally:
        hip.hipGraphExecDestroy(gexec)
        hip.hipGraphDestroy(graph)
