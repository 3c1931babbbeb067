"""mi_reduce_bcast_mixed on the GPU: every output bit for bit the composition
the header defines (tests.mixed.expected_mixed: the oracle's fp32 fold of the
oracle's conversions, or the oracle's conversion of its fp32 fold), and byte
for byte what the GPU's own two-step sequence leaves (mi_convert x K into
scratch buffers and an fp32 mi_reduce_bcast; mi_reduce_multi into an fp32
scratch buffer and mi_convert x M).  All four dtype pairs, each narrowing
variant, widening with and without an accumulator and with the accumulator in
place.  Bounds and tile edges are tests/test_gpu_mixed_bounds.py's, the dense
NaN table tests/test_gpu_mixed_nan.py's."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import oneccl_amd
from oneccl_amd import _lib
from tests.mixed import NARROWING, PAIR_IDS, PAIRS, SUM, WIDENING, call_mixed, expected_mixed
from tests.util import BF16, FP16, FP32, assert_same, rand_array

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 5  # > 40: rand_array's specials are present
KM = [(1, 1), (1, 3), (2, 1), (2, 2), (3, 16), (8, 3), (9, 2), (16, 3)]
_SIGNED = {2: np.int16, 4: np.int32}


@functools.lru_cache(maxsize=None)
def _inputs(dt):
    """16 inputs of dtype dt and an accumulator, drawn once; never changed."""
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


def _sequence(dins, idt, odt, flags, k, m, dacc):
    """The sequence the fused call replaces, from calls that exist without it;
    returns its m outputs."""
    import torch
    mi, s = _lib.mi(), _stream()
    eso = 4 if odt == FP32 else 2
    outs = [_filled(eso) for _ in range(m)]
    if odt == FP32:
        scratch = [torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(k)]
        for x, c in zip(dins[:k], scratch):
            _lib.check(mi.mi_convert(x.data_ptr(), idt, c.data_ptr(), FP32, N, 0, s), "mi_convert")
        lst = ([dacc] if dacc is not None else []) + scratch
        _lib.check(mi.mi_reduce_bcast(_lib.void_ptr_array([t.data_ptr() for t in lst]), len(lst),
                                      _lib.void_ptr_array([t.data_ptr() for t in outs]), m, N, FP32, SUM, 0, s),
                   "mi_reduce_bcast")
    else:
        f = torch.empty(N, dtype=torch.int32, device="cuda")
        _lib.check(mi.mi_reduce_multi(_lib.void_ptr_array([t.data_ptr() for t in dins[:k]]), k, f.data_ptr(), N, FP32,
                                      SUM, 0, s), "mi_reduce_multi")
        for o in outs:
            _lib.check(mi.mi_convert(f.data_ptr(), FP32, o.data_ptr(), odt, N, flags, s), "mi_convert")
    return outs


def _run(idt, odt, flags, acc_mode):
    """acc_mode: None, "separate" or "inplace" (acc == outs[0])."""
    import torch
    ins = _inputs(idt)
    dins = [_dev(a) for a in ins]
    eso = 4 if odt == FP32 else 2
    for k, m in KM:
        if acc_mode and k > 15:
            k = 15
        acc = _acc() if acc_mode else None
        what = f"{idt}->{odt} flags {flags:#x} k={k} m={m} acc={acc_mode}"
        outs = [_filled(eso) for _ in range(m)]
        dacc = None
        if acc_mode == "separate":
            dacc = _dev(acc)
        elif acc_mode == "inplace":
            dacc = _dev(acc)
            outs[0] = dacc.view(torch.uint8)
        call_mixed([t.data_ptr() for t in dins[:k]], idt, [t.data_ptr() for t in outs], odt, N, flags,
                   dacc.data_ptr() if dacc is not None else None, _stream())
        seq = _sequence(dins, idt, odt, flags, k, m, _dev(acc) if acc_mode else None)
        torch.cuda.synchronize()
        exp = expected_mixed(list(ins[:k]), idt, odt, flags, acc)
        for o, t in enumerate(outs):
            assert_same(_host(t, _np(odt)), exp, odt, f"{what}: output {o}")
            assert torch.equal(t, seq[o]), f"{what}: output {o} differs from the two-step sequence's"
        if acc_mode == "separate":
            assert_same(_host(dacc, np.float32), acc, FP32, f"{what}: acc changed")
    for j, (t, a) in enumerate(zip(dins, ins)):
        assert_same(_host(t, _np(idt)), a, idt, f"{idt}->{odt}: inputs[{j}] changed")


@pytest.mark.parametrize("idt,odt,flags", NARROWING, ids=PAIR_IDS[2:])
def test_narrowing(idt, odt, flags):
    _run(idt, odt, flags, None)


@pytest.mark.parametrize("acc_mode", [None, "separate", "inplace"], ids=["no-acc", "acc", "acc-in-place"])
@pytest.mark.parametrize("idt,odt,flags", WIDENING, ids=PAIR_IDS[:2])
def test_widening(idt, odt, flags, acc_mode):
    _run(idt, odt, flags, acc_mode)


@pytest.mark.parametrize("idt,odt", [(BF16, FP32), (FP16, FP32)], ids=["bf16", "fp16"])
def test_flags_change_no_bit_when_widening(idt, odt):
    import torch
    ins = _inputs(idt)
    dins = [_dev(a) for a in ins[:3]]
    exp = expected_mixed(list(ins[:3]), idt, odt, 0)
    for flags in (0x1, 0x2, 0x4, 0x8, 0xF, 0x1F):
        out = _filled(4)
        call_mixed([t.data_ptr() for t in dins], idt, [out.data_ptr()], odt, N, flags, None, _stream())
        torch.cuda.synchronize()
        assert_same(_host(out, np.float32), exp, FP32, f"flags {flags:#x}")


def test_wrapper():
    """oneccl_amd.reduce_bcast_mixed: dtypes from the tensors, flags=None the
    reference's (bf16: round to nearest even), acc in place."""
    import torch
    b = _inputs(BF16)[:3]
    tb = [_dev(a).view(torch.bfloat16) for a in b]
    acc = _dev(_acc()).view(torch.float32)
    other = torch.zeros(N, dtype=torch.float32, device="cuda")
    oneccl_amd.reduce_bcast_mixed(tb, [acc, other], acc=acc)
    f = _inputs(FP32)[:4]
    tf = [_dev(a).view(torch.float32) for a in f]
    ob = [torch.zeros(N, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    oh = torch.zeros(N, dtype=torch.float16, device="cuda")
    oneccl_amd.reduce_bcast_mixed(tf, ob)
    oneccl_amd.reduce_bcast_mixed(tf, [oh])
    oneccl_amd.reduce_bcast_mixed(tf, [ob[1]], flags=0)  # truncation
    torch.cuda.synchronize()
    e = expected_mixed(list(b), BF16, FP32, 0, _acc())
    assert_same(_host(acc.view(torch.int32), np.float32), e, FP32, "acc in place")
    assert_same(_host(other.view(torch.int32), np.float32), e, FP32, "second output")
    assert_same(_host(ob[0].view(torch.int16), np.uint16), expected_mixed(list(f), FP32, BF16, 0x2), BF16, "bf16 rne")
    assert_same(_host(ob[1].view(torch.int16), np.uint16), expected_mixed(list(f), FP32, BF16, 0), BF16, "bf16 trunc")
    assert_same(_host(oh.view(torch.int16), np.uint16), expected_mixed(list(f), FP32, FP16, 0), FP16, "fp16")
    with pytest.raises(_lib.MiReduceError, match=r"outs\[0\] overlaps inputs\[1\]"):
        oneccl_amd.reduce_bcast_mixed(tf, [tf[1].view(torch.bfloat16)[:N]])  # the first half of an input's bytes


# ---- graph capture --------------------------------------------------------------------------

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
    k, m = 3, 2
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
        call_mixed([t.data_ptr() for t in dins], idt, [t.data_ptr() for t in outs], odt, N, flags,
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
            exp = expected_mixed(list(ins), idt, odt, flags, acc)
            for o, t in enumerate(outs):
                assert_same(_host(t, _np(odt)), exp, odt, f"replay {rep}: output {o}")
            if with_acc:
                acc = exp
    finally:
        hip.hipGraphExecDestroy(gexec)
        hip.hipGraphDestroy(graph)
