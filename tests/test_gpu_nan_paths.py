"""NaN and Inf bits of mi_reduce_batch, mi_reduce_bcast and
mi_reduce_bcast_scaled, bit for bit, on every kernel path that folds them.

mi_reduce and mi_reduce_multi are pinned to the reference's own vectors
(tests/test_gpu_ref_vectors.py, test_gpu_ref_comp_vectors.py), to the sparse
NaN inputs of tests/test_gpu_nan.py and to the fuzz.  The three entry points
above run kernel text of their own on a NaN row, and their other tests draw
inputs from tests.util.rand_array, whose bf16 / fp16 arrays hold no payload
and no signalling NaN and never two specials at one index.  Here they get the
inputs of tests/nanvec.py: the reference's vectors re-addressed (expected:
the reference's), a dense table of special pairs and the sparse inputs
(expected: tests.guard.oracle_fold, tied to the reference's vectors on the
CPU by tests/test_nanvec.py).  Every comparison is tests.util.assert_same
with NaN payloads; nothing has a tolerance.  Operands are carved out of one
tests.guard.Arena per test, so one check() also shows that every input that
is not an output, and every byte between the operands, is unchanged.

Which kernel text each test reaches (oneccl_amd/csrc/reduce_kernels.hpp; knob =
how the test routes to it):

  reduce2_batch_kernel          test_batch, "common": reduce2_tile's NaN row re-loading its operands, and
  (launch_reduce_batch)         which of a descriptor's operands is the accumulator (the NaN that wins, the
                                sign of a +-0 tie); the 256 one-element descriptors of the reference's
                                scalar path cross kBatchMax = 64 four times; one descriptor has in == inout
  reduce_kernel, elements       test_batch, "one-differs": mi_set_unaligned_vectors(0) and one descriptor's
                                `in` an element off its inout, which leaves the table for a launch of its own
  bcast_kernel<.., 8 / 16>      test_fanout[*-tile]: fan_fold (for fp16 reached through the fan-out only:
                                fan_kernel has that fold written out) with x86_refold; k = 1 through
                                bcast_k1 (the bytes as loaded); head and tail through bcast_elem
  bcast_stride_kernel, tiles    test_fanout[*-stride] (mi_set_max_blocks(1)): its own fold, finish_fold,
                                native_minmax and k = 1 select
  bcast_stride_kernel, elements test_fanout[*-elem] (outputs an element apart): bcast_elem over the count
  bcast_scaled_kernel           test_fanout_scaled[*-tile]: fan_fold under a multiplier, finish_scaled's NaN
                                select on the refolded row, bcast_k1's scaled rule
  bcast_scaled_stride_kernel    test_fanout_scaled[*-stride]: its own fold with finish_scaled<.., true>
  ..., elements                 test_fanout_scaled[*-elem]: bcast_elem's k = 1 scaled rule
  fan_kernel, reduce2_kernel    test_multi_table: the dense table through the kernels the reference's
                                vectors already pin, so that a disagreement above is the new paths', not
                                the oracle's

Each fan-out case runs with separate outputs and with outs[0] == inputs[0]
(on the element loop that output keeps the input's misalignment and the next
one differs); the scaled ones also with outs[i] == inputs[i] for all i at
(2, 2) and (8, 8).  MI_F_BF16_TAIL_TRUNC16 has no oracle: the reference's
keep-precision vectors pin it, and under a multiplier the table's NaN bits
are compared with the GPU's own unscaled call (as tests/test_gpu_scaled.py).

Not run: destinations on a peer GPU (every operand is on one device), element
counts above 2^32, the integer types.
"""
from __future__ import annotations

import numpy as np
import pytest

from oneccl_amd import _lib
from tests import nanvec as nv
from tests.guard import Arena, arena_bytes
from tests.guard import es_of as _es
from tests.nanvec import F_TAIL
from tests.test_gpu_bounds import Knobs, _stream
from tests.test_gpu_scaled import expected_scaled
from tests.util import BF16, FP16, OP_NAME, OPS, assert_same

pytestmark = pytest.mark.gpu

SUM = 0
LP = (BF16, FP16)
PATHS = {"tile": {}, "stride": {"max_blocks": 1}, "elem": {}}
TABLE_KS = [1, 2, 3, 9, 16]
SCALES = [0.5, -2.5, 1 / 3]
SPARSE_N = 4096 + 13
V_IDS = [v[0] for v in nv.VARIANTS]
BF16_ALL = ("bf16-0xf", BF16, 0xF)  # every bf16 bit: the table under a multiplier only (no oracle)


def _mis(dt, head):
    """The misalignment in bytes that leaves `head` scalar elements."""
    return (16 - head * _es(dt)) % 16


def _golden_mis(dt):
    return _mis(dt, min(3, nv.per_vec(dt) - 1))


def _noise(like):
    return np.full(like.nbytes, 0x5A, np.uint8).view(like.dtype)


# ---- the cases of one variant: (label, op, inputs, unscaled fold or None, m, misalignment) ----------

def fold_cases(dt, flags, ops, table=True):
    """(2, 2) the reference's 2-input vectors; (8, 3) its fans; (5, 2) its
    batch and keep-precision vectors; the table at k = 1, 2, 3, 9, 16 and the
    sparse inputs at k = 3, m = 2."""
    out = []
    tmis = _mis(dt, nv.head_tail(dt)[0])
    for op in ops:
        for src, m in ((nv.golden_two_input(), 2), (nv.golden_fans(), 3), (nv.golden_chunks(), 2)):
            for c in nv.golden(src, dt, flags, op):
                out.append((c["key"], op, c["ins"], c["expected"], m, _golden_mis(dt)))
        if not table:
            continue
        for k in TABLE_KS:
            if flags & F_TAIL:  # no oracle: the caller gets the fold from the GPU's unscaled call
                out.append((f"table k={k} {OP_NAME[op]}", op, nv.special_table(dt, k, *nv.head_tail(dt)), None, 2, tmis))
            else:
                ins, exp = nv.table_case(dt, flags, op, k)
                out.append((f"table k={k} {OP_NAME[op]}", op, ins, exp, 2, tmis))
        if dt in LP and not flags & F_TAIL:
            ins, exp = nv.sparse_case(dt, flags, op, 3, SPARSE_N)
            out.append((f"sparse k=3 {OP_NAME[op]}", op, ins, exp, 2, _golden_mis(dt)))
    return out


def place_fanout(ar, tag, dt, ins, m, mis, path, alias):
    """alias: "none", "first" (outs[0] is inputs[0]) or "all" (outs[i] is
    inputs[i], m == k).  On the element loop output o sits o elements past
    the common misalignment (so outs[0] keeps the inputs' and outs[1]
    differs); an input that is an output sits where that output does."""
    es = _es(dt)
    omis = [(mis + (o * es if path == "elem" else 0)) % 16 for o in range(m)]
    aliased = {"none": 0, "first": 1, "all": m}[alias]
    assert aliased <= len(ins)
    pin = [ar.place(x, omis[j] if j < aliased else mis, "inout" if j < aliased else "in", f"{tag}.in{j}")
           for j, x in enumerate(ins)]
    pout = [pin[o] if o < aliased else ar.place(_noise(ins[0]), omis[o], "out", f"{tag}.out{o}") for o in range(m)]
    if path == "elem":
        assert len({p.ptr % 16 for p in pout}) > 1
    return pin, pout


def run_fanout(dt, flags, runs, path, what):
    """runs: (label, op, inputs, expected, m, misalignment, alias, scale or
    None).  One arena, every launch under the path's knobs, one check() of
    the arena, then all m outputs of every run against `expected`."""
    import torch
    es = _es(dt)
    nops = sum(len(r[2]) + r[4] for r in runs)
    ar = Arena(arena_bytes(sum((len(r[2]) + r[4]) * r[2][0].size * es for r in runs), nops), "device", seed=len(runs))
    placed = [place_fanout(ar, f"r{i}", dt, r[2], r[4], r[5], path, r[6]) for i, r in enumerate(runs)]
    ar.snapshot()
    m_ = _lib.mi()
    with Knobs(**PATHS[path]):
        for (label, op, ins, exp, m, mis, alias, scale), (pin, pout) in zip(runs, placed):
            pi, po = _lib.void_ptr_array([p.ptr for p in pin]), _lib.void_ptr_array([p.ptr for p in pout])
            if scale is None:
                _lib.check(m_.mi_reduce_bcast(pi, len(pin), po, m, ins[0].size, dt, op, flags, _stream()),
                           "mi_reduce_bcast")
            else:
                _lib.check(m_.mi_reduce_bcast_scaled(pi, len(pin), po, m, ins[0].size, dt, op, flags, scale,
                                                     _stream()), "mi_reduce_bcast_scaled")
        torch.cuda.synchronize()
    ar.check(what=what)  # bounds, and every input that is not an output unchanged
    for (label, op, ins, exp, m, mis, alias, scale), (pin, pout) in zip(runs, placed):
        for o, p in enumerate(pout):
            assert_same(ar.read(p), exp, dt, f"{what}: {label}, k={len(ins)} m={m} alias={alias} scale={scale!r}, "
                                             f"output {o}")


# ---- mi_reduce_bcast ---------------------------------------------------------------------------

FANOUT_VARIANTS = nv.VARIANTS + [nv.KEEP_TAIL]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name,dt,flags", FANOUT_VARIANTS, ids=[v[0] for v in FANOUT_VARIANTS])
def test_fanout(name, dt, flags, path):
    """Every op; each case with separate outputs and with outs[0] ==
    inputs[0].  The keep-precision variant with the truncated tail has the
    reference's vectors only."""
    cases = fold_cases(dt, flags, OPS, table=not flags & F_TAIL)
    assert cases
    runs = [(label, op, ins, exp, m, mis, alias, None) for label, op, ins, exp, m, mis in cases
            for alias in ("none", "first")]
    run_fanout(dt, flags, runs, path, f"mi_reduce_bcast {name} {path}")


# ---- mi_reduce_bcast_scaled --------------------------------------------------------------------

_scaled_cache = {}


def _scaled_expected(name, label, ins, dt, flags, scale, F):
    key = (name, label, scale)
    if key not in _scaled_cache:
        _scaled_cache[key] = expected_scaled(ins, dt, flags, scale, unscaled=F)
    return _scaled_cache[key]


def _gpu_unscaled(dt, flags, cases):
    """The GPU's unscaled fold of each case through m = 1 (mi_reduce_multi's
    kernels), for the variant the oracle does not model."""
    import torch
    from tests.util import from_dev, to_dev
    out = []
    for label, op, ins, F, m, mis in cases:
        holders = [to_dev(np.ascontiguousarray(x)) for x in ins]
        t, p = to_dev(_noise(ins[0]))
        _lib.check(_lib.mi().mi_reduce_bcast(_lib.void_ptr_array([q for _, q in holders]), len(ins),
                                             _lib.void_ptr_array([p]), 1, ins[0].size, dt, op, flags, _stream()))
        torch.cuda.synchronize()
        out.append(from_dev(t, ins[0]))
    return out


SCALED_VARIANTS = FANOUT_VARIANTS + [BF16_ALL]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name,dt,flags", SCALED_VARIANTS, ids=[v[0] for v in SCALED_VARIANTS])
def test_fanout_scaled(name, dt, flags, path):
    """Sum under 0.5, -2.5 and 1/3: +-inf and +-0 with the product's sign,
    every NaN as the unscaled call stores it (for k = 1 in storage precision
    as loaded, a signalling one still signalling); separate outputs, outs[0]
    == inputs[0], and outs[i] == inputs[i] for all i at (2, 2) and (8, 8)."""
    cases = fold_cases(dt, flags, [SUM], table=flags != nv.KEEP_TAIL[2])
    assert cases
    if flags == BF16_ALL[2]:
        assert all(F is None for _, _, _, F, _, _ in cases)
        folds = _gpu_unscaled(dt, flags, cases)
        cases = [c[:3] + (F,) + c[4:] for c, F in zip(cases, folds)]
    runs = []
    for label, op, ins, F, m, mis in cases:
        for scale in SCALES:
            exp = _scaled_expected(name, label, ins, dt, flags, scale, F)
            runs += [(label, op, ins, exp, m, mis, alias, scale) for alias in ("none", "first")]
            if len(ins) in (2, 8) and not label.startswith("sparse"):
                runs.append((label, op, ins, exp, len(ins), mis, "all", scale))
    run_fanout(dt, flags, runs, path, f"mi_reduce_bcast_scaled {name} {path}")


# ---- mi_reduce_batch ----------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
@pytest.mark.parametrize("name,dt,flags", nv.VARIANTS, ids=V_IDS)
def test_batch(name, dt, flags, op):
    """One call holding the reference's 2-input vectors of this (dtype, impl,
    op) at their counts (its 256 one-element calls as 256 descriptors), the
    table, the table's second input with in == inout, and the sparse inputs:
    at one misalignment per descriptor (the batch kernel), then with the
    table's `in` an element off under mi_set_unaligned_vectors(0) (that
    descriptor leaves for the element loop)."""
    import torch
    es, per = _es(dt), nv.per_vec(dt)
    descs = []  # (label, inout, in or None for in == inout, expected, misalignment)
    for c in nv.golden(nv.golden_two_input(), dt, flags, op):
        b, a = c["ins"]
        if c.get("calls"):
            descs += [(f"{c['key']}[{i}]", b[i:i + 1], a[i:i + 1], c["expected"][i:i + 1], (i % per) * es)
                      for i in range(c["calls"])]
        else:
            descs.append((c["key"], b, a, c["expected"], _golden_mis(dt)))
    (t0, t1), texp = nv.table_case(dt, flags, op, 2)
    table_at = len(descs)
    tmis = _mis(dt, nv.head_tail(dt)[0])
    descs.append(("table", t0, t1, texp, tmis))
    descs.append(("table, in == inout", t1, None, nv.fold([t1, t1], dt, op, flags), tmis))
    if dt in LP:
        for n in (5, 61, SPARSE_N):
            (s0, s1), sexp = nv.sparse_case(dt, flags, op, 2, n)
            descs.append((f"sparse n={n}", s0, s1, sexp, _golden_mis(dt)))
    if dt not in LP:
        assert len(descs) > 4 * 64
    for run, knobs in (("common", {}), ("one-differs", {"unaligned": 0})):
        ar = Arena(arena_bytes(2 * sum(d[1].nbytes for d in descs), 2 * len(descs)), "device", seed=op)
        placed = []
        for i, (label, inout, in_, exp, mis) in enumerate(descs):
            pio = ar.place(inout, mis, "inout", f"d{i}.inout")
            off = es if (run == "one-differs" and i == table_at) else 0
            pin = pio if in_ is None else ar.place(in_, (mis + off) % 16, "in", f"d{i}.in")
            placed.append((pin, pio))
        ar.snapshot()
        with Knobs(**knobs):
            arr = _lib.desc_array([(pin.ptr, pio.ptr, d[1].size) for d, (pin, pio) in zip(descs, placed)])
            _lib.check(_lib.mi().mi_reduce_batch(arr, len(descs), dt, op, flags, _stream()), "mi_reduce_batch")
            torch.cuda.synchronize()
        ar.check(what=f"mi_reduce_batch {name} {run}")  # bounds, and every `in` unchanged
        for (label, inout, in_, exp, mis), (pin, pio) in zip(descs, placed):
            assert_same(ar.read(pio), exp, dt, f"mi_reduce_batch {name} {OP_NAME[op]} {run}: {label}")


# ---- mi_reduce_multi with the table ---------------------------------------------------------------

MULTI_VARIANTS = [v for v in nv.VARIANTS if v[0] in ("fp16-0x1", "fp16-0x11", "bf16-0x3", "fp32", "fp64")]


@pytest.mark.parametrize("name,dt,flags", MULTI_VARIANTS, ids=[v[0] for v in MULTI_VARIANTS])
def test_multi_table(name, dt, flags):
    """The dense table through the lean 2-input kernel and the fan kernel,
    which the reference's vectors pin: the oracle and the pinned kernels
    agree on it."""
    import torch
    assert len(MULTI_VARIANTS) == 5
    tmis = _mis(dt, nv.head_tail(dt)[0])
    cases = [(op, k) + nv.table_case(dt, flags, op, k) for op in OPS for k in (2, 3, 9, 16)]
    ar = Arena(arena_bytes(sum((k + 1) * exp.nbytes for _, k, _, exp in cases), sum(k + 1 for _, k, _, _ in cases)),
               "device", seed=dt)
    placed = []
    for i, (op, k, ins, exp) in enumerate(cases):
        pin = [ar.place(x, tmis, "in", f"c{i}.in{j}") for j, x in enumerate(ins)]
        placed.append((pin, ar.place(_noise(exp), tmis, "out", f"c{i}.out")))
    ar.snapshot()
    for (op, k, ins, exp), (pin, pout) in zip(cases, placed):
        _lib.check(_lib.mi().mi_reduce_multi(_lib.void_ptr_array([p.ptr for p in pin]), k, pout.ptr, exp.size, dt, op,
                                             flags, _stream()), "mi_reduce_multi")
    torch.cuda.synchronize()
    ar.check(what=f"mi_reduce_multi {name}")
    for (op, k, ins, exp), (pin, pout) in zip(cases, placed):
        assert_same(ar.read(pout), exp, dt, f"mi_reduce_multi {name} {OP_NAME[op]} k={k}")
