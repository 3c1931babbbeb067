"""mi_reduce_bcast writes its m outputs, all of each and nothing else.

The arena method of tests/test_gpu_bounds.py: many cases carved out of one
guarded Arena (tests/guard.py), one snapshot, every launch, one check() of
the whole arena, then every output compared bit for bit with the oracle's
fold (tests.guard.oracle_fold, tests.util.assert_same; no tolerance
anywhere).  Shapes are the tile edges: bodies of 0, 1, T-1, T, T+1 and 2T+1
16-byte vectors crossed with scalar heads and tails of 0, 1 and 16/es - 1
elements, and one element at misalignment es.

An output that is exactly one of the inputs (in place) is placed as that
input with role "inout"; its guards are drawn so that a spilling lane's
load-fold-store of the neighbouring bytes would change them (bcast_guards).
Separate outputs reuse the output guard pair of reduce_guards.

Who guards what (the rows tests/guard.py's table would hold for the kernels
of mi_reduce_bcast; knob = how the test routes to it):

  bcast_kernel<.., 8 / 16>      test_tile_kernel (k <= 8 / k > 8, all outputs separate; k = 1 the pure
                                fan-out), test_tile_kernel_in_place (outs[i] == inputs[i]; outs[0] ==
                                inputs[2]), test_tile_kernel_fp32_accumulate
  bcast_stride_kernel, tiles    test_stride_kernel_under_grid_cap (mi_set_max_blocks(1), (3))
  bcast_stride_kernel, elements test_element_loop_outputs_differ (outputs at differing misalignments),
                                test_element_loop_inputs_differ (mi_set_unaligned_vectors(0)),
                                test_element_loop_byte_misaligned_fp32 (odd byte offsets)
  unaligned vector loads        test_unaligned_vector_loads (mi_set_unaligned_vectors(1), inputs at their
                                own misalignments, outputs at one)
  m = 1 -> mi_reduce_multi      test_one_output_is_reduce_multi (fan_kernel: tests/test_gpu_bounds.py)
  bucket layout                 test_touching_outputs_in_one_bucket
  any path, random shapes       test_fuzz (aliased outputs among them)

Destinations on a peer GPU have not been run: every operand here is on one
device.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from oneccl_amd import _lib
from oneccl_amd.comp import F_ACC_FP32, F_BF16_RNE, F_MINMAX_INOUT_FIRST
from tests.guard import (DT_OP, DT_OP_IDS, GUARD, T_GENERAL, T_LEAN, Arena, _bits, arena_bytes,
                         guard_conditions, oracle_fold, reduce_guards)
from tests.guard import es_of as _es
from tests.guard import ref_flags as _flags
from tests.guard import tile_shapes as shapes
from tests.test_gpu_bounds import Knobs, _stream
from tests.util import ALL_DTYPES, BF16, FP16, FP32, assert_same, rand_array

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=256)
def bcast_guards(dt, op, k, n, flags, aliased):
    """reduce_guards' out-of-place guards (before, after), redrawn where the
    guard of an aliased input (`aliased`: the inputs that are also outputs)
    equals zero or the fold of zeros (what a lane past the end that loaded
    zeros would store into every output), or where the guards of all aliased
    inputs equal the fold of the inputs' guards (what a lane that got through
    in place would store into every output: a min or max is always one of its
    operands, so one guard that differs is all that can be asked; for k = 1
    the fold is the identity and nothing can)."""
    sides = []
    zeros_fold = _bits(oracle_fold([np.zeros(n, oracle.NP_DTYPE[dt]) for _ in range(k)], dt, op, flags))
    for side, (ing, out) in enumerate(reduce_guards(dt, op, k, n, flags, False)):
        ing, out = [g.copy() for g in ing], out.copy()
        for r in range(64):
            # each array is redrawn only where it is itself at fault (small integer products draw a
            # zero one time in seven: redrawing all 16 guards of a position together would not settle)
            bad = {k: guard_conditions(ing, out, dt, op, flags, False)}  # index k: the separate outputs' guard
            for j in aliased:
                bad[j] = (_bits(ing[j]) == 0) | (_bits(ing[j]) == zeros_fold)
            if aliased and k > 1:
                fold = _bits(oracle_fold(ing, dt, op, flags))
                all_equal = np.logical_and.reduce([_bits(ing[j]) == fold for j in aliased])
                for j in range(k):  # the fold is every input's business
                    bad[j] = bad.get(j, False) | all_equal
            if not any(b.any() for b in bad.values()):
                break
            for j, b in bad.items():
                fresh = rand_array(dt, n, seed=((side + 3) * 131 + j) * 97 + r, op=op, specials=False)
                (ing[j] if j < k else out)[b] = fresh[b]
        else:
            raise AssertionError(f"bcast_guards did not converge: dtype {dt} op {op} k {k} aliased {aliased}")
        sides.append((ing, out))
    return sides


def case(dt, op, k, m, n, in_mis=0, out_mis=0, alias=None, flags=None):
    """in_mis / out_mis: one misalignment for all, or one per operand.
    alias: {output index: input index} for outputs that are that input."""
    flags = _flags(dt) if flags is None else flags
    in_mis = [in_mis] * k if isinstance(in_mis, int) else list(in_mis)
    out_mis = [out_mis] * m if isinstance(out_mis, int) else list(out_mis)
    return (dt, op, flags, k, m, n, in_mis, out_mis, dict(alias or {}))


def place_bcast(ar, i, c, seed):
    dt, op, flags, k, m, n, in_mis, out_mis, alias = c
    es = _es(dt)
    out_of = {j: o for o, j in alias.items()}
    assert len(out_of) == len(alias), "two outputs on one input would overlap"
    (gb_in, gb_out), (ga_in, ga_out) = bcast_guards(dt, op, k, GUARD // es, flags, tuple(sorted(out_of)))
    ins = [rand_array(dt, n, seed=1000 * seed + 37 * i + j, op=op) for j in range(k)]
    pin = [ar.place(x, out_mis[out_of[j]] if j in out_of else in_mis[j], "inout" if j in out_of else "in",
                    f"c{i}.in{j}", (gb_in[j], ga_in[j])) for j, x in enumerate(ins)]
    pout = []
    for o in range(m):
        if o in alias:
            pout.append(pin[alias[o]])
        else:  # starts as non-zero noise of the dtype
            noise = rand_array(dt, n, seed=7000 + 1000 * seed + 37 * i + o, op=op, specials=False)
            pout.append(ar.place(noise, out_mis[o], "out", f"c{i}.out{o}", (gb_out, ga_out)))
    return pin, pout, (oracle_fold(ins, dt, op, flags) if n else None)


def launch(c, pin, pout):
    dt, op, flags, k, m, n = c[:6]
    _lib.check(_lib.mi().mi_reduce_bcast(_lib.void_ptr_array([p.ptr for p in pin]), k,
                                         _lib.void_ptr_array([p.ptr for p in pout]), m, n, dt, op, flags, _stream()),
               "mi_reduce_bcast")


def run_bcasts(cases, what, seed=0, **knobs):
    import torch
    nops = sum(c[3] + c[4] - len(c[8]) for c in cases)
    total = sum((c[3] + c[4] - len(c[8])) * c[5] * _es(c[0]) for c in cases)
    ar = Arena(arena_bytes(total, nops), "device", seed=seed)
    placed = [place_bcast(ar, i, c, seed) for i, c in enumerate(cases)]
    ar.snapshot()
    with Knobs(**knobs):
        for c, (pin, pout, _) in zip(cases, placed):
            launch(c, pin, pout)
        torch.cuda.synchronize()
    ar.check(what=what)
    for c, (pin, pout, exp) in zip(cases, placed):
        if exp is None:
            continue
        for o, p in enumerate(pout):
            assert_same(ar.read(p), exp, c[0], f"{what}: output {o} of case (dt, op, flags, k, m, count, in_mis, "
                                               f"out_mis, alias) = {c}")


def _common(dt, op, k, m, T, alias=None, flags=None):
    return [case(dt, op, k, m, n, mis, mis, alias, flags) for n, mis in shapes(_es(dt), T)]


# ---- bcast_kernel<.., 8> / <.., 16> --------------------------------------------------

KM = [(2, 2), (3, 5), (8, 8), (9, 16), (16, 2), (1, 3)]


@pytest.mark.parametrize("k,m", KM, ids=[f"k{k}-m{m}" for k, m in KM])
@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_tile_kernel(dt, op, k, m):
    """All outputs separate, every operand at the outputs' misalignment: 8
    input slots (k <= 8) and 16, the packed integer fold and the widened one,
    the m-iteration store loop; k = 1 is the pure fan-out."""
    run_bcasts(_common(dt, op, k, m, T_LEAN), f"bcast_kernel k={k} m={m}", seed=dt * 4 + op)


@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_tile_kernel_in_place(dt, op):
    """outs[i] == inputs[i] for all i (the one-shot allreduce) at (2, 2),
    (8, 8), (9, 9); at (3, 5) outs[0] == inputs[2] and the rest separate."""
    cases = []
    for k in (2, 8, 9):
        cases += _common(dt, op, k, k, T_LEAN, {i: i for i in range(k)})
    cases += _common(dt, op, 3, 5, T_LEAN, {0: 2})
    run_bcasts(cases, "bcast_kernel in place", seed=100 + dt * 4 + op)


@pytest.mark.parametrize("dt,flags", [(BF16, F_ACC_FP32), (BF16, F_ACC_FP32 | F_BF16_RNE | F_MINMAX_INOUT_FIRST),
                                      (FP16, F_ACC_FP32 | F_MINMAX_INOUT_FIRST)],
                         ids=["bf16-acc32-trunc", "bf16-acc32-rne", "fp16-acc32"])
def test_tile_kernel_fp32_accumulate(dt, flags):
    cases = []
    for (k, m), op in (((3, 2), 0), ((9, 3), 3)):
        cases += _common(dt, op, k, m, T_LEAN, None, flags)
        cases += _common(dt, op, k, m, T_LEAN, {0: 0}, flags)
    run_bcasts(cases, "bcast_kernel fp32-accumulate", seed=200 + dt)


# ---- m = 1 ---------------------------------------------------------------------------

def test_one_output_is_reduce_multi():
    """(5, 1): byte for byte what mi_reduce_multi writes (and the oracle's fold)."""
    import torch
    k = 5
    for dt, op in ((FP32, 0), (BF16, 3), (FP16, 1), (0, 2)):
        es, flags = _es(dt), _flags(dt)
        shp = shapes(es, T_LEAN)
        ar = Arena(arena_bytes(sum(n for n, _ in shp) * es * (k + 2), len(shp) * (k + 2)), "device", seed=dt)
        placed = []
        for i, (n, mis) in enumerate(shp):
            c = case(dt, op, k, 2, n, mis, mis)  # two separate outputs placed: one per entry point
            placed.append((c, *place_bcast(ar, i, c, 300 + dt)))
        ar.snapshot()
        for c, pin, pout, _ in placed:
            arr = _lib.void_ptr_array([p.ptr for p in pin])
            _lib.check(_lib.mi().mi_reduce_bcast(arr, k, _lib.void_ptr_array([pout[0].ptr]), 1, c[5], dt, op, flags,
                                                 _stream()), "mi_reduce_bcast")
            _lib.check(_lib.mi().mi_reduce_multi(arr, k, pout[1].ptr, c[5], dt, op, flags, _stream()))
        torch.cuda.synchronize()
        ar.check(what="m = 1")
        for c, pin, pout, exp in placed:
            if exp is not None:
                got = ar.read(pout[0])
                assert np.array_equal(got.view(np.uint8), ar.read(pout[1]).view(np.uint8)), f"case {c}"
                assert_same(got, exp, dt, f"m = 1, case {c}")


# ---- bcast_stride_kernel: tiles under a grid cap ----------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_stride_kernel_under_grid_cap(dt, op, cap):
    """mi_set_max_blocks(1) / (3): one or three blocks stride over the tiles
    and end in the partial one; (2, 2) in place and (3, 4) separate."""
    cases = _common(dt, op, 2, 2, T_GENERAL, {0: 0, 1: 1}) + _common(dt, op, 3, 4, T_GENERAL)
    run_bcasts(cases, f"bcast_stride_kernel max_blocks={cap}", seed=400 + dt, max_blocks=cap)


# ---- operands at differing misalignments ------------------------------------------------

def _differing(dt, op, k, m, T, ins_differ, outs_differ, alias=None):
    """Inputs and / or outputs at misalignments that differ from shape to
    shape and from operand to operand, by whole elements."""
    es = _es(dt)
    per = 16 // es
    out = []
    for i, (n, mis) in enumerate(shapes(es, T)):
        im = [((mis // es + 1 + j + i) % per) * es for j in range(k)] if ins_differ else [mis] * k
        om = [((mis // es + 2 * o + i) % per) * es for o in range(m)] if outs_differ else [mis] * m
        if ins_differ and all(x == mis for x in im):
            im[-1] = (mis + es) % 16
        if outs_differ and len(set(om)) == 1:
            om[-1] = (om[0] + es) % 16
        out.append(case(dt, op, k, m, n, im, om, alias))
    return out


@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_element_loop_outputs_differ(dt, op):
    """Outputs at differing misalignments have no common vector grid: the
    element loop, whatever mi_set_unaligned_vectors says; (2, 2) with
    outs[1] == inputs[0] and (5, 3)."""
    cases = _differing(dt, op, 2, 2, T_LEAN, False, True, {1: 0}) + _differing(dt, op, 5, 3, T_LEAN, True, True)
    run_bcasts(cases, "element loop, outputs differ", seed=500 + dt, unaligned=1)


@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_element_loop_inputs_differ(dt, op):
    """mi_set_unaligned_vectors(0) with inputs off the outputs' grid."""
    cases = _differing(dt, op, 2, 2, T_LEAN, True, False) + _differing(dt, op, 5, 3, T_LEAN, True, False, {2: 4})
    run_bcasts(cases, "element loop, inputs differ", seed=600 + dt, unaligned=0)


@pytest.mark.parametrize("dt,op", DT_OP, ids=DT_OP_IDS)
def test_unaligned_vector_loads(dt, op):
    """mi_set_unaligned_vectors(1): the tile kernel on the outputs' common
    grid with each input at its own misalignment (an input that is an output
    sits on the grid); (2, 2) and (5, 3)."""
    cases = _differing(dt, op, 2, 2, T_LEAN, True, False) + _differing(dt, op, 5, 3, T_LEAN, True, False, {2: 4})
    run_bcasts(cases, "unaligned vector loads", seed=700 + dt, unaligned=1)


def test_element_loop_byte_misaligned_fp32():
    """fp32 operands at odd byte offsets are not element-aligned: the element
    loop under either setting of the knob."""
    for unaligned in (0, 1):
        cases = []
        for n in (1, 3, 255, 257, 4 * T_LEAN + 1):
            for im, om in (([1, 1], [1, 1]), ([1, 3], [7, 7]), ([0, 5], [0, 0]), ([2, 0], [15, 3])):
                for op in (0, 3):
                    cases.append(case(FP32, op, 2, 2, n, im, om, flags=0))
        run_bcasts(cases, f"element loop, byte-misaligned fp32, unaligned={unaligned}", seed=800 + unaligned,
                   unaligned=unaligned)


# ---- workload shape: the outputs are touching chunks of one bucket ---------------------------

@pytest.mark.parametrize("op", [0, 3], ids=["sum", "max"])
@pytest.mark.parametrize("dt", [FP32, BF16, 0], ids=["f32", "bf16", "i8"])
def test_touching_outputs_in_one_bucket(dt, op):
    """Three outputs that are the touching thirds of one bucket, of odd counts
    (so they sit at three misalignments: the element loop) and of a count that
    keeps them on one grid (the tile kernel).  A spill from one lands in its
    neighbour, so the whole bucket is compared; its outer guards stay."""
    import torch
    es, flags, k, m = _es(dt), _flags(dt), 2, 3
    for n in (1, 77, 1025, 2049, 16 * (T_LEAN + 1)):
        ins = [rand_array(dt, n, seed=900 + j + n, op=op) for j in range(k)]
        (gb_in, gb_out), (ga_in, ga_out) = reduce_guards(dt, op, k, GUARD // es, flags, False)
        ar = Arena(arena_bytes((k + m) * n * es, k + 1), "device", seed=n + dt)
        pin = [ar.place(x, es * j % 16, "in", f"in{j}", (gb_in[j], ga_in[j])) for j, x in enumerate(ins)]
        bucket = ar.place(rand_array(dt, m * n, seed=77, op=op, specials=False), 0, "out", "bucket", (gb_out, ga_out))
        subs = [ar.sub(bucket, o * n, n, "out", f"chunk{o}") for o in range(m)]
        ar.snapshot()
        # the middle chunk first in the list: the order of outs[] is the caller's
        order = [1, 0, 2]
        _lib.check(_lib.mi().mi_reduce_bcast(_lib.void_ptr_array([p.ptr for p in pin]), k,
                                             _lib.void_ptr_array([subs[o].ptr for o in order]), m, n, dt, op, flags,
                                             _stream()), "mi_reduce_bcast")
        torch.cuda.synchronize()
        ar.check(what=f"touching outputs n={n}")
        exp = oracle_fold(ins, dt, op, flags)
        assert_same(ar.read(bucket), np.concatenate([exp] * m), dt, f"whole bucket, n={n}")


# ---- fuzz ------------------------------------------------------------------------------------

def test_fuzz():
    """About 200 seeded cases in four arenas: k, m <= 16, count <= 5000, any
    dtype and op under the reference flags, element-aligned misalignments
    (half the cases with the outputs on one grid, so both the tile kernel and
    the element loop run), a random subset of the outputs being inputs."""
    rng = np.random.default_rng(20240611)
    for batch in range(4):
        cases = []
        for _ in range(50):
            dt = int(rng.choice(ALL_DTYPES))
            op = int(rng.integers(0, 4))
            es = _es(dt)
            per = 16 // es
            k, m = int(rng.integers(1, 17)), int(rng.integers(1, 17))
            n = int(rng.choice([rng.integers(1, 64), rng.integers(1, 5001)]))
            im = [int(rng.integers(0, per)) * es for _ in range(k)]
            if rng.random() < 0.5:
                om = [int(rng.integers(0, per)) * es] * m
            else:
                om = [int(rng.integers(0, per)) * es for _ in range(m)]
            na = int(rng.integers(0, min(k, m) + 1)) if rng.random() < 0.6 else 0
            alias = dict(zip(rng.permutation(m)[:na].tolist(), rng.permutation(k)[:na].tolist()))
            cases.append(case(dt, op, k, m, n, im, om, alias))
        run_bcasts(cases, f"fuzz batch {batch}", seed=1000 + batch)
