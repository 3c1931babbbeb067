"""mi_reduce_bcast_mixed_scaled writes its m outputs, all of each and nothing
else, at scale 1/3.

The arena method, the guard-element scheme, the misalignments and the three
routes are tests/test_gpu_mixed_bounds.py's (its case(), on_grid() and the
module docstring): many cases carved out of one guarded arena, one snapshot,
every launch, one check() of the whole arena, then every output compared bit
for bit with tests.mixed_scaled.expected_mixed_scaled.  The guards are drawn
against the scaled composition: an output-side guard differs from zero and from
what a spilling lane would store there, an in-place accumulator's from zero and
from the composition of the guards.

Counts: 1, 7 and 8 (no body group, the scalar path alone; one group), 511, 512
and 513 around one 512-element tile (tests.mixed.T_GROUPS * 8), and 1024 + 5
(two tiles and a partial one), each at scalar heads of 0, 1 and 16 / es_out - 1
elements.

  mixed_scaled_kernel<.., 8 / 16>        test_tile_kernel
  mixed_scaled_stride_kernel, tiles      test_stride_kernel_under_grid_cap
  mixed_scaled_stride_kernel, elements   test_element_loop_outputs_differ,
                                         test_element_loop_inputs_off_grid
  unaligned input vectors                test_unaligned_input_vectors"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.guard import GUARD, Arena, _bits, arena_bytes
from tests.mixed import F_TAIL, PAIR_IDS, PAIRS, T_GROUPS, knobs
from tests.mixed_scaled import call_mixed_scaled, expected_mixed_scaled
from tests.test_gpu_mixed_bounds import _acc_modes, _es, case, on_grid
from tests.util import FP32, assert_same, rand_array

pytestmark = pytest.mark.gpu

SCALE = 1 / 3
COUNTS = (1, 7, 8, 511, 512, 513, 1024 + 5)
assert T_GROUPS * 8 == 512


def shapes(es_out):
    """(count, head): every count at every scalar head."""
    return [(n, h) for n in COUNTS for h in sorted({0, 1, 16 // es_out - 1})]


@functools.lru_cache(maxsize=None)
def scaled_guards(idt, odt, flags, k, acc_mode):
    """tests.test_gpu_mixed_bounds.mixed_guards against the scaled composition:
    per side (before, after) (input guards, acc guard or None, output guard),
    GUARD // 4 elements each, aligned by element index."""
    n = GUARD // 4
    variants = {flags & ~F_TAIL} | ({0} if flags & F_TAIL else set())  # a spilt element may round either way
    sides = []
    for side in range(2):
        def draw(dt, j, r):
            return rand_array(dt, n, seed=((side + 11) * 131 + j) * 97 + r + 1, specials=False)
        ing = [draw(idt, j, 0) for j in range(k)]
        accg = draw(FP32, k, 0) if acc_mode else None
        outg = draw(odt, k + 1, 0)
        for r in range(1, 65):
            folds = [_bits(expected_mixed_scaled(ing, idt, odt, f, SCALE, accg)) for f in variants]
            bad_out = (_bits(outg) == 0) | np.logical_or.reduce([_bits(outg) == f for f in folds])
            bad_acc = np.zeros(n, bool)
            if acc_mode == "inplace":
                bad_acc = (_bits(accg) == 0) | (_bits(accg) == folds[0])
            if not bad_out.any() and not bad_acc.any():
                break
            outg[bad_out] = draw(odt, k + 1, r)[bad_out]
            if bad_acc.any():
                accg[bad_acc] = draw(FP32, k, r)[bad_acc]
                for j in range(k):
                    ing[j][bad_acc] = draw(idt, j, r)[bad_acc]
        else:
            raise AssertionError(f"scaled_guards did not converge: {idt}->{odt} k {k} acc {acc_mode}")
        sides.append((ing, accg, outg))
    return sides


def place_case(ar, i, c, seed):
    idt, odt, flags, k, m, n, in_mis, out_mis, acc_mode, acc_mis = c
    (gb_in, gb_acc, gb_out), (ga_in, ga_acc, ga_out) = scaled_guards(idt, odt, flags, k, acc_mode)
    ins = [rand_array(idt, n, seed=1000 * seed + 37 * i + j) for j in range(k)]
    pin = [ar.place(x, in_mis[j], "in", f"c{i}.in{j}", (gb_in[j], ga_in[j])) for j, x in enumerate(ins)]
    acc = pacc = None
    if acc_mode:
        acc = rand_array(FP32, n, seed=1000 * seed + 37 * i + 29)
        pacc = ar.place(acc, out_mis[0] if acc_mode == "inplace" else acc_mis,
                        "inout" if acc_mode == "inplace" else "in", f"c{i}.acc", (gb_acc, ga_acc))
    pout = []
    for o in range(m):
        if o == 0 and acc_mode == "inplace":
            pout.append(pacc)
        else:  # starts as non-zero noise of the dtype
            noise = rand_array(odt, n, seed=7000 + 1000 * seed + 37 * i + o, specials=False)
            pout.append(ar.place(noise, out_mis[o], "out", f"c{i}.out{o}", (gb_out, ga_out)))
    return pin, pacc, pout, expected_mixed_scaled(ins, idt, odt, flags, SCALE, acc)


def run_cases(cases, what, seed=0, **kn):
    import torch
    nops = sum(c[3] + c[4] + (1 if c[8] == "separate" else 0) for c in cases)
    total = sum(c[5] * (c[3] * _es(c[0]) + c[4] * _es(c[1]) + (4 if c[8] == "separate" else 0)) for c in cases)
    ar = Arena(arena_bytes(total, nops), "device", seed=seed)
    placed = [place_case(ar, i, c, seed) for i, c in enumerate(cases)]
    ar.snapshot()
    stream = torch.cuda.current_stream().cuda_stream
    with knobs(**kn):
        for c, (pin, pacc, pout, _) in zip(cases, placed):
            call_mixed_scaled([p.ptr for p in pin], c[0], [p.ptr for p in pout], c[1], c[5], c[2], SCALE,
                              pacc.ptr if pacc is not None else None, stream)
        torch.cuda.synchronize()
    ar.check(what=what)
    for c, (pin, pacc, pout, exp) in zip(cases, placed):
        for o, p in enumerate(pout):
            assert_same(ar.read(p), exp, c[1], f"{what}: output {o} of case (idt, odt, flags, k, m, count, in_mis, "
                                               f"out_mis, acc, acc_mis) = {c}")


def _common(idt, odt, flags, k, m):
    return [case(idt, odt, flags, min(k, 15) if mode else k, m, n, h, mode)
            for mode in _acc_modes(odt) for n, h in shapes(_es(odt))]


@pytest.mark.parametrize("k,m", [(1, 1), (3, 2), (16, 3)], ids=["k1-m1", "k3-m2", "k16-m3"])
@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_tile_kernel(idt, odt, flags, k, m):
    """Default knobs, every operand on the outputs' grid: 8 input slots
    (k <= 8) and 16, the m-iteration store loop."""
    run_cases(_common(idt, odt, flags, k, m), f"mixed_scaled_kernel k={k} m={m}", seed=idt * 16 + flags + k)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_stride_kernel_under_grid_cap(idt, odt, flags, cap):
    """mi_set_max_blocks(1) / (3): one or three blocks stride over the tiles
    and end in the partial one; (2, 2) and (9, 1)."""
    cases = _common(idt, odt, flags, 2, 2) + _common(idt, odt, flags, 9, 1)
    run_cases(cases, f"mixed_scaled_stride_kernel max_blocks={cap}", seed=400 + idt + flags, max_blocks=cap)


@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_element_loop_outputs_differ(idt, odt, flags):
    """Outputs at differing misalignments have no common grid: the element
    loop, whatever mi_set_unaligned_vectors says; acc in place among them."""
    eso = _es(odt)
    cases = []
    for mode in _acc_modes(odt):
        for i, (n, h) in enumerate(shapes(eso)):
            for k, m in ((2, 2), (9, 3)):
                om = [(on_grid(h, eso) + (o + (i % 3 if o else 0)) * eso) % 16 for o in range(m)]
                if len(set(om)) == 1:
                    om[-1] = (om[0] + eso) % 16
                cases.append(case(idt, odt, flags, k, m, n, h, mode, out_mis=om))
    run_cases(cases, "element loop, outputs differ", seed=500 + idt + flags, unaligned=1)


def _inputs_off_grid(idt, odt, flags):
    """Each input at its own element offset from the outputs' grid (at least
    one of them off it), a separate acc one element off it."""
    esi, eso = _es(idt), _es(odt)
    cases = []
    for mode in _acc_modes(odt):
        for i, (n, h) in enumerate(shapes(eso)):
            for k, m in ((2, 2), (9, 3)):
                im = [(on_grid(h, esi) + (1 + j + i) * esi) % 16 for j in range(k)]
                if all(x == on_grid(h, esi) for x in im):
                    im[0] = (im[0] + esi) % 16
                cases.append(case(idt, odt, flags, k, m, n, h, mode, in_mis=im,
                                  acc_mis=(on_grid(h, 4) + 4) % 16 if mode == "separate" else None))
    return cases


@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_element_loop_inputs_off_grid(idt, odt, flags):
    """mi_set_unaligned_vectors(0) with inputs off the outputs' grid."""
    run_cases(_inputs_off_grid(idt, odt, flags), "element loop, inputs off the grid", seed=600 + idt + flags,
              unaligned=0)


@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_unaligned_input_vectors(idt, odt, flags):
    """mi_set_unaligned_vectors(1): the tile kernel on the outputs' grid with
    each input (and a separate acc) at its own element offset."""
    run_cases(_inputs_off_grid(idt, odt, flags), "unaligned input vectors", seed=700 + idt + flags, unaligned=1)
