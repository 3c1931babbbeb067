"""mi_reduce_bcast_mixed writes its m outputs, all of each and nothing else.

The arena method of tests/guard.py (Arena, check()): many cases carved out of
one guarded arena, one snapshot, every launch, one check() of the whole arena,
then every output compared bit for bit with the composition the header defines
(tests.mixed.expected_mixed; no tolerance anywhere).

Shapes are the tile edges.  With T the groups of 8 elements per tile of the
kernel as built (tests.mixed.T_GROUPS = 64: a one-wave block owns 64 * 2 runs
of 4 elements, 512 in all):
bodies of 0, 1, T - 1, T, T + 1 and 2T + 1 groups, crossed with scalar heads of
0, 1 and 16 / es_out - 1 elements, crossed with scalar tails of 0, 1 and 7
elements, plus one element at misalignment es_out.

Guards are elements of each operand's own dtype, drawn so that what a spilling
lane would store differs from what lies there (mixed_guards): the output-side
guard differs from zero (a lane past the end that loaded zeros stores the sum
of zeros) and from the composition of the operands' guards at the same element
index; an accumulator that is an output (in place) is drawn as
tests.test_gpu_bcast_bounds.bcast_guards draws an aliased input's: its guard
differs from zero and from the composition of the guards (what a lane that got
through in place would store over it).

Who guards what (the rows tests/guard.py's table would hold for the kernels of
mi_reduce_bcast_mixed; knob = how the test routes to it):

  mixed_kernel<.., 8 / 16>        test_tile_kernel (k <= 8 / k > 8; widening without acc, with a
                                  separate acc and with acc == outs[0])
  mixed_stride_kernel, tiles      test_stride_kernel_under_grid_cap (mi_set_max_blocks(1), (3))
  mixed_stride_kernel, elements   test_element_loop_outputs_differ (outputs at differing
                                  misalignments), test_element_loop_inputs_off_grid
                                  (mi_set_unaligned_vectors(0)), test_element_loop_not_element_aligned
  unaligned input vectors         test_unaligned_input_vectors (mi_set_unaligned_vectors(1), each input at
                                  its own element offset, acc off the grid too)
  MI_F_BF16_TAIL_TRUNC16          test_tail_trunc_threshold (count % 16 in 1, 7, 8, 9, 15 on the three
                                  routes)

Destinations on a peer GPU have not been run: every operand here is on one
device."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.guard import GUARD, Arena, _bits, arena_bytes
from tests.mixed import F_RNE, F_TAIL, PAIR_IDS, PAIRS, T_GROUPS, call_mixed, expected_mixed, knobs
from tests.util import BF16, FP32, assert_same, rand_array

pytestmark = pytest.mark.gpu


def _es(dt):
    return 4 if dt == FP32 else 2


def shapes(es_out, T):
    """(count, head): the tile edges of the module docstring."""
    heads = sorted({0, 1, 16 // es_out - 1})
    out = [(h + 8 * b + t, h) for b in (0, 1, T - 1, T, T + 1, 2 * T + 1) for h in heads for t in (0, 1, 7)]
    return out + [(1, 16 // es_out - 1)]  # one element at misalignment es_out


def on_grid(head, es):
    """The misalignment at which an operand's element `head` is on a 16-byte boundary."""
    return (16 - head * es % 16) % 16


@functools.lru_cache(maxsize=None)
def mixed_guards(idt, odt, flags, k, acc_mode):
    """Per side (before, after): (input guards, acc guard or None, output
    guard), GUARD // 4 elements each, aligned by element index."""
    n = GUARD // 4
    variants = {flags & ~F_TAIL} | ({0} if flags & F_TAIL else set())  # a spilt element may round either way
    sides = []
    for side in range(2):
        def draw(dt, j, r):
            return rand_array(dt, n, seed=((side + 5) * 131 + j) * 97 + r + 1, specials=False)
        ing = [draw(idt, j, 0) for j in range(k)]
        accg = draw(FP32, k, 0) if acc_mode else None
        outg = draw(odt, k + 1, 0)
        for r in range(1, 65):
            folds = [_bits(expected_mixed(ing, idt, odt, f, accg)) for f in variants]
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
            raise AssertionError(f"mixed_guards did not converge: {idt}->{odt} k {k} acc {acc_mode}")
        sides.append((ing, accg, outg))
    return sides


def case(idt, odt, flags, k, m, n, head, acc_mode=None, in_mis=None, out_mis=None, acc_mis=None):
    """Operands on the outputs' grid for scalar head `head` unless a
    misalignment is given (one for all, or one per operand)."""
    def each(v, default, count):
        v = default if v is None else v
        return [v] * count if isinstance(v, int) else list(v)
    return (idt, odt, flags, k, m, n, each(in_mis, on_grid(head, _es(idt)), k), each(out_mis, on_grid(head, _es(odt)), m),
            acc_mode, on_grid(head, 4) if acc_mis is None else acc_mis)


def place_case(ar, i, c, seed):
    idt, odt, flags, k, m, n, in_mis, out_mis, acc_mode, acc_mis = c
    (gb_in, gb_acc, gb_out), (ga_in, ga_acc, ga_out) = mixed_guards(idt, odt, flags, k, acc_mode)
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
    return pin, pacc, pout, (expected_mixed(ins, idt, odt, flags, acc) if n else None)


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
            call_mixed([p.ptr for p in pin], c[0], [p.ptr for p in pout], c[1], c[5], c[2],
                       pacc.ptr if pacc is not None else None, stream)
        torch.cuda.synchronize()
    ar.check(what=what)
    for c, (pin, pacc, pout, exp) in zip(cases, placed):
        if exp is None:
            continue
        for o, p in enumerate(pout):
            assert_same(ar.read(p), exp, c[1], f"{what}: output {o} of case (idt, odt, flags, k, m, count, in_mis, "
                                               f"out_mis, acc, acc_mis) = {c}")


def _acc_modes(odt):
    return (None, "separate", "inplace") if odt == FP32 else (None,)


def _common(idt, odt, flags, k, m, T):
    return [case(idt, odt, flags, min(k, 15) if mode else k, m, n, h, mode)
            for mode in _acc_modes(odt) for n, h in shapes(_es(odt), T)]


# ---- mixed_kernel<.., 8> / <.., 16> -----------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(1, 1), (3, 2), (8, 1), (16, 3)], ids=["k1-m1", "k3-m2", "k8-m1", "k16-m3"])
@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_tile_kernel(idt, odt, flags, k, m):
    """Default knobs, every operand on the outputs' grid: 8 input slots
    (k <= 8) and 16, the m-iteration store loop; k = 1 the conversion."""
    run_cases(_common(idt, odt, flags, k, m, T_GROUPS), f"mixed_kernel k={k} m={m}", seed=idt * 16 + flags + k)


# ---- mixed_stride_kernel: tiles under a grid cap ----------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_stride_kernel_under_grid_cap(idt, odt, flags, cap):
    """mi_set_max_blocks(1) / (3): one or three blocks stride over the tiles
    and end in the partial one; (2, 2) and (9, 1)."""
    T = T_GROUPS
    cases = _common(idt, odt, flags, 2, 2, T) + _common(idt, odt, flags, 9, 1, T)
    run_cases(cases, f"mixed_stride_kernel max_blocks={cap}", seed=400 + idt + flags, max_blocks=cap)


# ---- the element loop -------------------------------------------------------------------------------

@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_element_loop_outputs_differ(idt, odt, flags):
    """Outputs at differing misalignments have no common grid: the element
    loop, whatever mi_set_unaligned_vectors says; (2, 2) and (9, 3), acc in
    place among them."""
    eso, T = _es(odt), T_GROUPS
    cases = []
    for mode in _acc_modes(odt):
        for i, (n, h) in enumerate(shapes(eso, T)):
            for k, m in ((2, 2), (9, 3)):
                om = [(on_grid(h, eso) + (o + (i % 3 if o else 0)) * eso) % 16 for o in range(m)]
                if len(set(om)) == 1:
                    om[-1] = (om[0] + eso) % 16
                cases.append(case(idt, odt, flags, k, m, n, h, mode, out_mis=om))
    run_cases(cases, "element loop, outputs differ", seed=500 + idt + flags, unaligned=1)


def _inputs_off_grid(idt, odt, flags, T):
    """Each input at its own element offset from the outputs' grid (at least
    one of them off it), acc one element off it."""
    esi, eso = _es(idt), _es(odt)
    cases = []
    for mode in _acc_modes(odt):
        for i, (n, h) in enumerate(shapes(eso, T)):
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
    run_cases(_inputs_off_grid(idt, odt, flags, T_GROUPS), "element loop, inputs off the grid", seed=600 + idt + flags,
              unaligned=0)


@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_unaligned_input_vectors(idt, odt, flags):
    """mi_set_unaligned_vectors(1): the tile kernel on the outputs' grid with
    each input (and a separate acc) at its own element offset."""
    run_cases(_inputs_off_grid(idt, odt, flags, T_GROUPS), "unaligned input vectors", seed=700 + idt + flags,
              unaligned=1)


def test_element_loop_not_element_aligned():
    """Operands at odd byte offsets are not element-aligned: the element loop
    under either setting of the knob."""
    T = T_GROUPS
    for unaligned in (0, 1):
        cases = []
        for idt, odt, flags in PAIRS:
            for n in (1, 3, 255, 8 * T + 9):
                for im, om in (([1, 1], [1, 1]), ([0, 3], [0, 0]), ([0, 0], [5, 5]), ([2, 0], [15, 3])):
                    cases.append(case(idt, odt, flags, 2, 2, n, 0, None, in_mis=im, out_mis=om))
            if odt == FP32:
                cases.append(case(idt, odt, flags, 2, 1, 8 * T + 9, 0, "separate", acc_mis=2))
        run_cases(cases, f"element loop, not element-aligned, unaligned={unaligned}", seed=800 + unaligned,
                  unaligned=unaligned)


# ---- MI_F_BF16_TAIL_TRUNC16 -------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["tile", "stride", "elements"])
def test_tail_trunc_threshold(route):
    """Head 0 and count % 16 in 1, 7 (the truncated run stays in the scalar
    tail), 8 (it is the last body group), 9, 15 (scalar tail and the last body
    group): the threshold is an element index, so the body's last group must
    truncate where the scalar path would."""
    T = T_GROUPS
    kn = {"tile": {}, "stride": {"max_blocks": 1}, "elements": {"unaligned": 0}}[route]
    cases = []
    for q in (0, 1, T // 2, T // 2 + 1):  # multiples of 16 elements below the truncated run
        for r in (1, 7, 8, 9, 15):
            n = 16 * q + r
            im = [2, 0, 0] if route == "elements" else None  # one input off the grid: the element loop
            cases.append(case(FP32, BF16, F_RNE | F_TAIL, 3, 2, n, 0, None, in_mis=im))
    for c in cases:  # the expectation does truncate a run that differs from rounding somewhere
        assert c[5] % 16 in (1, 7, 8, 9, 15)
    run_cases(cases, f"tail-trunc threshold, {route}", seed=900, **kn)
    x = [rand_array(FP32, 16 * T + 9, seed=5 + j) for j in range(3)]
    a, b = expected_mixed(x, FP32, BF16, F_RNE | F_TAIL), expected_mixed(x, FP32, BF16, F_RNE)
    assert (a[-9:] != b[-9:]).any() and (a[:-9] == b[:-9]).all()
