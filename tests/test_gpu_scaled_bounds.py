"""mi_reduce_bcast_scaled writes its m outputs, all of each and nothing else.

The arena method of tests/test_gpu_bcast_bounds.py, whose placement this
reuses (place_bcast and its bcast_guards): many cases carved out of one guarded
Arena (tests/guard.py), one snapshot, every launch, one check() of the whole
arena, then every output compared bit for bit with
tests.test_gpu_scaled.expected_scaled of the inputs as placed.  The scale
rotates over 1/3, 1/8, -2.5 and 1e-30 from case to case.

Shapes are the tile edges of the 64-vector tile, tile_shapes(es, T_LEAN):
bodies of 0, 1, 63, 64, 65 and 129 16-byte vectors crossed with scalar heads
and tails of 0, 1 and 16/es - 1 elements, and one element at misalignment es:
the smallest shapes at which a tile edge can go wrong.  The grid-stride
kernel's own tile is 256 vectors, so its test adds the edges of that one.

The guards stay sound under a multiplier: they hold no zero byte pattern of
the dtype, while a lane past the end that loaded zeros would store 0 * s, a
signed zero; in place, a lane that got through would store s times the fold
of its neighbours, which equals a neighbour only by accident of the draw
(s != 1 in every case).

Who guards what (the rows tests/guard.py's table would hold for the kernels
of mi_reduce_bcast_scaled; knob = how the test routes to it):

  bcast_scaled_kernel<.., 8 / 16>      test_tile_kernel (k <= 8 / k > 8, all outputs separate; m = 1 and
                                       k = 1 among them), test_tile_kernel_in_place (outs[i] == inputs[i];
                                       outs[0] == inputs[2])
  bcast_scaled_stride_kernel, tiles    test_stride_kernel_under_grid_cap (mi_set_max_blocks(1), (3); in
                                       place and separate)
  bcast_scaled_stride_kernel, elements test_element_loop (mi_set_unaligned_vectors(0); outputs at differing
                                       misalignments, one of them an input)
  bcast_elem under a multiplier        the scalar heads and tails of every shape above

MI_F_BF16_TAIL_TRUNC16 is left to tests/test_gpu_scaled.py (the oracle has no
fold for it); its kernels differ from bf16 0x7's in the rounding of the last
count % 16 elements only.
"""
from __future__ import annotations

import pytest

from oneccl_amd import _lib
from tests.guard import T_LEAN, Arena, arena_bytes
from tests.guard import es_of as _es
from tests.test_gpu_bcast_bounds import _common, _differing, place_bcast
from tests.test_gpu_bounds import Knobs, _stream
from tests.test_gpu_scaled import SCALES, SUM, VARIANT_IDS, VARIANTS, expected_scaled
from tests.util import assert_same

pytestmark = pytest.mark.gpu

T_STRIDE = 256  # bcast_scaled_stride_kernel's tile: kBlock vectors
VAR = [(v, i) for v, i in zip(VARIANTS, VARIANT_IDS) if not v[1] & 0x8]
variants = pytest.mark.parametrize("dt,flags", [v for v, _ in VAR], ids=[i for _, i in VAR])


def run_scaled(cases, what, seed=0, **knobs):
    import torch
    nops = sum(c[3] + c[4] - len(c[8]) for c in cases)
    total = sum((c[3] + c[4] - len(c[8])) * c[5] * _es(c[0]) for c in cases)
    ar = Arena(arena_bytes(total, nops), "device", seed=seed)
    placed = [place_bcast(ar, i, c, seed) for i, c in enumerate(cases)]
    ar.snapshot()
    mi = _lib.mi()
    with Knobs(**knobs):
        for i, (c, (pin, pout, _)) in enumerate(zip(cases, placed)):
            dt, _, flags, k, m, n = c[:6]
            _lib.check(mi.mi_reduce_bcast_scaled(_lib.void_ptr_array([p.ptr for p in pin]), k,
                                                 _lib.void_ptr_array([p.ptr for p in pout]), m, n, dt, SUM, flags,
                                                 SCALES[i % len(SCALES)], _stream()), "mi_reduce_bcast_scaled")
        torch.cuda.synchronize()
    ar.check(what=what)
    for i, (c, (pin, pout, _)) in enumerate(zip(cases, placed)):
        if not c[5]:
            continue
        exp = expected_scaled([ar.original(p) for p in pin], c[0], c[2], SCALES[i % len(SCALES)])
        for o, p in enumerate(pout):
            assert_same(ar.read(p), exp, c[0], f"{what}: output {o} of case {i} (dt, op, flags, k, m, count, in_mis, "
                                               f"out_mis, alias) = {c}, scale {SCALES[i % len(SCALES)]!r}")


# ---- bcast_scaled_kernel<.., 8> / <.., 16> -------------------------------------------

@variants
def test_tile_kernel(dt, flags):
    """All outputs separate, every operand at the outputs' misalignment: 8
    input slots (k <= 8) and 16; one output, and one input, among them."""
    cases = []
    for k, m in ((1, 2), (3, 1), (8, 3), (9, 2), (16, 2)):
        cases += _common(dt, SUM, k, m, T_LEAN, None, flags)
    run_scaled(cases, "bcast_scaled_kernel", seed=dt * 16 + flags)


@variants
def test_tile_kernel_in_place(dt, flags):
    """outs[i] == inputs[i] for all i (the averaged one-shot allreduce) at
    (2, 2), (8, 8), (9, 9); at (3, 5) outs[0] == inputs[2] and the rest
    separate; (1, 1) scales a buffer in place."""
    cases = []
    for k in (1, 2, 8, 9):
        cases += _common(dt, SUM, k, k, T_LEAN, {i: i for i in range(k)}, flags)
    cases += _common(dt, SUM, 3, 5, T_LEAN, {0: 2}, flags)
    run_scaled(cases, "bcast_scaled_kernel in place", seed=100 + dt * 16 + flags)


# ---- bcast_scaled_stride_kernel ----------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
@variants
def test_stride_kernel_under_grid_cap(dt, flags, cap):
    """mi_set_max_blocks(1) / (3): one or three blocks stride over the tiles
    and end in the partial one; (2, 2) in place and (3, 4) separate over the
    64-vector edges, (9, 2) over the kernel's own 256-vector edges."""
    cases = _common(dt, SUM, 2, 2, T_LEAN, {0: 0, 1: 1}, flags) + _common(dt, SUM, 3, 4, T_LEAN, None, flags)
    cases += _common(dt, SUM, 9, 2, T_STRIDE, {1: 3}, flags)
    run_scaled(cases, f"bcast_scaled_stride_kernel max_blocks={cap}", seed=400 + dt * 16 + flags, max_blocks=cap)


def _with_flags(cases, flags):
    return [c[:2] + (flags,) + c[3:] for c in cases]


@variants
def test_element_loop(dt, flags):
    """mi_set_unaligned_vectors(0) with outputs at differing misalignments (no
    common vector grid): (2, 2) with outs[1] == inputs[0], (5, 3) with every
    operand at its own, and (1, 2)."""
    cases = _differing(dt, SUM, 2, 2, T_LEAN, False, True, {1: 0}) + _differing(dt, SUM, 5, 3, T_LEAN, True, True)
    cases += _differing(dt, SUM, 1, 2, T_LEAN, True, True)
    run_scaled(_with_flags(cases, flags), "element loop under a multiplier", seed=500 + dt * 16 + flags, unaligned=0)

